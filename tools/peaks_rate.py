#!/usr/bin/env python3
"""Cost of the density-peak clustering and the kernel density of a latent index beside the k-NN self-join of the same run, on one box:
    python tools/peaks_rate.py [--small] [--no-batch] [--kernels N | --summary TRACE.csv N] [out.txt]
Indices of N = 16,384 and 131,072 seeded rows of 128 columns (--small: the first only).  Prints (and appends to out.txt), host clock around
synchronous calls, warm, min / median of five:
  (a) the density pass: Engine.index_density with the index's own rows as host queries, each leaving out its own position;
  (b) the yardstick: Engine.index_query with k = 1 on the same rows as host queries -- the same 3 N Q D of distance arithmetic and the
      same upload of the queries -- and the ratio (a) / (b);
  (c) Engine.index_peaks (both passes, device to device), and the parent pass as what (c) leaves once the density pass is taken off:
      (c) - ((a) - (a0)), (a0) being call (a) against an index of 64 rows -- the upload of the queries and the call's fixed costs;
      the kernels' own times come from --kernels / --summary;
  (d) LatentIndex.density_peaks end to end beside its bandwidth step (neighbour_graph) timed alone, min / median of three each;
  (e) two timings of the host twins (_hip.peaks_host: std::thread, as many threads as the process may use, 16 at most) at 16,384 rows:
      the host route;
  (f) Engine.density_batch on 128 QM9-shaped molecules (bench.py's shape) against an index of 2,400,000 atom rows beside forward +
      download alone and Engine.index_query_batch with k = 1 on the same index and batch (--no-batch: left out).
FLOP/s are over 3 N Q D.  --kernels N: one call each of (c), (a) and (b) at that size and no timing, for a run of its own under
`rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/peaks_rate.py --kernels N`.  --summary TRACE.csv N [out.txt] (no GPU)
reads that run's *_kernel_trace.csv and prints per kernel the time summed over a call's launches."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
argv = sys.argv[1:]
TAKES = {"--kernels": 1, "--summary": 2}
opt, args, i = {}, [], 0
while i < len(argv):
    if argv[i] in TAKES:
        opt[argv[i]] = argv[i + 1:i + 1 + TAKES[argv[i]]]
        i += 1 + TAKES[argv[i]]
    else:
        if not argv[i].startswith("--"):
            args.append(argv[i])
        i += 1
out_path = args[0] if args else None
D = 128


def say(line):
    print(line, flush=True)
    if out_path:
        open(out_path, "a").write(line + "\n")


def timed(f, runs=5):
    t = []
    for r in range(runs):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return min(t), float(np.median(t))


def summary(path, N):
    import csv, re
    runs = {}
    for r in csv.DictReader(open(path)):
        k = re.search(r"(peaks_tile_kernel(<false>|<true>|ILb0E|ILb1E)|peaks_\w+_kernel|knn_\w+_kernel)", r["Kernel_Name"])
        if k:
            name = k.group(0)
            if name.startswith("peaks_tile_kernel"):
                name = "peaks_tile_kernel<density>" if k.group(2) in ("<false>", "ILb0E") else "peaks_tile_kernel<parent>"
            runs.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    flop = 3.0 * N * N * D
    say("kernels of one Engine.index_peaks, one Engine.index_density and one Engine.index_query (k = 1) of the %d rows themselves, N = %d x %d "
        "(rocprofv3 --kernel-trace; launches, us summed over them, us of the longest):" % (N, N, D))
    for k in sorted(runs):
        t = runs[k]
        say("  %-28s %5d x %12.1f %12.1f" % (k, len(t), sum(t), max(t)))
    if "peaks_tile_kernel<density>" in runs and "knn_tile_kernel" in runs:
        d, p, q = runs["peaks_tile_kernel<density>"], runs.get("peaks_tile_kernel<parent>", [0.0]), sum(runs["knn_tile_kernel"])
        one = sum(d) / len(d)
        say("  one density pass %.1f us = %.3g FLOP/s over 3 N N D; the parent pass %.1f us = %.3g FLOP/s; knn_tile_kernel over all its query groups "
            "%.1f us = %.3g FLOP/s; density / k-NN %.3f, parent / k-NN %.3f" % (one, flop / (one * 1e-6), sum(p) / len(p), flop / (sum(p) / len(p) * 1e-6),
                                                                                   q, flop / (q * 1e-6), one / q, sum(p) / len(p) / q))


if "--summary" in opt:
    summary(opt["--summary"][0], int(opt["--summary"][1]))
    sys.exit(0)

import scann_oracle as so
from scann import _hip
from scann.models import LatentIndex
from scann.models import latent_index as li
from scann.models.scann_model import HipModel

cfg = so.default_config("qm9")
model = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True)
eng = model.engine


def make(N, seed=7):
    """rows around 40 centres, so that there are peaks to find"""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((40, D), dtype=np.float32)
    rows = centres[rng.integers(0, 40, N)] + rng.standard_normal((N, D), dtype=np.float32)
    lat = LatentIndex(model, "atom")
    for i in range(0, N, 1 << 18):
        lat.add_rows(rows[i:i + (1 << 18)])
    return lat, rows


GAMMA = _hip.rbf_gamma(12.0)  # h^2 = 144: of the order of the squared distance between neighbours in make()'s rows (unit noise in 128 columns)

if "--kernels" in opt:
    N = int(opt["--kernels"][0])
    lat, rows = make(N)
    eng.index_peaks(lat._ix, GAMMA)
    eng.index_density(lat._ix, rows, GAMMA, np.arange(N))
    eng.index_query(lat._ix, rows, 1)
    lat.free()
    sys.exit(0)

for N in (16384,) if "--small" in argv else (16384, 131072):
    lat, rows = make(N)
    own = np.arange(N)
    flop = 3.0 * N * N * D
    eng.index_peaks(lat._ix, GAMMA), eng.index_density(lat._ix, rows, GAMMA, own), eng.index_query(lat._ix, rows, 1)  # warm
    ta = timed(lambda: eng.index_density(lat._ix, rows, GAMMA, own))
    tb = timed(lambda: eng.index_query(lat._ix, rows, 1))
    tc = timed(lambda: eng.index_peaks(lat._ix, GAMMA))
    tiny = LatentIndex(model, "atom").add_rows(rows[:64])
    eng.index_density(tiny._ix, rows, GAMMA)
    t0_ = timed(lambda: eng.index_density(tiny._ix, rows, GAMMA))
    tiny.free()
    t_parent = tc[0] - (ta[0] - t0_[0])
    say("density peaks of N = %d rows x %d columns, gamma %.6g" % (N, D, GAMMA))
    say("(a) Engine.index_density, the rows as host queries: %9.2f / %9.2f ms (min / median of 5): %.3g FLOP/s over 3 N N D" % (
        ta[0] * 1e3, ta[1] * 1e3, flop / ta[0]))
    say("(b) Engine.index_query, k = 1, the same queries:    %9.2f / %9.2f ms: %.3g FLOP/s; (a) / (b) = %.3f (medians %.3f)" % (
        tb[0] * 1e3, tb[1] * 1e3, flop / tb[0], ta[0] / tb[0], ta[1] / tb[1]))
    say("(c) Engine.index_peaks, both passes on the device:  %9.2f / %9.2f ms: %.3g FLOP/s over 6 N N D; (c) / (b) = %.3f" % (
        tc[0] * 1e3, tc[1] * 1e3, 2 * flop / tc[0], tc[0] / tb[0]))
    say("    (a0) call (a) against 64 rows: %9.2f / %9.2f ms; the density pass (a) - (a0) = %9.2f ms; the parent pass (c) - ((a) - (a0)) = %9.2f ms: "
        "%.3g FLOP/s, %.3f x the density pass, %.3f x (b) - (a0)" % (t0_[0] * 1e3, t0_[1] * 1e3, (ta[0] - t0_[0]) * 1e3, t_parent * 1e3, flop / t_parent,
                                                                   t_parent / (ta[0] - t0_[0]), t_parent / (tb[0] - t0_[0])))
    t_graph = timed(lambda: li.neighbour_graph(lat), runs=3)
    out = []
    t_all = timed(lambda: out.append(lat.density_peaks(k=40)[0]), runs=3)
    res = out[-1]
    say("(d) LatentIndex.density_peaks(k=40) end to end: %9.1f / %9.1f ms (min / median of 3); its bandwidth step (neighbour_graph) timed alone: "
        "%9.1f / %9.1f ms; h = %.4g, sizes %d .. %d, decision[38:42] %s" % (t_all[0] * 1e3, t_all[1] * 1e3, t_graph[0] * 1e3, t_graph[1] * 1e3,
                                                                         res["bandwidth"], res["size"].min(), res["size"].max(),
                                                                         " ".join("%.4g" % g for g in res["decision"][38:42])))
    if N <= 20000:
        th = []
        for _ in range(2):
            t0 = time.perf_counter()
            _hip.peaks_host(rows, GAMMA)
            th.append(time.perf_counter() - t0)
        same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(_hip.peaks_host(rows, GAMMA).values(), eng.index_peaks(lat._ix, GAMMA).values()))
        say("(e) the host twins (_hip.peaks_host), %d threads: %9.1f and %9.1f ms: %.0f x (c); both routes agree in %s" % (
            min(16, len(os.sched_getaffinity(0))), th[0] * 1e3, th[1] * 1e3, min(th) / tc[0], "every bit" if same else "NOT every bit"))
    lat.free()

if "--no-batch" not in argv and "--small" not in argv:
    inputs = so.pad_batch(*so.synth_dataset(128, 5), g_update=True)[0]
    pk = _hip.pack_inputs(inputs)
    rb = eng.upload(pk)
    q = model.predict(pk, outputs=["after_Lc"])[0]
    N = 2400000
    rng = np.random.default_rng(7)
    rows = (rng.standard_normal((N, D), dtype=np.float32) * q.std(0) + q.mean(0)).astype(np.float32)
    ix = eng.index_create(D)
    for i in range(0, N, 1 << 18):
        eng.index_add(ix, rows[i:i + (1 << 18)])
    lvl = _hip.OUT_AFTER_LC
    gamma = _hip.rbf_gamma(float(np.sqrt(2.0 * (q.std(0) ** 2).sum())))  # h^2: the mean squared distance between two such rows

    def forward():
        eng.forward_resident(rb)
        eng.download(rb)

    forward(), eng.density_batch(ix, rb, lvl, gamma), eng.index_query_batch(ix, rb, lvl, 1)  # warm
    tf, td, tq = timed(forward), timed(lambda: eng.density_batch(ix, rb, lvl, gamma)), timed(lambda: eng.index_query_batch(ix, rb, lvl, 1))
    flop = 3.0 * N * len(q) * D
    say("(f) 128 QM9-shaped molecules (%d atoms) against %d atom rows x %d: forward + download %8.2f / %8.2f ms; Engine.density_batch %8.2f / %8.2f ms "
        "(%.3g FLOP/s over 3 N Q D behind the forward); Engine.index_query_batch, k = 1: %8.2f / %8.2f ms (%.3g FLOP/s); density / k-NN behind the "
        "forward %.3f" % (len(q), N, D, tf[0] * 1e3, tf[1] * 1e3, td[0] * 1e3, td[1] * 1e3, flop / (td[0] - tf[0]), tq[0] * 1e3, tq[1] * 1e3,
                          flop / (tq[0] - tf[0]), (td[0] - tf[0]) / (tq[0] - tf[0])))
    ix.free()
    rb.free()
