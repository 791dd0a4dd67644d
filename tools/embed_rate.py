#!/usr/bin/env python3
"""Cost of the neighbour embedding of a latent index on the device against its host twin, on one box:
    python tools/embed_rate.py [--small] [--kernels N | --summary TRACE.csv N] [out.txt]
Indices of N = 16,384 and 131,072 seeded rows of 128 columns (--small: the first only).  Prints (and appends to out.txt), host clock around
synchronous calls, warm, min / median of three:
  (a) one iteration of Engine.embed_iterate: the difference of a call of 22 and a call of 2 iterations over 20 (upload, download and the
      wait cancel), and the N (N - 1) pairs per second that is if all of it were the repulsion kernel;
  (b) LatentIndex.embed end to end with the default schedule (250 + 500 iterations), split into the initial layout (pca), the neighbour
      graph, the affinities (host) and the iterations;
  (c) three iterations of the host twin (_hip.embed_iterate_host, up to 16 threads) on the same state, and the ratio to (a).
--kernels N: a call of 12 iterations at that size and no timing, for a run of its own under `rocprofv3 --kernel-trace --output-format csv
-d DIR -- python tools/embed_rate.py --kernels N`.  --summary TRACE.csv N [out.txt] (no GPU) reads that run's *_kernel_trace.csv and prints
per kernel the time of one launch, min / median over the launches behind the first two iterations, with embed_repulse_kernel's pairs per
second."""
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


def timed(f, runs=3):
    t = []
    for r in range(runs):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return min(t), float(np.median(t))


def summary(path, N):
    import csv, re
    runs = {}
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        k = re.search(r"embed_\w+_kernel", r["Kernel_Name"])
        if k:
            runs.setdefault(k.group(0), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    say("kernels of Engine.embed_iterate, N = %d (rocprofv3 --kernel-trace; us per launch, min / median of the launches behind the first two "
        "iterations):" % N)
    total = 0.0
    for k in sorted(runs):
        t = sorted(runs[k][2:])
        total += t[0]
        note = "   %.3g pairs: %.3g pairs/s" % (N * (N - 1.0), N * (N - 1.0) / (t[0] * 1e-6)) if k == "embed_repulse_kernel" else ""
        say("  %-24s %4d x %10.1f / %10.1f%s" % (k, len(t), t[0], float(np.median(t)), note))
    say("  %-24s        %10.1f   (one iteration: the kernels' minima together)" % ("all of them", total))


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


def make(N):
    """rows around 40 centres, so that the map has something to find"""
    rng = np.random.default_rng(7)
    centres = 4.0 * rng.standard_normal((40, D), dtype=np.float32)
    rows = centres[rng.integers(0, 40, N)] + rng.standard_normal((N, D), dtype=np.float32)
    lat = LatentIndex(model, "atom")
    for i in range(0, N, 1 << 16):
        lat.add_rows(rows[i:i + (1 << 16)])
    return lat


def state_of(lat, perplexity=10):
    t0 = time.perf_counter()
    pca, _ = lat.pca(2)
    y0 = li.embed_initial_layout(pca["coordinates"])
    t1 = time.perf_counter()
    pos, d2 = li.neighbour_graph(lat)
    t2 = time.perf_counter()
    graph = li.embed_affinities(d2, pos, perplexity)
    t3 = time.perf_counter()
    return graph, y0, (t1 - t0, t2 - t1, t3 - t2)


if "--kernels" in opt:
    N = int(opt["--kernels"][0])
    lat = make(N)
    graph, y0, _ = state_of(lat)
    eng.embed_iterate(*graph, y0, np.zeros_like(y0), np.ones_like(y0), 12, 12.0, 0.5, max(200.0, N / 12.0))
    lat.free()
    sys.exit(0)

for N in (16384,) if "--small" in argv else (16384, 131072):
    lat = make(N)
    lr = max(200.0, N / 12.0)
    graph, y0, (t_pca, t_graph, t_aff) = state_of(lat)
    u0, g0 = np.zeros_like(y0), np.ones_like(y0)
    mid = eng.embed_iterate(*graph, y0, u0, g0, 50, 12.0, 0.5, lr)  # warm, and a layout in mid-flight
    st = (mid["y"], mid["u"], mid["gain"])
    t2 = timed(lambda: eng.embed_iterate(*graph, *st, 2, 12.0, 0.5, lr))
    t22 = timed(lambda: eng.embed_iterate(*graph, *st, 22, 12.0, 0.5, lr))
    per = (t22[0] - t2[0]) / 20.0
    say("neighbour embedding of N = %d rows x %d columns, %d edges" % (N, D, len(graph[1])))
    say("(a) Engine.embed_iterate: 2 iterations %9.2f / %9.2f ms, 22 iterations %9.2f / %9.2f ms (min / median of 3): %8.3f ms per iteration; "
        "%.3g pairs are %.3g pairs/s if all of it were the repulsion kernel" % (t2[0] * 1e3, t2[1] * 1e3, t22[0] * 1e3, t22[1] * 1e3, per * 1e3,
                                                                              N * (N - 1.0), N * (N - 1.0) / per))
    t0 = time.perf_counter()
    res, emb = lat.embed()
    t_all = time.perf_counter() - t0
    say("(b) LatentIndex.embed end to end, 250 + 500 iterations: %9.1f ms; its steps timed alone before it: the initial layout (pca) %8.1f ms, the neighbour "
        "graph %8.1f ms, the affinities (host) %8.1f ms; that leaves %9.1f ms for 752 iterations in four calls and two KL sums; kl %.4f -> %.4f" % (
            t_all * 1e3, t_pca * 1e3, t_graph * 1e3, t_aff * 1e3, (t_all - t_pca - t_graph - t_aff) * 1e3, res["kl_init"], res["kl"]))
    th = timed(lambda: _hip.embed_iterate_host(*graph, *st, 3, 12.0, 0.5, lr), runs=1 if N > 50000 else 3)
    same = _hip.embed_iterate_host(*graph, *st, 2, 12.0, 0.5, lr)["y"].view(np.uint32) == eng.embed_iterate(*graph, *st, 2, 12.0, 0.5, lr)["y"].view(np.uint32)
    say("(c) three iterations of the host twin, OMP_NUM_THREADS %s: %9.1f ms, %8.2f ms per iteration: %.0f x the device's; two iterations of both "
        "agree in %s" % (os.environ.get("OMP_NUM_THREADS", "unset"), th[0] * 1e3, th[0] / 3 * 1e3, th[0] / 3 / per, "every bit" if same.all() else "NOT every bit"))
    lat.free()
