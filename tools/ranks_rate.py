#!/usr/bin/env python3
"""Cost of the exact neighbour ranks of a latent index beside the density self-join and the k = 1 search of the same run, on one box:
    python tools/ranks_rate.py [--small] [out.txt]
Indices of N = 16,384 and 131,072 seeded rows of 128 columns (--small: the first only).  Prints (and appends to out.txt), host clock around
synchronous calls, warm, min / median of five (three at 131,072 rows):
  (a) Engine.index_ranks over all rows with m = 31 probes, the best case: the probes are each row's true 31 nearest rows, so all but
      31 pairs of a query are dropped after one compare;
  (b) the worst case: 31 random rows as probes, where about half of all pairs pass the compare, search their bin and do an LDS atomic;
  (c) a 2-column index (map coordinates) with (b)'s kind of probes: the search is not hidden behind a 128-column chain;
  beside the yardsticks of the same rows in the same run, which are the parent's kernels: Engine.index_density with the index's own rows as
  host queries, each leaving out its own position (the same 3 N N D of distance arithmetic), and Engine.index_query with k = 1;
  (d) LatentIndex.map_quality of the PCA map end to end at 16,384 rows beside its steps: the two neighbour graphs and the two rank passes;
  (e) at 16,384 rows the host twin (_hip.ranks_host, std::thread, 16 threads at most) on case (a).
No ratio was fixed beforehand.  FLOP/s are over 3 N N D.  The kernel's registers come from the compiler
(make -C scann--material_amd/csrc resource-usage)."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
argv = sys.argv[1:]
args = [a for a in argv if not a.startswith("--")]
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


import scann_oracle as so
from scann import _hip
from scann.models import LatentIndex
from scann.models import latent_index as li
from scann.models.scann_model import HipModel

cfg = so.default_config("qm9")
model = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True)
eng = model.engine


def make(N, seed=7):
    """rows around 40 centres, as tools/peaks_rate.py makes them"""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((40, D), dtype=np.float32)
    rows = centres[rng.integers(0, 40, N)] + rng.standard_normal((N, D), dtype=np.float32)
    lat = LatentIndex(model, "atom")
    for i in range(0, N, 1 << 18):
        lat.add_rows(rows[i:i + (1 << 18)])
    return lat, rows


GAMMA = _hip.rbf_gamma(12.0)
say("ranks_tile_kernel (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): 138 VGPRs, no scratch, 50,944 bytes of LDS, "
    "3 waves per SIMD: three workgroups per CU")

for N in (16384,) if "--small" in argv else (16384, 131072):
    lat, rows = make(N)
    own = np.arange(N)
    flop = 3.0 * N * N * D
    runs = 5 if N <= 20000 else 3
    say("ranks of N = %d rows x %d columns, m = 31" % (N, D))
    eng.index_density(lat._ix, rows, GAMMA, own)  # warm
    tb = timed(lambda: eng.index_density(lat._ix, rows, GAMMA, own), runs)
    eng.index_query(lat._ix, rows[:4096], 1)
    t0 = time.perf_counter()
    for a in range(0, N, 4096):
        eng.index_query(lat._ix, rows[a:a + 4096], 1)
    tq = time.perf_counter() - t0
    say("    Engine.index_density, the rows as host queries: %9.2f / %9.2f ms (min / median of %d): %.3g FLOP/s over 3 N N D;  Engine.index_query, "
        "k = 1, the rows 4,096 at a time: %9.2f ms" % (tb[0] * 1e3, tb[1] * 1e3, runs, flop / tb[0], tq * 1e3))
    t0 = time.perf_counter()
    near, _ = li.neighbour_graph(lat)
    tg = time.perf_counter() - t0
    far = np.random.default_rng(1).integers(0, N, (N, 31)).astype(np.int32)
    for name, probe in (("(a) the 31 nearest rows", near), ("(b) 31 random rows", far)):
        r = eng.index_ranks(lat._ix, probe)["rank"]
        ta = timed(lambda: eng.index_ranks(lat._ix, probe), runs)
        say("%s: Engine.index_ranks %9.2f / %9.2f ms: %.3g FLOP/s; / density = %.3f (medians %.3f), / search = %.3f; mean rank %.1f" % (
            name, ta[0] * 1e3, ta[1] * 1e3, flop / ta[0], ta[0] / tb[0], ta[1] / tb[1], ta[0] / tq, float(r[r >= 0].mean())))
    low = li._CoordIndex(model, np.ascontiguousarray(rows[:, :2]))  # (an index of another width on the same handle, as map_quality makes one)
    eng.index_density(low._ix, rows[:, :2], GAMMA, own)
    tb2 = timed(lambda: eng.index_density(low._ix, rows[:, :2], GAMMA, own), runs)
    eng.index_ranks(low._ix, far)
    tc = timed(lambda: eng.index_ranks(low._ix, far), runs)
    eng.index_ranks(low._ix, li.neighbour_graph(low)[0])
    near2 = li.neighbour_graph(low)[0]
    tc2 = timed(lambda: eng.index_ranks(low._ix, near2), runs)
    say("(c) a 2-column index, 31 random rows: Engine.index_ranks %9.2f / %9.2f ms; its 31 nearest rows %9.2f / %9.2f ms; Engine.index_density on "
        "it %9.2f / %9.2f ms: (c) / density = %.3f" % (tc[0] * 1e3, tc[1] * 1e3, tc2[0] * 1e3, tc2[1] * 1e3, tb2[0] * 1e3, tb2[1] * 1e3, tc[0] / tb2[0]))
    low.free()
    if N <= 20000:
        res, _ = lat.pca(2)
        out = []
        lat.map_quality(res)
        tm = timed(lambda: out.append(lat.map_quality(res)), 3)
        q = out[-1]
        say("(d) LatentIndex.map_quality of pca(2) end to end: %9.1f / %9.1f ms (min / median of 3); the latent neighbour graph alone %9.1f ms; "
            "trustworthiness %.4f continuity %.4f overlap %.4f R_NX area %.4f" % (tm[0] * 1e3, tm[1] * 1e3, tg * 1e3, q["trustworthiness"],
                                                                                q["continuity"], q["neighbour_overlap"], q["rnx_auc"]))
        th = []
        for _ in range(2):
            t0 = time.perf_counter()
            host = _hip.ranks_host(rows, near, dist2=True)
            th.append(time.perf_counter() - t0)
        dev = eng.index_ranks(lat._ix, near, dist2=True)
        td = timed(lambda: eng.index_ranks(lat._ix, near, dist2=True))
        same = all(host[k].tobytes() == dev[k].tobytes() for k in host)
        say("(e) the host twin (_hip.ranks_host) on (a), %d threads: %9.1f and %9.1f ms: %.0f x the device call (%9.2f ms); both routes agree in %s" % (
            min(16, len(os.sched_getaffinity(0))), th[0] * 1e3, th[1] * 1e3, min(th) / td[0], td[0] * 1e3, "every bit" if same else "NOT every bit"))
    lat.free()
