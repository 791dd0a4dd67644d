#!/usr/bin/env python3
"""Cost of the radius search over a latent-space index (scann_index_within) beside the k = 1 nearest-row search of the same rows in the
same run, on one box:
    python tools/within_rate.py [--small] [out.txt]
Two row sets of 128 columns: rows around 40 centres in shuffled order (tools/cells_rate.py's set) and unstructured Gaussian rows;
N = 131,072 and 2,400,000 (--small: the first only).  One process, host clock around synchronous calls, warm, min / median of three,
the routes alternating.  Radii come from the rows themselves: a quarter of the least nearest-row distance of the queries (no hit), and
the thresholds at which count-only calls, bisected, find about 1 and about 30 rows per query.  Prints (and appends to out.txt):
  (a) Engine.index_within of 2,304 host queries -- 128 QM9-shaped molecules of 18 atoms: rows of the set, perturbed -- without and with
      a partition, beside Engine.index_query at k = 1 on the unpartitioned index (the yardstick: knn_tile_kernel) and on the partitioned one;
      the visited share of (128-query group, 64-row tile) pairs and whether both answers agree in every byte;
  (b) at 131,072 rows the upper = 1 self-join (Engine.index_within_rows over all rows) without and with a partition, beside
      Engine.index_mst of the same rows divided by its Boruvka rounds -- one all-pairs pass of that kernel;
  (c) LatentIndex.duplicates end to end beside LatentIndex.hierarchy(min_samples=1) + cut(height=radius) at 131,072 rows;
  (d) the host twin (_hip.within_host) on 16,384 rows, 2,304 queries."""
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


def timed(fns, runs=3):
    """the calls alternating: (min, median) in ms of each"""
    ts = [[] for _ in fns]
    for r in range(runs):
        for fn, t in zip(fns, ts):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
    return [(min(t) * 1e3, float(np.median(t)) * 1e3) for t in ts]


import scann_oracle as so
from scann import _hip
from scann.models import LatentIndex
from scann.models import latent_index as li
from scann.models.scann_model import HipModel

cfg = so.default_config("qm9")
model = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True)
eng = model.engine


def make_rows(kind, N, seed=7):
    rng = np.random.default_rng(seed)
    if kind == "40 centres":
        centres = 4.0 * rng.standard_normal((40, D), dtype=np.float32)
        return centres[rng.integers(0, 40, N)] + rng.standard_normal((N, D), dtype=np.float32)
    return rng.standard_normal((N, D), dtype=np.float32)


def index_of(rows):
    lat = LatentIndex(model, "atom")
    for i in range(0, len(rows), 1 << 18):
        lat.add_rows(rows[i:i + (1 << 18)])
    return lat


def same(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in a if isinstance(a[k], np.ndarray))


def radii_from(ix, q, per_query):
    """dist2 thresholds with about ``per_query`` rows per query below them: a quarter of the least nearest-row dist2 for 0, else the
    bisection (in the logarithm) of count-only calls between the least and the greatest 32nd-nearest dist2"""
    d32 = eng.index_query(ix, q, 32)["dist2"]
    out = []
    for m in per_query:
        if m == 0:
            out.append(float(d32.min()) * 0.25)
            continue
        lo, hi = float(d32.min()), float(d32[:, -1].max())
        for _ in range(30):
            mid = float(np.sqrt(lo * hi))
            if eng.index_within(ix, q, mid, count_only=True)["total"] < m * len(q):
                lo = mid
            else:
                hi = mid
        out.append(hi)
    return out


sizes = (131072,) if "--small" in argv else (131072, 2400000)
for kind in ("40 centres", "gaussian"):
    for N in sizes:
        rows = make_rows(kind, N)
        rng = np.random.default_rng(1)
        q = rows[rng.integers(0, N, 2304)] + np.float32(0.3) * rng.standard_normal((2304, D), dtype=np.float32)
        plain, cut = index_of(rows), index_of(rows)
        info = cut.partition(li.auto_cells(N))
        say("%s, N = %d rows x %d columns; partition: %d cells, %d tiles" % (kind, N, D, info["cells"], info["tiles"]))
        radii = radii_from(plain._ix, q, (0, 1, 30))
        say("(a) Engine.index_within, 2,304 host queries, beside Engine.index_query at k = 1 (min / median ms):")
        for r2 in radii:
            a, b = eng.index_within(plain._ix, q, r2), eng.index_within(cut._ix, q, r2)
            st = cut.search_stats()
            eng.index_query(plain._ix, q, 1), eng.index_query(cut._ix, q, 1)
            t = timed([lambda: eng.index_query(plain._ix, q, 1), lambda: eng.index_within(plain._ix, q, r2),
                       lambda: eng.index_query(cut._ix, q, 1), lambda: eng.index_within(cut._ix, q, r2),
                       lambda: eng.index_within(plain._ix, q, r2, count_only=True)])
            say("    radius2 %10.4f, %7.2f hits per query: k = 1 full %8.2f / %8.2f; within full %8.2f / %8.2f (%.3f x the k = 1 search), "
                "count only %8.2f / %8.2f; k = 1 partitioned %8.2f / %8.2f; within partitioned %8.2f / %8.2f, kept %5.1f %% of %d pairs; "
                "answers %s" % (r2, a["total"] / 2304.0, t[0][0], t[0][1], t[1][0], t[1][1], t[1][0] / t[0][0], t[4][0], t[4][1], t[2][0], t[2][1],
                                t[3][0], t[3][1], 100.0 * st["visited_share"], st["total"], "equal in every byte" if same(a, b) else "DIFFER"))
        if N == 131072:
            say("(b) the upper = 1 self-join of all rows, beside one all-pairs pass of scann_index_mst (the call / its rounds):")
            own = eng.index_query_rows(plain._ix, 0, 4096, 2)["dist2"][:, 1:]  # the nearest other row of 4,096 rows
            for r2 in (float(own.min()) * 0.25, float(np.sort(own.ravel())[len(own) // 64])):
                a = eng.index_within_rows(plain._ix, 0, N, r2, upper=1)
                b = eng.index_within_rows(cut._ix, 0, N, r2, upper=1)
                st = cut.search_stats()
                t = timed([lambda: eng.index_within_rows(plain._ix, 0, N, r2, upper=1), lambda: eng.index_within_rows(cut._ix, 0, N, r2, upper=1)])
                say("    radius2 %10.4f, %d pairs: full %9.1f / %9.1f ms, partitioned %9.1f / %9.1f ms, kept %5.1f %% of %d pairs, answers %s" % (
                    r2, a["total"], t[0][0], t[0][1], t[1][0], t[1][1], 100.0 * st["visited_share"], st["total"],
                    "equal in every byte" if same(a, b) else "DIFFER"))
            rounds = eng.index_mst(plain._ix)["rounds"]
            t = timed([lambda: eng.index_mst(plain._ix)], runs=2)
            say("    scann_index_mst: %9.1f / %9.1f ms in %d rounds: %9.1f ms a round" % (t[0][0], t[0][1], rounds, t[0][0] / rounds))
            say("(c) duplicates end to end beside hierarchy(min_samples=1) + cut(height=radius):")
            radius = float(np.sqrt(np.sort(own.ravel())[len(own) // 64]))
            da, db = plain.duplicates(radius), cut.duplicates(radius)
            labels = plain.hierarchy(min_samples=1)[1].cut(height=radius)
            t = timed([lambda: plain.duplicates(radius), lambda: cut.duplicates(radius), lambda: plain.hierarchy(min_samples=1)[1].cut(height=radius)], runs=2)
            say("    radius %.4f: duplicates %9.1f / %9.1f ms, with a partition %9.1f / %9.1f ms, hierarchy + cut %9.1f / %9.1f ms; %d groups, "
                "routes %s; the cut has %d clusters" % (radius, t[0][0], t[0][1], t[1][0], t[1][1], t[2][0], t[2][1], da["n_groups"],
                                                         "equal in every byte" if same(da, db) else "DIFFER", len(np.unique(labels))))
        plain.free()
        cut.free()
rows = make_rows("40 centres", 16384)
q = rows[np.random.default_rng(1).integers(0, 16384, 2304)] + np.float32(0.3)
t = timed([lambda: _hip.within_host(rows, q, 100.0)], runs=2)
say("(d) the host twin, 16,384 rows x 2,304 queries: %9.1f / %9.1f ms" % t[0])
