#!/usr/bin/env python3
"""Cost of the exact minimum spanning tree of a latent index (scann_index_mst) beside the passes it is made of, on one box:
    python tools/mst_rate.py [--small] [out.txt]
Indices of N = 16,384 and 131,072 seeded rows of 128 columns around 40 centres (--small: the first only), min_samples 5, one process, host
clock around synchronous calls, warm.  Prints (and appends to out.txt):
  (a) per Boruvka round of one Engine.index_mst: the components before it, the host time around it (search, merge, component step and
      the 12-byte read-back) and the share of tiles whose arithmetic the label rule skipped (scann_mst_last_rounds);
  (b) Engine.index_mst end to end, min / median of three, beside Engine.index_peaks (two passes) and Engine.index_query with k = 1 and
      the rows themselves as host queries (one pass) of the same run;
  (c) the yardstick for round 1, which skips nothing and is the parent pass's arithmetic: the parent pass of Engine.index_peaks as
      tools/peaks_rate.py derives it -- index_peaks less the density pass, the density pass being Engine.index_density of the rows
      themselves less the same call against 64 rows -- derived twice, each from minima of three; round 1 as a ratio to it beside the
      spread between the two derivations;
  (d) LatentIndex.hierarchy end to end with its parts: the neighbour graph (core distances), the tree, the host assembly
      (LatentHierarchy and clusters(20));
  (e) at 16,384 rows the host twin (_hip.mst_host: std::thread, as many threads as the process may use, 16 at most) and whether both
      routes agree in every bit."""
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


def timed(f, runs=3):
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
    """rows around 40 centres (tools/peaks_rate.py's)"""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((40, D), dtype=np.float32)
    rows = centres[rng.integers(0, 40, N)] + rng.standard_normal((N, D), dtype=np.float32)
    lat = LatentIndex(model, "atom")
    for i in range(0, N, 1 << 18):
        lat.add_rows(rows[i:i + (1 << 18)])
    return lat, rows


GAMMA = _hip.rbf_gamma(12.0)

for N in (16384,) if "--small" in argv else (16384, 131072):
    lat, rows = make(N)
    own = np.arange(N)
    flop = 3.0 * N * N * D
    t_graph = timed(lambda: li.neighbour_graph(lat, strict=False))
    core2 = li.hierarchy_core2(rows, 5, lambda x: li.neighbour_graph(lat, strict=False))
    eng.index_mst(lat._ix, core2), eng.index_peaks(lat._ix, GAMMA), eng.index_density(lat._ix, rows, GAMMA, own), eng.index_query(lat._ix, rows, 1)  # warm
    say("minimum spanning tree of N = %d rows x %d columns, min_samples 5" % (N, D))
    tree = eng.index_mst(lat._ix, core2)
    log = _hip.mst_last_rounds()
    say("(a) one Engine.index_mst, %d rounds, %d tiles a round:" % (tree["rounds"], log["tiles"]))
    for r in range(len(log["components"])):
        say("    round %2d: %7d components before it, %9.2f ms, %5.1f %% of the tiles skipped" % (
            r + 1, log["components"][r], log["seconds"][r] * 1e3, 100.0 * log["skipped"][r] / max(log["tiles"], 1)))
    first = log["seconds"][0]
    tm = timed(lambda: eng.index_mst(lat._ix, core2))
    firsts = [first]
    for _ in range(2):
        eng.index_mst(lat._ix, core2)
        firsts.append(_hip.mst_last_rounds()["seconds"][0])
    first = min(firsts)
    tq = timed(lambda: eng.index_query(lat._ix, rows, 1))
    tiny = LatentIndex(model, "atom").add_rows(rows[:64])
    eng.index_density(tiny._ix, rows, GAMMA)
    parents = []
    for rep in range(2):
        tc = timed(lambda: eng.index_peaks(lat._ix, GAMMA))
        ta = timed(lambda: eng.index_density(lat._ix, rows, GAMMA, own))
        t0_ = timed(lambda: eng.index_density(tiny._ix, rows, GAMMA))
        parents.append(tc[0] - (ta[0] - t0_[0]))
    tiny.free()
    say("(b) Engine.index_mst end to end: %9.2f / %9.2f ms (min / median of 3): %.2f passes' worth at the rate of round 1; Engine.index_peaks "
        "%9.2f ms; Engine.index_query, k = 1, the rows as host queries %9.2f / %9.2f ms" % (
            tm[0] * 1e3, tm[1] * 1e3, tm[0] / first, tc[0] * 1e3, tq[0] * 1e3, tq[1] * 1e3))
    spread = abs(parents[0] - parents[1]) / min(parents)
    say("(c) the parent pass of Engine.index_peaks, derived twice: %9.2f and %9.2f ms (spread %.3f); round 1 of the tree (min of 3) %9.2f ms = "
        "%.3g FLOP/s over 3 N N D: %.3f x the parent pass" % (parents[0] * 1e3, parents[1] * 1e3, spread, first * 1e3, flop / first, first / min(parents)))
    out = []
    t_all = timed(lambda: out.append(lat.hierarchy(min_samples=5)))
    res, h = out[-1]
    t0 = time.perf_counter()
    h2 = li.LatentHierarchy(res["a"], res["b"], res["w"], res["core2"], N, h.ids, h.atoms, 5, "atom", D)
    c = h2.clusters(20)
    t_host = time.perf_counter() - t0
    say("(d) LatentIndex.hierarchy(min_samples=5) end to end: %9.1f / %9.1f ms (min / median of 3); the neighbour graph alone %9.1f / %9.1f ms; the "
        "tree alone %9.1f ms; the host assembly (LatentHierarchy + clusters(20)) %9.1f ms: %d clusters, %d rows noise" % (
            t_all[0] * 1e3, t_all[1] * 1e3, t_graph[0] * 1e3, t_graph[1] * 1e3, tm[0] * 1e3, t_host * 1e3, len(c["size"]), int((c["label"] < 0).sum())))
    if N <= 20000:
        th = []
        for _ in range(2):
            t0 = time.perf_counter()
            twin = _hip.mst_host(rows, core2)
            th.append(time.perf_counter() - t0)
        same = all(np.array_equal(twin[k].view(np.uint8), tree[k].view(np.uint8)) for k in "abw")
        say("(e) the host twin (_hip.mst_host), %d threads: %9.1f and %9.1f ms: %.0f x (b); both routes agree in %s" % (
            min(16, len(os.sched_getaffinity(0))), th[0] * 1e3, th[1] * 1e3, min(th) / tm[0], "every bit" if same else "NOT every bit"))
    lat.free()
