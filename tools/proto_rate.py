#!/usr/bin/env python3
"""Cost of the prototype selection (MMD-critic) on the device beside the greedy k-center selection, on one box:
    python tools/proto_rate.py [--small] [out.txt]
A pool of N = 131,072 rows of 128 columns around 40 centres in shuffled order (tools/cells_rate.py's set; --small: N = 16,384), m = 64
and m = 256.  Prints (and appends to out.txt), host clock around synchronous calls, warm, medians of alternating runs:
  (a) scann_index_prototypes and (b) scann_index_select with the same m: the comparator is the k-center pick, which streams the same
      bytes per pick -- the call, the marginal pick (m = 256 against m = 64) and what is left of the call without its picks, which for (a)
      is the self-join that gives A (with the upload of nothing: the rows are resident);
  (c) scann_index_criticisms, 64 picks;
  (d) LatentIndex.prototypes(m = 64, criticisms = 16) end to end, and how much of it is the automatic bandwidth's neighbour graph;
  (e) the host twin scann_prototypes_host at 16,384 rows, m = 64, on the threads the call takes (at most 16)."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
import scann_oracle as so
from scann import _hip
from scann.models import latent_index as li
from scann.models.scann_model import HipModel
args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else None
N = 16384 if "--small" in sys.argv else 131072
D, MS, ROUNDS = 128, (64, 256), 5


def say(line):
    print(line, flush=True)
    if out_path:
        open(out_path, "a").write(line + "\n")


def median_ms(f, rounds=ROUNDS):
    t = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3


cfg = so.default_config("qm9")
model = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True)
eng = model.engine
rng = np.random.default_rng(7)
centres = 4.0 * rng.standard_normal((40, D), dtype=np.float32)
rows = centres[rng.integers(0, 40, N)] + rng.standard_normal((N, D), dtype=np.float32)
index = li.LatentIndex(model, "structure")
for i in range(0, N, 1 << 16):
    index.add_rows(rows[i:i + (1 << 16)])
ix = index._ix
t0 = time.perf_counter()
graph = li.neighbour_graph(index)
t_graph = (time.perf_counter() - t0) * 1e3
h = li.peaks_auto_bandwidth(graph[1], 31)
gamma = _hip.rbf_gamma(h)
say("pool of N = %d rows x %d columns around 40 centres = %.1f MB; bandwidth %.4g (automatic), gamma %.4g" % (N, D, N * D * 4 / 1e6, h, gamma))
eng.index_prototypes(ix, 8, gamma), eng.index_select(ix, None, 8)  # warm: the workspaces are in the block cache
t = {"proto": {m: [] for m in MS}, "select": {m: [] for m in MS}}
for r in range(ROUNDS):  # alternating: whatever else the box runs falls on both alike
    for m in MS:
        for name, call in (("proto", lambda: eng.index_prototypes(ix, m, gamma)), ("select", lambda: eng.index_select(ix, None, m))):
            t0 = time.perf_counter()
            got = call()
            t[name][m].append((time.perf_counter() - t0) * 1e3)
            assert got["count"] == m
med = {name: {m: float(np.median(v)) for m, v in per.items()} for name, per in t.items()}
pick = {name: (med[name][256] - med[name][64]) / 192 * 1e3 for name in med}  # us
for name, label in (("proto", "(a) scann_index_prototypes"), ("select", "(b) scann_index_select    ")):
    say("  %s  m = 64: %9.3f ms   m = 256: %9.3f ms   marginal pick %8.2f us = %7.1f GB/s of pool rows   call less its picks (m = 64): %9.3f ms" % (
        label, med[name][64], med[name][256], pick[name], N * D * 4 / (pick[name] * 1e-6) / 1e9, med[name][64] - 64 * pick[name] * 1e-3))
say("  a prototype pick costs %.2f x a k-center pick; the self-join and the rest of the call outside the picks are %.1f %% of the call at m = 64, "
    "%.1f %% at m = 256" % (pick["proto"] / pick["select"], 100 * (1 - 64 * pick["proto"] * 1e-3 / med["proto"][64]),
                            100 * (1 - 256 * pick["proto"] * 1e-3 / med["proto"][256])))
p = eng.index_prototypes(ix, 64, gamma)
weight = li.prototypes_weights(p["A"], p["B"], 64)[2]
c_ms = median_ms(lambda: eng.index_criticisms(ix, weight, p["position"], 64, gamma))
say("  (c) scann_index_criticisms, 64 picks: %9.3f ms = %8.2f us per pick" % (c_ms, c_ms / 64 * 1e3))
e2e = median_ms(lambda: index.prototypes(64, criticisms=16), rounds=3)
fixed = median_ms(lambda: index.prototypes(64, criticisms=16, bandwidth=h), rounds=3)
say("  (d) LatentIndex.prototypes(64, criticisms=16): %9.1f ms with the automatic bandwidth, %9.1f ms with the bandwidth given: the neighbour "
    "graph is %.1f %% of it (%.1f ms when timed alone, cold)" % (e2e, fixed, 100 * (e2e - fixed) / e2e, t_graph))
n_host = min(N, 16384)
host = median_ms(lambda: _hip.prototypes_host(rows[:n_host], 64, gamma), rounds=3)
say("  (e) scann_prototypes_host, %d rows, m = 64, %d CPUs: %9.1f ms" % (n_host, len(os.sched_getaffinity(0)), host))
index.free()
