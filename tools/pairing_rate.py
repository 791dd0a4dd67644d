#!/usr/bin/env python3
"""Cost of the one-to-one pairing (scann_index_pairing_batch / scann_index_pairing) beside the match call that feeds it, on one box:
    python tools/pairing_rate.py [out.txt]
128 QM9-shaped molecules (bench.py's shape) are the query structures; the index holds N = 2,400,000 rows of global_dim = 128 columns in
segments of the batch's molecule sizes (tools/match_rate.py's index), shortlist 32, k = 5, chamfer.  Prints (and appends to out.txt) the
median per-call time, host clock around synchronous calls, warm, alternating rounds, of
  (a) scann_forward_resident + scann_batch_download,
  (b) scann_index_match_batch with k = 5 and (c) with k = 32 (the shortlist),
  (d) scann_index_pairing_batch: its forward, the shortlist (c), the pairing of the 128 x 32 pairs, the rerank,
  (e) scann_index_pairing on the same 4,096 pairs as host queries (no forward, no shortlist): staging, pairing_kernel, the copies back,
then the same call (e) in pairs per second on indices of their own -- QM9-sized pairs, Q = 64, 128 x 128 and the 128 x 1 worst case (all
dummy rows identical: about Q^2 / 2 steps) -- and the host route for the 4,096 pairs: the rows downloaded, NumPy distances and SciPy's
linear_sum_assignment on 16 threads."""
import os, sys, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
import scann_oracle as so
from scann import _hip
from scann.models.scann_model import HipModel
args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else None
K, S, N = 5, 32, 2400000


def say(line):
    print(line, flush=True)
    if out_path:
        open(out_path, "a").write(line + "\n")


def median_ms(calls, n=3, rounds=3):
    for i in range(2):
        for fn in calls.values():
            fn()
    t = {k: [] for k in calls}
    for r in range(rounds):  # alternating rounds: whatever else the box runs falls on all of them alike
        for k, fn in calls.items():
            t0 = time.perf_counter()
            for i in range(n):
                fn()
            t[k].append((time.perf_counter() - t0) / n)
    return {k: float(np.median(v)) * 1e3 for k, v in t.items()}


cfg = so.default_config("qm9")
inputs = so.pad_batch(*so.synth_dataset(128, 5), g_update=True)[0]
pk = _hip.pack_inputs(inputs)
model = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True)
eng = model.engine
rb = eng.upload(pk)
q = model.predict(pk, outputs=["after_Lc"])[0]
q_first = np.asarray(pk.mol_offset, dtype=np.int64)
D = q.shape[1]
rng = np.random.default_rng(7)
own = np.diff(q_first)
sizes = []
while sum(sizes) < N:
    sizes.extend(int(s) for s in rng.choice(own, 4096))
sizes = np.array(sizes)
sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), N)) + 1]
sizes[-1] -= sizes.sum() - N
seg_first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
ix = eng.index_create(D)
for i in range(0, N, 1 << 18):  # (a chunk of rows at a time: the host never holds the whole index)
    j = min(N, i + (1 << 18))
    rows = (rng.standard_normal((j - i, D), dtype=np.float32) * q.std(0) + q.mean(0)).astype(np.float32)
    eng.index_add(ix, rows, np.searchsorted(seg_first, np.arange(i, j), side="right").astype(np.int64) - 1)
assert len(eng.index_segments(ix)[0]) == len(sizes)

short = eng.index_match(ix, q, q_first, S, "chamfer")
ps, pg = np.repeat(np.arange(len(own)), S), short["segment"].ravel()
assert np.all(pg >= 0)


def forward():
    eng.forward_resident(rb)
    eng.download(rb)


calls = {"a forward + download": forward, "b index_match_batch, k = 5": lambda: eng.index_match_batch(ix, rb, K, "chamfer"),
         "c index_match_batch, k = 32": lambda: eng.index_match_batch(ix, rb, S, "chamfer"),
         "d index_pairing_batch, shortlist 32, k = 5": lambda: eng.index_pairing_batch(ix, rb, K, S, "chamfer"),
         "e index_pairing, the 4,096 pairs": lambda: eng.index_pairing(ix, q, q_first, ps, pg)}
med = median_ms(calls)
say("pairing rerank: N = %d rows x D = %d in %d segments, %d query structures of %d atoms in all, shortlist %d, k = %d, chamfer (medians of 3 rounds of 3 calls)" % (
    N, D, len(sizes), len(own), len(q), S, K))
for k in calls:
    say("  (%s) %-44s %9.3f ms" % (k[0], k[2:], med[k]))
c, d, e = med["c index_match_batch, k = 32"], med["d index_pairing_batch, shortlist 32, k = 5"], med["e index_pairing, the 4,096 pairs"]
say("  the rerank adds (d) - (c) = %.3f ms to the match call that feeds it (%.3f ms): %.1f %%; the pairing call alone (e): %.3f ms = %.0f pairs/s" % (
    d - c, c, 100 * (d - c) / c, e, len(ps) / e * 1e3))
if d - c > c:
    say("  THE RERANK COSTS MORE THAN THE MATCH CALL: see (e) for where the time goes")

# the host route for the same pairs: rows downloaded, SciPy's solver, 16 threads
from scipy.optimize import linear_sum_assignment


def host_pair(e):
    s, g = ps[e], pg[e]
    a, b = q[q_first[s]:q_first[s + 1]], seg_rows[g]
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(2)
    r, cidx = linear_sum_assignment(d2)
    return float(d2[r, cidx].sum())


t0 = time.perf_counter()
need = np.unique(pg)
seg_rows = {int(g): eng.index_read(ix, int(seg_first[g]), int(sizes[g]))[0] for g in need}
t_read = time.perf_counter() - t0
t0 = time.perf_counter()
with ThreadPoolExecutor(16) as pool:
    list(pool.map(host_pair, range(len(ps))))
t_solve = time.perf_counter() - t0
say("  host route for the 4,096 pairs: %d segments read back %.1f ms, NumPy distances + linear_sum_assignment on 16 threads %.1f ms: %.1f x (e)" % (
    len(need), t_read * 1e3, t_solve * 1e3, (t_read + t_solve) * 1e3 / e))
ix.free()
rb.free()

# the pairing call alone on pairs of one shape: n query atoms against m rows, P pairs in one call
say("pairing call alone (scann_index_pairing, host queries; staging, pairing_kernel, copies back; medians of 3 rounds of 3 calls)")
for label, n, m, P in (("QM9-sized, 18 x 18", 18, 18, 8192), ("Q = 64, 64 x 64", 64, 64, 4096), ("128 x 128", 128, 128, 2048),
                       ("128 x 1 (the worst case)", 128, 1, 2048), ("1 x 128", 1, 128, 2048)):
    n_seg, n_set = 256, 64
    rows = rng.standard_normal((n_seg * m, D), dtype=np.float32)
    qq = rng.standard_normal((n_set * n, D), dtype=np.float32)
    one = eng.index_create(D)
    eng.index_add(one, rows, np.repeat(np.arange(n_seg, dtype=np.int64), m))
    a, b = rng.integers(0, n_set, P), rng.integers(0, n_seg, P)
    ms = median_ms({"x": lambda: eng.index_pairing(one, qq, np.arange(n_set + 1) * n, a, b)})["x"]
    say("  %-26s %5d pairs  %9.3f ms  %10.0f pairs/s" % (label, P, ms, P / ms * 1e3))
    one.free()
