#!/usr/bin/env python3
"""Cost of the structure matching against the atom-level row search and against the route without it, on one resident batch and box:
    python tools/match_rate.py [--kernels] [out.txt]
128 QM9-shaped molecules (bench.py's shape) are the query structures; the index holds N = 2,400,000 rows of global_dim = 128 columns (the
atoms of QM9) in segments of 12 .. 25 rows (the sizes of the batch's molecules, drawn at random), k = 5, chamfer.  The index rows are
seeded random rows with the moments of the model's own representations (the cost does not depend on the values).
Prints (and appends to out.txt) the median per-call time, host clock around synchronous calls, warm, of
  (a) scann_forward_resident + scann_batch_download,
  (b) scann_index_match_batch (its own forward + download, the tile kernel, the merge, the pair kernel, the copies of the results),
  (c) scann_index_query_batch at atom level on the same index and batch: the same 3 N Q D of distance arithmetic, reduced per row,
  (d) scann_index_match on the same rows as host vectors (no forward),
  (e) the route without the feature: the forward with after_Lc selected, its download and the scann_output_read copy (device part),
      then NumPy on the host against a host copy of the rows -- per query structure the product form |q|^2 + |r|^2 - 2 q.r through one
      sgemm, minimum.reduceat / add.reduceat over the segments, argpartition + sort of the k least (host part; timed on the first 8
      structures and scaled to the batch's 128),
and the ratio (b) - (a) over (c) - (a): the reductions, the tile padding and the range plan on top of the same arithmetic.
--kernels: a few calls of (d) and no timing, for a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/match_rate.py
--kernels`: the kernel time of match_tile_kernel / knn_merge_kernel / match_pair_kernel proper."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
import scann_oracle as so
from scann import _hip
from scann.models.scann_model import HipModel
args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else None
K, N, HOST_SETS = 5, 2400000, 8


def say(line):
    print(line, flush=True)
    if out_path:
        open(out_path, "a").write(line + "\n")


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
sizes = []
own = np.diff(q_first)
while sum(sizes) < N:
    sizes.extend(int(s) for s in rng.choice(own, 4096))
sizes = np.array(sizes)
sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), N)) + 1]
sizes[-1] -= sizes.sum() - N
seg_first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
ids = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
rows = (rng.standard_normal((N, D), dtype=np.float32) * q.std(0) + q.mean(0)).astype(np.float32)
ix = eng.index_create(D)
for i in range(0, N, 1 << 18):
    eng.index_add(ix, rows[i:i + (1 << 18)], ids[i:i + (1 << 18)])
assert len(eng.index_segments(ix)[0]) == len(sizes)


def forward():
    eng.forward_resident(rb)
    eng.download(rb)


def route_device():
    eng.set_outputs(after_lc=True)
    try:
        eng.forward_resident(rb)
        eng.download(rb)
        return eng.read_output(rb, _hip.OUT_AFTER_LC)
    finally:
        eng.set_outputs()


def host_match(qs, r2):
    """chamfer of one query structure against every segment, the k least: the product form, reduceat over the segments"""
    d = (qs * qs).sum(1)[:, None] + r2[None, :] - np.float32(2) * (qs @ rows.T)
    f = np.minimum.reduceat(d, seg_first[:-1], axis=1).astype(np.float64).mean(0)
    g = np.add.reduceat(d.min(0).astype(np.float64), seg_first[:-1]) / sizes
    score = f + g
    part = np.argpartition(score, K - 1)[:K]
    return part[np.argsort(score[part], kind="stable")]


calls = {"a forward + download": forward, "b index_match_batch": lambda: eng.index_match_batch(ix, rb, K, "chamfer"),
         "c index_query_batch, atom level": lambda: eng.index_query_batch(ix, rb, _hip.OUT_AFTER_LC, K),
         "d index_match, host queries": lambda: eng.index_match(ix, q, q_first, K, "chamfer"), "e without: device part": route_device}
if "--kernels" in sys.argv:
    for i in range(5):
        calls["d index_match, host queries"]()
    ix.free()
    rb.free()
    sys.exit(0)
n, rounds = 3, 3
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
r2 = (rows * rows).sum(1)
t0 = time.perf_counter()
host = [host_match(q[q_first[s]:q_first[s + 1]], r2) for s in range(HOST_SETS)]
host_ms = (time.perf_counter() - t0) * 1e3 * len(own) / HOST_SETS
got = eng.index_match(ix, q, q_first, K, "chamfer")
same = float(np.mean([np.array_equal(got["segment"][s], host[s]) for s in range(HOST_SETS)]))
ix.free()
rb.free()
med = {k: float(np.median(v)) * 1e3 for k, v in t.items()}
Q = len(q)
say("structure matching: N = %d rows x D = %d in %d segments, %d query structures of %d atoms in all, k = %d, chamfer (medians of %d rounds of %d calls)" % (
    N, D, len(sizes), len(own), Q, K, rounds, n))
for k in calls:
    say("  (%s) %-34s %9.3f ms" % (k[0], k[2:], med[k]))
say("  (e) %-34s %9.1f ms (NumPy product form + reduceat, %d structures timed, scaled to %d)" % ("without: host part", host_ms, HOST_SETS, len(own)))
a, b, c = med["a forward + download"], med["b index_match_batch"], med["c index_query_batch, atom level"]
say("  price of the feature (b) - (a): %.3f ms; the atom-level search (c) - (a): %.3f ms; ratio %.2f" % (b - a, c - a, (b - a) / (c - a)))
say("  route without it (e): %.1f ms = %.1f x (b)" % (med["e without: device part"] + host_ms, (med["e without: device part"] + host_ms) / b))
sec = med["d index_match, host queries"] * 1e-3
say("  match call (d): %.2f TFLOP/s over 3 N Q D (%.1f %% of 157 TF)" % (3.0 * N * Q * D / sec / 1e12, 100 * 3.0 * N * Q * D / sec / 1e12 / 157))
say("  query structures (of the %d timed on the host) for which the NumPy product form names the same k segments in order: %.0f %%" % (HOST_SETS, 100 * same))
