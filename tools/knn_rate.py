#!/usr/bin/env python3
"""Cost of the latent-space nearest-neighbour search against the route without it, on one resident batch and box:
    python tools/knn_rate.py [structure | atom | both] [--kernels] [out.txt]
128 QM9-shaped molecules (bench.py's shape) are the queries.  structure: an index of N = 130,831 rows (QM9's size) of dense_out = 128
columns, k = 5; atom: N = 2,400,000 rows of global_dim = 128 columns (the atoms of QM9), the batch's atoms as queries, k = 5.  The index
rows are seeded random rows with the moments of the model's own representations (the search's cost does not depend on the values).
Prints (and appends to out.txt) the median per-call time, host clock around synchronous calls, warm, of
  (a) scann_forward_resident + scann_batch_download,
  (b) scann_index_query_batch (its own forward + download, the search, the merge, the copies of the results),
  (c) scann_index_query on the same queries as host vectors (search, merge and copies, no forward),
  (d) the route without the feature: the forward with the level's output selected, its download and the scann_output_read copy (device
      part), then NumPy brute force on the host against a host copy of the rows -- the product form |q|^2 + |r|^2 - 2 q.r through one
      sgemm (the fastest NumPy can do, and the form that loses near-duplicates: the comparator is given every advantage) and
      argpartition + sort of the k least (host part),
and the search's achieved GB/s over N * D * 4 bytes and FLOP/s over 3 * N * Q * D from (c), against 8 TB/s and 157 TF.
--kernels: a few calls of (c) and no timing, for a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/knn_rate.py
<what> --kernels`: the kernel time of knn_tile_kernel / knn_merge_kernel proper."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
import scann_oracle as so
from scann import _hip
from scann.models.scann_model import HipModel
args = [a for a in sys.argv[1:] if not a.startswith("--")]
what = args[0] if args else "both"
out_path = args[1] if len(args) > 1 else None
K = 5
SIZES = {"structure": 130831, "atom": 2400000}


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


def host_brute_force(q, rows, r2, k, block=16384):
    """the k least of |q|^2 + |r|^2 - 2 q.r per query, rows taken `block` queries x all rows at a time where that fits"""
    out_d, out_i = [], []
    step = max(1, min(len(q), (1 << 28) // max(len(rows), 1)))  # <= 1 GiB of fp32 distances at a time
    for i in range(0, len(q), step):
        qq = q[i:i + step]
        d = (qq * qq).sum(1)[:, None] + r2[None, :] - np.float32(2) * (qq @ rows.T)
        part = np.argpartition(d, k - 1, axis=1)[:, :k]
        pd = np.take_along_axis(d, part, axis=1)
        o = np.argsort(pd, axis=1, kind="stable")
        out_d.append(np.take_along_axis(pd, o, axis=1))
        out_i.append(np.take_along_axis(part, o, axis=1))
    return np.concatenate(out_d), np.concatenate(out_i)


def run(level):
    N, lvl = SIZES[level], _hip.KNN_LEVELS[level]
    name = "bf_property" if level == "structure" else "after_Lc"
    q = model.predict(pk, outputs=[name])[0]
    D = q.shape[1]
    rng = np.random.default_rng(7)
    rows = (rng.standard_normal((N, D), dtype=np.float32) * q.std(0) + q.mean(0)).astype(np.float32)
    ix = eng.index_create(D)
    for i in range(0, N, 1 << 18):
        eng.index_add(ix, rows[i:i + (1 << 18)])
    r2 = (rows * rows).sum(1)

    def forward():
        eng.forward_resident(rb)
        eng.download(rb)

    def route_device():
        eng.set_outputs(after_lc=level == "atom", bf_property=level == "structure")
        try:
            eng.forward_resident(rb)
            eng.download(rb)
            return eng.read_output(rb, lvl)
        finally:
            eng.set_outputs()

    calls = {"a forward + download": forward, "b index_query_batch": lambda: eng.index_query_batch(ix, rb, lvl, K),
             "c index_query, host queries": lambda: eng.index_query(ix, q, K), "d without: device part": route_device}
    if "--kernels" in sys.argv:
        for i in range(5):
            calls["c index_query, host queries"]()
        ix.free()
        return
    n, rounds = (20, 5) if level == "structure" else (3, 3)
    for i in range(3):
        for fn in calls.values():
            fn()
    t = {k: [] for k in calls}
    for r in range(rounds):  # alternating rounds: whatever else the box runs falls on all of them alike
        for k, fn in calls.items():
            t0 = time.perf_counter()
            for i in range(n):
                fn()
            t[k].append((time.perf_counter() - t0) / n)
    host_t = []
    for r in range(3 if level == "structure" else 1):
        t0 = time.perf_counter()
        hd, hi = host_brute_force(q, rows, r2, K)
        host_t.append(time.perf_counter() - t0)
    got = eng.index_query(ix, q, K)
    same = float((got["position"] == hi).mean())
    ix.free()
    med = {k: float(np.median(v)) * 1e3 for k, v in t.items()}
    host = float(np.median(host_t)) * 1e3
    Q = len(q)
    say("%s level: N = %d rows x D = %d, Q = %d queries, k = %d (medians of %d rounds of %d calls)" % (level, N, D, Q, K, rounds, n))
    for k in calls:
        say("  (%s) %-30s %9.3f ms" % (k[0], k[2:], med[k]))
    say("  (d) %-30s %9.1f ms (NumPy product form + argpartition, median of %d)" % ("without: host part", host, len(host_t)))
    say("  price of the feature (b) - (a): %.3f ms; route without it (d): %.1f ms = %.1f x (b)" % (
        med["b index_query_batch"] - med["a forward + download"], med["d without: device part"] + host,
        (med["d without: device part"] + host) / med["b index_query_batch"]))
    sec = med["c index_query, host queries"] * 1e-3
    gbs, tfs = N * D * 4 * -(-Q // 1024) / sec / 1e9, 3.0 * N * Q * D / sec / 1e12
    say("  search call (c): %.1f GB/s of index rows (%.2f %% of 8 TB/s), %.2f TFLOP/s over 3 N Q D (%.1f %% of 157 TF): nearer the %s ceiling" % (
        gbs, 100 * gbs / 8000, tfs, 100 * tfs / 157, "VALU" if tfs / 157 > gbs / 8000 else "HBM"))
    say("  places where the NumPy product form names another row than the search: %.2f %%" % (100 * (1 - same)))


for level in (("structure", "atom") if what == "both" else (what,)):
    run(level)
rb.free()
