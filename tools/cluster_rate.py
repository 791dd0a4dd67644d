#!/usr/bin/env python3
"""Cost of the k-means clustering on the device against the route without it, on one box:
    python tools/cluster_rate.py [--tenth] [--kernels] [out.txt]
A QM9-sized atom-level shape: N = 2,400,000 seeded standard-normal rows of 128 columns (--tenth: 240,000), k = 64 and 256, the initial
centres k rows of the pool.  Standard-normal rows do not settle in a few rounds, so max_iter updates are made.
Prints (and appends to out.txt), host clock around synchronous calls, warm, three runs each, min / median:
  (a) scann_index_kmeans with max_iter = 1 and max_iter = 5: the difference / 4 is one Lloyd iteration (assignment, sums, new centres);
  (b) LatentIndex.cluster end to end (k-center seeding, 5 updates, labels and distances copied back, medoids and inertia on the host);
  (c) the route without it, one iteration: the rows are on the host already (LatentIndex.rows(), not counted); an index of the k
      centres, Engine.index_query k = 1 of all rows against it, and the update in NumPy (a stable sort by label, np.add.reduceat).
--kernels: two calls of (a) with max_iter = 5 per k and no timing, for a run of its own under `rocprofv3 --kernel-trace --stats -- python
tools/cluster_rate.py --kernels`: the times of kmeans_assign_kernel, kmeans_sum_kernel and kmeans_finalise_kernel proper.  Per call
6 assignments and 5 sums / new centres run; the 6th launches of the latter two return at once.
The assignment is N x k x 128 (subtraction, fused multiply-add) pairs.  A packed fp32 instruction does two of either per lane, so the
kernel needs N x k x 128 packed instruction-lanes, and the chip issues 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3 T of them per second
(times 2 elements x 2 flops: the 157.3 TFLOP/s vector peak of MI355X_MICROARCH.md).  The share printed is that floor over the time."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
import scann_oracle as so
from scann.models import LatentIndex
from scann.models.scann_model import HipModel
args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else None
N = 240000 if "--tenth" in sys.argv else 2400000
D = 128
KS = (64, 256)
PACKED_LANES = 157.3e12 / 4  # packed fp32 instruction-lanes per second


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


cfg = so.default_config("qm9")
model = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True)
eng = model.engine
rng = np.random.default_rng(7)
rows = rng.standard_normal((N, D), dtype=np.float32)
lat = LatentIndex(model, "atom")
for i in range(0, N, 1 << 18):
    lat.add_rows(rows[i:i + (1 << 18)])
ix = lat._ix


def host_update(rows, label, centres):
    """the new centres in NumPy (fp32 sums in row order, not the kernel's integer sums)"""
    order = np.argsort(label, kind="stable")
    ls = label[order]
    starts = np.flatnonzero(np.r_[True, ls[1:] != ls[:-1]])
    sums = np.add.reduceat(rows[order], starts, axis=0)
    out = centres.copy()
    out[ls[starts]] = sums / np.diff(np.r_[starts, len(ls)])[:, None].astype(np.float32)
    return out


def without(centres):
    cix = eng.index_create(D)
    eng.index_add(cix, centres)
    q = eng.index_query(cix, rows, 1)
    cix.free()
    return host_update(rows, q["position"][:, 0], centres), q["position"][:, 0]


say("k-means over N = %d rows x %d columns = %.1f MB, seeded standard-normal rows" % (N, D, N * D * 4 / 1e6))
for k in KS:
    pos = (np.arange(k) * (N // k)).astype(np.int32)
    if "--kernels" in sys.argv:
        for i in range(2):
            eng.index_kmeans(ix, pos, 5)
        continue
    r5 = eng.index_kmeans(ix, pos, 5)  # warm: the workspace is in the block cache
    assert r5["n_iter"] == 5 and not r5["converged"]
    t1 = timed(lambda: eng.index_kmeans(ix, pos, 1))
    t5 = timed(lambda: eng.index_kmeans(ix, pos, 5))
    per = [(b - a) / 4 for a, b in zip(t1, t5)]
    lanes = 1.0 * N * k * D
    say("k = %3d  (a) scann_index_kmeans: max_iter 1 %8.2f / %8.2f ms, max_iter 5 %8.2f / %8.2f ms (min / median of 3): one Lloyd iteration "
        "%7.3f / %7.3f ms; if all of it were the assignment: %.1f %% of the packed-fp32 instruction rate" % (
            k, t1[0] * 1e3, t1[1] * 1e3, t5[0] * 1e3, t5[1] * 1e3, per[0] * 1e3, per[1] * 1e3, 100 * lanes / per[0] / PACKED_LANES))
    te = timed(lambda: lat.cluster(k, max_iter=5))
    say("         (b) LatentIndex.cluster(k, max_iter=5), k-center seeding and the host's medoids included: %8.2f / %8.2f ms" % (te[0] * 1e3, te[1] * 1e3))
    cen = rows[pos]
    new, lab = without(cen)  # warm
    same = int((lab == eng.index_kmeans(ix, pos, 0)["label"]).sum())
    tw = timed(lambda: without(cen))
    say("         (c) without it, one iteration (centres index, index_query k = 1 of the %d host rows, NumPy update): %8.1f / %8.1f ms = "
        "%.0f x (a)'s iteration (min against min); %d of %d labels are the device's" % (N, tw[0] * 1e3, tw[1] * 1e3, tw[0] / per[0], same, N))
lat.free()
