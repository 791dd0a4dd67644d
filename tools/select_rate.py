#!/usr/bin/env python3
"""Cost of the greedy k-center selection on the device against the route without it, on one box:
    python tools/select_rate.py [structure | atom | both] [--kernels] [out.txt]
structure: a pool of N = 130,831 rows (QM9's size) of 128 columns; atom: N = 2,400,000 rows of 128 columns (the atoms of QM9).  The rows
are seeded random rows (the cost does not depend on the values); no reference (the reference costs one k = 1 query of the pool, which
tools/knn_rate.py measures).  M = 100 and M = 1,000.
Prints (and appends to out.txt), host clock around synchronous calls, warm, medians of repeated runs:
  (a) scann_index_select: all M picks enqueued on one stream, one wait;
  (b) the route without it: scann_index_read of the whole pool, then the same greedy loop in NumPy on the host -- per pick one pass
      d = ((rows - centre)^2).sum(1), mind = minimum(mind, d), argmax -- timed over a few picks and scaled to M (every pick costs the same),
and per pick the time and the bytes per second of a pick, N x stride x 4 bytes / time, beside the 8 TB/s of HBM.
--kernels: two calls of (a) with M = 100 and no timing, for a run of its own under `rocprofv3 --kernel-trace --stats -- python
tools/select_rate.py <what> --kernels`: the time of kcenter_step_kernel proper."""
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
SIZES = {"structure": 130831, "atom": 2400000}
D = 128
HOST_PICKS = {"structure": 20, "atom": 3}  # picks of the host loop that are timed


def say(line):
    print(line, flush=True)
    if out_path:
        open(out_path, "a").write(line + "\n")


cfg = so.default_config("qm9")
eng = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True).engine


def host_picks(rows, n_pick):
    """the greedy loop in NumPy (fp32, not the kernel's bits): -> positions"""
    mind = np.full(len(rows), np.inf, np.float32)
    pos = []
    for i in range(n_pick):
        p = int(np.argmax(mind))
        pos.append(p)
        mind[p] = -1.0
        d = rows - rows[p]
        np.minimum(mind, np.einsum("rc,rc->r", d, d), out=mind)
    return pos


def run(level):
    N = SIZES[level]
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((N, D), dtype=np.float32)
    ix = eng.index_create(D)
    for i in range(0, N, 1 << 18):
        eng.index_add(ix, rows[i:i + (1 << 18)])
    del rows
    if "--kernels" in sys.argv:
        for i in range(2):
            eng.index_select(ix, None, 100)
        ix.free()
        return
    eng.index_select(ix, None, 100)  # warm: the workspace is in the block cache
    rounds = 5 if level == "structure" else 3
    t = {100: [], 1000: []}
    for r in range(rounds):  # alternating: whatever else the box runs falls on both alike
        for m in t:
            t0 = time.perf_counter()
            got = eng.index_select(ix, None, m)
            t[m].append(time.perf_counter() - t0)
            assert got["count"] == m
    read_t, host_t = [], []
    for r in range(3 if level == "structure" else 1):
        t0 = time.perf_counter()
        back = eng.index_read(ix)[0]
        read_t.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        hp = host_picks(back, HOST_PICKS[level])
        host_t.append((time.perf_counter() - t0) / HOST_PICKS[level])
    same = int(np.sum(np.asarray(hp) == got["position"][:len(hp)]))
    ix.free()
    read, per_host = float(np.median(read_t)), float(np.median(host_t))
    nbytes = N * D * 4
    say("%s level: pool of N = %d rows x %d columns = %.1f MB (%s the 256 MiB Infinity Cache), no reference" % (
        level, N, D, nbytes / 1e6, "fits" if nbytes < (256 << 20) else "does not fit"))
    for m, v in t.items():
        sec = float(np.median(v))
        say("  M = %4d  (a) scann_index_select %10.3f ms = %8.2f us per pick, %7.1f GB/s of pool rows per pick (%.1f %% of 8 TB/s)   "
            "(b) without: read %.1f ms + host loop %.1f ms = %.1f x (a)" % (
                m, sec * 1e3, sec / m * 1e6, nbytes / (sec / m) / 1e9, 100 * nbytes / (sec / m) / 8e12, read * 1e3, per_host * m * 1e3,
                (read + per_host * m) / sec))
    d100, d1000 = float(np.median(t[100])), float(np.median(t[1000]))
    say("  marginal pick (M = 1,000 against M = 100): %.2f us; host loop: %.2f ms per pick (median of %d runs of %d picks); device per pick "
        "%s the host's" % ((d1000 - d100) / 900 * 1e6, per_host * 1e3, len(host_t), HOST_PICKS[level],
                           "beats" if d1000 / 1000 < per_host else "DOES NOT beat"))
    say("  first %d picks of the NumPy loop that are the device's: %d (NumPy's sums are not the kernel's chain; ties may fall otherwise)" % (len(hp), same))


for level in (("structure", "atom") if what == "both" else (what,)):
    run(level)
