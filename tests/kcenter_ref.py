"""Reference of the greedy k-center selection (scann_index_select / scann_kcenter_host, include/scann_hip.h), restated in plain NumPy
over a given fp32 distance function ``dist2(a [na, dim], b [nb, dim]) -> [na, nb]``: eligibility, the total order (mind descending,
position ascending), the stop rule and the tails.  It shares no code with the C twin."""
import numpy as np


def exact_dist2(a, b):
    """plain NumPy squares and sums in fp32: the kernel's chain exactly where every difference, square and partial sum is a small
    integer (no fused multiply-add is needed there)"""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    out = np.zeros((len(a), len(b)), np.float32)
    with np.errstate(all="ignore"):
        for j in range(a.shape[1]):  # columns ascending
            d = a[:, j][:, None] - b[:, j][None, :]
            out = (d * d + out).astype(np.float32)
    return out


def select(rows, ref, m, stop_dist2, dist2):
    """-> (position [m] int32, radius2 [m] fp32, count); places behind count: -1 / +inf"""
    rows = np.asarray(rows, np.float32)
    n = len(rows)
    pos = np.full(m, -1, np.int32)
    rad = np.full(m, np.inf, np.float32)
    if n == 0:
        return pos, rad, 0
    eligible = np.isfinite(rows).all(axis=1)
    mind = np.full(n, np.inf, np.float32)
    if ref is not None and len(ref):
        with np.errstate(all="ignore"):
            d = np.asarray(dist2(rows, np.asarray(ref, np.float32)), np.float32)
        d = np.where(np.isnan(d), np.float32(np.inf), d)  # a NaN distance never counts
        mind = d.min(axis=1)
    picked = np.zeros(n, bool)
    count = 0
    for i in range(m):
        cand = np.nonzero(eligible & ~picked)[0]
        if len(cand) == 0:
            break
        top = mind[cand].max()
        p = int(cand[mind[cand] == top][0])  # the first position among the largest
        if stop_dist2 > 0 and mind[p] < np.float32(stop_dist2):
            break
        pos[i], rad[i] = p, mind[p]
        picked[p] = True
        count += 1
        with np.errstate(all="ignore"):
            d = np.asarray(dist2(rows, rows[p:p + 1]), np.float32)[:, 0]
        upd = eligible & (d < mind)  # (rows that are not eligible are never read again)
        mind = np.where(upd, d, mind)
    return pos, rad, count


def certificate(rows, ref, pos, radius2, count, dist2, stop_dist2=0.0, m=None):
    """An independent check of a finished selection from the full distance matrices: radius2[i] is the least distance of pick i to the
    reference and the earlier picks; no unpicked eligible row had a larger one at that moment, and none with an equal one lay at a lower
    position; the selection ended for one of the three reasons.  Raises AssertionError."""
    rows = np.asarray(rows, np.float32)
    n = len(rows)
    eligible = np.isfinite(rows).all(axis=1)
    with np.errstate(all="ignore"):
        D = np.asarray(dist2(rows, rows), np.float32)
        base = np.full(n, np.inf, np.float32)
        if ref is not None and len(ref):
            dr = np.asarray(dist2(rows, np.asarray(ref, np.float32)), np.float32)
            base = np.where(np.isnan(dr), np.float32(np.inf), dr).min(axis=1)
    pos = np.asarray(pos)[:count]
    assert len(set(pos.tolist())) == count and np.all(eligible[pos])
    taken = np.zeros(n, bool)
    cover = base.copy()
    for i, p in enumerate(pos):
        assert np.float32(radius2[i]).view(np.uint32) == cover[p].view(np.uint32), (i, p, radius2[i], cover[p])
        others = eligible & ~taken
        assert not np.any(cover[others] > cover[p]), (i, p)
        assert not np.any((cover[others] == cover[p]) & (np.arange(n)[others] < p)), (i, p)
        taken[p] = True
        cover = np.where(eligible & (D[:, p] < cover), D[:, p], cover)
    left = eligible & ~taken
    if m is not None and count < m and left.any():  # it stopped early with rows left: only the threshold can have ended it
        assert stop_dist2 > 0 and cover[left].max() < np.float32(stop_dist2)
