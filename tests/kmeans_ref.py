"""Reference of the k-means clustering (scann_index_kmeans / scann_kmeans_host, include/scann_hip.h), restated in plain NumPy over a given
fp32 distance function ``dist2(a [na, dim], b [nb, dim]) -> [na, nb]``: eligibility, the total order (dist2 ascending, centre index
ascending), the column scales, the integer sums, the loop and its end.  It shares no code with the C twin.  ``fma_dist2`` is the kernel's
chain in plain NumPy: the fused multiply-add is formed exactly from fp64 pieces, so the restatement needs nothing of the library.  (After
an update the centres are means, not small integers: squares and sums in plain fp32 are no longer the chain, even on small-integer rows.)"""
import numpy as np


def fma32(d, acc):
    """fl32(d * d + acc) with ONE rounding, for fp32 arrays: d * d is exact in fp64 (48 bits); its fp64 sum s with acc comes with its exact
    error (two-sum); s rounds to fp32 as the true sum does unless s lies exactly half way between two fp32 values, where the error
    decides the side (and a true tie goes to even, as the conversion does)"""
    p = d.astype(np.float64) * d.astype(np.float64)
    a = acc.astype(np.float64)
    s = p + a
    bb = s - p
    err = (p - (s - bb)) + (a - bb)  # s + err == p + a exactly
    r = s.astype(np.float32)
    away = np.where(s > r.astype(np.float64), np.float32(np.inf), np.float32(-np.inf))
    other = np.nextafter(r, away)  # the fp32 neighbour on s's side of r
    half_way = np.isfinite(s) & np.isfinite(other) & ((r.astype(np.float64) + other.astype(np.float64)) * 0.5 == s) & (s != r.astype(np.float64))
    # s is r's side of the true sum iff err points from s towards r
    towards_other = np.sign(err) == np.sign(other.astype(np.float64) - s)
    return np.where(half_way & (err != 0), np.where(towards_other, other, r), r).astype(np.float32)


def fma_dist2(a, b):
    """[na, nb] fp32: acc = fma(a[j] - b[j], a[j] - b[j], acc), columns ascending, the difference rounded once -- the chain of
    scann_knn_distsq in NumPy alone"""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    out = np.zeros((len(a), len(b)), np.float32)
    with np.errstate(all="ignore"):
        for j in range(a.shape[1]):
            out = fma32(a[:, j][:, None] - b[:, j][None, :], out)
    return out


def eligible(rows):
    return np.isfinite(rows).all(axis=1) if len(rows) else np.zeros(0, bool)


def exponents(rows):
    """e_j: the frexp exponent of the largest |x| of column j over the eligible rows; 0 for a column of zeros or without such a row"""
    rows = np.asarray(rows, np.float32)
    ok = eligible(rows)
    if not ok.any():
        return np.zeros(rows.shape[1], np.int64)
    m = np.abs(rows[ok]).max(axis=0)
    return np.where(m > 0, np.frexp(m)[1], 0).astype(np.int64)


def quantise(rows, e):
    """q(x, j) = llrint(ldexp((double) x, 30 - e_j)): exact scaling, round to nearest even"""
    return np.rint(np.ldexp(np.asarray(rows, np.float64), (30 - e).astype(np.int32))).astype(np.int64)


def assign(rows, centres, dist2):
    """-> (label int32, dist2 fp32): the first centre under (dist2, index); -1 / +inf for ineligible rows and where no centre qualifies"""
    rows = np.asarray(rows, np.float32)
    n = len(rows)
    label = np.full(n, -1, np.int32)
    d2 = np.full(n, np.inf, np.float32)
    ok = np.nonzero(eligible(rows))[0]
    if len(ok) == 0:
        return label, d2
    with np.errstate(all="ignore"):
        D = np.asarray(dist2(rows[ok], np.asarray(centres, np.float32)), np.float32)
    nan = np.isnan(D)  # a NaN never qualifies
    key = np.where(nan, np.float32(np.inf), D)
    best = key.argmin(axis=1)  # the first index among the least: ties stay with the lower index
    # where the least is +inf the first centre whose distance is no NaN is taken (+inf is ordered); none: -1
    at_inf = np.isposinf(key[np.arange(len(ok)), best])
    best = np.where(at_inf, (~nan).argmax(axis=1), best)
    some = (~nan).any(axis=1)
    label[ok[some]] = best[some]
    d2[ok[some]] = D[np.arange(len(ok)), best][some]
    return label, d2


def update(rows, label, centres, e=None):
    """U(label, C): per cluster the int64 sum of q over its rows, divided in fp64, scaled back and rounded to fp32; empty clusters stay"""
    rows = np.asarray(rows, np.float32)
    e = exponents(rows) if e is None else e
    out = np.array(centres, dtype=np.float32, copy=True)
    for c in range(len(out)):
        member = label == c
        n = int(member.sum())
        if n:
            S = quantise(rows[member], e).sum(axis=0, dtype=np.int64)
            out[c] = np.ldexp(S.astype(np.float64) / np.float64(n), (e - 30).astype(np.int32)).astype(np.float32)
    return out


def kmeans(rows, init, max_iter, stop_changed, dist2):
    """-> {"label", "dist2", "centre", "size", "n_iter", "converged"} as the C calls give them"""
    rows = np.asarray(rows, np.float32)
    C = np.array(init, dtype=np.float32, copy=True)
    e = exponents(rows)
    prev = np.full(len(rows), -1, np.int32)
    t = 0
    while True:
        label, d2 = assign(rows, C, dist2)
        changed = int((label != prev).sum())
        prev = label
        if changed <= stop_changed or t == max_iter:
            break
        C = update(rows, label, C, e)
        t += 1
    return {"label": label, "dist2": d2, "centre": C, "size": np.bincount(label[label >= 0], minlength=len(C)).astype(np.int64), "n_iter": t,
            "converged": changed <= stop_changed}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want, label=""):
    """two results equal: labels, sizes, n_iter, converged, and dist2 / centres bit for bit.  Raises AssertionError."""
    assert got["n_iter"] == want["n_iter"] and bool(got["converged"]) == bool(want["converged"]), (label, got["n_iter"], want["n_iter"], got["converged"], want["converged"])
    assert got["label"].dtype == np.int32 and np.array_equal(got["label"], want["label"]), (label, int((got["label"] != want["label"]).sum()))
    assert np.array_equal(_bits(got["dist2"]), _bits(want["dist2"])), (label, "dist2")
    assert np.array_equal(_bits(got["centre"]), _bits(want["centre"])), (label, "centre")
    assert got["size"].dtype == np.int64 and np.array_equal(got["size"], want["size"]), (label, "size")


def certificate(rows, result, dist2, stop_changed=0):
    """An independent check of a finished clustering from its outputs alone: every label is the argmin under (dist2, index) of the full
    distance matrix against the returned centres, with that dist2; sizes is the bincount; and a run that converged with stop_changed = 0
    after at least one update is a fixed point: U(label, centres) == centres bit for bit.  Raises AssertionError."""
    rows = np.asarray(rows, np.float32)
    label, d2 = assign(rows, result["centre"], dist2)
    assert np.array_equal(result["label"], label)
    assert np.array_equal(_bits(result["dist2"]), _bits(d2))
    assert np.array_equal(result["size"], np.bincount(label[label >= 0], minlength=len(result["centre"])))
    if result["converged"] and stop_changed == 0 and result["n_iter"] >= 1:
        assert np.array_equal(_bits(update(rows, label, result["centre"])), _bits(result["centre"]))
