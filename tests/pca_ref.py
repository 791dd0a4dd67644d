"""Reference of the principal-component map of a latent index (scann_index_moments / scann_index_project and their host twins,
include/scann_hip.h), restated in plain NumPy from the header's text: eligibility, the 30-bit mean, the centred values and their scales,
b, the int64 scatter, the fp64 covariance expression, and the projection's fp32 chains with the fused multiply-add formed exactly from
fp64 pieces.  It shares no code with the C twin and needs nothing of the library."""
import numpy as np


def bits(n):
    """b = min(24, (62 - L) // 2), L the bit length of n"""
    return min(24, (62 - int(n).bit_length()) // 2)


def top_exponents(a):
    """per column the frexp exponent of the largest |value|; 0 for a column of zeros"""
    m = np.abs(a).max(axis=0)
    return np.where(m > 0, np.frexp(m)[1], 0).astype(np.int32)


def eligible(rows):
    return np.isfinite(rows).all(axis=1) if len(rows) else np.zeros(0, bool)


def quantised(rows):
    """-> (n, mean fp32, f int32, b, u int64 [n, dim]) of the eligible rows"""
    rows = np.asarray(rows, np.float32)
    x = rows[eligible(rows)]
    n = len(x)
    e = top_exponents(x)
    q = np.rint(np.ldexp(x.astype(np.float64), 30 - e)).astype(np.int64)
    S = q.sum(axis=0, dtype=np.int64)
    mean = np.ldexp(S.astype(np.float64) / np.float64(n), e - 30).astype(np.float32)
    y = (x - mean).astype(np.float32)  # fp32, rounded once
    f = top_exponents(y)
    b = bits(n)
    u = np.rint(np.ldexp(y.astype(np.float64), b - f)).astype(np.int64)
    return n, mean, f, b, u


def covariance(n, f, b, T, R, i=None):
    """the fp64 expression, as written; rows ``i`` of the matrix only (default: all)"""
    i = np.arange(len(f)) if i is None else np.asarray(i)
    Ri, Rj = R[i].astype(np.float64)[:, None], R.astype(np.float64)[None, :]
    prod = Ri * Rj
    corr = prod / np.float64(n)
    diff = T.astype(np.float64) - corr
    return np.ldexp(diff / np.float64(n - 1), f[i][:, None] + f[None, :] - 2 * b)


def moments(rows, only=None):
    """-> {"n", "mean", "cov", "col_exp", "bits"} as the C calls give them; ``only``: the rows of cov to form (cov is then [len(only), dim])"""
    n, mean, f, b, u = quantised(rows)
    assert n >= 2
    R = u.sum(axis=0, dtype=np.int64)
    T = (u.T @ u) if only is None else (u[:, np.asarray(only)].T @ u)  # int64: exact, |T| < 2^62
    # Python integers, which cannot overflow, at a few places
    rng = np.random.default_rng(0)
    for _ in range(4):
        a, c = int(rng.integers(T.shape[0])), int(rng.integers(T.shape[1]))
        col = u[:, a] if only is None else u[:, np.asarray(only)[a]]
        assert int(T[a, c]) == sum(int(p) * int(q) for p, q in zip(col.tolist(), u[:, c].tolist()))
    return {"n": n, "mean": mean, "cov": covariance(n, f, b, T, R, only), "col_exp": f, "bits": b}


def fma32(a, b, acc):
    """fl32(a * b + acc) with ONE rounding, for fp32 arrays: a * b is exact in fp64 (48 bits); its fp64 sum s with acc comes with its
    exact error (two-sum); s rounds to fp32 as the true sum does unless s lies exactly half way between two fp32 values, where the error
    decides the side"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = acc.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # s + err == p + c exactly
    r = s.astype(np.float32)
    away = np.where(s > r.astype(np.float64), np.float32(np.inf), np.float32(-np.inf))
    other = np.nextafter(r, away)  # the fp32 neighbour on s's side of r
    half_way = np.isfinite(s) & np.isfinite(other) & ((r.astype(np.float64) + other.astype(np.float64)) * 0.5 == s) & (s != r.astype(np.float64))
    towards_other = np.sign(err) == np.sign(other.astype(np.float64) - s)
    return np.where(half_way & (err != 0), np.where(towards_other, other, r), r).astype(np.float32)


def project(rows, mean, components, scale=None):
    """-> {"coords" [n, m], "dist2" [n], with scale "md2" [n]}: the chains of the definition, columns / components ascending"""
    rows, mean, W = np.asarray(rows, np.float32), np.asarray(mean, np.float32), np.asarray(components, np.float32)
    n, m = len(rows), len(W)
    with np.errstate(all="ignore"):
        y = (rows - mean).astype(np.float32)
        z = np.zeros((n, m), np.float32)
        d2 = np.zeros(n, np.float32)
        for j in range(rows.shape[1]):
            z = fma32(np.broadcast_to(y[:, j][:, None], (n, m)), np.broadcast_to(W[:, j][None, :], (n, m)), z)
            d2 = fma32(y[:, j], y[:, j], d2)
        out = {"coords": z, "dist2": d2}
        if scale is not None:
            md = np.zeros(n, np.float32)
            for c in range(m):
                t = (z[:, c] * np.float32(scale[c])).astype(np.float32)
                md = fma32(t, t, md)
            out["md2"] = md
    return out


def _pattern(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(got, want, label=""):
    """two arrays equal bit for bit (fp32 or fp64; integers by value).  A NaN equals any NaN: the definition gives neither its sign nor
    its payload.  Raises AssertionError."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind != "f":
        assert np.array_equal(got, want), label
        return
    differ = (_pattern(got) != _pattern(want)) & ~(np.isnan(got) & np.isnan(want))
    assert not differ.any(), (label, int(differ.sum()), "of", differ.size, "first at", np.argwhere(differ)[:3].tolist())


def same_moments(got, want, label=""):
    assert got["n"] == want["n"] and got["bits"] == want["bits"], (label, got["n"], want["n"], got["bits"], want["bits"])
    same(got["mean"], want["mean"], label + " mean")
    same(np.asarray(got["col_exp"], np.int32), np.asarray(want["col_exp"], np.int32), label + " col_exp")
    same(got["cov"], want["cov"], label + " cov")


def same_projection(got, want, label=""):
    assert sorted(got) == sorted(want), (label, sorted(got), sorted(want))
    for key in want:
        same(got[key], want[key], "%s %s" % (label, key))
