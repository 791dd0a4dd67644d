"""A plain NumPy restatement of the silhouette pass (scann_index_silhouette / scann_silhouette_host, include/scann_hip.h) and the cases
the host and the GPU tests share.  The terms go through ``_hip.knn_dist2_matrix`` (the chain of scann_knn_distsq), ``np.sqrt`` on fp32
(correctly rounded), ``np.ldexp`` on fp32, ``np.rint`` and integer sums; the finish is fp64 NumPy.  Nothing here is threaded or tiled."""
import numpy as np

LIMIT = 2 ** 31


class OutOfRange(Exception):
    pass


def counting_rows(rows, labels):
    return np.isfinite(rows).all(axis=1) & (np.asarray(labels) >= 0)


def silhouette(rows, labels, n_clusters, qpos=None, squared=False, shift=0):
    """{"count", "a", "b", "other", "sums"} of the definition; OutOfRange where the call returns SCANN_ERR_RANGE"""
    from scann import _hip

    rows = np.ascontiguousarray(rows, np.float32)
    labels = np.asarray(labels, np.int64)
    N, C = len(rows), int(n_clusters)
    cnt = counting_rows(rows, labels)
    count = np.bincount(labels[cnt], minlength=C).astype(np.int64)
    q = np.arange(N) if qpos is None else np.asarray(qpos, np.int64)
    a, b = np.full(len(q), np.nan), np.full(len(q), np.nan)
    other = np.full(len(q), -1, np.int32)
    sums = np.full((len(q), C), -1, np.int64)
    live = np.flatnonzero(cnt[q]) if len(q) else np.zeros(0, np.int64)
    if len(live):
        with np.errstate(invalid="ignore", over="ignore"):
            d = _hip.knn_dist2_matrix(rows[q[live]], rows)                   # fp32 [n_live, N], the query first
            e = d if squared else np.sqrt(d)                                 # fp32
            f = np.ldexp(e, np.int32(shift))                                 # fp32: ldexpf
        assert e.dtype == np.float32 and f.dtype == np.float32
        pair = cnt[None, :] & (np.arange(N)[None, :] != q[live][:, None])    # the terms of the call
        if (~np.isfinite(e[pair])).any() or (np.rint(f[pair].astype(np.float64)) > LIMIT).any():
            raise OutOfRange()
        t = np.where(pair, np.rint(f), 0).astype(np.int64)
        onehot = (labels[None, :] == np.arange(C)[:, None]) & cnt[None, :]   # [C, N]
        S = t @ onehot.T.astype(np.int64)                                    # int64 sums: no order
        sums[live] = S
        for r, i in enumerate(live):
            ci = labels[q[i]]
            a[i] = 0.0 if count[ci] == 1 else np.ldexp(np.float64(S[r, ci]), -shift) / np.float64(count[ci] - 1)
            for c in range(C):                                               # ascending: among equal means the lower c stays
                if c == ci or count[c] == 0:
                    continue
                m = np.ldexp(np.float64(S[r, c]), -shift) / np.float64(count[c])
                if other[i] < 0 or m < b[i]:
                    b[i], other[i] = m, c
    return {"count": count, "a": a, "b": b, "other": other, "sums": sums}


def same(got, want, what=""):
    """every output bit for bit"""
    assert np.array_equal(got["count"], want["count"]), what + ": count"
    assert np.array_equal(got["sums"], want["sums"]), what + ": sums"
    assert np.array_equal(got["other"], want["other"]), what + ": other"
    for key in ("a", "b"):
        assert got[key].dtype == np.float64
        assert np.array_equal(got[key].view(np.uint64) | (np.isnan(got[key]) * np.uint64(1 << 63)),  # (a NaN's sign is no part of it)
                              np.asarray(want[key], np.float64).view(np.uint64) | (np.isnan(want[key]) * np.uint64(1 << 63))), what + ": " + key


def blobs(n_per, dim, k, seed, spread=0.05, offset=0.0):
    """k Gaussian blobs of n_per rows around well-separated centres: (rows fp32, planted labels)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, dim)) * 1.0
    rows = np.concatenate([c + spread * rng.standard_normal((n_per, dim)) for c in centres]) + offset
    lab = np.repeat(np.arange(k), n_per)
    order = rng.permutation(len(rows))
    return rows[order].astype(np.float32), lab[order].astype(np.int32)


def pathological_case(N, dim, seed=0, C=5):
    """(rows, labels): random rows in C loose groups with what goes wrong in one pool -- unlabelled rows (-1), cluster 3 empty, cluster 4
    one row, coincident rows (in one cluster and across two), rows with a NaN / an inf (one of them labelled), a row far away"""
    rng = np.random.default_rng(1000 * N + dim + seed)
    lab = rng.integers(0, 3, N).astype(np.int32)
    rows = (rng.standard_normal((N, dim)) + 2.0 * lab[:, None] * (np.arange(dim) % 3 == 0)).astype(np.float32)
    if N >= 8:
        lab[::7] = -1                       # unlabelled
        rows[3] = rows[1]                   # coincident rows, whatever their labels
        rows[5] = rows[1]
        lab[5] = (lab[1] + 1) % 3
        lab[1], lab[3] = max(lab[1], 0), max(lab[1], 0)
    if N >= 60:
        rows[10, dim - 1] = np.nan          # labelled, not eligible: counts for nothing
        lab[10] = 1
        rows[11, 0] = np.inf
        rows[12, dim // 2] = -np.inf
        lab[12] = -1
        rows[20] *= np.float32(30.0)        # far, finite
        rows[40:48] = rows[39]              # a run of coincident rows
        lab[40:48] = lab[39] = 2
    if N >= 2:
        lab[N - 1] = 4                      # a singleton
    return rows, lab


def shift_for(rows, metric):
    """the shift ``LatentIndex.silhouette`` would choose for these rows (0 with fewer than two eligible rows)"""
    from scann import _hip

    try:
        mo = _hip.moments_host(rows)
    except ValueError:
        return 0
    return _hip.silhouette_shift(mo["col_exp"], np.diagonal(mo["cov"]), metric)
