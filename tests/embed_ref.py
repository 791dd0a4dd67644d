"""An independent NumPy restatement of one iteration of the neighbour embedding (scann_embed_iterate, the definition in
include/scann_hip.h) -- dense over the pairs, the fused steps through ``pca_ref.fma32`` --, the fp64 dense gradient of the KL objective,
and the inputs the host and the GPU tests share."""
import numpy as np

import pca_ref

BLOCK, SPAN = 128, 32


def tree_sum(v):
    """fp64 [n, ...] -> the sum over axis 0 in the definition's tree: blocks of 128 positions added in position order from +0, the
    block sums in block order within a span of 32 blocks, the span sums in span order"""
    v = np.asarray(v, np.float64)
    total = np.zeros(v.shape[1:])
    for s0 in range(0, len(v), BLOCK * SPAN):
        span = np.zeros(v.shape[1:])
        for b0 in range(s0, min(len(v), s0 + BLOCK * SPAN), BLOCK):
            block = np.zeros(v.shape[1:])
            for i in range(b0, min(len(v), b0 + BLOCK)):
                block = block + v[i]
            span = span + block
        total = total + span
    return total


def pairs(y):
    """dx, dy, w [N, N] fp32 of every pair (i, j)"""
    y = np.asarray(y, np.float32)
    with np.errstate(all="ignore"):
        dx = (y[:, None, 0] - y[None, :, 0]).astype(np.float32)
        dy = (y[:, None, 1] - y[None, :, 1]).astype(np.float32)
        d = pca_ref.fma32(dy, dy, (dx * dx).astype(np.float32))
        w = (np.float32(1.0) / (np.float32(1.0) + d)).astype(np.float32)
    return dx, dy, w


def repulsion(y):
    """Z_i, Rx_i, Ry_i fp64 [N] of every row, and Z"""
    N = len(y)
    dx, dy, w = pairs(y)
    ww = (w * w).astype(np.float32)
    rows = np.arange(N)
    tot = np.zeros((3, N))
    for s0 in range(0, N, BLOCK * SPAN):
        span = np.zeros((3, N))
        for b0 in range(s0, min(N, s0 + BLOCK * SPAN), BLOCK):
            z, rx, ry = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(N, np.float32)
            for j in range(b0, min(N, b0 + BLOCK)):
                on = rows != j  # j = i is skipped: the chains take no step
                z = np.where(on, (z + w[:, j]).astype(np.float32), z)
                rx = np.where(on, pca_ref.fma32(ww[:, j], dx[:, j], rx), rx)
                ry = np.where(on, pca_ref.fma32(ww[:, j], dy[:, j], ry), ry)
            span = span + np.stack([z, rx, ry]).astype(np.float64)
        tot = tot + span
    return tot[0], tot[1], tot[2], float(tree_sum(tot[0]))


def iterate(row_first, col, p, y, u, gain, exaggeration, momentum, lr):
    """one iteration: {"y", "u", "gain", "grad" fp32 [N, 2], "z"}"""
    y, u, gain = np.asarray(y, np.float32), np.asarray(u, np.float32), np.asarray(gain, np.float32)
    p = np.asarray(p, np.float32)
    N = len(y)
    f32 = np.float32
    with np.errstate(all="ignore"):
        _, Rx, Ry, Z = repulsion(y)
        dx, dy, w = pairs(y)
        a = np.zeros((N, 2), np.float32)
        for i in range(N):
            ax, ay = np.zeros(1, np.float32), np.zeros(1, np.float32)
            for e in range(int(row_first[i]), int(row_first[i + 1])):
                j = int(col[e])
                q = np.array([p[e] * w[i, j]], np.float32)
                ax = pca_ref.fma32(q, dx[i, j:j + 1], ax)
                ay = pca_ref.fma32(q, dy[i, j:j + 1], ay)
            a[i] = ax[0], ay[0]
        R = np.stack([Rx, Ry], axis=1)
        g = (4.0 * (np.float64(f32(exaggeration)) * a.astype(np.float64) - R / Z)).astype(np.float32)
        gn = np.where((g > 0) == (u > 0), (gain * f32(0.8)).astype(np.float32), (gain + f32(0.2)).astype(np.float32))
        gn = np.maximum(gn, f32(0.01))
        t = ((f32(lr) * gn).astype(np.float32) * g).astype(np.float32)
        un = pca_ref.fma32(np.full_like(u, f32(momentum)), u, -t)
        y1 = (y + un).astype(np.float32)
        mean = (tree_sum(y1.astype(np.float64)) / np.float64(N)).astype(np.float32)
        return {"y": (y1 - mean).astype(np.float32), "u": un, "gain": gn.astype(np.float32), "grad": g, "z": Z}


def iterate_n(row_first, col, p, y, u, gain, n_iter, exaggeration, momentum, lr):
    out = {"y": np.asarray(y, np.float32), "u": np.asarray(u, np.float32), "gain": np.asarray(gain, np.float32), "z": 0.0}
    for _ in range(n_iter):
        out = iterate(row_first, col, p, out["y"], out["u"], out["gain"], exaggeration, momentum, lr)
    return out


def dense_gradient(row_first, col, p, y, exaggeration):
    """fp64, no fixed order: 4 (exaggeration sum_j p_ij w_ij (y_i - y_j) - sum_j w_ij^2 (y_i - y_j) / Z), the gradient of the KL
    divergence (at exaggeration 1) with respect to y_i for a symmetric p"""
    y = np.asarray(y, np.float64)
    N = len(y)
    diff = y[:, None, :] - y[None, :, :]
    w = 1.0 / (1.0 + (diff * diff).sum(axis=2))
    np.fill_diagonal(w, 0.0)
    P = np.zeros((N, N))
    P[np.repeat(np.arange(N), np.diff(row_first)), col] = np.asarray(p, np.float64)
    att = ((P * w)[:, :, None] * diff).sum(axis=1)
    rep = ((w * w)[:, :, None] * diff).sum(axis=1) / w.sum()
    return 4.0 * (float(exaggeration) * att - rep)


def random_graph(N, rng, most=62, symmetric=False):
    """random CSR rows of 0 .. ``most`` entries (never the row itself, columns ascending, some rows empty) with weights that sum to
    about 1; ``symmetric``: the union with the transposed edges, equal weights both ways"""
    deg = rng.integers(0, min(most, N - 1) + 1, N)
    deg[rng.random(N) < 0.1] = 0
    rows, cols = [], []
    for i in range(N):
        c = rng.choice(N - 1, int(deg[i]), replace=False)
        c = np.sort(c + (c >= i))
        rows.append(np.full(len(c), i))
        cols.append(c)
    row, col = np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64)
    val = rng.random(len(col))
    if symmetric:
        key = np.unique(np.concatenate([row * N + col, col * N + row]))
        row, col = key // N, key % N
        lo, hi = np.minimum(row, col), np.maximum(row, col)
        val = ((lo * 7919 + hi * 104729) % 1000 + 1) / 1000.0  # a function of the unordered pair
    row_first = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=N), out=row_first[1:])
    p = (val / max(val.sum(), 1e-300)).astype(np.float32)
    return row_first, col.astype(np.int32), p


def random_state(N, seed, spread=1.0, most=62, symmetric=False):
    """(row_first, col, p, y, u, gain) of a layout in mid-flight"""
    rng = np.random.default_rng(seed)
    row_first, col, p = random_graph(N, rng, most, symmetric)
    y = (spread * rng.standard_normal((N, 2))).astype(np.float32)
    u = (0.01 * spread * rng.standard_normal((N, 2))).astype(np.float32)
    gain = rng.choice(np.array([0.01, 0.8, 1.0, 1.2, 2.4], np.float32), (N, 2))
    return row_first, col, p, y, u, gain


def same_state(got, want, what, keys=("y", "u", "gain", "grad")):
    """every bit of the arrays and of z"""
    for k in keys:
        a, b = np.ascontiguousarray(got[k], np.float32), np.ascontiguousarray(want[k], np.float32)
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        bad = np.nonzero(a.view(np.uint32) != b.view(np.uint32))
        assert not len(bad[0]), "%s: %s differs at %d places, first row %d: %r against %r" % (
            what, k, len(bad[0]), bad[0][0], a[bad[0][0]], b[bad[0][0]])
    assert np.float64(got["z"]).view(np.uint64) == np.float64(want["z"]).view(np.uint64), (what, "z", got["z"], want["z"])


def blobs(seed=0, new=0):
    """600 rows in 16 columns, six planted blobs of 100: centres 6 * standard_normal, unit noise; (rows fp32, labels), and with ``new``
    that many further rows per blob drawn behind them: (rows, labels, new_rows, new_labels)"""
    rng = np.random.default_rng(seed)
    centres = 6.0 * rng.standard_normal((6, 16))
    labels = np.repeat(np.arange(6), 100)
    rows = (centres[labels] + rng.standard_normal((600, 16))).astype(np.float32)
    if not new:
        return rows, labels
    new_labels = np.repeat(np.arange(6), new)
    return rows, labels, (centres[new_labels] + rng.standard_normal((6 * new, 16))).astype(np.float32), new_labels


def blob_share(coords, labels, k=5):
    """the share of rows whose ``k`` nearest map neighbours all carry the row's label"""
    c = np.asarray(coords, np.float64)
    d = ((c[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    near = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float((labels[near] == labels[:, None]).all(axis=1).mean())
