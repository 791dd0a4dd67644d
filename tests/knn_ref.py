"""Reference of the latent-space nearest-neighbour search (scann_index_query, include/scann_hip.h): the squared distances in fp64, the
bound the fp32 difference-form chain holds against them, and the selection under the total order (dist2 ascending, position ascending)
given a distance matrix."""
import numpy as np

EPS = 2.0 ** -24


def dist2_f64(q, rows):
    """[nq, n] fp64: sum over the columns of (q - r)^2, the difference formed in fp64 from the fp32 inputs"""
    q = np.asarray(q, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.float64)
    out = np.empty((q.shape[0], rows.shape[0]))
    for i in range(q.shape[0]):
        d = rows - q[i]
        out[i] = np.einsum("rc,rc->r", d, d)
    return out


def chain_bound(dim):
    """relative error of the fp32 chain acc = fmaf(q - r, q - r, acc) against exact arithmetic: one rounding in the difference, counted
    twice in the square, one per accumulation, and second-order terms -- all terms are non-negative, so nothing amplifies"""
    return (dim + 3) * EPS


def select(dist2, k, ids=None, query_ids=None, atoms=None):
    """The first k rows of every query under (dist2 ascending, position ascending); rows with ids[r] == query_ids[i] are skipped, rows
    with a NaN distance never qualify.  -> (dist2 [nq, k], position [nq, k], id [nq, k], atom [nq, k]); places without a row hold
    +inf, -1, -1, -1."""
    dist2 = np.asarray(dist2)
    nq, n = dist2.shape
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    atoms = np.full(n, -1, np.int32) if atoms is None else np.asarray(atoms, dtype=np.int32)
    od = np.full((nq, k), np.inf, dtype=dist2.dtype)
    op = np.full((nq, k), -1, dtype=np.int32)
    oi = np.full((nq, k), -1, dtype=np.int64)
    oa = np.full((nq, k), -1, dtype=np.int32)
    pos = np.arange(n)
    for i in range(nq):
        ok = ~np.isnan(dist2[i])
        if query_ids is not None:
            ok &= ids != query_ids[i]
        cand = pos[ok]
        order = cand[np.lexsort((cand, dist2[i][cand]))][:k]  # last key first: distance, then position
        m = len(order)
        od[i, :m], op[i, :m], oi[i, :m], oa[i, :m] = dist2[i][order], order, ids[order], atoms[order]
    return od, op, oi, oa
