"""NumPy reference of the attention rollout (scann_attention_rollout, include/scann_hip.h) from padded inputs and padded attention maps
[B, H, M, N], in a given dtype, written as the row gather the definition states:

  abar[l][e]     = (a[l][e][0] + ... + a[l][e][H-1]) * (1 / H), heads in index order, or a[l][e][k] for one head
  (T_l R)[i, :]  = residual * R[i, :] + (1 - residual) * sum over atom i's unmasked slots, in slot order, of abar * R[neighbour, :]
                   for an atom with a real neighbour; R[i, :] otherwise (whatever its padded map row holds: 1/N by the fp32 convention)
  R              = T_{depth-1} .. T_0 I;   attribution[j] = sum over i, ascending, of ga[i] * R[i, j]

Packed edges are the unmasked slots of real atoms in slot order, so slot order is the CSR order of the C call.  Test-only."""
import numpy as np


def masks(inputs):
    """(atom mask [B, M], real-edge mask [B, M, N]) of a padded input dict"""
    nmask = np.asarray(inputs["neighbor_mask"]) != 0
    amask = np.asarray(inputs["atom_mask"]).reshape(nmask.shape[:2]) != 0
    return amask, nmask & amask[:, :, None]


def edge_weights(a, head, dtype):
    """maps of one structure and layer [H, n, N] -> abar [n, N]"""
    a = a.astype(dtype)
    if head is not None:
        return a[head]
    ab = a[0]
    for k in range(1, a.shape[0]):
        ab = ab + a[k]
    return ab * (dtype(1) / dtype(a.shape[0]))


def rollout(inputs, maps, ga=None, residual=0.5, head=None, depth=None, dtype=np.float64):
    """maps: the L padded attention maps [B, H, M, N]; ga: padded GlobalAttention scores [B, M, 1] or None.
    -> (R [B, M, M] with row / column at the padded position of the atom and 0 at padding, attribution [B, M, 1] or None), in dtype."""
    dtype = np.dtype(dtype).type
    amask, em = masks(inputs)
    nbr = np.asarray(inputs["neighbors"])
    B, M, N = em.shape
    depth = len(maps) if depth is None else depth
    res, om = dtype(residual), dtype(1) - dtype(residual)
    R_out = np.zeros((B, M, M), dtype)
    attr = None if ga is None else np.zeros((B, M, 1), dtype)
    for b in range(B):
        pos = np.nonzero(amask[b])[0]
        n = len(pos)
        local = np.cumsum(amask[b]) - 1  # padded position -> index among the structure's real atoms
        e = em[b, pos]                                                     # [n, N]
        nb = np.clip(local[np.clip(nbr[b, pos], 0, M - 1)], 0, max(n - 1, 0))  # [n, N]; whatever a masked slot names is never used
        has = e.any(1)
        R = np.eye(n, dtype=dtype)
        for l in range(depth):
            ab = edge_weights(np.asarray(maps[l])[b][:, pos, :], head, dtype)
            acc = np.zeros((n, n), dtype)
            for k in range(N):  # slot order; a masked slot adds an exact 0
                acc = acc + np.where(e[:, k, None], ab[:, k, None] * R[nb[:, k]], dtype(0))
            R = np.where(has[:, None], res * R + om * acc, R)
        R_out[b][np.ix_(pos, pos)] = R
        if ga is not None:
            g = np.asarray(ga)[b, pos, 0].astype(dtype)
            s = np.zeros(n, dtype)
            for i in range(n):
                s = s + g[i] * R[i]
            attr[b, pos, 0] = s
    return R_out, attr


def dense_rollout(inputs, maps, residual=0.5, head=None, depth=None):
    """The same quantity by an independent route, fp64: dense n x n layer matrices (np.add.at over the real edges) multiplied with
    np.linalg.multi_dot.  -> R [B, M, M]."""
    amask, em = masks(inputs)
    nbr = np.asarray(inputs["neighbors"])
    B, M, N = em.shape
    depth = len(maps) if depth is None else depth
    out = np.zeros((B, M, M))
    for b in range(B):
        pos = np.nonzero(amask[b])[0]
        n = len(pos)
        local = np.cumsum(amask[b]) - 1
        rows, slots = np.nonzero(em[b, pos])
        cols = local[nbr[b, pos][rows, slots]]
        has = em[b, pos].any(1)
        Ts = []
        for l in range(depth):
            a = np.asarray(maps[l], dtype=np.float64)[b][:, pos, :]  # [H, n, N]
            ab = a.mean(0) if head is None else a[head]
            A = np.zeros((n, n))
            np.add.at(A, (rows, cols), ab[rows, slots])
            T = residual * np.eye(n) + (1.0 - residual) * A
            T[~has] = np.eye(n)[~has]
            Ts.append(T)
        R = Ts[0] if len(Ts) == 1 else np.linalg.multi_dot(Ts[::-1])
        out[b][np.ix_(pos, pos)] = R
    return out


def kernel_bound(depth, H, n_max_deg):
    """relative entrywise bound of the fp32 kernel arithmetic against this reference in fp64 on the same maps: all terms are
    non-negative, per layer at most H roundings in the head mean, N_max in the products and the row sum, 4 in the mix; factor 2 for
    second-order terms and an unfused multiply-add"""
    return 2.0 * depth * (H + n_max_deg + 4) * 2.0 ** -24
