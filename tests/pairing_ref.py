"""The definition of the pairing (include/scann_hip.h, scann_index_pairing) in NumPy, for tests: the cost matrix from a given matrix D of
fp32 squared distances, the optimum from SciPy's linear_sum_assignment and, for Q <= 7, from all permutations as well, so that the value
does not rest on SciPy alone.  The optimum, the shift and the score do not depend on an algorithm; the map does (ties), so the tests
compare maps between the kernel and the host twin and check here that a map is a one-to-one map that attains the optimum."""
import itertools
import math

import numpy as np

MAX_ATOMS = 128


def shift_of(dmax):
    """30 - ilogb(Dmax) for Dmax > 0 (math.frexp gives the true exponent of a subnormal too), 0 for Dmax = 0"""
    dmax = float(dmax)
    return 0 if dmax == 0 else 30 - (math.frexp(dmax)[1] - 1)


def quantise(D):
    """(shift, t int64 [n, m]) of a comparable D, None otherwise"""
    D = np.asarray(D, np.float32)
    if D.shape[1] > MAX_ATOMS or not np.isfinite(D).all():
        return None
    shift = shift_of(D.max())
    t = np.rint(np.ldexp(D.astype(np.float64), shift))  # exact scaling, then to nearest even
    assert t.min() >= 0 and t.max() <= 2 ** 31
    return shift, t.astype(np.int64)


def cost_matrix(t):
    """the square matrix of step 4 from t [n, m]"""
    n, m = t.shape
    Q = max(n, m)
    C = np.zeros((Q, Q), np.int64)
    C[:n, :m] = t
    if n < m:
        C[n:, :] = t.min(axis=0)[None, :]
    if m < n:
        C[:, m:] = t.min(axis=1)[:, None]
    return C


def optimum(C):
    """min over permutations of sum C[i, pi(i)]: SciPy's, and by brute force where that is feasible"""
    from scipy.optimize import linear_sum_assignment

    C = np.asarray(C, np.int64)
    r, c = linear_sum_assignment(C)
    total = int(C[r, c].sum())
    if C.shape[0] <= 7:
        rows = np.arange(C.shape[0])
        assert total == min(int(C[rows, list(p)].sum()) for p in itertools.permutations(range(C.shape[0])))
    return total


def procedure(C):
    """step 6 word for word: (col_of_row, total); O(Q^3) in Python, for small matrices"""
    C = [[int(x) for x in row] for row in np.asarray(C)]
    Q, INF = len(C), 1 << 62
    u, v, p = [0] * Q, [0] * Q, [-1] * Q
    for i in range(Q):
        minv, used, way, j0 = [INF] * Q, [False] * Q, [-1] * Q, -1
        while True:
            if j0 >= 0:
                used[j0] = True
            i0 = i if j0 < 0 else p[j0]
            delta, j1 = INF, -1
            for j in range(Q):
                if used[j]:
                    continue
                cur = C[i0][j] - u[i0] - v[j]
                assert cur >= 0  # reduced costs never go negative
                if cur < minv[j]:
                    minv[j], way[j] = cur, j0
                if minv[j] < delta:
                    delta, j1 = minv[j], j
            u[i] += delta
            for j in range(Q):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == -1:
                break
        while j0 >= 0:
            p[j0] = i if way[j0] == -1 else p[way[j0]]
            j0 = way[j0]
    col = np.empty(Q, np.int32)
    col[p] = np.arange(Q)
    return col, sum(C[p[j]][j] for j in range(Q))


def score_of(total, shift, Q):
    return np.float32(math.ldexp(float(total), -shift) / float(Q))  # total < 2^53: exact; one division in fp64, one rounding to fp32


def pair(D):
    """{"score", "total", "shift"} of the definition from D [n, m] fp32"""
    q = quantise(D)
    if q is None:
        return {"score": np.float32(np.inf), "total": -1, "shift": 0}
    shift, t = q
    total = optimum(cost_matrix(t))
    return {"score": score_of(total, shift, max(t.shape)), "total": total, "shift": shift}


def check_map(D, partner, partner_dist2, total):
    """``partner`` [n] (index within the segment, -1: surplus) is one to one, its distances are D's and it attains ``total``"""
    D = np.asarray(D, np.float32)
    n, m = D.shape
    q = quantise(D)
    if q is None:
        assert total == -1 and np.all(partner == -1) and np.all(np.isposinf(partner_dist2))
        return
    _, t = q
    real = partner >= 0
    assert np.all(partner[real] < m) and len(set(partner[real].tolist())) == int(real.sum()) == min(n, m)
    assert np.array_equal(partner_dist2[real].view(np.uint32), D[np.nonzero(real)[0], partner[real]].view(np.uint32))
    assert np.array_equal(partner_dist2[~real].view(np.uint32), D[~real].min(axis=1).view(np.uint32)) if (~real).any() else True
    # the cost of the map: real pairs pay t, a surplus atom of either side its least t
    cost = int(t[np.nonzero(real)[0], partner[real]].sum()) + int(t[~real].min(axis=1).sum())
    left = np.setdiff1d(np.arange(m), partner[real])
    cost += int(t[:, left].min(axis=0).sum()) if len(left) else 0
    assert cost == total, (cost, total)


def rerank(short_segment, short_score, pair_score, k):
    """One structure's answer from its shortlist: the first k of (pairing score, segment) over the places that hold a segment.
    Returns the places [k] (-1: the tail)."""
    places = [p for p in range(len(short_segment)) if short_segment[p] >= 0]
    places.sort(key=lambda p: (float(pair_score[p]), int(short_segment[p])))
    return (places + [-1] * k)[:k]
