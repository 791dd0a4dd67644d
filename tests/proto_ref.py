"""Reference of the prototypes and criticisms of a latent index (scann_index_prototypes / scann_index_criticisms and the twins
scann_prototypes_host / scann_criticisms_host, include/scann_hip.h), restated from the full term matrix in plain Python integers over a
given fp32 distance function ``dist2(a [na, dim], b [nb, dim]) -> [na, nb]`` and a given weight function ``weight(dist2 array, gamma)
-> fp32 array``: the prototype loop as defined, the criticism loop, the weights between them, the MMD curve, the MMD of two samples
as an exact rational, and a certificate that evaluates the greedy objective J(S + c) in fractions.Fraction for every candidate.  It
shares no code with the C twin.  The planted clusters of the tests are here as well."""
from fractions import Fraction

import numpy as np

import peaks_ref

ONE = 2 ** 30


def term_matrix(rows, dist2, weight, gamma):
    """t(i, j) as a list of lists of Python ints, and the eligibility of the rows"""
    rows = np.asarray(rows, np.float32)
    ok = peaks_ref.eligible(rows)
    if len(rows) == 0:
        return [], ok
    T = peaks_ref.terms(dist2(rows, rows), weight, gamma)
    return [[int(x) for x in r] for r in T], ok


def prototypes(rows, m, dist2, weight, gamma):
    """{"position", "score", "b_at_pick" (lists of the picks made), "A", "B" [N] Python ints, "n"}: the loop of the definition"""
    T, ok = term_matrix(rows, dist2, weight, gamma)
    N = len(T)
    el = [i for i in range(N) if ok[i]]
    n = len(el)
    A = [sum(T[i][j] for j in el) if ok[i] else -1 for i in range(N)]
    B = [0] * N
    picked, pos, score, bap = set(), [], [], []
    for s in range(m):
        best = None
        for i in el:  # positions ascending: a later row wins only with a strictly larger score
            if i in picked:
                continue
            sc = (s + 1) * A[i] - n * B[i]
            if best is None or sc > best[0]:
                best = (sc, i)
        if best is None:
            break
        sc, p = best
        pos.append(p), score.append(sc), bap.append(B[p])
        picked.add(p)
        for i in el:
            B[i] += T[i][p]
    return {"position": pos, "score": score, "b_at_pick": bap, "A": A, "B": B, "n": n, "T": T}


def objective(T, el, S):
    """J(S) = 2 / (n s) sum_{l in S} A_l - 1 / s^2 sum_{l, l' in S} t(l, l'), an exact rational (in units of 2^30)"""
    n, s = len(el), len(S)
    a = sum(sum(T[l][j] for j in el) for l in S)
    k = sum(T[l][l2] for l in S for l2 in S)
    return Fraction(2 * a, n * s) - Fraction(k, s * s)


def certificate(rows, position, dist2, weight, gamma):
    """every pick is the argmax of J(S + c) over the eligible rows c not picked before, ties to the lowest position"""
    T, ok = term_matrix(rows, dist2, weight, gamma)
    el = [i for i in range(len(T)) if ok[i]]
    S = []
    for p in [int(x) for x in position]:
        cand = [c for c in el if c not in S]
        assert p in cand, p
        J = {c: objective(T, el, S + [c]) for c in cand}
        top = max(J.values())
        assert J[p] == top and p == min(c for c in cand if J[c] == top), (len(S), p)
        S.append(p)


def weights(A, B, n_picks, witness="under"):
    """(W, weight) [N] Python ints: W_i = m' A_i - n B_i, max(W, 0) or |W| shifted right until the largest has 31 bits; 0 for an
    ineligible row"""
    n = sum(1 for a in A if a >= 0)
    W = [n_picks * a - n * b if a >= 0 else 0 for a, b in zip(A, B)]
    aw = [max(w, 0) if witness == "under" else abs(w) for w in W]
    shift = max(0, max(aw, default=0).bit_length() - 31)
    return W, [w >> shift for w in aw]


def criticisms(rows, weight_, exclude, c, dist2, weight, gamma):
    """{"position", "score"}: the criticism loop of the definition"""
    T, ok = term_matrix(rows, dist2, weight, gamma)
    N = len(T)
    live = [i for i in range(N) if ok[i] and i not in set(int(e) for e in exclude) and int(weight_[i]) > 0]
    cmax = [0] * N
    pos, score = [], []
    for _ in range(c):
        best = None
        for i in live:
            if i in pos:
                continue
            sc = int(weight_[i]) * (ONE - cmax[i])
            if best is None or sc > best[0]:
                best = (sc, i)
        if best is None or best[0] <= 0:
            break
        pos.append(best[1]), score.append(best[0])
        for i in live:
            cmax[i] = max(cmax[i], T[i][best[1]])
    return {"position": pos, "score": score}


def mmd_curve(T, el, position):
    """mmd2 between the eligible rows and the first s picks, s = 1 .. m', straight from the term matrix, as exact rationals"""
    n = len(el)
    total = sum(T[i][j] for i in el for j in el)
    out = []
    for s in range(1, len(position) + 1):
        S = position[:s]
        cross = sum(T[l][j] for l in S for j in el)
        kk = sum(T[l][l2] for l in S for l2 in S)
        out.append((Fraction(total, n * n) - Fraction(2 * cross, n * s) + Fraction(kk, s * s)) / ONE)
    return out


def mmd_two(a, b, dist2, weight, gamma):
    """the squared MMD of two samples of finite rows as an exact rational: every mean over all pairs, a row with itself included"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)

    def total(x, y):
        return sum(int(v) for v in peaks_ref.terms(dist2(x, y), weight, gamma).reshape(-1))

    na, nb = len(a), len(b)
    return (Fraction(total(a, a), na * na) + Fraction(total(b, b), nb * nb) - Fraction(2 * total(a, b), na * nb)) / ONE


PLANTED_SIZES = (600, 300, 100, 30)


def planted(seed, dim=16, spread=8.0):
    """Four Gaussian clusters of 600 / 300 / 100 / 30 rows of unit variance in ``dim`` columns, their centres ``spread`` apart along
    four axes, shuffled: (rows fp32 [1030, dim], planted label [1030])"""
    rng = np.random.default_rng(seed)
    centres = np.zeros((4, dim), np.float32)
    for c in range(4):
        centres[c, c] = spread
    label = np.repeat(np.arange(4), PLANTED_SIZES)
    rows = centres[label] + rng.standard_normal((len(label), dim)).astype(np.float32)
    perm = rng.permutation(len(label))
    return np.ascontiguousarray(rows[perm], dtype=np.float32), label[perm]
