"""Reference of the density-peak clustering and the kernel density of a latent index (scann_index_density / scann_index_peaks and the
twins scann_density_host / scann_peaks_host, include/scann_hip.h), restated in plain NumPy and Python integers over a given fp32 distance
function ``dist2(a [na, dim], b [nb, dim]) -> [na, nb]`` and a given weight function ``weight(dist2 array, gamma) -> fp32 array``: the
terms, the sums, the "above" order, the parents, the host assembly, and a certificate of a result from the full matrices.  It shares no
code with the C twin.  The two planted data sets of the tests are here as well."""
import math

import numpy as np


def eligible(rows):
    rows = np.asarray(rows, np.float32)
    return np.isfinite(rows).all(axis=1) if len(rows) else np.zeros(0, bool)


def terms(D, weight, gamma):
    """t = round-to-nearest-even(2^30 w) per pair as Python-sized integers (int64 array); a NaN distance contributes nothing"""
    D = np.asarray(D, np.float32)
    w = np.asarray(weight(D, np.float32(gamma)), np.float32).astype(np.float64)
    t = np.rint(np.ldexp(np.where(np.isnan(D), 0.0, w), 30))  # exact in fp64; rint rounds half to even
    assert ((t >= 0) & (t <= 2 ** 30)).all()
    return t.astype(np.int64)


def density(rows, q, dist2, weight, gamma, skip=None):
    """S of every query: a list of Python ints; -1 for an ineligible query"""
    rows, q = np.asarray(rows, np.float32), np.asarray(q, np.float32)
    if len(q) == 0:
        return []
    T = terms(dist2(q, rows), weight, gamma) if len(rows) else np.zeros((len(q), 0), np.int64)
    ok = eligible(q)
    out = []
    for i in range(len(q)):
        if not ok[i]:
            out.append(-1)
            continue
        s = 0
        for j in range(len(rows)):
            if skip is not None and skip[i] >= 0 and j == skip[i]:
                continue
            s += int(T[i, j])
        out.append(s)
    return out


def above(sj, j, si, i):
    return sj > si or (sj == si and j < i)


def peaks(rows, dist2, weight, gamma):
    """(sums [N] Python ints, parent [N], delta2 [N] fp32, D [N, N]) of the self-join"""
    rows = np.asarray(rows, np.float32)
    N = len(rows)
    ok = eligible(rows)
    D = dist2(rows, rows) if N else np.zeros((0, 0), np.float32)
    T = terms(D, weight, gamma) if N else np.zeros((0, 0), np.int64)
    sums = [sum(int(T[i, j]) for j in range(N) if j != i and ok[j]) if ok[i] else -1 for i in range(N)]
    parent, delta2 = [-1] * N, [np.float32(np.inf)] * N
    for i in range(N):
        if not ok[i]:
            continue
        best = None
        for j in range(N):  # positions ascending: a later row wins only if strictly nearer
            if not ok[j] or not above(sums[j], j, sums[i], i) or np.isnan(D[i, j]):
                continue
            if best is None or D[i, j] < D[i, best]:
                best = j
        if best is not None:
            parent[i], delta2[i] = best, D[i, best]
    return sums, np.array(parent, np.int32), np.array(delta2, np.float32), D


def certificate(rows, sums, parent, delta2, dist2):
    """A result checked from the full distance matrix without repeating the search: no row above i is nearer than parent_i, and none
    equally near lies at a lower position; exactly one eligible row has no parent, and nothing is above it; the parents ascend the
    density order (so they form a tree); ineligible rows carry (-1, -1, +inf)."""
    rows = np.asarray(rows, np.float32)
    N = len(rows)
    ok = eligible(rows)
    D = dist2(rows, rows) if N else np.zeros((0, 0), np.float32)
    assert np.array_equal(D.view(np.uint32), D.T.view(np.uint32)) or np.isnan(D).any(), "dist2 is not symmetric"
    sums = [int(s) for s in sums]
    roots = 0
    for i in range(N):
        if not ok[i]:
            assert sums[i] == -1 and parent[i] == -1 and delta2[i] == np.inf, i
            continue
        assert sums[i] >= 0, i
        ups = [j for j in range(N) if ok[j] and above(sums[j], j, sums[i], i) and not np.isnan(D[i, j])]
        p = int(parent[i])
        if p < 0:
            roots += 1
            assert not ups and delta2[i] == np.inf, i
            continue
        assert p in ups and np.float32(delta2[i]).view(np.uint32) == D[i, p].view(np.uint32), i
        for j in ups:
            assert D[i, j] > D[i, p] or (D[i, j] == D[i, p] and j >= p), (i, j, p)
    assert roots == (1 if ok.any() else 0)


def assemble(sums, parent, delta2, k=None, min_density=None, min_delta=None):
    """The host half restated row by row: {"label", "density", "delta", "g", "centre_position", "size", "decision"}"""
    N = len(sums)
    sums = [int(s) for s in sums]
    el = [i for i in range(N) if sums[i] >= 0]
    n_el = len(el)
    dens = [math.ldexp(sums[i], -30) / n_el if sums[i] >= 0 else float("nan") for i in range(N)]
    delta = [math.sqrt(float(delta2[i])) if sums[i] >= 0 else float("inf") for i in range(N)]
    g = {}
    for i in el:
        g[i] = float("inf") if parent[i] < 0 else 0.0 if sums[i] == 0 else math.ldexp(sums[i], -30) * delta[i]  # (never 0 * inf)
    order = sorted(el, key=lambda i: (-sums[i], i))
    by_g = sorted(el, key=lambda i: (-g[i], i))
    if k is not None:
        centres = set(by_g[:k])
    else:
        centres = {i for i in el if parent[i] < 0 or (dens[i] >= min_density and delta[i] >= min_delta)}
    cpos = [i for i in order if i in centres]
    number = {c: n for n, c in enumerate(cpos)}
    label = [-1] * N
    for i in order:
        label[i] = number[i] if i in centres else label[parent[i]]
    size = [sum(1 for x in label if x == n) for n in range(len(cpos))]
    return {"label": np.array(label, np.int32), "density": np.array(dens, np.float64), "delta": np.array(delta, np.float64),
            "centre_position": np.array(cpos, np.int32), "size": np.array(size, np.int64), "decision": np.array([g[i] for i in by_g], np.float64)}


def small_integer_rows(n, dim, seed, lo=-3, hi=4):
    """rows whose differences, squares and partial sums are small integers: plain fp32 squares and sums are the chain's bits"""
    return np.random.default_rng(seed).integers(lo, hi, size=(n, dim)).astype(np.float32)


BLOB_SIZES = (300, 120, 60)


def blobs(seed):
    """Three planted blobs of 300 / 120 / 60 rows in 3 of 128 columns, shuffled: (rows fp32 [480, 128], planted label [480])"""
    rng = np.random.default_rng(seed)
    centres = np.zeros((3, 128), np.float32)
    centres[0, 5], centres[1, 40], centres[2, 99] = 12.0, 12.0, 12.0
    label = np.repeat(np.arange(3), BLOB_SIZES)
    rows = centres[label]
    rows[:, [5, 40, 99]] += rng.standard_normal((len(label), 3)).astype(np.float32)
    perm = rng.permutation(len(label))
    return np.ascontiguousarray(rows[perm], dtype=np.float32), label[perm]


CRESCENT_RADIUS = 24.0


def crescents(seed, n=800, dim=16):
    """Two interleaved crescents in the first two of ``dim`` columns, Gaussian noise of standard deviation 1.0 on every column, the
    coordinates rounded to integers (so that plain fp32 arithmetic gives the chain's bits), shuffled: (rows fp32 [n, dim], label [n])"""
    rng = np.random.default_rng(seed)
    half = n // 2
    t = rng.uniform(0.0, np.pi, n)
    label = np.repeat(np.arange(2), (half, n - half))
    x = np.where(label == 0, np.cos(t), 1.0 - np.cos(t)) * CRESCENT_RADIUS
    y = np.where(label == 0, np.sin(t), 0.5 - np.sin(t)) * CRESCENT_RADIUS
    rows = rng.standard_normal((n, dim))
    rows[:, 0] += x
    rows[:, 1] += y
    perm = rng.permutation(n)
    return np.ascontiguousarray(np.rint(rows[perm]), dtype=np.float32), label[perm]


def matches(label, planted):
    """the share of rows whose label maps one-to-one onto the planted one under the best assignment of a 2- or 3-cluster labelling"""
    import itertools

    label, planted = np.asarray(label), np.asarray(planted)
    k = int(planted.max()) + 1
    return max(float(np.mean(np.array(perm)[np.clip(label, 0, k - 1)] == planted) if (label >= 0).all() and label.max() < k else 0.0)
               for perm in itertools.permutations(range(k)))
