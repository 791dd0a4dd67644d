"""A plain NumPy restatement of the exact neighbour ranks (scann_index_ranks / scann_ranks_host, include/scann_hip.h) and of the map
scores on top of them (LatentIndex.map_quality), and the cases the host and the GPU tests share.  The distances go through
``_hip.knn_dist2_matrix`` (the chain of scann_knn_distsq); the ranking is one stable argsort per query -- positions ascending, so equal
distances stay in position order: the search's total order.  Nothing here is threaded, tiled, sorted by probe or binned."""
import numpy as np


def eligible(rows):
    return np.isfinite(rows).all(axis=1)


def ranks(rows, probe, qpos=None):
    """{"rank" int32 [nq, m], "dist2" fp32 [nq, m]} of the definition"""
    from scann import _hip

    rows = np.ascontiguousarray(rows, np.float32)
    probe = np.asarray(probe, np.int64)
    N = len(rows)
    q = np.arange(N) if qpos is None else np.asarray(qpos, np.int64)
    ok = eligible(rows)
    rank = np.full(probe.shape, -1, np.int32)
    dist2 = np.full(probe.shape, np.inf, np.float32)
    for n, i in enumerate(q):
        if not ok[i]:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            d = _hip.knn_dist2_matrix(rows[i:i + 1], rows)[0]                # fp32 [N], the query first
        others = np.flatnonzero(ok & (np.arange(N) != i))                    # positions ascending
        order = others[np.argsort(d[others], kind="stable")]                 # by (dist2, position)
        place = np.full(N, -1, np.int64)
        place[order] = np.arange(len(order))
        for p, j in enumerate(probe[n]):
            if j >= 0 and place[j] >= 0:
                rank[n, p], dist2[n, p] = place[j], d[j]
    return {"rank": rank, "dist2": dist2}


def same(got, want, what=""):
    assert got["rank"].dtype == np.int32 and got["rank"].tobytes() == np.asarray(want["rank"], np.int32).tobytes(), what + ": rank"
    if "dist2" in want and "dist2" in got:
        assert got["dist2"].dtype == np.float32 and got["dist2"].tobytes() == np.asarray(want["dist2"], np.float32).tobytes(), what + ": dist2"


def pathological_pool(N, dim, seed=0):
    """random rows with what goes wrong in one pool: from 65 rows on 40 coincident rows (more ties than probes, all settled by position),
    a row with a NaN, a row with an inf and two finite rows whose distance overflows to +inf; a small pool has a coincident pair"""
    rng = np.random.default_rng(1000 * N + dim + seed)
    rows = rng.standard_normal((N, dim)).astype(np.float32)
    if N >= 3:
        rows[2] = rows[0]
    if N >= 65:
        rows[20:60] = rows[20]
        rows[10, dim - 1] = np.nan
        rows[11, 0] = np.inf
        rows[61, 0] = np.float32(3e19)       # (3e19 + 3e19)^2 is above the largest fp32 number
        rows[62, 0] = np.float32(-3e19)
    return rows


def probe_lists(N, nq, m, seed=0, qpos=None):
    """int32 [nq, m]: random positions with -1, the query itself, ineligible rows (by position 10, 11 where the pool has them) and
    repeats among them; from 65 rows on some lists inside the coincident run"""
    rng = np.random.default_rng(seed * 7919 + N * 31 + m)
    q = np.arange(N) if qpos is None else np.asarray(qpos)
    probe = rng.integers(-1, N, (nq, m)).astype(np.int32)
    probe[::3, 0] = q[::3][:nq]                                  # the query itself
    if m >= 2:
        probe[1::4, m - 1] = probe[1::4, 0]                      # a repeat
    if N >= 65:
        probe[::5, m // 2] = 10 + (np.arange(len(probe[::5])) % 2)  # the rows with a NaN / an inf
        for r in range(2, nq, 11):
            probe[r] = rng.integers(20, 60, m)                   # thresholds equal in distance, differing in position only
    return probe


def all_others(N, i):
    """every position but i in chunks of 32, -1 behind the end: int32 [n_chunk, 32]"""
    others = np.delete(np.arange(N, dtype=np.int32), i)
    out = np.full(((len(others) + 31) // 32, 32), -1, np.int32)
    out.reshape(-1)[:len(others)] = others
    return out


def scores(rank_latent, rank_map, N, k):
    """(trustworthiness, continuity, neighbour overlap) at k in fp64, row by row, from the ranks [n, >= k]"""
    rl, rm = np.asarray(rank_latent, np.float64)[:, :k], np.asarray(rank_map, np.float64)[:, :k]
    coef = 2.0 / (k * (2.0 * N - 3.0 * k - 1.0))
    row_t = [1.0 - coef * sum(max(0.0, r + 1.0 - k) for r in row) for row in rl]
    row_c = [1.0 - coef * sum(max(0.0, r + 1.0 - k) for r in row) for row in rm]
    row_q = [sum(1.0 for r in row if r < k) / k for row in rl]
    return {"row_trustworthiness": np.array(row_t), "row_continuity": np.array(row_c), "row_overlap": np.array(row_q),
            "trustworthiness": float(np.mean(row_t)), "continuity": float(np.mean(row_c)), "neighbour_overlap": float(np.mean(row_q))}


def tie_free_rows(N, dim, lim, seed, base=None, jitter=None):
    """N integer-valued fp32 rows drawn one at a time, coordinates in +-lim (lim <= 1000, dim <= 3) -- or, with ``base`` [N, dim] and
    ``jitter``, row i = base[i] + integers in +-jitter.  A draw is rejected if it gives any existing row two equal squared distances or
    a zero distance, or has two equal distances itself.  Every squared distance is then an integer below 2^24: exact in fp32 and in fp64,
    and no row sees a tie, so any correct ordering is THE ordering."""
    assert dim <= 3 and lim <= 1000 and (jitter is None or lim + jitter <= 1400)
    rng = np.random.default_rng(seed)
    rows = np.zeros((N, dim), np.int64)
    D = np.zeros((N, N), np.int64)
    n = 0
    while n < N:
        r = rng.integers(-lim, lim + 1, dim) if base is None else np.asarray(base[n], np.int64) + rng.integers(-jitter, jitter + 1, dim)
        d = ((rows[:n] - r) ** 2).sum(axis=1)
        if (d == 0).any() or len(np.unique(d)) != n or (D[:n, :n] == d[:, None]).any():
            continue
        rows[n] = r
        D[n, :n] = D[:n, n] = d
        n += 1
    assert D.max() < 2 ** 24
    return rows.astype(np.float32)


def has_no_ties(rows):
    """no row of integer-valued ``rows`` has two equal squared distances, or a zero distance to another row"""
    x = np.asarray(rows, np.int64)
    D = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(D, -1)
    return all(len(np.unique(row)) == len(row) for row in D) and not (D == 0).any()
