"""Reference of the radius search over a latent-space index (scann_index_within, scann_index_within_rows, scann_within_host;
include/scann_hip.h), restated in plain NumPy from the header's text: the hits of a query are the rows with dist2 <= radius2 (fp32,
inclusive; a NaN never qualifies, +inf only at radius2 = +inf), minus the rows of the query's id, the query's own position and, with
``upper``, the positions at or below it; they are listed by (dist2, position).  The distance matrix is the fp32 chain the caller passes
in, as for tests/knn_ref.py, whose order this is.  The pruned plan runs over a partition as tests/cells_ref.py lays it out, with
cells_ref.bound.  It shares no code with the C side."""
import numpy as np

import cells_ref

TILE = cells_ref.TILE
GROUP = cells_ref.GROUP
PASS = cells_ref.PASS


def hit_mask(dist2, radius2, ids=None, query_ids=None, query_pos=None, upper=0, positions=None):
    """bool [nq, n]: which (query, row) pairs are hits; ``positions`` [n]: the rows' positions in the index (default 0 .. n - 1)"""
    d = np.asarray(dist2, np.float32)
    nq, n = d.shape
    pos = np.arange(n) if positions is None else np.asarray(positions)
    with np.errstate(invalid="ignore"):
        ok = d <= np.float32(radius2)  # (a comparison with NaN is false)
    if query_ids is not None:
        row_ids = pos.astype(np.int64) if ids is None else np.asarray(ids, np.int64)[pos]
        ok &= row_ids[None, :] != np.asarray(query_ids, np.int64)[:, None]
    if query_pos is not None:
        qp = np.asarray(query_pos)[:, None]
        ok &= (pos[None, :] > qp) if upper else (pos[None, :] != qp)
    return ok


def _assemble(lists, nq):
    """per query a list of (dist2, position) -> the result dict, every query's entries in the total order"""
    count = np.array([len(l) for l in lists], np.int64).reshape(nq)
    first = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    d, p = [], []
    for l in lists:
        if len(l):
            a = np.array([x[0] for x in l], np.float32)
            b = np.array([x[1] for x in l], np.int64)
            order = np.lexsort((b, a))  # last key first: dist2, then position
            d.append(a[order])
            p.append(b[order])
    return {"count": count, "first": first, "total": int(first[-1]),
            "dist2": np.concatenate(d).astype(np.float32) if d else np.zeros(0, np.float32),
            "position": np.concatenate(p).astype(np.int32) if p else np.zeros(0, np.int32)}


def within(dist2, radius2, ids=None, query_ids=None, query_pos=None, upper=0):
    """The definition over the full matrix: {"count" [nq], "first" [nq + 1], "total", "dist2", "position" [total]}"""
    d = np.asarray(dist2, np.float32)
    ok = hit_mask(d, radius2, ids, query_ids, query_pos, upper)
    return _assemble([[(d[i, r], int(r)) for r in np.nonzero(ok[i])[0]] for i in range(d.shape[0])], d.shape[0])


def same(got, want, label="", entries=True):
    """two results equal in every byte"""
    assert np.array_equal(np.asarray(got["count"], np.int64), want["count"]), (label, "count")
    assert np.array_equal(np.asarray(got["first"], np.int64), want["first"]), (label, "first")
    if entries:
        assert np.array_equal(np.asarray(got["position"], np.int32), want["position"]), (label, "position")
        g, w = np.ascontiguousarray(got["dist2"], np.float32), want["dist2"]
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)), (label, "dist2")


def pruned(rows, part, q, radius2, dist2, ids=None, query_ids=None, query_pos=None, upper=0, bound_fn=cells_ref.bound):
    """The pruned route over a host partition ``part`` of ``rows``: -> (result, stats {"total", "seeds", "visited", "groups"}).  Queries
    go in passes of 1024, ordered by (nearest centre, distance to it, place) and cut into groups of 128; a (group, tile) pair is skipped
    iff the bound exceeds radius2, strictly, for every query of the group; loose tiles are always visited, pad entries never qualify.
    (The library orders a pass by a walk through the centres instead of by their numbers: only the groups, hence the stats, can differ.)"""
    rows, q = np.asarray(rows, np.float32), np.asarray(q, np.float32)
    n, nq = len(rows), len(q)
    C, T, first, perm = part["cells"], part["tiles"], part["first_tile"], part["perm"]
    tile_cell = np.full(T, -1)
    for c in range(C):
        tile_cell[first[c]:first[c + 1]] = c
    lists = [[] for _ in range(nq)]
    stats = {"total": 0, "seeds": 0, "visited": 0, "groups": 0}
    for q0 in range(0, nq, PASS):
        idx = np.arange(q0, min(nq, q0 + PASS))
        with np.errstate(all="ignore"):
            D = np.asarray(dist2(q[idx], part["centre"]), np.float32) if C else np.zeros((len(idx), 0), np.float32)
        if C:
            valid = ~np.isnan(D)
            near = np.where(valid, D, np.float32(np.inf)).argmin(axis=1)
            near = np.where(np.isposinf(np.where(valid, D, np.float32(np.inf))[np.arange(len(idx)), near]), valid.argmax(axis=1), near)
            near = np.where(valid.any(axis=1), near, -1)
        else:
            near = np.full(len(idx), -1)
        near_d = np.array([D[i, c] if c >= 0 else np.inf for i, c in enumerate(near)], np.float32)
        order = np.lexsort((np.arange(len(idx)), np.where(near < 0, np.float32(0), near_d), np.where(near < 0, C, near)))
        for g0 in range(0, len(idx), GROUP):
            local = order[g0:g0 + GROUP]
            members = idx[local]
            visited = 0
            for t in range(T):
                if tile_cell[t] >= 0 and np.all(bound_fn(D[local, tile_cell[t]], part["lo"][t], part["hi"][t]) > np.float64(np.float32(radius2))):
                    continue
                visited += 1
                p = perm[t * TILE:(t + 1) * TILE]
                p = p[p >= 0]
                with np.errstate(all="ignore"):
                    d = np.asarray(dist2(q[members], rows[p]), np.float32)
                ok = hit_mask(d, radius2, ids, None if query_ids is None else np.asarray(query_ids)[members],
                              None if query_pos is None else np.asarray(query_pos)[members], upper, positions=p)
                for a, b in zip(*np.nonzero(ok)):
                    lists[members[a]].append((d[a, b], int(p[b])))
            stats["total"] += (n + TILE - 1) // TILE
            stats["visited"] += visited
            stats["groups"] += 1
    return _assemble(lists, nq), stats


def groups_of(i, j, n_rows):
    """the least position of every row's connected component under the pairs (i, j): a plain union-find"""
    parent = list(range(n_rows))

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        ra, rb = root(a), root(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([root(x) for x in range(n_rows)], np.int32)
