"""Reference of an index's partition into cells and of the nearest-row search that skips cells out of reach (scann_index_partition,
scann_cells_host, scann_cell_bound; include/scann_hip.h), restated in plain NumPy: the bound in fp64, the layout from the references of
the selection and of k-means (tests/kcenter_ref.py, tests/kmeans_ref.py) by a lexsort, the padding and the shells, and the pruned search
itself -- groups of 128 queries, seeds, the survivor rule -- over a host partition.  It shares no code with the C side."""
import numpy as np

import kcenter_ref
import kmeans_ref

EPS = 2.0 ** -12
ABS = 2.0 ** -64
TILE = 64
GROUP = 128
PASS = 1024


def bound(D, lo, hi):
    """lb of the header, elementwise over broadcast fp32 arrays, in fp64"""
    D, lo, hi = np.broadcast_arrays(np.asarray(D, np.float32), np.asarray(lo, np.float32), np.asarray(hi, np.float32))
    with np.errstate(all="ignore"):
        a, r_lo, r_hi = np.sqrt(D.astype(np.float64)), np.sqrt(lo.astype(np.float64)), np.sqrt(hi.astype(np.float64))
        g = np.maximum((1.0 - EPS) * a - (1.0 + EPS) * r_hi, (1.0 - EPS) * r_lo - (1.0 + EPS) * a) - ABS
        lb = np.where(g > 0, (1.0 - EPS) * (g * g), 0.0)
    return np.where(np.isfinite(D) & np.isfinite(hi), lb, 0.0)


def partition(rows, cells, max_iter, dist2):
    """The definition: -> {"cells", "tiles", "pad", "largest", "centre", "perm", "first_tile", "lo", "hi"} as ``_hip.cells_host`` gives them"""
    rows = np.asarray(rows, np.float32)
    n = len(rows)
    pos, _, C = kcenter_ref.select(rows, None, min(cells, n), 0.0, dist2)
    label, d2 = np.full(n, -1, np.int32), np.full(n, np.inf, np.float32)
    centre = np.zeros((0, rows.shape[1]), np.float32)
    if C:
        km = kmeans_ref.kmeans(rows, rows[pos[:C]], max_iter, 0, dist2)
        label, d2, centre = km["label"], km["dist2"], km["centre"]
    cell = np.where(label < 0, C, label)
    order = np.lexsort((np.arange(n), np.where(label < 0, np.float32(0), d2), cell))  # last key first: cell, dist2, position
    perm, first, lo, hi = [], [], [], []
    for c in range(C + 1):
        first.append(len(perm) // TILE)
        mine = order[cell[order] == c]
        for t0 in range(0, len(mine), TILE):
            t = mine[t0:t0 + TILE]
            perm.extend(list(t) + [-1] * (TILE - len(t)))
            lo.append(d2[t[0]] if c < C else np.float32(0))
            hi.append(d2[t[-1]] if c < C else np.float32(np.inf))
    first.append(len(perm) // TILE)
    size = np.bincount(label[label >= 0], minlength=max(C, 1))
    return {"cells": C, "tiles": len(lo), "pad": len(perm) - n, "largest": int(size.max()) if C else 0, "centre": np.asarray(centre, np.float32),
            "perm": np.asarray(perm, np.int32), "first_tile": np.asarray(first, np.int32), "lo": np.asarray(lo, np.float32),
            "hi": np.asarray(hi, np.float32)}


def same(got, want, label=""):
    """two partitions equal in every byte"""
    for key in ("cells", "tiles", "pad", "largest"):
        assert got[key] == want[key], (label, key, got[key], want[key])
    for key in ("perm", "first_tile"):
        assert np.array_equal(got[key], want[key]), (label, key)
    for key in ("centre", "lo", "hi"):
        assert got[key].shape == want[key].shape and np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), (label, key)


def before(d, p, e, q):
    return d < e or (d == e and p < q)


def pruned_search(rows, part, q, k, dist2, ids=None, query_ids=None, bound_fn=bound):
    """The pruned search over a host partition ``part`` of ``rows``: -> (dist2 [nq, k], position [nq, k], stats {"total", "seeds",
    "visited", "groups"}).  Queries go in passes of 1024, ordered by (nearest centre, distance to it, place) and cut into groups of 128.
    A query's seed is, within its nearest cell, the tile of least bound (a tile of 64 real rows before a partial one, then the earlier
    tile); the group visits the union of its seeds, which gives tau_q -- the k-th qualifying distance, +inf with fewer --; then every
    loose tile and every other tile with bound <= tau_q for some q of the group, where distances above tau_q are dropped."""
    rows, q = np.asarray(rows, np.float32), np.asarray(q, np.float32)
    n, nq = len(rows), len(q)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    C, T, first, perm = part["cells"], part["tiles"], part["first_tile"], part["perm"]
    tile_cell = np.full(T, -1)
    for c in range(C):
        tile_cell[first[c]:first[c + 1]] = c
    full = perm.reshape(T, TILE)[:, -1] >= 0 if T else np.zeros(0, bool)
    od, op = np.full((nq, k), np.inf, np.float32), np.full((nq, k), -1, np.int32)
    stats = {"total": 0, "seeds": 0, "visited": 0, "groups": 0}
    full_tiles = (n + TILE - 1) // TILE

    def visit(tiles, members, lists, tau):
        for t in tiles:
            p = perm[t * TILE:(t + 1) * TILE]
            p = p[p >= 0]
            with np.errstate(all="ignore"):
                d = np.asarray(dist2(q[members], rows[p]), np.float32)
                ok = ~np.isnan(d) & ~(d > tau[:, None])  # a NaN never qualifies; above tau: dropped, equal: kept
            if query_ids is not None:
                ok &= ids[p][None, :] != np.asarray(query_ids)[members][:, None]
            for a, b in zip(*np.nonzero(ok)):
                lists[a].append((d[a, b], int(p[b])))

    for q0 in range(0, nq, PASS):
        idx = np.arange(q0, min(nq, q0 + PASS))
        with np.errstate(all="ignore"):
            D = np.asarray(dist2(q[idx], part["centre"]), np.float32) if C else np.zeros((len(idx), 0), np.float32)
        key = np.where(np.isnan(D), np.float32(np.inf), D)
        near = key.argmin(axis=1) if C else np.zeros(len(idx), np.int64)
        if C:  # the first centre that is no NaN where the least is +inf; none: -1
            at_inf = np.isposinf(key[np.arange(len(idx)), near])
            near = np.where(at_inf, (~np.isnan(D)).argmax(axis=1), near)
            near = np.where((~np.isnan(D)).any(axis=1), near, -1)
        else:
            near = np.full(len(idx), -1)
        near_d = np.array([D[i, c] if c >= 0 else np.inf for i, c in enumerate(near)], np.float32)
        order = np.lexsort((np.arange(len(idx)), np.where(near < 0, np.float32(0), near_d), np.where(near < 0, C, near)))
        for g0 in range(0, len(idx), GROUP):
            local = order[g0:g0 + GROUP]  # places within the pass
            members = idx[local]
            seeds = set()
            for i in local:
                c = near[i]
                if c < 0:
                    continue
                ts = np.arange(first[c], first[c + 1])
                if len(ts) == 0:
                    continue
                b = bound_fn(near_d[i], part["lo"][ts], part["hi"][ts])
                best = np.lexsort((ts, ~full[ts], b))[0]
                seeds.add(int(ts[best]))
            lists = [[] for _ in members]
            visit(sorted(seeds), members, lists, np.full(len(members), np.inf, np.float32))
            tau = np.array([sorted(l)[k - 1][0] if len(l) >= k else np.inf for l in lists], np.float32)
            survivors = []
            for t in range(T):
                if t in seeds:
                    continue
                if tile_cell[t] < 0:
                    survivors.append(t)
                    continue
                b = bound_fn(D[local, tile_cell[t]], part["lo"][t], part["hi"][t])
                if not np.all(b > tau.astype(np.float64)):
                    survivors.append(t)
            visit(survivors, members, lists, tau)
            for a, i in enumerate(members):
                best = sorted(lists[a])[:k]
                for j, (v, pp) in enumerate(best):
                    od[i, j], op[i, j] = v, pp
            stats["total"] += full_tiles
            stats["seeds"] += len(seeds)
            stats["visited"] += len(seeds) + len(survivors)
            stats["groups"] += 1
    return od, op, stats
