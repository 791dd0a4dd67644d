"""Reference of the hierarchical clustering of a latent index (scann_index_mst and the twin scann_mst_host, include/scann_hip.h;
LatentHierarchy), restated in plain NumPy and Python over a given fp32 distance function ``dist2(a [na, dim], b [nb, dim]) -> [na, nb]``:
the weight, the edge order, the tree as Kruskal's algorithm over all pairs and again as Boruvka rounds with the per-row rule, the core
distances, the cuts, and the condensed tree with its excess-of-mass selection, top-down on sets of rows.  It shares no code with the C
twin or with ``scann.models.latent_index``.  The planted data sets of the tests are here as well."""
import math

import numpy as np

import peaks_ref


def eligible(rows):
    rows = np.asarray(rows, np.float32)
    return np.isfinite(rows).all(axis=1) if len(rows) else np.zeros(0, bool)


def weights(rows, core2, dist2):
    """W [N, N] fp32: max(dist2, core2_i, core2_j)"""
    rows = np.asarray(rows, np.float32)
    N = len(rows)
    W = dist2(rows, rows) if N else np.zeros((0, 0), np.float32)
    if core2 is not None:
        c = np.asarray(core2, np.float32)
        W = np.maximum(np.maximum(W, c[:, None]), c[None, :])
    return W.astype(np.float32)


def kruskal(rows, core2, dist2):
    """(a, b, w): the minimum spanning tree over the eligible rows under the edge order (w, min, max), its edges in that order"""
    rows = np.asarray(rows, np.float32)
    ok = np.flatnonzero(eligible(rows))
    W = weights(rows, core2, dist2)
    i, j = np.triu_indices(len(ok), 1)
    i, j = ok[i], ok[j]
    w = W[i, j]
    assert not np.isnan(w).any()
    order = np.lexsort((j, i, w))
    up = list(range(len(rows)))

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x

    a, b, ww = [], [], []
    for e in order.tolist():
        if len(a) == len(ok) - 1:
            break
        x, y = find(int(i[e])), find(int(j[e]))
        if x != y:
            up[x] = y
            a.append(int(i[e])), b.append(int(j[e])), ww.append(w[e])
    assert len(a) == max(len(ok) - 1, 0)
    return np.array(a, np.int32), np.array(b, np.int32), np.array(ww, np.float32)


def before(e, f):
    """edge e = (w, lo, hi) comes before f"""
    return e[0] < f[0] or (e[0] == f[0] and (e[1], e[2]) < (f[1], f[2]))


def boruvka(rows, core2, dist2):
    """(a, b, w, rounds): the same tree by Boruvka rounds as the device runs them -- per row the first row of another component under
    (w, position), positions ascending and only a strictly smaller weight replacing the incumbent; per component the first of its rows'
    edges under (w, min, max); an edge picked from both sides is taken once"""
    rows = np.asarray(rows, np.float32)
    N = len(rows)
    ok = eligible(rows)
    W = weights(rows, core2, dist2)
    comp = [i if ok[i] else -1 for i in range(N)]
    edges, rounds = [], 0
    while len({c for c in comp if c >= 0}) > 1:
        rounds += 1
        pick = {}
        for q in range(N):
            if comp[q] < 0:
                continue
            best = None
            for r in range(N):
                if comp[r] < 0 or comp[r] == comp[q]:
                    continue
                if best is None or W[q, r] < W[q, best]:
                    best = r
            e = (W[q, best], min(q, best), max(q, best))
            if comp[q] not in pick or before(e, pick[comp[q]]):
                pick[comp[q]] = e
        new = set(pick.values())
        edges += sorted(new, key=lambda e: (e[1], e[2]))
        up = {c: c for c in pick}

        def find(x):
            while up[x] != x:
                x = up[x]
            return x

        for _, lo, hi in new:
            x, y = find(comp[lo]), find(comp[hi])
            assert x != y, "the picked edges close a cycle"
            up[max(x, y)] = min(x, y)
        comp = [find(c) if c >= 0 else -1 for c in comp]
    edges.sort(key=lambda e: (e[0], e[1], e[2]))
    return (np.array([e[1] for e in edges], np.int32), np.array([e[2] for e in edges], np.int32), np.array([e[0] for e in edges], np.float32),
            rounds)


def core2(rows, min_samples, dist2):
    """dist2 to the min_samples-th nearest other eligible row under (dist2, position); the farthest where there are fewer (at most 31
    are looked at), 0 for a row alone and for ineligible rows"""
    rows = np.asarray(rows, np.float32)
    ok = eligible(rows)
    D = dist2(rows, rows)
    out = np.zeros(len(rows), np.float32)
    for i in np.flatnonzero(ok):
        others = [j for j in np.flatnonzero(ok) if j != i]
        if others:
            d = sorted(D[i, j] for j in others)[:31]
            out[i] = d[min(min_samples, len(d)) - 1]
    return out


def number_by_least_member(sets, n_rows):
    """label [n_rows] of disjoint sets of rows, numbered by their least member; -1 elsewhere"""
    label = np.full(n_rows, -1, np.int32)
    for k, s in enumerate(sorted(sets, key=min)):
        label[sorted(s)] = k
    return label


def split(vertices, edge_ids, a, b):
    """a subtree (its vertices, its edges as ascending indices) without its last edge: ((vertices, edges) of the side of a[last], of b[last])"""
    last, rest = edge_ids[-1], edge_ids[:-1]
    adj = {v: [] for v in vertices}
    for e in rest:
        adj[a[e]].append(b[e]), adj[b[e]].append(a[e])
    seen, todo = {a[last]}, [a[last]]
    while todo:
        for y in adj[todo.pop()]:
            if y not in seen:
                seen.add(y), todo.append(y)
    return (seen, [e for e in rest if a[e] in seen]), (vertices - seen, [e for e in rest if a[e] not in seen])


def cut(a, b, w, n_rows, height=None, k=None):
    """the flat clustering after the merges at sqrt(w) <= height, or after the first n - k merges"""
    a, b = [int(x) for x in a], [int(x) for x in b]
    rows = sorted(set(a) | set(b))
    n_merge = len(rows) - k if k is not None else sum(1 for x in w if math.sqrt(float(x)) <= height)
    sets = {v: {v} for v in rows}
    for e in range(n_merge):
        s = sets[a[e]] | sets[b[e]]
        for v in s:
            sets[v] = s
    return number_by_least_member({frozenset(s) for s in sets.values()}, n_rows)


def clusters(a, b, w, n_rows, min_cluster_size):
    """The condensed tree and the excess-of-mass selection restated top-down on sets of rows: {"label", "probability", "persistence",
    "birth2", "exemplar"}"""
    a, b = [int(x) for x in a], [int(x) for x in b]
    w = [np.float32(x) for x in w]
    out = {"label": np.full(n_rows, -1, np.int32), "probability": np.zeros(n_rows), "persistence": np.zeros(0), "birth2": np.zeros(0, np.float32),
           "exemplar": np.zeros(0, np.int32)}
    if not a:
        return out
    positive = [1.0 / math.sqrt(float(x)) for x in w if x > 0]
    zero_lambda = max(positive) if positive else 1.0
    lam = [zero_lambda if x == 0 else 1.0 / math.sqrt(float(x)) for x in w]
    cl = [{"parent": None, "birth": 0.0, "birth2": np.float32(np.inf), "leave": {}, "children": []}]
    work = [((set(a) | set(b)), list(range(len(a))), 0)]
    while work:
        vertices, edge_ids, c = work.pop()
        e = edge_ids[-1]
        sides = split(vertices, edge_ids, a, b)
        if all(len(s[0]) >= min_cluster_size for s in sides):
            for s in sides:
                cl.append({"parent": c, "birth": lam[e], "birth2": w[e], "leave": {}, "children": [], "size": len(s[0])})
                cl[c]["children"].append(len(cl) - 1)
                work.append((s[0], s[1], len(cl) - 1))
            continue
        for s in sides:
            if len(s[0]) >= min_cluster_size:
                work.append((s[0], s[1], c))
            else:
                for v in s[0]:
                    cl[c]["leave"][v] = lam[e]

    def stability(c):
        return (sum(x - cl[c]["birth"] for x in cl[c]["leave"].values())
                + sum(cl[k]["size"] * (cl[k]["birth"] - cl[c]["birth"]) for k in cl[c]["children"]))

    def select(c):  # (total, the selected clusters at or below c)
        below = [select(k) for k in cl[c]["children"]]
        total = sum(t for t, _ in below)
        if c != 0 and stability(c) >= total:
            return stability(c), [c]
        return total, [x for _, s in below for x in s]

    def members(c):  # row -> lambda_leave over c and everything below it
        m = dict(cl[c]["leave"])
        for k in cl[c]["children"]:
            m.update(members(k))
        return m

    chosen = sorted(select(0)[1], key=lambda c: min(members(c)))
    for k, c in enumerate(chosen):
        m = members(c)
        top = max(m.values())
        for v, x in m.items():
            out["label"][v] = k
            out["probability"][v] = min(x / top, 1.0) if top > 0 else 1.0
    out["persistence"] = np.array([stability(c) for c in chosen])
    out["birth2"] = np.array([cl[c]["birth2"] for c in chosen], np.float32)
    out["exemplar"] = np.array([min(v for v, x in members(c).items() if x == max(members(c).values())) for c in chosen], np.int32)
    return out


def lattice_rows(n, seed, side=4):
    """integer-lattice rows in 3 columns: ties everywhere, coincident rows among them"""
    return np.random.default_rng(seed).integers(0, side, size=(n, 3)).astype(np.float32)


N_OUTLIERS = 80


def crescents_with_outliers(seed=0):
    """``peaks_ref.crescents(seed)`` (800 integer rows, 16 columns) plus 80 outliers, uniform integers in -60 .. 89 on every column,
    shuffled among them: (rows fp32 [880, 16], planted label [880], -1 for an outlier)"""
    rows, label = peaks_ref.crescents(seed)
    rng = np.random.default_rng(seed + 1000)
    out = rng.integers(-60, 90, size=(N_OUTLIERS, rows.shape[1])).astype(np.float32)
    perm = rng.permutation(len(rows) + N_OUTLIERS)
    return (np.ascontiguousarray(np.concatenate([rows, out])[perm], dtype=np.float32),
            np.concatenate([label, np.full(N_OUTLIERS, -1)])[perm])


def unequal_blobs(seed=0):
    """Three blobs of 300 / 300 / 100 rows, standard deviations 1, 3 and 0.5, centres 40 apart, in 8 columns, shuffled"""
    rng = np.random.default_rng(seed)
    sizes, sigma = (300, 300, 100), (1.0, 3.0, 0.5)
    centres = np.zeros((3, 8))
    centres[0, 0] = centres[1, 1] = centres[2, 2] = 40.0 / math.sqrt(2.0)  # 40 between any two
    label = np.repeat(np.arange(3), sizes)
    rows = centres[label] + rng.standard_normal((len(label), 8)) * np.asarray(sigma)[label][:, None]
    perm = rng.permutation(len(label))
    return np.ascontiguousarray(rows[perm], dtype=np.float32), label[perm]


def same_partition(x, y):
    """two labellings name the same partition (noise -1 included as a class of its own)"""
    x, y = np.asarray(x), np.asarray(y)
    pairs = set(zip(x.tolist(), y.tolist()))
    return len(pairs) == len(set(x.tolist())) == len(set(y.tolist())) and all((p == -1) == (q == -1) for p, q in pairs)
