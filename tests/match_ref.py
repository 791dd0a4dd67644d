"""Reference of the structure matching (scann_index_match, include/scann_hip.h) in NumPy, given a matrix of squared distances between
the query rows and the index rows: the segments of an id sequence, the parts of every (query set, segment) pair, the three scores, the
selection under the total order (score ascending, segment ascending) with ids and exclusion, and the witnesses."""
import numpy as np

MEASURES = {"chamfer": 0, "hausdorff": 1, "cover": 2}


def segments(ids):
    """(first int64, count int32, id int64) of the maximal runs of consecutive equal ids, in position order"""
    ids = np.asarray(ids, dtype=np.int64)
    if len(ids) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64)
    first = np.concatenate([[0], np.nonzero(ids[1:] != ids[:-1])[0] + 1]).astype(np.int64)
    count = np.diff(np.concatenate([first, [len(ids)]])).astype(np.int32)
    return first, count, ids[first]


def nanmin_with_witness(d):
    """min of a vector over its entries that are not NaN and the least index that attains it; (+inf, -1) if there is none"""
    best, wit = np.float32(np.inf), -1
    for j in range(len(d)):
        if d[j] != d[j]:
            continue
        if wit < 0 or d[j] < best:
            best, wit = d[j], j
    return best, wit


def pair(D):
    """One pair from its fp32 distance block D [n, m] -> (parts [4] fp32, F, G fp64, f [n] fp32, witness of f [n], g [m], witness of g [m])"""
    D = np.asarray(D, dtype=np.float32)
    n, m = D.shape
    ok = ~np.isnan(D)
    filled = np.where(ok, D, np.float32(np.inf))
    f, g = filled.min(axis=1), filled.min(axis=0)
    # the least index that attains the min among the entries that count (a +inf entry attains a +inf min; a NaN never does)
    wf = np.where(ok.any(axis=1), np.argmax(ok & (filled == f[:, None]), axis=1), -1)
    wg = np.where(ok.any(axis=0), np.argmax(ok & (filled == g[None, :]), axis=0), -1)
    with np.errstate(invalid="ignore"):  # fp64, index ascending: accumulate adds one element after the other (no pairwise tree)
        F = np.add.accumulate(f.astype(np.float64))[-1] / np.float64(n)
        G = np.add.accumulate(g.astype(np.float64))[-1] / np.float64(m)
    parts = np.array([np.float32(F), np.float32(G), f.max(), g.max()], dtype=np.float32)
    return parts, F, G, f, wf, g, wg


def score_of(measure, parts, F, G):
    measure = MEASURES.get(measure, measure)
    if measure == 0:
        return np.float32(F + G)  # the add in fp64, rounded once
    if measure == 1:
        return max(parts[2], parts[3])
    return np.float32(F)


def all_pairs(D, q_first, ids):
    """pair() of every (query set, segment) of D [nq, N]: [S][n_seg] -- what match() takes as ``pairs`` when it is called more than once"""
    D = np.asarray(D, dtype=np.float32)
    first, count, _ = segments(ids)
    return [[pair(D[int(q_first[s]):int(q_first[s + 1]), first[g]:first[g] + count[g]]) for g in range(len(first))]
            for s in range(len(q_first) - 1)]


def match(D, q_first, ids, k, measure, query_ids=None, pairs=None):
    """The definition over D [nq, N]: -> {"score" [S, k], "segment", "id", "size", "parts" [S, k, 4], "match_position" [nq, k],
    "match_dist2" [nq, k], "all_parts" [S, n_seg, 4], "all_scores" [S, n_seg]}; places without a segment hold the tail."""
    D = np.asarray(D, dtype=np.float32)
    q_first = np.asarray(q_first, dtype=np.int64)
    S, nq = len(q_first) - 1, int(q_first[-1])
    first, count, sid = segments(ids)
    n_seg = len(first)
    out = {"score": np.full((S, k), np.inf, np.float32), "segment": np.full((S, k), -1, np.int32), "id": np.full((S, k), -1, np.int64),
           "size": np.zeros((S, k), np.int32), "parts": np.full((S, k, 4), np.inf, np.float32),
           "match_position": np.full((nq, k), -1, np.int32), "match_dist2": np.full((nq, k), np.inf, np.float32),
           "all_parts": np.zeros((S, n_seg, 4), np.float32), "all_scores": np.zeros((S, n_seg), np.float32)}
    for s in range(S):
        a0, a1 = int(q_first[s]), int(q_first[s + 1])
        res = pairs[s] if pairs is not None else [pair(D[a0:a1, first[g]:first[g] + count[g]]) for g in range(n_seg)]
        sc = np.array([score_of(measure, r[0], r[1], r[2]) for r in res], dtype=np.float32).reshape(n_seg)
        assert not np.isnan(sc).any()
        for g in range(n_seg):
            out["all_parts"][s, g], out["all_scores"][s, g] = res[g][0], sc[g]
        cand = np.arange(n_seg)
        if query_ids is not None:
            cand = cand[sid != query_ids[s]]
        order = cand[np.lexsort((cand, sc[cand]))][:k]  # last key first: score, then segment
        for p, g in enumerate(order):
            out["score"][s, p], out["segment"][s, p], out["id"][s, p], out["size"][s, p] = sc[g], g, sid[g], count[g]
            out["parts"][s, p] = res[g][0]
            wf = res[g][4]
            out["match_position"][a0:a1, p] = np.where(wf >= 0, first[g] + wf, -1)
            out["match_dist2"][a0:a1, p] = res[g][3]
    return out
