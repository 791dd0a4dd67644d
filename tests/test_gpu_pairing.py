"""GPU tests of the one-to-one atom maps (scann_index_pairing through Engine.index_pairing / index_pairing_batch,
HipModel.pair_structures / align_structures).  Every comparison with the host twin (scann_pairing_host) is an equality of bytes.

1. Kernel equals twin: all query x segment pairs of an index whose segment sizes lie around the size classes (32, 64, 128) and the 64-lane
   column split, two of them above the limit, in one shuffled call with repeats; Gaussian rows, the pathological pool of tests/rank_ref.py
   (NaN, inf, overflow, coincident rows) and integer-valued rows in three values (ties, long alternating paths); dim 2, 3, 128, 130; a
   segment across a storage-chunk boundary; planted pairs.
2. Rerank equals the definition, assembled from index_match (the shortlist) and the twin, for the three measures; k = shortlist, a
   shortlist above the number of segments, every segment excluded, an empty index.
3. Invariance, bitwise: a structure alone / in another call / at another place; one add or many.
4. End to end on the 24-molecule model of tests/test_gpu_match.py: pair_structures is index_pairing on the model's rows, y the plain
   forward's; every indexed structure finds itself with the identity map; align_structures returns a planted permutation; state; a generic
   width, SCANN_GENERIC=1, SCANN_EXACT=1; errors; the CLI."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # the child process of the environment-switch tests
    for p in (os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, p)

import pairing_ref  # noqa: E402
import rank_ref  # noqa: E402
import scann_oracle as so  # noqa: E402
from analysis_checks import amask_of, padded, setup, training_twin  # noqa: E402
from test_gpu_match import atom_rows, firsts, ids_of  # noqa: E402

pytestmark = pytest.mark.gpu

MEASURES = ("chamfer", "hausdorff", "cover")
SEG_SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
SET_SIZES = [1, 2, 33, 64, 65, 127, 128, 5]
INT_SEGS, INT_SETS = (1, 5, 7, 9), (1, 4, 6)  # integer-valued rows in three values: sizes 2, 63, 65, 128 and 2, 65, 128


@pytest.fixture(scope="module")
def engine(hip_lib):
    cfg, w, inputs, model = setup(n=4)
    yield model.engine
    model.engine.close()


def twin_pairs(q, q_first, rows, seg_first, pair_set, pair_seg):
    """index_pairing's dict from the host twin, pair by pair"""
    from scann import _hip

    out = {"score": [], "total": [], "shift": [], "partner_position": [], "partner_dist2": []}
    memo = {}
    for s, g in zip(pair_set, pair_seg):
        if (s, g) not in memo:
            memo[(s, g)] = _hip.pairing_host(q[q_first[s]:q_first[s + 1]], rows[seg_first[g]:seg_first[g + 1]])
        r = memo[(s, g)]
        out["score"].append(r["score"]), out["total"].append(r["total"]), out["shift"].append(r["shift"])
        out["partner_position"].append(np.where(r["partner"] >= 0, seg_first[g] + r["partner"], -1))
        out["partner_dist2"].append(r["partner_dist2"])
    return {"score": np.array(out["score"], np.float32), "total": np.array(out["total"], np.int64), "shift": np.array(out["shift"], np.int32),
            "partner_position": np.concatenate(out["partner_position"]).astype(np.int32) if len(pair_set) else np.zeros(0, np.int32),
            "partner_dist2": np.concatenate(out["partner_dist2"]).astype(np.float32) if len(pair_set) else np.zeros(0, np.float32)}


def same(got, ref, label):
    for key in ref:
        a, b = got[key], ref[key]
        assert a.shape == b.shape and a.dtype == b.dtype, (label, key, a.shape, b.shape, a.dtype, b.dtype)
        if a.tobytes() != b.tobytes():
            bad = np.nonzero(a.view(np.uint32 if a.itemsize == 4 else np.uint64) != b.view(np.uint32 if b.itemsize == 4 else np.uint64))[0][:5]
            print("%s: %s differs at %s: got %s, expected %s" % (label, key, bad.tolist(), a[bad], b[bad]))
        assert a.tobytes() == b.tobytes(), (label, key)


def mixed_rows(sizes, int_groups, dim, seed):
    """the pathological pool over all rows, the groups ``int_groups`` replaced by integer-valued rows in three values"""
    first = firsts(sizes)
    rows = rank_ref.pathological_pool(int(first[-1]), dim, seed=seed)
    rng = np.random.default_rng(seed + 17)
    for g in int_groups:
        rows[first[g]:first[g + 1]] = rng.integers(0, 3, (sizes[g], dim)).astype(np.float32)
    return rows, first


@pytest.mark.parametrize("dim", [2, 3, 128, 130])
def test_kernel_equals_twin(engine, dim):
    rows, seg_first = mixed_rows(SEG_SIZES, INT_SEGS, dim, 1)
    q, q_first = mixed_rows(SET_SIZES, INT_SETS, dim, 2)
    rng = np.random.default_rng(dim)
    ps, pg = [a.ravel() for a in np.meshgrid(np.arange(len(SET_SIZES)), np.arange(len(SEG_SIZES)), indexing="ij")]
    extra = rng.integers(0, len(ps), 20)  # repeats
    order = rng.permutation(len(ps) + 20)
    ps, pg = np.concatenate([ps, ps[extra]])[order], np.concatenate([pg, pg[extra]])[order]
    ix = engine.index_create(dim)
    try:
        engine.index_add(ix, rows, ids_of(SEG_SIZES))
        got = engine.index_pairing(ix, q, q_first, ps, pg)
        ref = twin_pairs(q, q_first, rows, seg_first, ps, pg)
        same(got, ref, "dim %d" % dim)
        assert np.array_equal(got["offset"], firsts(np.diff(q_first)[ps]))
        # what the pool planted shows: the long segments, the NaN / inf / overflow rows are not comparable, the rest is
        sc = {(s, g): got["score"][e] for e, (s, g) in enumerate(zip(ps, pg))}
        for s in range(len(SET_SIZES)):
            for g in range(len(SEG_SIZES)):
                dead = g in (2, 3, 10, 11) or s in (2, 3)
                assert np.isposinf(sc[(s, g)]) == dead, (s, g, sc[(s, g)])
        # the definition's value by SciPy, on a pair of every class
        from scann import _hip

        for s, g in ((0, 0), (7, 4), (4, 5), (5, 8), (6, 9)):
            e = int(np.nonzero((ps == s) & (pg == g))[0][0])
            D = _hip.knn_dist2_matrix(q[q_first[s]:q_first[s + 1]], rows[seg_first[g]:seg_first[g + 1]])
            want = pairing_ref.pair(D)
            assert got["total"][e] == want["total"] and got["shift"][e] == want["shift"] and got["score"][e].tobytes() == want["score"].tobytes()
            o = got["offset"]
            pos = got["partner_position"][o[e]:o[e + 1]]
            pairing_ref.check_map(D, np.where(pos >= 0, pos - seg_first[g], -1), got["partner_dist2"][o[e]:o[e + 1]], int(got["total"][e]))
        # no pairs: nothing to do
        none = engine.index_pairing(ix, q, q_first, [], [])
        assert none["score"].shape == (0,) and none["partner_position"].shape == (0,)
    finally:
        ix.free()


def test_a_segment_across_the_chunk_boundary(engine):
    """1,024 columns: a storage chunk holds 16,384 rows, and the 128-row segment of rows 16,300 .. 16,427 lies in two of them"""
    rng = np.random.default_rng(3)
    dim = 1024
    sizes = [100] * 163 + [128, 72]
    N = sum(sizes)
    rows = rng.standard_normal((N, dim)).astype(np.float32)
    q_first = firsts([128, 3, 40])
    q = rng.standard_normal((171, dim)).astype(np.float32)
    perm = rng.permutation(128)
    rows[16300 + perm] = q[:128]  # set 0 is the segment, permuted
    ix = engine.index_create(dim)
    try:
        engine.index_add(ix, rows, ids_of(sizes))
        ps, pg = np.array([0, 1, 2, 0, 2]), np.array([163, 163, 163, 162, 164])
        got = engine.index_pairing(ix, q, q_first, ps, pg)
        same(got, twin_pairs(q, q_first, rows, firsts(sizes), ps, pg), "two chunks")
        assert got["score"][0] == 0 and np.array_equal(got["partner_position"][:128], 16300 + perm)
    finally:
        ix.free()


def test_planted_pairs(engine):
    rng = np.random.default_rng(5)
    dim = 128
    sizes = [20, 20, 33, 7, 7]
    f = firsts(sizes)
    rows = (rng.standard_normal((sum(sizes), dim)) * 2).astype(np.float32)
    q_first = firsts([20, 7, 12])
    q = (rng.standard_normal((39, dim)) * 2).astype(np.float32)
    perm = rng.permutation(20)
    rows[f[0]:f[1]] = q[:20]                # segment 0 is query 0
    rows[f[1] + perm] = q[:20]              # segment 1 is a permuted copy
    rows[f[2] + 11, 5] = np.nan             # a NaN row inside segment 2
    rows[f[3]:f[4]] = q[20]                 # segment 3 is seven copies of one row ...
    q[21:27] = q[20]                        # ... and so is query 1: Dmax = 0
    rows[f[4]:f[5]] = q[20]
    rows[f[4], 0] += np.float32(1)          # segment 4: one row a little off
    ix = engine.index_create(dim)
    try:
        engine.index_add(ix, rows, ids_of(sizes))
        ps, pg = [a.ravel() for a in np.meshgrid(np.arange(3), np.arange(5), indexing="ij")]
        got = engine.index_pairing(ix, q, q_first, ps, pg)
        same(got, twin_pairs(q, q_first, rows, f, ps, pg), "planted")
        o = got["offset"]
        assert got["score"][0] == 0 and got["total"][0] == 0 and np.array_equal(got["partner_position"][o[0]:o[1]], np.arange(20))
        assert got["score"][1] == 0 and np.array_equal(got["partner_position"][o[1]:o[2]], f[1] + perm) and not got["partner_dist2"][o[1]:o[2]].any()
        for e in (2, 7, 12):  # the NaN segment: not comparable
            assert np.isposinf(got["score"][e]) and got["total"][e] == -1 and got["shift"][e] == 0
            assert np.all(got["partner_position"][o[e]:o[e + 1]] == -1) and np.all(np.isposinf(got["partner_dist2"][o[e]:o[e + 1]]))
        e = 8  # query 1 against segment 3: Dmax = 0, shift 0, the identity by the tie rule
        assert got["score"][e] == 0 and got["shift"][e] == 0 and np.array_equal(got["partner_position"][o[e]:o[e + 1]], f[3] + np.arange(7))
        e = 9  # ... against segment 4: one pair pays 1
        assert got["shift"][e] == 30 and got["total"][e] == 1 << 30 and got["score"][e] == np.float32(1 / 7)
    finally:
        ix.free()


def test_invariance_of_a_structure_and_of_how_the_index_was_built(engine):
    rng = np.random.default_rng(9)
    dim = 130
    sizes = [17, 40, 1, 64, 100, 128, 3, 65]
    N = sum(sizes)
    rows = rng.integers(0, 3, (N, dim)).astype(np.float32)
    rows[:200] = rng.standard_normal((200, dim)).astype(np.float32)
    ids = ids_of(sizes)
    qs = [17, 1, 128, 30, 64]
    q_first = firsts(qs)
    q = rng.integers(0, 3, (int(q_first[-1]), dim)).astype(np.float32)
    one, many = engine.index_create(dim), engine.index_create(dim)
    try:
        engine.index_add(one, rows, ids)
        at = 0
        for step in [1, 63, 64, 65, 7, 100, 3]:  # the adds cut through segments
            engine.index_add(many, rows[at:at + step], ids[at:at + step])
            at += step
        engine.index_add(many, rows[at:], ids[at:])
        ps, pg = [a.ravel() for a in np.meshgrid(np.arange(len(qs)), np.arange(len(sizes)), indexing="ij")]
        full = engine.index_pairing(one, q, q_first, ps, pg)
        again = engine.index_pairing(many, q, q_first, ps, pg)
        for key in full:
            assert full[key].tobytes() == again[key].tobytes(), key
        s = 3  # structure 3 alone, and at another place among other structures, its pairs in another order
        a0, a1 = q_first[s], q_first[s + 1]
        alone = engine.index_pairing(one, q[a0:a1], [0, a1 - a0], np.zeros(len(sizes), int), np.arange(len(sizes)))
        moved_q = np.concatenate([q[q_first[4]:q_first[5]], q[a0:a1], q[q_first[0]:q_first[1]]])
        rev = np.arange(len(sizes))[::-1]
        moved = engine.index_pairing(one, moved_q, firsts([qs[4], qs[s], qs[0]]), np.ones(len(sizes), int), rev)
        sel = np.nonzero(ps == s)[0]
        for j, e in enumerate(sel):
            g = pg[e]
            r = len(sizes) - 1 - g
            for key in ("score", "total", "shift"):
                assert full[key][e].tobytes() == alone[key][g].tobytes() == moved[key][r].tobytes(), (key, g)
            for key in ("partner_position", "partner_dist2"):
                x = full[key][full["offset"][e]:full["offset"][e + 1]]
                assert x.tobytes() == alone[key][alone["offset"][g]:alone["offset"][g + 1]].tobytes(), (key, g)
                assert x.tobytes() == moved[key][moved["offset"][r]:moved["offset"][r + 1]].tobytes(), (key, g)
    finally:
        one.free()
        many.free()


# ---- the rerank ----

BATCH_KEYS = ("score", "segment", "id", "size", "total", "shift", "short_score", "short_place", "partner_position", "partner_dist2")


def rerank_ref(eng, ix, qrows, q_first, k, shortlist, measure, query_ids=None):
    """index_pairing_batch's answer from the definition: the shortlist of index_match, the twin on every shortlisted pair, the order"""
    from scann import _hip

    sl = eng.index_match(ix, qrows, q_first, shortlist, measure, query_ids=query_ids)
    rows, _, _ = eng.index_read(ix)
    first, count, sid = eng.index_segments(ix)
    B, A = len(q_first) - 1, len(qrows)
    out = {"score": np.full((B, k), np.inf, np.float32), "segment": np.full((B, k), -1, np.int32), "id": np.full((B, k), -1, np.int64),
           "size": np.zeros((B, k), np.int32), "total": np.full((B, k), -1, np.int64), "shift": np.zeros((B, k), np.int32),
           "short_score": np.full((B, k), np.inf, np.float32), "short_place": np.full((B, k), -1, np.int32),
           "partner_position": np.full((A, k), -1, np.int32), "partner_dist2": np.full((A, k), np.inf, np.float32)}
    for s in range(B):
        a0, a1 = q_first[s], q_first[s + 1]
        segs = sl["segment"][s]
        res = [_hip.pairing_host(qrows[a0:a1], rows[first[g]:first[g] + count[g]]) if g >= 0 else None for g in segs]
        places = pairing_ref.rerank(segs, sl["score"][s], [np.inf if r is None else r["score"] for r in res], k)
        for j, pl in enumerate(places):
            if pl < 0:
                continue
            g, r = segs[pl], res[pl]
            out["score"][s, j], out["segment"][s, j], out["id"][s, j], out["size"][s, j] = r["score"], g, sid[g], count[g]
            out["total"][s, j], out["shift"][s, j], out["short_score"][s, j], out["short_place"][s, j] = r["total"], r["shift"], sl["score"][s, pl], pl
            out["partner_position"][a0:a1, j] = np.where(r["partner"] >= 0, first[g] + r["partner"], -1)
            out["partner_dist2"][a0:a1, j] = r["partner_dist2"]
    return out


@pytest.fixture(scope="module")
def world(hip_lib):
    """the 24-molecule QM9-shaped model of test_gpu_match.setup, an atom-level index of its data, 9 query molecules and their rows"""
    cfg, w, data, model = setup(n=24, seed=0)
    queries = padded("qm9", 9, 1, cfg)
    ix = model.build_index(data, level="atom", ids=np.arange(24) * 2 + 100, batch_size=16)
    y, ga = model.predict(queries)
    yield {"cfg": cfg, "w": w, "data": data, "model": model, "queries": queries, "ix": ix, "y": y, "ga": ga, "qrows": atom_rows(model, queries),
           "q_first": firsts(amask_of(queries).sum(1))}
    ix.free()
    model.engine.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_rerank_equals_the_definition(world, measure):
    from scann import _hip

    eng, ix, queries = world["model"].engine, world["ix"], world["queries"]
    qm = amask_of(queries)
    rb = eng.upload(_hip.pack_inputs(queries))
    try:
        qid = np.array([100, 102, 7, 146, 104, 7, 7, 120, 122], np.int64)
        for k, shortlist, ids in ((3, 8, None), (5, 5, None), (2, 32, None), (4, 24, qid), (1, 1, None)):  # (32: above the 24 segments)
            got = eng.index_pairing_batch(ix._ix, rb, k, shortlist, measure, query_ids=ids)
            assert got["y"].tobytes() == world["y"][:, 0].tobytes() and got["ga"].tobytes() == world["ga"][qm][:, 0].tobytes()
            ref = rerank_ref(eng, ix._ix, world["qrows"], world["q_first"], k, shortlist, measure, query_ids=ids)
            same({n: got[n] for n in BATCH_KEYS}, ref, "%s k %d shortlist %d" % (measure, k, shortlist))
            assert np.all(got["segment"] >= 0) and np.all(np.diff(got["score"], axis=1) >= 0)
            if ids is not None:
                assert not np.any(got["id"] == ids[:, None])
    finally:
        rb.free()


def test_rerank_tails(world):
    """every segment excluded, and an empty index: the tail everywhere"""
    from scann import _hip

    eng = world["model"].engine
    rb = eng.upload(_hip.pack_inputs(world["queries"]))
    one, empty = eng.index_create(128), eng.index_create(128)
    try:
        eng.index_add(one, world["qrows"][:12], np.full(12, 3, np.int64))
        for ix, ids in ((one, np.full(9, 3, np.int64)), (empty, None)):
            got = eng.index_pairing_batch(ix, rb, 3, 7, "chamfer", query_ids=ids)
            same({n: got[n] for n in BATCH_KEYS}, rerank_ref(eng, ix, world["qrows"], world["q_first"], 3, 7, "chamfer", query_ids=ids), "tail")
            for key, tail in (("segment", -1), ("id", -1), ("size", 0), ("total", -1), ("shift", 0), ("short_place", -1), ("partner_position", -1)):
                assert np.all(got[key] == tail), key
            assert np.all(np.isposinf(got["score"])) and np.all(np.isposinf(got["short_score"])) and np.all(np.isposinf(got["partner_dist2"]))
        got = eng.index_pairing_batch(one, rb, 3, 7, "chamfer")  # one segment, nothing excluded: place 0, then the tail
        assert np.all(got["segment"][:, 0] == 0) and np.all(got["segment"][:, 1:] == -1) and np.all(got["size"][:, 0] == 12)
    finally:
        rb.free()
        one.free()
        empty.free()


# ---- end to end ----

def permuted(inputs, perms):
    """the padded batch with the atoms of structure b moved: new position perms[b][i] holds old atom i (neighbour lists keep their order)"""
    out = {k: np.array(v) for k, v in inputs.items()}
    am = amask_of(inputs)
    for b, pi in enumerate(perms):
        n = len(pi)
        assert am[b, :n].all() and not am[b, n:].any()
        for key, v in inputs.items():
            v = np.asarray(v)
            if v.ndim >= 2 and v.shape[1] == am.shape[1]:
                out[key][b, pi] = v[b, :n]
        nb = np.asarray(inputs["neighbors"])[b, :n]
        nmask = np.asarray(inputs["neighbor_mask"])[b, :n].reshape(nb.shape) != 0
        out["neighbors"][b, pi] = np.where(nmask, np.asarray(pi)[np.clip(nb, 0, n - 1)], nb)
    return out


def test_pair_structures_is_the_pairing_on_the_models_rows(world):
    from scann import _hip

    model, ix, queries, data = world["model"], world["ix"], world["queries"], world["data"]
    eng, qm, qcnt = model.engine, amask_of(queries), amask_of(queries).sum(1)
    _, atoms = ix.names()
    first, count, sid = ix.segments()
    for measure in ("chamfer", "cover"):
        got = model.pair_structures(queries, ix, k=3, shortlist=8, measure=measure, batch_size=4)
        ref = rerank_ref(eng, ix._ix, world["qrows"], world["q_first"], 3, 8, measure)
        assert got["predict_property"].tobytes() == world["y"].tobytes()
        assert got["distance"].tobytes() == np.sqrt(ref["score"]).tobytes() and np.array_equal(got["neighbor_id"], ref["id"])
        assert np.array_equal(got["neighbor_size"], ref["size"]) and np.array_equal(got["surplus"], qcnt[:, None] - ref["size"])
        assert got["shortlist_distance"].tobytes() == np.sqrt(ref["short_score"]).tobytes() and np.array_equal(got["shortlist_place"], ref["short_place"])
        pos = ref["partner_position"]
        assert np.array_equal(got["paired_atom"][qm], np.where(pos >= 0, atoms[np.maximum(pos, 0)], -1))
        assert got["paired_distance"][qm].tobytes() == np.sqrt(ref["partner_dist2"]).tobytes()
        assert np.all(got["paired_atom"][~qm] == -1) and not got["paired_distance"][~qm].any()
        # and index_pairing on the same rows, pair by pair
        ps, pg = np.repeat(np.arange(9), 3), ref["segment"].ravel()
        direct = eng.index_pairing(ix._ix, world["qrows"], world["q_first"], ps, pg)
        assert direct["score"].tobytes() == ref["score"].tobytes() and np.array_equal(direct["total"], ref["total"].ravel())
    # the indexed structures themselves: place 0, distance 0, the identity map; with exclude_ids not
    dm, cnt = amask_of(data), amask_of(data).sum(1)
    own = np.arange(24) * 2 + 100
    me = model.pair_structures(data, ix, k=2, shortlist=6)
    loo = model.pair_structures(data, ix, k=2, shortlist=6, exclude_ids=own)
    assert not me["distance"][:, 0].any() and np.array_equal(me["neighbor_id"][:, 0], own) and np.array_equal(me["neighbor_size"][:, 0], cnt)
    assert not me["surplus"][:, 0].any() and not me["paired_distance"][..., 0].any()
    assert np.array_equal(me["paired_atom"][..., 0][dm], np.concatenate([np.arange(c) for c in cnt]))
    assert np.all(loo["distance"][:, 0] > 0) and not np.any(loo["neighbor_id"] == own[:, None])
    # packed in, packed out
    pk = _hip.pack_inputs(queries)
    p, g = model.pair_structures(pk, ix, k=3), model.pair_structures(queries, ix, k=3)
    assert p["paired_atom"].shape == (qcnt.sum(), 3) and np.array_equal(p["paired_atom"], g["paired_atom"][qm])
    assert p["paired_distance"].tobytes() == g["paired_distance"][qm].tobytes() and p["distance"].tobytes() == g["distance"].tobytes()


def test_align_structures_returns_a_planted_permutation(world):
    model, data = world["model"], world["data"]
    x = {k: np.asarray(v)[:6] for k, v in data.items()}
    cnt = amask_of(x).sum(1)
    rng = np.random.default_rng(2)
    perms = [rng.permutation(c) for c in cnt]
    r = model.align_structures(x, permuted(x, perms), batch_size=4)
    am = amask_of(x)
    print("align: distances", r["distance"])
    assert r["distance"].shape == (6,) and r["atom_map"].shape == am.shape and r["atom_distance"].shape == am.shape and not r["surplus"].any()
    for b in range(6):
        assert np.array_equal(r["atom_map"][b, :cnt[b]], perms[b]) and np.all(r["atom_map"][b, cnt[b]:] == -1), b
    assert np.all(r["distance"] < 1e-3)  # the same atoms in another order: the rows differ by summation order at the most
    y = model.predict(x)[0]
    assert r["predict_property"].tobytes() == y.tobytes() and np.allclose(r["predict_property_b"], y, rtol=1e-5, atol=1e-6)
    # against other structures: a map one to one, the surplus counted
    z = {k: np.asarray(v)[6:12] for k, v in data.items()}
    r = model.align_structures(x, z)
    cz = amask_of(z).sum(1)
    assert np.array_equal(r["surplus"], cnt - cz)
    for b in range(6):
        real = r["atom_map"][b][r["atom_map"][b] >= 0]
        assert len(set(real.tolist())) == len(real) == min(cnt[b], cz[b]) and np.all(real < cz[b])


def test_selected_outputs_and_weights_survive(hip_lib):
    from scann import _hip

    cfg, w, data, model = setup(n=6, seed=1)
    eng = model.engine
    names = ["local_attention_1", "bf_property"]
    before = model.predict(data, outputs=names)
    y0, ga0 = model.predict(data)
    w0 = {k: v.copy() for k, v in eng.get_weights().items()}
    eng.set_outputs([1], bf_property=True)
    try:
        rb = eng.upload(_hip.pack_inputs(data))
        eng.forward_resident(rb)
        y_first, _ = eng.download(rb)
        ix = eng.index_create(128)
        eng.index_add_batch(ix, rb, _hip.OUT_AFTER_LC, np.arange(6))
        r = eng.index_pairing_batch(ix, rb, 2, 4, "chamfer")
        assert r["y"].tobytes() == y_first.tobytes() and not r["score"][:, 0].any() and np.array_equal(r["id"][:, 0], np.arange(6))
        wrong = eng.index_create(64)
        with pytest.raises(_hip.ScannHipError):
            eng.index_pairing_batch(wrong, rb, 2, 4)
        eng.forward_resident(rb)
        eng.download(rb)
        with pytest.raises(_hip.ScannHipError):
            eng.read_output(rb, _hip.OUT_AFTER_LC)  # the handle's selection is what it was
        rb.free()
        ix.free()
        wrong.free()
    finally:
        eng.set_outputs()
    after = model.predict(data, outputs=names)
    assert all(x.tobytes() == y_.tobytes() for x, y_ in zip(before, after))
    y1, ga1 = model.predict(data)
    assert y0.tobytes() == y1.tobytes() and ga0.tobytes() == ga1.tobytes()
    for k, v in eng.get_weights().items():
        assert v.tobytes() == w0[k].tobytes(), k


def test_errors_name_what_is_wrong(hip_lib):
    from scann import _hip

    cfg, w, data, model = setup(n=4, seed=1)
    eng = model.engine
    rb = eng.upload(_hip.pack_inputs(data))
    ix = eng.index_create(128)
    eng.index_add(ix, np.zeros((3, 128), np.float32))
    q = np.zeros((200, 128), np.float32)
    score = np.zeros(64, np.float32)

    def pairing(q_first=(0, 1, 2), pair_set=(0, 1), pair_seg=(0, 2), index=ix, handle=eng, sc=score, qp=q, n_pairs=None):
        qf, a, b = np.asarray(q_first, np.int32), np.asarray(pair_set, np.int32), np.asarray(pair_seg, np.int32)
        return eng.lib.scann_index_pairing(handle._h, index._h, _hip._ptr(qp), _hip._ptr(qf), len(qf) - 1, _hip._ptr(a), _hip._ptr(b),
                                           len(a) if n_pairs is None else n_pairs, _hip._ptr(sc), None, None, None, None)

    def batch(k=3, shortlist=8, measure=0, index=ix, db=rb, sc=score):
        return eng.lib.scann_index_pairing_batch(eng._h, index._h, None if db is None else db._h, None, measure, shortlist, k, None, None, _hip._ptr(sc),
                                                 None, None, None, None, None, None, None, None, None)

    def message(e=eng):
        return (eng.lib.scann_last_error(e._h) or b"").decode()

    assert pairing() == 0 and not score[:2].any()  # all outputs but score may be NULL
    assert pairing(pair_set=(0, 2)) == -1 and "pair_set[1] is 2" in message()
    assert pairing(pair_seg=(3, 0)) == -1 and "pair_segment[0] is 3" in message()
    assert pairing(pair_set=(-1, 0)) == -1 and "pair_set[0]" in message()
    assert pairing(sc=None) == -1 and "score is null" in message()
    assert pairing(qp=None) == -1 and "empty query" in message()
    assert pairing(q_first=(0,)) == -1 and "empty query" in message()
    assert pairing(q_first=(0, 2, 2)) == -1 and "query structure 1 is an empty set" in message()
    assert pairing(q_first=(0, 5, 134)) == -2 and "query structure 1 has 129 atoms" in message() and "SCANN_PAIRING_MAX_ATOMS" in message()
    assert pairing(n_pairs=-1) == -1 and "n_pairs" in message()
    assert pairing(pair_set=(), pair_seg=()) == 0
    for k in (0, 33):
        assert batch(k=k) == -1 and "k %d outside 1 .. 32" % k in message()
    for k, s in ((3, 2), (3, 33), (5, 0)):
        assert batch(k=k, shortlist=s) == -1 and "shortlist %d outside k = %d .. 32" % (s, k) in message()
    for m in (3, -1):
        assert batch(measure=m) == -1 and "measure %d" % m in message()
    assert batch(sc=None) == -1 and "score is null" in message()
    assert batch(db=None) == -1 and "null argument" in message()
    narrow = eng.index_create(64)
    assert batch(index=narrow) == -1 and "64 columns" in message() and "global_dim is 128" in message()
    cfg2, w2, _, other = setup(n=4, seed=1)
    assert pairing(handle=other.engine) == -1 and "another handle" in message(other.engine)
    assert batch() == 0
    # the Python layer
    for bad in (dict(q_first=[0, 129, 200]), dict(q_first=[0, 100]), dict(pair_set=[2]), dict(pair_segment=[3]), dict(pair_set=[0, 1])):
        kw = dict(q_first=[0, 100, 200], pair_set=[0], pair_segment=[0])
        kw.update(bad)
        with pytest.raises(ValueError):
            eng.index_pairing(ix, q, **kw)
    with pytest.raises(ValueError):
        eng.index_pairing(ix, q[:, :64], [0, 100, 200], [0], [0])
    with pytest.raises(ValueError):
        eng.index_pairing_batch(ix, rb, 3, 2)
    with pytest.raises(ValueError):
        eng.index_pairing_batch(ix, rb, 3, 8, query_ids=[1])
    rb.free()
    ix.free()
    narrow.free()


def test_generic_widths(hip_lib):
    """widths other than 128 / 8 (the plain-fp32 kernels): after_Lc rows of 96 columns"""
    cfg, w, data, model = setup(n=9, seed=41, local_dim=64, num_head=4, global_dim=96, dense_out=32)
    ix = model.build_index(data, level="atom", batch_size=4)
    assert ix.dim == 96
    rows, cnt = atom_rows(model, data), amask_of(data).sum(1)
    got = model.pair_structures(data, ix, k=4, shortlist=6, measure="hausdorff", batch_size=5)
    ref = rerank_ref(model.engine, ix._ix, rows, firsts(cnt), 4, 6, "hausdorff")
    assert got["distance"].tobytes() == np.sqrt(ref["score"]).tobytes() and not got["distance"][:, 0].any() and np.array_equal(got["neighbor_id"], ref["id"])
    ix.free()


def child_scenario():
    """what the environment-switch children run: pair_structures is the definition on the model's rows, y is the forward's"""
    cfg, w, data, model = setup(n=10, seed=3)
    queries = padded("qm9", 6, 4, cfg)
    ix = model.build_index(data, level="atom", batch_size=4)
    qrows, qcnt = atom_rows(model, queries), amask_of(queries).sum(1)
    y, _ = model.predict(queries)
    for measure in MEASURES:
        got = model.pair_structures(queries, ix, k=3, shortlist=7, measure=measure, batch_size=4)
        ref = rerank_ref(model.engine, ix._ix, qrows, firsts(qcnt), 3, 7, measure)
        assert got["distance"].tobytes() == np.sqrt(ref["score"]).tobytes() and np.array_equal(got["neighbor_id"], ref["id"]), measure
        assert got["predict_property"].tobytes() == y.tobytes(), measure
    ix.free()


@pytest.mark.parametrize("switch", ["SCANN_GENERIC", "SCANN_EXACT"])
def test_under_an_environment_switch(hip_lib, switch):
    """a 128 / 8 handle forced onto the plain-fp32 kernels (SCANN_GENERIC=1), a handle whose forwards run exact-fp32 (SCANN_EXACT=1):
    a fresh process each"""
    e = dict(os.environ)
    e[switch] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_training_handle(hip_lib):
    """after two training steps the pairings are an inference handle's with the same weights, and weights, gradients and the following
    (deterministic) step are those of a twin that never made the calls"""
    from scann import _hip

    cfg, w, data, _ = setup(n=8, seed=5, n_attention=2)

    def calls(train_model, rb, inference):
        eng, (inf_model, rb2) = train_model.engine, inference()
        inf = inf_model.engine
        a, b = eng.index_create(128), inf.index_create(128)
        eng.index_add_batch(a, rb, _hip.OUT_AFTER_LC, np.arange(8))
        inf.index_add_batch(b, rb2, _hip.OUT_AFTER_LC, np.arange(8))
        qa, qb = eng.index_pairing_batch(a, rb, 3, 6, "chamfer", np.arange(8)), inf.index_pairing_batch(b, rb2, 3, 6, "chamfer", np.arange(8))
        for key in qa:
            assert qa[key].tobytes() == qb[key].tobytes() and qa[key].dtype == qb[key].dtype, key
        a.free()
        b.free()

    training_twin(cfg, w, _hip.pack_inputs(data), calls)


def test_cli_writes_the_pairs(hip_lib, tmp_path):
    """predict_model.py --pair 3: pair_<target>.pickle, one unpadded dict per structure, leave-one-out over the dataset itself; the other
    files' bytes are those of a run without the flag"""
    import yaml

    from scann.models import SCANN
    from scann.models.scann_model import save_container

    n = 20
    de, dn = so.synth_dataset(n, 5)
    full = np.empty(n, dtype=object)
    for i in range(n):
        full[i] = {"Atomic": de[i][0], "Properties": {"homo": float(i)}}
    np.save(tmp_path / "data_energy.npy", full, allow_pickle=True)
    np.save(tmp_path / "data_nei.npy", dn, allow_pickle=True)
    cfg = so.default_config("qm9")
    cfg["model"]["n_attention"] = 2
    cfg["hyper"].update(batch_size=8, scaler=False, use_ref=False, target="homo", data_energy_path=str(tmp_path / "data_energy.npy"),
                        data_nei_path=str(tmp_path / "data_nei.npy"), save_path=str(tmp_path / "run"))
    out = tmp_path / "model"
    os.makedirs(out / "models")
    yaml.safe_dump(cfg, open(out / "config.yaml", "w"))
    save_container(str(out / "models" / "model_homo.h5"), cfg, so.init_weights(cfg, 77, perturb=True))
    cli = [sys.executable, os.path.join(ROOT, "predict_model.py"), str(out)]
    r = subprocess.run(cli, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    plain = {f: open(out / f, "rb").read() for f in ("ga_scores_homo.pickle", "energy_pre_homo.pickle")}
    assert not os.path.exists(out / "pair_homo.pickle")
    r = subprocess.run(cli + ["--pair", "3", "--pair-shortlist", "6", "--pair-measure", "cover"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f, b in plain.items():
        assert open(out / f, "rb").read() == b, f
    got = pickle.load(open(out / "pair_homo.pickle", "rb"))
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    data = scann.dataIter
    index = scann.build_index(data, level="atom", ids=data.indexes)
    i = 0
    for b in range(len(data)):
        inputs, _ = data[b]
        sel = np.asarray(data.indexes[b * 8:(b + 1) * 8])
        ref = scann.pair_structures(inputs, index, k=3, shortlist=6, measure="cover", exclude_ids=sel)
        am = amask_of(inputs)
        for s in range(len(sel)):
            d = got[i]
            assert sorted(d) == ["distance", "neighbor_id", "neighbor_size", "paired_atom", "paired_distance", "predict_property", "shortlist_distance",
                                 "shortlist_place", "surplus"]
            for key in ("distance", "neighbor_id", "neighbor_size", "shortlist_distance", "shortlist_place", "surplus"):
                assert np.array_equal(d[key], ref[key][s]), key
            assert np.array_equal(d["paired_atom"], ref["paired_atom"][s][am[s]]) and np.array_equal(d["paired_distance"], ref["paired_distance"][s][am[s]])
            assert d["predict_property"] == float(ref["predict_property"][s, 0])
            n_at = len(de[sel[s]][0])
            assert d["paired_atom"].shape == (n_at, 3) and np.all(d["paired_atom"] < d["neighbor_size"][None, :])
            assert np.array_equal((d["paired_atom"] < 0).sum(0), np.maximum(d["surplus"], 0))
            assert sel[s] not in d["neighbor_id"] and np.all(d["neighbor_id"] >= 0) and np.all(d["distance"] > 0)
            i += 1
    assert i == n == len(got)
    index.free()


if __name__ == "__main__":
    child_scenario()
    print("child ok")
