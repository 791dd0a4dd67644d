"""One-to-one atom maps between structures (scann_index_pairing) -- what needs no GPU: the solver twin scann_pairing_solve_host on integer
matrices against SciPy's optimum (and all permutations for Q <= 7); the pair twin scann_pairing_host against the NumPy definition of
tests/pairing_ref.py on the host twin's distances; the bitwise symmetry of the score; the integer lower bounds; header, ctypes and
library; the kernel's scratch; the sanitizer program; and the Python layer (argument checks before any upload, re-padding, surplus,
the facade, the CLI flags) over a stand-in engine."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import abi_checks
import match_ref
import pairing_ref
import scann_oracle as so
from test_match_host import _MatchStandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scann--material_amd", "csrc")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the solver twin ----

def _check_solver(C, identity=False):
    from scann import _hip

    col, total = _hip.pairing_solve_host(C)
    Q = C.shape[0]
    assert col.dtype == np.int32 and sorted(col.tolist()) == list(range(Q))  # a permutation ...
    assert int(C[np.arange(Q), col].astype(np.int64).sum()) == total == pairing_ref.optimum(C)  # ... that attains the optimum
    if identity:
        assert np.array_equal(col, np.arange(Q))
    return col, total


@pytest.mark.parametrize("Q", [1, 2, 7, 64, 128])
def test_solver_twin_on_integer_matrices(hip_lib, Q):
    rng = np.random.default_rng(Q)
    for rep in range(6 if Q <= 7 else 2):
        _check_solver(rng.integers(0, 1000, (Q, Q)))
        _check_solver(rng.integers(0, 2, (Q, Q)))            # 0 / 1: ties everywhere, long alternating paths
        _check_solver(rng.integers(0, 2 ** 31 + 1, (Q, Q)))  # the whole range
        top = rng.integers(0, 2 ** 31 + 1, (Q, Q))
        top[rng.random((Q, Q)) < 0.7] = 2 ** 31              # entries 2^31
        _check_solver(top)
    _check_solver(np.full((Q, Q), 5), identity=True)         # all equal: the tie rule gives the identity
    _check_solver(np.full((Q, Q), 2 ** 31), identity=True)
    if Q <= 7:  # the map is the procedure's, word for word
        for rep in range(10):
            C = rng.integers(0, 4, (Q, Q))
            col, total = _check_solver(C)
            ref_col, ref_total = pairing_ref.procedure(C)
            assert np.array_equal(col, ref_col) and total == ref_total


def test_solver_twin_refuses(hip_lib):
    from scann import _hip

    for bad in (np.zeros((2, 3), np.int64), np.zeros((0, 0), np.int64), np.zeros((2, 2), np.float32), np.array([[0, -1], [0, 0]]),
                np.array([[0, 2 ** 31 + 1], [0, 0]]), np.zeros(4, np.int64)):
        with pytest.raises(ValueError):
            _hip.pairing_solve_host(bad)
    c = np.array([1, 2, 3, 2 ** 31 + 1], np.uint32)
    assert hip_lib.scann_pairing_solve_host(_hip._ptr(c), 2, None, None) == -1
    assert hip_lib.scann_pairing_solve_host(None, 2, None, None) == -1
    assert hip_lib.scann_pairing_solve_host(_hip._ptr(c), 0, None, None) == -1
    assert hip_lib.scann_pairing_solve_host(_hip._ptr(c), _hip.PAIRING_SOLVE_MAX + 1, None, None) == -1


# ---- the pair twin ----

def _pair(a, b):
    """the twin's answer, checked against the definition on the host twin's distances"""
    from scann import _hip

    r = _hip.pairing_host(a, b)
    D = _hip.knn_dist2_matrix(a, b)
    ref = pairing_ref.pair(D)
    assert r["score"].dtype == np.float32 and _bits(r["score"]) == _bits(ref["score"]) and r["total"] == ref["total"] and r["shift"] == ref["shift"]
    pairing_ref.check_map(D, r["partner"], r["partner_dist2"], r["total"])
    return r, D


@pytest.mark.parametrize("dim", [1, 3, 130])
def test_pair_twin_is_the_definition(hip_lib, dim):
    from scann import _hip

    rng = np.random.default_rng(dim)
    for n, m in ((1, 1), (1, 128), (128, 1), (128, 128), (3, 7), (7, 3), (17, 23), (65, 64), (5, 5)):
        for integer in (False, True):
            a = rng.integers(0, 3, (n, dim)).astype(np.float32) if integer else rng.standard_normal((n, dim)).astype(np.float32)
            b = rng.integers(0, 3, (m, dim)).astype(np.float32) if integer else rng.standard_normal((m, dim)).astype(np.float32)
            ab, D = _pair(a, b)
            ba, _ = _pair(b, a)
            assert _bits(ab["score"]) == _bits(ba["score"]) and ab["total"] == ba["total"] and ab["shift"] == ba["shift"]  # symmetric, bit for bit
            assert int((ab["partner"] < 0).sum()) == max(n - m, 0)
            # the integer lower bounds
            shift, t = pairing_ref.quantise(D)
            if n <= m:
                assert ab["total"] >= int(t.min(axis=0).sum())
            if m <= n:
                assert ab["total"] >= int(t.min(axis=1).sum())
            if max(n, m) <= 23:  # the map is the procedure's
                col, total = pairing_ref.procedure(pairing_ref.cost_matrix(t))
                assert total == ab["total"] and np.array_equal(np.where(col[:n] < m, col[:n], -1), ab["partner"])


def test_pair_twin_on_planted_pairs(hip_lib):
    from scann import _hip

    rng = np.random.default_rng(4)
    a = rng.standard_normal((23, 3)).astype(np.float32)
    perm = rng.permutation(23)
    b = np.empty_like(a)
    b[perm] = a                                     # b[perm[i]] = a[i]: a permuted copy scores 0 and returns the permutation
    r, _ = _pair(a, b)
    assert r["score"] == 0 and r["total"] == 0 and np.array_equal(r["partner"], perm) and not r["partner_dist2"].any()
    # the counting example: rows {3 x a, 3 x b} against {5 x a, 1 x b}, |a - b|^2 = 8 -- chamfer 0, the pairing 16 / 6
    x, y = [0, 0], [2, 2]
    A, B = np.array([x, x, x, y, y, y], np.float32), np.array([x, x, x, x, x, y], np.float32)
    assert match_ref.pair(_hip.knn_dist2_matrix(A, B))[0][:2].sum() == 0
    r, _ = _pair(A, B)
    assert _bits(r["score"]) == _bits(np.float32(8 / 3)) and r["shift"] == 27 and r["total"] == 16 << 27
    assert np.array_equal(r["partner"], [0, 1, 2, 5, 3, 4])
    # Dmax = 0
    z = np.full((4, 3), 1.5, np.float32)
    r, _ = _pair(z, z[:3])
    assert r["score"] == 0 and r["total"] == 0 and r["shift"] == 0 and np.array_equal(r["partner"], [0, 1, 2, -1]) and not r["partner_dist2"].any()
    # subnormal distances, and distances near the top of the range
    for scale, lo, hi in ((1e-22, 150, 179), (1e18, -97, -60)):
        p = (rng.standard_normal((9, 3)) * scale).astype(np.float32)
        q = (rng.standard_normal((11, 3)) * scale).astype(np.float32)
        r, D = _pair(p, q)
        assert lo <= r["shift"] <= hi and 0 < r["total"] < 2 ** 38 and np.isfinite(r["score"]) and r["score"] > 0
        assert (D.max() < 1.2e-38) == (scale < 1)  # the small ones are subnormal indeed
        assert _bits(_pair(q, p)[0]["score"]) == _bits(r["score"])
    # rows at 1e20: the distances overflow -- not comparable; a NaN row; a segment above the limit
    p, q = rng.standard_normal((5, 3)).astype(np.float32), rng.standard_normal((6, 3)).astype(np.float32)
    p[0, 0], q[0, 0] = 1e20, -1e20
    cases = [(p, q)]
    p2 = p.copy()
    p2[0, 0] = np.nan
    cases += [(p2, q[1:]), (q[1:], p2), (q, rng.standard_normal((129, 3)).astype(np.float32))]
    for u, w in cases:
        r, _ = _pair(u, w)
        assert np.isposinf(r["score"]) and r["total"] == -1 and r["shift"] == 0 and np.all(r["partner"] == -1) and np.all(np.isposinf(r["partner_dist2"]))
    for u, w in ((rng.standard_normal((129, 3)), q), (q[:0], q), (q, q[:0]), (q, q[:, :2]), (q[0], q)):
        with pytest.raises(ValueError):
            _hip.pairing_host(u, w)


# ---- header, ctypes, library, the kernel ----

def test_header_ctypes_and_library_agree(hip_lib):
    import ctypes as C

    from scann import _hip

    h = abi_checks.header()
    abi_checks.declared("int scann_index_pairing(scann_handle_t* h, scann_index_t* idx, const float* q, const int32_t* q_first /* [n_sets + 1] */, int64_t n_sets, "
                        "const int32_t* pair_set, const int32_t* pair_segment, int64_t n_pairs, float* score, int64_t* total, int32_t* shift, "
                        "int32_t* partner_pos, float* partner_dist2);",
                        "int scann_index_pairing_batch(scann_handle_t* h, scann_index_t* idx, scann_dbatch_t* db, const int64_t* query_ids, int32_t measure, "
                        "int32_t shortlist, int32_t k, float* y, float* ga, float* score, int32_t* segment, int64_t* ids, int32_t* sizes, int64_t* total, "
                        "int32_t* shift, float* short_score, int32_t* short_place, int32_t* partner_pos, float* partner_dist2);",
                        "int scann_pairing_host(const float* a, int64_t n, const float* b, int64_t m, int64_t dim, float* score, int64_t* total, int32_t* shift, "
                        "int32_t* partner, float* partner_dist2);",
                        "int scann_pairing_solve_host(const uint32_t* cost, int32_t Q, int32_t* col_of_row, int64_t* total);")
    assert "#define SCANN_PAIRING_MAX_ATOMS %d" % _hip.PAIRING_MAX_ATOMS in h and _hip.PAIRING_MAX_ATOMS == pairing_ref.MAX_ATOMS == 128
    assert "#define SCANN_PAIRING_SOLVE_MAX %d" % _hip.PAIRING_SOLVE_MAX in h
    assert _hip.MATCH_MEASURES == {"chamfer": 0, "hausdorff": 1, "cover": 2}  # the pairing is no fourth measure
    P = C.c_void_p
    sig = abi_checks.signatures({
        "scann_index_pairing": (C.c_int, [P, P, P, P, C.c_int64, P, P, C.c_int64] + [P] * 5),
        "scann_index_pairing_batch": (C.c_int, [P, P, P, P, C.c_int32, C.c_int32, C.c_int32] + [P] * 12),
        "scann_pairing_host": (C.c_int, [P, C.c_int64, P, C.c_int64, C.c_int64] + [P] * 5),
        "scann_pairing_solve_host": (C.c_int, [P, C.c_int32, P, P])})
    for n in ("scann_index_pairing", "scann_index_pairing_batch", "scann_pairing_host", "scann_pairing_solve_host"):
        assert hasattr(hip_lib, n), n
    # the error returns that need no handle
    assert hip_lib.scann_index_pairing(None, None, None, None, 1, None, None, 0, None, None, None, None, None) == -1
    assert hip_lib.scann_index_pairing_batch(None, None, None, None, 0, 32, 5, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    z = np.zeros((2, 3), np.float32)
    assert hip_lib.scann_pairing_host(None, 2, _hip._ptr(z), 2, 3, None, None, None, None, None) == -1
    assert hip_lib.scann_pairing_host(_hip._ptr(z), 2, _hip._ptr(z), 2, 0, None, None, None, None, None) == -1
    assert hip_lib.scann_pairing_host(_hip._ptr(z), 129, _hip._ptr(z), 2, 3, None, None, None, None, None) == -2  # unsupported, as a query structure
    assert hip_lib.scann_pairing_host(_hip._ptr(z), 2, _hip._ptr(z), 2, 3, None, None, None, None, None) == 0    # every output may be NULL
    for bad in (True, 2.5, None, 4, 33):
        with pytest.raises(ValueError):
            _hip.check_pairing_shortlist(bad, 5)
    assert _hip.check_pairing_shortlist(5, 5) == 5 and _hip.check_pairing_shortlist(np.int64(32), 5) == 32


def test_pairing_kernel_uses_no_scratch(hip_lib):
    """the three size classes of pairing_kernel (csrc/scann_pairing.hip) spill nothing, read from the built library's kernel descriptors"""
    from scann import _hip

    kern = {n: v for n, v in abi_checks.device_kernels(_hip.LIB_PATH).items() if "pairing_kernel" in n}
    assert len(kern) == 3, sorted(kern)
    for name, (scratch, vgpr) in kern.items():
        assert scratch == 0, (name, scratch, vgpr)
        for other in ("match_", "knn_", "head_", "pca_", "rbf_", "kmeans_", "rollout_", "shapley_", "kcenter_", "ablate_kernel", "input_grad_kernel"):
            assert other not in name, (name, other)  # (the sibling tests count their kernels by these)


def test_twins_under_the_sanitizers():
    """make asan-pairing: the stand-alone program drives both twins under AddressSanitizer + UBSan"""
    r = subprocess.run(["make", "-C", CSRC, "asan-pairing"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "scann_pairing_check: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- the Python layer over a stand-in engine ----

class _PairStandIn(_MatchStandIn):
    """test_match_host's stand-in with the pairing call: the shortlist by match_ref, the pairs by the host twin, the rerank by pairing_ref"""

    def index_pairing_batch(self, ix, rb, k, shortlist, measure="chamfer", query_ids=None):
        from scann import _hip

        p = rb.packed
        self.calls.append(("pair", measure, k, shortlist, p.n_struct, None if query_ids is None else list(query_ids)))
        rows, _, _ = self._rows(p, _hip.OUT_AFTER_LC, ix.dim)
        D = _hip.knn_dist2_matrix(rows, ix.rows) if len(ix.rows) else np.zeros((len(rows), 0), np.float32)
        sl = match_ref.match(D, p.mol_offset, ix.ids, shortlist, measure, query_ids=query_ids)
        first, count, sid = match_ref.segments(ix.ids)
        B, A = p.n_struct, p.n_atom
        out = {"y": (10.0 + np.arange(B) + self.seen).astype(np.float32), "ga": np.zeros(A, np.float32), "score": np.full((B, k), np.inf, np.float32),
               "segment": np.full((B, k), -1, np.int32), "id": np.full((B, k), -1, np.int64), "size": np.zeros((B, k), np.int32),
               "total": np.full((B, k), -1, np.int64), "shift": np.zeros((B, k), np.int32), "short_score": np.full((B, k), np.inf, np.float32),
               "short_place": np.full((B, k), -1, np.int32), "partner_position": np.full((A, k), -1, np.int32),
               "partner_dist2": np.full((A, k), np.inf, np.float32)}
        for s in range(B):
            a0, a1 = p.mol_offset[s], p.mol_offset[s + 1]
            segs = sl["segment"][s]
            res = [_hip.pairing_host(rows[a0:a1], ix.rows[first[g]:first[g] + count[g]]) if g >= 0 else None for g in segs]
            places = pairing_ref.rerank(segs, sl["score"][s], [np.inf if r is None else r["score"] for r in res], k)
            for j, pl in enumerate(places):
                if pl < 0:
                    continue
                g, r = segs[pl], res[pl]
                out["score"][s, j], out["segment"][s, j], out["id"][s, j], out["size"][s, j] = r["score"], g, sid[g], count[g]
                out["total"][s, j], out["shift"][s, j], out["short_score"][s, j], out["short_place"][s, j] = r["total"], r["shift"], sl["score"][s, pl], pl
                out["partner_position"][a0:a1, j] = np.where(r["partner"] >= 0, first[g] + r["partner"], -1)
                out["partner_dist2"][a0:a1, j] = r["partner_dist2"]
        self.seen += B
        return out


def _model(cfg):
    return abi_checks.stand_in_model(cfg, _PairStandIn)


def _batch(n=5, seed=2):
    cfg = so.default_config("qm9")
    inputs, _ = so.pad_batch(*so.synth_dataset(n, seed), g_update=True)
    return cfg, inputs


def test_bad_arguments_raise_before_any_upload(hip_lib):
    from scann import _hip

    cfg, inputs = _batch(3)
    m = _model(cfg)
    atoms = m.build_index(inputs, level="atom")
    structs = m.build_index(inputs, level="structure")
    up = m.engine.uploads
    m.engine.calls.clear()
    for kw in (dict(k=0), dict(k=33), dict(k=2.5), dict(k=True), dict(measure="euclid"), dict(measure=3), dict(measure=None), dict(batch_size=0),
               dict(exclude_ids=[1, 2]), dict(exclude_ids=[1, 2, 3, 4]), dict(shortlist=4), dict(shortlist=33), dict(shortlist=8.0), dict(shortlist=None),
               dict(k=9, shortlist=8)):
        with pytest.raises(ValueError):
            m.pair_structures(inputs, atoms, **kw)
    with pytest.raises(ValueError, match="atom-level"):
        m.pair_structures(inputs, structs)
    with pytest.raises(ValueError):
        m.pair_structures(inputs, "not an index")
    with pytest.raises(ValueError):
        _model(so.default_config("qm9")).pair_structures(inputs, atoms)  # another model's index
    big = {k: np.array(v) for k, v in inputs.items()}
    B, M = np.shape(big["neighbors"])[:2]
    reps = -(-(_hip.PAIRING_MAX_ATOMS + 1) // M)
    big = {k: np.concatenate([v] * reps, axis=1) for k, v in big.items()}
    big["atom_mask"][:] = 0
    big["atom_mask"][1, :_hip.PAIRING_MAX_ATOMS + 1] = 1
    with pytest.raises(ValueError, match="structure 1 has %d atoms" % (_hip.PAIRING_MAX_ATOMS + 1)):
        m.pair_structures(big, atoms)
    with pytest.raises(ValueError, match="structure 1 has %d atoms" % (_hip.PAIRING_MAX_ATOMS + 1)):
        m.align_structures(big, inputs)
    with pytest.raises(ValueError, match="3 structures against 2"):
        m.align_structures(inputs, {k: np.asarray(v)[:2] for k, v in inputs.items()})
    with pytest.raises(ValueError):
        m.align_structures(inputs, inputs, batch_size=0)
    assert m.engine.uploads == up and not m.engine.calls


def test_chunks_repadding_surplus_and_leave_one_out(hip_lib):
    from scann import _hip

    cfg, inputs = _batch(5, seed=3)
    m = _model(cfg)
    ids = [40, 41, 42, 43, 44]
    ix = m.build_index(inputs, level="atom", ids=ids, batch_size=2)
    amask = np.asarray(inputs["atom_mask"]).reshape(5, -1) != 0
    cnt = amask.sum(1)
    m.engine.calls.clear()
    m.engine.seen = 0  # the queries are the indexed structures again
    r = m.pair_structures(inputs, ix, k=2, shortlist=4, batch_size=2)
    assert [c[4] for c in m.engine.calls] == [2, 2, 1] and all(c[:4] == ("pair", 0, 2, 4) and c[5] is None for c in m.engine.calls)
    B, M = amask.shape
    assert sorted(r) == ["distance", "neighbor_id", "neighbor_size", "paired_atom", "paired_distance", "predict_property", "shortlist_distance",
                         "shortlist_place", "surplus"]
    for key in ("distance", "neighbor_id", "neighbor_size", "shortlist_distance", "shortlist_place", "surplus"):
        assert r[key].shape == (B, 2), key
    assert r["paired_atom"].shape == (B, M, 2) and r["paired_distance"].shape == (B, M, 2) and r["predict_property"].shape == (B, 1)
    assert r["distance"].dtype == np.float32 and r["neighbor_id"].dtype == np.int64 and r["paired_atom"].dtype == np.int32 and r["surplus"].dtype == np.int32
    assert np.array_equal(r["predict_property"][:, 0], 10.0 + np.arange(5))
    # every structure finds itself: distance 0, the identity map, nothing surplus, first in the shortlist too
    assert np.array_equal(r["neighbor_id"][:, 0], ids) and not r["distance"][:, 0].any() and np.array_equal(r["neighbor_size"][:, 0], cnt)
    assert not r["surplus"][:, 0].any() and not r["shortlist_place"][:, 0].any() and not r["shortlist_distance"][:, 0].any()
    assert np.array_equal(r["surplus"], cnt[:, None] - r["neighbor_size"])
    for b in range(B):
        pos = np.nonzero(amask[b])[0]
        assert np.array_equal(r["paired_atom"][b, pos, 0], np.arange(len(pos))) and not r["paired_distance"][b, pos, 0].any()
        assert np.all(r["paired_atom"][b, ~amask[b]] == -1) and not r["paired_distance"][b, ~amask[b]].any()
        # the second neighbour: one to one, and exactly max(n - m, 0) atoms surplus
        second = r["paired_atom"][b, pos, 1]
        real = second[second >= 0]
        assert len(set(real.tolist())) == len(real) == min(cnt[b], r["neighbor_size"][b, 1]) and np.all(real < r["neighbor_size"][b, 1])
        assert int((second < 0).sum()) == max(int(r["surplus"][b, 1]), 0)
    # leave-one-out; a PackedBatch gives packed arrays; k above what is left: the tail
    m.engine.seen = 0
    pk = _hip.pack_inputs(inputs)
    pk = _hip.PackedBatch(pk.atomic, pk.mol_offset, pk.edge_offset, pk.edge_col, pk.edge_dist, pk.edge_weight)
    p = m.pair_structures(pk, ix, k=5, shortlist=5, measure="hausdorff", exclude_ids=ids, batch_size=3)
    assert [c[5] for c in m.engine.calls[-2:]] == [[40, 41, 42], [43, 44]] and m.engine.calls[-1][1] == 1
    assert p["paired_atom"].shape == (cnt.sum(), 5) and p["paired_distance"].shape == (cnt.sum(), 5)
    assert not np.any(p["neighbor_id"] == np.array(ids)[:, None]) and np.all(p["distance"][:, 0] > 0)
    assert np.all(p["neighbor_id"][:, 4] == -1) and np.all(np.isinf(p["distance"][:, 4])) and np.all(p["neighbor_size"][:, 4] == 0)
    assert np.all(p["paired_atom"][:, 4] == -1) and np.all(np.isinf(p["paired_distance"][:, 4])) and not p["surplus"][:, 4].any()
    assert np.all(p["shortlist_place"][:, 4] == -1) and np.all(np.isinf(p["shortlist_distance"][:, 4]))
    assert np.all(np.diff(p["distance"][:, :4], axis=1) >= 0)  # ranked by the pairing score


def test_scann_facade_denormalises_the_predictions_only(hip_lib):
    from scann.models.scann_model import FACADE, SCANN

    assert "pair_structures" not in dict(FACADE) and "align_structures" not in dict(FACADE)  # written by hand
    assert SCANN.pair_structures.__qualname__ == "SCANN.pair_structures" and SCANN.align_structures.__qualname__ == "SCANN.align_structures"
    cfg, inputs = _batch(3)
    s = SCANN.__new__(SCANN)
    s.model = _model(cfg)
    s.mean, s.std = 2.0, -0.5
    ix = s.build_index(inputs, level="atom")
    s.model.engine.seen = 0
    raw = s.model.pair_structures(inputs, ix, k=2, shortlist=3, measure="cover")
    s.model.engine.seen = 0
    got = s.pair_structures(inputs, ix, k=2, shortlist=3, measure="cover")
    assert np.array_equal(got["predict_property"], raw["predict_property"] * -0.5 + 2.0)
    for k in raw:
        if k != "predict_property":
            assert np.array_equal(got[k], raw[k]), k
    # align_structures: both predictions, nothing else
    fake = {"distance": np.ones(3, np.float32), "atom_map": np.zeros((3, 4), np.int32), "predict_property": np.ones((3, 1), np.float32),
            "predict_property_b": np.full((3, 1), 3, np.float32)}
    s.model.align_structures = lambda a, b, batch_size=None: {k: v.copy() for k, v in fake.items()}
    got = s.align_structures(inputs, inputs)
    assert np.array_equal(got["predict_property"], fake["predict_property"] * -0.5 + 2.0)
    assert np.array_equal(got["predict_property_b"], fake["predict_property_b"] * -0.5 + 2.0)
    assert np.array_equal(got["distance"], fake["distance"]) and np.array_equal(got["atom_map"], fake["atom_map"])


def test_predict_model_cli_takes_pair():
    pytest.importorskip("sklearn")
    spec = importlib.util.spec_from_file_location("predict_model_cli_pair", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parser().parse_args(["some_dir", "--pair", "5", "--pair-shortlist", "16", "--pair-measure", "cover", "--pair-index", "atoms.npz"])
    assert a.pair == 5 and a.pair_shortlist == 16 and a.pair_measure == "cover" and a.pair_index == "atoms.npz"
    d = cli.parser().parse_args(["some_dir"])
    assert d.pair == 0 and d.pair_shortlist == 32 and d.pair_measure == "chamfer" and d.pair_index == "" and d.match == 0
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--pair-measure", "euclid"])
    with pytest.raises(SystemExit):
        cli.main(cli.parser().parse_args(["some_dir", "--pair", "33"]))
    with pytest.raises(SystemExit):
        cli.main(cli.parser().parse_args(["some_dir", "--pair", "5", "--pair-shortlist", "4"]))
    with pytest.raises(SystemExit):
        cli.main(cli.parser().parse_args(["some_dir", "--pair", "5", "--pair-shortlist", "33"]))
