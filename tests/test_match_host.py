"""Structure matching over a latent-space index (scann_index_match) -- what needs no GPU: the host twin scann_match_parts_host against the
NumPy definition of tests/match_ref.py on the host twin's distances, bit for bit (planted NaN / inf rows, duplicate rows, sets and
segments of one row); the bitwise symmetry of Chamfer and Hausdorff; the segment rule; the selection under (score, segment) with ids and
exclusion; and the Python layer (argument checks before any upload, chunking, re-padding, the facade) over a stand-in engine."""
import importlib.util
import os

import numpy as np
import pytest

import abi_checks
import match_ref
import scann_oracle as so
from test_knn_host import _StandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _sets(rng, sizes, dim, scale=1.0):
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return (rng.standard_normal((int(first[-1]), dim)) * scale).astype(np.float32), first


# ---- the host twin against the definition ----

@pytest.mark.parametrize("dim", [128, 64, 130, 3])
def test_host_twin_is_the_definition_bit_for_bit(hip_lib, dim):
    from scann import _hip

    rng = np.random.default_rng(dim)
    q, q_first = _sets(rng, [1, 2, 17, 1, 64, 5], dim)
    rows, seg_first = _sets(rng, [1, 1, 9, 63, 1, 30, 2], dim)
    rows[40] = q[20]           # a query row itself (set 3, one atom): f = 0
    rows[[11, 12, 50]] = rows[5]  # duplicate rows: the witness is the least position
    rows[20, 2] = np.nan       # a NaN row inside a segment
    rows[75, 0] = np.inf       # an inf row: its distances are +inf, which count
    rows[0] = np.nan           # a one-row segment that is all NaN: nothing counts
    q[25, 1] = np.nan          # a NaN query atom (set 4)
    D = _hip.knn_dist2_matrix(q, rows)
    parts = _hip.match_parts_host(q, q_first, rows, seg_first)
    ids = np.repeat(np.arange(len(seg_first) - 1), np.diff(seg_first))
    ref = match_ref.match(D, q_first, ids, 3, "chamfer")
    assert parts.shape == ref["all_parts"].shape == (6, 7, 4)
    assert np.array_equal(_bits(parts), _bits(ref["all_parts"]))
    assert not np.isnan(parts).any()
    # what was planted shows: a NaN atom makes F and Fmax of its set +inf, the all-NaN segment makes everything +inf
    assert np.all(np.isinf(parts[4, :, 0])) and np.all(np.isinf(parts[4, :, 2])) and np.all(np.isinf(parts[:, 0]))
    assert np.isinf(parts[0, 3, 1]) and np.isinf(parts[0, 3, 3]) and np.isfinite(parts[0, 3, 0])  # the NaN row of segment 3: g = +inf
    assert parts[3, 3, 0] == 0 and parts[3, 3, 2] == 0  # set 3 is one atom, and segment 3 holds it
    # the witnesses of the reference against a plain walk
    for s in range(6):
        for g in range(7):
            blk = D[q_first[s]:q_first[s + 1], seg_first[g]:seg_first[g + 1]]
            _, _, _, f, wf, gg, wg = match_ref.pair(blk)
            for i in range(blk.shape[0]):
                assert match_ref.nanmin_with_witness(blk[i]) == (f[i], wf[i])
            for j in range(blk.shape[1]):
                assert match_ref.nanmin_with_witness(blk[:, j]) == (gg[j], wg[j])
    assert match_ref.pair(np.array([[1, 0, 0, 2]], np.float32))[4][0] == 1  # among equal distances the least position
    assert match_ref.pair(D[q_first[0]:q_first[1], 11:13])[4][0] == 0  # rows 11 and 12 are duplicates


def test_chamfer_and_hausdorff_are_symmetric_bit_for_bit(hip_lib):
    from scann import _hip

    rng = np.random.default_rng(11)
    for dim in (128, 130, 7):
        a, a_first = _sets(rng, [3, 1, 32, 20, 7], dim, 2.0)
        b, b_first = _sets(rng, [5, 19, 1, 40], dim, 2.0)
        b[6] = a[1]
        ab = _hip.match_parts_host(a, a_first, b, b_first)
        ba = _hip.match_parts_host(b, b_first, a, a_first)
        # the roles swapped: F <-> G, Fmax <-> Gmax
        assert np.array_equal(_bits(ab[..., [1, 0, 3, 2]]), _bits(ba.transpose(1, 0, 2)))
        Dab, Dba = _hip.knn_dist2_matrix(a, b), _hip.knn_dist2_matrix(b, a)
        assert np.array_equal(_bits(Dab), _bits(Dba.T))
        for measure in ("chamfer", "hausdorff"):
            for s in range(5):
                for g in range(4):
                    x = match_ref.pair(Dab[a_first[s]:a_first[s + 1], b_first[g]:b_first[g + 1]])
                    y = match_ref.pair(Dba[b_first[g]:b_first[g + 1], a_first[s]:a_first[s + 1]])
                    sx, sy = match_ref.score_of(measure, x[0], x[1], x[2]), match_ref.score_of(measure, y[0], y[1], y[2])
                    assert _bits(sx) == _bits(sy), (measure, s, g)
        x = match_ref.pair(Dab[a_first[2]:a_first[3], b_first[1]:b_first[2]])
        assert match_ref.score_of("cover", x[0], x[1], x[2]) != match_ref.score_of("cover", x[0], x[2], x[1])  # the directed form is not


def test_segments_are_the_maximal_runs_of_one_id():
    f, c, i = match_ref.segments([7, 7, 7, 3, 7, 7, 5, 5, 3])  # returning ids give new segments
    assert np.array_equal(f, [0, 3, 4, 6, 8]) and np.array_equal(c, [3, 1, 2, 2, 1]) and np.array_equal(i, [7, 3, 7, 5, 3])
    from scann.models import LatentIndex

    ix = LatentIndex(_model(so.default_config("qm9")), "atom")  # LatentIndex.segments hands the engine's table through
    ix.add_rows(np.zeros((5, 128), np.float32), ids=[7, 7, 3, 7, 7]).add_rows(np.zeros((4, 128), np.float32), ids=[7, 5, 5, 3])
    f, c, i = ix.segments()
    assert np.array_equal(f, [0, 2, 3, 6, 8]) and np.array_equal(c, [2, 1, 3, 2, 1]) and np.array_equal(i, [7, 3, 7, 5, 3])
    f, c, i = match_ref.segments([4])
    assert np.array_equal(f, [0]) and np.array_equal(c, [1]) and np.array_equal(i, [4])
    f, c, i = match_ref.segments([])
    assert len(f) == len(c) == len(i) == 0
    f, c, i = match_ref.segments(np.arange(5))
    assert np.array_equal(f, np.arange(5)) and np.all(c == 1)
    f, c, i = match_ref.segments([2, 2, 2, 2])
    assert np.array_equal(f, [0]) and np.array_equal(c, [4])


def test_selection_order_ties_exclusion_and_the_tail():
    from scann import _hip

    assert match_ref.MEASURES == _hip.MATCH_MEASURES
    # one query atom against one-row segments: the score is the distance (cover) or twice it (chamfer)
    D = np.array([[4, 1, 1, np.nan, 0.5, 1]], np.float32)
    ids = np.array([10, 11, 12, 13, 14, 11])
    r = match_ref.match(D, [0, 1], ids, 8, "cover")
    assert np.array_equal(r["segment"][0], [4, 1, 2, 5, 0, 3, -1, -1])  # ties to the earlier segment, the NaN segment last (+inf), the tail
    assert np.array_equal(r["score"][0, :5], np.array([0.5, 1, 1, 1, 4], np.float32)) and np.all(np.isinf(r["score"][0, 5:]))
    assert np.array_equal(r["id"][0], [14, 11, 12, 11, 10, 13, -1, -1]) and np.array_equal(r["size"][0], [1, 1, 1, 1, 1, 1, 0, 0])
    assert np.array_equal(r["match_position"][0], [4, 1, 2, 5, 0, -1, -1, -1]) and np.isinf(r["match_dist2"][0, 5])
    assert np.all(np.isinf(r["parts"][0, 6:]))
    c = match_ref.match(D, [0, 1], ids, 3, "chamfer")
    assert np.array_equal(c["score"][0], np.array([1, 2, 2], np.float32)) and np.array_equal(c["segment"][0], [4, 1, 2])
    x = match_ref.match(D, [0, 1], ids, 3, "hausdorff", query_ids=[11])  # both runs of id 11 are skipped
    assert np.array_equal(x["segment"][0], [4, 2, 0])
    e = match_ref.match(D, [0, 1], np.full(6, 3), 2, "cover", query_ids=[3])
    assert np.all(e["segment"] == -1) and np.all(np.isinf(e["score"])) and np.all(e["match_position"] == -1)
    z = match_ref.match(np.zeros((2, 0), np.float32), [0, 2], [], 2, "cover")
    assert np.all(z["segment"] == -1) and np.all(z["size"] == 0)


def test_measures_on_a_pair_worked_by_hand(hip_lib):
    from scann import _hip

    D = np.array([[1, 4, 9], [16, 2, 25]], np.float32)  # f = 1, 2; g = 1, 2, 9
    parts, F, G, f, wf, g, wg = match_ref.pair(D)
    assert F == 1.5 and G == 4.0 and np.array_equal(parts, np.array([1.5, 4.0, 2, 9], np.float32))
    assert np.array_equal(wf, [0, 1]) and np.array_equal(wg, [0, 1, 0])
    assert match_ref.score_of("chamfer", parts, F, G) == 5.5 and match_ref.score_of(1, parts, F, G) == 9 and match_ref.score_of("cover", parts, F, G) == 1.5
    # points on a line: atoms at 0 and 10, rows at 1, 12 and 3 -> D = [[1, 144, 9], [81, 4, 49]], f = 1, 4, g = 1, 4, 9
    got = _hip.match_parts_host(np.array([[0], [10]], np.float32), [0, 2], np.array([[1], [12], [3]], np.float32), [0, 3])[0, 0]
    assert np.array_equal(got, np.array([2.5, np.float32(14 / 3), 4, 9], np.float32))


def test_argument_checks_of_the_bindings(hip_lib):
    from scann import _hip

    assert [_hip.check_match_measure(m) for m in ("chamfer", "hausdorff", "cover", 0, 1, 2, np.int32(2))] == [0, 1, 2, 0, 1, 2, 2]
    for bad in ("euclid", 3, -1, None, True, 1.0, "Chamfer"):
        with pytest.raises(ValueError):
            _hip.check_match_measure(bad)
    q, rows = np.zeros((4, 8), np.float32), np.zeros((5, 8), np.float32)
    assert _hip.match_parts_host(q, [0, 1, 4], rows, [0, 5]).shape == (2, 1, 4)
    for qf, sf in (([0, 4, 4], [0, 5]), ([1, 4], [0, 5]), ([0, 3], [0, 5]), ([0, 4], [0, 2, 2, 5]), ([0, 2, 1, 4], [0, 5]), ([0], [0, 5]), ([0, 4], [0, 6])):
        with pytest.raises(ValueError):
            _hip.match_parts_host(q, qf, rows, sf)
    with pytest.raises(ValueError):
        _hip.match_parts_host(q, [0, 4], np.zeros((5, 7), np.float32), [0, 5])
    assert hip_lib.scann_match_parts_host(None, None, 1, None, None, 1, 8, None) == -1
    assert hip_lib.scann_index_segments(None, None, None, None) == -1
    assert hip_lib.scann_index_match(None, None, None, None, 1, None, 0, 5, None, None, None, None, None, None, None) == -1
    assert hip_lib.scann_index_match_batch(None, None, None, None, 0, 5, None, None, None, None, None, None, None, None, None) == -1


def test_header_ctypes_and_library_agree(hip_lib):
    import ctypes as C

    from scann import _hip

    h = abi_checks.header()
    abi_checks.declared("int64_t scann_index_segments(const scann_index_t* idx, int64_t* first, int32_t* count, int64_t* id);",
                        "int scann_index_match(scann_handle_t* h, scann_index_t* idx, const float* q, const int32_t* q_first /* [n_sets + 1] */, int64_t n_sets, "
                        "const int64_t* query_ids, int32_t measure, int32_t k, float* score, int32_t* segment, int64_t* ids, int32_t* sizes, float* parts, "
                        "int32_t* match_pos, float* match_dist2);",
                        "int scann_index_match_batch(scann_handle_t* h, scann_index_t* idx, scann_dbatch_t* db, const int64_t* query_ids, int32_t measure, "
                        "int32_t k, float* y, float* ga, float* score, int32_t* segment, int64_t* ids, int32_t* sizes, float* parts, int32_t* match_pos, "
                        "float* match_dist2);")
    for name, v in _hip.MATCH_MEASURES.items():
        assert "#define SCANN_MATCH_%s %d" % (name.upper(), v) in h
    assert "#define SCANN_MATCH_MAX_ATOMS %d" % _hip.MATCH_MAX_ATOMS in h and _hip.MATCH_MAX_ATOMS >= 128
    P = C.c_void_p
    sig = abi_checks.signatures({
        "scann_index_segments": (C.c_int64, [P, P, P, P]),
        "scann_index_match": (C.c_int, [P, P, P, P, C.c_int64, P, C.c_int32, C.c_int32] + [P] * 7),
        "scann_index_match_batch": (C.c_int, [P, P, P, P, C.c_int32, C.c_int32] + [P] * 9),
        "scann_match_parts_host": (C.c_int, [P, P, C.c_int64, P, P, C.c_int64, C.c_int64, P])})
    for n in ("scann_index_segments", "scann_index_match", "scann_index_match_batch", "scann_match_parts_host"):
        assert hasattr(hip_lib, n), n


def test_match_kernels_use_no_scratch(hip_lib):
    """the tile kernel and the pair kernel of csrc/scann_match.hip spill nothing, read from the built library's kernel descriptors"""
    from scann import _hip

    kern = {n: v for n, v in abi_checks.device_kernels(_hip.LIB_PATH).items() if "match_" in n}
    assert len(kern) == 2 and sum("match_tile_kernel" in n for n in kern) == 1 and sum("match_pair_kernel" in n for n in kern) == 1, sorted(kern)
    for name, (scratch, vgpr) in kern.items():
        assert scratch == 0, (name, scratch, vgpr)


# ---- the Python layer over a stand-in engine ----

class _MatchStandIn(_StandIn):
    """test_knn_host's stand-in (atom rows [s, a, 0, ...]) with the matching calls, answered by match_ref on the host twin's distances"""

    def index_names(self, ix):
        return ix.ids.copy(), ix.atoms.copy()

    def index_segments(self, ix):
        return match_ref.segments(ix.ids)

    def index_match_batch(self, ix, rb, k, measure="chamfer", query_ids=None):
        from scann import _hip

        p = rb.packed
        self.calls.append(("match", measure, k, p.n_struct, None if query_ids is None else list(query_ids)))
        rows, _, _ = self._rows(p, _hip.OUT_AFTER_LC, ix.dim)
        D = _hip.knn_dist2_matrix(rows, ix.rows) if len(ix.rows) else np.zeros((len(rows), 0), np.float32)
        out = match_ref.match(D, p.mol_offset, ix.ids, k, measure, query_ids=query_ids)
        out["y"], out["ga"] = (10.0 + np.arange(p.n_struct) + self.seen).astype(np.float32), np.zeros(p.n_atom, np.float32)
        self.seen += p.n_struct
        return out


def _model(cfg):
    return abi_checks.stand_in_model(cfg, _MatchStandIn)


def _batch(n=5, seed=2):
    cfg = so.default_config("qm9")
    inputs, _ = so.pad_batch(*so.synth_dataset(n, seed), g_update=True)
    return cfg, inputs


def test_bad_arguments_raise_before_any_upload(hip_lib):
    cfg, inputs = _batch(3)
    m = _model(cfg)
    atoms = m.build_index(inputs, level="atom")
    structs = m.build_index(inputs, level="structure")
    up = m.engine.uploads
    m.engine.calls.clear()
    for kw in (dict(k=0), dict(k=33), dict(k=2.5), dict(k=True), dict(measure="euclid"), dict(measure=3), dict(measure=None), dict(batch_size=0),
               dict(exclude_ids=[1, 2]), dict(exclude_ids=[1, 2, 3, 4])):
        with pytest.raises(ValueError):
            m.match_structures(inputs, atoms, **kw)
    with pytest.raises(ValueError, match="atom-level"):
        m.match_structures(inputs, structs)
    with pytest.raises(ValueError):
        m.match_structures(inputs, "not an index")
    with pytest.raises(ValueError):
        _model(so.default_config("qm9")).match_structures(inputs, atoms)  # another model's index
    # a structure above the atom limit is named
    from scann import _hip

    big = {k: np.array(v) for k, v in inputs.items()}
    B, M = np.shape(big["neighbors"])[:2]
    reps = -(-(_hip.MATCH_MAX_ATOMS + 1) // M)
    big = {k: np.concatenate([v] * reps, axis=1) for k, v in big.items()}
    big["atom_mask"][:] = 0
    big["atom_mask"][1, :_hip.MATCH_MAX_ATOMS + 1] = 1
    with pytest.raises(ValueError, match="structure 1 has %d atoms" % (_hip.MATCH_MAX_ATOMS + 1)):
        m.match_structures(big, atoms)
    assert m.engine.uploads == up and not m.engine.calls


def test_chunks_repadding_and_leave_one_out(hip_lib):
    from scann import _hip

    cfg, inputs = _batch(5, seed=3)
    m = _model(cfg)
    ix = m.build_index(inputs, level="atom", ids=[40, 41, 42, 43, 44], batch_size=2)
    amask = np.asarray(inputs["atom_mask"]).reshape(5, -1) != 0
    cnt = amask.sum(1)
    first, count, sid = ix.segments()
    assert np.array_equal(sid, [40, 41, 42, 43, 44]) and np.array_equal(count, cnt) and np.array_equal(first, np.concatenate([[0], np.cumsum(cnt)[:-1]]))
    m.engine.calls.clear()
    m.engine.seen = 0  # the queries are the indexed structures again
    r = m.match_structures(inputs, ix, k=2, batch_size=2)
    assert [c[3] for c in m.engine.calls] == [2, 2, 1] and all(c[1] == 0 and c[4] is None for c in m.engine.calls)
    B, M = amask.shape
    assert sorted(r) == ["distance", "matched_atom", "matched_distance", "neighbor_id", "neighbor_size", "parts", "predict_property"]
    assert r["distance"].shape == (B, 2) and r["neighbor_id"].shape == (B, 2) and r["neighbor_size"].shape == (B, 2) and r["parts"].shape == (B, 2, 4)
    assert r["matched_atom"].shape == (B, M, 2) and r["matched_distance"].shape == (B, M, 2) and r["predict_property"].shape == (B, 1)
    assert r["distance"].dtype == np.float32 and r["neighbor_id"].dtype == np.int64 and r["matched_atom"].dtype == np.int32
    assert np.array_equal(r["predict_property"][:, 0], 10.0 + np.arange(5))
    # every structure finds itself: distance 0, its own atoms in order
    assert np.array_equal(r["neighbor_id"][:, 0], [40, 41, 42, 43, 44]) and not r["distance"][:, 0].any() and np.array_equal(r["neighbor_size"][:, 0], cnt)
    for b in range(B):
        pos = np.nonzero(amask[b])[0]
        assert np.array_equal(r["matched_atom"][b, pos, 0], np.arange(len(pos))) and not r["matched_distance"][b, pos, 0].any()
        assert np.all(r["matched_atom"][b, ~amask[b]] == -1) and not r["matched_distance"][b, ~amask[b]].any()
    # leave-one-out; a PackedBatch gives packed arrays; k above what is left: the tail
    m.engine.seen = 0
    pk = _hip.pack_inputs(inputs)
    pk = _hip.PackedBatch(pk.atomic, pk.mol_offset, pk.edge_offset, pk.edge_col, pk.edge_dist, pk.edge_weight)
    p = m.match_structures(pk, ix, k=5, measure="hausdorff", exclude_ids=[40, 41, 42, 43, 44], batch_size=3)
    assert [c[4] for c in m.engine.calls[-2:]] == [[40, 41, 42], [43, 44]] and m.engine.calls[-1][1] == 1
    assert p["matched_atom"].shape == (cnt.sum(), 5) and p["matched_distance"].shape == (cnt.sum(), 5)
    assert not np.any(p["neighbor_id"] == np.array([40, 41, 42, 43, 44])[:, None]) and np.all(p["distance"][:, 0] > 0)
    assert np.all(p["neighbor_id"][:, 4] == -1) and np.all(np.isinf(p["distance"][:, 4])) and np.all(p["neighbor_size"][:, 4] == 0)
    assert np.all(p["matched_atom"][:, 4] == -1) and np.all(np.isinf(p["matched_distance"][:, 4]))


def test_scann_facade_denormalises_the_prediction_only(hip_lib):
    from scann.models.scann_model import SCANN

    cfg, inputs = _batch(3)
    s = SCANN.__new__(SCANN)
    s.model = _model(cfg)
    s.mean, s.std = 2.0, -0.5
    ix = s.build_index(inputs, level="atom")
    s.model.engine.seen = 0
    raw = s.model.match_structures(inputs, ix, k=2, measure="cover")
    s.model.engine.seen = 0
    got = s.match_structures(inputs, ix, k=2, measure="cover")
    assert np.array_equal(got["predict_property"], raw["predict_property"] * -0.5 + 2.0)
    for k in ("distance", "neighbor_id", "neighbor_size", "parts", "matched_atom", "matched_distance"):
        assert np.array_equal(got[k], raw[k]), k


def test_predict_model_cli_takes_match():
    pytest.importorskip("sklearn")
    spec = importlib.util.spec_from_file_location("predict_model_cli_match", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parser().parse_args(["some_dir", "--match", "5", "--match-measure", "cover", "--match-index", "atoms.npz"])
    assert a.match == 5 and a.match_measure == "cover" and a.match_index == "atoms.npz"
    d = cli.parser().parse_args(["some_dir"])
    assert d.match == 0 and d.match_measure == "chamfer" and d.match_index == ""
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--match-measure", "euclid"])
    with pytest.raises(SystemExit):
        cli.main(cli.parser().parse_args(["some_dir", "--match", "33"]))
