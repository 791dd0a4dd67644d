"""Host tests of the latent-space index (scann_index_*, HipModel.build_index / nearest, LatentIndex): the host twin of the kernel's
distance chain against fp64 within the derived bound, near-duplicates and identical rows included; the selection reference (ties by
position, exclude ids, fewer than k rows); the Python layer on a stand-in engine (argument errors before any upload, re-padding to
[B, M, k], slicing by batch_size, save / load round trip, de-normalisation); header, ctypes table and library agree; the kernels use no
scratch; predict_model.py takes --nearest.  No GPU."""
import importlib.util
import os
import types

import numpy as np
import pytest

import abi_checks
import knn_ref
import scann_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the distance chain ----

@pytest.mark.parametrize("dim", [1, 3, 128, 130, 1024])
def test_host_twin_against_fp64_within_the_bound(hip_lib, dim):
    from scann import _hip

    rng = np.random.default_rng(dim)
    q = rng.standard_normal((24, dim)).astype(np.float32)
    far = rng.standard_normal((40, dim)).astype(np.float32) * np.float32(3.0)
    near = (q[:16] + np.float32(1e-3) * rng.standard_normal((16, dim)).astype(np.float32)).astype(np.float32)  # near-duplicates of queries 0 .. 15
    rows = np.concatenate([far, near, q[:8]])  # ... and queries 0 .. 7 themselves
    got = _hip.knn_dist2_matrix(q, rows)
    ref = knn_ref.dist2_f64(q, rows)
    assert got.dtype == np.float32 and got.shape == (24, 64)
    for i in range(8):
        assert got[i, 56 + i] == 0.0  # an identical row: exactly 0
    nz = ref > 0
    err = float(np.max(np.abs(got.astype(np.float64) - ref)[nz] / ref[nz]))
    print("dim %d: largest relative error %.3e = %.2f of the bound %.3e" % (dim, err, err / knn_ref.chain_bound(dim), knn_ref.chain_bound(dim)))
    assert err <= knn_ref.chain_bound(dim)
    assert np.array_equal(got == 0, ref == 0)
    # the near-duplicates: the bound holds on exactly the pairs the product form loses
    nd = np.array([[i, 40 + i] for i in range(16)])
    e_nd = np.abs(got[nd[:, 0], nd[:, 1]].astype(np.float64) - ref[nd[:, 0], nd[:, 1]]) / ref[nd[:, 0], nd[:, 1]]
    assert np.max(e_nd) <= knn_ref.chain_bound(dim)
    # one pair through the scalar entry point: the same bits; and the chain written out in NumPy fp32 (no fused multiply-add there, so
    # only for values whose squares are exact: small integers)
    for i, r in ((0, 0), (3, 43), (5, 61)):
        assert _hip.knn_dist2(q[i], rows[r]).view(np.uint32) == got[i, r].view(np.uint32)
    a = rng.integers(-8, 9, (5, dim)).astype(np.float32)
    b = rng.integers(-8, 9, (7, dim)).astype(np.float32)
    assert np.array_equal(_hip.knn_dist2_matrix(a, b), ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1).astype(np.float32))


def test_product_form_loses_the_near_duplicates():
    """why the kernel is not a matrix product: |q|^2 + |r|^2 - 2 q.r in fp32 on near-duplicates has no correct digit"""
    rng = np.random.default_rng(0)
    q = rng.standard_normal((64, 128)).astype(np.float32) * np.float32(4.0)
    r = (q + np.float32(1e-3) * rng.standard_normal(q.shape).astype(np.float32)).astype(np.float32)
    ref = ((q.astype(np.float64) - r.astype(np.float64)) ** 2).sum(-1)
    prod = (q * q).sum(-1, dtype=np.float32) + (r * r).sum(-1, dtype=np.float32) - np.float32(2) * (q * r).sum(-1, dtype=np.float32)
    assert float(np.max(np.abs(prod.astype(np.float64) - ref) / ref)) > 0.1


# ---- the selection reference ----

def test_selection_ties_exclusion_and_short_lists():
    d = np.array([[3.0, 1.0, 1.0, 0.5, 1.0, np.nan, 7.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    ids = np.array([10, 11, 12, 13, 11, 15, 16])
    atoms = np.array([0, 1, 2, 3, 4, 5, 6], dtype=np.int32)
    od, op, oi, oa = knn_ref.select(d, 4, ids=ids, atoms=atoms)
    assert np.array_equal(op, [[3, 1, 2, 4], [0, 1, 2, 3]])  # ties by position
    assert np.array_equal(od[0], np.array([0.5, 1, 1, 1], np.float32)) and np.array_equal(oi[0], [13, 11, 12, 11]) and np.array_equal(oa[0], [3, 1, 2, 4])
    od, op, oi, oa = knn_ref.select(d, 4, ids=ids, atoms=atoms, query_ids=np.array([11, 99]))
    assert np.array_equal(op[0], [3, 2, 0, 6]) and np.array_equal(op[1], [0, 1, 2, 3])  # both rows of id 11 skipped; the NaN row never
    od, op, oi, oa = knn_ref.select(d[:, :3], 5, ids=ids[:3])
    assert np.array_equal(op[0], [1, 2, 0, -1, -1]) and np.array_equal(oi[0], [11, 12, 10, -1, -1]) and np.array_equal(oa[0], [-1] * 5)
    assert np.all(np.isinf(od[0, 3:])) and od.dtype == np.float32
    od, op, oi, oa = knn_ref.select(np.zeros((2, 0), np.float32), 3)
    assert np.all(np.isinf(od)) and np.all(op == -1) and np.all(oi == -1)


# ---- the Python layer against a stand-in engine ----

class _Ix:
    def __init__(self, dim, engine=None):
        self.dim, self.rows, self.ids, self.atoms = dim, np.zeros((0, dim), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int32)
        self.engine = engine  # the stand-in that counts this index's free

    def __len__(self):
        return len(self.rows)

    def free(self):
        if self.engine is not None:
            self.engine.freed += 1


class _StandIn:
    """the Engine surface the index uses.  Row of structure s (global count over the engine's batches): [s, 0, ...]; of its atom a:
    [s, a, 0, ...].  A query's distances are computed by knn_ref on those rows."""
    training = True  # (padded inputs go through the host packer: the stand-in reads mol_offset)

    def __init__(self, cfg):
        self.cfg = types.SimpleNamespace(dense_out=int(cfg["model"]["dense_out"]), global_dim=int(cfg["model"]["global_dim"]))
        self.uploads, self.calls, self.seen, self.created, self.freed = 0, [], 0, 0, 0

    def num_streams(self):
        return 2

    def upload(self, packed):
        self.uploads += 1
        return types.SimpleNamespace(packed=packed, free=lambda: None, release=lambda: None)

    def index_create(self, dim):
        self.created += 1
        return _Ix(dim, self)

    def index_add(self, ix, rows, ids=None, atoms=None):
        rows = np.asarray(rows, np.float32)
        n = len(rows)
        ix.ids = np.concatenate([ix.ids, np.arange(len(ix.rows), len(ix.rows) + n) if ids is None else ids]).astype(np.int64)
        ix.atoms = np.concatenate([ix.atoms, np.full(n, -1) if atoms is None else atoms]).astype(np.int32)
        ix.rows = np.concatenate([ix.rows, rows])

    def index_read(self, ix, first=0, n=None):
        return ix.rows.copy(), ix.ids.copy(), ix.atoms.copy()

    def _rows(self, p, level, dim):
        from scann import _hip

        cnt = np.diff(p.mol_offset)
        if level == _hip.OUT_BF_PROPERTY:
            rows = np.zeros((p.n_struct, dim), np.float32)
            rows[:, 0] = np.arange(p.n_struct) + self.seen
            return rows, None, cnt
        rows = np.zeros((p.n_atom, dim), np.float32)
        rows[:, 0] = np.repeat(np.arange(p.n_struct) + self.seen, cnt)
        rows[:, 1] = np.arange(p.n_atom) - np.repeat(p.mol_offset[:-1], cnt)
        return rows, rows[:, 1].astype(np.int32), cnt

    def index_add_batch(self, ix, rb, level, ids=None):
        from scann import _hip

        p = rb.packed
        self.calls.append(("add", level, p.n_struct))
        rows, atoms, cnt = self._rows(p, level, ix.dim)
        ids = np.arange(p.n_struct) if ids is None else np.asarray(ids)
        self.index_add(ix, rows, ids if level == _hip.OUT_BF_PROPERTY else np.repeat(ids, cnt), atoms)
        self.seen += p.n_struct

    def index_query_batch(self, ix, rb, level, k, query_ids=None):
        from scann import _hip

        p = rb.packed
        self.calls.append(("query", level, k, p.n_struct, None if query_ids is None else list(query_ids)))
        rows, _, cnt = self._rows(p, level, ix.dim)
        qid = None if query_ids is None else (np.asarray(query_ids) if level == _hip.OUT_BF_PROPERTY else np.repeat(query_ids, cnt))
        d = knn_ref.dist2_f64(rows, ix.rows).astype(np.float32)
        od, op, oi, oa = knn_ref.select(d, k, ids=ix.ids, atoms=ix.atoms, query_ids=qid)
        out = {"y": (10.0 + np.arange(p.n_struct) + self.seen).astype(np.float32), "ga": np.zeros(p.n_atom, np.float32), "dist2": od, "id": oi,
               "atom": oa, "position": op}
        self.seen += p.n_struct
        return out


def _model(cfg):
    return abi_checks.stand_in_model(cfg, _StandIn)


def _batch(n=5, seed=2):
    cfg = so.default_config("qm9")
    inputs, _ = so.pad_batch(*so.synth_dataset(n, seed), g_update=True)
    return cfg, inputs


def test_bad_arguments_raise_before_any_upload():
    from scann.models import LatentIndex

    cfg, inputs = _batch(3)
    m = _model(cfg)
    for kw in (dict(level="molecule"), dict(level=None), dict(batch_size=0), dict(batch_size=-2)):
        with pytest.raises(ValueError):
            m.build_index(inputs, **kw)
    with pytest.raises(ValueError):
        m.build_index(inputs, ids=[1, 2])
    assert m.engine.uploads == 0 and not m.engine.calls
    ix = m.build_index(inputs)
    up = m.engine.uploads
    m.engine.calls.clear()
    for kw in (dict(k=0), dict(k=33), dict(k=-1), dict(k=2.5), dict(k=None), dict(k=True), dict(batch_size=0), dict(exclude_ids=[1, 2])):
        with pytest.raises(ValueError):
            m.nearest(inputs, ix, **kw)
    with pytest.raises(ValueError):
        m.nearest(inputs, "not an index")
    # an index of another model, and one whose width does not fit this model
    other = _model(so.default_config("qm9"))
    with pytest.raises(ValueError):
        other.nearest(inputs, ix)
    cfg2 = so.default_config("qm9")
    cfg2["model"]["dense_out"] = 64
    small = _model(cfg2)
    ix64 = LatentIndex(small, "structure")
    ix64.model = m  # (what a caller could do by hand: the width still gives it away)
    with pytest.raises(ValueError):
        m.nearest(inputs, ix64)
    assert m.engine.uploads == up and not m.engine.calls


def test_structure_level_slicing_ids_and_the_mean_distance():
    from scann import _hip

    cfg, inputs = _batch(5)
    m = _model(cfg)
    ix = m.build_index(inputs, batch_size=2)
    assert [c[2] for c in m.engine.calls] == [2, 2, 1] and len(ix) == 5 and ix.level == "structure" and ix.dim == 128
    rows, ids, atoms = ix.rows()
    assert np.array_equal(ids, np.arange(5)) and np.all(atoms == -1) and np.array_equal(rows[:, 0], np.arange(5))
    m.engine.calls.clear()
    m.engine.seen = 0  # the queries are the indexed structures again
    r = m.nearest(inputs, ix, k=3, batch_size=2)
    assert [c[3] for c in m.engine.calls] == [2, 2, 1] and all(c[4] is None for c in m.engine.calls)
    assert sorted(r) == ["distance", "latent_distance", "neighbor_id", "predict_property"]
    assert r["predict_property"].shape == (5, 1) and r["distance"].shape == (5, 3) and r["neighbor_id"].shape == (5, 3) and r["latent_distance"].shape == (5, 1)
    assert r["distance"].dtype == np.float32 and r["neighbor_id"].dtype == np.int64 and r["latent_distance"].dtype == np.float32
    assert np.array_equal(r["predict_property"][:, 0], 10.0 + np.arange(5))
    # rows are [s, 0, ..]: structure s's neighbours are s (0), then s - 1 before s + 1 (the tie goes to the earlier position)
    assert np.array_equal(r["neighbor_id"], [[0, 1, 2], [1, 0, 2], [2, 1, 3], [3, 2, 4], [4, 3, 2]])
    assert np.array_equal(r["distance"], np.array([[0, 1, 2], [0, 1, 1], [0, 1, 1], [0, 1, 1], [0, 1, 2]], np.float32))
    want = ((r["distance"][:, 0] + r["distance"][:, 1]) + r["distance"][:, 2]) / np.float32(3)
    assert np.array_equal(r["latent_distance"][:, 0], want)
    one = m.nearest(inputs, ix, k=3, batch_size=64)
    # leave-one-out, ids given; k larger than what is left: the tail
    m.engine.seen = 0
    loo = m.nearest(inputs, ix, k=5, exclude_ids=np.arange(5), batch_size=3)
    assert [c[4] for c in m.engine.calls[-2:]] == [[0, 1, 2], [3, 4]]
    assert np.array_equal(loo["neighbor_id"][0], [1, 2, 3, 4, -1]) and np.isinf(loo["distance"][0, 4]) and np.all(np.isinf(loo["latent_distance"]))
    assert np.array_equal(loo["distance"][2, :4], np.array([1, 1, 2, 2], np.float32))
    assert one["distance"].shape == (5, 3)
    # custom ids, two adds, a PackedBatch
    pk = _hip.pack_inputs(inputs)
    pk = _hip.PackedBatch(pk.atomic, pk.mol_offset, pk.edge_offset, pk.edge_col, pk.edge_dist, pk.edge_weight)
    m2 = _model(cfg)
    ix2 = m2.build_index(pk, ids=[7, 5, 3, 2, 9], batch_size=4)
    ix2.add(_hip.slice_packed(pk, 0, 2))
    assert np.array_equal(ix2.rows()[1], [7, 5, 3, 2, 9, 5, 6]) and len(ix2) == 7


def test_atom_level_repadding():
    from scann import _hip

    cfg, inputs = _batch(4, seed=3)
    m = _model(cfg)
    ix = m.build_index(inputs, level="atom", ids=[40, 41, 42, 43], batch_size=3)
    amask = np.asarray(inputs["atom_mask"]).reshape(4, -1) != 0
    cnt = amask.sum(1)
    assert len(ix) == cnt.sum() and ix.dim == 128
    rows, ids, atoms = ix.rows()
    assert np.array_equal(ids, np.repeat([40, 41, 42, 43], cnt)) and np.array_equal(atoms, np.concatenate([np.arange(c) for c in cnt]))
    m.engine.seen = 0
    r = m.nearest(inputs, ix, k=2, batch_size=3)
    B, M = amask.shape
    assert sorted(r) == ["distance", "latent_distance", "neighbor_atom", "neighbor_id", "predict_property"]
    assert r["distance"].shape == (B, M, 2) and r["neighbor_id"].shape == (B, M, 2) and r["neighbor_atom"].shape == (B, M, 2)
    assert r["latent_distance"].shape == (B, M, 1) and r["predict_property"].shape == (B, 1)
    for b in range(B):
        pos = np.nonzero(amask[b])[0]
        assert np.array_equal(r["neighbor_id"][b, pos, 0], np.full(len(pos), 40 + b))  # the atom itself first, distance 0
        assert np.array_equal(r["neighbor_atom"][b, pos, 0], np.arange(len(pos))) and not r["distance"][b, pos, 0].any()
        assert np.all(r["distance"][b, pos, 1] == 1)
        assert np.all(r["neighbor_id"][b, ~amask[b]] == -1) and np.all(r["neighbor_atom"][b, ~amask[b]] == -1)
        assert not r["distance"][b, ~amask[b]].any() and not r["latent_distance"][b, ~amask[b]].any()
        assert np.all(r["latent_distance"][b, pos, 0] == np.float32(0.5))
    # leave-one-out at atom level skips every atom of the structure; a PackedBatch gives packed arrays
    m.engine.seen = 0
    pk = _hip.pack_inputs(inputs)
    pk = _hip.PackedBatch(pk.atomic, pk.mol_offset, pk.edge_offset, pk.edge_col, pk.edge_dist, pk.edge_weight)
    p = m.nearest(pk, ix, k=2, exclude_ids=[40, 41, 42, 43])
    assert p["distance"].shape == (cnt.sum(), 2) and p["neighbor_atom"].shape == (cnt.sum(), 2) and p["latent_distance"].shape == (cnt.sum(), 1)
    assert not np.any(p["neighbor_id"] == np.repeat([40, 41, 42, 43], cnt)[:, None])
    assert np.array_equal(p["distance"][:, 0] > 0, np.ones(cnt.sum(), bool))


def test_save_and_load_round_trip(tmp_path):
    from scann.models import LatentIndex

    cfg, inputs = _batch(4, seed=3)
    m = _model(cfg)
    for level in ("structure", "atom"):
        ix = m.build_index(inputs, level=level, ids=[9, 8, 7, 6])
        path = str(tmp_path / ("ix_%s.npz" % level))
        ix.save(path)
        assert os.path.exists(path)
        with np.load(path) as z:
            assert sorted(z.files) == ["atoms", "dim", "ids", "level", "rows"] and str(z["level"]) == level and int(z["dim"]) == 128
        m2 = _model(cfg)
        back = LatentIndex.load(m2, path)
        assert back.level == level and back.dim == ix.dim and len(back) == len(ix) and back.model is m2
        for a, b in zip(ix.rows(), back.rows()):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    cfg2 = so.default_config("qm9")
    cfg2["model"]["global_dim"] = 96
    with pytest.raises(ValueError):
        LatentIndex.load(_model(cfg2), path)  # the atom-level index of 128 columns


def test_scann_facade_denormalises_the_prediction_only():
    from scann.models.scann_model import SCANN

    cfg, inputs = _batch(3)
    s = SCANN.__new__(SCANN)
    s.model = _model(cfg)
    s.mean, s.std = 2.0, -0.5
    ix = s.build_index(inputs)
    s.model.engine.seen = 0
    raw = s.model.nearest(inputs, ix, k=2)
    s.model.engine.seen = 0
    got = s.nearest(inputs, ix, k=2)
    assert np.array_equal(got["predict_property"], raw["predict_property"] * -0.5 + 2.0)
    for k in ("distance", "neighbor_id", "latent_distance"):
        assert np.array_equal(got[k], raw[k]), k


# ---- ABI ----

def test_header_ctypes_and_library_agree(hip_lib):
    import ctypes as C

    from scann import _hip

    h = abi_checks.header()
    abi_checks.declared("int scann_index_create(scann_handle_t* h, int32_t dim, scann_index_t** out);",
                        "void scann_index_free(scann_handle_t* h, scann_index_t* idx);",
                        "int64_t scann_index_size(const scann_index_t* idx);",
                        "int scann_index_add(scann_handle_t* h, scann_index_t* idx, const float* rows, int64_t n, const int64_t* ids, const int32_t* atoms);",
                        "int scann_index_read(scann_handle_t* h, scann_index_t* idx, int64_t first, int64_t n, float* rows, int64_t* ids, int32_t* atoms);",
                        "int scann_index_query(scann_handle_t* h, scann_index_t* idx, const float* q, int64_t nq, const int64_t* query_ids, int32_t k, "
                        "float* dist2, int64_t* ids, int32_t* atoms, int32_t* pos);",
                        "int scann_index_add_batch(scann_handle_t* h, scann_index_t* idx, scann_dbatch_t* db, int32_t level, const int64_t* ids);",
                        "int scann_index_query_batch(scann_handle_t* h, scann_index_t* idx, scann_dbatch_t* db, int32_t level, const int64_t* query_ids, "
                        "int32_t k, float* y, float* ga, float* dist2, int64_t* ids, int32_t* atoms, int32_t* pos);",
                        "float scann_knn_distsq(const float* q, const float* r, int64_t d);",
                        "void scann_knn_distsq_matrix(const float* q, int64_t nq, const float* rows, int64_t n, int64_t d, float* out);")
    assert "#define SCANN_ABI_VERSION 1" in h
    assert "#define SCANN_KNN_MAX_K %d" % _hip.KNN_MAX_K in h and _hip.KNN_MAX_K == 32
    assert _hip.KNN_LEVELS == {"structure": _hip.OUT_BF_PROPERTY, "atom": _hip.OUT_AFTER_LC}
    P = C.c_void_p
    sig = abi_checks.signatures({
        "scann_index_create": (C.c_int, [P, C.c_int32, C.POINTER(P)]),
        "scann_index_free": (None, [P, P]), "scann_index_size": (C.c_int64, [P]),
        "scann_index_add": (C.c_int, [P, P, P, C.c_int64, P, P]),
        "scann_index_read": (C.c_int, [P, P, C.c_int64, C.c_int64, P, P, P]),
        "scann_index_query": (C.c_int, [P, P, P, C.c_int64, P, C.c_int32, P, P, P, P]),
        "scann_index_add_batch": (C.c_int, [P, P, P, C.c_int32, P]),
        "scann_index_query_batch": (C.c_int, [P, P, P, C.c_int32, P, C.c_int32] + [P] * 6),
        "scann_knn_distsq": (C.c_float, [P, P, C.c_int64]),
        "scann_knn_distsq_matrix": (None, [P, C.c_int64, P, C.c_int64, C.c_int64, P])})
    for n in sig:
        assert hasattr(hip_lib, n), n


def test_null_arguments_are_errors_not_crashes(hip_lib):
    assert hip_lib.scann_index_create(None, 128, None) == -1
    assert hip_lib.scann_index_size(None) == -1
    assert hip_lib.scann_index_add(None, None, None, 0, None, None) == -1
    assert hip_lib.scann_index_read(None, None, 0, 0, None, None, None) == -1
    assert hip_lib.scann_index_query(None, None, None, 1, None, 5, None, None, None, None) == -1
    assert hip_lib.scann_index_add_batch(None, None, None, 2, None) == -1
    assert hip_lib.scann_index_query_batch(None, None, None, 2, None, 5, None, None, None, None, None, None) == -1
    hip_lib.scann_index_free(None, None)
    assert hip_lib.scann_knn_distsq(None, None, 4) == 0.0
    hip_lib.scann_knn_distsq_matrix(None, 1, None, 1, 4, None)


def test_knn_kernels_use_no_scratch(hip_lib):
    """the tile kernel and the merge of csrc/scann_knn.hip spill nothing, read from the built library's kernel descriptors"""
    from scann import _hip

    kern = {n: v for n, v in abi_checks.device_kernels(_hip.LIB_PATH).items() if "knn_" in n}
    assert len(kern) == 2 and sum("knn_tile_kernel" in n for n in kern) == 1 and sum("knn_merge_kernel" in n for n in kern) == 1, sorted(kern)
    for name, (scratch, vgpr) in kern.items():
        assert scratch == 0, (name, scratch, vgpr)


def test_predict_model_cli_takes_nearest():
    pytest.importorskip("sklearn")
    spec = importlib.util.spec_from_file_location("predict_model_cli_nearest", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parser().parse_args(["some_dir", "--nearest", "3", "--nearest-level", "atom", "--nearest-index", "train.npz"])
    assert a.nearest == 3 and a.nearest_level == "atom" and a.nearest_index == "train.npz"
    d = cli.parser().parse_args(["some_dir"])
    assert d.nearest == 0 and d.nearest_level == "structure" and d.nearest_index == ""
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--nearest-level", "bond"])
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--nearest", "three"])
    with pytest.raises(SystemExit):
        cli.main(cli.parser().parse_args(["some_dir", "--nearest", "33"]))
