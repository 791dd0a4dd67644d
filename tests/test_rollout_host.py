"""Host tests of the attention rollout (scann_attention_rollout, HipModel.attention_rollout): the row-gather reference of
tests/rollout_ref.py against an independent dense formulation on the oracle's attention maps, with an isolated atom, a duplicated
neighbour and a self edge planted; the properties the definition promises; the Python layer on a stand-in engine (argument errors
before any upload, re-padding to [B, M, M], slicing by batch_size, de-normalisation); header, ctypes table and library agree; the
kernels use no scratch; predict_model.py takes --rollout.  No GPU."""
import importlib.util
import os
import types

import numpy as np
import pytest

import abi_checks
import rollout_ref
import scann_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def planted(kind, n=6, seed=4):
    """a batch of oracle maps (fp32 graph, so a row without a neighbour holds 1/N) with one real atom isolated, one neighbour named twice
    and one atom its own neighbour: (cfg, inputs, maps [L][B, H, M, N], ga [B, M, 1], where = the three (b, m))"""
    cfg = so.default_config(kind)
    w = so.init_weights(cfg, 3, perturb=True)
    inputs, _ = so.pad_batch(*so.synth_dataset(n, seed, kind=kind), g_update=cfg["model"]["g_update"])
    inputs = {k: np.array(v) for k, v in inputs.items()}
    amask, em = rollout_ref.masks(inputs)
    deg = em.sum(-1)
    iso = (1, int(np.nonzero(amask[1])[0][1]))
    inputs["neighbor_mask"][iso[0], iso[1], :] = False
    dup = next((b, m) for b in range(2, n) for m in np.nonzero(amask[b])[0] if deg[b, m] >= 2 and em[b, m, 0] and em[b, m, 1])
    inputs["neighbors"][dup[0], dup[1], 1] = inputs["neighbors"][dup[0], dup[1], 0]
    own = next((b, m) for b in range(n) for m in np.nonzero(amask[b])[0] if deg[b, m] >= 1 and em[b, m, 0] and (b, m) not in (iso, dup))
    inputs["neighbors"][own[0], own[1], 0] = own[1]
    inter = {}
    _, ga = so.forward(cfg, w, inputs, np.float32, intermediates=inter)
    maps = [inter["attn_local_%d" % (k + 1)] for k in range(cfg["model"]["n_attention"])]
    N = em.shape[2]
    assert np.all(maps[0][iso[0], :, iso[1], :] == np.float32(1.0) / np.float32(N))  # the fp32 convention the reference must ignore
    return cfg, inputs, maps, ga, (iso, dup, own)


def maps64(cfg, inputs):
    """the fp64 oracle's maps and scores of the same batch: every real row sums to 1 to fp64 rounding"""
    inter = {}
    _, ga = so.forward(cfg, so.init_weights(cfg, 3, perturb=True), inputs, np.float64, intermediates=inter)
    return [inter["attn_local_%d" % (k + 1)] for k in range(cfg["model"]["n_attention"])], ga


@pytest.fixture(scope="module", params=["qm9", "mp2018"])
def case(request):
    return planted(request.param)


@pytest.mark.parametrize("kw", [dict(), dict(residual=0.0), dict(residual=0.25, depth=2), dict(head=3), dict(depth=1, head=0)],
                         ids=["default", "res0", "res025_d2", "head3", "d1_head0"])
def test_row_gather_equals_dense_products(case, kw):
    cfg, inputs, maps, ga, (iso, dup, own) = case
    R, _ = rollout_ref.rollout(inputs, maps, ga, dtype=np.float64, **kw)
    D = rollout_ref.dense_rollout(inputs, maps, **kw)
    assert np.allclose(R, D, rtol=1e-12, atol=1e-300)
    assert np.array_equal(R != 0, D != 0)
    # the isolated atom's row is the identity row (its padded map row holds 1/N)
    row = np.zeros(R.shape[2])
    row[iso[1]] = 1.0
    assert np.array_equal(R[iso[0], iso[1]], row)


def test_rows_and_attribution_sum_to_one(case):
    cfg, inputs, _, _, _ = case
    maps, ga = maps64(cfg, inputs)
    amask, _ = rollout_ref.masks(inputs)
    for kw in (dict(), dict(residual=0.1, head=1), dict(depth=3)):
        R, attr = rollout_ref.rollout(inputs, maps, ga, dtype=np.float64, **kw)
        assert np.max(np.abs(R.sum(-1)[amask] - 1.0)) <= 1e-12
        assert not R[~amask].any() and not R.transpose(0, 2, 1)[~amask].any()
        assert (R >= 0).all()
        s = ga.astype(np.float64)[..., 0].sum(1)
        assert np.max(np.abs(attr[..., 0].sum(1) - 1.0)) <= 1e-12 and np.max(np.abs(s - 1.0)) <= 1e-12
        assert not attr[~amask].any()


def test_depth_one_without_residual_is_the_densified_head_mean_map(case):
    cfg, inputs, maps, ga, (iso, dup, own) = case
    amask, em = rollout_ref.masks(inputs)
    R, _ = rollout_ref.rollout(inputs, maps, depth=1, residual=0.0, dtype=np.float64)
    B, M, N = em.shape
    want = np.zeros((B, M, M))
    a = maps[0].astype(np.float64).mean(1)  # [B, M, N]
    for b, m, k in zip(*np.nonzero(em)):
        want[b, m, inputs["neighbors"][b, m, k]] += a[b, m, k]
    want[iso[0], iso[1], iso[1]] = 1.0  # no edges: the atom keeps its row
    assert np.allclose(R, want, rtol=1e-12, atol=0)
    # the duplicated neighbour holds the sum of both slots, the self edge sits on the diagonal
    b, m = dup
    assert np.isclose(R[b, m, inputs["neighbors"][b, m, 0]], a[b, m, 0] + a[b, m, 1], rtol=1e-12)
    b, m = own
    assert R[b, m, m] >= a[b, m, 0] * (1 - 1e-12) > 0


def test_full_residual_is_the_identity(case):
    cfg, inputs, maps, ga, _ = case
    amask, _ = rollout_ref.masks(inputs)
    for dt in (np.float32, np.float64):
        R, attr = rollout_ref.rollout(inputs, maps, ga, residual=1.0, dtype=dt)
        for b in range(len(amask)):
            assert np.array_equal(R[b], np.diag(amask[b].astype(dt)))
        assert np.array_equal(attr, ga.astype(dt) * amask[..., None])


def test_one_head_uses_that_head_only(case):
    cfg, inputs, maps, ga, _ = case
    rng = np.random.default_rng(0)
    other = [m.copy() for m in maps]
    for m in other:
        m[:, [0, 1, 3, 4, 5, 6, 7]] = rng.random(m[:, [0, 1, 3, 4, 5, 6, 7]].shape, dtype=np.float32)
    a, _ = rollout_ref.rollout(inputs, maps, head=2, dtype=np.float64)
    b, _ = rollout_ref.rollout(inputs, other, head=2, dtype=np.float64)
    c, _ = rollout_ref.rollout(inputs, maps, head=5, dtype=np.float64)
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_relabelling_the_atoms_permutes_rows_and_columns(case):
    cfg, inputs, maps, ga, _ = case
    amask, _ = rollout_ref.masks(inputs)
    B, M = amask.shape
    rng = np.random.default_rng(1)
    perm = np.stack([rng.permutation(M) for _ in range(B)])  # new position p holds old atom perm[b, p]
    inv = np.argsort(perm, axis=1)
    b_ix = np.arange(B)[:, None]
    moved = dict(inputs)
    moved["atom_mask"] = np.asarray(inputs["atom_mask"])[b_ix, perm]
    moved["neighbor_mask"] = inputs["neighbor_mask"][b_ix, perm]
    moved["neighbors"] = inv[b_ix[:, :, None], np.clip(inputs["neighbors"], 0, M - 1)[b_ix, perm]]
    maps_m = [m[b_ix, :, perm].transpose(0, 2, 1, 3) for m in maps]  # [B, H, M, N] with the atom axis permuted
    ga_m = ga[b_ix, perm]
    R, attr = rollout_ref.rollout(inputs, maps, ga, dtype=np.float64)
    Rm, attr_m = rollout_ref.rollout(moved, maps_m, ga_m, dtype=np.float64)
    assert np.allclose(Rm, R[b_ix[:, :, None], perm[:, :, None], perm[:, None, :]], rtol=1e-12, atol=1e-300)
    assert np.allclose(attr_m, attr[b_ix, perm], rtol=1e-12, atol=1e-300)


def test_fp32_reference_is_inside_the_kernel_bound(case):
    """the bound the GPU test holds the kernel to, rehearsed on the reference's own fp32 arithmetic"""
    cfg, inputs, maps, ga, _ = case
    _, em = rollout_ref.masks(inputs)
    L, H = len(maps), maps[0].shape[1]
    R64, _ = rollout_ref.rollout(inputs, maps, dtype=np.float64)
    R32, _ = rollout_ref.rollout(inputs, maps, dtype=np.float32)
    nz = R64 > 1e-30
    err = float(np.max(np.abs(R32[nz] - R64[nz]) / R64[nz]))
    assert err <= rollout_ref.kernel_bound(L, H, int(em.sum(-1).max())), err


# ---- the Python layer against a stand-in engine ----

class _StandIn:
    """the Engine surface attention_rollout uses: y = 10 + s, ga = local atom index, attribution = 100 s + local index,
    rollout block of structure s = 1000 s + 10 i + j"""
    training = True  # (padded inputs go through the host packer: the stand-in reads mol_offset)

    def __init__(self):
        self.uploads, self.calls, self.seen = 0, [], 0

    def num_streams(self):
        return 2

    def upload(self, packed):
        self.uploads += 1
        return types.SimpleNamespace(packed=packed, free=lambda: None, release=lambda: None)

    def attention_rollout(self, rb, residual=0.5, head=None, depth=None, matrix=True):
        p = rb.packed
        self.calls.append((residual, head, depth, matrix, p.n_struct))
        cnt = np.diff(p.mol_offset).astype(np.int64)
        local = (np.arange(p.n_atom) - np.repeat(p.mol_offset[:-1], cnt)).astype(np.int32)
        s = np.repeat(np.arange(p.n_struct) + self.seen, cnt)
        out = {"y": (10.0 + np.arange(p.n_struct) + self.seen).astype(np.float32), "ga": local.astype(np.float32),
               "attribution": (100.0 * s + local).astype(np.float32), "rollout_offset": np.concatenate([[0], np.cumsum(cnt * cnt)])}
        if matrix:
            out["rollout"] = np.concatenate([(1000.0 * (k + self.seen) + 10.0 * np.arange(n)[:, None] + np.arange(n)[None, :]).ravel()
                                             for k, n in enumerate(cnt)] + [np.zeros(0)]).astype(np.float32)
        self.seen += p.n_struct
        return out


def _model(cfg):
    return abi_checks.stand_in_model(cfg, lambda config: _StandIn())


def _batch(n=5):
    cfg = so.default_config("qm9")
    inputs, _ = so.pad_batch(*so.synth_dataset(n, 2), g_update=True)
    return cfg, inputs


@pytest.mark.parametrize("kw", [dict(residual=-0.1), dict(residual=1.5), dict(residual=float("nan")), dict(residual="half"), dict(residual=None),
                                dict(head=8), dict(head=-1), dict(head=1.5), dict(depth=0), dict(depth=8), dict(depth=-2),
                                dict(batch_size=0), dict(batch_size=-3)])
def test_bad_arguments_raise_before_any_upload(kw):
    cfg, inputs = _batch(3)
    m = _model(cfg)
    with pytest.raises(ValueError):
        m.attention_rollout(inputs, **kw)
    assert m.engine.uploads == 0 and not m.engine.calls


def test_repadding_and_slicing():
    from scann import _hip

    cfg, inputs = _batch(5)
    m = _model(cfg)
    r = m.attention_rollout(inputs, residual=0.25, head=3, depth=2, batch_size=2)
    assert m.engine.calls == [(0.25, 3, 2, True, 2), (0.25, 3, 2, True, 2), (0.25, 3, 2, True, 1)]
    amask = np.asarray(inputs["atom_mask"]).reshape(5, -1) != 0
    B, M = amask.shape
    assert sorted(r) == ["atom_attribution", "global_attention", "predict_property", "rollout"]
    assert r["predict_property"].shape == (B, 1) and r["global_attention"].shape == (B, M, 1) and r["atom_attribution"].shape == (B, M, 1)
    assert r["rollout"].shape == (B, M, M) and all(v.dtype == np.float32 for v in r.values())
    assert np.array_equal(r["predict_property"][:, 0], 10.0 + np.arange(B))
    for b in range(B):
        pos = np.nonzero(amask[b])[0]
        n = len(pos)
        assert np.array_equal(r["atom_attribution"][b, pos, 0], 100.0 * b + np.arange(n))
        assert np.array_equal(r["global_attention"][b, pos, 0], np.arange(n))
        assert not r["atom_attribution"][b, ~amask[b]].any() and not r["global_attention"][b, ~amask[b]].any()
        assert np.array_equal(r["rollout"][b][np.ix_(pos, pos)], 1000.0 * b + 10.0 * np.arange(n)[:, None] + np.arange(n)[None, :])
        assert not r["rollout"][b][~amask[b]].any() and not r["rollout"][b][:, ~amask[b]].any()
    one = _model(cfg).attention_rollout(inputs, residual=0.25, head=3, depth=2, batch_size=64)
    for k in r:
        assert np.array_equal(r[k], one[k]), k
    # defaults reach the engine as None; matrix=False returns no rollout
    m2 = _model(cfg)
    r2 = m2.attention_rollout(inputs, matrix=False)
    assert m2.engine.calls == [(0.5, None, None, False, 5)] and sorted(r2) == ["atom_attribution", "global_attention", "predict_property"]
    assert np.array_equal(r2["atom_attribution"], r["atom_attribution"])
    # a PackedBatch: the packed arrays and the offsets of the blocks
    pk = _hip.pack_inputs(inputs)
    pk = _hip.PackedBatch(pk.atomic, pk.mol_offset, pk.edge_offset, pk.edge_col, pk.edge_dist, pk.edge_weight)
    m3 = _model(cfg)
    r3 = m3.attention_rollout(pk, batch_size=2)
    assert [c[-1] for c in m3.engine.calls] == [2, 2, 1]
    assert sorted(r3) == ["atom_attribution", "global_attention", "predict_property", "rollout", "rollout_offset"]
    cnt = np.diff(pk.mol_offset).astype(np.int64)
    assert np.array_equal(r3["rollout_offset"], np.concatenate([[0], np.cumsum(cnt * cnt)])) and r3["rollout_offset"].dtype == np.int64
    assert np.array_equal(r3["atom_attribution"], r["atom_attribution"][amask][:, 0])
    for b in range(B):
        blk = r3["rollout"][r3["rollout_offset"][b]:r3["rollout_offset"][b + 1]].reshape(cnt[b], cnt[b])
        assert np.array_equal(blk, r["rollout"][b][np.ix_(amask[b], amask[b])])


def test_scann_facade_denormalises_the_prediction_only():
    from scann.models.scann_model import SCANN

    cfg, inputs = _batch(3)
    s = SCANN.__new__(SCANN)
    s.model = _model(cfg)
    s.mean, s.std = 2.0, -0.5
    raw = _model(cfg).attention_rollout(inputs, residual=0.3)
    got = s.attention_rollout(inputs, residual=0.3)
    assert s.model.engine.calls[0][0] == 0.3
    assert np.array_equal(got["predict_property"], raw["predict_property"] * -0.5 + 2.0)
    for k in ("global_attention", "atom_attribution", "rollout"):
        assert np.array_equal(got[k], raw[k]), k


# ---- ABI ----

def test_header_ctypes_and_library_agree(hip_lib):
    import ctypes as C

    from scann import _hip

    h = flat = abi_checks.header()
    assert "int64_t scann_rollout_floats(scann_handle_t* h, const scann_dbatch_t* db);" in flat
    assert ("int scann_attention_rollout(scann_handle_t* h, scann_dbatch_t* db, float residual, int32_t head, int32_t depth, float* y, "
            "float* ga, float* attribution, float* rollout);") in flat
    assert "#define SCANN_ABI_VERSION 1" in h
    assert "#define SCANN_ROLLOUT_MAX_ATOMS %d" % _hip.ROLLOUT_MAX_ATOMS in h and _hip.ROLLOUT_MAX_ATOMS == _hip.ABLATE_MAX_ATOMS == 960
    sig = abi_checks.signatures({
        "scann_rollout_floats": (C.c_int64, [C.c_void_p, C.c_void_p]),
        "scann_attention_rollout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_int32] + [C.c_void_p] * 4)})
    assert hasattr(hip_lib, "scann_rollout_floats") and hasattr(hip_lib, "scann_attention_rollout")


def test_null_handle_is_an_error_not_a_crash(hip_lib):
    assert hip_lib.scann_attention_rollout(None, None, 0.5, -1, 0, None, None, None, None) == -1
    assert hip_lib.scann_rollout_floats(None, None) == -1


def test_rollout_kernels_use_no_scratch(hip_lib):
    """the three column-slab instantiations of csrc/scann_rollout.hip and its edge-weight pre-pass spill nothing, read from the built
    library's kernel descriptors"""
    from scann import _hip

    kern = {n: v for n, v in abi_checks.device_kernels(_hip.LIB_PATH).items() if "rollout_" in n}
    assert len(kern) == 4 and sum("rollout_kernel" in n for n in kern) == 3, sorted(kern)
    for name, (scratch, vgpr) in kern.items():
        assert scratch == 0, (name, scratch, vgpr)


def test_predict_model_cli_takes_rollout():
    pytest.importorskip("sklearn")
    spec = importlib.util.spec_from_file_location("predict_model_cli_rollout", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parser().parse_args(["some_dir", "--rollout", "--rollout-residual", "0.25", "--rollout-head", "3"])
    assert a.rollout is True and a.rollout_residual == 0.25 and a.rollout_head == 3
    d = cli.parser().parse_args(["some_dir"])
    assert d.rollout is False and d.rollout_residual == 0.5 and d.rollout_head == -1
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--rollout-head", "first"])
