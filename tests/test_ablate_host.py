"""Host tests of the per-atom contributions (scann_ablate_pooling, HipModel.atom_contributions): the reference shortcut of
tests/ablate_ref.py (global pooling and head from the after_Lc rows of one forward) equals the reference's own recipe -- a forward per kept
set on inputs whose atom_mask is edited; the Python layer refuses bad arguments before anything is uploaded, re-pads, maps the ranking
back to padded indices and de-normalises as documented (stand-in engine); the C header, the ctypes table and the library agree; the
128-wide kernel uses no scratch; predict_model.py takes --contributions.  No GPU."""
import importlib.util
import os
import types

import numpy as np
import pytest

import abi_checks
import ablate_ref
import scann_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small(kind="qm9", n=3, seed=5, L=2, target=None, **over):
    cfg = so.default_config(kind)
    cfg["model"]["n_attention"] = L
    cfg["model"].update(over)
    if target:
        cfg["hyper"]["target"] = target
    w = so.init_weights(cfg, 3, perturb=True)
    inputs, _ = so.pad_batch(*so.synth_dataset(n, seed, kind=kind), g_update=cfg["model"]["g_update"])
    return cfg, w, inputs


@pytest.mark.parametrize("case", [dict(), dict(use_ga_norm=False), dict(target="e_b"), dict(g_update=False)],
                         ids=["qm9", "no_ga_norm", "e_b", "base"])
@pytest.mark.parametrize("mode", ablate_ref.MODES)
def test_shortcut_equals_a_forward_per_kept_set(mode, case):
    """the literal recipe (oracle.forward with atom_mask = 1 on S only) against ablate_ref.ablate, fp64, NaN positions included"""
    cfg, w, inputs = _small(**case)
    z, mol = ablate_ref.after_lc(cfg, w, inputs, np.float64)
    y0, ga = so.forward(cfg, w, inputs, np.float64)
    amask = np.asarray(inputs["atom_mask"]).reshape(ga.shape[:2]) != 0
    order = np.concatenate([np.argsort(-ga[b, amask[b], 0], kind="stable") for b in range(len(amask))])
    got, y = ablate_ref.ablate(cfg, w, z, mol, mode, order, np.float64)
    assert np.allclose(y, y0[:, 0], rtol=1e-12, atol=1e-14)
    n_nan = 0
    for b in range(len(amask)):
        pos = np.nonzero(amask[b])[0]
        n = len(pos)
        for e in range(n):
            keep = ablate_ref.kept_set(mode, n, order[mol[b]:mol[b + 1]], e)
            edited = dict(inputs)
            m = np.array(inputs["atom_mask"], copy=True)
            mb = m[b].reshape(-1)  # (a view of row b whatever the trailing shape)
            mb[pos[~keep]] = 0
            edited["atom_mask"] = m
            with np.errstate(invalid="ignore", divide="ignore"):
                lit = so.forward(cfg, w, edited, np.float64)[0][b, 0]
            g = got[mol[b] + e]
            assert np.isnan(lit) == np.isnan(g), (b, e, lit, g)
            n_nan += int(np.isnan(lit))
            if not np.isnan(lit):
                assert abs(lit - g) <= 1e-11 * max(1.0, abs(lit)), (b, e, lit, g)
    # with use_ga_norm exactly the poolings over one atom or none are 0 / 0 (structures of >= 3 atoms: none in leave-one-out, k = n - 1 and
    # k = n of the deletion curve, k = 1 of the insertion curve); without it nothing is
    per = {"leave_one_out": 0, "deletion": 2, "insertion": 1}[mode]
    assert n_nan == (per * len(amask) if cfg["model"]["use_ga_norm"] else 0)


def test_kept_sets():
    order = np.array([2, 0, 3, 1])
    assert ablate_ref.kept_set("leave_one_out", 4, order, 1).tolist() == [True, False, True, True]
    assert ablate_ref.kept_set("deletion", 4, order, 1).tolist() == [False, True, False, True]
    assert ablate_ref.kept_set("deletion", 4, order, 3).tolist() == [False] * 4
    assert ablate_ref.kept_set("insertion", 4, order, 0).tolist() == [False, False, True, False]
    assert ablate_ref.kept_set("insertion", 4, order, 3).tolist() == [True] * 4


# ---- the Python layer against a stand-in engine ----

class _StandIn:
    """the Engine surface atom_contributions uses: y = 10 + s, ga = local atom index, ablated = 100 s + local entry, order = the
    structure's atoms reversed"""
    training = True  # (padded inputs go through the host packer: the stand-in reads mol_offset)

    def __init__(self):
        self.uploads, self.calls, self.seen = 0, [], 0

    def num_streams(self):
        return 2

    def upload(self, packed):
        self.uploads += 1
        return types.SimpleNamespace(packed=packed, free=lambda: None, release=lambda: None)

    def ablate_pooling(self, rb, mode="leave_one_out"):
        p = rb.packed
        self.calls.append((mode, p.n_struct))
        cnt = np.diff(p.mol_offset)
        local = (np.arange(p.n_atom) - np.repeat(p.mol_offset[:-1], cnt)).astype(np.int32)
        s = np.repeat(np.arange(p.n_struct) + self.seen, cnt)
        out = {"y": (10.0 + np.arange(p.n_struct) + self.seen).astype(np.float32), "ga": local.astype(np.float32),
               "ablated": (100.0 * s + local).astype(np.float32), "order": (np.repeat(cnt, cnt) - 1 - local).astype(np.int32)}
        self.seen += p.n_struct
        return out


def _model(cfg):
    return abi_checks.stand_in_model(cfg, lambda config: _StandIn())


def _batch(n=5):
    cfg = so.default_config("qm9")
    inputs, _ = so.pad_batch(*so.synth_dataset(n, 2), g_update=True)
    return cfg, inputs


@pytest.mark.parametrize("kw", [dict(mode="loo"), dict(mode=None), dict(batch_size=0), dict(batch_size=-3)])
def test_bad_arguments_raise_before_any_upload(kw):
    cfg, inputs = _batch(3)
    m = _model(cfg)
    with pytest.raises(ValueError):
        m.atom_contributions(inputs, **kw)
    assert m.engine.uploads == 0 and not m.engine.calls


@pytest.mark.parametrize("mode", ablate_ref.MODES)
def test_repadding_order_and_slicing(mode):
    cfg, inputs = _batch(5)
    m = _model(cfg)
    r = m.atom_contributions(inputs, mode=mode, batch_size=2)
    assert m.engine.calls == [(mode, 2), (mode, 2), (mode, 1)]
    amask = np.asarray(inputs["atom_mask"]).reshape(5, -1) != 0
    B, M = amask.shape
    assert r["y"].shape == (B, 1) and r["global_attention"].shape == (B, M, 1) and r["ablated"].shape == (B, M, 1)
    assert r["order"].shape == (B, M) and r["order"].dtype == np.int32
    assert ("contribution" in r) == (mode == "leave_one_out")
    for b in range(B):
        pos = np.nonzero(amask[b])[0]
        n = len(pos)
        assert np.array_equal(r["ablated"][b, pos, 0], 100.0 * b + np.arange(n))
        assert np.all(r["ablated"][b, ~amask[b], 0] == 0) and np.all(r["global_attention"][b, ~amask[b], 0] == 0)
        assert np.array_equal(r["order"][b, pos], pos[::-1])  # rank e at the e-th real atom's position, as a padded index
        assert np.all(r["order"][b, ~amask[b]] == -1)
        if mode == "leave_one_out":
            assert np.array_equal(r["contribution"][b, pos, 0], np.float32(10.0 + b) - r["ablated"][b, pos, 0])
            assert np.all(r["contribution"][b, ~amask[b], 0] == 0) and r["contribution"].dtype == np.float32
    one = _model(cfg).atom_contributions(inputs, mode=mode, batch_size=64)
    for k in r:
        assert np.array_equal(r[k], one[k]), k


def test_scann_facade_denormalises():
    from scann.models.scann_model import SCANN

    cfg, inputs = _batch(3)
    s = SCANN.__new__(SCANN)
    s.model = _model(cfg)
    s.mean, s.std = 2.0, -0.5
    raw = _model(cfg).atom_contributions(inputs)
    got = s.atom_contributions(inputs)
    real = (np.asarray(inputs["atom_mask"]).reshape(3, -1) != 0)[..., None]
    assert np.array_equal(got["y"], raw["y"] * -0.5 + 2.0)
    assert np.array_equal(got["ablated"], np.where(real, raw["ablated"] * -0.5 + 2.0, 0))
    assert np.array_equal(got["contribution"], raw["contribution"] * -0.5)
    assert np.array_equal(got["global_attention"], raw["global_attention"]) and np.array_equal(got["order"], raw["order"])


# ---- ABI ----

def test_header_ctypes_and_library_agree(hip_lib):
    import ctypes as C

    from scann import _hip

    h = abi_checks.header()
    assert ("int scann_ablate_pooling(scann_handle_t* h, scann_dbatch_t* db, int32_t mode, float* y, float* ga, float* y_abl, "
            "int32_t* order);") in h
    assert "#define SCANN_ABI_VERSION 1" in h
    for name, v in (("LEAVE_ONE_OUT", 0), ("DELETION", 1), ("INSERTION", 2), ("MAX_ATOMS", _hip.ABLATE_MAX_ATOMS)):
        assert "#define SCANN_ABLATE_%s %d" % (name, v) in h
    assert _hip.ABLATE_MODES == {"leave_one_out": 0, "deletion": 1, "insertion": 2}
    abi_checks.signatures({"scann_ablate_pooling": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])})
    assert hasattr(hip_lib, "scann_ablate_pooling")


def test_null_handle_is_an_error_not_a_crash(hip_lib):
    assert hip_lib.scann_ablate_pooling(None, None, 0, None, None, None, None) == -1


def test_ablate_kernel_uses_no_scratch(hip_lib):
    """the MFMA kernel of csrc/scann_ablate.hip (and its plain-fp32 twin) spill nothing, read from the built library's kernel descriptors"""
    from scann import _hip

    kern = {n: v for n, v in abi_checks.device_kernels(_hip.LIB_PATH).items() if "ablate_kernel" in n}
    assert len(kern) == 2, sorted(kern)
    for name, (scratch, vgpr) in kern.items():
        assert scratch == 0, (name, scratch, vgpr)


def test_predict_model_cli_takes_contributions():
    pytest.importorskip("sklearn")
    spec = importlib.util.spec_from_file_location("predict_model_cli_abl", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.parser().parse_args(["some_dir", "--contributions", "deletion"]).contributions == "deletion"
    assert cli.parser().parse_args(["some_dir"]).contributions == ""
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--contributions", "shapley"])
