"""Host tests of Monte Carlo dropout (scann_predict_mc, HipModel.predict_uncertainty): the C header declares the entry points, the
NumPy twin of the masks (tests/mc_ref.py) equals the library's own definition, the Python layer refuses bad arguments before anything
is uploaded and slices / de-normalises as documented (stand-in engine), and predict_model.py takes --mc-samples.  No GPU."""
import importlib.util
import os
import types

import numpy as np
import pytest

import abi_checks
import mc_ref
import scann_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_points():
    h = abi_checks.header()
    assert "int scann_predict_mc(scann_handle_t* h, scann_dbatch_t* db, int32_t n_samples, uint64_t seed," in h
    assert "double scann_mc_drop_scale(uint64_t seed, int32_t t, uint64_t key, uint32_t tag, uint64_t idx, float p);" in h


def test_numpy_twin_equals_the_library_masks(hip_lib):
    from scann import _hip

    rng = np.random.default_rng(3)
    seeds = [0, 1, 12345, 2**63 + 17, 2**64 - 1]
    keys = [0, 1, 7, 2**40 + 3, 2**64 - 1]
    tags = [mc_ref.DROP_TAG_EMBED, 0, 5, mc_ref.DROP_TAG_ATTN, mc_ref.DROP_TAG_ATTN + 6]
    n = 0
    for seed in seeds:
        for t in (0, 1, 31):
            for key in keys:
                for tag in tags:
                    for p in (0.05, 0.1, 0.5):
                        idx = rng.integers(0, 1 << 20, size=4).astype(np.uint64)
                        twin = mc_ref.drop_scale(mc_ref.mc_seed(seed, t, key), tag, idx, p)
                        got = [_hip.mc_drop_scale(seed, t, key, tag, int(i), p) for i in idx]
                        assert np.array_equal(np.asarray(got), twin), (seed, t, key, tag, p)
                        n += 1
    assert n == 5 * 3 * 5 * 5 * 3
    # a mask keeps about 1 - p of the elements and scales them by 1 / (1 - p)
    f = mc_ref.drop_scale(mc_ref.mc_seed(9, 0, 0), 1000, np.arange(100000, dtype=np.uint64), 0.1)
    assert abs((f == 0).mean() - 0.1) < 0.01 and np.all((f == 0) | (f == np.float32(1) / np.float32(0.9)))
    assert _hip.mc_drop_scale(1, 0, 0, 1000, 3, 0.0) == 1.0


class _StandIn:
    """the Engine surface predict_uncertainty uses: y samples = 1 + t + s / 10 per structure, ga = atom index within the structure"""

    def __init__(self):
        self.uploads = 0
        self.calls = []

    def num_streams(self):
        return 2

    def upload(self, packed):
        self.uploads += 1
        return types.SimpleNamespace(packed=packed, free=lambda: None, release=lambda: None)

    def predict_mc(self, rb, samples, seed=0, keys=None, p_drop=None, p_attn=None, want_ga=True, want_samples=False):
        p = rb.packed
        self.calls.append((samples, seed, None if keys is None else list(keys), p_drop, p_attn))
        k = np.zeros(p.n_struct) if keys is None else np.asarray(keys, np.float64)
        ys = np.stack([1.0 + t + k / 10 for t in range(samples)]).astype(np.float32)
        ga = (np.arange(p.n_atom) - np.repeat(p.mol_offset[:-1], np.diff(p.mol_offset))).astype(np.float32)
        out = {"y_mean": ys.mean(0), "y_std": ys.std(0, ddof=1), "ga_mean": ga, "ga_std": ga / 2}
        if want_samples:
            out["y_samples"] = ys
        return out


def _model(cfg):
    return abi_checks.stand_in_model(cfg, lambda config: _StandIn(), ring=True)


def _batch(n=5):
    from scann import _hip

    cfg = so.default_config("qm9")
    de, dn = so.synth_dataset(n, 2)
    inputs, _ = so.pad_batch(de, dn, True)
    return cfg, inputs, _hip.pack_inputs(inputs)


@pytest.mark.parametrize("kw", [dict(samples=1), dict(samples=0), dict(rate=1.0), dict(rate=-0.1), dict(attention_rate=1.5),
                                dict(rate=float("nan")), dict(keys=[1, 2])],
                         ids=["T1", "T0", "rate1", "rate_neg", "attn_rate", "rate_nan", "keys_len"])
def test_bad_arguments_raise_before_any_upload(kw):
    cfg, inputs, pk = _batch()
    m = _model(cfg)
    for x in (inputs, pk):
        with pytest.raises(ValueError):
            m.predict_uncertainty(x, **kw)
    assert m.engine.uploads == 0


def test_defaults_slicing_and_repadding():
    cfg, inputs, pk = _batch(7)
    m = _model(cfg)
    keys = np.arange(7) * 3
    got = m.predict_uncertainty(inputs, samples=4, seed=5, keys=keys, batch_size=3, return_samples=True)
    assert m.engine.uploads == 3
    assert [c[1] for c in m.engine.calls] == [5, 5, 5] and [c[2] for c in m.engine.calls] == [[0, 3, 6], [9, 12, 15], [18]]
    assert all(c[3] == 0.1 and c[4] == 0.0 for c in m.engine.calls)  # qm9 config: use_drop off
    B, M = np.shape(inputs["atom_mask"])[:2]
    amask = np.asarray(inputs["atom_mask"]).reshape(B, M) != 0
    assert got["predict_property"].shape == (7, 1) and got["predict_property_std"].shape == (7, 1)
    assert got["global_attention"].shape == (B, M, 1) and got["global_attention_std"].shape == (B, M, 1)
    assert (got["global_attention"][~amask] == 0).all() and (got["global_attention_std"][~amask] == 0).all()
    assert got["samples"].shape == (4, 7, 1)
    assert np.allclose(got["samples"][:, :, 0], np.stack([1.0 + t + keys / 10 for t in range(4)]))
    one = m.predict_uncertainty(inputs, samples=4, seed=5, keys=keys, batch_size=100, return_samples=True)
    for k in one:
        assert np.array_equal(one[k], got[k]), k
    cfg["model"]["use_drop"] = True
    m = _model(cfg)
    r = m.predict_uncertainty(pk, samples=2, rate=0.2)
    assert m.engine.calls[-1][3:] == (0.2, 0.05) and r["global_attention"].shape == (B, M, 1)  # (a packed batch of a padded dict re-pads)


def test_scann_facade_denormalises():
    from scann.models.scann_model import SCANN

    cfg, inputs, _ = _batch(3)
    s = SCANN.__new__(SCANN)
    s.model = _model(cfg)
    s.mean, s.std = 2.0, -0.5
    raw = s.model.predict_uncertainty(inputs, samples=3, return_samples=True)
    got = s.predict_uncertainty(inputs, samples=3, return_samples=True)
    assert np.array_equal(got["predict_property"], raw["predict_property"] * -0.5 + 2.0)
    assert np.array_equal(got["predict_property_std"], raw["predict_property_std"] * 0.5)
    assert np.array_equal(got["samples"], raw["samples"] * -0.5 + 2.0)
    assert np.array_equal(got["global_attention"], raw["global_attention"])


def test_predict_model_cli_takes_mc_samples():
    pytest.importorskip("sklearn")
    spec = importlib.util.spec_from_file_location("predict_model_cli_mc", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parser().parse_args(["some_dir", "--mc-samples", "16", "--mc-seed", "3"])
    assert a.mc_samples == 16 and a.mc_seed == 3
    a = cli.parser().parse_args(["some_dir"])
    assert a.mc_samples == 0 and a.mc_seed == 0
