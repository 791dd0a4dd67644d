"""GPU: the filled edge-tile plan (scann_plan_tiles_filled; tests/test_tile_fill_host.py checks the plan itself) changes no byte.  A
row's arithmetic does not depend on its place in a tile, an atom's edges stay contiguous and in order inside their tile, the softmax and
the LayerNorm of the context are per atom.  A resident batch's first forward runs the piece-major edge kernels on the contiguous plan,
its later ones on the filled plan (scann_batch_tile_plan says which): both, and the forwards of a handle made under SCANN_TILE_FILL=0
on the same weights, must return equal bytes for y, the GlobalAttention scores, every layer's attention map, after_Lc and bf_property;
so must scann_predict_mc (its masks are keyed by the caller's edge numbers) and a model set.  Every test asserts that the plan is filled
where it should be -- with fewer tiles than scann_batch_info reports -- so that it cannot pass by running the same launches twice.
The oracle's side is the existing parity, size, output, Monte Carlo and model-set suites."""
import numpy as np
import pytest

import scann_oracle as so
import size_batches as sb
from test_gpu_mc_sizes import keys_of, same_bits
from test_gpu_output_sizes import L, new_model
from test_tile_fill_host import hand_built_32

pytestmark = pytest.mark.gpu

# batch -> (configuration, use_ring, tile rows, chunked atoms, is the plan filled)
CASES = {"hand_built_32": ("qm9", False, 32, 0, True), "qm9_b260": ("qm9", False, 64, 0, True), "qm9_ring_b260": ("qm9", True, 64, 0, True),
         "mp2018_b128": ("mp2018", False, 64, 0, True), "sparse_atoms": ("qm9", False, 64, 0, False), "chunked": ("qm9", False, 64, 6, False)}
OUTPUTS = ["local_attention_%d" % k for k in range(L)] + ["after_Lc", "bf_property"]


def config_of(kind, use_ring=False, **over):
    cfg = so.default_config(kind)
    cfg["model"].update(dict(n_attention=L, use_ring=use_ring), **over)
    return cfg, so.init_weights(cfg, 3, perturb=True)


def batch_of(name):
    return hand_built_32() if name == "hand_built_32" else getattr(sb, name)()[0]


def pair(cfg, w, monkeypatch):
    """(the default handle, a handle on the same weights made under SCANN_TILE_FILL=0)"""
    return new_model(cfg, w), new_model(cfg, w, monkeypatch, SCANN_TILE_FILL="0")


def check_plan(eng, rb, pk, rows, big_atoms, filled):
    """the resident batch is on the plan it is meant to be on: the contiguous one (`filled` False) or the host planner's filled one"""
    from scann import _hip

    info = eng.batch_info(rb)
    assert info["tile_rows"] == rows and info["big_atoms"] == big_atoms, info
    got, n = eng.tile_plan(rb)
    assert got == filled, (got, n, info)
    if filled:
        ok, atom_row, _, tiles = _hip.plan_tiles_filled(pk, rows, 24)
        assert ok and n == len(tiles) < info["tiles"] and not np.array_equal(atom_row, np.arange(pk.n_atom))
    else:
        assert n == info["tiles"]


def forwards(model, pk, rows, big_atoms, filled, n=2, outputs=True):
    """the outputs of `n` >= 2 forwards of `pk` uploaded once: the first on the contiguous plan, the others on the filled one if `filled`"""
    from scann import _hip

    eng = model.engine
    rb = eng.upload(pk)
    runs = []
    try:
        if outputs:
            eng.set_outputs(range(L), after_lc=True, bf_property=True)
        for i in range(n):
            check_plan(eng, rb, pk, rows, big_atoms, filled and i > 1)  # (the second forward makes the plan)
            eng.forward_resident(rb, 0)
            out = dict(zip(("y", "ga"), eng.download(rb)))
            if outputs:
                out.update({"local_attention_%d" % k: eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, k) for k in range(L)})
                out["after_Lc"] = eng.read_output(rb, _hip.OUT_AFTER_LC)
                out["bf_property"] = eng.read_output(rb, _hip.OUT_BF_PROPERTY)
            runs.append(out)
        check_plan(eng, rb, pk, rows, big_atoms, filled)
    finally:
        eng.set_outputs()
        rb.free()
    return runs


def same_outputs(label, pk, got, want):
    for n in sorted(want):
        same_bits("%s: %s" % (label, n), got[n], want[n], *((pk, "structure") if n == "y" else (pk, "atom") if n == "ga" else ()))


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_are_the_bytes_of_the_contiguous_plan(hip_lib, monkeypatch, name):
    kind, use_ring, rows, big_atoms, filled = CASES[name]
    pk = batch_of(name)
    deg = np.diff(pk.edge_offset)
    assert (pk.ring is not None) == use_ring
    if name == "hand_built_32":
        assert (deg == 0).any() and deg.max() == 32
    if name == "sparse_atoms":  # degrees 0 .. 3: the atom limit closes the tiles of either plan, best fit saves none -- the identity
        assert deg.max() == 3 and (deg == 0).any()
    cfg, w = config_of(kind, use_ring)
    fill, plain = pair(cfg, w, monkeypatch)
    first, second = forwards(fill, pk, rows, big_atoms, filled)
    off = forwards(plain, pk, rows, big_atoms, False)
    assert sorted(first) == sorted(OUTPUTS + ["y", "ga"])
    same_outputs(name + ", filled against the same handle's first forward", pk, second, first)
    same_outputs(name + ", filled against SCANN_TILE_FILL=0", pk, second, off[1])
    same_outputs(name + ", SCANN_TILE_FILL=0 twice", pk, off[1], off[0])
    assert np.isfinite(first["y"]).all() and np.abs(first["local_attention_1"]).max() > 0
    # without outputs selected (the plain, first-layer and last-layer instantiations instead of their ATTN twins)
    a, b = forwards(fill, pk, rows, big_atoms, filled, outputs=False)
    same_outputs(name + ", no outputs", pk, b, a)
    same_bits(name + ": y with and without outputs", a["y"], first["y"], pk, "structure")


def test_three_layers_run_the_middle_kernel(hip_lib, monkeypatch):
    """L = 3 on qm9_b260: first (fused basis, species tables), middle and last (DEAD) launch of the plain family; three forwards"""
    pk = batch_of("qm9_b260")
    cfg, w = config_of("qm9", n_attention=3)
    fill, plain = pair(cfg, w, monkeypatch)
    runs = forwards(fill, pk, 64, 0, True, n=3, outputs=False)
    off = forwards(plain, pk, 64, 0, False, n=1, outputs=False)
    for r in runs:
        same_outputs("L = 3", pk, r, off[0])


def test_monte_carlo_samples_are_the_bytes_of_the_contiguous_plan(hip_lib, monkeypatch):
    """scann_predict_mc, both rates active, T = 2, qm9_b260: the MC instantiations (general first layer under p_drop); the attention masks
    are keyed by the structure-local number of the CALLER's edge.  The first call's second sample runs on the filled plan, the second
    call's both"""
    pk = batch_of("qm9_b260")
    cfg, w = config_of("qm9", n_attention=3, use_drop=True)
    fill, plain = pair(cfg, w, monkeypatch)
    keys, out = keys_of(pk.n_struct), []
    for model, filled in ((fill, True), (plain, False)):
        eng = model.engine
        rb = eng.upload(pk)
        for call in range(2):
            check_plan(eng, rb, pk, 64, 0, filled and call > 0)
            out.append(eng.predict_mc(rb, 2, seed=11, keys=keys, p_drop=0.1, p_attn=0.05, want_samples=True))
        check_plan(eng, rb, pk, 64, 0, filled)
        rb.free()
    for i in (1, 2, 3):
        for k in ("y_samples", "y_mean", "y_std", "ga_mean", "ga_std"):
            same_bits("predict_mc run %d: %s" % (i, k), out[i][k], out[0][k])
    assert not np.array_equal(out[0]["y_samples"][0], out[0]["y_samples"][1])


def test_model_set_is_the_bytes_of_the_contiguous_plan(hip_lib, monkeypatch):
    """two members on qm9_b260: the SET instantiations, the set forwarded twice on the resident batch"""
    from scann.models import ModelSet
    from test_gpu_model_set import members

    pk = batch_of("qm9_b260")
    cfg, _ = config_of("qm9")
    mem = members(cfg, 2)
    a = ModelSet(mem, device=0)
    monkeypatch.setenv("SCANN_TILE_FILL", "0")
    b = ModelSet(mem, device=0)
    monkeypatch.delenv("SCANN_TILE_FILL")
    out = []
    for ms, filled in ((a, True), (b, False)):
        eng = ms.engine
        rb = eng.upload(pk)
        for i in range(2):
            check_plan(eng, rb, pk, 64, 0, filled and i > 1)
            eng.forward_models(rb, 0)
            out.append(eng.models_download(rb))
        check_plan(eng, rb, pk, 64, 0, filled)
        rb.free()
    for i in (1, 2, 3):
        same_bits("set run %d: y" % i, out[i][0], out[0][0])
        same_bits("set run %d: ga" % i, out[i][1], out[0][1])
    assert not np.array_equal(out[0][0][0], out[0][0][1])
