"""GPU: Monte Carlo dropout (scann_predict_mc) on the far side of the launch code's switches -- 64-row edge tiles (by degree and by
edge count), chunk tiles merged by edge_merge_kernel, 64-row atom tiles, the first layer fed from the per-species tables -- and its
promises at the edges: degenerate structures, the range guard.  tests/test_gpu_mc_dropout.py runs the 32-row side of the same kernels.

Every sample is compared with the torch fp64 restatement run with the same structure-local masks (tests/mc_ref.py) under the rule of
test_every_sample_matches_the_oracle: rel_err(y_gpu, y64) <= max(RTOL, 2 rel_err(y32, y64)).  Each test asserts from the uploaded batch
(batch_info) that it is on the side it is meant to be.  The batches are those of tests/size_batches.py; tests/test_sizes_host.py pins
their plans without a GPU.  The measured errors and bounds are collected in PARITY_LINES (tools/mc_parity.py writes them to
profiles/mc_parity.txt)."""
import numpy as np
import pytest

import mc_ref
import scann_oracle as so
import size_batches as sb
from test_gpu_parity import RTOL, rel_err

pytestmark = pytest.mark.gpu

SEED = 20231
RATES = {"drop+attn": (0.1, 0.05), "attn_only": (0.0, 0.05), "drop_only": (0.1, 0.0)}
W64 = dict(local_dim=64, num_head=4, global_dim=96, dense_out=32)  # the 64x4 widths of test_gpu_mc_dropout.CASES
BRANCH = {True: "g_update", False: "base"}
PARITY_LINES = []  # "case  sample  rel_err  bound" of every oracle comparison this module has run


@pytest.fixture(scope="module")
def cache():
    """key -> value, computed on first use for the whole module"""
    store = {}

    def get(key, make):
        if key not in store:
            store[key] = make()
        return store[key]

    return get


def mc_config(name, L, g_update=True, widths=None, **over):
    cfg = so.default_config("mp2018" if name.startswith("mp2018") else "qm9")
    cfg["model"].update(n_attention=L, g_update=g_update, use_drop=True, **over)
    if widths:
        cfg["model"].update(widths)
        cfg["model"]["n_atoms"] = 100
    return cfg, so.init_weights(cfg, 3, perturb=True)


def batch(cache, name, g_update=True):
    return cache(("batch", name, g_update), lambda: getattr(sb, name)(g_update)[0])


def keys_of(n):
    """one non-trivial uint64 key per structure"""
    return np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64(0xC0FFEE)


def new_model(cfg, w, monkeypatch=None, plain=False):
    from scann.models.scann_model import HipModel

    if not plain:
        return HipModel(cfg, w, device=0, infer=True)
    monkeypatch.setenv("SCANN_GENERIC", "1")  # (read when the handle is made)
    model = HipModel(cfg, w, device=0, infer=True)
    monkeypatch.delenv("SCANN_GENERIC")
    return model


def run_mc(model, pk, T, keys, rates, expect, seed=SEED):
    """predict_mc on the uploaded batch, after `expect(info)` has asserted which side of the switches it is on"""
    eng = model.engine
    rb = eng.upload(pk)
    info = eng.batch_info(rb)
    expect(info)
    r = eng.predict_mc(rb, T, seed=seed, keys=keys, p_drop=rates[0], p_attn=rates[1], want_samples=True)
    rb.free()
    assert r["y_samples"].shape == (T, pk.n_struct)
    return r


def oracle(cache, key, cfg, w, pk, T, keys, rates, monkeypatch, n32=None, seed=SEED):
    """per sample t < T the fp64 restatement's (y, ga); for t < n32 (default: all) the fp32 restatement's error against it.
    (T may be smaller than the number of samples drawn on the GPU: check_oracle then compares the first T.)"""
    import torch_ref

    def make():
        m = cfg["model"]
        p_drop, p_attn = rates
        y64, ga64, e32 = [], [], []
        for t in range(T):
            y, ga = mc_ref.sample_ref(cfg, w, pk, seed, t, keys, p_drop, p_attn, monkeypatch)
            y64.append(y)
            ga64.append(ga)
            if t < (T if n32 is None else n32):
                monkeypatch.setattr(torch_ref, "drop_scale_np", mc_ref.local_drop_twin(pk, t, keys, m["local_dim"]))
                y32 = torch_ref.forward_packed(cfg, w, pk, "float32", drop=(seed, p_drop) if p_drop > 0 else None,
                                               attn_scale=mc_ref.attn_scales(pk, seed, t, keys, m["num_head"], m["n_attention"], p_attn))[0]
                e32.append(rel_err(np.asarray(y32).ravel(), y))
        return dict(y64=y64, ga64=np.stack(ga64), e32=e32)

    return cache(("oracle",) + key, make)


def worst_structure(pk, got, ref):
    """(structure, its atoms, got, ref) where |got - ref| is largest"""
    s = int(np.argmax(np.abs(np.asarray(got, np.float64) - ref)))
    return s, int(pk.mol_offset[s + 1] - pk.mol_offset[s]), float(got[s]), float(ref[s])


def check_oracle(label, pk, r, ref):
    """every sample the oracle was run for under the project's rule (the fp32 error of the last sample restated in fp32 bounds those
    that were not); GA mean / std against the fp64 per-sample scores at 10 RTOL, where the oracle has all the samples"""
    ys = r["y_samples"]
    for t in range(len(ref["y64"])):
        e = rel_err(ys[t], ref["y64"][t])
        bound = max(RTOL, 2 * ref["e32"][min(t, len(ref["e32"]) - 1)])
        line = "%-44s %-7d %-12.3e %.3e" % (label, t, e, bound)
        print(line)
        PARITY_LINES.append(line)
        assert e <= bound, (label, t, e, bound, worst_structure(pk, ys[t], ref["y64"][t]))
    assert not np.array_equal(ys[0], ys[1])  # the samples differ
    g = ref["ga64"]
    if len(g) < ys.shape[0]:
        return
    e_gm = rel_err(r["ga_mean"], g.mean(0))
    e_gs = float(np.max(np.abs(r["ga_std"] - g.std(0, ddof=1)))) / max(float(np.abs(g).max()), 1e-30)
    line = "%-44s %-7s %-12.3e %.3e" % (label, "ga_mean", e_gm, 10 * RTOL)
    PARITY_LINES.append(line)
    PARITY_LINES.append("%-44s %-7s %-12.3e %.3e" % (label, "ga_std", e_gs, 10 * RTOL))
    print(line, " ga_std %.3e" % e_gs)
    assert e_gm <= 10 * RTOL and e_gs <= 10 * RTOL, (label, e_gm, e_gs)


def same_bits(label, got, want, pk=None, unit=None, first=0):
    """float32 arrays equal bit for bit; a failure names the first differing element -- with `pk`, as the structure (`unit` "structure")
    or the atom and its structure (`unit` "atom") of pk that the last index, counted from `first`, stands for"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    if not diff.any():
        return
    idx = tuple(int(i) for i in np.argwhere(diff)[0])
    where = ""
    if unit == "structure":
        where = " (structure %d)" % (first + idx[-1])
    elif unit == "atom":
        a = first + idx[-1]
        s = int(np.searchsorted(pk.mol_offset, a, side="right")) - 1
        where = " (atom %d of structure %d, its neighbours: %d)" % (a - int(pk.mol_offset[s]), s, int(pk.edge_offset[a + 1] - pk.edge_offset[a]))
    raise AssertionError("%s: %d of %d values differ, first at %s%s: %r != %r" % (label, int(diff.sum()), got.size, idx, where, got[idx], want[idx]))


def same_result(label, pk, got, want, s0, s1):
    """the predict_mc results `got` of structures [s0, s1) of `pk` run alone against their rows in the whole batch's `want`"""
    a0, a1 = int(pk.mol_offset[s0]), int(pk.mol_offset[s1])
    same_bits(label + " y_samples", got["y_samples"], want["y_samples"][:, s0:s1], pk, "structure", s0)
    for k in ("y_mean", "y_std"):
        same_bits(label + " " + k, got[k], want[k][s0:s1], pk, "structure", s0)
    for k in ("ga_mean", "ga_std"):
        same_bits(label + " " + k, got[k], want[k][a0:a1], pk, "atom", a0)


def expect_rows(rows, big_atoms=0, atoms_above=None):
    def check(info):
        assert info["tile_rows"] == rows and info["big_atoms"] == big_atoms, info
        if atoms_above is not None:
            assert info["atoms"] > atoms_above, info
        else:
            assert info["atoms"] <= sb.ATOM_TILE_32_MAX, info

    return check


# ---- A. 64-row MC edge kernels ----

@pytest.mark.parametrize("rates", list(RATES))
@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
def test_64_row_edge_tiles_by_degree_match_the_oracle(hip_lib, monkeypatch, cache, g_update, rates):
    """deg40: edge_kernel<G, 2, .., MC> on a few hundred edges -- three layers, so that the first (fused basis), a middle and the last
    (DEAD) launch are MC instantiations; attn_only on this embedding feeds the first layer from the per-species tables; drop_only runs
    the plain 64-row edge kernels behind the MC atom kernels"""
    name, T = "deg40", 3
    pk = batch(cache, name, g_update)
    assert pk.n_edge <= sb.EDGE_TILE_32_MAX_EDGES and int(np.diff(pk.edge_offset).max()) > sb.EDGE_TILE_32_MAX_DEGREE
    keys = keys_of(pk.n_struct)
    cfg, w = mc_config(name, 3, g_update)
    r = run_mc(new_model(cfg, w), pk, T, keys, RATES[rates], expect_rows(64))
    ref = oracle(cache, (name, g_update, rates), cfg, w, pk, T, keys, RATES[rates], monkeypatch)
    check_oracle("%s %s %s" % (name, BRANCH[g_update], rates), pk, r, ref)


def test_64_row_edge_tiles_by_edge_count_match_the_oracle(hip_lib, monkeypatch, cache):
    """mp2018_b128: 43 k edges, degrees up to 24, the crystal configuration's embedding"""
    name, T = "mp2018_b128", 2
    pk = batch(cache, name)
    assert pk.n_edge > sb.EDGE_TILE_32_MAX_EDGES
    keys = keys_of(pk.n_struct)
    cfg, w = mc_config(name, 2)
    r = run_mc(new_model(cfg, w), pk, T, keys, RATES["drop+attn"], expect_rows(64))
    ref = oracle(cache, (name,), cfg, w, pk, T, keys, RATES["drop+attn"], monkeypatch, n32=1)
    check_oracle("%s g_update drop+attn" % name, pk, r, ref)


# ---- B. chunk tiles ----

@pytest.mark.parametrize("rates", ["drop+attn", "attn_only"])
@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
def test_chunk_tiles_under_attention_dropout_match_the_oracle(hip_lib, monkeypatch, cache, g_update, rates):
    """chunked: six atoms of 65 to 219 neighbours.  A chunk tile keys its masks with the structure-local edge index of the chunk and
    leaves its softmax state for edge_merge_kernel; the reference drops weights AFTER the softmax has been normalised, so the chunk's
    sum must stay undropped while its context is dropped -- the oracle comparison sees either being wrong (the restatement with the six
    atoms' weights normalised again after the drop moves y by 1.2e-4 to 1.3e-3 on each of these samples, the measured error is 1e-6; a
    wrong mask index moves it by far more).  Three implementations: the
    MFMA kernels, the plain-fp32 path forced onto 128 / 8 (gen_attn_kernel<MC> at max_degree 219), and that path at 64 / 4 widths."""
    name, T = "chunked", 3
    pk = batch(cache, name, g_update)
    keys = keys_of(pk.n_struct)
    expect = expect_rows(64, big_atoms=6)
    label = "%s %s %s" % (name, BRANCH[g_update], rates)
    cfg, w = mc_config(name, 2, g_update)
    ref = oracle(cache, (name, g_update, rates), cfg, w, pk, T, keys, RATES[rates], monkeypatch)
    r_fast = run_mc(new_model(cfg, w), pk, T, keys, RATES[rates], expect)
    check_oracle(label + " mfma", pk, r_fast, ref)
    r_plain = run_mc(new_model(cfg, w, monkeypatch, plain=True), pk, T, keys, RATES[rates], expect)
    check_oracle(label + " plain", pk, r_plain, ref)
    for t in range(T):  # two implementations of one graph under the same masks
        e = rel_err(r_fast["y_samples"][t], r_plain["y_samples"][t])
        assert e <= RTOL, (label, t, e, worst_structure(pk, r_fast["y_samples"][t], r_plain["y_samples"][t].astype(np.float64)))
    assert not np.array_equal(r_fast["y_samples"], r_plain["y_samples"])  # (they ARE different arithmetic)
    cfg4, w4 = mc_config(name, 2, g_update, widths=W64)
    ref4 = oracle(cache, (name, g_update, rates, "64x4"), cfg4, w4, pk, T, keys, RATES[rates], monkeypatch)
    check_oracle(label + " 64x4", pk, run_mc(new_model(cfg4, w4), pk, T, keys, RATES[rates], expect), ref4)


# ---- C. 64-row MC atom kernels ----

@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
def test_64_row_atom_tiles_match_the_oracle(hip_lib, monkeypatch, cache, g_update):
    """sparse_atoms (34,231 atoms, isolated ones among them): atom_kernel<F, M, 2, .., MC> -- g_update: the FFN variants in modes 0 and 2
    and the non-FFN one in mode 0; base: mode 1.  The fp64 restatement of a sample takes about as long as the NumPy oracle of
    test_inference_on_the_sparse_batch_matches_the_oracle, so the base branch has sample 0 of its two restated and compared."""
    name, T = "sparse_atoms", 2
    pk = batch(cache, name, g_update)
    keys = keys_of(pk.n_struct)
    cfg, w = mc_config(name, 2, g_update, use_attn_norm=True)
    r = run_mc(new_model(cfg, w), pk, T, keys, RATES["drop+attn"], expect_rows(64, atoms_above=sb.ATOM_TILE_32_MAX))
    ref = oracle(cache, (name, g_update), cfg, w, pk, T if g_update else 1, keys, RATES["drop+attn"], monkeypatch, n32=1)
    check_oracle("%s %s drop+attn" % (name, BRANCH[g_update]), pk, r, ref)


# ---- D. the tile height changes no bit ----

@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
@pytest.mark.parametrize("name", ["mp2018_b128", "sparse_atoms"])
def test_samples_at_size_equal_those_of_small_sub_batches(hip_lib, cache, name, g_update):
    """a row's arithmetic is the same instruction sequence at both tile heights, and the masks are keyed by structure-local
    indices: every cut of the batch that sits on the small side of the switches, sampled alone with its slice of the keys on 32-row
    tiles, gives the bits its structures get in the whole batch -- at atom and edge numbers far from a structure's own"""
    from scann.parallel import slice_packed

    T = 2
    pk = batch(cache, name, g_update)
    keys = keys_of(pk.n_struct)
    cfg, w = mc_config(name, 2, g_update)
    model = new_model(cfg, w)
    big = run_mc(model, pk, T, keys, RATES["drop+attn"],
                 expect_rows(64, atoms_above=sb.ATOM_TILE_32_MAX if name == "sparse_atoms" else None))
    cuts = sb.small_cuts(pk)
    assert len(cuts) >= 2
    for lo, hi in cuts:
        sub = slice_packed(pk, lo, hi)
        assert sb.small_side(sub.n_atom, sub.n_edge)
        got = run_mc(model, sub, T, keys[lo:hi], RATES["drop+attn"], expect_rows(32))
        same_result("%s %s structures [%d, %d)" % (name, BRANCH[g_update], lo, hi), pk, got, big, lo, hi)
    print("%s %s: %d cuts on 32-row tiles, the whole batch's bits" % (name, BRANCH[g_update], len(cuts)))


@pytest.mark.parametrize("rates", ["drop+attn", "attn_only"])
@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
@pytest.mark.parametrize("name", ["deg40", "chunked"])
def test_a_structure_gets_the_same_bits_beside_one_that_forces_64_row_tiles(hip_lib, cache, name, g_update, rates):
    """deg40 / chunked: the flanking molecules alone run on 32-row edge tiles and must give the bits they get in the mixed batch (64
    rows); the large structure alone stays on 64 rows (and its chunk tiles) and must give the bits it gets behind other structures"""
    from scann.parallel import slice_packed

    T = 3
    pk = batch(cache, name, g_update)
    keys = keys_of(pk.n_struct)
    n_big = 6 if name == "chunked" else 0
    cfg, w = mc_config(name, 3 if name == "deg40" else 2, g_update)
    model = new_model(cfg, w)
    whole = run_mc(model, pk, T, keys, RATES[rates], expect_rows(64, big_atoms=n_big))
    mid = pk.n_struct // 2
    for lo, hi, expect in ((0, mid, expect_rows(32)), (mid, mid + 1, expect_rows(64, big_atoms=n_big)), (mid + 1, pk.n_struct, expect_rows(32))):
        got = run_mc(model, slice_packed(pk, lo, hi), T, keys[lo:hi], RATES[rates], expect)
        same_result("%s %s %s structures [%d, %d)" % (name, BRANCH[g_update], rates, lo, hi), pk, got, whole, lo, hi)


def test_a_sample_does_not_depend_on_how_many_are_drawn(hip_lib, cache):
    """the batch's sample workspace grows with the first larger call and is laid out by the call's own T: on one resident batch (deg40,
    64-row edge tiles) samples 0 and 1 of a 2-sample call, of the 5-sample call that makes the workspace grow, and of a 2-sample call
    in the grown workspace are the same bits, and so are the two 2-sample calls' reductions"""
    pk = batch(cache, "deg40")
    keys = keys_of(pk.n_struct)
    cfg, w = mc_config("deg40", 3)
    eng = new_model(cfg, w).engine
    rb = eng.upload(pk)
    expect_rows(64)(eng.batch_info(rb))
    runs = [eng.predict_mc(rb, T, seed=SEED, keys=keys, p_drop=0.1, p_attn=0.05, want_samples=True) for T in (2, 5, 2)]
    rb.free()
    same_bits("samples 0, 1 of 5 against those of 2", runs[1]["y_samples"][:2], runs[0]["y_samples"], pk, "structure")
    assert len({runs[1]["y_samples"][t].tobytes() for t in range(5)}) == 5  # five different samples
    for k in runs[0]:
        same_bits("2 samples again after 5: " + k, runs[2][k], runs[0][k], pk, "atom" if k.startswith("ga") else "structure")


# ---- E. degenerate structures ----

def test_a_batch_without_edges_matches_the_oracle(hip_lib, monkeypatch, cache):
    """the three-structure batch of test_degenerate_batches, every atom isolated: the embedding and ResidualNorm masks apply, the
    attention rate has nothing to drop -- the samples are those of attention rate 0, bit for bit"""
    from scann import _hip

    B, M, N, T = 3, 4, 2, 3
    atomic = np.array([[6, 1, 1, 0], [8, 1, 0, 0], [7, 6, 1, 1]], dtype="int32")
    inputs = {"atomic": atomic, "atom_mask": (atomic != 0)[..., None], "neighbors": np.zeros((B, M, N), "int32"),
              "neighbor_mask": np.zeros((B, M, N), bool), "neighbor_weight": np.zeros((B, M, N), "float32"),
              "neighbor_distance": np.zeros((B, M, N), "float32")}
    pk = _hip.pack_inputs(inputs)
    assert pk.n_edge == 0 and pk.n_atom == 9
    keys = keys_of(B)
    cfg, w = mc_config("qm9", 2)
    model = new_model(cfg, w)

    def expect(info):
        assert info["edges"] == 0 and info["atoms"] == 9, info

    r = run_mc(model, pk, T, keys, RATES["drop+attn"], expect)
    ref = oracle(cache, ("no_edges",), cfg, w, pk, T, keys, RATES["drop+attn"], monkeypatch)
    check_oracle("no_edges g_update drop+attn", pk, r, ref)
    r0 = run_mc(model, pk, T, keys, RATES["drop_only"], expect)
    for k in r:
        same_bits("no edges, attention rate 0.05 against 0: " + k, r[k], r0[k])


def test_a_one_atom_structure_is_nan_and_stays_local(hip_lib):
    """use_ga_norm: a one-atom structure's score is the reference's 0 / 0, so its mean and std are NaN as the plain forward's y is --
    and every other structure's samples are, bit for bit, those of the batch without it under the same keys"""
    from scann import _hip

    T = 3
    cfg, w = mc_config("qm9", 2, use_ga_norm=True)
    de, dn = so.synth_dataset(6, 8)
    mols = _hip.pack_inputs(so.pad_batch(de, dn, True)[0])
    lone = _hip.PackedBatch([6], [0, 1], [0, 0], [], [], [])
    at = 3
    pk = _hip.concat_packed([_hip.slice_packed(mols, 0, at), lone, _hip.slice_packed(mols, at, mols.n_struct)])
    assert pk.n_struct == 7 and int(pk.mol_offset[at + 1] - pk.mol_offset[at]) == 1
    a_lone = int(pk.mol_offset[at])
    keys = keys_of(pk.n_struct)
    others = np.arange(pk.n_struct) != at
    model = new_model(cfg, w)
    assert np.isnan(model.engine.forward(pk)[0][at])
    r = run_mc(model, pk, T, keys, RATES["drop+attn"], expect_rows(32))
    assert np.isnan(r["y_mean"][at]) and np.isnan(r["y_std"][at]) and np.isnan(r["y_samples"][:, at]).all()
    assert np.isfinite(r["y_samples"][:, others]).all() and np.isfinite(r["y_std"][others]).all()
    assert np.isfinite(np.delete(r["ga_mean"], a_lone)).all() and np.isfinite(np.delete(r["ga_std"], a_lone)).all()
    ref = run_mc(model, mols, T, keys[others], RATES["drop+attn"], expect_rows(32))
    same_bits("y_samples beside a one-atom structure", r["y_samples"][:, others], ref["y_samples"], mols, "structure")
    for k in ("y_mean", "y_std"):
        same_bits(k + " beside a one-atom structure", r[k][others], ref[k], mols, "structure")
    for k in ("ga_mean", "ga_std"):
        same_bits(k + " beside a one-atom structure", np.delete(r[k], a_lone), ref[k], mols, "atom")


# ---- F. the range guard during sampling ----

def test_out_of_range_activation_fails_sampling_before_any_output_is_written(hip_lib):
    """the two out-of-range checkpoints of test_activation_outside_the_split_fp16_range_is_rerun_in_exact_fp32: the MC kernels have no
    exact-fp32 twins, so scann_predict_mc returns SCANN_ERR_RANGE naming itself and the layer, with every output array as the caller
    left it; the guard word is consumed -- the next forward of the batch re-runs exactly once and returns a fresh handle's bits, and
    with sane weights again the handle samples a fresh handle's bits"""
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg = so.default_config("qm9")
    w = so.init_weights(cfg, 1234, perturb=True)
    de, dn = so.synth_dataset(6, 0)
    pk = _hip.pack_inputs(so.pad_batch(de, dn, True)[0])
    B, A, T = pk.n_struct, pk.n_atom, 3
    keys = keys_of(B)
    bad1 = dict(w)
    bad1["local_attention_1/layer_norm_g/gamma"] = (w["local_attention_1/layer_norm_g/gamma"] * 3.0e5).astype(np.float32)  # geom' ~ 3e5
    bad2 = dict(w)
    bad2["after_Lc/bias"] = (w["after_Lc/bias"] + 1.0e5).astype(np.float32)  # the activation with no LayerNorm behind it
    good = HipModel(cfg, w, device=0, infer=True)
    rb_good = good.engine.upload(pk)
    mc_good = good.engine.predict_mc(rb_good, T, seed=SEED, keys=keys, p_drop=0.1, p_attn=0.05, want_samples=True)
    rb_good.free()
    sentinel = np.float32(-7.25e11).view(np.uint32)
    for bad, where in ((bad1, "local_attention_"), (bad2, "after_Lc")):
        model = HipModel(cfg, bad, device=0, infer=True)
        eng = model.engine
        rb = eng.upload(pk)
        outs = [np.full(n, sentinel, np.uint32) for n in (B, B, A, A, T * B)]
        rc = eng.lib.scann_predict_mc(eng._h, rb._h, T, SEED, keys.ctypes.data, 0.1, 0.05, *[o.ctypes.data for o in outs])
        msg = (eng.lib.scann_last_error(eng._h) or b"").decode()
        assert rc == -7, (rc, msg)  # SCANN_ERR_RANGE
        assert "scann_predict_mc" in msg and where in msg and "65504" in msg, msg
        for name, o in zip(("y_mean", "y_std", "ga_mean", "ga_std", "y_samples"), outs):
            assert np.all(o == sentinel), (where, name, int((o != sentinel).sum()))
        # a forward of the same resident batch: the exact-fp32 re-run, once, and the bits of a handle that never sampled
        assert eng.exact_reruns() == 0
        eng.forward_resident(rb, 0)
        y, ga = eng.download(rb)
        assert eng.exact_reruns() == 1
        fresh = HipModel(cfg, bad, device=0, infer=True)
        rbf = fresh.engine.upload(pk)
        fresh.engine.forward_resident(rbf, 0)
        yf, gaf = fresh.engine.download(rbf)
        rbf.free()
        assert np.isfinite(y).all() and fresh.engine.exact_reruns() == 1
        same_bits(where + ": y after the refused call", y, yf, pk, "structure")
        same_bits(where + ": ga after the refused call", ga, gaf, pk, "atom")
        # sane weights again: sampling works, no further re-run, a fresh handle's bits
        model.set_weights(w)
        r = eng.predict_mc(rb, T, seed=SEED, keys=keys, p_drop=0.1, p_attn=0.05, want_samples=True)
        rb.free()
        assert eng.exact_reruns() == 1
        for k in mc_good:
            same_bits("%s: %s with sane weights again" % (where, k), r[k], mc_good[k], pk, "atom" if k.startswith("ga") else "structure")
