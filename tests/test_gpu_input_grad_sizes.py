"""GPU: the input gradients (scann_input_grads / HipModel.input_gradients) on every variant of the backward the call can take.  The
call is the data-gradient mode of the training backward (backward_impl(..., ig), csrc/scann_train_host.cpp): everything upstream of its
three leaves (csrc/scann_input_grad.hip) is the size-switched backward that tests/test_gpu_sizes.py holds to autograd for the WEIGHT
gradients only.  Here the batches of tests/size_batches.py go through the mode itself -- 64-row tiles, 2 to 8 atoms per wave, two
LayerNorm row groups, chunk tiles, L = 7, the modular chain (a training handle begun under SCANN_TRAIN_FUSED=0), the plain-fp32 backward
past GEN_LN_64_ROWS_MAX, leaf subsets, a training handle that has used Dropout.

No new tolerance: (a) test_gpu_input_grads.check as it stands -- every entry under the batch's normalisation, error <= min(GRAD_CAP,
max(GRAD_FLOOR, GRAD_SLACK x the torch-fp32 graph's error)) against fp64 autograd (tests/input_grad_ref.py), y within 1e-4 of its scale;
(b) every structure under its OWN normalisation (test_gpu_input_grads.structure_errors): error at size <= max(that rule with the
structure's own fp32 error, 2 x the same structure's error in its small-side sub-batch (size_batches.small_cuts) on the same handle) --
the factor of test_a_structure_alone_matches_it_inside_a_mixed_batch: a size variant may make no structure worse than the tested small
side by more than the existing rule allows.

Every test first asserts from the uploaded batch (batch_info) that it is on the side it is named for.  The CPU references are computed
once per module and (batch, configuration), shared by the legs that share a configuration, and must be finite in every entry.  One
line per comparison goes to PARITY_LINES (tools/input_grad_sizes.py writes them to profiles/input_grads_sizes.txt)."""
import itertools

import numpy as np
import pytest

import scann_oracle as so
import size_batches as sb
import test_gpu_input_grads as ig

pytestmark = pytest.mark.gpu

FLAG = {"neighbor_distance": "distance", "neighbor_weight": "weight", "ring_aromatic": "ring", "atomic": "cgcnn"}
PARITY_LINES = []  # one line per comparison this module has run
RATIOS = []        # (error / bound, worst structure's error / its bound -- nan where the comparison has none) of each line
HEADER = "%-24s %-18s %-11s %-11s %-11s %s" % ("case", "leaf", "error", "fp32 graph", "bound", "worst structure's error / its bound")

# case -> (batch, what size_batches.LARGE calls it or how it is told apart, configuration).  n_attention = 2 unless named
CASES = {
    "sparse": ("sparse_atoms", "sparse_atoms", {}),
    "sparse_base": ("sparse_atoms", "sparse_atoms", dict(g_update=False)),
    "ring64": ("qm9_ring_b260", "qm9_ring_b260", dict(use_ring=True)),
    "cgcnn64_base": ("qm9_b260_cgcnn", "qm9_b260", dict(feature="cgcnn", g_update=False)),
    "mp": ("mp2018_b128", "mp2018_b128", {}),  # (the fused side of modular_mp)
    "mp_L7": ("mp2018_b128", "mp2018_b128", dict(n_attention=7)),
    "mp_base": ("mp2018_b128", "mp2018_b128", dict(g_update=False)),
    "chunked_ring": ("chunked_ring", "chunked", dict(use_ring=True)),
    "deg40_base": ("deg40", "deg40", dict(g_update=False)),
    "small_general": ("small_general", "small", dict(use_ring=True, feature="cgcnn")),  # (the fused side of modular_small_general)
}
MODULAR = {"modular_sparse": "sparse", "modular_mp": "mp", "modular_mp_base": "mp_base", "modular_small_general": "small_general"}


@pytest.fixture(scope="module")
def cache():
    """key -> value, computed on first use for the whole module"""
    store = {}

    def get(key, make):
        if key not in store:
            store[key] = make()
        return store[key]

    return get


def config(batch, **over):
    """test_gpu_sizes.config: the species count (n_atoms) of the data set the batch is shaped after, two LocalAttention layers"""
    cfg = so.default_config("mp2018" if batch.startswith("mp2018") else "qm9")
    cfg["model"]["n_attention"] = 2
    cfg["model"].update(over)
    return cfg, so.init_weights(cfg, 3, perturb=True)


def case_of(cache, case):
    """(cfg, weights, PackedBatch, targets, side) of a case; a batch is packed once per branch"""
    batch, side, over = CASES[case]
    cfg, w = config(batch, **over)
    g_update = bool(cfg["model"]["g_update"])
    pk, targets = cache(("batch", batch, g_update), lambda: getattr(sb, batch)(g_update))
    return cfg, w, pk, targets, side


def references(cache, case, cfg, w, pk):
    """((y, gradients) of fp64 autograd, the torch-fp32 graph's gradients): once per (batch, configuration); finite in every entry --
    no batch here has a one-atom structure (NaN under use_ga_norm), tests/test_input_grad_sizes_host.py"""
    import input_grad_ref

    def make():
        y64, ref = input_grad_ref.input_grads(cfg, w, pk)
        _, g32 = input_grad_ref.input_grads(cfg, w, pk, dtype="float32")
        assert np.isfinite(y64).all() and all(np.isfinite(r).all() for r in ref.values()), case
        assert set(ref) == set(ig.wrt_of(cfg))
        return (y64, ref), g32

    batch, _, over = CASES[case]
    return cache(("refs", batch, tuple(sorted(over.items()))), make)


def assert_side(info, side):
    """the uploaded batch is on the side of the switches its case is named for"""
    if side in sb.LARGE:
        assert sb.crosses(side, info["atoms"], info["edges"], info["max_degree"], info["tile_rows"], info["big_atoms"]), (side, info)
    elif side == "chunked":
        assert info["big_atoms"] > 0 and info["tile_rows"] == 64, info
    elif side == "deg40":
        assert info["tile_rows"] == 64 and info["big_atoms"] == 0 and info["edges"] <= sb.EDGE_TILE_32_MAX_EDGES, info
    else:
        assert side == "small" and info["tile_rows"] == 32 and info["big_atoms"] == 0, info


def input_grads(eng, pk, wrt, expect=None):
    """Engine.input_grads of a batch uploaded for the call, under HipModel.input_gradients' names"""
    rb = eng.upload(pk)
    try:
        if expect is not None:
            expect(eng.batch_info(rb))
        got = eng.input_grads(rb, **{FLAG[k]: k in wrt for k in FLAG})
    finally:
        rb.free()
    assert set(got) == set(wrt) | {"y"}, sorted(got)
    got["predict_property"] = got.pop("y").reshape(-1, 1)
    return got


def small_side_grads(eng, pk, wrt, side):
    """the same gradients from the sub-batches of size_batches.small_cuts, each on the small side of every switch, concatenated.  (A
    batch that is large by one structure's degrees alone -- chunked, deg40 -- has no smaller side to cut: its one cut is itself)"""
    from scann import _hip

    cuts = sb.small_cuts(pk)
    assert cuts[0][0] == 0 and cuts[-1][1] == pk.n_struct and (len(cuts) >= 2) == (side in sb.LARGE), (side, cuts)

    def expect(info):
        if side in sb.LARGE:
            assert info["tile_rows"] == 32 and sb.small_side(info["atoms"], info["edges"]), info

    parts = [input_grads(eng, _hip.slice_packed(pk, lo, hi), wrt, expect) for lo, hi in cuts]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}, len(cuts)


def record(case, leaf, err, e32, bound, ratio, note=""):
    line = "%-24s %-18s %-11.3e %-11.3e %-11.3e %.3f%s" % (case, leaf, err, e32, bound, ratio, note)
    print(line)
    PARITY_LINES.append(line)
    RATIOS.append((err / bound, ratio))


def check_case(label, got, small, cfg, w, pk, refs, g32):
    """(a) and (b) of the module docstring; every figure is printed before anything is asserted"""
    (y64, ref) = refs
    e_gpu, e_32 = ig.errors(got, ref), ig.errors(g32, ref)
    s_gpu, s_small, s_32 = (ig.structure_errors(x, ref, pk) for x in (got, small, g32))
    worst = {}
    for k in ref:
        lim = np.maximum(np.minimum(ig.GRAD_CAP, np.maximum(ig.GRAD_FLOOR, ig.GRAD_SLACK * s_32[k])), 2 * s_small[k])
        assert lim.shape == (pk.n_struct,) and s_gpu[k].shape == (pk.n_struct,)  # (no structure is skipped)
        s = int(np.argmax(s_gpu[k] / lim))
        worst[k] = (float(s_gpu[k][s] / lim[s]), s, float(s_gpu[k][s]), float(s_small[k][s]), float(s_32[k][s]))
        record(label, k, e_gpu[k], e_32[k], min(ig.GRAD_CAP, max(ig.GRAD_FLOOR, ig.GRAD_SLACK * e_32[k])), worst[k][0],
               "  (structure %d: %.2e at size, %.2e on the small side, fp32 graph %.2e)" % worst[k][1:])
    ig.check(got, cfg, w, pk, refs, g32)
    bad = {k: v for k, v in worst.items() if not v[0] <= 1.0}
    assert not bad, (label, "leaf: (error / bound, structure, error at size, on the small side, of the fp32 graph)", bad)


def run_case(cache, case, eng, label=None):
    cfg, w, pk, _, side = case_of(cache, case)
    wrt = ig.wrt_of(cfg)
    refs, g32 = references(cache, case, cfg, w, pk)
    got = input_grads(eng, pk, wrt, lambda info: assert_side(info, side))
    small, _ = small_side_grads(eng, pk, wrt, side)
    check_case(label or case, got, small, cfg, w, pk, refs, g32)
    return got


def inference_engine(cfg, w):
    from scann.models.scann_model import HipModel

    return HipModel(cfg, w, device=0, infer=True).engine


def modular_engine(cfg, w, monkeypatch):
    """a training handle whose scann_train_begin read SCANN_TRAIN_FUSED=0: the only handle whose input gradients run the modular chain"""
    from scann.models.scann_model import HipModel

    monkeypatch.setenv("SCANN_TRAIN_FUSED", "0")
    eng = HipModel(cfg, w, device=0).engine
    eng.train_begin()
    monkeypatch.delenv("SCANN_TRAIN_FUSED")
    return eng


def fused_result(cache, case):
    """the case's gradients on an inference handle (always the fused chains), once per module"""
    def make():
        cfg, w, pk, _, side = case_of(cache, case)
        return input_grads(inference_engine(cfg, w), pk, ig.wrt_of(cfg), lambda info: assert_side(info, side))

    return cache(("fused", case), make)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. the fused chains at size, on an inference handle ----

@pytest.mark.parametrize("case", list(CASES))
def test_input_gradients_at_size_match_autograd(hip_lib, cache, case):
    """Gaps 2 to 5 of the data-gradient mode, each by the stage of backward_impl it reaches.
    sparse / sparse_base (gap 2; 34,231 atoms, 8,577 of them without a neighbour): rn_bwd_kernel<2> in bwd_residual_norm, the KEEP
    forward on 64-row atom tiles, attn_bwd16_kernel at 8 atoms per wave in bwd_attention, two LayerNorm row groups, and atoms whose
    rows of d_dist / d_weight are empty between atoms whose rows are not (basis_input_grad_kernel / base_input_grad_kernel).
    sparse_base, mp_base, deg40_base, cgcnn64_base (gap 3): bwd_base_branch's launch_base_input_grad once per layer, adding into
    d_dist / d_weight zeroed once by the call, on 64-row edge tiles (edge_bwd-free chain: launch_edge_dang, launch_gather_sum).
    ring64, cgcnn64_base, chunked_ring (gap 4): bwd_embed_leaf -- embed_input_grad_kernel, one workgroup per atom, reading dC after
    Pend::flush on tail_s -- for ring_aromatic on 64-row edge tiles (the general embedding, no species tables), for atomic [n_atom, 92]
    at thousands of atoms, and behind chunk tiles.
    mp_L7 (gap 5): bwd_geometry seven times on 64-row tiles, the geometry gradient alternating between edGa and edGb before
    bwd_basis_leaf reads it; mp2018_b128 has degrees above 16, so bwd_attention runs attn_bwd_kernel and edge_bwd_kernel<2, false>."""
    cfg, w, _, _, _ = case_of(cache, case)
    got = run_case(cache, case, inference_engine(cfg, w))
    cache(("fused", case), lambda: got)


# ---- 2. the modular chain: a training handle begun under SCANN_TRAIN_FUSED=0 ----

@pytest.mark.parametrize("case", list(MODULAR))
def test_input_gradients_on_the_modular_chain_match_autograd(hip_lib, monkeypatch, cache, case):
    """Gap 1: SCANN_TRAIN_FUSED is read by scann_train_begin only, so the !b.fused halves of bwd_residual_norm (ln_bwd_kernel) and
    bwd_geometry (launch_ln_bwd_edge, launch_atom_sums, the fp32-MFMA launch_linear chain) and the workspace that keeps T and ang
    (keep_all) run in the data-gradient mode only on such a handle.  Same references and bounds as the fused case of the same batch --
    and NOT its bytes: the fused chains multiply in split fp16, the modular ones in fp32 MFMA, so equal bytes over thousands of edges
    mean the switch did not take (the only way a test can see which chain ran)"""
    fused_case = MODULAR[case]
    cfg, w, _, _, _ = case_of(cache, fused_case)
    got = run_case(cache, fused_case, modular_engine(cfg, w, monkeypatch), label=case)
    fused = fused_result(cache, fused_case)
    same = [k for k in ig.wrt_of(cfg) if same_bits(got[k], fused[k])]
    assert not same, (case, "the modular handle returned the fused chains' bytes in", same)
    d = {k: float(np.abs(got[k].astype(np.float64) - fused[k]).max() / np.abs(fused[k]).max()) for k in ig.wrt_of(cfg)}
    print("%s: |modular - fused| / max |fused| = %s" % (case, d))


# ---- 3. the plain-fp32 backward past GEN_LN_64_ROWS_MAX ----

def test_input_gradients_on_the_plain_fp32_kernels_at_size(hip_lib, monkeypatch, cache):
    """Gap 6: SCANN_GENERIC=1 at 128 / 8 on sparse_atoms -- gen_backward(..., ig) with gen_ln_chunks past 64 rows per chunk and
    isolated atoms present, its leaves the same three kernels at run-time width.  The reference of `sparse`; beside it the ordinary
    handle's result under the cross-check of test_plain_fp32_training_cross_checks_the_mfma_path_at_size (2e-4 of the tensor's
    largest entry)"""
    case = "sparse"
    cfg, w, pk, _, _ = case_of(cache, case)
    assert pk.n_atom > sb.GEN_LN_64_ROWS_MAX and int((np.diff(pk.edge_offset) == 0).sum()) > 1000
    monkeypatch.setenv("SCANN_GENERIC", "1")
    plain = inference_engine(cfg, w)
    monkeypatch.delenv("SCANN_GENERIC")
    got = run_case(cache, case, plain, label="plain_sparse")
    mfma = fused_result(cache, case)
    for k in ig.wrt_of(cfg):
        err = float(np.abs(got[k] - mfma[k]).max()) / max(float(np.abs(mfma[k]).max()), 1e-12)
        record("plain_sparse vs mfma", k, err, float("nan"), 2e-4, float("nan"))
        assert err <= 2e-4, (k, err)
    assert not any(same_bits(got[k], mfma[k]) for k in ig.wrt_of(cfg))  # (the plain kernels ran)


# ---- 4. promises of the call at size ----

def subsets(names):
    return [c for n in range(1, len(names) + 1) for c in itertools.combinations(names, n)]


@pytest.mark.parametrize("case", ["ring64", "small_general"])
def test_leaf_subsets_are_the_same_bytes(hip_lib, cache, case):
    """Gap 7: basis_input_grad_kernel / base_input_grad_kernel / embed_input_grad_kernel take null d_dist / d_weight / d_ring /
    d_cgcnn, and bwd_embed_leaf returns early without an atom leaf.  Every non-empty subset of the configuration's leaves returns, bit
    for bit, what the call with all leaves returns for those names (scann_input_grad.hip: one fixed summation order per output), the
    same y, and no other key"""
    cfg, w, pk, _, side = case_of(cache, case)
    eng = inference_engine(cfg, w)
    names = ig.wrt_of(cfg)
    rb = eng.upload(pk)
    assert_side(eng.batch_info(rb), side)
    full = eng.input_grads(rb, **{FLAG[k]: True for k in names})
    assert set(full) == set(names) | {"y"} and all(np.abs(full[k]).max() > 0 for k in names)
    for sub in subsets(names)[:-1]:
        got = eng.input_grads(rb, **{FLAG[k]: k in sub for k in FLAG})
        assert set(got) == set(sub) | {"y"}, (sub, sorted(got))
        bad = [k for k in got if not same_bits(got[k], full[k])]
        assert not bad, (case, sub, bad)
    rb.free()


@pytest.mark.parametrize("case", ["sparse", "mp_base", "modular_sparse"])
def test_two_calls_at_size_return_identical_bits(hip_lib, monkeypatch, cache, case):
    """the base leaf's per-layer += is ordered by the one stream of the mode; no leaf and nothing upstream of one ends in an atomic, on
    the fused or the modular chain, at 8 atoms per wave or on 64-row tiles"""
    fused_case = MODULAR.get(case, case)
    cfg, w, pk, _, side = case_of(cache, fused_case)
    eng = modular_engine(cfg, w, monkeypatch) if case in MODULAR else inference_engine(cfg, w)
    rb = eng.upload(pk)
    assert_side(eng.batch_info(rb), side)
    a, b = eng.input_grads(rb), eng.input_grads(rb)
    rb.free()
    bad = [k for k in a if not same_bits(a[k], b[k])]
    assert sorted(a) == ["neighbor_distance", "neighbor_weight", "y"] and not bad, bad


def test_training_handle_with_dropout_set(hip_lib, cache):
    """Gap 8: scann_input_grads runs its own training forward with both Dropout rates 0 (train_forward_impl(h, db, nullptr, 0, 0, ..))
    whatever the handle's scann_set_attention_dropout rate and the batch's last training forward were: after two train_step with
    Dropout 0.1 and attention dropout 0.3 on mp2018_b128 the gradients are autograd's at the handle's current weights, with no dropout
    in the reference.  The call leaves db->kept false: scann_train_backward without a new scann_train_forward is refused
    (SCANN_ERR_INVALID, the message names the forward), and a further train_step works"""
    import input_grad_ref
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg, w, pk, targets, side = case_of(cache, "mp")
    eng = HipModel(cfg, w, device=0).engine
    eng.train_begin()
    eng.set_attention_dropout(0.3)
    rb = eng.upload(pk)
    assert_side(eng.batch_info(rb), side)
    for seed in (11, 12):
        sse, count = eng.train_step(rb, targets, 1e-3, dropout=0.1, seed=seed)
        assert np.isfinite(sse) and count == pk.n_struct
    w1 = eng.get_weights()
    assert any(not np.array_equal(w1[k], np.asarray(w[k], np.float32)) for k in w1)
    got = eng.input_grads(rb)
    got["predict_property"] = got.pop("y").reshape(-1, 1)
    with pytest.raises(_hip.ScannHipError) as ei:
        eng.train_backward(rb, 1.0, pk.n_struct)
    assert ei.value.code == -1 and "scann_train_forward" in str(ei.value), str(ei.value)  # SCANN_ERR_INVALID (include/scann_hip.h)
    sse, count = eng.train_step(rb, targets, 1e-3, dropout=0.1, seed=13)
    assert np.isfinite(sse) and sse > 0 and count == pk.n_struct
    rb.free()
    y64, ref = input_grad_ref.input_grads(cfg, w1, pk)
    _, g32 = input_grad_ref.input_grads(cfg, w1, pk, dtype="float32")
    assert np.isfinite(y64).all() and all(np.isfinite(r).all() for r in ref.values())
    e_gpu, e_32 = ig.errors(got, ref), ig.errors(g32, ref)
    for k in ref:
        record("train_dropout_mp", k, e_gpu[k], e_32[k], min(ig.GRAD_CAP, max(ig.GRAD_FLOOR, ig.GRAD_SLACK * e_32[k])), float("nan"))
    ig.check(got, cfg, w1, pk, (y64, ref), g32)
