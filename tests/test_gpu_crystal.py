"""GPU: crystals whose neighbour lists repeat an atom and point at the atom itself (tests/crystal_batches.py) -- the lists a small unit
cell really has (fcc Cu: one atom, twelve edges to itself), which no other batch of the suite contains -- on every path: the forward and
its selected outputs, the exact-fp32 and plain-fp32 kernels, the device packer, ModelSet, the fused / modular / plain / deterministic
backward with its reverse adjacency, input gradients, Monte Carlo dropout and the attention rollout.

Every bound is a rule the suite already has, imported from the module that owns it: rel_err <= RTOL against the fp64 oracle
(test_gpu_outputs.check_against_oracle), check_grads against fp64 autograd (test_gpu_training), the sub-batch-sum rule of
test_gpu_sizes, test_gpu_input_grads.check, test_gpu_mc_sizes.check_oracle, test_gpu_rollout.check_kernel.
tests/test_crystal_host.py pins without a GPU that the batches are what they are named and that the references agree on them; every test
here asserts from the uploaded batch (batch_info) that it runs on the tiles it is meant to.  The CPU references are computed once per
module.  One line per comparison goes to PARITY_LINES (tools/crystal_parity.py writes them to profiles/crystal_parity.txt)."""
import importlib.util
import os

import numpy as np
import pytest

import crystal_batches as cb
import rollout_ref
import scann_oracle as so
import size_batches as sb
import test_gpu_output_sizes as tos
from test_gpu_mc_sizes import BRANCH, RATES, W64, expect_rows, same_bits
from test_gpu_outputs import RTOL, all_names, check_against_oracle, oracle_outputs, rel_err

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_crystal_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tg = _load("test_gpu_training")  # check_grads, grad_reference, grad_errors
ts = _load("test_gpu_sizes")     # check_sum_over_small_sub_batches, margin, FLOAT_ATOMIC

L = tos.L
ONE_ATOM = ("cells_small_1atom", "lattices")  # batches with one-atom cells: NaN under use_ga_norm
PARITY_LINES = []  # "case  tensor or output  error  the fp32 reference's error  bound" of every comparison this module has run
HEADER = "%-38s %-30s %-12s %-12s %s" % ("case", "tensor / output", "error", "fp32 ref", "bound")


def record(case, what, err, e32, bound):
    line = "%-38s %-30s %-12.3e %-12.3e %.3e" % (case, what, err, e32, bound)
    print(line)
    PARITY_LINES.append(line)


@pytest.fixture(scope="module")
def cache():
    """key -> value, computed on first use for the whole module"""
    store = {}

    def get(key, make):
        if key not in store:
            store[key] = make()
        return store[key]

    return get


def expect_of(name):
    rows, n_big, _ = cb.PLAN[name]
    return expect_rows(rows, big_atoms=n_big)


def batch(cache, name, g_update=True, general=False):
    """(padded inputs, PackedBatch, targets) of the crystal batch `name`"""
    def make():
        from scann import _hip

        inputs, targets = cb.padded_general(name, g_update) if general else cb.padded(name, g_update)
        return inputs, _hip.pack_inputs(inputs), np.asarray(targets, np.float32)

    return cache(("batch", name, g_update, general), make)


def oracle(cache, key, cfg, w, inputs):
    """the NumPy oracle in (fp32, fp64): test_gpu_outputs.oracle_outputs plus "y" and "ga", once per (batch, config) `key`"""
    def make():
        out = []
        for dt in (np.float32, np.float64):
            ref = oracle_outputs(cfg, w, inputs, dt)
            ref["y"], ref["ga"] = so.forward(cfg, w, inputs, dt)
            out.append(ref)
        return tuple(out)

    return cache(("oracle",) + key, make)


def forward_against_oracle(label, cache, key, cfg, w, model, inputs, pk, expect, monkeypatch):
    """every selected output, y and the GlobalAttention scores of the padded-array call (the device packer, repad_edges) against the
    fp64 oracle at RTOL -- the resident packed batch first, whose bytes the padded call must return.  Returns the packed outputs"""
    packed = tos.run_outputs(model, pk, expect)
    names = all_names(cfg)
    got = tos.padded_outputs(model, inputs, names, packed, monkeypatch)
    ref32, ref64 = oracle(cache, key, cfg, w, inputs)
    measured = []
    try:
        check_against_oracle(cfg, w, inputs, got, names, fp64_bound=True, refs=(ref32, ref64), measured=measured)
    finally:
        for n, e, _ in measured:
            record(label, n, e, rel_err(ref32[n], ref64[n]), RTOL)
    assert [m[0] for m in measured] == names and all(e <= RTOL for _, e, _ in measured), measured
    y, ga = model.predict(inputs)
    same_bits(label + ": y of the padded call", y[:, 0], packed["y"])
    same_bits(label + ": ga of the padded call", ga, pk.repad_ga(packed["ga"]))
    fin = np.isfinite(ref64["y"][:, 0])  # (a one-atom cell under use_ga_norm: the reference's NaN, compared by test_one_atom_cells_...)
    amask = (np.asarray(inputs["atom_mask"])[..., 0] != 0) & fin[:, None]
    for n, g, sel in (("y", y, fin), ("ga", ga, amask)):
        e = rel_err(g[sel], ref64[n][sel])
        record(label, n, e, rel_err(ref32[n][sel], ref64[n][sel]), RTOL)
        assert e <= RTOL, (label, n, e)
    assert np.array_equal(np.isfinite(y[:, 0]), fin)
    return packed


# ---- 1. forward: every output against the fp64 oracle ----

FORWARD = [(n, False) for n in ("lattices", "cells_small", "cells_deg40", "cells_chunked")] + [("cells_small", True)]


@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
@pytest.mark.parametrize("name,ga_norm", FORWARD, ids=["%s-%s" % (n, "ga_norm" if g else "no_ga_norm") for n, g in FORWARD])
def test_every_output_matches_the_oracle(hip_lib, monkeypatch, cache, name, ga_norm, g_update):
    """lattices / cells_small: 32-row edge tiles; cells_deg40: 64-row tiles by degree, 73 edges of one cell gathering two rows;
    cells_chunked: chunk tiles whose chunks all gather the same one to three rows, merged by attn_merge_kernel.  g_update: the first
    layer fed from the per-species tables"""
    inputs, pk, _ = batch(cache, name, g_update)
    cfg, w = cb.config(g_update, use_ga_norm=ga_norm)
    label = "%s %s%s" % (name, BRANCH[g_update], "" if ga_norm else " no_ga_norm")
    forward_against_oracle(label, cache, (name, g_update, ga_norm), cfg, w, tos.new_model(cfg, w), inputs, pk, expect_of(name), monkeypatch)


@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
def test_large_batch_matches_the_torch_graph_and_the_oracle(hip_lib, monkeypatch, cache, g_update):
    """cells_large: 64-row edge tiles by edge count, each holding several whole cells.  The packed forward against
    torch_ref.forward_packed in fp64 (y, GA scores), and every selected output against the padded oracle"""
    import torch_ref

    name = "cells_large"
    inputs, pk, _ = batch(cache, name, g_update)
    assert pk.n_edge > sb.EDGE_TILE_32_MAX_EDGES and int(np.diff(pk.edge_offset).max()) <= sb.FUSE_ATTN_MAX_DEGREE
    cfg, w = cb.config(g_update)
    model = tos.new_model(cfg, w)
    label = "%s %s" % (name, BRANCH[g_update])
    packed = forward_against_oracle(label, cache, (name, g_update, True), cfg, w, model, inputs, pk, expect_rows(64), monkeypatch)
    y64, ga64 = cache(("torch", name, g_update), lambda: torch_ref.forward_packed(cfg, w, pk))
    y32, ga32 = torch_ref.forward_packed(cfg, w, pk, "float32")
    y, ga = model.predict(pk)
    same_bits(label + ": y of the packed call", y[:, 0], packed["y"])
    for n, g, r64, r32 in (("y (torch)", y[:, 0], y64[:, 0], y32[:, 0]), ("ga (torch)", packed["ga"], ga64, ga32)):
        e = rel_err(g, r64)
        record(label, n, e, rel_err(r32, r64), RTOL)
        assert e <= RTOL, (label, n, e)


@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
def test_general_embedding_matches_the_oracle(hip_lib, monkeypatch, cache, g_update):
    """cells_small with use_ring and feature cgcnn: embed_kernel writes the centres, the first layer has no per-species tables"""
    inputs, pk, _ = batch(cache, "cells_small", g_update, general=True)
    assert pk.ring is not None and pk.cgcnn is not None
    cfg, w = cb.config(g_update, use_ring=True, feature="cgcnn")
    label = "cells_small ring+cgcnn %s" % BRANCH[g_update]
    forward_against_oracle(label, cache, ("general", g_update), cfg, w, tos.new_model(cfg, w), inputs, pk, expect_rows(32), monkeypatch)


@pytest.mark.parametrize("name", ["cells_small", "cells_chunked"])
def test_exact_and_plain_fp32_kernels_match_the_oracle(hip_lib, monkeypatch, cache, name):
    """the other two GPU implementations of the graph: SCANN_EXACT=1 (the row-major EX instantiations, attn_merge_kernel on the chunk
    tiles) and SCANN_GENERIC=1 (run_forward_generic at 128 / 8, and the 64 / 4 widths that only run there) -- each against the oracle, and
    within 2 RTOL of the split-fp16 handle's outputs (test_gpu_output_sizes.agree)"""
    inputs, pk, _ = batch(cache, name)
    expect = expect_of(name)
    cfg, w = cb.config()
    key = (name, True, True)
    fast = forward_against_oracle("%s g_update split-fp16" % name, cache, key, cfg, w, tos.new_model(cfg, w), inputs, pk, expect, monkeypatch)
    exact = tos.new_model(cfg, w, monkeypatch, SCANN_EXACT="1")
    got = forward_against_oracle("%s g_update exact" % name, cache, key, cfg, w, exact, inputs, pk, expect, monkeypatch)
    assert exact.engine.exact_reruns() == 0
    tos.agree("%s exact against split-fp16" % name, got, fast, all_names(cfg), 2 * RTOL)
    plain = tos.new_model(cfg, w, monkeypatch, SCANN_GENERIC="1")
    got = forward_against_oracle("%s g_update plain" % name, cache, key, cfg, w, plain, inputs, pk, expect, monkeypatch)
    tos.agree("%s plain against mfma" % name, got, fast, all_names(cfg), 2 * RTOL)
    cfg4, w4 = cb.config(**W64)
    got4 = forward_against_oracle("%s g_update 64x4" % name, cache, (name, True, True, "64x4"), cfg4, w4, tos.new_model(cfg4, w4), inputs, pk,
                                  expect, monkeypatch)
    assert got4["local_attention_1"].shape[1] == 4 and got4["after_Lc"].shape[1] == 96


# ---- 2. independence, bit for bit ----

OUT_NAMES = ["local_attention_%d" % k for k in range(L)] + ["after_Lc", "bf_property", "y", "ga"]


def same_structure(label, got, s_got, pk_got, whole, s, pk):
    """structure s_got of the outputs `got` (of pk_got) is structure s of `whole` (of pk) in every output, bit for bit"""
    def rows(p, i):
        a0, a1 = int(p.mol_offset[i]), int(p.mol_offset[i + 1])
        return a0, a1, int(p.edge_offset[a0]), int(p.edge_offset[a1])

    ga0, ga1, ge0, ge1 = rows(pk_got, s_got)
    a0, a1, e0, e1 = rows(pk, s)
    for n in OUT_NAMES:
        if n.startswith("local_attention_"):
            same_bits("%s %s" % (label, n), got[n][ge0:ge1], whole[n][e0:e1])
        elif n in ("after_Lc", "ga"):
            same_bits("%s %s" % (label, n), got[n][ga0:ga1], whole[n][a0:a1], pk, "atom", a0)
        else:
            same_bits("%s %s" % (label, n), got[n][s_got:s_got + 1], whole[n][s:s + 1], pk, "structure", s)


@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
def test_a_cell_alone_equals_itself_in_a_batch_and_beside_a_hub(hip_lib, cache, g_update):
    """a cell forwarded alone (32-row tiles), inside cells_small (32-row tiles shared with other cells) and behind cells_deg40's 33- and
    40-edge cell (64-row tiles): the same bytes in every selected output, y and the GA scores; and a permutation of the structures
    permutes the outputs"""
    from scann import _hip

    _, pk, _ = batch(cache, "cells_small", g_update)
    _, pk40, _ = batch(cache, "cells_deg40", g_update)
    hub = _hip.slice_packed(pk40, pk40.n_struct // 2, pk40.n_struct // 2 + 1)
    assert int(np.diff(hub.edge_offset).max()) == 40
    cfg, w = cb.config(g_update)
    model = tos.new_model(cfg, w)
    whole = tos.run_outputs(model, pk, expect_rows(32))
    for s in (0, 2, 5, 13):  # two atoms; eight, one of them pointed at by no edge; six; seven, the batch's last
        one = _hip.slice_packed(pk, s, s + 1)
        label = "cells_small %s structure %d " % (BRANCH[g_update], s)
        same_structure(label + "alone", tos.run_outputs(model, one, expect_rows(32)), 0, one, whole, s, pk)
        pair = _hip.concat_packed([hub, one])
        same_structure(label + "behind the hub", tos.run_outputs(model, pair, expect_rows(64)), 1, pair, whole, s, pk)
    perm = np.random.default_rng(3).permutation(pk.n_struct)
    shuffled = _hip.concat_packed([_hip.slice_packed(pk, int(s), int(s) + 1) for s in perm])
    got = tos.run_outputs(model, shuffled, expect_rows(32))
    for j, s in enumerate(perm):
        same_structure("cells_small %s permuted, structure %d" % (BRANCH[g_update], s), got, j, shuffled, whole, int(s), pk)


def test_one_atom_cells_are_nan_under_ga_norm_and_touch_nothing_else(hip_lib, cache):
    """use_ga_norm divides a one-atom structure's single aggregate by its own norm 0 (the reference's NaN): y of those cells is NaN, and
    every other structure's outputs are the bytes it has in the batch without them"""
    from scann import _hip

    _, pk, _ = batch(cache, "cells_small_1atom")
    cfg, w = cb.config(use_ga_norm=True)
    model = tos.new_model(cfg, w)
    single = np.diff(pk.mol_offset) == 1
    assert 0 < single.sum() < pk.n_struct
    whole = tos.run_outputs(model, pk, expect_rows(32))
    assert np.array_equal(np.isnan(whole["y"]), single), whole["y"]
    keep = [int(s) for s in np.nonzero(~single)[0]]
    rest = _hip.concat_packed([_hip.slice_packed(pk, s, s + 1) for s in keep])
    got = tos.run_outputs(model, rest, expect_rows(32))
    assert np.isfinite(got["y"]).all() and np.isfinite(got["ga"]).all()
    for j, s in enumerate(keep):
        same_structure("cells_small_1atom structure %d without the one-atom cells" % s, got, j, rest, whole, s, pk)
    for n in OUT_NAMES[:L + 1]:  # a one-atom cell's own maps and after_Lc rows are ordinary numbers: its self-loops' weights sum to 1
        assert np.isfinite(whole[n]).all(), n
    assert np.array_equal(np.isnan(whole["bf_property"]).all(1), single) and np.array_equal(np.isnan(whole["bf_property"]).any(1), single)


def test_model_set_members_equal_their_single_models(hip_lib, cache):
    """ModelSet with two members on cells_small: each member's y and GA scores are its single model's, bit for bit"""
    import test_gpu_model_set as tm
    from scann.models import ModelSet

    inputs, pk, _ = batch(cache, "cells_small")
    cfg, _ = cb.config()
    mem = tm.members(cfg, 2)
    ref = tm.singles(mem, inputs)
    ms = ModelSet(mem, device=0)
    tm.assert_members_equal(ms.predict(inputs), ref)
    tm.assert_members_equal(ms.predict(pk), ref)


# ---- 3. training ----

def train_config(name, g_update=True, **over):
    return cb.config(g_update, use_ga_norm=name not in ONE_ATOM, **over)


def grad_refs(cache, key, cfg, w, pk, targets, **kw):
    return cache(("grads",) + key, lambda: tg.grad_reference(cfg, w, pk, targets, **kw))


def train_grads(model, pk, targets, expect, dropout=0.0, seed=0, begin=True, repeat=1):
    """(sse, gradients) of `repeat` forward + backward passes over the batch uploaded once"""
    eng = model.engine
    if begin:
        eng.train_begin()
    rb = eng.upload(pk)
    expect(eng.batch_info(rb))
    out = []
    for _ in range(repeat):
        sse = eng.train_forward(rb, targets, dropout=dropout, seed=seed)
        eng.zero_grads()
        eng.train_backward(rb, sse, pk.n_struct)
        out.append((sse, eng.get_grads()))
    rb.free()
    return out[0] if repeat == 1 else out


def check_grads(label, got, sse, cfg, w, pk, targets, refs, rmse_tol=1e-5):
    """test_gpu_training.check_grads, unchanged, and the loss; the tensor that comes closest to its bound goes to PARITY_LINES first"""
    _, ref, g32 = refs
    e_gpu, e_32 = tg.grad_errors(got, ref), tg.grad_errors(g32, ref)
    bound = {k: min(tg.GRAD_CAP, max(tg.GRAD_FLOOR, tg.GRAD_SLACK * e_32[k])) for k in ref}
    k = max(ref, key=lambda t: e_gpu[t] / bound[t])
    record(label, k, e_gpu[k], e_32[k], bound[k])
    rmse, _ = tg.check_grads(got, cfg, w, pk, targets, refs=refs)
    assert abs(np.sqrt(sse / pk.n_struct) - rmse) <= rmse_tol * max(rmse, 1e-6), (label, np.sqrt(sse / pk.n_struct), rmse)


TRAIN = ["cells_deg16", "cells_small", "cells_small_1atom", "cells_large", "cells_chunked", "lattices"]


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "modular"])
@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
@pytest.mark.parametrize("name", TRAIN)
def test_gradients_match_autograd(hip_lib, monkeypatch, cache, name, g_update, fused):
    """the reverse-adjacency sums of the backward (atom_gather3_kernel, gather_sum_kernel, gather_prod_sum_kernel, atom_sums_kernel) over
    atoms whose incoming edges outnumber their structure's atoms, come from themselves, or do not exist; the gated weight-gradient
    operand X[nb[r]] * X2[r] of wgrad_kernel with repeated nb[r].  cells_deg16 / lattices: the attention backward fused into
    edge_bwd_kernel<1, true>; cells_small: attn_bwd_kernel; cells_large: edge_bwd_kernel<2, ..> on 64-row tiles; cells_chunked: chunk
    tiles.  SCANN_TRAIN_FUSED=0: the modular chain"""
    from scann.models.scann_model import HipModel

    _, pk, targets = batch(cache, name, g_update)
    cfg, w = train_config(name, g_update)
    monkeypatch.setenv("SCANN_TRAIN_FUSED", fused)
    sse, got = train_grads(HipModel(cfg, w, device=0), pk, targets, expect_of(name))
    refs = grad_refs(cache, (name, g_update), cfg, w, pk, targets)
    check_grads("%s %s %s" % (name, BRANCH[g_update], "fused" if fused == "1" else "modular"), got, sse, cfg, w, pk, targets, refs)


def test_dropout_gradients_match_autograd(hip_lib, cache):
    """the two Dropout(0.1) layers and the attention Dropout on cells_small, with the library's masks rebuilt on the host (torch_ref's
    drop= and attn_scale=): the attention mask element is edge * 8 + head, so two edges of one (atom, neighbour) pair draw their own"""
    import torch_ref
    from scann.models.scann_model import HipModel

    name, seed, p = "cells_small", 987654321, 0.1
    _, pk, targets = batch(cache, name)
    cfg, w = train_config(name)
    model = HipModel(cfg, w, device=0)
    model.engine.train_begin()
    model.engine.set_attention_dropout(p)
    sse, got = train_grads(model, pk, targets, expect_of(name), dropout=p, seed=seed, begin=False)
    idx = np.arange(pk.n_edge * 8, dtype=np.uint64)
    scales = [torch_ref.drop_scale_np(seed, 2000 + l, idx, p).reshape(pk.n_edge, 8) for l in range(L)]
    assert 0.05 < np.mean(scales[1] == 0) < 0.15
    refs = grad_refs(cache, (name, "drop"), cfg, w, pk, targets, attn_scale=scales, drop=(seed, p))
    check_grads("%s g_update dropout" % name, got, sse, cfg, w, pk, targets, refs, rmse_tol=2e-5)


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "modular"])
def test_gradients_at_size_equal_the_sum_over_small_sub_batches(hip_lib, monkeypatch, cache, fused):
    """test_gpu_sizes.py's rule on cells_large: the 64-row backward of the whole batch against the sum of the 32-row backward over
    size_batches.small_cuts"""
    from scann.models.scann_model import HipModel

    name = "cells_large"
    _, pk, targets = batch(cache, name)
    cfg, w = train_config(name)
    monkeypatch.setenv("SCANN_TRAIN_FUSED", fused)
    eng = HipModel(cfg, w, device=0).engine
    eng.train_begin()
    n_cuts, worst = ts.check_sum_over_small_sub_batches(eng, pk, targets, lambda rb: expect_rows(64)(eng.batch_info(rb)),
                                                        "%s fused=%s" % (name, fused))
    assert n_cuts >= 2
    label = "%s sum over %d sub-batches %s" % (name, n_cuts, "fused" if fused == "1" else "modular")
    record(label, worst[False][1], worst[False][0], float("nan"), 2e-5)
    record(label, worst[True][1], worst[True][0], float("nan"), tg.GRAD_FLOOR)


def test_plain_fp32_backward(hip_lib, monkeypatch, cache):
    """cells_small on the plain-fp32 training kernels: at 64 / 4 widths against autograd; forced onto 128 / 8 (SCANN_GENERIC=1) against
    autograd and against the MFMA path under the bound of test_plain_fp32_training_cross_checks_the_mfma_path"""
    from scann.models.scann_model import HipModel

    name = "cells_small"
    _, pk, targets = batch(cache, name)
    cfg4, w4 = train_config(name, **W64)
    sse, got = train_grads(HipModel(cfg4, w4, device=0), pk, targets, expect_of(name))
    check_grads("%s g_update 64x4" % name, got, sse, cfg4, w4, pk, targets, grad_refs(cache, (name, True, "64x4"), cfg4, w4, pk, targets),
                rmse_tol=2e-5)
    cfg, w = train_config(name)
    sse_a, ga = train_grads(HipModel(cfg, w, device=0), pk, targets, expect_of(name))
    monkeypatch.setenv("SCANN_GENERIC", "1")
    plain = HipModel(cfg, w, device=0)
    monkeypatch.delenv("SCANN_GENERIC")
    sse_b, gb = train_grads(plain, pk, targets, expect_of(name))
    assert abs(sse_a - sse_b) <= 1e-4 * sse_a
    worst = (0.0, "")
    for k in ga:
        scale = max(float(np.abs(ga[k]).max()), 1e-12)
        err = float(np.abs(ga[k] - gb[k]).max()) / scale
        worst = max(worst, (err, k))
    record("%s g_update plain against mfma" % name, worst[1], worst[0], float("nan"), 2e-4)
    assert worst[0] <= 2e-4, worst
    check_grads("%s g_update plain" % name, gb, sse_b, cfg, w, pk, targets, grad_refs(cache, (name, True), cfg, w, pk, targets), rmse_tol=2e-5)


@pytest.mark.parametrize("name", ["cells_small", "cells_large"])
def test_deterministic_backward_repeats_its_bits(hip_lib, cache, name):
    """the deterministic slots: two backward passes give the same bits in every tensor, and the gradients still meet check_grads"""
    from scann.models.scann_model import HipModel

    _, pk, targets = batch(cache, name)
    cfg, w = train_config(name)
    (sse, a), (_, b) = train_grads(HipModel(cfg, w, device=0, deterministic=True), pk, targets, expect_of(name), repeat=2)
    bad = [k for k in a if not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))]
    assert not bad, bad
    check_grads("%s g_update deterministic" % name, a, sse, cfg, w, pk, targets, grad_refs(cache, (name, True), cfg, w, pk, targets))


def test_reverse_adjacency_built_late_trains_to_the_same_bits(hip_lib, cache):
    """the frame of test_batch_uploaded_before_training_mode_trains_the_same: cells_small uploaded before train_begin gets its reverse
    adjacency on the first backward (ensure_reverse counts and sorts the device copy of edge_col: 602 repeated pairs, 178 self-loops,
    two atoms nobody points at).  In deterministic mode every tensor has the bits of the batch uploaded in training mode"""
    from scann.models.scann_model import HipModel

    name = "cells_small"
    _, pk, targets = batch(cache, name)
    cfg, w = train_config(name)
    eng = HipModel(cfg, w, device=0, deterministic=True).engine
    early = eng.upload(pk)
    y0, _ = eng.forward(pk)
    assert np.isfinite(y0).all()
    eng.train_begin()
    late = eng.upload(pk)
    grads = []
    for rb in (late, early, late):
        sse = eng.train_forward(rb, targets, dropout=0.0, seed=5)
        eng.zero_grads()
        eng.train_backward(rb, sse, pk.n_struct)
        grads.append(eng.get_grads())
    late.free()
    early.free()
    for g in grads[1:]:
        bad = [k for k in g if not np.array_equal(g[k].view(np.uint32), grads[0][k].view(np.uint32))]
        assert not bad, bad
    tg.check_grads(grads[1], cfg, w, pk, targets, refs=grad_refs(cache, (name, True), cfg, w, pk, targets))


# ---- 4. calls built on the forward ----

IG_CASES = {"cells_small-g_update": ("cells_small", True, False), "cells_small-base": ("cells_small", False, False),
            "lattices-g_update": ("lattices", True, False), "lattices-base": ("lattices", False, False),
            "cells_small-ring+cgcnn": ("cells_small", True, True)}


@pytest.mark.parametrize("case", list(IG_CASES))
def test_input_gradients_match_autograd(hip_lib, cache, case):
    """the per-edge leaves of edges that share their (atom, neighbour) pair each get their own gradient; test_gpu_input_grads.check
    against input_grad_ref.  Two calls return the same bits; the padded result holds 0 in masked slots"""
    import input_grad_ref
    import test_gpu_input_grads as ig
    from scann.models.scann_model import HipModel

    name, g_update, general = IG_CASES[case]
    inputs, pk, _ = batch(cache, name, g_update, general)
    over = dict(use_ring=True, feature="cgcnn") if general else {}
    cfg, w = train_config(name, g_update, **over)
    model = HipModel(cfg, w, device=0, infer=True)
    wrt = ig.wrt_of(cfg)
    got = model.input_gradients(pk, wrt=wrt)
    refs = input_grad_ref.input_grads(cfg, w, pk)
    e_gpu = ig.check(got, cfg, w, pk, refs=refs)
    _, g32 = input_grad_ref.input_grads(cfg, w, pk, dtype="float32")
    e_32 = ig.errors(g32, refs[1])
    for k in e_gpu:
        record("input gradients " + case, k, e_gpu[k], e_32[k], min(ig.GRAD_CAP, max(ig.GRAD_FLOOR, ig.GRAD_SLACK * e_32[k])))
    again = model.input_gradients(pk, wrt=wrt)
    for k in got:
        same_bits("input gradients %s, second call: %s" % (case, k), again[k], got[k])
    pad = model.input_gradients(inputs, wrt=wrt)
    amask, em = rollout_ref.masks(inputs)
    for k in ("neighbor_distance", "neighbor_weight"):
        assert pad[k].shape == em.shape and not pad[k][~em].any(), k
        same_bits("input gradients %s, padded call: %s" % (case, k), pad[k][em], got[k])
    for k in wrt[2:]:
        assert not pad[k][~amask].any(), k
        same_bits("input gradients %s, padded call: %s" % (case, k), pad[k][amask], got[k])


@pytest.mark.parametrize("rates", ["drop+attn", "attn_only"])
@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
def test_monte_carlo_samples_match_the_oracle(hip_lib, monkeypatch, cache, g_update, rates):
    """individual MC dropout samples on cells_small against tests/mc_ref.py under test_gpu_mc_sizes.check_oracle's bound"""
    import test_gpu_mc_sizes as mc

    name, T = "cells_small", 3
    _, pk, _ = batch(cache, name, g_update)
    keys = mc.keys_of(pk.n_struct)
    cfg, w = mc.mc_config("mp2018", L, g_update)
    r = mc.run_mc(mc.new_model(cfg, w), pk, T, keys, RATES[rates], expect_rows(32))
    ref = mc.oracle(cache, ("crystal", name, g_update, rates), cfg, w, pk, T, keys, RATES[rates], monkeypatch)
    label = "MC %s %s %s" % (name, BRANCH[g_update], rates)
    n0 = len(mc.PARITY_LINES)
    try:
        mc.check_oracle(label, pk, r, ref)
    finally:
        for line in mc.PARITY_LINES[n0:]:
            f = line[len("%-44s " % label):].split()
            e32 = ref["e32"][int(f[0])] if f[0].isdigit() else float("nan")
            record(label, "sample " + f[0] if f[0].isdigit() else f[0], float(f[1]), e32, float(f[2]))


def pair_keyed_scales(pk, scales):
    """attention-dropout factors as they would be if the mask were keyed by (atom, neighbour) and not by the edge: every edge takes
    the factors of the first edge of its pair"""
    row = np.repeat(np.arange(pk.n_atom), np.diff(pk.edge_offset))
    _, first = np.unique(row.astype(np.int64) * pk.n_atom + pk.edge_col, return_inverse=True)
    lead = np.full(first.max() + 1, pk.n_edge, np.int64)
    np.minimum.at(lead, first, np.arange(pk.n_edge))
    return [s[lead[first]] for s in scales]


def test_monte_carlo_masks_are_keyed_by_the_edge_not_by_the_pair(hip_lib, monkeypatch, cache):
    """Edges that share (atom, neighbour) draw different masks.  predict_mc returns no attention weights, so this is read off y of the
    cells whose edges all share one pair or two -- fcc Cu and bcc Fe (self-loops only), NaCl, CsCl, diamond -- in `lattices` at attention
    dropout 0.5: the samples match the reference with one mask element per edge and head under the usual bound, while the same
    reference with the masks keyed by the pair is more than 100 RTOL away on every one of those cells"""
    import mc_ref
    import test_gpu_mc_sizes as mc
    import torch_ref

    name, T, rates = "lattices", 3, (0.0, 0.5)
    _, pk, _ = batch(cache, name)
    keys = mc.keys_of(pk.n_struct)
    cfg, w = mc.mc_config("mp2018", L, use_ga_norm=False)
    r = mc.run_mc(mc.new_model(cfg, w), pk, T, keys, rates, expect_rows(32))
    ref = mc.oracle(cache, ("crystal", name, "p_attn 0.5"), cfg, w, pk, T, keys, rates, monkeypatch)
    mc.check_oracle("MC lattices g_update p_attn=0.5", pk, r, ref)
    few = [i for i, n in enumerate(cb.LATTICE_NAMES) if n != "SrTiO3" and n != "hcp_Mg"]
    scale = float(np.sqrt(np.mean(np.square(ref["y64"][0]))))
    for t in range(T):
        alt = pair_keyed_scales(pk, mc_ref.attn_scales(pk, mc.SEED, t, keys, 8, L, rates[1]))
        y_alt = np.asarray(torch_ref.forward_packed(cfg, w, pk, attn_scale=alt)[0]).ravel()
        away = np.abs(y_alt - ref["y64"][t])[few] / scale
        print("sample %d: the pair-keyed reference is %s x rms(y) from the edge-keyed one" % (t, np.array2string(away, precision=3)))
        assert away.min() > 100 * RTOL, (t, away)
        assert np.max(np.abs(r["y_samples"][t] - ref["y64"][t])[few]) / scale <= RTOL


@pytest.mark.parametrize("name", ["lattices", "cells_small"])
def test_attention_rollout_adds_parallel_edges(hip_lib, cache, name):
    """INTEGRATION.md section 3, "several edges to one neighbour (periodic images) add, an edge from an atom to itself is an ordinary
    edge": the rollout against tests/rollout_ref.py on the GPU's own maps under test_gpu_rollout.check_kernel's derived bound; rows and
    attributions sum to 1; fcc Cu rolls out to [[1]]; NaCl's rows are those of the two-atom chain its six parallel edges add up to"""
    import test_gpu_rollout as tr
    from scann.models.scann_model import HipModel

    inputs, pk, _ = batch(cache, name)
    cfg, w = train_config(name)
    model = HipModel(cfg, w, device=0, infer=True)
    got = model.attention_rollout(inputs)
    maps = tr.gpu_maps(model, cfg, inputs)
    e, bnd = tr.check_kernel(got, cfg, inputs, maps, name + " rollout")
    record("rollout " + name, "rollout", e, float("nan"), bnd)
    amask, em = rollout_ref.masks(inputs)
    sum_bnd = 2 * L * (int(em.sum(-1).max()) + 4) * tr.EPS  # test_y_and_ga_are_the_forwards_and_rows_sum_to_one
    R = got["rollout"].astype(np.float64)
    dev = float(np.max(np.abs(R.sum(-1)[amask] - 1.0)))
    record("rollout " + name, "|row sum - 1|", dev, float("nan"), sum_bnd)
    assert dev <= sum_bnd
    s = got["atom_attribution"].astype(np.float64)[..., 0].sum(1)
    dev_a = float(np.max(np.abs(s - 1.0)))
    attr_bnd = sum_bnd + (amask.sum(1).max() + 1) * tr.EPS + 1e-5  # (+ the GA scores' own |sum - 1| <= 1e-5, test_gpu_sizes)
    record("rollout " + name, "|attribution sum - 1|", dev_a, float("nan"), attr_bnd)
    assert dev_a <= attr_bnd
    if name == "lattices":
        fcc, nacl = cb.LATTICE_NAMES.index("fcc_Cu"), cb.LATTICE_NAMES.index("NaCl")
        assert abs(R[fcc, 0, 0] - 1.0) <= sum_bnd and not R[fcc].ravel()[1:].any(), R[fcc, 0, 0]
        R64, _ = rollout_ref.rollout(inputs, maps, got["global_attention"])
        assert np.max(np.abs(R[nacl, :2, :2] - R64[nacl, :2, :2]) / R64[nacl, :2, :2]) <= bnd
        assert np.max(np.abs(R[nacl, :2, :2] - 0.5)) <= sum_bnd, R[nacl, :2, :2]  # ([[.5, .5], [.5, .5]]^2: the six weights sum to 1)
