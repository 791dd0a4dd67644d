"""GPU: the LOW end of the split-fp16 projections' range.  The 128 / 8 forward carries every fp32 operand of a 128-wide projection
as hi = fp16(x), lo = fp16(x - hi): 22 significant bits while lo is a normal fp16 number, an absolute quantum of 2^-25 below, so a
row of operands that are all small loses relative precision in proportion to its size (tests/split_ref.py emulates the scheme,
tests/test_low_range_host.py shows that an unguarded forward leaves the bound from k ~ 14 on).  The checkpoints here are ordinary
fp32 checkpoints whose named tensors are scaled by 2^-k -- exact in fp32 -- in front of a normalisation that makes the results
scale-free; the reference evaluates every one of them to ~2e-6.

Acceptance rule (test_branches): every asserted tensor, against the fp64 oracle, is within max(RTOL = 1e-4, 2 x the fp32 oracle's own
error), and finite.  Asserted: predict_property, global_attention, every local_attention_<k>, after_Lc, bf_property through
predict(outputs=...), and, where debug_read is valid (a handle on the split kernels), every layer's centres, geometry and context.
What scann_load_weights decides -- the fast path, or the exact-fp32 kernels with the cause named -- must be what split_ref.small_operands,
its NumPy restatement, decides; nothing may be re-run at run time.  Every figure is printed before it is asserted (pytest -s)."""
import importlib.util
import os

import numpy as np
import pytest

import scann_oracle as so
import split_ref as sr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_low_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tp = _load("test_gpu_parity")     # RTOL, rel_err
to = _load("test_gpu_outputs")    # check_against_oracle
tg = _load("test_gpu_training")   # check_grads

assert tp.RTOL == sr.RTOL


@pytest.fixture(scope="module")
def cache():
    """key -> value, computed on first use for the whole module and left unchanged"""
    store = {}

    def get(key, make):
        if key not in store:
            store[key] = make()
        return store[key]

    return get


def qm9_inputs(cfg, n=8, seed=0):
    de, dn = so.synth_dataset(n, seed)
    return so.pad_batch(de, dn, cfg["model"]["g_update"])[0]


def base_weights(cache, cfg):
    return cache(("w", tuple(sorted(cfg["model"].items()))), lambda: so.init_weights(cfg, 1234, perturb=True))


def report(label, rows, exact):
    for n, e, b, fin, e32 in rows:
        print("LOWRANGE | %-40s | %-18s | fp32 %.2e | gpu %.2e | bound %.2e | %s%s" % (label, n, e32, e, b, "exact" if exact else "split",
                                                                                    "" if fin else " NOT FINITE"))


def check_model(model, cfg, w, inputs, refs, label, debug=True):
    """the module's rule on one handle: the public outputs, the handle's path, and the per-layer tensors or their refusal"""
    from scann import _hip

    eng = model.engine
    r32, r64 = refs
    names = sr.output_names(cfg)
    reason = sr.small_operands(cfg, w)
    got = dict(zip(names, model.predict(inputs, outputs=names)))
    rows = sr.judge(got, r32, r64, names)
    exact = eng.weights_exact()
    lrows, refusal = per_layer(eng, cfg, inputs, refs) if debug else ([], None)
    report(label, rows + lrows, exact)
    print("LOWRANGE   %s: load-time rule: %s" % (label, reason))
    assert not sr.failures(rows), (label, sr.failures(rows))
    y, ga = got["predict_property"], got["global_attention"]  # test_branches, in its own words
    assert tp.rel_err(y, r64["predict_property"]) <= max(tp.RTOL, 2 * tp.rel_err(r32["predict_property"], r64["predict_property"]))
    assert tp.rel_err(ga, r64["global_attention"]) <= max(tp.RTOL, 2 * tp.rel_err(r32["global_attention"], r64["global_attention"]))
    # (copies: check_against_oracle rewrites the 1/N rows of the fp64 attention maps it is handed)
    to.check_against_oracle(cfg, w, inputs, [got[n] for n in names[2:]], names[2:], fp64_bound=True,
                            refs=({n: r32[n] for n in names[2:]}, {n: np.array(r64[n]) for n in names[2:]}))
    assert exact == (reason is not None), (label, exact, reason)
    assert eng.exact_reruns() == 0, label  # decided when the weights were loaded: no forward is run twice
    if debug and exact:  # only the split kernels keep every layer: refused, naming the tensor, never the split kernels' numbers
        assert refusal is not None and refusal.code == -2 and reason.split(":")[0] in str(refusal), refusal
    else:
        assert refusal is None and not sr.failures(lrows), (label, refusal, sr.failures(lrows))
    return rows + lrows


def per_layer(eng, cfg, inputs, refs):
    """(rows of every layer's centres / geometry / context from a debug forward, None) or ([], the error the forward raised)"""
    from scann import _hip

    L = cfg["model"]["n_attention"]
    eng.set_debug(True)
    rb = eng.upload(_hip.pack_inputs(inputs))
    try:
        eng.forward_resident(rb, 0)
        eng.sync()
        layers = {}
        for l in range(L + 1):
            layers["centers_%d" % l] = eng.debug_read(rb, 0, l)
            if cfg["model"]["g_update"]:
                layers["geometry_%d" % l] = eng.debug_read(rb, 1, l)
            if l >= 1:
                layers["context_%d" % l] = eng.debug_read(rb, 2, l)
        return sr.judge(layers, refs[0], refs[1]), None
    except _hip.ScannHipError as e:
        return [], e
    finally:
        eng.set_debug(False)
        rb.free()


def run_case(cache, case, k, model=None, label=None, inputs=None, key=None, debug=True):
    from scann.models.scann_model import HipModel

    cfg = sr.config(**(model or {}))
    w = sr.scaled(base_weights(cache, cfg), case, k)
    if inputs is None:
        inputs = cache(("inputs", cfg["model"]["g_update"]), lambda: qm9_inputs(cfg))
    refs = cache(("refs", case, k, tuple(sorted((model or {}).items())), key), lambda: sr.references(cfg, w, inputs))
    hm = HipModel(cfg, w, device=0, infer=True)
    return cfg, w, inputs, refs, hm, check_model(hm, cfg, w, inputs, refs, label or "%s k=%d" % (case, k), debug=debug)


# ---- 1. the cases, k in {0, 6, 10, 14, 18} ----

@pytest.mark.parametrize("k", sr.KS)
@pytest.mark.parametrize("case", sr.CASES)
def test_small_operands_keep_the_bound(hip_lib, cache, case, k):
    """A small centres, B small geometry, D small readout input (and small after_Lc kernel), W small kernels in a layer, R the
    ResidualNorm's hidden row (dense_2 raised by 2^10 at most: 0.153 x 2^11 would pass 255.9), M mixed rows -- every second component
    small, which must stay on the fast path: a row's largest element decides its precision; P centres AND geometry small, whose product
    is the key projection's operand; E the first layer's centres, swish(dense_embed(embedding)), which no LayerNorm precedes"""
    _, _, _, _, hm, _ = run_case(cache, case, k)
    if k == 0 or case == "M":
        assert not hm.engine.weights_exact()


@pytest.mark.parametrize("k", sr.KS)
@pytest.mark.parametrize("case,model", [("A", dict(g_update=False)), ("A_no_attn_norm", dict(use_attn_norm=False)), ("E", dict(g_update=False))],
                         ids=["base", "no_attn_norm", "E_base"])
def test_small_centres_on_the_other_branches(hip_lib, cache, case, model, k):
    """case A on the base branch (the K = 20 filter feeds the key projection) and without ResidualNorm (the centres of layer 1 are
    local_attention_0/layer_norm's output); case E on the base branch (the first layer's key operand is centres x filtered Gaussians)"""
    run_case(cache, case, k, model=model, label="%s %s k=%d" % (case, "base" if "g_update" in model else "no_attn_norm", k))


@pytest.mark.parametrize("g_update", [True, False], ids=["scann_plus", "base"])
def test_edges_beyond_the_last_gaussian_centre(hip_lib, cache, g_update):
    """case G: an ordinary checkpoint, neighbor_distance 1 A and 2 A beyond the last Gaussian centre on a quarter of the edges -- every
    Gaussian of those rows is tiny (at best exp(-4), exp(-16)); the fused first layer, then the table-free plain one (debug forward)"""
    from scann.models.scann_model import HipModel

    cfg = sr.config(g_update=g_update)
    w = base_weights(cache, cfg)
    inputs = sr.far_edges(qm9_inputs(cfg), cfg)
    hm = HipModel(cfg, w, device=0, infer=True)
    check_model(hm, cfg, w, inputs, sr.references(cfg, w, inputs), "G g_update=%s" % g_update)
    assert not hm.engine.weights_exact()


# ---- 2. shapes: case A at k = 14 ----

def test_small_centres_on_64_row_tiles(hip_lib, cache):
    """260 qm9 molecules: the 64-row edge tiles and the wide atom tiles"""
    from scann import _hip

    cfg = sr.config()
    inputs = qm9_inputs(cfg, 260, 9)
    _, _, _, _, hm, _ = run_case(cache, "A", 14, inputs=inputs, key="b260", label="A k=14 260 molecules")
    rb = hm.engine.upload(_hip.pack_inputs(inputs))
    assert hm.engine.batch_info(rb)["tile_rows"] == 64
    rb.free()


def many_neighbours(g_update=True):
    """three structures, the middle one of 100 atoms with atoms of 99, 65 and 70 neighbours: chunk tiles and edge_merge_kernel"""
    rng = np.random.default_rng(11)
    A = 100
    degs = {0: 99, 1: 65, 7: 70}
    nb = []
    for a in range(A):
        d = degs.get(a, int(rng.integers(0, 9)))
        js = rng.choice(np.delete(np.arange(A), a), d, replace=False)
        ang = rng.uniform(0.4, 3.5, size=d)
        nb.append([[6, int(j), float(ang[i]), float(ang[i] / ang.max()), float(rng.uniform(0.9, 4.0))] for i, j in enumerate(js)])
    de, dn = so.synth_dataset(2, 3)
    de3, dn3 = np.empty(3, dtype=object), np.empty(3, dtype=object)
    de3[0], dn3[0] = de[0], dn[0]
    de3[1], dn3[1] = [[int(z) for z in rng.choice([1, 6, 7, 8], A)], 0.0], nb
    de3[2], dn3[2] = de[1], dn[1]
    return so.pad_batch(de3, dn3, g_update)[0]


def test_small_centres_with_more_than_64_neighbours(hip_lib, cache):
    from scann import _hip

    inputs = many_neighbours()
    _, _, _, _, hm, _ = run_case(cache, "A", 14, inputs=inputs, key="big", label="A k=14 >64 neighbours")
    rb = hm.engine.upload(_hip.pack_inputs(inputs))
    assert hm.engine.batch_info(rb)["big_atoms"] == 3
    rb.free()


@pytest.mark.parametrize("k", [0, 14])
def test_exact_zeros_are_not_small(hip_lib, cache, k):
    """an isolated atom, padded atom rows, masked neighbour slots, and a checkpoint with exact zeros in it -- a pruned kernel column, a
    LayerNorm beta and a bias that are 0 -- are representable: on their own (k = 0) they leave the handle on the fast path, and with
    case A's small centres (k = 14) the numbers still meet the bound"""
    from scann.models.scann_model import HipModel

    cfg = sr.config()
    inputs = {n: np.array(v) for n, v in qm9_inputs(cfg).items()}
    inputs["neighbor_mask"][3, 2, :] = False
    assert not inputs["atom_mask"].all()  # padded rows
    w = sr.scaled(base_weights(cache, cfg), "A", k)
    w["local_attention_1/key/kernel"] = w["local_attention_1/key/kernel"].copy()
    w["local_attention_1/key/kernel"][:, 5] = 0
    for n in ("local_attention_0/layer_norm/beta", "after_Lc/bias", "residual_norm_1/dense_1/bias"):
        w[n] = np.zeros_like(w[n])
    hm = HipModel(cfg, w, device=0, infer=True)
    check_model(hm, cfg, w, inputs, sr.references(cfg, w, inputs), "A k=%d zeros, isolated atom" % k)
    assert hm.engine.weights_exact() == (k == 14)


# ---- 3. every way a forward's numbers leave the handle: case A, k = 14 ----

def refused(call, reason):
    """None if call() raised the error that names the tensor and the cause, else its result: an entry point either meets its bound
    or refuses -- the policy a checkpoint with |w| >= 255.9 already follows for training and MC dropout"""
    from scann import _hip

    try:
        out = call()
    except _hip.ScannHipError as e:
        assert reason is not None, str(e)
        assert e.code == -2 and reason.split(":")[0] in str(e) and "2^-8" in str(e), str(e)
        print("LOWRANGE refused: %s" % e)
        return None
    return out


@pytest.fixture(scope="module")
def a14(cache):
    cfg = sr.config()
    w = sr.scaled(base_weights(cache, cfg), "A", 14)
    inputs = cache(("inputs", True), lambda: qm9_inputs(cfg))
    refs = cache(("refs", "A", 14, (), None), lambda: sr.references(cfg, w, inputs))
    return cfg, w, inputs, refs


def y_ga_ok(y, ga, refs, label, exact=True):
    r32, r64 = refs
    rows = sr.judge({"predict_property": np.reshape(y, r64["predict_property"].shape), "global_attention": np.reshape(ga, r64["global_attention"].shape)},
                    r32, r64)
    report(label, rows, exact)
    assert not sr.failures(rows), (label, rows)


def test_padded_packed_resident_and_dataset_paths(hip_lib, a14):
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg, w, inputs, refs = a14
    hm = HipModel(cfg, w, device=0, infer=True)
    eng = hm.engine
    y, ga = hm.predict(inputs)
    y_ga_ok(y, ga, refs, "A k=14 predict(padded)", eng.weights_exact())
    pk = _hip.pack_inputs(inputs)
    yp, gap = hm.predict(pk)
    assert np.array_equal(yp, y) and np.array_equal(gap, ga)
    names = sr.output_names(cfg)
    packed = hm.predict(pk, outputs=names)
    padded = hm.predict(inputs, outputs=names)
    amask = inputs["atom_mask"][..., 0] != 0
    em = inputs["neighbor_mask"] & amask[:, :, None]
    for n, g, p in zip(names, padded, packed):  # (the padded outputs were judged by test_small_operands_keep_the_bound)
        want = g.transpose(0, 2, 3, 1)[em] if n.startswith("local_attention_") else g[amask] if n == "after_Lc" else g
        assert np.array_equal(p, want), n
    # two resident batches on two streams, then their downloads
    rb1, rb2 = eng.upload(pk), eng.upload(pk)
    eng.forward_resident(rb1, 0)
    eng.forward_resident(rb2, 1)
    for rb in (rb1, rb2):
        yr, gar = eng.download(rb)
        assert np.array_equal(yr, y[:, 0]) and np.array_equal(pk.repad_ga(gar), ga)
        rb.free()
    # the dataset pipeline: the same structures in three batches
    parts = []
    for s in (slice(0, 3), slice(3, 6), slice(6, 8)):
        parts.append(({n: np.asarray(v)[s] for n, v in inputs.items()}, np.zeros(len(range(8)[s]), "float32")))
    yd, gad, _ = hm.predict_dataset(parts, group=2, want_ga=True)
    r32, r64 = refs
    rows = sr.judge({"predict_property": yd.reshape(-1, 1)}, r32, r64)
    report("A k=14 predict_dataset", rows, eng.weights_exact())
    assert not sr.failures(rows)
    assert tp.rel_err(np.concatenate([np.ravel(g) for g in gad]) if isinstance(gad, list) else gad, r64["global_attention"][amask].ravel()) <= \
        max(tp.RTOL, 2 * tp.rel_err(r32["global_attention"], r64["global_attention"]))
    assert eng.exact_reruns() == 0


def test_model_set_with_a_small_and_an_ordinary_member(hip_lib, cache, a14):
    from scann.models import ModelSet

    cfg, w, inputs, refs = a14
    w0 = base_weights(cache, cfg)
    refs0 = cache(("refs", "A", 0, (), None), lambda: sr.references(cfg, w0, inputs))
    got = ModelSet([(cfg, w), (cfg, w0)], device=0).predict(inputs)
    y_ga_ok(got["predict_property"][0], got["global_attention"][0], refs, "A k=14 set member 0 (small)")
    y_ga_ok(got["predict_property"][1], got["global_attention"][1], refs0, "A k=14 set member 1 (ordinary)", False)
    alone = ModelSet([(cfg, w0), (cfg, w0)], device=0).predict(inputs)  # the ordinary member keeps the bytes it has beside an ordinary one
    assert np.array_equal(got["predict_property"][1], alone["predict_property"][1])
    assert np.array_equal(got["global_attention"][1], alone["global_attention"][1])


def test_input_gradients_meet_their_bound_or_are_refused(hip_lib, a14):
    from scann import _hip
    from scann.models.scann_model import HipModel

    ti = _load("test_gpu_input_grads")
    cfg, w, inputs, _ = a14
    pk = _hip.pack_inputs(inputs)
    hm = HipModel(cfg, w, device=0, infer=True)
    got = refused(lambda: hm.input_gradients(pk), sr.small_operands(cfg, w))
    if got is not None:
        ti.check(got, cfg, w, pk)


def test_mc_dropout_meets_its_bound_or_is_refused(hip_lib, a14):
    """with both rates 0 every sample is the plain forward: its mean is held to the forward's bound, its deviation is 0"""
    from scann.models.scann_model import HipModel

    cfg, w, inputs, refs = a14
    hm = HipModel(cfg, w, device=0, infer=True)
    got = refused(lambda: hm.predict_uncertainty(inputs, samples=2, rate=0.0, attention_rate=0.0), sr.small_operands(cfg, w))
    if got is not None:
        y_ga_ok(got["predict_property"], got["global_attention"], refs, "A k=14 predict_mc", hm.engine.weights_exact())
        assert not got["predict_property_std"].any()


def test_training_meets_its_bound_or_is_refused(hip_lib, a14):
    """train_forward + train_backward under check_grads, or scann_train_begin's refusal; a debug forward of a training handle too"""
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg, w, inputs, _ = a14
    pk = _hip.pack_inputs(inputs)
    targets = np.random.default_rng(2).normal(0, 1, pk.n_struct).astype(np.float32)
    hm = HipModel(cfg, w, device=0)
    eng = hm.engine
    reason = sr.small_operands(cfg, w)
    if refused(lambda: (eng.train_begin(), True)[1], reason) is None:
        return
    rb = eng.upload(pk)
    sse = eng.train_forward(rb, targets, dropout=0.0, seed=0)
    eng.zero_grads()
    eng.train_backward(rb, sse, pk.n_struct)
    got = eng.get_grads()
    rb.free()
    tg.check_grads(got, cfg, w, pk, targets)


# ---- 4. no false alarms ----

def test_ordinary_checkpoints_stay_on_the_fast_path(hip_lib):
    """the default qm9 / mp2018 checkpoints, the Keras-default initialisation, the golden models and the Keras-layout fixture: not
    weights_exact, nothing re-run (their bytes are pinned by the golden / bits tests)"""
    from scann.models.scann_model import HipModel

    for label, cfg, w, inputs in sr.ordinary_checkpoints():
        hm = HipModel(cfg, w, device=0, infer=True)
        y = hm.predict(inputs)[0]
        assert np.isfinite(y).all(), label
        assert not hm.engine.weights_exact() and hm.engine.exact_reruns() == 0, label
