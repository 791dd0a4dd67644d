"""GPU: batches whose tensors pass 2^31 bytes, up to the upload limit (tests/size_batches.py: qm9_x118, sparse_x123, qm9_at_limit,
qm9_over_limit; tests/test_sizes_host.py pins their row counts without a GPU).

The atom and edge kernels address a tensor row as base + an unsigned 32-bit byte offset, which is why scann_batch_upload refuses a batch
of more than UPLOAD_MAX_ROWS = 8,388,607 atoms or edges.  Above SIGNED_OFFSET_ROWS = 4,194,304 rows any signed intermediate in such an
offset goes negative; at the limit the spare row behind the last edge ends 4 bytes below 2^32 and one row further wraps to the start of
the tensor.  A user meets these sizes through HipModel.predict(PackedBatch), engine.upload and concat_packed.

Reference rule.  Every large batch is a small seeded batch tiled n times (plus, at the limit, one filler structure), and a structure's
result does not depend on its batch (test_batch_composition_and_permutation): replica r of the large batch must give THE BYTES the small
batch gives when it is forwarded alone -- every replica is compared (a reshape and one ==), none sampled.  Replica boundaries do not fall
on tile boundaries, and the second forward of a resident batch runs on the filled tile plan.  The small batch alone is compared in the
same test with the fp64 / fp32 oracle (gradients: fp64 autograd) under the bound the suite uses for it at small size, so the chain ends in
a high-precision reference and not in the code under test.  A wrong offset at these sizes may also show as a GPU fault rather than as a
wrong number: the cases are ordered smallest first.

Not covered: sparse_x123 cut or extended to UPLOAD_MAX_ROWS ATOMS -- its edges (1.5 per atom) would then pass the limit too, so the
atom tensors' last admitted row is not reached by any batch the upload admits with this degree distribution; the limit is tested on the
edge rows (qm9_at_limit).

Memory: these batches take device memory in the tens of gigabytes.  A case skips only when the upload, train_begin or a forward returns
the library's out-of-memory status (the message is the skip reason); one large batch is resident at a time, freed in a `finally`.  Every
case appends its rows, the bytes of its largest tensor, its wall time and the device memory it took to RECORD_LINES
(tools/large_rows_record.py writes them to profiles/large_rows.txt)."""
import contextlib
import time

import numpy as np
import pytest

import scann_oracle as so
import size_batches as sb
import test_gpu_training as tg
from test_gpu_mc_sizes import check_oracle as check_mc_oracle, keys_of, oracle as mc_oracle
from test_gpu_outputs import all_names, check_against_oracle
from test_gpu_parity import RTOL, rel_err, strict_rel_err
from test_gpu_tile_fill import check_plan

pytestmark = pytest.mark.gpu

SCANN_ERR_UNSUPPORTED, SCANN_ERR_OOM = -2, -6  # include/scann_hip.h
LIMIT_MESSAGE = "scann_batch_upload: more than 8,388,607 atoms or edges in one batch; split it"  # scann_batch.cpp upload_impl
W64 = dict(local_dim=64, num_head=4, global_dim=96, dense_out=32)
W256 = dict(local_dim=256, num_head=8)
RECORD_LINES = []  # "case  atoms  edges  largest tensor  wall  device memory  [skipped: why]" of every case this module has run


@pytest.fixture(scope="module")
def cache():
    """key -> value, computed on first use for the whole module"""
    store = {}

    def get(key, make):
        if key not in store:
            store[key] = make()
        return store[key]

    return get


def config(L, g_update=True, widths=None, **over):
    cfg = so.default_config("qm9")
    cfg["model"].update(n_attention=L, g_update=g_update, **over)
    if widths:
        cfg["model"].update(widths)
        cfg["model"]["n_atoms"] = 100  # (setup_widths of test_gpu_training.py)
    return cfg, so.init_weights(cfg, 3, perturb=True)


def large(cache, name, g_update=True):
    """(large PackedBatch, replicas, small PackedBatch, the small batch's padded inputs, its targets)"""
    def make():
        big, n, small = getattr(sb, name)(g_update)
        data = sb.sparse_atoms_data() if name == "sparse_x123" else sb.qm9_b260_data()
        inputs, targets = sb.padded(data, g_update)
        return big, n, small, inputs, np.asarray(targets, np.float32)

    return cache(("batch", name, g_update), make)


@contextlib.contextmanager
def case(label, pk, width=128):
    """one line of RECORD_LINES per case: rows, bytes of its largest tensor ([max(atoms, edges), width] fp32), wall time, device memory
    taken (entry["memory"], set by `resident`), and the reason if it skipped"""
    entry = {"memory": None}
    t0 = time.perf_counter()
    why = ""
    try:
        yield entry
    except pytest.skip.Exception as e:
        why = "  skipped: %s" % e
        raise
    finally:
        mem = "not measured" if entry["memory"] is None else "%.1f GB" % (entry["memory"] / 1e9)
        line = "%-44s atoms %-9d edges %-9d largest tensor [%d, %d] %.3e bytes  wall %.1f s  device memory %s%s" % (
            label, pk.n_atom, pk.n_edge, max(pk.n_atom, pk.n_edge), width, max(pk.n_atom, pk.n_edge) * width * 4.0,
            time.perf_counter() - t0, mem, why)
        print(line)
        RECORD_LINES.append(line)


@contextlib.contextmanager
def out_of_memory_skips():
    """the library's out-of-memory status, and nothing else, skips"""
    from scann import _hip

    try:
        yield
    except _hip.ScannHipError as e:
        if e.code == SCANN_ERR_OOM:
            pytest.skip("out of device memory: %s" % e)
        raise


@contextlib.contextmanager
def resident(eng, pk, entry=None):
    """`pk` uploaded, and freed whatever happens; entry["memory"]: the device's free bytes before the upload minus those when the case is
    done with the batch (hipMemGetInfo: blocks the process had cached from earlier batches are not counted)"""
    free0 = eng.device_memory()[0]
    with out_of_memory_skips():
        rb = eng.upload(pk)
    try:
        info = eng.batch_info(rb)
        assert (info["structs"], info["atoms"], info["edges"]) == (pk.n_struct, pk.n_atom, pk.n_edge), info
        yield rb
        if entry is not None:
            entry["memory"] = free0 - eng.device_memory()[0]
    finally:
        rb.free()


def same_replicas(label, got, want, n, rest=None):
    """the first n * len(want) rows of `got` are `want` n times over, bit for bit; the rows behind them are `rest` (None: there are none).
    A failure names the first differing replica and element"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    rows = want.shape[0]
    assert got.shape[1:] == want.shape[1:] and got.shape[0] == n * rows + (0 if rest is None else len(rest)), (label, got.shape, want.shape, n)
    diff = got[:n * rows].reshape((n,) + want.shape).view(np.uint32) != want.view(np.uint32)[None]
    if diff.any():
        idx = tuple(int(i) for i in np.argwhere(diff)[0])
        raise AssertionError("%s: %d of %d values differ in %d of %d replicas, first in replica %d at %s: %r != %r" % (
            label, int(diff.sum()), diff.size, int(diff.reshape(n, -1).any(1).sum()), n, idx[0], idx[1:],
            got[:n * rows].reshape((n,) + want.shape)[idx], want[idx[1:]]))
    if rest is not None:
        rest = np.ascontiguousarray(rest, np.float32)
        d2 = got[n * rows:].view(np.uint32) != rest.view(np.uint32)
        assert not d2.any(), "%s: %d of %d values of the structure behind the replicas differ, first at %s" % (
            label, int(d2.sum()), d2.size, tuple(int(i) for i in np.argwhere(d2)[0]))


def forward_alone(model, pk, outputs=0):
    """{"y", "ga"} (and the selected outputs of `outputs` layers) of `pk` uploaded and forwarded once"""
    return forwards(model, pk, None, 1, outputs)[0]


def forwards(model, pk, filled, n, outputs=0, entry=None):
    """the results of `n` forwards of `pk` uploaded once.  filled not None: the batch is on 64-row tiles without chunk tiles, its first
    forward runs on the contiguous tile plan, the second makes the filled one (scann_batch_tile_plan) if `filled`"""
    from scann import _hip

    eng = model.engine
    runs = []
    with resident(eng, pk, entry) as rb:
        try:
            if outputs:
                eng.set_outputs(range(outputs), after_lc=True, bf_property=True)
            for i in range(n):
                if filled is not None:
                    check_plan(eng, rb, pk, 64, 0, filled and i > 1)
                with out_of_memory_skips():
                    eng.forward_resident(rb, 0)
                    out = dict(zip(("y", "ga"), eng.download(rb)))
                if outputs:
                    out.update({"local_attention_%d" % k: eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, k) for k in range(outputs)})
                    out["after_Lc"] = eng.read_output(rb, _hip.OUT_AFTER_LC)
                    out["bf_property"] = eng.read_output(rb, _hip.OUT_BF_PROPERTY)
                runs.append(out)
            if filled is not None and n > 1:
                check_plan(eng, rb, pk, 64, 0, filled)
        finally:
            eng.set_outputs()
    return runs


def check_small_against_oracle(label, cfg, w, small, inputs, got, cache, key, widths=False):
    """y and the GlobalAttention scores of the small batch alone against the NumPy oracle in fp64, under test_branches' /
    test_widths_other_than_128_and_8_heads' bound max(RTOL, 2 x the fp32 oracle's own error against fp64); where the graph is the shipped
    g_update one also rel_err <= RTOL against the fp32 oracle (test_forward_matches_oracle_qm9)"""
    y32, ga32 = cache(("oracle32",) + key, lambda: so.forward(cfg, w, inputs, np.float32))
    y64, ga64 = cache(("oracle64",) + key, lambda: so.forward(cfg, w, inputs, np.float64))
    y, ga = got["y"].reshape(-1, 1), small.repad_ga(got["ga"])
    e_y, e_ga = rel_err(y, y64), rel_err(ga, ga64)
    b_y, b_ga = max(RTOL, 2 * rel_err(y32, y64)), max(RTOL, 2 * rel_err(ga32, ga64))
    print("%s: small batch against the fp64 oracle: y %.2e (bound %.2e) ga %.2e (bound %.2e)" % (label, e_y, b_y, e_ga, b_ga))
    assert e_y <= b_y and e_ga <= b_ga, (label, e_y, b_y, e_ga, b_ga)
    if cfg["model"]["g_update"] and not widths:
        assert rel_err(y, y32) <= RTOL and rel_err(ga, ga32) <= RTOL, (label, rel_err(y, y32), rel_err(ga, ga32))
    if widths:
        assert strict_rel_err(y, y32) <= 10 * RTOL, (label, strict_rel_err(y, y32))


# ---- 1. inference at 2^31: both batches, both branches, both tile plans ----

@pytest.mark.parametrize("name,g_update", [("qm9_x118", True), ("qm9_x118", False), ("sparse_x123", True)],
                         ids=["qm9_x118-g_update", "qm9_x118-base", "sparse_x123-g_update"])
def test_every_replica_is_the_small_batch_forwarded_alone(hip_lib, cache, name, g_update):
    """128 / 8, L = 3: the first, middle and last launch families (test_three_layers_run_the_middle_kernel).  qm9_x118: 4.2 M edges, the
    edge tensors pass 2^31 bytes (g_update: piece-major tiles, the second forward on the filled plan; base: the row-major kernel and the
    [E, 20] basis).  sparse_x123: 4.2 M atoms, isolated ones among them, and 6.3 M edges -- 96/128-row atom tiles past 2^31 bytes as well"""
    from scann.models.scann_model import HipModel

    big, n, small, inputs, _ = large(cache, name, g_update)
    assert big.n_edge > sb.SIGNED_OFFSET_ROWS and (name != "sparse_x123" or big.n_atom > sb.SIGNED_OFFSET_ROWS)
    cfg, w = config(3, g_update)
    model = HipModel(cfg, w, device=0, infer=True)
    label = "inference %s %s" % (name, "g_update" if g_update else "base")
    filled = g_update and name == "qm9_x118"  # (sparse_x123: the atom limit closes the tiles of either plan; base: no tile-order side)
    with case(label, big) as entry:
        alone = forward_alone(model, small)
        check_small_against_oracle(label, cfg, w, small, inputs, alone, cache, (name, g_update, 3))
        assert np.isfinite(alone["y"]).all() and len(np.unique(alone["y"])) > small.n_struct // 2
        runs = forwards(model, big, filled, 2, entry=entry)
        for i, r in enumerate(runs):
            same_replicas("%s, forward %d: y" % (label, i), r["y"], alone["y"], n)
            same_replicas("%s, forward %d: ga" % (label, i), r["ga"], alone["ga"], n)


# ---- 2. selected outputs, Monte Carlo dropout, input gradients ----

def test_selected_outputs_of_every_replica(hip_lib, cache):
    """every local_attention_<k> ([n_edge, 8]: the caller's edge numbers past 2^22), after_Lc and bf_property on qm9_x118, both plans"""
    from scann import _hip
    from scann.models.scann_model import HipModel

    big, n, small, inputs, _ = large(cache, "qm9_x118")
    cfg, w = config(3)
    names = all_names(cfg)
    model = HipModel(cfg, w, device=0, infer=True)
    with case("selected outputs qm9_x118", big) as entry:
        alone = forward_alone(model, small, outputs=3)
        padded = [_hip.repad_local_attention(alone[k], inputs["atom_mask"], inputs["neighbor_mask"]) if k.startswith("local_attention_")
                  else _hip.repad_atoms(alone[k], inputs["atom_mask"]) if k == "after_Lc" else alone[k] for k in names]
        check_against_oracle(cfg, w, inputs, padded, names)                    # the fp32 oracle at RTOL
        check_against_oracle(cfg, w, inputs, padded, names, fp64_bound=True)   # the fp64 oracle at max(RTOL, 2 x the fp32 oracle's error)
        runs = forwards(model, big, True, 2, outputs=3, entry=entry)
        for i, r in enumerate(runs):
            for k in names + ["y", "ga"]:
                same_replicas("selected outputs, forward %d: %s" % (i, k), r[k], alone[k], n)


def test_monte_carlo_samples_of_every_replica(hip_lib, monkeypatch, cache):
    """scann_predict_mc, T = 2, both rates active; replica r of structure s carries key s, so it draws structure s's masks
    (test_gpu_mc_dropout.py::test_batch_invariance states the property).  The small batch's samples and its GA mean / std are held to
    the torch fp64 restatement run with the same structure-local masks, under test_gpu_mc_sizes.check_oracle's rule:
    rel_err(y_gpu, y64) <= max(RTOL, 2 rel_err(y32, y64)) per sample, 10 RTOL for the GA reductions"""
    from scann.models.scann_model import HipModel

    big, n, small, _, _ = large(cache, "qm9_x118")
    cfg, w = config(3, use_drop=True)
    eng = HipModel(cfg, w, device=0, infer=True).engine
    keys = keys_of(small.n_struct)
    seed, rates = 11, (0.1, 0.05)
    kw = dict(seed=seed, p_drop=rates[0], p_attn=rates[1], want_samples=True)
    with case("monte carlo dropout qm9_x118", big) as entry:
        with resident(eng, small) as rb:
            alone = eng.predict_mc(rb, 2, keys=keys, **kw)
        assert not np.array_equal(alone["y_samples"][0], alone["y_samples"][1]) and np.isfinite(alone["y_samples"]).all()
        ref = mc_oracle(cache, ("qm9_b260", 3, seed) + rates, cfg, w, small, 2, keys, rates, monkeypatch, seed=seed)
        check_mc_oracle("large rows: qm9_b260 alone, drop+attn", small, alone, ref)
        with resident(eng, big, entry) as rb:
            got = []
            for call in range(2):  # (the first call's second sample and the second call run on the filled plan)
                check_plan(eng, rb, big, 64, 0, call > 0)
                with out_of_memory_skips():
                    got.append(eng.predict_mc(rb, 2, keys=np.tile(keys, n), **kw))
            check_plan(eng, rb, big, 64, 0, True)
        for call, r in enumerate(got):
            for k in ("y_mean", "y_std", "ga_mean", "ga_std"):
                same_replicas("predict_mc call %d: %s" % (call, k), r[k], alone[k], n)
            for t in range(2):
                same_replicas("predict_mc call %d: sample %d" % (call, t), r["y_samples"][t], alone["y_samples"][t], n)


def test_input_gradients_of_every_replica(hip_lib, cache):
    """d y_s / d neighbor_distance and d neighbor_weight ([n_edge]) on qm9_x118, under the comparison of
    test_a_structure_alone_matches_it_inside_a_mixed_batch: the replicas' gradients and the small batch's against fp64 autograd of the
    small batch by check's rule (max(GRAD_FLOOR, GRAD_SLACK x the fp32 graph's error), capped), and a replica against the small batch
    alone within max(GRAD_FLOOR, 2 x the larger of their two errors) -- that comparison is not bitwise at small size either"""
    import input_grad_ref
    import test_gpu_input_grads as ig
    from scann.models.scann_model import HipModel

    big, n, small, _, _ = large(cache, "qm9_x118")
    cfg, w = config(2)
    eng = HipModel(cfg, w, device=0, infer=True).engine
    wrt = ("neighbor_distance", "neighbor_weight")
    with case("input gradients qm9_x118", big) as entry:
        y64, ref = input_grad_ref.input_grads(cfg, w, small)
        _, g32 = input_grad_ref.input_grads(cfg, w, small, dtype="float32")
        e_32 = ig.errors(g32, ref)
        bound = {k: min(ig.GRAD_CAP, max(ig.GRAD_FLOOR, ig.GRAD_SLACK * e_32[k])) for k in wrt}
        with resident(eng, small) as rb:
            alone = eng.input_grads(rb)
        with resident(eng, big, entry) as rb:
            with out_of_memory_skips():
                got = eng.input_grads(rb)
        e_alone = ig.errors(alone, {k: ref[k] for k in wrt})
        assert all(e_alone[k] <= bound[k] for k in wrt), (e_alone, bound)
        scale_y = max(float(np.sqrt(np.mean(y64 ** 2))), 1e-6)
        assert np.max(np.abs(alone["y"] - y64)) <= 1e-4 * scale_y
        same_replicas("input gradients: y", got["y"], alone["y"], n)
        for k in wrt:
            r = ref[k]
            norm = max(float(np.abs(r).max()), float(np.sqrt(np.mean(r * r))), 1e-12)  # (errors()' normalisation)
            g = np.asarray(got[k], np.float64).reshape(n, -1)
            e_rep = np.abs(g - r[None]).max(1) / norm  # each replica against fp64 autograd
            assert (e_rep <= bound[k]).all(), (k, int(np.argmax(e_rep)), float(e_rep.max()), bound[k])
            a = np.asarray(alone[k], np.float64)
            norm_a = max(float(np.abs(a).max()), float(np.sqrt(np.mean(a * a))), 1e-12)
            d_rep = np.abs(g - a[None]).max(1) / norm_a  # ... and against the small batch alone
            lim = np.maximum(ig.GRAD_FLOOR, 2 * np.maximum(e_rep, e_alone[k]))
            assert (d_rep <= lim).all(), (k, int(np.argmax(d_rep - lim)), float(d_rep.max()))
            print("input gradients %s: worst replica against autograd %.2e (alone %.2e, bound %.2e), against alone %.2e" % (
                k, e_rep.max(), e_alone[k], bound[k], d_rep.max()))


# ---- 3. training: fused, modular, deterministic ----

def train_config():
    return config(2)  # (config("qm9_b260") of test_gpu_sizes.py)


def grad_refs(cache, cfg, w, small, targets):
    return cache(("grads", "qm9_b260"), lambda: tg.grad_reference(cfg, w, small, targets))


def step_grads(eng, rb, targets, count):
    with out_of_memory_skips():
        sse = eng.train_forward(rb, targets)
        eng.zero_grads()
        eng.train_backward(rb, sse, count)
    return sse, eng.get_grads()


def check_step_then_forward(eng, rb_big, small, n, cfg, inputs):
    """one adam_step, then a forward of the large batch and of the small one on the same handle: the repacked weight images and the
    inference kernels see the handle the training kernels just wrote.  The small batch's y is held to the fp64 oracle run on the
    weights the handle reports after the step (get_weights), under max(RTOL, 2 x the fp32 oracle's own error)"""
    eng.adam_step(1e-3)
    eng.forward_resident(rb_big, 0)
    y, ga = eng.download(rb_big)
    with resident(eng, small) as rb:
        eng.forward_resident(rb, 0)
        y_s, ga_s = eng.download(rb)
    assert np.isfinite(y_s).all()
    w1 = eng.get_weights()
    y32, y64 = so.forward(cfg, w1, inputs, np.float32)[0], so.forward(cfg, w1, inputs, np.float64)[0]
    e, b = rel_err(y_s.reshape(-1, 1), y64), max(RTOL, 2 * rel_err(y32, y64))
    print("forward after adam_step: small batch against the fp64 oracle on the stepped weights: y %.2e (bound %.2e)" % (e, b))
    assert e <= b, (e, b)
    same_replicas("forward after adam_step: y", y, y_s, n)
    same_replicas("forward after adam_step: ga", ga, ga_s, n)
    return y_s


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "modular"])
def test_training_gradients_of_the_replicated_batch_match_autograd(hip_lib, monkeypatch, cache, fused):
    """qm9_x118, L = 2, targets tiled: the loss of the replicated batch is the small batch's loss and its gradient is mathematically the
    small batch's gradient, so check_grads holds it to the fp64 autograd of the small batch alone (rule and constants unchanged), with
    the fused backward kernels and with the modular ones; then one adam_step and a forward on the same handle"""
    from scann.models.scann_model import HipModel

    big, n, small, inputs, targets = large(cache, "qm9_x118")
    cfg, w = train_config()
    monkeypatch.setenv("SCANN_TRAIN_FUSED", fused)
    eng = HipModel(cfg, w, device=0).engine
    with case("training qm9_x118 %s" % ("fused" if fused == "1" else "modular"), big) as entry:
        refs = grad_refs(cache, cfg, w, small, targets)
        with out_of_memory_skips():
            eng.train_begin()
        y0 = None
        with resident(eng, big, entry) as rb:
            sse, got = step_grads(eng, rb, np.tile(targets, n), big.n_struct)
            rmse, e_gpu = tg.check_grads(got, cfg, w, small, targets, refs=refs)
            got_rmse = np.sqrt(sse / big.n_struct)
            assert abs(got_rmse - rmse) <= 1e-5 * max(rmse, 1e-6), (got_rmse, rmse)
            w0 = eng.get_weights()
            y0 = check_step_then_forward(eng, rb, small, n, cfg, inputs)
            w1 = eng.get_weights()
        assert any(not np.array_equal(w0[k], w1[k]) for k in w0)  # (the step moved the weights the forward then ran on)
        print("training fused=%s: worst gradient error %.2e, rmse rel err %.2e, |y| after the step %.3f" % (
            fused, max(e_gpu.values()), abs(got_rmse - rmse) / rmse, float(np.abs(y0).mean())))


def test_deterministic_training_of_the_replicated_batch_is_bitwise_reproducible(hip_lib, cache):
    """deterministic mode on qm9_x118: two runs of the step give the same bits in every gradient, and those match autograd"""
    from scann.models.scann_model import HipModel

    big, n, small, inputs, targets = large(cache, "qm9_x118")
    cfg, w = train_config()
    eng = HipModel(cfg, w, device=0).engine
    with case("training qm9_x118 deterministic", big) as entry:
        refs = grad_refs(cache, cfg, w, small, targets)
        with out_of_memory_skips():
            eng.train_begin()
        eng.set_deterministic(True)
        with resident(eng, big, entry) as rb:
            t = np.tile(targets, n)
            sse_a, a = step_grads(eng, rb, t, big.n_struct)
            sse_b, b = step_grads(eng, rb, t, big.n_struct)
            assert sse_a == sse_b
            differ = [k for k in a if not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))]
            assert not differ, differ
            rmse, _ = tg.check_grads(a, cfg, w, small, targets, refs=refs)
            assert abs(np.sqrt(sse_a / big.n_struct) - rmse) <= 1e-5 * max(rmse, 1e-6)
            check_step_then_forward(eng, rb, small, n, cfg, inputs)


# ---- 4. the upload limit ----

def limit_case(cache, model, cfg, w, label, width, key, widths=False, n_forward=2):
    """qm9_at_limit: every replica equals the small batch alone, the filler structure (the last rows below 2^32 bytes) equals the filler
    alone; both alone against the oracle"""
    big, n, small, inputs, _ = large(cache, "qm9_at_limit")
    assert big.n_edge == sb.UPLOAD_MAX_ROWS
    filler = sb.limit_filler()
    f_inputs, _ = sb.padded(sb.limit_filler_data())
    with case(label, big, width) as entry:
        alone, f_alone = forward_alone(model, small), forward_alone(model, filler)
        check_small_against_oracle(label, cfg, w, small, inputs, alone, cache, ("qm9_b260",) + key, widths)
        check_small_against_oracle(label + " (filler)", cfg, w, filler, f_inputs, f_alone, cache, ("filler",) + key, widths)
        filled = None if widths else True
        for i, r in enumerate(forwards(model, big, filled, n_forward, entry=entry)):
            same_replicas("%s, forward %d: y" % (label, i), r["y"], alone["y"], n, rest=f_alone["y"])
            same_replicas("%s, forward %d: ga" % (label, i), r["ga"], alone["ga"], n, rest=f_alone["ga"])


def test_the_last_admitted_row(hip_lib, cache):
    """exactly UPLOAD_MAX_ROWS edges on the 128 / 8 kernels, L = 3, forwarded twice (contiguous, then filled plan)"""
    from scann.models.scann_model import HipModel

    cfg, w = config(3)
    limit_case(cache, HipModel(cfg, w, device=0, infer=True), cfg, w, "limit qm9_at_limit 128/8", 128, (True, 3))


def test_one_edge_more_is_refused_at_upload(hip_lib, cache):
    """UPLOAD_MAX_ROWS + 1 edges: SCANN_ERR_UNSUPPORTED with the text of scann_batch.cpp, from the check in front of every allocation"""
    from scann import _hip
    from scann.models.scann_model import HipModel

    over, _, _ = sb.qm9_over_limit()
    assert over.n_edge == sb.UPLOAD_MAX_ROWS + 1
    cfg, w = config(3)
    eng = HipModel(cfg, w, device=0, infer=True).engine
    with case("limit qm9_over_limit (refused)", over):
        with pytest.raises(_hip.ScannHipError) as ei:
            eng.upload(over).free()
        assert ei.value.code == SCANN_ERR_UNSUPPORTED and LIMIT_MESSAGE in str(ei.value), (ei.value.code, str(ei.value))


# ---- 5. widths other than 128: the plain-fp32 kernels ----

def test_the_limit_at_64_wide(hip_lib, cache):
    """64 / 4 (global_dim 96, dense_out 32), L = 2 on qm9_at_limit: the plain-fp32 kernels' [E, 64] tensors end 256 bytes below 2^31
    (the last admitted row is the last below it), their [E, 192] concatenations and workspace offsets lie far beyond"""
    from scann.models.scann_model import HipModel

    cfg, w = config(2, widths=W64)
    limit_case(cache, HipModel(cfg, w, device=0, infer=True), cfg, w, "limit qm9_at_limit 64/4", 64, ("64x4", 2), widths=True, n_forward=1)


def test_256_wide_tensors_pass_two_to_the_32_bytes(hip_lib, cache):
    """256 / 8, L = 2 on qm9_x118: the upload limit is computed for 128 columns whatever the model's width, so it admits this batch,
    whose [E, 256] tensors are 4.3e9 bytes -- the plain-fp32 kernels index in 64 bits"""
    from scann.models.scann_model import HipModel

    big, n, small, inputs, _ = large(cache, "qm9_x118")
    assert big.n_edge * 256 * 4 > 1 << 32
    cfg, w = config(2, widths=W256)
    model = HipModel(cfg, w, device=0, infer=True)
    label = "widths qm9_x118 256/8"
    with case(label, big, 256) as entry:
        alone = forward_alone(model, small)
        check_small_against_oracle(label, cfg, w, small, inputs, alone, cache, ("qm9_b260", "256x8", 2), widths=True)
        (r,) = forwards(model, big, None, 1, entry=entry)
        same_replicas(label + ": y", r["y"], alone["y"], n)
        same_replicas(label + ": ga", r["ga"], alone["ga"], n)
