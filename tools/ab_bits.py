"""Do two builds of the library give the same bytes on every route into the forward schedule?
    python tools/ab_bits.py libA.so libB.so [...]
Each library runs the scenarios below in a child process of its own and prints one digest per scenario, by name; a scenario whose
digests differ between the libraries is named at the end.  (The same library given twice shows what is not reproducible by itself.)"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import copy, hashlib, os, sys
import numpy as np
ROOT = sys.argv[1]
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle")]
import scann_oracle as so
from scann import _hip
from scann.models import ModelSet
from scann.models.scann_model import HipModel

WIDTHS = dict(local_dim=64, num_head=4, global_dim=96, dense_out=32)


def emit(name, parts):  # one digest of everything parts() returns; an error the library reports is an outcome like another
    h = hashlib.sha256()

    def walk(p):
        if isinstance(p, dict):
            p = [p[k] for k in sorted(p)]
        if isinstance(p, (list, tuple)):
            for a in p:
                walk(a)
        elif p is not None:
            h.update(np.ascontiguousarray(p).tobytes())

    try:
        walk(parts())
    except _hip.ScannHipError as e:
        h = hashlib.sha256(("error: %s" % e).encode())
        print("(%s: %s)" % (name, e), file=sys.stderr)
    print("%-34s %s" % (name, h.hexdigest()[:32]), flush=True)


def config(kind="qm9", L=None, target=None, widths=None, **over):
    cfg = so.default_config(kind)
    if L is not None:
        cfg["model"]["n_attention"] = L
    cfg["model"].update(over)
    if widths:
        cfg["model"].update(widths)
        cfg["model"]["n_atoms"] = 100
    if target:
        cfg["hyper"]["target"] = target
    return cfg


def batch(cfg, n, seed):  # (padded inputs, targets, packed batch)
    ring, cg = bool(cfg["model"]["use_ring"]), cfg["model"]["feature"] == "cgcnn"
    de, dn = so.synth_dataset(n, seed, use_ring=ring)
    inputs, t = so.pad_batch(de, dn, cfg["model"]["g_update"], use_ring=ring)
    if cg:
        inputs["atomic"] = np.random.default_rng(5).integers(0, 2, size=(101, 92)).astype("float32")[inputs["atomic"]]
    return inputs, np.asarray(t, np.float32), _hip.pack_inputs(inputs)


def big_batch(g_update):  # one structure whose atoms have 64 neighbours and one atom 65 (chunk tiles, the merge kernels) beside a small one
    rng = np.random.default_rng(0)
    A = 70
    big = [[[6, int(j), float(rng.uniform(0.4, 3.5)), 1.0, float(rng.uniform(0.9, 4.0))]
            for j in rng.choice(np.delete(np.arange(A), a), 64, replace=False)] for a in range(A)]
    big[0].append([6, 1, 1.0, 1.0, 1.0])
    de, dn = so.synth_dataset(1, 3)
    de2, dn2 = np.empty(2, dtype=object), np.empty(2, dtype=object)
    de2[0], dn2[0] = [[6] * A, 0.0], big
    de2[1], dn2[1] = de[0], dn[0]
    inputs, _ = so.pad_batch(de2, dn2, g_update)
    return inputs, _hip.pack_inputs(inputs)


def members(cfg, K, seed=3, targets=None):
    out = []
    for m in range(K):
        c = copy.deepcopy(cfg)
        if targets:
            c["hyper"]["target"] = targets[m]
        out.append((c, so.init_weights(c, seed + 17 * m, perturb=True)))
    return out


def selected_outputs(eng, rb, L):
    return [eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, l) for l in range(L)] + [eng.read_output(rb, _hip.OUT_AFTER_LC),
                                                                                     eng.read_output(rb, _hip.OUT_BF_PROPERTY)]


CONFIGS = {"qm9": config("qm9"), "mp2018": config("mp2018"), "base": config(L=2, g_update=False), "ring": config(L=2, use_ring=True),
           "cgcnn": config(L=2, feature="cgcnn"), "e_b": config(L=2, target="e_b"), "64x4": config(L=2, widths=WIDTHS, use_drop=True)}

# 1. streamed and resident forward
for name in ("qm9", "mp2018", "base", "ring", "64x4"):
    cfg = CONFIGS[name]
    eng = HipModel(cfg, so.init_weights(cfg, 1234, perturb=True), device=0, infer=True).engine
    for n, seed in ((128, 3), (700, 4)) if name in ("qm9", "mp2018") else ((128, 3),):
        pk = batch(cfg, n, seed)[2]
        emit("forward/%s/%d/streamed" % (name, n), lambda: [eng.forward(pk)])
        rb = eng.upload(pk)
        eng.forward_resident(rb, 1)
        emit("forward/%s/%d/resident" % (name, n), lambda: [eng.download(rb)])
        rb.free()

# 2. an atom of more than 64 neighbours, the attention maps of its layers selected
for name, g_update in (("g_update", True), ("base", False)):
    cfg = config(L=2, g_update=g_update)
    eng = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True).engine
    pk = big_batch(g_update)[1]
    emit("big_atom/%s/plain" % name, lambda: [eng.forward(pk)])
    eng.set_outputs([0, 1], after_lc=True, bf_property=True)
    rb = eng.upload(pk)
    eng.forward_resident(rb, 0)
    emit("big_atom/%s/outputs" % name, lambda: [eng.download(rb), selected_outputs(eng, rb, 2)])
    rb.free()

# 4. SCANN_EXACT=1 (read when the handle is created), and a forward whose range guard fires: the download re-runs it exact
os.environ["SCANN_EXACT"] = "1"
for name in ("qm9", "base", "ring"):
    cfg = CONFIGS[name]
    eng = HipModel(cfg, so.init_weights(cfg, 1234, perturb=True), device=0, infer=True).engine
    emit("exact/env/%s" % name, lambda: [eng.forward(batch(cfg, 24, 3)[2])])
del os.environ["SCANN_EXACT"]
cfg = config(L=3)
w = so.init_weights(cfg, 3, perturb=True)
w["after_Lc/bias"] = (w["after_Lc/bias"] + 1.0e5).astype(np.float32)
eng = HipModel(cfg, w, device=0, infer=True).engine
pk = batch(cfg, 6, 1)[2]
eng.set_outputs(range(3), after_lc=True, bf_property=True)
rb = eng.upload(pk)
eng.forward_resident(rb, 1)
emit("exact/range_rerun", lambda: [eng.download(rb), selected_outputs(eng, rb, 3), np.int64(eng.exact_reruns())])
emit("exact/range_rerun/streamed", lambda: [eng.forward(pk), np.int64(eng.exact_reruns())])
rb.free()

# 6. training forward + backward + Adam, deterministic mode, dropout and attention dropout on; the tensors kept for scann_debug_read
for name in ("qm9", "base", "ring", "64x4"):
    cfg = copy.deepcopy(CONFIGS[name])
    cfg["model"]["n_attention"] = 2
    eng = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, deterministic=True).engine
    _, t, pk = batch(cfg, 48, 11)
    eng.train_begin()
    eng.set_attention_dropout(0.05)
    rb = eng.upload(pk)
    sse = eng.train_forward(rb, t, dropout=0.1, seed=5)
    kept = [eng.debug_read(rb, what, 1) for what in (3, 5, 7)] if name == "qm9" else []
    eng.zero_grads()
    eng.train_backward(rb, sse, pk.n_struct)
    emit("train/%s/forward_backward" % name, lambda: [np.float64(sse), eng.download(rb), kept, eng.get_grads()])
    eng.adam_step(1e-3)
    emit("train/%s/adam" % name, lambda: [eng.get_weights()])
    steps = [eng.train_step(rb, t, 1e-3, dropout=0.1, seed=6 + i) for i in range(2)]
    emit("train/%s/two_steps" % name, lambda: [np.float64(steps), eng.get_weights()])
    emit("train/%s/inference_after" % name, lambda: [eng.forward(pk)])
    rb.free()

# 3, 5, 7, 8, 9, 10 on ONE handle per configuration, in this order: selected outputs; scann_set_debug; scann_input_grads under a handle
# rate of attention dropout (the Monte Carlo call after it reads that rate back); scann_predict_mc while outputs are selected; a model set of
# 3 on another slot, then of 4 with one exact-fp32 member; scann_ablate_pooling and scann_attention_rollout
for name in ("qm9", "base", "ring", "cgcnn", "e_b", "64x4"):
    cfg = copy.deepcopy(CONFIGS[name])
    cfg["model"]["n_attention"] = 2
    L, mfma = 2, name != "64x4"
    mem = members(cfg, 3, targets=["e_b", "homo", "e_b"] if name == "e_b" else None)
    ms = ModelSet(mem, device=0)
    eng = ms.engine
    inputs, _, pk = batch(cfg, 6, 1)
    rb = eng.upload(pk)
    eng.set_outputs(range(L), after_lc=True, bf_property=True)
    eng.forward_resident(rb, 0)
    emit("chain/%s/outputs" % name, lambda: [selected_outputs(eng, rb, L), eng.download(rb)])
    eng.set_outputs()
    if mfma:
        eng.set_debug(True)
        eng.forward_resident(rb, 0)
        eng.sync()
        emit("chain/%s/debug" % name, lambda: [[eng.debug_read(rb, what, l) for l in range(L + 1) for what in (0, 1, 2)
                                                if (what != 1 or cfg["model"]["g_update"]) and (what != 2 or l >= 1)], eng.download(rb)])
        eng.set_debug(False)
    eng.set_attention_dropout(0.05)
    emit("chain/%s/input_grads" % name, lambda: [eng.input_grads(rb, ring=name == "ring", cgcnn=name == "cgcnn")])
    emit("chain/%s/mc_after_input_grads" % name, lambda: [eng.predict_mc(rb, 3, seed=9, want_samples=True)])  # (p_attn: the handle's rate)
    eng.set_attention_dropout(0.0)
    eng.set_outputs([0], after_lc=True)
    eng.forward_resident(rb, 0)
    before = [eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 0), eng.read_output(rb, _hip.OUT_AFTER_LC)]
    keys = np.arange(pk.n_struct, dtype=np.uint64) * 7919 + 1
    emit("chain/%s/mc_p_attn_0" % name, lambda: [eng.predict_mc(rb, 4, seed=1, keys=keys, p_attn=0.0, want_samples=True)])
    emit("chain/%s/mc_p_attn_0.05" % name, lambda: [eng.predict_mc(rb, 4, seed=2, keys=keys, p_drop=0.1, p_attn=0.05, want_samples=True)])
    after = [eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 0), eng.read_output(rb, _hip.OUT_AFTER_LC)]
    emit("chain/%s/forward_around_mc" % name, lambda: [after, eng.download(rb), np.int32(all(np.array_equal(a, b) for a, b in zip(before, after)))])
    # (tests/test_gpu_model_set.py: test_set_leaves_the_handle_untouched)
    eng.forward_resident(rb, 0)
    z = eng.read_output(rb, _hip.OUT_AFTER_LC)
    eng.forward_models(rb, 1)
    ys = eng.models_download(rb)
    emit("chain/%s/set_of_3" % name, lambda: [ys, eng.download(rb), eng.read_output(rb, _hip.OUT_AFTER_LC), np.int32(np.array_equal(z, eng.read_output(rb, _hip.OUT_AFTER_LC)))])
    emit("chain/%s/set_of_3/predict" % name, lambda: [ms.predict(inputs)])
    eng.set_outputs()
    if mfma:  # member 1 of 4 on the exact-fp32 kernels: a run of one member, the single-member fallback and a run of two in one forward
        mem4 = members(cfg, 4, targets=["e_b", "homo", "e_b", "homo"] if name == "e_b" else None)
        w1 = dict(mem4[1][1])
        k = w1["local_attention_0/query/kernel"].copy()
        k[3, 5] = 300.0
        w1["local_attention_0/query/kernel"] = k
        mem4[1] = (mem4[1][0], w1)
        eng.models_load([w for _, w in mem4], relu_out=[int(c["hyper"]["target"] == "e_b") for c, _ in mem4])
        eng.forward_models(rb, 1)
        emit("chain/%s/set_of_4_one_exact" % name, lambda: [eng.models_download(rb), eng.download(rb)])
    emit("chain/%s/ablate" % name, lambda: [[eng.ablate_pooling(rb, mode) for mode in ("leave_one_out", "deletion", "insertion")]])
    emit("chain/%s/rollout" % name, lambda: [eng.attention_rollout(rb), eng.attention_rollout(rb, residual=0.3, head=1, depth=1)])
    emit("chain/%s/forward_last" % name, lambda: [eng.forward(pk)])
    rb.free()

# 9. sets on the chunk tiles (the merge kernel's set launch) and through the range-guard re-run of every member
cfg = config(L=2)
inputs, pk = big_batch(True)
ms = ModelSet(members(cfg, 3), device=0)
emit("set/big_atom", lambda: [ms.predict(inputs)])
cfg = config(L=3)
mem = members(cfg, 3)
w1 = dict(mem[1][1])
w1["after_Lc/bias"] = (w1["after_Lc/bias"] + 1.0e5).astype(np.float32)
mem[1] = (mem[1][0], w1)
ms = ModelSet(mem, device=0)
emit("set/range_rerun", lambda: [ms.predict(batch(cfg, 6, 1)[0]), np.int64(ms.engine.exact_reruns())])
print("done", flush=True)
'''
runs = []
for lib in sys.argv[1:]:
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=dict(os.environ, SCANN_HIP_LIB=os.path.abspath(lib)), capture_output=True, text=True)
    print("== %s (exit %d)\n%s%s" % (lib, r.returncode, r.stdout, r.stderr[-2000:]), flush=True)
    runs.append(dict(line.split() for line in r.stdout.splitlines() if len(line.split()) == 2) if r.returncode == 0 and "done" in r.stdout else None)
    if runs[-1] is None:
        sys.exit("a library did not finish its scenarios: nothing more is started on the GPU")
diff = sorted({k for a in runs for k in a if any(b.get(k) != a[k] for b in runs)})
print("same bytes in all %d scenarios" % len(runs[0]) if not diff else "DIFFERENT: " + ", ".join(diff))
