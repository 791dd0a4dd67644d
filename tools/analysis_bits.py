"""Do two checkouts give the same bytes from HipModel's batched analysis calls?
    python tools/analysis_bits.py TREE_A TREE_B [...]
Each tree (its own Python package and its own lib/libscann_hip.so) runs, in a child process of its own, input_gradients,
atom_contributions, attention_rollout, nearest, predict_uncertainty and LatentIndex.add on one fixed synthetic set -- so.synth_dataset,
as a padded dict and as a PackedBatch, with a batch_size smaller than the set so that several chunks run -- and saves every key of every
returned dict; the arrays are then compared byte for byte (dtype and shape included), and a key that differs is named at the end.  Each
child also prints the wall time of one warm multi-chunk call per method (the median of three)."""
import os, subprocess, sys, tempfile
import numpy as np
CHILD = r'''
import os, sys, time
import numpy as np
ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle")]
import scann_oracle as so
from scann import _hip
from scann.models.scann_model import HipModel

N, BS = 37, 8  # five chunks, the last one short
cfg = so.default_config("qm9")
model = HipModel(cfg, so.init_weights(cfg, 1234, perturb=True), device=0, infer=True)
inputs, _ = so.pad_batch(*so.synth_dataset(N, 7), g_update=True)
pk = _hip.pack_inputs(inputs)
ref_inputs, _ = so.pad_batch(*so.synth_dataset(50, 8), g_update=True)
keys = np.arange(N) * 7919 + 1
saved = {}


def run(name, call):
    res = call()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    print("%-40s %8.2f ms" % (name, 1e3 * sorted(ts)[1]), flush=True)
    for k, v in res.items():
        saved["%s/%s" % (name, k)] = np.asarray(v)


for kind, x in (("padded", inputs), ("packed", pk)):
    run("input_gradients/" + kind, lambda: model.input_gradients(x, batch_size=BS))
    if kind == "padded":
        for mode in ("leave_one_out", "deletion", "insertion"):
            run("atom_contributions/%s/%s" % (mode, kind), lambda: model.atom_contributions(x, mode=mode, batch_size=BS))
    run("attention_rollout/" + kind, lambda: model.attention_rollout(x, batch_size=BS))
    run("attention_rollout/head1_depth2_vectors/" + kind, lambda: model.attention_rollout(x, residual=0.3, head=1, depth=2, matrix=False, batch_size=BS))
    run("predict_uncertainty/" + kind, lambda: model.predict_uncertainty(x, samples=5, seed=3, keys=keys, attention_rate=0.05, batch_size=BS,
                                                                         return_samples=True))
    for level in ("structure", "atom"):
        index = model.build_index(ref_inputs, level=level, batch_size=16)
        rows, ids, atoms = index.rows()
        saved.update({"index/%s/%s/rows" % (level, kind): rows, "index/%s/%s/ids" % (level, kind): ids, "index/%s/%s/atoms" % (level, kind): atoms})
        run("nearest/%s/%s" % (level, kind), lambda: model.nearest(x, index, k=4, batch_size=BS))
        index.add(x, ids=np.arange(N) + 1000, batch_size=BS)  # LatentIndex.add in several chunks, then the leave-one-out query
        rows, ids, atoms = index.rows()
        saved.update({"index+/%s/%s/rows" % (level, kind): rows, "index+/%s/%s/ids" % (level, kind): ids, "index+/%s/%s/atoms" % (level, kind): atoms})
        run("nearest/%s/%s/exclude" % (level, kind), lambda: model.nearest(x, index, k=4, exclude_ids=np.arange(N) + 1000, batch_size=BS))
        index.free()
np.savez(OUT, **saved)
print("done", flush=True)
'''
runs = []
with tempfile.TemporaryDirectory() as tmp:
    for i, tree in enumerate(sys.argv[1:]):
        out = os.path.join(tmp, "%d.npz" % i)
        env = {k: v for k, v in os.environ.items() if k != "SCANN_HIP_LIB"}  # (each tree's own library)
        r = subprocess.run([sys.executable, "-c", CHILD, os.path.abspath(tree), out], env=env, capture_output=True, text=True)
        print("== %s (exit %d)\n%s%s" % (tree, r.returncode, r.stdout, r.stderr[-2000:]), flush=True)
        if r.returncode != 0 or "done" not in r.stdout:
            sys.exit("a tree did not finish its calls: nothing more is started on the GPU")
        with np.load(out) as z:
            runs.append({k: z[k] for k in z.files})
same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()  # noqa: E731
diff = sorted({k for a in runs for k in a if any(k not in b or not same(a[k], b[k]) for b in runs)})
print("same bytes in all %d arrays" % len(runs[0]) if not diff else "DIFFERENT: " + ", ".join(diff))
