#!/usr/bin/env python3
"""Exactness of the attention rollout on the GPU, per fixture of tests/test_gpu_rollout.py:
    python tools/rollout_parity.py [out.txt]
Kernel arithmetic: the largest relative error of the rollout against tests/rollout_ref.py in fp64 on the GPU's own maps, beside the
derived bound 2 * depth * (H + N_max + 4) * 2^-24.  End to end: rel_err of the GPU's rollout and attribution against the fp64 oracle's,
beside the fp32 oracle's own (the bound is max(1e-4, 2 x the latter))."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
import rollout_ref
import scann_oracle as so
import size_batches
import test_gpu_rollout as t
lines = ["kernel arithmetic (GPU's own maps)   max relative error   bound"]
cases = dict(t.KERNEL_CASES)
cases["giant960"] = (dict(L=2, data=size_batches.giant_data(960)), dict())
for case, (mk, kw) in cases.items():
    cfg, w, inputs, model = t.setup(**mk)
    e, b = t.check_kernel(model.attention_rollout(inputs, **kw), cfg, inputs, t.gpu_maps(model, cfg, inputs), case, **kw)
    lines.append("%-36s %-20.3e %.3e" % (case, e, b))
lines.append("end to end against the fp64 oracle   rel_err(gpu, fp64)   rel_err(fp32 oracle, fp64)")
for kind in ("qm9", "mp2018"):
    cfg, w, inputs, model = t.setup(kind=kind, n=16, seed=1, isolate=True)
    got = model.attention_rollout(inputs)
    ref = {}
    for dt in (np.float64, np.float32):
        inter = {}
        _, ga = so.forward(cfg, w, inputs, dt, intermediates=inter)
        ref[dt] = rollout_ref.rollout(inputs, [inter["attn_local_%d" % (k + 1)] for k in range(cfg["model"]["n_attention"])], ga, dtype=dt)
    amask, _ = rollout_ref.masks(inputs)
    for name, i, sel in (("rollout", 0, slice(None)), ("atom_attribution", 1, amask)):
        lines.append("%-36s %-20.3e %.3e" % (kind + " " + name, t.rel_err(got[name][sel], ref[np.float64][i][sel]),
                                              t.rel_err(ref[np.float32][i][sel], ref[np.float64][i][sel])))
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
