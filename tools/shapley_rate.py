#!/usr/bin/env python3
"""Cost of scann_shapley on one box, against the host route measured in the same run:
    python tools/shapley_rate.py [out.txt]
128 QM9-shaped molecules at 64 and 256 walks per structure and tests/size_batches.py's mp2018_b128 at 64.  Per configuration: the median
time of the whole call (host clock around the synchronous call, warm; it includes its forward and downloads), of the pair kernel, the walk
kernel and the reduction between events (scann_shapley_profile), the walk kernel's achieved FLOP/s -- per structure and walk 2 n^2 d for
rep = A K plus n heads of 2 d dout -- and the host route: the after_Lc rows downloaded (model.predict(outputs=["after_Lc"])), then
tests/shapley_ref.py's fp32 path (prefix values through the NumPy oracle, the fp64 reduction) on the same walks, timed once; for
mp2018_b128 on every 8th structure only, scaled by the structures' share of sum n^2 (marked ~)."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
import scann_oracle as so
import shapley_ref as sr
import size_batches
from scann import _hip
from scann.models.scann_model import HipModel

lines = ["scann_shapley on one MI355X, warm (tools/shapley_rate.py): medians of 5 rounds of 10 calls; kernels between events; host route timed once in the same run",
         "what                          P    call ms   pair ms   walk ms  reduce ms  walk TFLOP/s   host route s   host / call"]
for what, kind, data, Ps, every in (("qm9 (128 molecules)", "qm9", so.synth_dataset(128, 5), (64, 256), 1),
                                    ("mp2018_b128", "mp2018", size_batches.mp2018_b128_data(), (64,), 8)):
    cfg = so.default_config(kind)
    w = so.init_weights(cfg, 3, perturb=True)
    pk = _hip.pack_inputs(so.pad_batch(*data, g_update=True)[0])
    model = HipModel(cfg, w, device=0, infer=True)
    eng = model.engine
    rb = eng.upload(pk)
    keys = np.arange(pk.n_struct)
    n = np.diff(pk.mol_offset).astype(np.float64)
    d, dout = cfg["model"]["global_dim"], cfg["model"]["dense_out"]
    for P in Ps:
        for i in range(3):
            got = eng.shapley(rb, P, seed=1, keys=keys, want_values=True)
        call = []
        for r in range(5):
            t0 = time.perf_counter()
            for i in range(10):
                eng.shapley(rb, P, seed=1, keys=keys)
            call.append((time.perf_counter() - t0) / 10)
        ms = np.median(np.array([eng.shapley_profile(rb, P, seed=1, keys=keys) for i in range(11)]), axis=0)
        flop = P * float(np.sum(2 * n * n * d + n * (2 * d * dout + 2 * dout)))
        sel = np.arange(0, pk.n_struct, every)
        t0 = time.perf_counter()
        z = model.predict(pk, outputs=["after_Lc"])[0]
        rows = np.concatenate([np.arange(pk.mol_offset[s], pk.mol_offset[s + 1]) for s in sel])
        mol = np.concatenate([[0], np.cumsum(n[sel])]).astype(np.int64)
        perms = got["perms"][:, rows]
        v32 = np.concatenate([sr.prefix_values(cfg, w, z[rows], mol, perms[p0:p0 + 8], np.float32)[0] for p0 in range(0, P, 8)])
        sr.reduce(v32, perms, mol, sr.prefix_values(cfg, w, z[rows], mol, perms[:1], np.float32)[1])
        host = (time.perf_counter() - t0) * float(np.sum(n * n) / np.sum(n[sel] * n[sel]))
        c = float(np.median(call))
        lines.append("%-28s %4d  %8.3f  %8.3f  %8.3f  %9.3f  %12.2f  %12s%.2f  %12.0f" % (
            what, P, c * 1e3, ms[0], ms[1], ms[2], flop / (ms[1] * 1e-3) / 1e12, "~" if every > 1 else "", host, host / c))
        print(lines[-1], flush=True)
    lines.append("  (%s: %d structures, %d atoms, largest %d)" % (what, pk.n_struct, pk.n_atom, int(n.max())))
    rb.free()
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
