#!/usr/bin/env python3
"""Cost of one Monte Carlo dropout sample against one plain inference forward, on the same resident QM9-shaped batch and box:
    python tools/mc_rate.py [samples]
at two shapes: the bench's 10-batch launch group (10 x 128 structures concatenated) and one batch of 128.  Alternates rounds of
scann_predict_mc (default rates, T samples, synchronous, mean / std copied back) and of T plain forwards of the batch followed by one
download, and prints the median time per sample, per forward and their ratio."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), ROOT]
import bench
from scann import _hip
from scann.models.scann_model import HipModel, normalize_config
T = int(sys.argv[1]) if len(sys.argv) > 1 else 30
cfg = normalize_config({"model": dict(bench.QM9_MODEL), "hyper": {"target": "homo"}})
eng = HipModel(cfg, device=0, seed=1234, infer=True).engine
rng = np.random.default_rng(0)
for name, n_batch in (("10 x 128", 10), ("1 x 128", 1)):
    pk = _hip.concat_packed([bench.synth_packed_batch(rng, 128) for _ in range(n_batch)])
    rb = eng.upload(pk)
    for i in range(3):
        eng.predict_mc(rb, T, seed=i)
        for _ in range(T):
            eng.forward_resident(rb, 0)
        eng.download(rb)
    rounds = 7
    t_mc, t_fw = [], []
    for r in range(rounds):
        t0 = time.perf_counter()
        eng.predict_mc(rb, T, seed=100 + r)
        t_mc.append((time.perf_counter() - t0) / T)
        t0 = time.perf_counter()
        for _ in range(T):
            eng.forward_resident(rb, 0)
        eng.download(rb)
        t_fw.append((time.perf_counter() - t0) / T)
    rb.free()
    mc, fw = np.median(t_mc) * 1e3, np.median(t_fw) * 1e3
    print("%s structures (%d atoms, %d edges), T = %d: %.3f ms per MC sample, %.3f ms per plain forward, ratio %.2f (medians of %d rounds)"
          % (name, pk.n_atom, pk.n_edge, T, mc, fw, mc / fw, rounds))
