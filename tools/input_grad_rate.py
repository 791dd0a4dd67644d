#!/usr/bin/env python3
"""Cost of the input gradients against a training step, on the same resident QM9-shaped batch and box:
    python tools/input_grad_rate.py [batch] [key=value ...]      e.g.  g_update=False
Alternates rounds of scann_input_grads (d y / d distance and weight; synchronous by contract, outputs copied back) and
scann_train_step (Dropout 0.1, synchronous) and prints the median per-call time of each."""
import os, sys, time, ast
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), ROOT]
import bench
from scann.models.scann_model import HipModel, normalize_config
B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
over = {}
for kv in sys.argv[2:]:
    k, v = kv.split("=")
    over[k] = ast.literal_eval(v)
cfg = normalize_config({"model": dict(bench.QM9_MODEL, **over), "hyper": {"target": "homo"}})
eng = HipModel(cfg, device=0, seed=1234).engine
eng.train_begin()
rng = np.random.default_rng(0)
rb = eng.upload(bench.synth_packed_batch(rng, B))
tg = rng.normal(size=B).astype(np.float32)
for i in range(20):
    eng.input_grads(rb)
    eng.train_step(rb, tg, 5e-4, dropout=0.1, seed=i)
n, rounds = 50, 5
t_ig, t_st = [], []
for r in range(rounds):
    t0 = time.perf_counter()
    for i in range(n):
        eng.input_grads(rb)
    t_ig.append((time.perf_counter() - t0) / n)
    t0 = time.perf_counter()
    for i in range(n):
        eng.train_step(rb, tg, 5e-4, dropout=0.1, seed=100 + r * n + i)
    t_st.append((time.perf_counter() - t0) / n)
rb.free()
print("batch %d %s: input_grads %.3f ms per call, train_step %.3f ms per step (medians of %d rounds of %d)"
      % (B, over or "SCANN+", np.median(t_ig) * 1e3, np.median(t_st) * 1e3, rounds, n))
