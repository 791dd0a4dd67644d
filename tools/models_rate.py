#!/usr/bin/env python3
"""K models of one architecture over one resident QM9-shaped batch, three ways (K = 5 by default):
    python tools/models_rate.py [K]
(a) K single-model forwards back to back on one handle, (b) K handles, one stream each, their forwards enqueued before any download,
(c) the model set: one scann_forward_models + scann_models_download.  At one batch of 128 structures and at the bench's 10-batch launch
group; prints the median WALL time per call on the host (all K predictions: launches, the synchronising download and its copy) over
alternating rounds -- not device time alone."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), ROOT]
import bench
from scann import _hip
from scann.models.scann_model import HipModel, keras_default_init, normalize_config
K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
cfg = normalize_config({"model": dict(bench.QM9_MODEL), "hyper": {"target": "homo"}})
models = [HipModel(cfg, device=0, seed=1234 + m, infer=True) for m in range(K)]
one = models[0].engine
one.models_load([m.get_weights() for m in models])
rng = np.random.default_rng(0)
for name, n_batch in (("1 x 128", 1), ("10 x 128", 10)):
    pk = _hip.concat_packed([bench.synth_packed_batch(rng, 128) for _ in range(n_batch)])
    rbs = [m.engine.upload(pk) for m in models]
    rb = rbs[0]

    def a():
        for _ in range(K):
            one.forward_resident(rb, 0)
        one.download(rb)

    def b():
        for m, r in zip(models, rbs):
            m.engine.forward_resident(r, 0)
        for m, r in zip(models, rbs):
            m.engine.download(r)

    def c():
        one.forward_models(rb, 0)
        one.models_download(rb)

    ways = (("a", a), ("b", b), ("c", c))
    for _, f in ways:
        for _ in range(5):
            f()
    t = {k: [] for k, _ in ways}
    for _ in range(21):
        for k, f in ways:
            t0 = time.perf_counter()
            f()
            t[k].append(time.perf_counter() - t0)
    for r in rbs:
        r.free()
    med = {k: np.median(v) * 1e6 for k, v in t.items()}
    print("%s structures (%d atoms, %d edges), K = %d: (a) %d forwards on one handle %.0f us, (b) %d handles one stream each %.0f us, "
          "(c) model set %.0f us wall time per call (medians of 21 rounds); (c) / (a) = %.2f, (c) / (b) = %.2f"
          % (name, pk.n_atom, pk.n_edge, K, K, med["a"], K, med["b"], med["c"], med["c"] / med["a"], med["c"] / med["b"]))
