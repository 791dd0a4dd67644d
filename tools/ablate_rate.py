#!/usr/bin/env python3
"""Cost of scann_ablate_pooling against the unablated answer, on one resident batch and box:
    python tools/ablate_rate.py [qm9 | mp2018 | giant:<atoms>] [--kernels]
qm9: 128 QM9-shaped molecules; mp2018: tests/size_batches.py's mp2018_b128; giant:<n>: one structure of n atoms between two molecules.
Prints the median per-call time of (a) scann_forward_resident + scann_batch_download and (b) scann_ablate_pooling per mode (host clock
around synchronous calls, warm).  --kernels: a few calls of each and no timing, for a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/ablate_rate.py <what> --kernels`: ablate_kernel beside readout_kernel in one trace."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
import scann_oracle as so
import size_batches
from scann import _hip
from scann.models.scann_model import HipModel
args = [a for a in sys.argv[1:] if not a.startswith("--")]
what = args[0] if args else "qm9"
kind = "mp2018" if what == "mp2018" else "qm9"
data = size_batches.mp2018_b128_data() if what == "mp2018" else size_batches.giant_data(int(what.split(":")[1])) if what.startswith("giant:") \
    else so.synth_dataset(128, 5)
cfg = so.default_config(kind)
pk = _hip.pack_inputs(so.pad_batch(*data, g_update=True)[0])
eng = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True).engine
rb = eng.upload(pk)
MODES = ("leave_one_out", "deletion", "insertion")


def forward():
    eng.forward_resident(rb)
    eng.download(rb)


if "--kernels" in sys.argv:
    for i in range(13):
        forward()
        for m in MODES:
            eng.ablate_pooling(rb, m)
    rb.free()
    sys.exit(0)
for i in range(20):
    forward()
    for m in MODES:
        eng.ablate_pooling(rb, m)
n, rounds = 30, 5
t = {k: [] for k in ("forward",) + MODES}
for r in range(rounds):  # alternating rounds: whatever else the box runs falls on all of them alike
    for k in t:
        fn = forward if k == "forward" else (lambda k=k: eng.ablate_pooling(rb, k))
        t0 = time.perf_counter()
        for i in range(n):
            fn()
        t[k].append((time.perf_counter() - t0) / n)
rb.free()
med = {k: float(np.median(v)) * 1e3 for k, v in t.items()}
print("%s: %d structures, %d atoms, largest %d: forward + download %.3f ms; ablate_pooling %s (medians of %d rounds of %d calls; each "
      "includes its own forward + download)" % (what, pk.n_struct, pk.n_atom, int(np.diff(pk.mol_offset).max()), med["forward"],
                                                ", ".join("%s %.3f ms (+%.3f)" % (m, med[m], med[m] - med["forward"]) for m in MODES), rounds, n))
