#!/usr/bin/env python3
"""Cost of scann_attention_rollout against the only other route to the same numbers, on one resident batch and box:
    python tools/rollout_rate.py [qm9 | mp2018 | big220 | giant:<atoms>] [--kernels | --conflicts] [out.txt]
qm9: bench.py's shape, 128 QM9-shaped molecules; mp2018: tests/size_batches.py's mp2018_b128; big220 / giant:<n>: the large structures of
tests/test_gpu_rollout.py.  Prints (and appends to out.txt) the median per-call time, host clock around synchronous calls, warm, of
  (a) scann_forward_resident + scann_batch_download,
  (b) Engine.attention_rollout(matrix=False), (c) the same with matrix=True (each includes its own forward + download),
  (d) the route without the call: the forward with every attention map selected, its download and the L scann_output_read copies (device
      part, the batch resident: no upload in it), then re-padding and tests/rollout_ref.py in fp32 on the host (host part).
--kernels: a few calls of (b), (c) and no timing, for a run of its own under `rocprofv3 --kernel-trace --stats -- python
tools/rollout_rate.py <what> --kernels`, or under `rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -- ...` (counters alone, no tracing
beside them): the measured LDS bank-conflict share is conflict cycles / active cycles of rollout_kernel.
--conflicts: no GPU; the share the lane mapping predicts from the batch's indices (csrc/scann_rollout.hip's header): a 32-lane half of a
wave reads 32 / C slab rows per gather step, and two different rows congruent modulo 64 / C meet on a bank (C = 16 only)."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
import scann_oracle as so
import size_batches
import rollout_ref
from scann import _hip
args = [a for a in sys.argv[1:] if not a.startswith("--")]
what = args[0] if args else "qm9"
out_path = args[1] if len(args) > 1 else None
kind = "mp2018" if what == "mp2018" else "qm9"
if what == "mp2018":
    data = size_batches.mp2018_b128_data()
elif what.startswith("giant:"):
    data = size_batches.giant_data(int(what.split(":")[1]))
elif what == "big220":
    import test_gpu_rollout
    data = test_gpu_rollout.big220_data()
else:
    data = so.synth_dataset(128, 5)
cfg = so.default_config(kind)
inputs = so.pad_batch(*data, g_update=True)[0]
pk = _hip.pack_inputs(inputs)
L = cfg["model"]["n_attention"]
shape = "%s: %d structures, %d atoms, %d edges, largest %d" % (what, pk.n_struct, pk.n_atom, pk.n_edge, int(np.diff(pk.mol_offset).max()))


def say(line):
    print(line)
    if out_path:
        open(out_path, "a").write(line + "\n")


def slab(max_atoms):  # csrc/scann_rollout.hip rollout_slab
    return 32 if max_atoms <= 32 else 64 if max_atoms <= 128 else 32 if max_atoms <= 512 else 16


if "--conflicts" in sys.argv:
    C = slab(int(np.diff(pk.mol_offset).max()))
    rows_per_half, steps, extra = 32 // C if C < 32 else 1, 0, 0
    for s in range(pk.n_struct):
        a0, a1 = int(pk.mol_offset[s]), int(pk.mol_offset[s + 1])
        deg = np.diff(pk.edge_offset[a0:a1 + 1])
        for i0 in range(0, a1 - a0, rows_per_half):  # the rows one half walks together, step t = their t-th edges
            rows = range(i0, min(i0 + rows_per_half, a1 - a0))
            for t in range(int(max(deg[i] for i in rows))):
                nb = sorted({int(pk.edge_col[pk.edge_offset[a0 + i] + t]) - a0 for i in rows if t < deg[i]})
                banks = [j % (64 // C) for j in nb]
                steps += 1
                extra += max(banks.count(b) for b in set(banks)) - 1
    say("%s: C = %d, %d rows per 32-lane half: %d gather steps, %d predicted extra LDS cycles = %.1f %%" % (
        shape, C, rows_per_half, steps, extra, 100.0 * extra / max(steps, 1)))
    sys.exit(0)

from scann.models.scann_model import HipModel
eng = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True).engine
rb = eng.upload(pk)


def forward():
    eng.forward_resident(rb)
    eng.download(rb)


def maps_route():
    eng.set_outputs(range(L))
    try:
        eng.forward_resident(rb)
        y, ga = eng.download(rb)
        return ga, [eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, k) for k in range(L)]
    finally:
        eng.set_outputs()


CALLS = {"a forward + download": forward, "b rollout, attribution only": lambda: eng.attention_rollout(rb, matrix=False),
         "c rollout with the matrix": lambda: eng.attention_rollout(rb, matrix=True), "d maps route, device part": maps_route}
if "--kernels" in sys.argv:
    for i in range(13):
        CALLS["b rollout, attribution only"]()
        CALLS["c rollout with the matrix"]()
    rb.free()
    sys.exit(0)
for i in range(20):
    for fn in CALLS.values():
        fn()
n, rounds = 30, 5
t = {k: [] for k in CALLS}
for r in range(rounds):  # alternating rounds: whatever else the box runs falls on all of them alike
    for k, fn in CALLS.items():
        t0 = time.perf_counter()
        for i in range(n):
            fn()
        t[k].append((time.perf_counter() - t0) / n)
ga, maps = maps_route()
rb.free()
t0 = time.perf_counter()
padded = [_hip.repad_local_attention(m, inputs["atom_mask"], inputs["neighbor_mask"]) for m in maps]
rollout_ref.rollout(inputs, padded, pk.repad_ga(ga), dtype=np.float32)
host = (time.perf_counter() - t0) * 1e3
med = {k: float(np.median(v)) * 1e3 for k, v in t.items()}
say(shape + " (medians of %d rounds of %d calls)" % (rounds, n))
for k in CALLS:
    say("  (%s) %-28s %.3f ms%s" % (k[0], k[2:], med[k], "" if k[0] in "ad" else "  (+%.3f over (a), %.2f x (d)'s device part)" % (
        med[k] - med["a forward + download"], med[k] / med["d maps route, device part"])))
say("  (d) %-28s %.1f ms (re-padding + rollout_ref in fp32, one run)" % ("maps route, host part", host))
