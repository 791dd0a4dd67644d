#!/usr/bin/env python3
"""Cost of the inference outputs beyond y and the GlobalAttention scores: ``HipModel.predict_dataset`` over QM9-shaped batches of 128
(PackedDataset, groups of 8 batches, the handle's streams) with no outputs, with every layer's local-attention weights, and with the
two representations (after_Lc, bf_property).  The legs alternate over ``--reps`` rounds; each leg's time is host-clock wall time of a
whole pass (predict_dataset returns after its last download).  The same three selections once more on the device alone ("device_*"):
resident groups forwarded back to back over the handle's streams, host clock around the launches and a final synchronisation (no
download, no host-side repadding).  Prints one JSON line and writes it to ``--out``.

The extra stores are 8 heads x 4 B = 32 B per edge and layer (plus 512 B per atom for after_Lc, 512 B per structure for bf_property)
written by the kernels, and the same bytes copied to the host and repadded per structure by predict_dataset."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), ROOT]

import numpy as np  # noqa: E402

import bench  # noqa: E402  (the benchmark's QM9-shaped batches and configuration)


def qm9_dataset(n_mol, batch, seed=0):
    """bench.py's QM9-shaped molecules as a PackedDataset (CSR arrays, neighbour indices inside their structure)"""
    from scann.utils import PackedDataset

    rng = np.random.default_rng(seed)
    parts = [bench.synth_packed_batch(rng, batch) for _ in range(-(-n_mol // batch))]
    mol, eoff, atomic, local, dist, wgt = [0], [0], [], [], [], []
    for b in parts:
        first = np.repeat(b.mol_offset[:-1], np.diff(b.mol_offset))
        local.append(b.edge_col - np.repeat(first, np.diff(b.edge_offset)))
        mol.extend((b.mol_offset[1:].astype(np.int64) + mol[-1]).tolist())
        eoff.extend((b.edge_offset[1:].astype(np.int64) + eoff[-1]).tolist())
        atomic.append(b.atomic)
        dist.append(b.edge_dist)
        wgt.append(b.edge_weight)
    n = len(mol) - 1
    return PackedDataset.from_arrays(mol, np.concatenate(atomic), eoff, np.concatenate(local), np.concatenate(dist), np.concatenate(wgt),
                                     np.zeros(n, np.float32), batch_size=batch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=16384)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="none,attention,representations")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true", help="the device_* legs only (for a kernel trace)")
    args = ap.parse_args()
    from scann.models.scann_model import HipModel, normalize_config

    cfg = normalize_config({"model": dict(bench.QM9_MODEL), "hyper": {"target": "homo"}})
    L = cfg["model"]["n_attention"]
    data = qm9_dataset(args.molecules, args.batch)
    args.molecules = len(data.target)
    model = HipModel(cfg, device=0, seed=1234, infer=True)
    legs = {"none": None, "attention": ["local_attention_%d" % k for k in range(L)], "representations": ["after_Lc", "bf_property"]}
    legs = {} if args.device_only else {k: legs[k] for k in args.legs.split(",")}

    def run(names):
        t0 = time.perf_counter()
        if names is None:
            r = model.predict_dataset(data, group=args.group)
        else:
            r = model.predict_dataset(data, group=args.group, outputs=names)
        return time.perf_counter() - t0, r

    for names in legs.values():  # warm-up: code objects, the block cache, pinned staging
        run(names)
    times = {k: [] for k in legs}
    y_ref = None
    for _ in range(args.reps):
        for k, names in legs.items():
            dt, r = run(names)
            times[k].append(dt)
            y_ref = r[0] if y_ref is None else y_ref
            assert np.array_equal(r[0], y_ref), k  # the predictions do not depend on the outputs asked for
    # the device alone: four resident groups, forwards back to back
    eng = model.engine
    ns = eng.num_streams()
    rbs = [eng.upload(data.batches(g * args.group, (g + 1) * args.group)[0]) for g in range(4)]
    sels = {"device_none": ((), False, False), "device_attention": (range(L), False, False), "device_representations": ((), True, True)}

    def dev(sel, iters):
        eng.set_outputs(sel[0], after_lc=sel[1], bf_property=sel[2])
        eng.sync()
        t0 = time.perf_counter()
        for i in range(iters):
            eng.forward_resident(rbs[i % len(rbs)], i % ns)
        eng.sync()
        dt = time.perf_counter() - t0
        eng.set_outputs()
        return dt

    for sel in sels.values():
        dev(sel, 8)
    dev_iters = 400
    for k in sels:
        times[k] = []
    for _ in range(args.reps):
        for k, sel in sels.items():
            times[k].append(dev(sel, dev_iters))
    dev_mol = sum(rb.packed.n_struct for rb in rbs) * dev_iters // len(rbs)
    for rb in rbs:
        rb.free()
    n_edge = int(data.edge_offset[-1])
    res = {"molecules": args.molecules, "atoms": int(data.mol_offset[-1]), "edges": n_edge, "layers": L, "batch": args.batch,
           "group": args.group, "reps": args.reps,
           "extra_attention_bytes_written": n_edge * 8 * 4 * L}
    for k, ts in times.items():
        dev_leg = k.startswith("device_")
        base = times["device_none" if dev_leg else "none"] if ("device_none" if dev_leg else "none") in times else None
        med = float(np.median(ts))
        res[k] = {"median_s": med, "min_s": float(np.min(ts)), "max_s": float(np.max(ts)),
                  "molecules_per_s": (dev_mol if dev_leg else args.molecules) / med}
        if base:
            res[k]["vs_none"] = med / float(np.median(base))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
