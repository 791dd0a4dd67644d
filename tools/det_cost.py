#!/usr/bin/env python3
"""Cost of the deterministic training mode (scann_set_deterministic): the training step of bench.py's QM9 configuration (7 layers,
dropout 0.1, two steps in flight as trainer.fit runs them) on resident QM9-shaped batches of 16, 128 and 1024, with the mode off and
on.  One handle per batch size; the two modes alternate run by run (--reps rounds of off, on), each run `--steps` steps timed by the
host clock from the first begin to the last end.  Prints the median ms per step of each mode and the added fraction, as one JSON line
(also written to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), ROOT]

import numpy as np  # noqa: E402

import bench  # noqa: E402  (the benchmark's QM9-shaped batches and configuration)


def run_steps(eng, pool, targets, n, i0):
    inflight = 0
    t0 = time.perf_counter()
    for i in range(i0, i0 + n):
        eng.train_step_begin(pool[i % len(pool)], targets[i % len(pool)], 5e-4 / (1.0 + 1e-5 * i), dropout=0.1, seed=i)
        inflight += 1
        if inflight == 2:
            eng.train_step_end()
            inflight -= 1
    while inflight:
        eng.train_step_end()
        inflight -= 1
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", default="16,128,1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100, help="steps per timed run (a quarter of it at batch 1024)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from scann.models.scann_model import HipModel, normalize_config

    res = {}
    for bs in [int(b) for b in args.batches.split(",")]:
        cfg = normalize_config({"model": dict(bench.QM9_MODEL), "hyper": {"target": "homo", "batch_size": bs}})
        eng = HipModel(cfg, device=0, seed=1234).engine
        eng.train_begin()
        rng = np.random.default_rng(7)
        pool = [eng.upload(bench.synth_packed_batch(rng, bs)) for _ in range(4)]
        targets = [rng.normal(size=bs).astype(np.float32) * 0.1 for _ in pool]
        steps = max(8, args.steps // 4) if bs >= 1024 else args.steps
        times = {"off": [], "on": []}
        i = 0
        for mode in ("off", "on"):  # warm both modes (the deterministic slots are allocated on a batch's first such backward)
            eng.set_deterministic(mode == "on")
            run_steps(eng, pool, targets, 10, i)
            i += 10
        for _ in range(args.reps):
            for mode in ("off", "on"):
                eng.set_deterministic(mode == "on")
                times[mode].append(run_steps(eng, pool, targets, steps, i))
                i += steps
        off, on = float(np.median(times["off"])), float(np.median(times["on"]))
        res[str(bs)] = {"ms_off": off, "ms_on": on, "added": on / off - 1.0, "runs_off": times["off"], "runs_on": times["on"]}
        for rb in pool:
            rb.free()
        eng.close()
    line = json.dumps({"what": "training step, deterministic mode off vs on (QM9, 7 layers, two steps in flight)", "batches": res})
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
