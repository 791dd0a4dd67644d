#!/usr/bin/env python3
"""What a fine-tuning step costs by where the floor lies, and that a step with no scale set costs what it did, on one box:
    python tools/finetune_rate.py [--rounds R] [--steps K] [--parent LIB] [out.txt]
The QM9-shaped batch of 128 molecules at L = 7 that `bench.py --train` uses (eight resident batches, dropout 0.1, scann_train_step with
two steps in flight), host clock around drained runs of K steps in ONE process, the modes alternated R times so that whatever else the
box runs falls on all alike; medians, with the spread (min .. max) of the rounds:
  floor L + 2 (head only), L + 1 (after_Lc, GlobalAttention and the head), L (the top layer up), (L + 1) / 2, 0 with the embedding frozen
  ... then all trainable with a scale of all ones (the scaled optimiser kernel), then with no scale set (the unscaled kernel).
--parent LIB (a library built from the parent commit, relative to scann--material_amd/lib/): the no-scale step of that library and of
this one in fresh processes, alternated R times as tools/ab5.sh alternates builds: the claim is that this library's median lies within
the spread of the parent's rounds."""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), ROOT]


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ROUNDS, STEPS, PARENT, LEG = opt("--rounds", 5), opt("--steps", 200), opt("--parent", ""), opt("--leg", "")
flags = {"--rounds", "--steps", "--parent", "--leg"}
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in flags]
out_path = args[0] if args else None
L, BATCH = 7, 128


def say(line):
    print(line, flush=True)
    if out_path:
        open(out_path, "a").write(line + "\n")


def setup():
    import bench
    import scann_oracle as so
    from scann import _hip
    from scann.models.scann_model import HipModel

    if LEG:  # a library of the parent commit lacks the entry points of this feature: bind what it has
        lib = ctypes.CDLL(_hip.LIB_PATH)
        _hip.SYMBOLS = [s for s in _hip.SYMBOLS if hasattr(lib, s[0])]
    cfg = so.default_config("qm9")
    cfg["model"]["n_attention"] = L
    w = so.init_weights(cfg, 1234)
    eng = HipModel(cfg, w, device=0).engine
    eng.train_begin()
    rng = np.random.default_rng(2000)
    pool = [eng.upload(bench.synth_packed_batch(rng, BATCH)) for _ in range(8)]
    targets = [rng.normal(size=BATCH).astype(np.float32) for _ in pool]
    return eng, w, pool, targets


def run_steps(eng, pool, targets, n, first=0):
    """n steps, two in flight as trainer.fit runs them, drained -> seconds"""
    eng.sync()
    t0 = time.perf_counter()
    inflight = 0
    for i in range(first, first + n):
        eng.train_step_begin(pool[i % 8], targets[i % 8], 5e-4 / (1.0 + 1e-5 * i), dropout=0.1, seed=i)
        inflight += 1
        if inflight == 2:
            eng.train_step_end()
            inflight -= 1
    while inflight:
        eng.train_step_end()
        inflight -= 1
    eng.sync()
    return time.perf_counter() - t0


def stats(ms):
    return "%7.3f ms per step (%.3f .. %.3f over %d rounds)" % (float(np.median(ms)), min(ms), max(ms), len(ms))


def leg():
    """one process, the no-scale step: prints the milliseconds per step of one drained run"""
    eng, _, pool, targets = setup()
    run_steps(eng, pool, targets, 20)
    print(json.dumps({"ms": run_steps(eng, pool, targets, STEPS, 20) / STEPS * 1e3}), flush=True)


def main():
    eng, w, pool, targets = setup()

    def floor_scale(f, also_frozen=()):
        return {n: 0.0 if eng.tensor_stage(n) < f or n.startswith(tuple(also_frozen)) else 1.0 for n in w}

    modes = [("floor L + 2 = %d (head only)" % (L + 2), floor_scale(L + 2)),
             ("floor L + 1 = %d (after_Lc, GlobalAttention, head)" % (L + 1), floor_scale(L + 1)),
             ("floor L = %d (top layer up)" % L, floor_scale(L)),
             ("floor (L + 1) / 2 = %d" % ((L + 1) // 2), floor_scale((L + 1) // 2)),
             ("floor 0, embedding table frozen", floor_scale(0, ("embed_atom/",))),
             ("all trainable, scale of all ones", {n: 1.0 for n in w}),
             ("all trainable, no scale set", None)]
    times = {name: [] for name, _ in modes}
    stages = {}
    run_steps(eng, pool, targets, 20)
    it = 20
    for _ in range(ROUNDS):
        for name, scale in modes:
            eng.set_lr_scale(scale)
            run_steps(eng, pool, targets, 10, it)  # the mode's own warm-up
            times[name].append(run_steps(eng, pool, targets, STEPS, it + 10) / STEPS * 1e3)
            stages[name] = eng.train_stages()
            it += STEPS + 10
    say("fine-tuning step, QM9-shaped batch of %d at L = %d, %d steps per run, two in flight, %d alternated rounds" % (BATCH, L, STEPS, ROUNDS))
    for name, _ in modes:
        say("  %-52s %s   stages run: %s" % (name, stats(times[name]), ",".join(map(str, stages[name]))))
    if PARENT:
        libs = {"parent": os.path.join(ROOT, "scann--material_amd", "lib", PARENT), "this": ""}
        ms = {k: [] for k in libs}
        for _ in range(ROUNDS):
            for k, path in libs.items():
                env = dict(os.environ, **({"SCANN_HIP_LIB": path} if path else {}))
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", k, "--steps", str(STEPS)], env=env, capture_output=True,
                                   text=True, timeout=300)
                if r.returncode != 0:
                    raise SystemExit("leg %s failed: %s" % (k, r.stderr[-2000:]))
                ms[k].append(json.loads(r.stdout.strip().splitlines()[-1])["ms"])
        say("no scale set, fresh processes alternated (%s against this build):" % PARENT)
        for k in libs:
            say("  %-52s %s" % (k, stats(ms[k])))
        inside = min(ms["parent"]) <= float(np.median(ms["this"])) <= max(ms["parent"])
        say("  this build's median lies %s the parent's spread" % ("within" if inside else "OUTSIDE"))


if __name__ == "__main__":
    leg() if LEG else main()
