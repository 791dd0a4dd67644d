#!/usr/bin/env python3
"""Cost of fitting a classification head on a latent index on the device against the route without it, on one box:
    python tools/logit_rate.py [--tenth] [--host-fit] [--kernels N C M | --summary TRACE.csv N C M] [out.txt]
An index of N = 2,400,000 seeded rows of 128 columns (--tenth: 240,000), labels from a noisy linear score.  Prints (and appends to
out.txt), host clock around synchronous calls, warm, three runs each, min / median:
  (a) one pass (Engine.index_logit_pass: labels and weights uploaded, kernels, sums downloaded, one wait) at C = 2 with M = 5 and with
      M = 30, and at C = 16 with M = 5; the last with the probabilities copied back as well;
  (b) LatentIndex.fit_class_head end to end (C = 2, the default grid and 4 folds), its iterations and passes;
  (c) the route a user has without the call: LatentIndex.rows() (the download), one pass of _hip.logit_pass_host (C = 2, M = 5 and M = 30),
      and a plain NumPy softmax gradient in fp32 (one model, C = 2) for scale; with --host-fit (or --tenth) the same optimiser on
      _hip.logit_pass_host end to end, otherwise its passes times the time of one host pass of its models.
--kernels N C M: four passes at that size and no timing, for a run of its own under `rocprofv3 --kernel-trace --output-format csv -d DIR --
python tools/logit_rate.py --kernels N C M`.  --summary TRACE.csv N C M [out.txt] (no GPU) reads that run's *_kernel_trace.csv and prints
per kernel the launches of one pass and their time summed, min / median over the three calls behind the first, with logit_pass_kernel's
2 N dim M C fp32 and 2 N (dim + 1) M C fp64 flops per second."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
argv = sys.argv[1:]
TAKES = {"--kernels": 3, "--summary": 4}
opt, args, i = {}, [], 0
while i < len(argv):
    if argv[i] in TAKES:
        opt[argv[i]] = argv[i + 1:i + 1 + TAKES[argv[i]]]
        i += 1 + TAKES[argv[i]]
    else:
        if not argv[i].startswith("--"):
            args.append(argv[i])
        i += 1
out_path = args[0] if args else None
tenth = "--tenth" in argv
N_ROWS = 240000 if tenth else 2400000
D = 128


def say(line):
    print(line, flush=True)
    if out_path:
        open(out_path, "a").write(line + "\n")


def timed(f, runs=3):
    t = []
    for r in range(runs):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return min(t), float(np.median(t))


def summary(path, N, C, M):
    """per-call kernel times from a kernel trace of `--kernels N C M`: the launches of every logit_* kernel in time order, cut into the
    run's four calls (the first is the warm-up and is left out)"""
    import csv, re
    runs = {}
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        k = re.search(r"logit_\w+_kernel", r["Kernel_Name"])
        if k:
            runs.setdefault(k.group(0), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    calls = 4
    say("kernels of Engine.index_logit_pass, N = %d x %d, C = %d, M = %d (rocprofv3 --kernel-trace; per call: launches, us summed over them, "
        "min / median of %d calls):" % (N, D, C, M, calls - 1))
    total = 0.0
    for k in sorted(runs):
        t = runs[k]
        if len(t) % calls:
            say("  %-24s %d launches do not make %d calls" % (k, len(t), calls))
            continue
        per = len(t) // calls
        sums = sorted(sum(t[c * per:(c + 1) * per]) for c in range(1, calls))
        total += sums[0]
        note = ""
        if k == "logit_pass_kernel":
            f32, f64 = 2.0 * N * D * M * C, 2.0 * N * (D + 1) * M * C
            note = "   %.3g fp32 + %.3g fp64 flops: %.2f + %.2f Tflop/s" % (f32, f64, f32 / (sums[0] * 1e-6) / 1e12, f64 / (sums[0] * 1e-6) / 1e12)
        say("  %-24s %3d x %10.1f / %10.1f%s" % (k, per, sums[0], float(np.median(sums)), note))
    say("  %-24s       %10.1f   (the kernels' minima together)" % ("all of them", total))


if "--summary" in opt:
    summary(opt["--summary"][0], *[int(x) for x in opt["--summary"][1:]])
    sys.exit(0)

import scann_oracle as so
from scann import _hip
from scann.models import LatentIndex
from scann.models import latent_index as li
from scann.models.scann_model import HipModel

cfg = so.default_config("qm9")
model = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True)
eng = model.engine


def make(N, C):
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((N, D), dtype=np.float32) * rng.uniform(0.05, 4, D).astype(np.float32) + rng.standard_normal(D).astype(np.float32)
    score = rows @ (rng.standard_normal(D).astype(np.float32) / np.float32(np.sqrt(D))) + np.float32(1.0) * rng.standard_normal(N, dtype=np.float32)
    lab = np.searchsorted(np.quantile(score, np.arange(1, C) / C), score).astype(np.int32)
    lat = LatentIndex(model, "atom")
    for i in range(0, N, 1 << 18):
        lat.add_rows(rows[i:i + (1 << 18)])
    return lat, lab


def weights_for(C, M, seed=1):
    return (np.random.default_rng(seed).standard_normal((M, C, D + 1)) * 0.05).astype(np.float32)


def folds_for(M, F=4):
    return (np.arange(M) % (F + 1) - 1).astype(np.int32)


if "--kernels" in opt:
    N, C, M = (int(x) for x in opt["--kernels"])
    lat, lab = make(N, C)
    mean = eng.index_moments(lat._ix)["mean"]
    for i in range(4):
        eng.index_logit_pass(lat._ix, lab, mean, weights_for(C, M), folds_for(M), 4)
    lat.free()
    sys.exit(0)

lat, lab2 = make(N_ROWS, 2)
ix = lat._ix
mean = eng.index_moments(ix)["mean"]
say("classification head over N = %d rows x %d columns" % (N_ROWS, D))
lab16 = (np.arange(N_ROWS) % 16).astype(np.int32)
for C, M, lab in ((2, 5, lab2), (2, 30, lab2), (16, 5, lab16)):
    U, fold = weights_for(C, M), folds_for(M)
    eng.index_logit_pass(ix, lab, mean, U, fold, 4)  # warm: the workspace is in the block cache
    ta = timed(lambda: eng.index_logit_pass(ix, lab, mean, U, fold, 4))
    f32, f64 = 2.0 * N_ROWS * D * M * C, 2.0 * N_ROWS * (D + 1) * M * C
    say("(a) scann_index_logit_pass, C = %2d, M = %2d (%3d logit columns, %d launch(es)): %9.2f / %9.2f ms (min / median of 3); %.3g fp32 + %.3g fp64 "
        "flops are %.2f + %.2f Tflop/s if all of the call were the kernel" % (C, M, C * M, -(-M // (64 // C)), ta[0] * 1e3, ta[1] * 1e3, f32, f64,
                                                                             f32 / ta[0] / 1e12, f64 / ta[0] / 1e12))
pof = np.array([1, 2, 3, 4], np.int32)
tp = timed(lambda: eng.index_logit_pass(ix, lab16, mean, weights_for(16, 5), folds_for(5), 4, pof))
say("    the same at C = 16, M = 5 with the probabilities [N, 16] copied back: %9.2f / %9.2f ms" % (tp[0] * 1e3, tp[1] * 1e3))
res, head = lat.fit_class_head(lab2)
tb = timed(lambda: lat.fit_class_head(lab2))
say("(b) LatentIndex.fit_class_head end to end, C = 2, %d strengths x (4 folds + 1): %9.2f / %9.2f ms; %d iterations, %d passes, %s; l2 %.4g, "
    "cv_accuracy %.4f, cv_brier %.4f" % (len(res["path"]["l2"]), tb[0] * 1e3, tb[1] * 1e3, res["iterations"], res["passes"], res["stopped"], res["l2"],
                                         res["cv_accuracy"], res["cv_brier"]))
t0 = time.perf_counter()
rows = lat.rows()[0]
t_down = time.perf_counter() - t0
say("(c) without the call: rows() download %8.1f ms; OMP_NUM_THREADS %s" % (t_down * 1e3, os.environ.get("OMP_NUM_THREADS", "unset")))
host_pass = {}
for M in (5, 30):
    U, fold = weights_for(2, M), folds_for(M)
    th = timed(lambda: _hip.logit_pass_host(rows, lab2, mean, U, fold, 4), runs=1 if N_ROWS > 1000000 else 3)
    host_pass[M] = th[0]
    say("    one pass of _hip.logit_pass_host, C = 2, M = %2d: %9.1f ms" % (M, th[0] * 1e3))


def numpy_gradient():
    w = weights_for(2, 1)[0]
    a = (rows - mean) @ w[:, :D].T + w[:, D]
    a -= a.max(axis=1, keepdims=True)
    p = np.exp(a)
    p /= p.sum(axis=1, keepdims=True)
    p[np.arange(len(rows)), lab2] -= 1
    return p.T @ (rows - mean)


tn = timed(numpy_gradient, runs=2)
say("    a plain NumPy softmax gradient in fp32, one model, C = 2: %9.1f ms (min of 2)" % (tn[0] * 1e3))
if tenth or "--host-fit" in argv:
    mo = _hip.moments_host(rows)

    def host_fit():
        run = lambda w, f, q=None: _hip.logit_pass_host(rows, lab2, mo["mean"], w, f, 4, q)  # noqa: E731
        return li.class_head_fit(run, mo, lab2, 2, None, 4, 100, 1e-4)

    t0 = time.perf_counter()
    fit = host_fit()
    say("    the same optimiser on _hip.logit_pass_host end to end: %9.1f ms (%d passes) + the download" % ((time.perf_counter() - t0) * 1e3, fit["passes"]))
else:
    say("    the same optimiser on _hip.logit_pass_host: %d passes of up to 30 models, at the time of one host pass with M = 30 about %.0f s "
        "(an upper estimate: models leave as they converge; --host-fit runs it)" % (res["passes"], res["passes"] * host_pass[30]))
lat.free()
