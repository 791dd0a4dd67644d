#!/usr/bin/env python3
"""Cost of fitting a readout head on a latent index on the device against the route without it, on one box:
    python tools/head_rate.py [--tenth] [--kernels N K | --summary TRACE.csv N K M L] [out.txt]
Index sizes N = 133,650 and 2,400,000 seeded rows of 128 columns (--tenth: 13,365 and 240,000), targets K = 1 and K = 12 linear in the rows
plus noise, the default grid.  Prints (and appends to out.txt), host clock around synchronous calls, warm, three runs each, min / median:
  (a) scann_index_fit_moments (Engine.index_fit_moments): eligibility, the augmented mean, the integer scatter with its cross block;
  (b) the eigen-decomposition of the X-X block and the closed form on the host;
  (c) scann_index_ridge_loo (Engine.index_ridge_loo) without and with the residuals copied back;
  (d) LatentIndex.fit_head end to end;
  (e) the route a user has without the calls: LatentIndex.rows() (the download), np.cov in fp64, numpy.linalg.eigh and the same closed
      form of the leave-one-out residuals in NumPy fp64, each part on its own line.
--kernels N K: four calls of fit_head at that size and no timing, for a run of its own under `rocprofv3 --kernel-trace --output-format
csv -d DIR -- python tools/head_rate.py --kernels N K`; it prints the components m and the strengths L of its fits.  --summary TRACE.csv N K
M L [out.txt] (no GPU) reads that run's
*_kernel_trace.csv and prints per kernel the launches of one fit_head and their time summed, min / median over the three calls behind
the first, with head_loo_kernel's 2 N m L (K + 1) flops per second beside pca_project_kernel's 2 N m dim of the same run."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
argv = sys.argv[1:]
TAKES = {"--kernels": 2, "--summary": 5}
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
SIZES = (13365, 240000) if tenth else (133650, 2400000)
D = 128
L_DEFAULT = 17


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


def summary(path, N, K, M, L):
    """per-call kernel times from a kernel trace of `--kernels N K`: the launches of every head_* / pca_* kernel in time order, cut into
    the run's four calls (the first is the warm-up and is left out)"""
    import csv, re
    runs = {}
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        k = re.search(r"(head|pca)_\w+_kernel(<\d>)?", r["Kernel_Name"])
        if k:
            runs.setdefault(k.group(0), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    calls = 4
    say("kernels of LatentIndex.fit_head, N = %d x %d, K = %d, default grid (rocprofv3 --kernel-trace; per call: launches, us summed over "
        "them, min / median of %d calls; m = %d components, L = %d strengths):" % (N, D, K, calls - 1, M, L))
    total = 0.0
    for k in sorted(runs):
        t = runs[k]
        if len(t) % calls:
            say("  %-28s %d launches do not make %d calls" % (k, len(t), calls))
            continue
        per = len(t) // calls
        sums = sorted(sum(t[c * per:(c + 1) * per]) for c in range(1, calls))
        total += sums[0]
        note = ""
        if k == "head_loo_kernel":  # two passes of a fit_head
            flops = 2.0 * 2 * N * M * L * (K + 1)
            note = "   2 passes x 2 N m L (K + 1) = %.3g flops: %.2f Tflop/s" % (flops, flops / (sums[0] * 1e-6) / 1e12)
        if k == "pca_project_kernel":
            flops = 2.0 * 2 * N * M * D
            note = "   2 passes x 2 N m dim = %.3g flops: %.2f Tflop/s" % (flops, flops / (sums[0] * 1e-6) / 1e12)
        say("  %-28s %3d x %10.1f / %10.1f%s" % (k, per, sums[0], float(np.median(sums)), note))
    say("  %-28s       %10.1f   (the kernels' minima together)" % ("all of them", total))


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


def make(N, K):
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((N, D), dtype=np.float32) * rng.uniform(0.05, 4, D).astype(np.float32) + rng.standard_normal(D).astype(np.float32)
    w = rng.standard_normal((D, K)).astype(np.float32) / np.float32(np.sqrt(D))
    t = (rows @ w + np.float32(0.5) * rng.standard_normal((N, K), dtype=np.float32)).astype(np.float32)
    lat = LatentIndex(model, "atom")
    for i in range(0, N, 1 << 18):
        lat.add_rows(rows[i:i + (1 << 18)])
    return lat, t


if "--kernels" in opt:
    lat, t = make(int(opt["--kernels"][0]), int(opt["--kernels"][1]))
    for i in range(4):
        res, head = lat.fit_head(t)
    print("m=%d L=%d" % (head.components.shape[0], len(res["path"]["l2"])))
    lat.free()
    sys.exit(0)


def host_route(lat, t, grid):
    """rows downloaded, np.cov, eigh and the closed form of the leave-one-out residuals at every strength of the grid, fp64"""
    t0 = time.perf_counter()
    r = lat.rows()[0]
    t1 = time.perf_counter()
    n = len(r)
    aug = np.concatenate([r, t], axis=1)
    mean = aug.mean(axis=0, dtype=np.float64)
    cov = np.cov(aug, rowvar=False, dtype=np.float64)
    t2 = time.perf_counter()
    s, U = np.linalg.eigh(cov[:D, :D])
    s, U = s[::-1], U[:, ::-1]
    t3 = time.perf_counter()
    z = (r - mean[:D].astype(np.float32)) @ U.astype(np.float32)  # [N, D] fp32, as a user would
    g = U.T @ cov[:D, D:]
    tc = t - mean[D:].astype(np.float32)
    sse = np.zeros((len(grid), t.shape[1]))
    z2 = z * z
    for l, lam in enumerate(grid):
        lev = 1.0 / n + z2 @ (1.0 / ((n - 1) * (s + lam))).astype(np.float32)
        e = tc - z @ (g / (s + lam)[:, None]).astype(np.float32)
        q = e / (1.0 - lev)[:, None]
        sse[l] = np.einsum("nk,nk->k", q, q, dtype=np.float64)
    t4 = time.perf_counter()
    return (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0), sse


for N in SIZES:
    for K in (1, 12):
        lat, t = make(N, K)
        ix = lat._ix
        mo = eng.index_fit_moments(ix, t)  # warm: the workspace is in the block cache
        say("readout head over N = %d rows x %d columns, K = %d targets; b = %d bits" % (N, D, K, mo["bits"]))
        ta = timed(lambda: eng.index_fit_moments(ix, t))
        say("(a) scann_index_fit_moments: %9.2f / %9.2f ms (min / median of 3)" % (ta[0] * 1e3, ta[1] * 1e3))
        tb = timed(lambda: li.head_closed_form(mo, D))
        fit = li.head_closed_form(mo, D)
        m, L = fit["m"], len(fit["l2"])
        say("(b) sym_eig and the closed form on the host, m = %d components, L = %d strengths: %9.2f / %9.2f ms" % (m, L, tb[0] * 1e3, tb[1] * 1e3))
        a = (ix, t, fit["mean"], fit["tmean"], fit["components"], fit["scale"], fit["coef"], fit["lev0"])
        first = eng.index_ridge_loo(*a)
        tc = timed(lambda: eng.index_ridge_loo(*a))
        pick = li.head_pick(first["sse"], fit["l2"])
        tr = timed(lambda: eng.index_ridge_loo(*a, pick))
        flops = 2.0 * N * m * L * (K + 1)
        say("(c) scann_index_ridge_loo: %9.2f / %9.2f ms; with the residuals copied back %9.2f / %9.2f ms; 2 N m L (K + 1) = %.3g flops are "
            "%.2f Tflop/s if all of the call were the kernel" % (tc[0] * 1e3, tc[1] * 1e3, tr[0] * 1e3, tr[1] * 1e3, flops, flops / tc[0] / 1e12))
        res, head = lat.fit_head(t)
        td = timed(lambda: lat.fit_head(t))
        say("(d) LatentIndex.fit_head end to end: %9.2f / %9.2f ms; picks %s, loo_rmse %s" % (td[0] * 1e3, td[1] * 1e3, pick.tolist(),
                                                                                            np.array2string(res["loo_rmse"][:3], precision=4)))
        runs = [host_route(lat, t, fit["l2"]) for _ in range(2 if N > 1000000 else 3)]
        tt = np.array([r[0] for r in runs])
        say("(e) without the calls: rows() download %8.1f, np.cov fp64 %8.1f, eigh %6.1f, closed form at the %d strengths %8.1f, in all %8.1f ms (min "
            "of %d); OMP_NUM_THREADS %s" % (tuple(tt.min(axis=0)[:3] * 1e3) + (L, tt.min(axis=0)[3] * 1e3, tt.min(axis=0)[4] * 1e3, len(runs),
                                            os.environ.get("OMP_NUM_THREADS", "unset"))))
        dev = np.sqrt(first["sse"][:, 0] / mo["n"])
        ref = np.sqrt(runs[0][1][:L, 0] / N)
        say("    loo_rmse of target 0 along the grid, device against the host route: largest relative difference %.3g" % float(np.max(np.abs(dev - ref) / ref)))
        lat.free()
