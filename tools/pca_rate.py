#!/usr/bin/env python3
"""Cost of the principal-component map on the device against the route without it, on one box:
    python tools/pca_rate.py [--tenth] [--kernels WHAT | --summary TRACE.csv WHAT] [--mad64 RATE] [out.txt]
A QM9-sized atom-level shape: N = 2,400,000 seeded rows of 128 columns (--tenth: 240,000), columns of different scale and offset.
Prints (and appends to out.txt), host clock around synchronous calls, warm, three runs each, min / median:
  (a) scann_index_moments (Engine.index_moments): eligibility, mean, the integer scatter, the fp64 covariance, one host wait;
  (b) the eigen-decomposition of the 128 x 128 covariance on the host (scann_sym_eig_host);
  (c) scann_index_project (Engine.index_project) with m = 2 and m = dim, coordinates and both distances copied back;
  (d) LatentIndex.pca(2) end to end;
  (e) the route a user has without the calls: LatentIndex.rows() (the download), np.cov in fp64 on the host's threads, numpy.linalg.eigh,
      and the projection (rows - mean) @ W.T in NumPy; each part on its own line.
--kernels WHAT (moments, project2 or projectdim): four calls of that one thing and no timing, for a run of its own under `rocprofv3
--kernel-trace --output-format csv -d DIR -- python tools/pca_rate.py --kernels WHAT`.  --summary TRACE.csv WHAT [out.txt] (no GPU)
then reads that run's *_kernel_trace.csv and prints, per pca_* kernel, the launches of one call and the time of one call summed over
them, min / median over the three calls behind the first, and the shares of the rates below.  One call of scann_index_project is
several launches where the coordinates pass through the 256 MiB device block a group of rows at a time (5 at m = 128 and 2.4 M rows),
so a kernel's time for the call is the sum over them, never a single launch.
The scatter is N x dim x (dim + 64) / 2 exact 32 x 32 + 64-bit multiply-adds as the kernel does them (whole 64 x 64 blocks of the upper
triangle); tools/mad64_rate.hip measures what the chip does of them per second from registers alone, and --mad64 RATE (multiply-adds per
second, its last line) makes this script print the kernel's share of it.  The projection is N x m x dim fused multiply-adds, two per
packed fp32 instruction-lane; the chip issues 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3 T of those per second."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
import scann_oracle as so
from scann import _hip
from scann.models import LatentIndex
from scann.models.scann_model import HipModel
argv = sys.argv[1:]
TAKES = {"--mad64": 1, "--kernels": 1, "--summary": 2}  # options and how many values follow them
opt, args, i = {}, [], 0
while i < len(argv):
    if argv[i] in TAKES:
        opt[argv[i]] = argv[i + 1:i + 1 + TAKES[argv[i]]]
        i += 1 + TAKES[argv[i]]
    else:
        if not argv[i].startswith("--"):
            args.append(argv[i])
        i += 1
mad64 = float(opt["--mad64"][0]) if "--mad64" in opt else None
WHATS = ("moments", "project2", "projectdim")
for o in ("--kernels", "--summary"):
    if o in opt and opt[o][-1] not in WHATS:
        raise SystemExit("%s: WHAT must be one of %s" % (o, ", ".join(WHATS)))
out_path = args[0] if args else None
N = 240000 if "--tenth" in argv else 2400000
D = 128
PACKED_LANES = 157.3e12 / 4  # packed fp32 instruction-lanes per second


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


def summary(path, what):
    """per-call kernel times from a kernel trace of `--kernels what`: the launches of every pca_* kernel in time order, cut into the
    run's calls (the first is the warm-up and is left out)"""
    import csv, re
    runs = {}
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        k = re.search(r"pca_\w+_kernel(<\d>)?", r["Kernel_Name"])
        if k:
            runs.setdefault(k.group(0), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    moments = ("pca_prepare_kernel", "pca_pass_kernel<0>", "pca_mean_kernel", "pca_pass_kernel<1>", "pca_scatter_kernel", "pca_finalise_kernel")
    # (the projections' runs make one call of the moments first, for the mean and the components: not theirs)
    names, calls = (moments, 5) if what == "moments" else (("pca_project_kernel", "pca_md2_kernel"), 4)
    m = {"project2": 2, "projectdim": D}.get(what)
    say("kernels of %s, N = %d x %d (rocprofv3 --kernel-trace; per call: launches, us summed over them, min / median of %d calls):" % (
        {"moments": "scann_index_moments", "project2": "scann_index_project m = 2", "projectdim": "scann_index_project m = %d" % D}[what], N, D, calls - 1))
    total = []
    for k in names:
        t = runs.get(k, [])
        if not t or len(t) % calls:
            raise SystemExit("%s: %d launches of %s do not make %d calls" % (path, len(t), k, calls))
        per = len(t) // calls
        sums = sorted(sum(t[c * per:(c + 1) * per]) for c in range(1, calls))
        total.append(sums)
        note = ""
        if k == "pca_scatter_kernel":
            mads = 1.0 * N * D * (D + 64) / 2
            note = "   %.3g multiply-adds: %.2f T/s" % (mads, mads / (sums[0] * 1e-6) / 1e12) + (
                "" if mad64 is None else " = %.1f %% of the register-only rate of %.2f T/s" % (100 * mads / (sums[0] * 1e-6) / mad64, mad64 / 1e12))
        if k == "pca_project_kernel":
            lanes = N * m * D / 2.0
            note = "   N x m x %d / 2 = %.3g packed fp32 instruction-lanes = %.1f %% of the 39.3 T lanes / s the chip issues" % (
                D, lanes, 100 * lanes / (sums[0] * 1e-6) / PACKED_LANES)
        say("  %-20s %2d x %9.1f / %9.1f%s" % (k, per, sums[0], float(np.median(sums)), note))
    say("  %-20s      %9.1f   (the kernels' minima together)" % ("all of them", sum(x[0] for x in total)))


if "--summary" in opt:
    summary(*opt["--summary"])
    sys.exit(0)

cfg = so.default_config("qm9")
model = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True)
eng = model.engine
rng = np.random.default_rng(7)
rows = rng.standard_normal((N, D), dtype=np.float32) * rng.uniform(0.05, 4, D).astype(np.float32) + rng.standard_normal(D).astype(np.float32)
lat = LatentIndex(model, "atom")
for i in range(0, N, 1 << 18):
    lat.add_rows(rows[i:i + (1 << 18)])
ix = lat._ix
mo = eng.index_moments(ix)  # warm: the workspace is in the block cache
w, v, sweeps = _hip.sym_eig(mo["cov"])
comp = v.astype(np.float32)
scale = (1 / np.sqrt(w)).astype(np.float32)
if "--kernels" in opt:
    for i in range(4):
        if opt["--kernels"][0] == "moments":
            eng.index_moments(ix)
        else:
            m = 2 if opt["--kernels"][0] == "project2" else D
            eng.index_project(ix, mo["mean"], comp[:m], scale[:m])
    lat.free()
    sys.exit(0)

say("principal-component map over N = %d rows x %d columns = %.1f MB; b = %d bits" % (N, D, N * D * 4 / 1e6, mo["bits"]))
ta = timed(lambda: eng.index_moments(ix))
mads = 1.0 * N * D * (D + 64) / 2
say("(a) scann_index_moments: %8.2f / %8.2f ms (min / median of 3); the scatter is %.3g 64-bit multiply-adds%s" % (
    ta[0] * 1e3, ta[1] * 1e3, mads, "" if mad64 is None else
    ": if all of the call were the scatter, %.1f %% of the measured register-only rate of %.2f T/s" % (100 * mads / ta[0] / mad64, mad64 / 1e12)))
tb = timed(lambda: _hip.sym_eig(mo["cov"]))
say("(b) scann_sym_eig_host, %d x %d, %d sweeps: %8.2f / %8.2f ms" % (D, D, sweeps, tb[0] * 1e3, tb[1] * 1e3))
for m in (2, D):
    eng.index_project(ix, mo["mean"], comp[:m], scale[:m])
    tc = timed(lambda: eng.index_project(ix, mo["mean"], comp[:m], scale[:m]))
    say("(c) scann_index_project m = %3d, %5.1f MB of results copied back: %8.2f / %8.2f ms; N x m x %d fused multiply-adds are %.1f %% of the "
        "packed-fp32 instruction rate if all of the call were the kernel" % (m, N * (m + 2) * 4 / 1e6, tc[0] * 1e3, tc[1] * 1e3, D,
                                                                              100 * (N * m * D / 2.0) / tc[0] / PACKED_LANES))
lat.pca(2)
td = timed(lambda: lat.pca(2))
say("(d) LatentIndex.pca(2) end to end: %8.2f / %8.2f ms" % (td[0] * 1e3, td[1] * 1e3))


def host_route(m):
    t0 = time.perf_counter()
    r = lat.rows()[0]
    t1 = time.perf_counter()
    mean = r.mean(axis=0, dtype=np.float64)
    cov = np.cov(r, rowvar=False, dtype=np.float64)
    t2 = time.perf_counter()
    hw, hv = np.linalg.eigh(cov)
    t3 = time.perf_counter()
    z = (r - mean.astype(np.float32)) @ hv[:, ::-1][:, :m].astype(np.float32)
    t4 = time.perf_counter()
    return (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0), cov, z


host_route(2)  # warm
for m in (2, D):
    runs = [host_route(m) for _ in range(3)]
    t = np.array([r[0] for r in runs])
    say("(e) without the calls, m = %3d: rows() download %7.1f, np.cov fp64 %7.1f, eigh %6.1f, NumPy projection %7.1f, in all %7.1f ms (min of 3 "
        "each; median in all %7.1f ms); OMP_NUM_THREADS %s" % ((m,) + tuple(t.min(axis=0) * 1e3) + (float(np.median(t[:, 4])) * 1e3, os.environ.get("OMP_NUM_THREADS", "unset"))))
cov = runs[0][1]
f = mo["col_exp"].astype(np.float64)
say("    the device's covariance against np.cov in fp64: largest |difference| over the definition's bound 2^(f_i + f_j - b + 2): %.4f" % float(
    (np.abs(mo["cov"] - cov) / 2.0 ** (f[:, None] + f[None, :] - mo["bits"] + 2)).max()))
lat.free()
