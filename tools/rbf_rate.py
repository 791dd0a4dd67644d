#!/usr/bin/env python3
"""Cost of the Gaussian landmark features and of fitting a kernel head on a latent index, on one box:
    python tools/rbf_rate.py [--tenth] [--kernels N] [out.txt]
Index sizes N = 133,650 and 2,400,000 seeded rows of 128 columns (--tenth: 13,365 and 240,000), m = 256 landmarks (the index's own k-center
picks), one target that is quadratic in a 3-dimensional latent of the rows.  Prints (and appends to out.txt), host clock around
synchronous calls, warm, five runs each, min / median:
  (a) scann_index_rbf_features (Engine.index_rbf_features; the feature index freed outside the clock);
  (b) in the same run scann_index_query with the 256 landmarks as queries, k = 1, over the same pool: the same 3 N m dim chain arithmetic
      with a top-1 walk instead of the weight epilogue and the 4 N m bytes of writes; and the ratio (a) / (b);
  (c) LatentIndex.fit_kernel_head end to end with the default grid of 6 bandwidths;
  (d) the route a user has without the calls: LatentIndex.rows() (the download), NumPy exp(-cdist^2 / 2 h^2) at one bandwidth, np.cov,
      eigh and the same closed form of the leave-one-out residuals in NumPy -- per bandwidth, so the whole grid costs 6 x that beside
      the one download.
--kernels N: five calls of (a) and (b) at that size and no timing, for a run of its own under `rocprofv3 --kernel-trace --stats`."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
argv = sys.argv[1:]
kernels_n = int(argv[argv.index("--kernels") + 1]) if "--kernels" in argv else 0
args = [a for i, a in enumerate(argv) if not a.startswith("--") and not (i and argv[i - 1] == "--kernels")]
out_path = args[0] if args else None
SIZES = (13365, 240000) if "--tenth" in argv else (133650, 2400000)
D, M = 128, 256


def say(line):
    print(line, flush=True)
    if out_path:
        open(out_path, "a").write(line + "\n")


def timed(f, runs=5, after=None):
    t = []
    for r in range(runs):
        t0 = time.perf_counter()
        x = f()
        t.append(time.perf_counter() - t0)
        if after:
            after(x)
    return min(t), float(np.median(t))


import scann_oracle as so
from scann import _hip
from scann.models import LatentIndex
from scann.models import latent_index as li
from scann.models.scann_model import HipModel

cfg = so.default_config("qm9")
model = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True)
eng = model.engine


def make(N):
    rng = np.random.default_rng(7)
    u = rng.standard_normal((N, 3), dtype=np.float32)
    rows = (u @ rng.standard_normal((3, D)).astype(np.float32) + np.float32(0.05) * rng.standard_normal((N, D), dtype=np.float32)).astype(np.float32)
    t = ((u * u).sum(1) + np.float32(0.05) * rng.standard_normal(N, dtype=np.float32)).astype(np.float32)
    lat = LatentIndex(model, "atom")
    for i in range(0, N, 1 << 18):
        lat.add_rows(rows[i:i + (1 << 18)])
    return lat, t


def landmarks(lat):
    sel = eng.index_select(lat._ix, None, M + 1, 0.0)
    Z = np.concatenate([eng.index_read(lat._ix, int(p), 1)[0] for p in sel["position"][:M]])
    return Z, float(sel["radius2"][M])


if kernels_n:
    lat, t = make(kernels_n)
    Z, R2 = landmarks(lat)
    gamma = _hip.rbf_gamma(np.sqrt(4 * R2))
    for i in range(5):
        eng.index_rbf_features(lat._ix, Z, gamma).free()
        eng.index_query(lat._ix, Z, 1)
    lat.free()
    sys.exit(0)


def host_route(lat, t, Z, h, grid):
    t0 = time.perf_counter()
    r = lat.rows()[0]
    t1 = time.perf_counter()
    n = len(r)
    d2 = (r * r).sum(1)[:, None] + (Z * Z).sum(1)[None, :] - 2.0 * (r @ Z.T)  # cdist^2 in the product form, fp32 as a user would
    phi = np.exp(np.maximum(d2, 0) * np.float32(-1.0 / (2 * h * h)))
    t2 = time.perf_counter()
    aug = np.concatenate([phi, t.reshape(-1, 1)], axis=1)
    mean = aug.mean(axis=0, dtype=np.float64)
    cov = np.cov(aug, rowvar=False, dtype=np.float64)
    s, U = np.linalg.eigh(cov[:M, :M])
    s, U = np.maximum(s[::-1], 0), U[:, ::-1]
    t3 = time.perf_counter()
    z = (phi - mean[:M].astype(np.float32)) @ U.astype(np.float32)
    g = U.T @ cov[:M, M:]
    tc = t.reshape(-1, 1) - mean[M:].astype(np.float32)
    z2 = z * z
    best = np.inf
    for lam in grid:
        lev = 1.0 / n + z2 @ (1.0 / ((n - 1) * (s + lam))).astype(np.float32)
        e = tc - z @ (g / (s + lam)[:, None]).astype(np.float32)
        q = e / (1.0 - lev)[:, None]
        best = min(best, float(np.einsum("nk,nk->", q, q, dtype=np.float64)))
    t4 = time.perf_counter()
    return (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0), 1.0 - best / (cov[M, M] * (n - 1))


for N in SIZES:
    lat, t = make(N)
    ix = lat._ix
    Z, R2 = landmarks(lat)
    h = float(np.sqrt(4 * R2))
    gamma = _hip.rbf_gamma(h)
    eng.index_rbf_features(ix, Z, gamma).free()  # warm: the chunks and the workspace are in the block cache
    eng.index_query(ix, Z, 1)
    say("Gaussian features over N = %d rows x %d columns, m = %d landmarks, covering radius %.4g, h = %.4g" % (N, D, M, np.sqrt(R2), h))
    ta = timed(lambda: eng.index_rbf_features(ix, Z, gamma), after=lambda o: o.free())
    tb = timed(lambda: eng.index_query(ix, Z, 1))
    chain = 3.0 * N * M * D
    say("(a) scann_index_rbf_features: %9.2f / %9.2f ms (min / median of 5); 3 N m dim = %.3g operations are %.2f Top/s, the %.3g bytes written "
        "%.0f GB/s, if all of the call were the kernel" % (ta[0] * 1e3, ta[1] * 1e3, chain, chain / ta[0] / 1e12, 4.0 * N * M, 4.0 * N * M / ta[0] / 1e9))
    say("(b) scann_index_query, the %d landmarks as queries, k = 1: %9.2f / %9.2f ms; (a) / (b) = %.2f (min) %.2f (median)" % (
        M, tb[0] * 1e3, tb[1] * 1e3, ta[0] / tb[0], ta[1] / tb[1]))
    res, head = lat.fit_kernel_head(t, landmarks=M)
    tc = timed(lambda: lat.fit_kernel_head(t, landmarks=M), runs=3)
    say("(c) LatentIndex.fit_kernel_head end to end, 6 bandwidths: %9.2f / %9.2f ms (min / median of 3); bandwidth %.4g, loo_r2 %.4f (path %s)" % (
        tc[0] * 1e3, tc[1] * 1e3, res["bandwidth"], res["loo_r2"][0], np.array2string(res["bandwidth_path"]["loo_r2"][:, 0], precision=4)))
    runs = [host_route(lat, t, Z, res["bandwidth"], res["path"]["l2"]) for _ in range(2)]
    tt = np.array([r[0] for r in runs]).min(axis=0)
    say("(d) without the calls, one bandwidth: rows() download %8.1f, NumPy features %8.1f, np.cov and eigh %8.1f, closed form at the %d strengths "
        "%8.1f, in all %8.1f ms (min of 2; loo_r2 %.4f); the grid of 6: %8.1f ms, %.1f x (c); OMP_NUM_THREADS %s" % (
            tt[0] * 1e3, tt[1] * 1e3, tt[2] * 1e3, len(res["path"]["l2"]), tt[3] * 1e3, tt[4] * 1e3, runs[0][1], (tt[0] + 6 * (tt[4] - tt[0])) * 1e3,
            (tt[0] + 6 * (tt[4] - tt[0])) / tc[0], os.environ.get("OMP_NUM_THREADS", "unset")))
    lat.free()
