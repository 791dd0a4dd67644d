#!/usr/bin/env python3
"""Cost of the silhouette of a labelled latent index beside the density self-join of the same run, on one box:
    python tools/silhouette_rate.py [--small] [--no-sample] [out.txt]
Indices of N = 16,384 and 131,072 seeded rows of 128 columns (--small: the first only).  Prints (and appends to out.txt), host clock around
synchronous calls, warm, min / median of five (three at 131,072 rows):
  (a) Engine.index_silhouette over all rows at C = 8, 64 and 1,024 balanced random labels, metric euclidean, the shift LatentIndex.silhouette
      chooses;
  (b) the yardstick: Engine.index_density with the index's own rows as host queries, each leaving out its own position -- the same 3 N N D
      of distance arithmetic -- and the ratio (a) / (b).  What to expect: the pass does the density pass's distance arithmetic and swaps the
      weight polynomial for a square root and a conversion, so at C = 8 it should land in the band the sibling kernels show against each
      other (1.00 - 1.10 x, README.md); every cluster is padded to whole 64-row tiles, at most 63 rows each, which is the price at C = 1,024;
  (c) a sampled call: 16,384 query positions against an index of 2,400,000 rows, C = 64 (--no-sample and --small: left out);
  (d) LatentIndex.choose_k over ks = 2, 4, 8, 16, 32, 64 end to end at 16,384 rows, and LatentIndex.silhouette alone;
  (e) at 16,384 rows the host twin (_hip.silhouette_host, std::thread, 16 threads at most) and sklearn.metrics.silhouette_samples on fp64
      copies with n_jobs = 16: the host routes.
FLOP/s are over 3 N Q D.  The kernel's registers come from the compiler (make -C scann--material_amd/csrc resource-usage)."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
argv = sys.argv[1:]
args = [a for a in argv if not a.startswith("--")]
out_path = args[0] if args else None
D = 128


def say(line):
    print(line, flush=True)
    if out_path:
        open(out_path, "a").write(line + "\n")


def timed(f, runs=5):
    t = []
    for r in range(runs):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return min(t), float(np.median(t))


import scann_oracle as so
from scann import _hip
from scann.models import LatentIndex
from scann.models.scann_model import HipModel

cfg = so.default_config("qm9")
model = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True)
eng = model.engine


def make(N, seed=7):
    """rows around 40 centres, as tools/peaks_rate.py makes them"""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((40, D), dtype=np.float32)
    rows = centres[rng.integers(0, 40, N)] + rng.standard_normal((N, D), dtype=np.float32)
    lat = LatentIndex(model, "atom")
    for i in range(0, N, 1 << 18):
        lat.add_rows(rows[i:i + (1 << 18)])
    return lat, rows


def shift_of(lat):
    mo = eng.index_moments(lat._ix)
    return _hip.silhouette_shift(mo["col_exp"], np.diagonal(mo["cov"]), "euclidean")


GAMMA = _hip.rbf_gamma(12.0)
say("sil_tile_kernel (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): 128 VGPRs (126 for the squared metric), no scratch, "
    "34,816 bytes of LDS, 4 waves per SIMD: four workgroups per CU")

for N in (16384,) if "--small" in argv else (16384, 131072):
    lat, rows = make(N)
    own = np.arange(N)
    flop = 3.0 * N * N * D
    shift = shift_of(lat)
    runs = 5 if N <= 20000 else 3
    say("silhouette of N = %d rows x %d columns, shift %d" % (N, D, shift))
    eng.index_density(lat._ix, rows, GAMMA, own)  # warm
    tb = timed(lambda: eng.index_density(lat._ix, rows, GAMMA, own), runs)
    tiny = LatentIndex(model, "atom").add_rows(rows[:64])
    eng.index_density(tiny._ix, rows, GAMMA)
    t0_ = timed(lambda: eng.index_density(tiny._ix, rows, GAMMA), runs)
    tiny.free()
    say("(b) Engine.index_density, the rows as host queries: %9.2f / %9.2f ms (min / median of %d): %.3g FLOP/s over 3 N N D; against 64 rows "
        "(the upload of the queries and the fixed costs) %9.2f ms" % (tb[0] * 1e3, tb[1] * 1e3, runs, flop / tb[0], t0_[0] * 1e3))
    for C in (8, 64, 1024):
        lab = (np.random.default_rng(C).permutation(N) % C).astype(np.int32)
        eng.index_silhouette(lat._ix, lab, C, None, "euclidean", shift)
        ta = timed(lambda: eng.index_silhouette(lat._ix, lab, C, None, "euclidean", shift), runs)
        pad = sum((int(n) + 63) // 64 * 64 for n in np.bincount(lab, minlength=C))
        say("(a) Engine.index_silhouette, C = %4d: %9.2f / %9.2f ms: %.3g FLOP/s; (a) / (b) = %.3f (medians %.3f), (a) / ((b) - upload) = %.3f; the "
            "padded clusters hold %d entries, %.3f x N" % (C, ta[0] * 1e3, ta[1] * 1e3, flop / ta[0], ta[0] / tb[0], ta[1] / tb[1],
                                                          ta[0] / (tb[0] - t0_[0]), pad, pad / N))
    if N <= 20000:
        ks = (2, 4, 8, 16, 32, 64)
        out = []
        tk = timed(lambda: out.append(lat.choose_k(ks)), 3)
        r = out[-1]
        res = lat.cluster(40)
        ts = timed(lambda: lat.silhouette(res["label"]), 3)
        say("(d) LatentIndex.choose_k(%s) end to end: %9.1f / %9.1f ms (min / median of 3); scores %s, best k %d; LatentIndex.silhouette of "
            "cluster(40) alone %9.1f / %9.1f ms, score %.4f" % (list(ks), tk[0] * 1e3, tk[1] * 1e3, " ".join("%.4f" % s for s in r["score"]),
                                                               r["best_k"], ts[0] * 1e3, ts[1] * 1e3, lat.silhouette(res["label"])["score"]))
        lab = res["label"]
        th = []
        for _ in range(2):
            t0 = time.perf_counter()
            host = _hip.silhouette_host(rows, lab, 40, None, "euclidean", shift)
            th.append(time.perf_counter() - t0)
        dev = eng.index_silhouette(lat._ix, lab, 40, None, "euclidean", shift)
        td = timed(lambda: eng.index_silhouette(lat._ix, lab, 40, None, "euclidean", shift))
        same = all(host[k].tobytes() == dev[k].tobytes() for k in host)
        say("(e) the host twin (_hip.silhouette_host), %d threads: %9.1f and %9.1f ms: %.0f x the device call (%9.2f ms); both routes agree in %s" % (
            min(16, len(os.sched_getaffinity(0))), th[0] * 1e3, th[1] * 1e3, min(th) / td[0], td[0] * 1e3, "every bit" if same else "NOT every bit"))
        try:
            from sklearn.metrics import silhouette_samples

            x64 = rows.astype(np.float64)
            t0 = time.perf_counter()
            s_ref = silhouette_samples(x64, lab, n_jobs=16)
            t_sk = time.perf_counter() - t0
            s_dev = lat.silhouette(lab)["silhouette"]
            say("    sklearn.metrics.silhouette_samples on fp64 copies, n_jobs = 16: %9.1f ms: %.0f x the device call; worst |s - s_sklearn| %.3g" % (
                t_sk * 1e3, t_sk / td[0], float(np.abs(s_dev - s_ref).max())))
        except ImportError:
            say("    sklearn is not installed: no silhouette_samples beside it")
    lat.free()

if "--no-sample" not in argv and "--small" not in argv:
    N, Q, C = 2400000, 16384, 64
    lat, rows = make(N, seed=9)
    del rows
    shift = shift_of(lat)
    lab = (np.random.default_rng(1).permutation(N) % C).astype(np.int32)
    q = np.sort(np.random.default_rng(2).choice(N, Q, replace=False)).astype(np.int32)
    eng.index_silhouette(lat._ix, lab, C, q, "euclidean", shift)
    tsamp = timed(lambda: eng.index_silhouette(lat._ix, lab, C, q, "euclidean", shift), 3)
    say("(c) Engine.index_silhouette, %d sampled positions against %d rows x %d, C = %d: %9.1f / %9.1f ms (min / median of 3): %.3g FLOP/s over "
        "3 N Q D" % (Q, N, D, C, tsamp[0] * 1e3, tsamp[1] * 1e3, 3.0 * N * Q * D / tsamp[0]))
    lat.free()
