"""Reference of the Gaussian landmark features and of the kernel head fitted on them (scann_rbf_weight / scann_index_rbf_features /
scann_rbf_head_batch and the twin scann_rbf_features_host, include/scann_hip.h): the weight chain restated in NumPy from the header's
text, the planted data of the "is it worth having" check, an fp64 ridge on Gaussian features for that check, and the host route of
``LatentIndex.fit_kernel_head`` -- the whole fit without a GPU, from the host twins and the module-level head_* functions, with the
choice of the landmarks, the bandwidth grid and the winning bandwidth restated here."""
import numpy as np

import pca_ref

# the header's coefficients, as text: the fp32 roundings of 2^(-1/2) (-ln 2)^j / j!
COEF = [float.fromhex(x) for x in ("0x1.6a09e6p-1", "-0x1.f5e466p-2", "0x1.5be298p-3", "-0x1.41839ep-5", "0x1.bdb696p-8", "-0x1.ee4fd2p-11",
                                   "0x1.c8d752p-14", "-0x1.69e51ep-17")]
FACTORS = (1.0, 2.0, 4.0, 8.0, 16.0, 32.0)


def weight(dist2, gamma):
    """the definition, operation by operation, for an fp32 array of dist2 >= 0 (or NaN / +inf): fp32 throughout, fmaf formed exactly"""
    f32 = np.float32
    d = np.asarray(dist2, f32)
    with np.errstate(all="ignore"):
        u = (d * f32(gamma)).astype(f32)
        live = u < f32(126)
        uu = np.where(live, u, f32(0))
        i = np.floor(uu).astype(f32)
        g = ((uu - i).astype(f32) - f32(0.5)).astype(f32)
        p = np.full(d.shape, f32(COEF[7]), f32)
        for j in range(6, -1, -1):
            p = pca_ref.fma32(p, g, np.full(d.shape, f32(COEF[j]), f32))
        r = np.ldexp(p, -i.astype(np.int32)).astype(f32)
    return np.where(live, r, np.where(np.isnan(u), f32(np.nan), f32(0))).astype(f32)


def gamma_of(h):
    return float(np.float32(np.log2(np.e) / (2.0 * float(h) * float(h))))


def planted(N, dim, latent, seed):
    """u ~ N(0, I_latent), rows = u A + 0.01 noise (fp32), t = |u|^2 + 0.05 noise: a target no linear head can read"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((N, latent))
    A = rng.standard_normal((latent, dim))
    rows = (u @ A + 0.01 * rng.standard_normal((N, dim))).astype(np.float32)
    t = ((u * u).sum(1) + 0.05 * rng.standard_normal(N)).astype(np.float32)
    return rows, t


def landmarks_of(rows, landmarks):
    """(positions [m], Z [m, dim], R2): a count -> the first m picks of the k-center selection of m + 1 and the next pick's radius2;
    positions -> those rows and the largest least distance of the rows to them (one pick against them as the reference)"""
    from scann import _hip

    if isinstance(landmarks, (int, np.integer)):
        m = int(landmarks)
        sel = _hip.kcenter_host(rows, None, m + 1)
        if sel["count"] < m + 1:
            raise ValueError("needs more usable rows than landmarks")
        pos = sel["position"][:m].astype(np.int64)
        return pos, rows[pos], float(sel["radius2"][m])
    pos = np.asarray(landmarks, np.int64)
    sel = _hip.kcenter_host(rows, rows[pos], 1)
    return pos, rows[pos], float(sel["radius2"][0]) if sel["count"] else 0.0


def host_fit(rows, t, landmarks=256, bandwidth="loo", l2="loo", names=None, level="structure", ids=None, atoms=None):
    """``LatentIndex.fit_kernel_head`` without a GPU -> (result, head)"""
    from scann import _hip
    from scann.models import latent_index as li

    rows = np.ascontiguousarray(rows, np.float32)
    t = _hip.check_head_targets(t, len(rows))
    K = t.shape[1]
    names = ["target_%d" % k for k in range(K)] if names is None else names
    ids = np.arange(len(rows), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    atoms = np.full(len(rows), -1, np.int32) if atoms is None else np.asarray(atoms, np.int32)
    grid = li.head_grid(l2)
    pos, Z, R2 = landmarks_of(rows, landmarks)
    if isinstance(bandwidth, str):
        if not R2 > 0:
            raise ValueError("covering radius 0")
        hs = [float(np.sqrt(R2 * f)) for f in FACTORS]
    else:
        hs = [float(x) for x in np.atleast_1d(bandwidth)]
    m, tried = len(pos), []
    for h in hs:
        phi = _hip.rbf_features_host(rows, Z, gamma_of(h))
        fit = li.head_closed_form(_hip.moments_host(np.concatenate([phi, t], axis=1)), m, grid)
        args = (phi, t, fit["mean"], fit["tmean"], fit["components"], fit["scale"], fit["coef"], fit["lev0"])
        pick = li.head_pick(_hip.ridge_loo_host(*args)["sse"], fit["l2"])
        loo = _hip.ridge_loo_host(*args, pick)
        sse, tss = loo["sse"][pick, np.arange(K)], fit["tvar"] * (fit["n"] - 1.0)
        score = sum(float(sse[k]) / float(tss[k]) for k in range(K) if tss[k] != 0)
        tried.append((h, score, fit, loo, pick, sse, tss))
    best = None
    for e in tried:  # the least score, ties to the larger h
        if best is None or e[1] < best[1] or (e[1] == best[1] and e[0] > best[0]):
            best = e
    h, _, fit, loo, pick, _, _ = best
    result, inner = li.head_result(fit, loo, pick, t, names, level, m)
    head = li.LatentKernelHead(Z, gamma_of(h), inner, level, rows.shape[1], names)
    n = fit["n"]
    with np.errstate(divide="ignore", invalid="ignore"):
        path = {"bandwidth": np.array(hs), "loo_rmse": np.array([np.sqrt(e[5] / n) for e in tried]),
                "loo_r2": np.array([1.0 - e[5] / e[6] for e in tried])}
    result.update({"bandwidth": h, "landmark_position": pos.astype(np.int32), "landmark_id": ids[pos], "landmark_atom": atoms[pos],
                   "covering_radius": float(np.sqrt(np.float64(R2))), "bandwidth_path": path})
    return result, head


HEAD_ARRAYS = ("mean", "tmean", "weights", "components", "scale", "sigma2", "l2")


def same_fit(got, head, want, head_w, label=""):
    """every result key and every head array, bit for bit"""
    assert sorted(got) == sorted(want), (label, sorted(got), sorted(want))
    for key in want:
        if key in ("names", "n_rows"):
            assert got[key] == want[key], (label, key, got[key], want[key])
        elif key in ("path", "bandwidth_path"):
            assert sorted(got[key]) == sorted(want[key])
            for k2 in want[key]:
                pca_ref.same(got[key][k2], want[key][k2], "%s %s %s" % (label, key, k2))
        else:
            pca_ref.same(np.asarray(got[key]), np.asarray(want[key]), "%s %s" % (label, key))
    pca_ref.same(head.landmarks, head_w.landmarks, label + " landmarks")
    assert head.gamma == head_w.gamma and head.level == head_w.level and head.dim == head_w.dim and head.names == head_w.names
    assert head.head.lev0 == head_w.head.lev0
    for key in HEAD_ARRAYS:
        pca_ref.same(getattr(head.head, key), getattr(head_w.head, key), "%s head %s" % (label, key))


def ridge64_r2(X, t, lam_grid):
    """leave-one-out R^2 of fp64 ridge regression (unpenalised intercept) of t on X at its best strength: the check's yardstick"""
    X, t = np.asarray(X, np.float64), np.asarray(t, np.float64)
    n = len(X)
    Xc, tc = X - X.mean(0), t - t.mean()
    s, U = np.linalg.eigh(Xc.T @ Xc / (n - 1))
    z, g = Xc @ U, U.T @ (Xc.T @ tc / (n - 1))
    best = -np.inf
    for lam in lam_grid:
        lev = 1.0 / n + (z * z / ((n - 1) * (s + lam))).sum(1)
        r = (tc - z @ (g / (s + lam))) / (1.0 - lev)
        best = max(best, 1.0 - float((r * r).sum() / (tc * tc).sum()))
    return best
