"""Reference of the readout head on a latent index (scann_index_fit_moments / scann_index_ridge_loo / scann_head_batch and the twin
scann_ridge_loo_host, include/scann_hip.h), restated in plain NumPy from the header's text: which rows count, the fp32 chains with the
fused multiply-add formed exactly (pca_ref.fma32), the residual epilogue, and the fp64 sums in blocks of 128 positions.  Beside it the
same formula in fp64 throughout, the closed form against explicit refits, and the host route of ``LatentIndex.fit_head``.  The
restatements share no code with the C twin."""
import numpy as np

import pca_ref

BLOCK = 128


def counts(rows, t):
    return np.isfinite(rows).all(axis=1) & np.isfinite(t).all(axis=1)


def augmented(rows, t):
    """[rows | t]: what scann_index_fit_moments takes the moments of"""
    t = np.asarray(t, np.float32)
    return np.concatenate([np.asarray(rows, np.float32), t.reshape(len(t), -1)], axis=1)


def loo(rows, t, mean, tmean, V, S, B, lev0, resid_l=None):
    """-> {"n", "sse", "sae", "sse_fit" [L, K], "dof" [L], with resid_l "resid" [N, K]}: the definition, operation by operation"""
    f32 = np.float32
    rows, t = np.asarray(rows, f32), np.asarray(t, f32).reshape(len(rows), -1)
    mean, tmean, V, S, B = (np.asarray(a, f32) for a in (mean, tmean, V, S, B))
    N, dim = rows.shape
    m, L, K = V.shape[0], S.shape[0], t.shape[1]
    ok = counts(rows, t)
    with np.errstate(all="ignore"):
        y = (rows - mean).astype(f32)
        z = np.zeros((N, m), f32)
        for j in range(dim):
            z = pca_ref.fma32(np.broadcast_to(y[:, j][:, None], (N, m)), np.broadcast_to(V[:, j][None, :], (N, m)), z)
        a = np.zeros((N, L), f32)
        p = np.zeros((N, L, K), f32)
        for c in range(m):
            tc = (z[:, c][:, None] * S[:, c][None, :]).astype(f32)
            a = pca_ref.fma32(tc, tc, a)
            p = pca_ref.fma32(np.broadcast_to(z[:, c][:, None, None], (N, L, K)), np.broadcast_to(B[:, :, c][None], (N, L, K)), p)
        lev = (f32(lev0) + a).astype(f32)
        d = (t - tmean).astype(f32)
        e = (d[:, None, :] - p).astype(f32)
        q = (e.astype(np.float64) / (1.0 - lev.astype(np.float64))[:, :, None]).astype(f32)
        r = np.where((lev < f32(1))[:, :, None], q, f32(np.inf)).astype(f32)
        out = {k: np.zeros((L, K)) for k in ("sse", "sae", "sse_fit")}
        out["dof"] = np.zeros(L)
        r64, e64, lev64 = r.astype(np.float64), e.astype(np.float64), lev.astype(np.float64)
        for g in range(0, N, BLOCK):
            blk = {k: np.zeros_like(v) for k, v in out.items()}
            for i in range(g, min(N, g + BLOCK)):
                if ok[i]:
                    blk["sse"] = blk["sse"] + r64[i] * r64[i]
                    blk["sae"] = blk["sae"] + np.abs(r64[i])
                    blk["sse_fit"] = blk["sse_fit"] + e64[i] * e64[i]
                    blk["dof"] = blk["dof"] + lev64[i]
            for k in out:
                out[k] = out[k] + blk[k]
    out["n"] = int(ok.sum())
    if resid_l is not None:
        res = np.full((N, K), np.nan, f32)
        for k, l in enumerate(resid_l):
            if l >= 0:
                res[ok, k] = r[ok, l, k]
        out["resid"] = res
    return out


def loo64(rows, t, mean, tmean, V, S, B, lev0, resid_l=None):
    """the same formula in fp64 throughout, plain sums"""
    rows, t = np.asarray(rows, np.float64), np.asarray(t, np.float64).reshape(len(rows), -1)
    mean, tmean, V, S, B = (np.asarray(a, np.float64) for a in (mean, tmean, V, S, B))
    ok = counts(rows, t)
    x, tt = rows[ok], t[ok]
    z = (x - mean) @ V.T
    lev = float(lev0) + np.einsum("nc,lc->nl", z * z, S * S)
    e = (tt - tmean)[:, None, :] - np.einsum("nc,lkc->nlk", z, B)
    with np.errstate(all="ignore"):
        r = np.where((lev < 1)[:, :, None], e / (1.0 - lev)[:, :, None], np.inf)
    out = {"n": int(ok.sum()), "sse": (r * r).sum(0), "sae": np.abs(r).sum(0), "sse_fit": (e * e).sum(0), "dof": lev.sum(0)}
    if resid_l is not None:
        res = np.full(t.shape, np.nan, np.float32)
        for k, l in enumerate(resid_l):
            if l >= 0:
                res[ok, k] = r[:, l, k]
        out["resid"] = res
    return out


def same_loo(got, want, label=""):
    assert got["n"] == want["n"], (label, got["n"], want["n"])
    for key in ("sse", "sae", "sse_fit", "dof") + (("resid",) if "resid" in want else ()):
        pca_ref.same(got[key], want[key], "%s %s" % (label, key))


def random_head(N, dim, m, L, K, seed=0):
    """arguments of a leave-one-out pass with leverages well below 1: (rows, t, mean, tmean, V, S, B, lev0)"""
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((N, dim)) * rng.uniform(0.5, 2, dim) + rng.standard_normal(dim)).astype(np.float32)
    t = rng.standard_normal((N, K)).astype(np.float32)
    mean = rows.mean(0).astype(np.float32)
    tmean = t.mean(0).astype(np.float32)
    V = (rng.standard_normal((m, dim)) / np.sqrt(dim)).astype(np.float32)
    S = (rng.uniform(0.2, 1.0, (L, m)) / np.sqrt(4.0 * m * max(N, 2))).astype(np.float32)
    B = (rng.standard_normal((L, K, m)) * 0.3).astype(np.float32)
    return rows, t, mean, tmean, V, S, B, np.float32(1.0 / N)


# ---- the closed form against explicit refits, fp64 ----

def closed_form_residuals(X, T, lam):
    """leave-one-out residuals [n, K] of ridge regression with an unpenalised intercept and penalty lam (n - 1) in the principal axes of X"""
    X, T = np.asarray(X, np.float64), np.asarray(T, np.float64).reshape(len(X), -1)
    n = len(X)
    xm, tm = X.mean(0), T.mean(0)
    Xc, Tc = X - xm, T - tm
    s, U = np.linalg.eigh(Xc.T @ Xc / (n - 1))
    z = Xc @ U
    g = U.T @ (Xc.T @ Tc / (n - 1))
    beta = g / (s + lam)[:, None]
    lev = 1.0 / n + (z * z / ((n - 1) * (s + lam))).sum(1)
    e = Tc - z @ beta
    return e / (1.0 - lev)[:, None]


def refit_residuals(X, T, lam):
    """the same residuals by n refits: row i left out, lambda' = lam (n - 1) / (n - 2), i.e. the same penalty alpha = lam (n - 1)"""
    X, T = np.asarray(X, np.float64), np.asarray(T, np.float64).reshape(len(X), -1)
    n, d = X.shape
    out = np.zeros_like(T)
    for i in range(n):
        keep = np.arange(n) != i
        Xi, Ti = X[keep], T[keep]
        xm, tm = Xi.mean(0), Ti.mean(0)
        Xc, Tc = Xi - xm, Ti - tm
        lam_i = lam * (n - 1) / (n - 2)
        b = np.linalg.solve(Xc.T @ Xc + lam_i * (n - 2) * np.eye(d), Xc.T @ Tc)
        out[i] = T[i] - (tm + (X[i] - xm) @ b)
    return out


# ---- the host route of LatentIndex.fit_head ----

def host_fit(rows, t, l2="loo", loo_fn=None, names=None, level="structure"):
    """``LatentIndex.fit_head`` without a GPU: moments_host of the augmented matrix, the product's closed form (sym_eig inside), and the
    leave-one-out passes by ``loo_fn`` (default: the C twin; ``loo64`` gives the fp64 restatement).  -> (result, head)"""
    from scann import _hip
    from scann.models import latent_index as li

    rows = np.ascontiguousarray(rows, np.float32)
    t = _hip.check_head_targets(t, len(rows))
    loo_fn = loo_fn or _hip.ridge_loo_host
    grid = li.head_grid(l2)
    fit = li.head_closed_form(_hip.moments_host(augmented(rows, t)), rows.shape[1], grid)
    args = (rows, t, fit["mean"], fit["tmean"], fit["components"], fit["scale"], fit["coef"], fit["lev0"])
    pick = li.head_pick(loo_fn(*args)["sse"], fit["l2"])
    names = ["target_%d" % k for k in range(t.shape[1])] if names is None else names
    return li.head_result(fit, loo_fn(*args, pick), pick, t, names, level, rows.shape[1])


def selection_case(N, dim, noise, seed):
    """the rows and two targets of the selection checks"""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((N, dim)) * rng.uniform(0.5, 2, dim) + 5 * rng.standard_normal(dim)).astype(np.float32)
    rw = np.random.default_rng(seed + 100)
    w = rw.standard_normal((dim, 2)) / np.sqrt(dim)
    T = ((X - 5) @ w + noise * rw.standard_normal((N, 2))).astype(np.float32)
    return X, T
