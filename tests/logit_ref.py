"""Reference of the classification head on a latent index (scann_index_logit_pass / scann_logit_head_batch and the twin
scann_logit_pass_host, include/scann_hip.h), restated in plain NumPy from the header's text: which rows count and train which model, the
fp32 logit chains with the fused multiply-add formed exactly (pca_ref.fma32), the softmax through the restated weight chain
(rbf_ref.weight), and the fp64 sums over the tree of blocks, spans and spans of the definition (np.cumsum adds strictly in order).  Beside
it an fp64 Newton fit of the same objective, the case builders, and the host route of ``LatentIndex.fit_class_head``.  The restatements
share no code with the C twin."""
import numpy as np

import pca_ref
import rbf_ref

BLOCK, SPAN = 128, 32
LOG2E = float.fromhex("0x1.715476p+0")


def softmax32(a, label):
    """a [n, C] fp32 logits, label [n] -> (p [n, C] fp32, best [n], brier [n] fp32): the definition, operation by operation"""
    f32 = np.float32
    n, C = a.shape
    with np.errstate(all="ignore"):
        amax, abest, best = a[:, 0].copy(), a[:, 0].copy(), np.zeros(n, np.int64)
        for k in range(1, C):
            amax = np.fmax(amax, a[:, k])  # fmaxf: a NaN loses against a number
            more = a[:, k] > abest
            abest, best = np.where(more, a[:, k], abest), np.where(more, k, best)
        w = rbf_ref.weight((amax[:, None] - a).astype(f32), LOG2E)
        S = w[:, 0].copy()
        for k in range(1, C):
            S = (S + w[:, k]).astype(f32)
        p = (w / S[:, None]).astype(f32)
        onehot = (np.arange(C)[None, :] == np.asarray(label)[:, None]).astype(f32)
        e = (p - onehot).astype(f32)
        b = np.zeros(n, f32)
        for k in range(C):
            b = pca_ref.fma32(e[:, k], e[:, k], b)
    return p, best, b


def logits32(rows, mean, U):
    """rows [n, dim], U [M, C, dim + 1] -> (y [n, dim], a [n, M, C]) fp32: the chain from the intercept, components ascending"""
    f32 = np.float32
    rows, mean, U = np.asarray(rows, f32), np.asarray(mean, f32), np.asarray(U, f32)
    n, dim = rows.shape
    M, C, _ = U.shape
    with np.errstate(all="ignore"):
        y = (rows - mean).astype(f32)
        a = np.broadcast_to(U[:, :, dim].reshape(1, M * C), (n, M * C)).astype(f32)
        for c in range(dim):
            a = pca_ref.fma32(np.broadcast_to(y[:, c][:, None], (n, M * C)), np.broadcast_to(U[:, :, c].reshape(1, M * C), (n, M * C)), a)
    return y, a.reshape(n, M, C)


def tree_sum(terms):
    """terms [N, ...] fp64, one per position (0 where a row adds nothing) -> their sum over the tree of the definition"""
    N = len(terms)
    total = np.zeros(terms.shape[1:])
    for s0 in range(0, N, BLOCK * SPAN):
        span = np.zeros(terms.shape[1:])
        for b0 in range(s0, min(N, s0 + BLOCK * SPAN), BLOCK):
            span = span + np.cumsum(terms[b0:b0 + BLOCK], axis=0)[-1]  # 0.0 + t_0 + t_1 + ... in position order
        total = total + span
    return total


def logit_pass(rows, labels, mean, U, fold=None, F=0, prob_of_fold=None):
    """-> {"n", "grad" [M, C, dim + 1], "stats" [M, 2, 3], with prob_of_fold "prob" [N, C]}: the definition"""
    f32 = np.float32
    rows, U = np.asarray(rows, f32), np.asarray(U, f32)
    labels = np.asarray(labels)
    N, dim = rows.shape
    M, C, _ = U.shape
    fold = np.full(M, -1) if fold is None else np.asarray(fold)
    out = {"grad": np.zeros((M, C, dim + 1)), "stats": np.zeros((M, 2, 3)), "n": 0}
    if prob_of_fold is not None:
        out["prob"] = np.full((N, C), np.nan, f32)
    if N == 0:
        return out
    counts = np.isfinite(rows).all(axis=1) & (labels >= 0) & (labels < C)
    out["n"] = int(counts.sum())
    y, a = logits32(rows, mean, U)
    y64 = np.concatenate([np.where(counts[:, None], y, 0).astype(np.float64), np.ones((N, 1))], axis=1)  # the intercept's "component" is 1
    pos_fold = np.arange(N) % F if F > 0 else np.zeros(N, np.int64)
    for j in range(M):
        p, best, brier = softmax32(a[:, j, :], labels)
        held = counts & (fold[j] >= 0) & (pos_fold == fold[j])
        train = counts & ~held
        onehot = (np.arange(C)[None, :] == labels[:, None]).astype(f32)
        with np.errstate(all="ignore"):
            r = (onehot - p).astype(f32)
        r64 = np.where(train[:, None], r, 0).astype(np.float64)
        for b0 in range(0, N, BLOCK * SPAN):  # (span by span: the terms of one span at a time keep the memory small)
            sl = slice(b0, min(N, b0 + BLOCK * SPAN))
            with np.errstate(all="ignore"):
                out["grad"][j] += tree_sum(r64[sl][:, :, None] * y64[sl][:, None, :])
        hit = (best == labels).astype(np.float64)
        for w, mask in enumerate((train, held)):
            terms = np.stack([mask.astype(np.float64), np.where(mask, hit, 0.0), np.where(mask, brier.astype(np.float64), 0.0)], axis=1)
            out["stats"][j, w] = tree_sum(terms)
        if prob_of_fold is not None:
            mine = counts & (np.asarray(prob_of_fold)[pos_fold] == j)
            out["prob"][mine] = p[mine]
    return out


def same_pass(got, want, label=""):
    assert got["n"] == want["n"], (label, got["n"], want["n"])
    for key in ("grad", "stats") + (("prob",) if "prob" in want else ()):
        pca_ref.same(got[key], want[key], "%s %s" % (label, key))
    assert ("prob" in got) == ("prob" in want), label


def random_pass(N, dim, C, M, F, seed=0, unlabelled=0.1, planted=True):
    """arguments of a pass: (rows, labels, mean, U, fold, F, prob_of_fold); with ``planted`` a few NaN / inf components and -1 labels"""
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((N, dim)) * rng.uniform(0.5, 2, dim) + rng.standard_normal(dim)).astype(np.float32)
    labels = rng.integers(0, C, N).astype(np.int32)
    if planted and N >= 8:
        labels[rng.random(N) < unlabelled] = -1
        bad = rng.choice(N, size=max(1, N // 50), replace=False)
        rows[bad[0::2], rng.integers(0, dim)] = np.nan
        rows[bad[1::2], rng.integers(0, dim)] = np.inf
    mean = rows[np.isfinite(rows).all(axis=1)].mean(0).astype(np.float32) if np.isfinite(rows).all(axis=1).any() else np.zeros(dim, np.float32)
    U = (rng.standard_normal((M, C, dim + 1)) * (1.5 / np.sqrt(dim))).astype(np.float32)
    fold = (np.arange(M) % (F + 1) - 1).astype(np.int32) if F else np.full(M, -1, np.int32)
    prob_of_fold = np.array([int(np.nonzero(fold == f)[0][0]) if (fold == f).any() else -1 for f in range(max(F, 1))], np.int32)
    if not F:
        prob_of_fold[0] = M - 1
    return rows, labels, mean, U, fold, F, prob_of_fold


# ---- the objective in fp64 and its Newton fit ----

def objective(rows, labels, U, l2, mean=None):
    """sum_i nll_i + (n - 1) l2 / 2 |W|^2 in fp64, over the rows with a label; U [C, dim + 1] in the original coordinates, the intercept
    last and unpenalised.  With every component kept |W|^2 is the same in the principal axes (an orthogonal change of basis)."""
    X, lab = np.asarray(rows, np.float64), np.asarray(labels)
    ok = lab >= 0
    X, lab = X[ok], lab[ok]
    mean = np.zeros(X.shape[1]) if mean is None else np.asarray(mean, np.float64)
    U = np.asarray(U, np.float64)
    a = (X - mean) @ U[:, :-1].T + U[:, -1]
    a = a - a.max(axis=1, keepdims=True)
    lse = np.log(np.exp(a).sum(axis=1))
    return float((lse - a[np.arange(len(lab)), lab]).sum() + (len(lab) - 1.0) * l2 / 2.0 * (U[:, :-1] ** 2).sum())


def newton_fit(rows, labels, C, l2, mean=None, iters=100):
    """the minimiser of ``objective`` by damped Newton steps in fp64 -> U [C, dim + 1]"""
    X, lab = np.asarray(rows, np.float64), np.asarray(labels)
    ok = lab >= 0
    X, lab = X[ok], lab[ok]
    n, dim = X.shape
    mean = np.zeros(dim) if mean is None else np.asarray(mean, np.float64)
    Z = np.concatenate([X - mean, np.ones((n, 1))], axis=1)
    pen = np.concatenate([np.full(dim, (n - 1.0) * l2), [0.0]])
    onehot = np.eye(C)[lab]
    U = np.zeros((C, dim + 1))
    f = objective(X, lab, U, l2, mean)
    for _ in range(iters):
        a = Z @ U.T
        p = np.exp(a - a.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        g = (p - onehot).T @ Z + pen[None, :] * U
        H = np.zeros((C, dim + 1, C, dim + 1))
        for k in range(C):
            for l in range(C):
                wgt = p[:, k] * ((k == l) - p[:, l])
                H[k, :, l, :] = (Z * wgt[:, None]).T @ Z
            H[k, :, k, :] += np.diag(pen)
        step = np.linalg.lstsq(H.reshape(C * (dim + 1), -1), g.ravel(), rcond=None)[0].reshape(C, dim + 1)
        t = 1.0
        while t > 1e-8:
            f_new = objective(X, lab, U - t * step, l2, mean)
            if f_new <= f:
                break
            t /= 2.0
        if not t > 1e-8 or f - f_new <= 1e-13 * abs(f):
            if t > 1e-8:
                U, f = U - t * step, f_new
            break
        U, f = U - t * step, f_new
    return U


def newton_cv_accuracy(rows, labels, C, l2, F):
    """held-out accuracy of the fp64 fit, the fold of a row its position mod F"""
    X, lab = np.asarray(rows, np.float64), np.asarray(labels)
    pos = np.arange(len(X)) % F
    hits = 0
    for f in range(F):
        U = newton_fit(X[pos != f], lab[pos != f], C, l2)
        a = X[pos == f] @ U[:, :-1].T + U[:, -1]
        hits += int((np.argmax(a, axis=1) == lab[pos == f]).sum())
    return hits / len(X)


def lbfgs64_gap(rows, labels, C, l2, tol, memory=8, iters=1000):
    """The yardstick of the optimiser check: a textbook L-BFGS in fp64 throughout (exact gradients, Armijo backtracking on the loss,
    the diagonal of Boehning's bound as the initial inverse Hessian) on ``objective``, stopped by the product's rule max |grad| / n <= tol
    -> (objective at the stop - objective at the Newton optimum) / n, iterations.  What stopping at ``tol`` costs, without any fp32."""
    X, lab = np.asarray(rows, np.float64), np.asarray(labels)
    ok = lab >= 0
    X, lab = X[ok], lab[ok]
    n, dim = X.shape
    mean = X.mean(0)
    s, Q = np.linalg.eigh((X - mean).T @ (X - mean) / (n - 1.0))
    Z = np.concatenate([(X - mean) @ Q, np.ones((n, 1))], axis=1)  # principal-axis coordinates and the intercept's 1
    pen = np.concatenate([np.full(dim, (n - 1.0) * l2), [0.0]])
    h0 = np.tile(np.concatenate([1.0 / ((n - 1.0) * (s / 2.0 + l2)), [2.0 / n]]), C)
    onehot = np.eye(C)[lab]

    def f_g(w):
        W = w.reshape(C, dim + 1)
        a = Z @ W.T
        a = a - a.max(axis=1, keepdims=True)
        e = np.exp(a)
        p = e / e.sum(axis=1, keepdims=True)
        f = float((np.log(e.sum(axis=1)) - a[np.arange(n), lab]).sum() + 0.5 * (pen[None, :] * W * W).sum())
        return f, ((p - onehot).T @ Z + pen[None, :] * W).ravel()

    w = np.zeros(C * (dim + 1))
    f, g = f_g(w)
    S, Y = [], []
    it = 0
    while np.abs(g).max() / n > tol and it < iters:
        q, al = g.copy(), []
        for sv, yv in zip(reversed(S), reversed(Y)):
            al.append(sv @ q / (yv @ sv))
            q -= al[-1] * yv
        q *= h0
        for (sv, yv), a in zip(zip(S, Y), reversed(al)):
            q += (a - yv @ q / (yv @ sv)) * sv
        d, t = -q, 1.0
        while True:
            f_new, g_new = f_g(w + t * d)
            if f_new <= f + 1e-4 * t * (g @ d) or t < 1e-10:
                break
            t /= 2.0
        sv, yv = t * d, g_new - g
        if yv @ sv > 0:
            S, Y = (S + [sv])[-memory:], (Y + [yv])[-memory:]
        w, f, g = w + t * d, f_new, g_new
        it += 1
    U = newton_fit(X, lab, C, l2, mean)
    return (f - objective(X, lab, U, l2, mean)) / n, it


def planted(N=600, dim=16, C=3, sep=8.0, seed=0):
    """C classes with centres sep e_k and unit noise: at sep = 8 the pairwise distances are 11.3 sigma"""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, N).astype(np.int32)
    rows = rng.standard_normal((N, dim))
    rows[np.arange(N), labels] += sep
    return rows.astype(np.float32), labels


# ---- the host route of LatentIndex.fit_class_head ----

def host_fit(rows, labels, l2="cv", folds=4, max_iter=100, tol=1e-4, classes=None, level="structure", raw=False):
    """``LatentIndex.fit_class_head`` without a GPU: moments_host, the product's optimiser and the passes by the C twin -> (result,
    head); ``raw``: the optimiser's own output instead"""
    from scann import _hip
    from scann.models import latent_index as li

    rows = np.ascontiguousarray(rows, np.float32)
    lab, classes = li.class_labels_arg(labels, classes, len(rows))
    grid, folds, max_iter, tol = li.class_fit_args(l2, folds, max_iter, tol)
    li.class_count_check(np.bincount(lab[lab >= 0], minlength=len(classes)), classes, folds)
    mo = _hip.moments_host(rows)

    def run_pass(weights, fold, prob_of_fold=None):
        return _hip.logit_pass_host(rows, lab, mo["mean"], weights, fold, folds, prob_of_fold)

    fit = li.class_head_fit(run_pass, mo, lab, len(classes), grid, folds, max_iter, tol)
    return fit if raw else li.class_head_result(fit, lab, classes, level, rows.shape[1])


def same_fit(got, head, want, head_w, skip=("cv_log_loss",), label=""):
    """every result key (but ``skip``) and every head array, bit for bit"""
    assert sorted(got) == sorted(want), (label, sorted(got), sorted(want))
    for key in want:
        if key in skip:
            continue
        if key == "path":
            assert sorted(got[key]) == sorted(want[key]), label
            for k in want[key]:
                pca_ref.same(np.asarray(got[key][k]), np.asarray(want[key][k]), "%s path %s" % (label, k))
        elif isinstance(want[key], np.ndarray):
            pca_ref.same(got[key], want[key], "%s %s" % (label, key))
        elif isinstance(want[key], float):
            pca_ref.same(np.float64(got[key]), np.float64(want[key]), "%s %s" % (label, key))
        else:
            assert got[key] == want[key], (label, key, got[key], want[key])
    for name in ("mean", "weights", "classes"):
        pca_ref.same(getattr(head, name), getattr(head_w, name), "%s head.%s" % (label, name))
    assert (head.l2, head.level, head.dim) == (head_w.l2, head_w.level, head_w.dim), label
