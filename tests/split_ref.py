"""NumPy emulation of the forward's split-fp16 projections, the low-range test cases, and the load-time rule that keeps
small operands off them.  TEST INFRASTRUCTURE ONLY (imported by test_low_range_host.py and test_gpu_low_range.py).

The 128 / 8 forward carries every fp32 operand x of a 128-wide projection as hi = fp16(x), lo = fp16(x - hi) (split4 on the device,
pack_weight_f16 on the host: round to nearest even, gradual underflow; weights are pre-scaled by 2^8) and forms a product from
three fp16 matrix products lo.hi + hi.lo + hi.hi into one accumulator.  While lo is a normal fp16 number the pair holds 22
significant bits; below that it has an ABSOLUTE quantum (2^-24, rounding error <= 2^-25), so an operand row whose largest
element is m carries a relative error of about 2^-25 / m.  `split_matmul` is that arithmetic (fp64 accumulation: the emulation is
about the operands, not about the order of the sums); `forward_split` is the oracle's forward with it patched into the
projections the GPU multiplies that way.

`small_operands` restates the classification scann_load_weights applies (scann_runtime.cpp, small_operand_reason): a checkpoint
for which it returns a reason runs its inference forwards on the exact-fp32 kernels, so `forward_guarded` -- what the GPU is
meant to compute -- is the fp32 oracle for those and the emulation for every other checkpoint."""
import contextlib

import numpy as np

import scann_oracle as so

WSCALE = 256.0
KS = (0, 6, 10, 14, 18)
# The rule's one constant.  An operand row (activations) or column (a kernel times 2^8) whose largest element m is below 2^-8
# carries 2^-25 / m > 2^-17 = 7.6e-6 of relative error per operand: more than a decade above fp32's 2^-24 and within a factor 13
# of the suite's bound of 1e-4, which the conditioning of two attention layers and the readout easily spends.  At m >= 2^-8 the
# split is within 2^-17 of every operand, and the k sweep of test_low_range_host.py shows what that leaves at the outputs.
SMALL = 2.0 ** -8


def split(x):
    """hi, lo fp16 parts of fp32 x, as fp32 arrays (values beyond 65504 become inf, as on the device)"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore"):
        hi = x.astype(np.float16).astype(np.float32)
        lo = (x - hi).astype(np.float16).astype(np.float32)
    return hi, lo


def split_matmul(x, w):
    """x [.., K] @ w [K, N] the way the split-fp16 kernels form it; fp32 result"""
    xh, xl = split(x)
    wh, wl = split(np.asarray(w, dtype=np.float32) * np.float32(WSCALE))
    xh, xl, wh, wl = (t.astype(np.float64) for t in (xh, xl, wh, wl))
    acc = np.matmul(xl, wh) + np.matmul(xh, wl) + np.matmul(xh, wh)
    return (acc / WSCALE).astype(np.float32)


def is_split_projection(cfg, prefix):
    """the Dense layers of the 128 / 8 forward that are multiplied in split-fp16 form with fp32 activations as operands: the
    K = 20 filters (Gaussians in [0, 1]) and dense_embed / bf_property / predict_property (plain fp32) are not"""
    leaf = prefix.rsplit("/", 1)[-1]
    if leaf == "filter_geo":
        return bool(cfg["model"].get("g_update", False))
    if leaf in ("query", "key", "dense_1", "dense_2"):
        return True
    return prefix == "after_Lc"


@contextlib.contextmanager
def _patched_dense(cfg):
    plain = so.dense

    def dense(x, w, prefix, dt, act=None):
        if np.dtype(dt) != np.float32 or not is_split_projection(cfg, prefix):
            return plain(x, w, prefix, dt, act)
        y = split_matmul(x, w[prefix + "/kernel"]) + w[prefix + "/bias"].astype(np.float32)
        return so.swish(y) if act == "swish" else y

    so.dense = dense
    try:
        yield
    finally:
        so.dense = plain


def forward_split(cfg, w, inputs, intermediates=None):
    """so.forward in fp32 with the unguarded split emulation in every projection the GPU's fast path multiplies that way"""
    with _patched_dense(cfg):
        return so.forward(cfg, w, inputs, np.float32, intermediates=intermediates)


# ---- the load-time classification (mirror of scann_runtime.cpp: small_operand_reason) ----

def _rms_out(gamma, beta, kernel, bias):
    """A LayerNorm output x = gamma * n + beta (n: zero mean, unit variance, taken as uncorrelated) through z = x . W + b: the
    root mean square of every z_j, sqrt(sum_k gamma_k^2 W_kj^2 + (sum_k beta_k W_kj + b_j)^2), in fp64"""
    g, b, W, c = (np.asarray(t, dtype=np.float64) for t in (gamma, beta, kernel, bias))
    return np.sqrt((g * g) @ (W * W) + (b @ W + c) ** 2)


def small_operands(cfg, w):
    """None, or why the split-fp16 projections would see an operand row / kernel column whose largest element is below SMALL:
    the text names the tensor.  Exact zeros are representable and never count: a column (or LayerNorm) of zeros is skipped."""
    m = cfg["model"]
    L, gu, an = m["n_attention"], m.get("g_update", False), m.get("use_attn_norm", True)
    if (m["local_dim"], m["global_dim"], m["dense_out"], m["num_head"]) != (128, 128, 128, 8):
        return None  # other widths run the plain-fp32 kernels

    def col_small(name, rows=None):
        W = np.abs(np.asarray(w[name], dtype=np.float64))
        if rows is not None:
            W = W[rows[0]:rows[1]]
        cm = W.max(0)
        cm = cm[cm > 0]
        return cm.size > 0 and cm.min() * WSCALE < SMALL

    def ln_size(prefix):  # the size of each component of this LayerNorm's output rows: sqrt(gamma_c^2 + beta_c^2)
        g, b = (np.asarray(w[prefix + s], dtype=np.float64) for s in ("/gamma", "/beta"))
        return np.sqrt(g * g + b * b)

    def ln_small(prefix):  # ... and the largest element a row is expected to have
        return 0 < ln_size(prefix).max() < SMALL

    def filter_size(prefix, top):  # a K = 20 filter is a function of one scalar: the largest |swish(gaussians(x) . W + b)| of each
        W, b = (np.asarray(w[prefix + s], dtype=np.float64) for s in ("/kernel", "/bias"))  # component over x = 0 .. top in 64 steps
        x = np.arange(65, dtype=np.float64)[:, None] * (top / 64.0)
        c = np.arange(so.N_GAUSS, dtype=np.float64)[None] * (top / (so.N_GAUSS - 1))
        z = np.exp(-(x - c) ** 2 / 0.25) @ W + b
        return np.abs(z / (1.0 + np.exp(-z))).max(0)

    gd = float(m["gaussian_d"])

    # the first layer's operands have no LayerNorm before them, but the loaded tensors fix them as well
    rows = first_centres(cfg, w)
    top = rows.max(1)
    if (top > 0).any() and top[top > 0].min() < SMALL:
        return "dense_embed: its swish output rows (the first layer's centres) stay below 2^-8"
    cen = rows.max(0)
    if gu and L > 0 and 0 < (filter_size("neighbor_d", gd) * filter_size("neighbor_w", 2 * np.pi)).max() < SMALL:
        return "neighbor_d, neighbor_w: the product of their swish outputs (the first layer's geometry) stays below 2^-8"
    for i in range(L):
        p, r = "local_attention_%d/" % i, "residual_norm_%d/" % i
        # the key projection's operand is a PRODUCT, component by component: centres x this layer's new geometry (base branch: x the
        # filtered Gaussians at their largest over the distances, times a neighbour weight that is 1 for an atom's widest neighbour)
        ang = cen * (ln_size(p + "layer_norm_g") if gu else filter_size(p + "filter_geo", gd))
        if 0 < ang.max() < SMALL:
            return p + "key: its operand rows (centres x geometry, component by component) stay below 2^-8"
        cen = ln_size((r if an else p) + "layer_norm")
        names = [p + "query/kernel", p + "key/kernel"] + ([r + "dense_1/kernel", r + "dense_2/kernel"] if an else [])
        for n in names:
            if col_small(n):
                return n + ": a column of the kernel is below 2^-16 throughout"
        if gu:
            for j, part in enumerate(("centre", "geometry", "neighbour")):
                if col_small(p + "filter_geo/kernel", (128 * j, 128 * j + 128)):
                    return p + "filter_geo/kernel: a column of its %s rows is below 2^-16 throughout" % part
            if ln_small(p + "layer_norm_g"):
                return p + "layer_norm_g: its output rows (the geometry) stay below 2^-8"
        ctx = p + "layer_norm"
        if ln_small(ctx):
            return ctx + ": its output rows (the context) stay below 2^-8"
        if an:
            if ln_small(r + "layer_norm"):
                return r + "layer_norm: its output rows (the centres) stay below 2^-8"
            # the swish hidden row of the ResidualNorm, the operand of dense_2: swish(z) ~ z / 2 for small z
            h = _rms_out(w[ctx + "/gamma"], w[ctx + "/beta"], w[r + "dense_1/kernel"], w[r + "dense_1/bias"])
            if 0 < h.max() * 0.5 < SMALL:
                return r + "dense_1: its swish output rows (the operand of dense_2) stay below 2^-8"
    for n in ("after_Lc/kernel", "global_attention/query/kernel", "global_attention/key/kernel"):
        if col_small(n):
            return n + ": a column of the kernel is below 2^-16 throughout"
    if L > 0:
        last = ("residual_norm_%d/layer_norm" if an else "local_attention_%d/layer_norm") % (L - 1)
        h = _rms_out(w[last + "/gamma"], w[last + "/beta"], w["after_Lc/kernel"], w["after_Lc/bias"])
        if 0 < h.max() * 0.5 < SMALL:
            return "after_Lc: its swish output rows (the operand of global_attention/query and key) stay below 2^-8"
    return None


def first_centres(cfg, w):
    """|centres| of the first layer, swish(dense_embed(.)), one row per input the table can hold: exact for the atomic embedding
    (rows 1 .., row 0 is the padding index; with use_ring times the four ring-feature combinations); for cgcnn features an upper
    bound of every row, taking the features in [0, 1] -- only a checkpoint whose rows are CERTAINLY small is then classified"""
    m = cfg["model"]
    f = lambda n: np.asarray(w[n], dtype=np.float64)
    We, be = f("dense_embed/kernel"), f("dense_embed/bias")
    if m.get("feature", "atomic") == "cgcnn":
        emb = (np.abs(f("embed_atom/bias")) + np.abs(f("embed_atom/kernel")).sum(0))[None]
        if m.get("use_ring", False):
            emb = np.concatenate([emb, (np.abs(f("extra_embed/bias")) + np.abs(f("extra_embed/kernel")).sum(0))[None]], 1)
        return np.abs(be) + emb @ np.abs(We)  # |swish(z)| <= |z|
    emb = f("embed_atom/embeddings")[1:]
    if m.get("use_ring", False):
        ring = np.array([[0, 0], [0, 1], [1, 0], [1, 1]], dtype=np.float64) @ f("extra_embed/kernel") + f("extra_embed/bias")
        emb = np.concatenate([np.repeat(emb, 4, 0), np.tile(ring, (emb.shape[0], 1))], 1)
    z = emb @ We + be
    return np.abs(z / (1.0 + np.exp(-z)))


def forward_guarded(cfg, w, inputs, intermediates=None):
    """what the GPU forward computes: the exact-fp32 kernels (the fp32 oracle) where the load-time rule fires, the split elsewhere"""
    if small_operands(cfg, w) is not None:
        return so.forward(cfg, w, inputs, np.float32, intermediates=intermediates)
    return forward_split(cfg, w, inputs, intermediates=intermediates)


# ---- the cases: checkpoints whose named tensors are scaled by 2^-k (exact in fp32), so that a following normalisation makes the
# asserted tensors scale-free ----

CASE_TENSORS = {
    "A": ["residual_norm_0/layer_norm/gamma", "residual_norm_0/layer_norm/beta", "local_attention_1/query/bias", "local_attention_1/key/bias"],
    "B": ["local_attention_1/layer_norm_g/gamma", "local_attention_1/layer_norm_g/beta", "local_attention_1/key/bias",
          "local_attention_1/query/kernel", "local_attention_1/query/bias"],
    "D": ["after_Lc/kernel", "after_Lc/bias", "global_attention/query/bias", "global_attention/key/bias"],
    "W": ["local_attention_1/key/kernel", "local_attention_1/key/bias", "local_attention_1/query/kernel", "local_attention_1/query/bias"],
    "R": ["residual_norm_0/dense_1/kernel", "residual_norm_0/dense_1/bias"],
}
# P, the key projection's operand is a product: centres AND geometry at 2^-k each (either alone is harmless at k = 6), the biases at 2^-2k
CASE_TENSORS["P"] = CASE_TENSORS["A"][:2] + ["local_attention_1/layer_norm_g/gamma", "local_attention_1/layer_norm_g/beta",
                                             "local_attention_1/query/kernel", "local_attention_1/query/bias", "local_attention_1/key/bias"]
# E, the first layer's centres: no LayerNorm precedes them, swish(dense_embed(embedding)) is fixed by the loaded tensors
CASE_TENSORS["E"] = ["dense_embed/kernel", "dense_embed/bias", "local_attention_0/query/bias", "local_attention_0/key/bias"]
TWICE = {"P": ("local_attention_1/query/bias", "local_attention_1/key/bias")}  # tensors scaled by 2^-2k
CASE_TENSORS["M"] = CASE_TENSORS["A"]
CASE_TENSORS["A_no_attn_norm"] = ["local_attention_0/layer_norm/gamma", "local_attention_0/layer_norm/beta"] + CASE_TENSORS["A"][2:]
CASES = ("A", "B", "D", "W", "R", "M", "P", "E")


def r_up(w, k):
    """case R: the power dense_2/kernel is raised by -- k while the kernel stays below 255.9, otherwise the largest that does"""
    top = float(np.abs(w["residual_norm_0/dense_2/kernel"]).max())
    while k > 0 and not top * 2.0 ** k < 255.9:
        k -= 1
    return k


def scaled(w, case, k):
    """the checkpoint of `case` at 2^-k; k = 0 returns the very arrays of w"""
    out = dict(w)
    if k == 0:
        return out
    f = np.float32(2.0 ** -k)
    for n in CASE_TENSORS[case]:
        t = np.array(w[n], dtype=np.float32)
        if case == "M":
            t[..., ::2] *= f  # every second component small, its neighbours ordinary: a row's LARGEST element decides its precision
        else:
            t *= f * f if n in TWICE.get(case, ()) else f
        out[n] = t
    if case == "R":
        out["residual_norm_0/dense_2/kernel"] = (w["residual_norm_0/dense_2/kernel"] * np.float32(2.0 ** r_up(w, k))).astype(np.float32)
    return out


def config(**model):
    cfg = so.default_config("qm9")
    cfg["model"]["n_attention"] = 2
    cfg["model"].update(model)
    return cfg


def ordinary_checkpoints():
    """(label, cfg, weights, padded inputs) of the checkpoints that must stay on the fast path: the default configurations, perturbed and at the
    Keras-default initialisation, the committed golden models and the Keras-layout .h5 fixture's weights"""
    import importlib.util
    import os

    here = os.path.dirname(os.path.abspath(__file__))

    def load(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(here, "golden", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    for name in ("qm9", "mp2018", "qm9_std"):
        for perturb in (True, False):
            cfg = so.default_config(name)
            de, dn = so.synth_dataset(4, 2, "mp2018" if name == "mp2018" else "qm9")
            yield "%s perturb=%s" % (name, perturb), cfg, so.init_weights(cfg, 1234, perturb=perturb), so.pad_batch(de, dn, cfg["model"]["g_update"])[0]
    for name in ("qm9", "mp2018"):  # a fresh base-branch model: its first layer's key operand is the smallest an ordinary checkpoint has
        cfg = so.default_config(name)
        cfg["model"]["g_update"] = False
        de, dn = so.synth_dataset(4, 2, name)
        yield "%s base perturb=False" % name, cfg, so.init_weights(cfg, 1234, perturb=False), so.pad_batch(de, dn, False)[0]
    mg = load("make_golden")
    for name in ("qm9_plus", "qm9_base", "qm9_no_norms", "qm9_e_b", "mp2018", "dense_and_sparse"):
        cfg, w, inputs = mg.build(name)
        yield "golden " + name, cfg, w, inputs
    # the committed Keras-layout file itself, through the package's own reader (the golden .npz files hold inputs and expected outputs,
    # no weights: their models are what make_golden.build returns, pinned to the files by test_golden_vectors)
    from scann.models.keras_import import load_keras_h5
    from scann.models.scann_model import normalize_config

    fx = load("make_keras_fixture")
    cfg, w = load_keras_h5(os.path.join(here, "golden", fx.NAME), {"model": {"n_atoms": 10, "scale": 0.5}, "hyper": {"target": "homo"}})
    de, dn = so.synth_dataset(4, 2)
    yield fx.NAME, normalize_config(cfg), w, so.pad_batch(de, dn, cfg["model"]["g_update"])[0]


def far_edges(inputs, cfg):
    """case G: every fourth real edge 1 A, every eighth 2 A beyond the last Gaussian centre -- all 20 Gaussians of those rows are tiny"""
    out = {k: np.array(v) for k, v in inputs.items()}
    d = out["neighbor_distance"]
    idx = np.flatnonzero(out["neighbor_mask"].ravel())
    d.ravel()[idx[::4]] = np.float32(cfg["model"]["gaussian_d"] + 1.0)
    d.ravel()[idx[::8]] = np.float32(cfg["model"]["gaussian_d"] + 2.0)
    return out


# ---- what is asserted: every output of the public API, by name, and the acceptance rule of test_branches ----

def _parity():
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("_split_ref_parity", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RTOL, rel_err = _parity().RTOL, _parity().rel_err  # the suite's own bound and error measure (test_gpu_parity.py)


def output_names(cfg):
    return (["predict_property", "global_attention"] + ["local_attention_%d" % k for k in range(cfg["model"]["n_attention"])] +
            ["after_Lc", "bf_property"])


def outputs_of(cfg, inputs, fwd):
    """name -> array in the layout predict(padded, outputs=...) returns, from fwd(intermediates) -> (y, ga); plus the per-layer
    centres / geometry / context under the oracle's names, real rows only (what debug_read returns)"""
    inter = {}
    y, ga = fwd(inter)
    amask = np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0
    emask = (np.asarray(inputs["neighbor_mask"]) != 0) & amask[:, :, None]
    L = cfg["model"]["n_attention"]
    out = {"predict_property": y, "global_attention": ga, "after_Lc": inter["after_Lc"] * amask[..., None], "bf_property": inter["struc_rep"]}
    for k in range(L):
        a = inter["attn_local_%d" % (k + 1)]
        if a.dtype == np.float64:  # (in fp64 a logit + -1e9 keeps the logit: the 1/N rows are an fp32 convention, test_gpu_outputs.py)
            a = a.copy()
            a.transpose(0, 2, 3, 1)[~emask.any(-1)] = 1.0 / emask.shape[2]
        out["local_attention_%d" % k] = a
    for l in range(L + 1):
        out["centers_%d" % l] = inter["centers_%d" % l][amask]
        if "geometry_%d" % l in inter:
            out["geometry_%d" % l] = inter["geometry_%d" % l][emask]
        if l >= 1:
            out["context_%d" % l] = inter["context_%d" % l][amask]
    return out


def references(cfg, w, inputs):
    """(fp32 oracle, fp64 oracle) outputs_of"""
    return tuple(outputs_of(cfg, inputs, lambda it, dt=dt: so.forward(cfg, w, inputs, dt, intermediates=it)) for dt in (np.float32, np.float64))


def judge(got, ref32, ref64, names=None):
    """[(name, error against fp64, bound = max(RTOL, 2 x the fp32 oracle's own error), finite, that fp32 error)] of every name in got"""
    rows = []
    for n in (names if names is not None else got):
        g = np.asarray(got[n])
        assert g.shape == ref64[n].shape, (n, g.shape, ref64[n].shape)
        e32 = rel_err(ref32[n], ref64[n])
        rows.append((n, rel_err(g, ref64[n]), max(RTOL, 2 * e32), bool(np.isfinite(g).all()), e32))
    return rows


def failures(rows):
    return [(n, e, b) for n, e, b, fin, _ in rows if not (fin and e <= b)]
