"""Host tests of the principal-component map (scann_index_moments / scann_index_project / scann_project_batch and their twins,
LatentIndex.pca, LatentProjection, HipModel.fit_projection / project): the host twins against the NumPy restatement of the definition
(tests/pca_ref.py), bit for bit; planted cases (a NaN row, an inf row, a constant column, all rows equal, duplicated rows); the b
formula; invariance under a permutation of the rows; the error bound against np.cov in fp64; the eigen-decomposition (orthogonality,
residual, eigenvalues against eigvalsh, order and sign, a repeated eigenvalue, a diagonal matrix, d = 1); LatentProjection's scale / rank
rule and its save / load; header, ctypes table and library agree; null and bad arguments; the kernels use no scratch and keep out of the
other kernels' name census; the Python layer raises before any upload; predict_model.py takes --project.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import abi_checks
import pca_ref
import scann_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_rows(N, dim, seed=None):
    rng = np.random.default_rng(N * 7 + dim * 3 if seed is None else seed)
    return (rng.standard_normal((N, dim)) * rng.uniform(0.01, 30, dim) + rng.standard_normal(dim) * 5).astype(np.float32)


# ---- moments ----

@pytest.mark.parametrize("dim", [1, 3, 16, 130])
@pytest.mark.parametrize("N", [2, 3, 100, 5000])
def test_moments_host_equals_the_definition(hip_lib, N, dim):
    from scann import _hip

    rows = random_rows(N, dim)
    got = _hip.moments_host(rows)
    pca_ref.same_moments(got, pca_ref.moments(rows), "N %d dim %d" % (N, dim))
    assert got["mean"].dtype == np.float32 and got["cov"].dtype == np.float64 and got["cov"].shape == (dim, dim)
    assert np.array_equal(got["cov"], got["cov"].T) and got["n"] == N and got["bits"] == 24
    # the error bound of the definition against the covariance in fp64
    ref = np.cov(rows.astype(np.float64), rowvar=False).reshape(dim, dim)
    f = got["col_exp"].astype(np.float64)
    bound = 2.0 ** (f[:, None] + f[None, :] - got["bits"] + 2)
    used = float((np.abs(got["cov"] - ref) / bound).max())
    print("N %d dim %d: %.4f of the bound" % (N, dim, used))
    assert used <= 1.0
    # a permutation of the rows: the same bits
    perm = np.random.default_rng(1).permutation(N)
    pca_ref.same_moments(_hip.moments_host(rows[perm]), got, "permuted")


def test_moments_host_threads_give_the_same_bits(hip_lib):
    """1,200 x 420 is above the twin's threshold for threading over the rows of T"""
    from scann import _hip

    rows = random_rows(1200, 420)
    pca_ref.same_moments(_hip.moments_host(rows), pca_ref.moments(rows), "threaded")


def test_moments_host_on_planted_rows(hip_lib):
    from scann import _hip

    rows = random_rows(300, 7, seed=5)
    rows[13, 6] = np.nan
    rows[200, 0] = np.inf
    rows[299, 3] = -np.inf
    rows[:, 2] = -1.75  # a constant column: its variance is exactly 0
    rows[50:60] = rows[4]  # duplicated rows
    got = _hip.moments_host(rows)
    pca_ref.same_moments(got, pca_ref.moments(rows), "planted")
    assert got["n"] == 297 and not got["cov"][2].any() and not got["cov"][:, 2].any() and got["mean"][2] == np.float32(-1.75)
    assert got["col_exp"][2] == 0
    # the ineligible rows count for nothing: the moments of the others alone
    clean = rows[np.isfinite(rows).all(axis=1)]
    pca_ref.same_moments(_hip.moments_host(clean), got, "without them")
    # all rows equal: the covariance is exactly 0, the mean the row
    same_rows = np.tile(random_rows(1, 16, seed=3), (50, 1))
    got = _hip.moments_host(same_rows)
    assert not got["cov"].any() and np.array_equal(got["mean"], same_rows[0]) and not got["col_exp"].any()
    # fewer than 2 eligible rows
    for bad in (rows[:1], rows[[13, 200, 5]], np.zeros((0, 3), np.float32)):
        with pytest.raises(ValueError, match="at least 2 rows"):
            _hip.moments_host(bad)


def test_bits_formula(hip_lib):
    from scann import _hip

    assert [_hip.pca_bits(n) for n in (2, 16383, 16384, 32767, 32768, 2400000, 2 ** 31 - 1)] == [24, 24, 23, 23, 23, 20, 15]
    for n in list(range(0, 70)) + [2 ** k + d for k in range(6, 31) for d in (-1, 0, 1)] + [2 ** 31 - 1]:
        b = _hip.pca_bits(n)
        assert b == pca_ref.bits(n) == min(24, (62 - n.bit_length()) // 2)
        assert n * 2 ** (2 * b) < 2 ** 62  # no partial sum of T can overflow
    for n in (-1, 2 ** 31):
        with pytest.raises(ValueError):
            _hip.pca_bits(n)
    # b at 16,383 / 16,384 rows, as the moments report it
    rows = random_rows(16384, 2)
    assert _hip.moments_host(rows[:16383])["bits"] == 24 and _hip.moments_host(rows)["bits"] == 23
    pca_ref.same_moments(_hip.moments_host(rows), pca_ref.moments(rows), "16,384 rows")


# ---- eigen-decomposition ----

def check_eig(a, label):
    from scann import _hip

    d = len(a)
    w, v, sweeps = _hip.sym_eig(a)
    tol = d * 2.0 ** -44  # Jacobi is backward stable to a modest multiple of d * eps: 512 x
    scale = max(abs(w[0]), abs(w[-1]), np.finfo(np.float64).tiny)
    orth = float(np.abs(v @ v.T - np.eye(d)).max())
    resid = float(np.abs(a @ v.T - v.T * w).max() / scale)
    eigs = float(np.abs(w - np.linalg.eigvalsh(a)[::-1]).max() / scale)
    print("%s: d %d, %d sweeps, orthogonality %.3g, residual %.3g, eigenvalues %.3g (allowed %.3g)" % (label, d, sweeps, orth, resid, eigs, tol))
    assert orth <= tol and resid <= tol and eigs <= tol
    assert np.all(np.diff(w) <= 0)  # descending
    top = np.abs(v).argmax(axis=1)  # the first index among ties
    assert np.all(v[np.arange(d), top] > 0)
    assert 1 <= sweeps < 64
    return w, v, sweeps


@pytest.mark.parametrize("d", [1, 2, 3, 16, 128])
def test_sym_eig_on_covariances(hip_lib, d):
    from scann import _hip

    cov = _hip.moments_host(random_rows(400, d))["cov"]
    check_eig(cov, "covariance")
    rng = np.random.default_rng(d)
    g = rng.standard_normal((d, d))
    check_eig(g + g.T, "indefinite")
    # only the upper triangle is read
    low = np.triu(cov) + np.tril(rng.standard_normal((d, d)), -1)
    a, b = _hip.sym_eig(cov), _hip.sym_eig(low)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_sym_eig_special_matrices(hip_lib):
    from scann import _hip

    # a diagonal matrix: no rotation, one sweep; order by value, ties by original column; every vector a unit vector
    w, v, sweeps = _hip.sym_eig(np.diag([1.0, 5.0, 5.0, -2.0, 0.0]))
    assert sweeps == 1 and w.tolist() == [5.0, 5.0, 1.0, 0.0, -2.0]
    assert v.argmax(axis=1).tolist() == [1, 2, 0, 4, 3] and np.array_equal(np.abs(v).sum(axis=1), np.ones(5)) and (v >= 0).all()
    # d = 1
    w, v, sweeps = _hip.sym_eig(np.array([[-3.5]]))
    assert w.tolist() == [-3.5] and v.tolist() == [[1.0]] and sweeps == 1
    # a repeated eigenvalue: 2 I + ones has eigenvalues (d + 2, 2, ..., 2)
    d = 6
    w, v, _ = check_eig(2 * np.eye(d) + np.ones((d, d)), "repeated")
    assert abs(w[0] - (d + 2)) <= 1e-13 and np.abs(w[1:] - 2).max() <= 1e-13
    # rank-deficient: more columns than rows
    w, v, _ = check_eig(_hip.moments_host(random_rows(10, 40))["cov"], "rank 9")
    assert np.abs(w[9:]).max() <= 40 * 2.0 ** -44 * w[0]
    # the sign rule: the largest entry of the leading vector of [[2, -1], [-1, 2]] (eigenvalue 3, vector (1, -1) / sqrt 2) is the first
    w, v, _ = _hip.sym_eig(np.array([[2.0, -1.0], [-1.0, 2.0]]))
    assert abs(w[0] - 3) <= 1e-15 and v[0, 0] > 0 and v[0, 1] < 0 and v[1, 0] > 0 and v[1, 1] > 0
    for bad in (np.zeros((2, 3)), np.zeros(4), np.array([[1.0, np.nan], [np.nan, 1.0]]), np.zeros((0, 0))):
        with pytest.raises(ValueError):
            _hip.sym_eig(bad)


# ---- projection ----

@pytest.mark.parametrize("N,dim,m", [(1, 1, 1), (50, 3, 2), (257, 130, 65), (100, 128, 128)])
def test_project_host_equals_the_definition(hip_lib, N, dim, m):
    from scann import _hip

    rng = np.random.default_rng(N + dim + m)
    rows = random_rows(N, dim)
    if N > 10:
        rows[5, dim - 1] = np.nan
        rows[6, 0] = np.inf
    mean = rng.standard_normal(dim).astype(np.float32)
    comp = rng.standard_normal((m, dim)).astype(np.float32)
    scale = rng.uniform(0, 2, m).astype(np.float32)
    scale[0] = 0  # a component left out of md2
    got = _hip.project_host(rows, mean, comp, scale)
    pca_ref.same_projection(got, pca_ref.project(rows, mean, comp, scale), "N %d dim %d m %d" % (N, dim, m))
    assert got["coords"].shape == (N, m) and got["coords"].dtype == np.float32
    pca_ref.same(got["dist2"], _hip.knn_dist2_matrix(rows, mean[None, :])[:, 0], "dist2 is the distance chain")
    if N > 10:
        assert np.isnan(got["coords"][5]).all() and np.isnan(got["md2"][5]) and not np.isfinite(got["dist2"][6])
    plain = _hip.project_host(rows, mean, comp)
    assert sorted(plain) == ["coords", "dist2"]
    pca_ref.same(plain["coords"], got["coords"], "without scale")


def test_latent_projection_scale_rank_save_and_load(hip_lib, tmp_path):
    from scann import _hip
    from scann.models import LatentProjection

    # a planted rank-deficient set: 40 rows in a 3-dimensional subspace of 8 columns, plus a constant column
    rng = np.random.default_rng(2)
    rows = (rng.standard_normal((40, 3)) @ rng.standard_normal((3, 8))).astype(np.float32)
    rows[:, 5] = 1.0
    mo = _hip.moments_host(rows)
    w, v, _ = _hip.sym_eig(mo["cov"])
    noise = 8 * 2.0 ** (2 * int(mo["col_exp"].max()) - mo["bits"] + 2)
    print("eigenvalues", w, "noise floor", noise)
    assert (w[:3] > noise).all() and (w[3:] <= noise).all()
    p = LatentProjection(mo["mean"], v.astype(np.float32), w, noise, "atom")
    assert p.rank == 3 and p.m == 8 and p.dim == 8 and p.scale.dtype == np.float32
    assert np.array_equal(p.scale[:3], (1 / np.sqrt(w[:3])).astype(np.float32)) and not p.scale[3:].any()
    # the components at or below the floor add nothing to the Mahalanobis distance
    r = _hip.project_host(rows, p.mean, p.components, p.scale)
    r3 = _hip.project_host(rows, p.mean, p.components[:3], p.scale[:3])
    pca_ref.same(r["md2"], r3["md2"], "md2 over the rank")
    out = p.finish(r)
    assert sorted(out) == ["coordinates", "distance_to_mean", "mahalanobis"]
    pca_ref.same(out["mahalanobis"], np.sqrt(r["md2"]), "mahalanobis")
    # the mean squared Mahalanobis distance of the fitted rows over a full-rank map is (n - 1) / n * rank, up to the fp32 chains
    assert abs(float(r["md2"].astype(np.float64).mean()) - 3 * 39 / 40) <= 1e-3
    p.save(str(tmp_path / "map.npz"))
    cfg = so.default_config("qm9")
    cfg["model"]["global_dim"] = 8
    model = type("M", (), {"config": cfg})()
    back = LatentProjection.load(model, str(tmp_path / "map.npz"))
    for key in ("mean", "components", "variance", "scale"):
        pca_ref.same(getattr(back, key), getattr(p, key), key)
    assert back.level == "atom" and back.rank == 3 and back.noise_floor == noise and back.dim == 8
    with np.load(str(tmp_path / "map.npz"), allow_pickle=False) as z:
        assert sorted(z.files) == ["components", "dim", "level", "mean", "noise_floor", "variance"]
    cfg["model"]["global_dim"] = 16
    with pytest.raises(ValueError, match="does not fit"):
        LatentProjection.load(model, str(tmp_path / "map.npz"))
    with pytest.raises(ValueError, match="does not fit"):
        p.check_model(model)
    for bad in (dict(level="bond"), dict(variance=w[:3]), dict(noise_floor=-1.0), dict(noise_floor=np.nan), dict(dim=9),
                dict(components=v[:, :7].astype(np.float32)), dict(mean=np.full(8, np.inf, np.float32)), dict(variance=np.full(8, np.nan))):
        args = dict(mean=mo["mean"], components=v.astype(np.float32), variance=w, noise_floor=noise, level="atom")
        args.update(bad)
        with pytest.raises(ValueError):
            LatentProjection(**args)


# ---- ABI, arguments, kernels ----

def test_header_and_python_agree(hip_lib):
    import ctypes as C

    from scann import _hip

    h = abi_checks.header()
    abi_checks.declared("int scann_index_moments(scann_handle_t* h, scann_index_t* pool, int64_t* n_eligible, float* mean /* [dim] */, "
                        "double* cov /* [dim * dim] */, int32_t* col_exp /* [dim] or NULL */, int32_t* bits /* or NULL */);",
                        "int scann_index_project(scann_handle_t* h, scann_index_t* pool, int64_t first, int64_t n, const float* mean, "
                        "const float* components, const float* scale, int32_t m, float* coords /* [n * m] */, float* md2 /* [n] or NULL */, "
                        "float* dist2 /* [n] or NULL */);",
                        "int scann_project_batch(scann_handle_t* h, scann_dbatch_t* db, int32_t level, const float* mean, const float* components, "
                        "const float* scale, int32_t m, float* y, float* ga, float* coords, float* md2, float* dist2);",
                        "int scann_moments_host(const float* rows, int64_t n, int64_t dim, int64_t* n_eligible, float* mean, double* cov, "
                        "int32_t* col_exp, int32_t* bits);",
                        "int scann_project_host(const float* rows, int64_t n, int64_t dim, const float* mean, const float* components, "
                        "const float* scale, int32_t m, float* coords, float* md2, float* dist2);",
                        "int scann_sym_eig_host(const double* a, int64_t d, double* w, double* v, int32_t* sweeps);",
                        "int scann_pca_bits(int64_t n);")
    assert "#define SCANN_ABI_VERSION 1" in h and hip_lib.scann_abi_version() == 1
    P = C.c_void_p
    sig = abi_checks.signatures({
        "scann_index_moments": (C.c_int, [P] * 7),
        "scann_index_project": (C.c_int, [P, P, C.c_int64, C.c_int64, P, P, P, C.c_int32, P, P, P]),
        "scann_project_batch": (C.c_int, [P, P, C.c_int32, P, P, P, C.c_int32, P, P, P, P, P]),
        "scann_moments_host": (C.c_int, [P, C.c_int64, C.c_int64, P, P, P, P, P]),
        "scann_project_host": (C.c_int, [P, C.c_int64, C.c_int64, P, P, P, C.c_int32, P, P, P]),
        "scann_sym_eig_host": (C.c_int, [P, C.c_int64, P, P, P]),
        "scann_pca_bits": (C.c_int, [C.c_int64])})
    for name in sig:
        assert hasattr(hip_lib, name), name


def test_null_and_bad_arguments_are_errors_not_crashes(hip_lib):
    import ctypes as C

    from scann import _hip

    P = _hip._ptr
    rows = np.arange(6, dtype=np.float32).reshape(3, 2) ** 2
    mean, cov, ex = np.zeros(2, np.float32), np.zeros((2, 2)), np.zeros(2, np.int32)
    ne = C.c_int64(0)
    assert hip_lib.scann_index_moments(None, None, C.byref(ne), P(mean), P(cov), None, None) == -1
    assert hip_lib.scann_index_project(None, None, 0, 1, P(mean), P(rows), None, 1, P(cov), None, None) == -1
    assert hip_lib.scann_project_batch(None, None, 2, P(mean), P(rows), None, 1, None, None, P(cov), None, None) == -1
    mh = hip_lib.scann_moments_host
    assert mh(None, 3, 2, C.byref(ne), P(mean), P(cov), P(ex), None) == -1       # rows null
    assert mh(P(rows), 3, 2, None, P(mean), P(cov), P(ex), None) == -1           # n_eligible null
    assert mh(P(rows), 3, 2, C.byref(ne), None, P(cov), P(ex), None) == -1       # mean null
    assert mh(P(rows), 3, 2, C.byref(ne), P(mean), None, P(ex), None) == -1      # cov null
    assert mh(P(rows), 3, 0, C.byref(ne), P(mean), P(cov), P(ex), None) == -1    # dim < 1
    assert mh(P(rows), -1, 2, C.byref(ne), P(mean), P(cov), P(ex), None) == -1
    assert mh(P(rows), 1, 2, C.byref(ne), P(mean), P(cov), P(ex), None) == -1 and ne.value == 1  # one row
    assert mh(P(rows), 3, 2, C.byref(ne), P(mean), P(cov), None, None) == 0 and ne.value == 3     # col_exp, bits may be null
    assert mean.tolist() == [np.float32(20 / 3), np.float32(35 / 3)]
    ph = hip_lib.scann_project_host
    comp, coords, md2 = np.ones((1, 2), np.float32), np.zeros((3, 1), np.float32), np.zeros(3, np.float32)
    assert ph(None, 3, 2, P(mean), P(comp), None, 1, P(coords), None, None) == -1   # rows null
    assert ph(P(rows), 3, 2, None, P(comp), None, 1, P(coords), None, None) == -1   # mean null
    assert ph(P(rows), 3, 2, P(mean), None, None, 1, P(coords), None, None) == -1   # components null
    assert ph(P(rows), 3, 2, P(mean), P(comp), None, 1, None, None, None) == -1     # coords null
    assert ph(P(rows), 3, 2, P(mean), P(comp), None, 0, P(coords), None, None) == -1  # m < 1
    assert ph(P(rows), 3, 2, P(mean), P(comp), None, 3, P(coords), None, None) == -1  # m > dim
    assert ph(P(rows), 3, 2, P(mean), P(comp), None, 1, P(coords), P(md2), None) == -1  # md2 without scale
    assert ph(P(rows), 3, 2, P(mean), P(comp), None, 1, P(coords), None, None) == 0
    eh = hip_lib.scann_sym_eig_host
    a, w, v = np.eye(2), np.zeros(2), np.zeros((2, 2))
    assert eh(None, 2, P(w), P(v), None) == -1 and eh(P(a), 2, None, P(v), None) == -1 and eh(P(a), 2, P(w), None, None) == -1
    assert eh(P(a), 0, P(w), P(v), None) == -1 and eh(P(a), 2, P(w), P(v), None) == 0  # sweeps may be null
    # the Python checks name the argument
    m3, c3, s3 = np.zeros(3, np.float32), np.ones((2, 3), np.float32), np.ones(2, np.float32)
    assert [x.dtype for x in _hip.check_pca_args([0, 0, 0], [[1, 0, 0]], [1])] == [np.float32] * 3
    for kw, word in ((dict(mean=np.zeros((1, 3))), "mean"), (dict(mean=np.zeros(0)), "mean"), (dict(dim=4), "mean"), (dict(mean="x"), "mean"),
                     (dict(components=np.ones(3)), "components"), (dict(components=np.ones((2, 4))), "components"),
                     (dict(components=np.ones((4, 3))), "components"), (dict(components=np.ones((0, 3))), "components"),
                     (dict(scale=np.ones(3)), "scale"), (dict(scale=np.ones((2, 1))), "scale"),
                     (dict(mean=np.float32([0, np.nan, 0])), "mean holds a non-finite"),
                     (dict(components=np.float32([[1, 0, 0], [0, np.inf, 0]])), "components holds a non-finite"),
                     (dict(scale=np.float32([1, -np.inf])), "scale holds a non-finite")):
        args = dict(mean=m3, components=c3, scale=s3)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            _hip.check_pca_args(**args)
    for bad in (np.zeros(3, np.float32), np.zeros((2, 0), np.float32)):
        with pytest.raises(ValueError):
            _hip.moments_host(bad)
        with pytest.raises(ValueError):
            _hip.project_host(bad, m3, c3)


def test_pca_kernels_use_no_scratch_and_keep_their_names_apart(hip_lib):
    """the kernels of csrc/scann_pca.hip spill nothing, read from the built library's kernel descriptors; their names stay out of the
    name census the other host tests take"""
    from scann import _hip

    kern = {n: v for n, v in abi_checks.device_kernels(_hip.LIB_PATH).items() if "pca_" in n}
    for want, count in (("pca_prepare_kernel", 1), ("pca_pass_kernel", 2), ("pca_mean_kernel", 1), ("pca_scatter_kernel", 1),
                        ("pca_finalise_kernel", 1), ("pca_project_kernel", 1), ("pca_md2_kernel", 1)):
        assert sum(want in n for n in kern) == count, (want, sorted(kern))
    assert len(kern) == 8, sorted(kern)
    for name, (scratch, vgpr) in kern.items():
        assert scratch == 0, (name, scratch, vgpr)
        for other in ("knn_", "kcenter_", "kmeans_", "rollout_", "ablate_", "input_grad_kernel"):
            assert other not in name, name


# ---- the Python layer against a stand-in engine ----

def _model(cfg):
    """test_knn_host's stand-in engine (rows [s, 0, ...] per structure, [s, a, 0, ...] per atom), with the moments and the projections
    answered by the host twins"""
    import test_knn_host as tk
    from scann import _hip

    class StandIn(tk._StandIn):
        def index_moments(self, ix):
            self.calls.append(("moments", len(ix)))
            return _hip.moments_host(ix.rows)

        def index_project(self, ix, mean, components, scale=None, first=0, n=None):
            self.calls.append(("project", len(components)))
            return _hip.project_host(ix.rows, mean, components, scale)

    m = tk._model(cfg)
    m.engine = StandIn(m.config)
    return m


def test_python_layer_raises_before_any_upload():
    from scann.models import LatentProjection

    cfg = so.default_config("qm9")
    inputs, _ = so.pad_batch(*so.synth_dataset(4, 2), g_update=True)
    m = _model(cfg)
    for kw in (dict(m=0), dict(m=129), dict(m=2.5), dict(m=None), dict(m=True), dict(level="bond"), dict(batch_size=0)):
        with pytest.raises(ValueError):
            m.fit_projection(inputs, **kw)
    with pytest.raises(ValueError):
        m.project(inputs, np.zeros((2, 128), np.float32))  # no LatentProjection
    narrow = LatentProjection(np.zeros(64, np.float32), np.ones((2, 64), np.float32), [2.0, 1.0], 0.0, "atom")
    with pytest.raises(ValueError, match="does not fit"):
        m.project(inputs, narrow)
    fits = LatentProjection(np.zeros(128, np.float32), np.ones((2, 128), np.float32), [2.0, 1.0], 0.0, "atom")
    with pytest.raises(ValueError):
        m.project(inputs, fits, batch_size=0)
    assert m.engine.uploads == 0 and not m.engine.calls and m.engine.created == 0
    pool = m.build_index(inputs)  # rows [s, 0, ...], s = 0 .. 3
    up = m.engine.uploads
    m.engine.calls.clear()
    for bad in (0, 129, 1.5, "2"):
        with pytest.raises(ValueError):
            pool.pca(bad)
    with pytest.raises(ValueError):
        pool.project(fits)  # an atom-level projection, a structure-level index
    with pytest.raises(ValueError):
        pool.project("a projection")
    with pytest.raises(ValueError):
        _model(so.default_config("qm9")).fit_projection(pool)  # another model's index
    assert not m.engine.calls and m.engine.uploads == up


def test_python_layer_result_on_a_stand_in_engine():
    from scann.models import LatentProjection

    cfg = so.default_config("qm9")
    inputs, _ = so.pad_batch(*so.synth_dataset(6, 2), g_update=True)
    m = _model(cfg)
    pool = m.build_index(inputs)  # rows [s, 0, ...], s = 0 .. 5: one direction, variance 3.5
    m.engine.calls.clear()
    r, proj = m.fit_projection(pool, m=2)
    assert m.engine.calls == [("moments", 6), ("project", 2)]
    assert sorted(r) == ["components", "coordinates", "distance_to_mean", "explained_variance_ratio", "mahalanobis", "mean", "n_rows",
                         "noise_floor", "rank", "total_variance", "variance"]
    assert isinstance(proj, LatentProjection) and proj.level == "structure" and proj.dim == 128 and proj.m == 2
    assert r["n_rows"] == 6 and r["rank"] == 1 and r["total_variance"] == 3.5 and r["variance"].tolist() == [3.5, 0.0]
    assert r["explained_variance_ratio"].tolist() == [3.5 / (3.5 * (1 + 130 * 2.0 ** -52)), 0.0] and r["mean"][0] == 2.5 and not r["mean"][1:].any()
    assert r["components"][0].tolist() == [1.0] + [0.0] * 127 and proj.scale.tolist() == [np.float32(1 / np.sqrt(3.5)), 0.0]
    assert r["coordinates"][:, 0].tolist() == [-2.5, -1.5, -0.5, 0.5, 1.5, 2.5] and not r["coordinates"][:, 1].any()
    assert r["distance_to_mean"].tolist() == [2.5, 1.5, 0.5, 0.5, 1.5, 2.5]
    assert np.array_equal(r["mahalanobis"], np.sqrt(np.square(r["coordinates"][:, 0] * proj.scale[0])))
    # a row with a non-finite component counts for nothing and maps to NaN
    pool.add_rows(np.full((1, 128), np.nan, np.float32))
    r2, _ = pool.pca(1)
    assert r2["n_rows"] == 6 and np.isnan(r2["coordinates"][6]).all() and np.isnan(r2["mahalanobis"][6]) and np.isnan(r2["distance_to_mean"][6])
    assert np.array_equal(r2["coordinates"][:6, 0], r["coordinates"][:, 0])
    # data instead of an index: indexed for the call
    created = m.engine.created
    r3, _ = m.fit_projection(inputs, m=1)
    assert m.engine.created == created + 1 and np.array_equal(r3["coordinates"][:, 0], r["coordinates"][:, 0])


def test_explained_ratio_sums_to_at_most_one():
    from scann.models.latent_index import explained_ratio

    rng = np.random.default_rng(0)
    for d in (1, 2, 3, 16, 128, 1024):
        for trial in range(50):
            w = np.sort(rng.uniform(0, 1, d) ** rng.integers(1, 9))[::-1] * 10.0 ** rng.integers(-20, 20)
            if trial % 3 == 0:
                w[d // 2:] = w[d // 2]  # equal eigenvalues
            if trial % 5 == 0 and d > 2:
                w[-2:] = [-1e-18 * w[0], -2e-18 * w[0]]  # rounding noise of a rank-deficient covariance
            r = explained_ratio(w)
            assert r.dtype == np.float64 and np.all(r >= 0) and np.all(np.diff(r) <= 0)
            for total in (r.sum(), np.cumsum(r)[-1], np.cumsum(r[::-1])[-1], sum(r.tolist())):
                assert total <= 1 and 1 - total <= 4 * (d + 2) * 2.0 ** -52
            assert r[: d // 2 + 1].sum() <= 1
    assert explained_ratio([0.0, 0.0]).tolist() == [0.0, 0.0] and explained_ratio([-1.0]).tolist() == [0.0]
    assert explained_ratio([3.0, 1.0]).tolist() == [3.0 / (4.0 * (1 + 4 * 2.0 ** -52)), 1.0 / (4.0 * (1 + 4 * 2.0 ** -52))]


def test_rotating_every_nonzero_entry_does_not_end_on_a_repeated_eigenvalue():
    """why scann_sym_eig_host drops an entry below half an ulp of both diagonal entries: the same sweeps restated in NumPy with the bare
    rule -- a rotation if and only if a_pq != 0 -- still rotate in their 64th sweep on 2 I + ones, whose eigenvalue 2 is five-fold,
    while with the dropping rule they end within a few sweeps (and so does the library)"""
    from scann import _hip

    def sweeps(a, drop):
        a = np.array(a, dtype=np.float64)
        d = len(a)
        for n_sweep in range(1, 65):
            rotated = False
            for p in range(d - 1):
                for q in range(p + 1, d):
                    apq, app, aqq = a[p, q], a[p, p], a[q, q]
                    if apq == 0:
                        continue
                    if drop and abs(app) + abs(apq) == abs(app) and abs(aqq) + abs(apq) == abs(aqq):
                        a[p, q] = a[q, p] = 0.0
                        continue
                    rotated = True
                    theta = (aqq - app) / (2 * apq)
                    t = (-1.0 if theta < 0 else 1.0) / (abs(theta) + np.sqrt(theta * theta + 1)) if np.isfinite(theta * theta) else 1 / (2 * theta)
                    c = 1 / np.sqrt(t * t + 1)
                    s = t * c
                    rp, rq = a[p].copy(), a[q].copy()
                    a[p], a[q] = c * rp - s * rq, s * rp + c * rq
                    a[p, p], a[q, q], a[p, q], a[q, p] = app - t * apq, aqq + t * apq, 0.0, 0.0
                    a[:, p], a[:, q] = a[p], a[q]
            if not rotated:
                return n_sweep, True
        return 64, False

    with np.errstate(all="ignore"):
        a = 2 * np.eye(6) + np.ones((6, 6))
        assert sweeps(a, drop=False) == (64, False)
        n, ended = sweeps(a, drop=True)
    assert ended and n <= 8
    assert _hip.sym_eig(a)[2] <= 8


def test_cli_takes_project():
    spec = importlib.util.spec_from_file_location("predict_model_cli", os.path.join(ROOT, "predict_model.py"))
    src = open(spec.origin).read()
    for flag in ("--project", "--project-level", "--project-out"):
        assert '"%s"' % flag in src, flag
    assert "projection_{}.pickle" in src and "fit_projection" in src
