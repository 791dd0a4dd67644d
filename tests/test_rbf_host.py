"""Host tests of the Gaussian landmark features and the kernel head (scann_rbf_weight, scann_rbf_features_host, the host route of
LatentIndex.fit_kernel_head, LatentKernelHead): the weight chain against the header's text restated in NumPy, bit for bit, and against
exp2 in fp64 within 3 x 2^-24; the feature twin with planted NaN / inf rows and against a plain NumPy exp; header, ctypes table and
library agree; the kernel uses no scratch; the feature is worth having -- on planted data a kernel head reads a target that no linear
head can --; which bandwidth wins; save / load; the Python layer raises before any upload; predict_model.py takes the flags.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import abi_checks
import head_ref
import pca_ref
import rbf_ref
import scann_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 3.0 * 2.0 ** -24  # relative, against exp2(-(double)u): measured 2.02 x 2^-24 with fmaf emulated in fp64; the real one is tighter


# ---- the weight chain ----

def test_weight_is_exactly_one_at_zero_and_stays_in_range(hip_lib):
    from scann import _hip

    rng = np.random.default_rng(0)
    for gamma in (1e-30, 0.37, 1.0, 3e4, 1e30):
        assert _hip.rbf_weight(0.0, gamma).view(np.uint32) == np.float32(1).view(np.uint32)
    d = np.concatenate([rng.uniform(0, 130, 200000), 10.0 ** rng.uniform(-40, 38, 200000), np.arange(0, 130), [125.99999, 126.0, 3e38]]).astype(np.float32)
    for gamma in (1.0, 0.01, 77.0):
        w = _hip.rbf_weight(d, gamma)
        assert w.dtype == np.float32 and w.shape == d.shape and np.all((w >= 0) & (w <= 1))
        with np.errstate(over="ignore"):
            u = (d * np.float32(gamma)).astype(np.float32)
        assert np.all(w[u >= 126] == 0) and np.all(w[u < 126] >= np.float32(2.0 ** -126)), "no denormal result arises"
    # whole u: exact powers of two
    assert np.array_equal(_hip.rbf_weight(np.arange(126, dtype=np.float32), 1.0), np.ldexp(np.float32(1), -np.arange(126)).astype(np.float32))


def test_weight_of_nan_inf_and_large_u(hip_lib):
    from scann import _hip

    assert np.isnan(_hip.rbf_weight(np.nan, 1.0)) and np.isnan(_hip.rbf_weight(np.float32([np.nan, 1.0]), 2.0)[0])
    assert _hip.rbf_weight(np.inf, 1e-20) == 0 and _hip.rbf_weight(126.0, 1.0) == 0 and _hip.rbf_weight(63.0, 2.0) == 0
    assert _hip.rbf_weight(3e38, 3e38) == 0  # u overflows to +inf
    assert _hip.rbf_weight(125.5, 1.0) == np.float32(2.0 ** -125.5)
    assert np.isnan(_hip.rbf_weight(np.inf, np.nan))


def test_weight_equals_the_restated_chain_and_exp2_within_the_bound(hip_lib):
    """2.3 M values of u over [0, 126): the twin against the NumPy restatement bit for bit, and against exp2(-(double)u)"""
    from scann import _hip

    rng = np.random.default_rng(1)
    d = np.concatenate([rng.uniform(0, 126, 1500000), rng.uniform(0, 2, 400000), 10.0 ** rng.uniform(-8, 2.1, 400000)]).astype(np.float32)
    worst = 0.0
    for gamma in (1.0, 0.73):
        w = _hip.rbf_weight(d, gamma)
        pca_ref.same(w, rbf_ref.weight(d, gamma), "gamma %g" % gamma)
        u = (d * np.float32(gamma)).astype(np.float32)
        live = u < 126
        ref = np.exp2(-u[live].astype(np.float64))
        worst = max(worst, float(np.max(np.abs(w[live].astype(np.float64) - ref) / ref)))
    print("%d values: largest relative error against exp2 %.3f x 2^-24 (bound 3)" % (2 * len(d), worst * 2.0 ** 24))
    assert worst <= BOUND
    # the scalar entry point is the array's
    for x in d[:200]:
        assert _hip.rbf_weight(float(x), 0.73).view(np.uint32) == _hip.rbf_weight(np.float32([x]), 0.73).view(np.uint32)[0]


def test_gamma_of_a_bandwidth():
    from scann import _hip

    for h in (0.01, 1.0, 3.7, 1e6):
        assert _hip.rbf_gamma(h) == float(np.float32(np.log2(np.e) / (2.0 * h * h))) == rbf_ref.gamma_of(h)
    for bad in (0.0, -1.0, np.nan, np.inf, "x", None, True, 1e-30, 1e30):
        with pytest.raises(ValueError):
            _hip.rbf_gamma(bad)


# ---- the feature twin ----

@pytest.mark.parametrize("N,dim,m", [(1, 1, 1), (127, 3, 5), (129, 130, 65), (300, 16, 257)])
def test_features_host(hip_lib, N, dim, m):
    from scann import _hip

    rng = np.random.default_rng(N + dim + m)
    rows = rng.standard_normal((N, dim)).astype(np.float32)
    Z = rng.standard_normal((m, dim)).astype(np.float32)
    h = float(np.sqrt(dim))
    gamma = _hip.rbf_gamma(h)
    if N > 100:
        rows[5, dim - 1] = np.nan
        rows[N - 1, 0] = np.inf
        rows[7] = 3e19  # finite, its distances overflow to +inf: the features are 0, not NaN
    phi = _hip.rbf_features_host(rows, Z, gamma)
    assert phi.shape == (N, m) and phi.dtype == np.float32
    # the definition: the weight chain on the distance chain, the pool row as q
    pca_ref.same(phi[np.isfinite(rows).all(1)], _hip.rbf_weight(_hip.knn_dist2_matrix(rows, Z), gamma)[np.isfinite(rows).all(1)], "definition")
    if N > 100:
        assert np.isnan(phi[5]).all() and np.isnan(phi[N - 1]).all() and not phi[7].any()
        assert not np.isnan(np.delete(phi, [5, N - 1], axis=0)).any()
    ok = np.isfinite(rows).all(1) & (np.abs(rows) < 1e10).all(1)
    d2 = ((rows[ok].astype(np.float64)[:, None, :] - Z.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    err = np.abs(phi[ok] - np.exp(-d2 / (2 * h * h)))
    print("N %d dim %d m %d: largest absolute deviation from NumPy's exp %.3g" % (N, dim, m, err.max()))
    assert err.max() <= 1e-6


def test_features_host_rejects_bad_arguments(hip_lib):
    from scann import _hip

    rows, Z = np.zeros((3, 4), np.float32), np.ones((2, 4), np.float32)
    for bad_z in (np.ones((2, 5), np.float32), np.ones((0, 4), np.float32), np.ones((1025, 4), np.float32), np.ones(4, np.float32), "z"):
        with pytest.raises(ValueError, match="landmarks"):
            _hip.rbf_features_host(rows, bad_z, 1.0)
    z = Z.copy()
    z[1, 2] = np.inf
    with pytest.raises(ValueError, match=r"landmark 1, column 2"):
        _hip.rbf_features_host(rows, z, 1.0)
    for bad_g in (0.0, -1.0, np.nan, np.inf, 1e-60, "g"):
        with pytest.raises(ValueError, match="gamma"):
            _hip.rbf_features_host(rows, Z, bad_g)
    lib, P = _hip.load_library(), _hip._ptr
    phi = np.full((3, 2), 7, np.float32)
    assert lib.scann_rbf_features_host(None, 3, 4, P(Z), 2, 1.0, P(phi)) == -1
    assert lib.scann_rbf_features_host(P(rows), 3, 4, None, 2, 1.0, P(phi)) == -1
    assert lib.scann_rbf_features_host(P(rows), 3, 4, P(Z), 2, 1.0, None) == -1
    assert lib.scann_rbf_features_host(P(rows), 3, 4, P(Z), 0, 1.0, P(phi)) == -1
    assert lib.scann_rbf_features_host(P(rows), 3, 4, P(z), 2, 1.0, P(phi)) == -1
    assert lib.scann_rbf_features_host(P(rows), 3, 4, P(Z), 2, 0.0, P(phi)) == -1 and np.all(phi == 7)
    assert lib.scann_rbf_features_host(P(rows), 0, 4, P(Z), 2, 1.0, None) == 0
    assert lib.scann_rbf_features_host(P(rows), 3, 4, P(Z), 2, 1.0, P(phi)) == 0 and np.all(phi == _hip.rbf_weight(4.0, 1.0))


# ---- header, table, library ----

def test_header_and_python_agree(hip_lib):
    import ctypes as C

    from scann import _hip

    abi_checks.declared("float scann_rbf_weight(float dist2, float gamma);",
                        "int scann_index_rbf_features(scann_handle_t* h, scann_index_t* pool, const float* landmarks /* host [m * dim] */, int32_t m, "
                        "float gamma, scann_index_t* out);",
                        "int scann_rbf_features_host(const float* rows, int64_t n, int64_t dim, const float* landmarks, int32_t m, float gamma, "
                        "float* phi /* [n * m] */);",
                        "int scann_rbf_head_batch(scann_handle_t* h, scann_dbatch_t* db, int32_t level, const float* landmarks, int32_t m, float gamma, "
                        "const float* mean /* [m] */, const float* tmean /* [K] */, const float* weights /* [K * m] */, int32_t K, "
                        "const float* components /* [mm * m] */, int32_t mm, const float* scale /* [K * mm] */, float lev0, float* y, float* ga, "
                        "float* pred /* [n * K] */, float* lev /* [n * K] */, float* phi /* [n * m] or NULL */);",
                        "#define SCANN_ABI_VERSION 1")
    abi_checks.declared("scann_rbf_weight(0, gamma) == 1.0f exactly", "lies in [0, 1]", "3 x 2^-24", "u >= 126", "NaN in all m features",
                        "0x1.6a09e6p-1,", "-0x1.f5e466p-2,", "0x1.5be298p-3,", "-0x1.41839ep-5,", "0x1.bdb696p-8,", "-0x1.ee4fd2p-11,", "0x1.c8d752p-14,",
                        "-0x1.69e51ep-17.")
    # the coefficients live in one place that the host and the device code include
    csrc = os.path.join(ROOT, "scann--material_amd", "csrc")
    holders = [f for f in sorted(os.listdir(csrc)) if "0x1.6a09e6p-1" in open(os.path.join(csrc, f), errors="replace").read()]
    assert holders == ["scann_rbf.h"], holders
    for f in ("scann_rbf.hip", "scann_rbf.cpp"):
        assert '#include "scann_rbf.h"' in open(os.path.join(csrc, f)).read()
    want = [2.0 ** -0.5 * (-np.log(2.0)) ** j / float(np.prod(np.arange(1, j + 1))) for j in range(8)]
    assert [np.float32(c) for c in want] == [np.float32(c) for c in rbf_ref.COEF] and all(float(np.float32(c)) == c for c in rbf_ref.COEF)
    P, I, L, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    sig = abi_checks.signatures({
        "scann_rbf_weight": (F, [F, F]),
        "scann_rbf_weight_array": (None, [P, L, F, P]),
        "scann_index_rbf_features": (C.c_int, [P, P, P, I, F, P]),
        "scann_rbf_features_host": (C.c_int, [P, L, L, P, I, F, P]),
        "scann_rbf_head_batch": (C.c_int, [P, P, I, P, I, F, P, P, P, I, P, I, P, F, P, P, P, P, P])})
    lib = _hip.load_library()
    assert all(hasattr(lib, n) for n in sig) and lib.scann_abi_version() == 1


def test_feature_kernel_uses_no_scratch(hip_lib):
    from scann import _hip

    kern = {n: v for n, v in abi_checks.device_kernels(_hip.LIB_PATH).items() if "rbf_" in n}
    assert len(kern) == 1 and "rbf_feature_kernel" in next(iter(kern)), sorted(kern)
    for name, (scratch, vgpr) in kern.items():
        assert scratch == 0 and vgpr <= 128, (name, scratch, vgpr)  # two workgroups per SIMD row, four per CU with 35 KB of LDS each
        for other in ("pca_", "knn_", "kcenter_", "kmeans_", "match_", "shapley_", "rollout_", "ablate_", "input_grad_kernel", "head_"):
            assert other not in name, name


# ---- the feature is worth having ----

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_kernel_head_reads_what_a_linear_head_cannot(hip_lib, seed):
    """planted(600, 128, 3): t = |u|^2 of a 3-dimensional latent u the rows are linear in.  The host route of fit_kernel_head with 64
    landmarks reaches a leave-one-out R^2 of at least 0.9, the host route of the linear fit_head at most 0.1"""
    rows, t = rbf_ref.planted(600, 128, 3, seed)
    kernel, head = rbf_ref.host_fit(rows, t, landmarks=64)
    linear, _ = head_ref.host_fit(rows, t)
    print("seed %d: kernel head loo_r2 %.4f at h = %.3g (covering radius %.3g; path %s), linear head loo_r2 %.4f" % (
        seed, kernel["loo_r2"][0], kernel["bandwidth"], kernel["covering_radius"], np.round(kernel["bandwidth_path"]["loo_r2"][:, 0], 4), linear["loo_r2"][0]))
    assert kernel["loo_r2"][0] >= 0.9
    assert linear["loo_r2"][0] <= 0.1
    assert head.m == 64 and head.k == 1 and head.dim == 128 and kernel["weights"].shape == (1, 64)


# ---- the result, the choice, save / load ----

def test_result_keys_and_the_choice_of_the_bandwidth(hip_lib):
    from scann import _hip

    rows, t = rbf_ref.planted(300, 8, 3, 5)
    T = np.stack([t, -2 * t + 1, np.full_like(t, 4.5)], axis=1)  # the last target has no variance: it is skipped in the score
    T[17, 0] = np.nan  # unlabelled
    ids, atoms = np.arange(300) * 3 + 1, np.arange(300, dtype=np.int32) % 7
    res, head = rbf_ref.host_fit(rows, T, landmarks=32, names=["a", "b", "c"], ids=ids, atoms=atoms)
    fit_keys = ["l2", "loo_rmse", "loo_mae", "loo_r2", "fit_rmse", "dof", "sigma2", "n_rows", "loo_prediction", "weights", "names", "path"]
    assert sorted(res) == sorted(fit_keys + ["bandwidth", "landmark_position", "landmark_id", "landmark_atom", "covering_radius", "bandwidth_path"])
    assert res["n_rows"] == 299 and res["weights"].shape == (3, 32) and np.isnan(res["loo_prediction"][17]).all()
    sel = _hip.kcenter_host(rows, None, 33)
    assert np.array_equal(res["landmark_position"], sel["position"][:32]) and res["covering_radius"] == float(np.sqrt(np.float64(sel["radius2"][32])))
    assert np.array_equal(res["landmark_id"], ids[sel["position"][:32]]) and np.array_equal(res["landmark_atom"], atoms[sel["position"][:32]])
    path = res["bandwidth_path"]
    assert np.array_equal(path["bandwidth"], np.sqrt(np.float64(sel["radius2"][32]) * np.array(rbf_ref.FACTORS)))
    assert path["loo_rmse"].shape == path["loo_r2"].shape == (6, 3)
    with np.errstate(invalid="ignore"):
        score = (1.0 - path["loo_r2"][:, :2]).sum(1)
    g = int(np.argmin(score))
    assert res["bandwidth"] == path["bandwidth"][g] and head.gamma == _hip.rbf_gamma(res["bandwidth"])
    assert abs(head.bandwidth / res["bandwidth"] - 1) < 1e-6
    pca_ref.same(res["loo_r2"][:2], path["loo_r2"][g, :2], "the winner's row of the path")
    # explicit bandwidths: one, and a tie (the same h twice is one h; two h with equal scores cannot be planted, so the rule is read
    # from the order: the larger h is tried first and a later one must be strictly better)
    one, _ = rbf_ref.host_fit(rows, T, landmarks=32, bandwidth=res["bandwidth"])
    pca_ref.same(one["loo_prediction"], res["loo_prediction"], "one explicit bandwidth")
    # explicit positions
    pos = sel["position"][:32][::-1].copy()
    by_pos, head_p = rbf_ref.host_fit(rows, T, landmarks=pos, bandwidth=res["bandwidth"])
    assert np.array_equal(by_pos["landmark_position"], pos) and by_pos["covering_radius"] == res["covering_radius"]
    pca_ref.same(head_p.landmarks, head.landmarks[::-1], "landmarks by position")


def test_ties_go_to_the_larger_bandwidth():
    from scann.models import latent_index as li

    t = np.float32([[0.0], [1.0], [2.0]])
    calls = []

    def run(gamma):
        calls.append(gamma)
        fit = {"n": 3, "tvar": np.array([1.0]), "l2": np.array([0.5]), "beta": np.zeros((1, 1, 2)), "V": np.eye(2), "mean": np.zeros(2, np.float32),
               "tmean": np.zeros(1, np.float32), "components": np.eye(2, dtype=np.float32), "scale": np.ones((1, 2), np.float32), "lev0": 1 / 3}
        loo = {"sse": np.array([[1.0]]), "sae": np.array([[1.0]]), "sse_fit": np.array([[1.0]]), "dof": np.array([1.0]), "resid": np.zeros((3, 1), np.float32)}
        return fit, loo, np.zeros(1, np.int32)

    res, head = li.kernel_head_result(run, np.array([1.0, 4.0, 2.0]), np.zeros((2, 5), np.float32), 1.0, np.array([0, 1]), np.arange(3), np.zeros(3, np.int32),
                                      t, ["x"], "structure", 5)
    assert res["bandwidth"] == 4.0 and len(calls) == 3 and np.array_equal(res["bandwidth_path"]["bandwidth"], [1.0, 4.0, 2.0])


def test_kernel_head_save_and_load(hip_lib, tmp_path):
    from scann.models import LatentKernelHead
    from scann.models.scann_model import HipModel  # noqa: F401  (the class whose config a head is checked against)

    rows, t = rbf_ref.planted(200, 128, 3, 3)
    _, head = rbf_ref.host_fit(rows, t, landmarks=16, names=["gap"])

    class Model:
        config = so.default_config("qm9")

    path = str(tmp_path / "kh.npz")
    head.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(["landmarks", "gamma", "mean", "tmean", "weights", "components", "scale", "lev0", "sigma2", "l2", "level", "dim", "names"])
    back = LatentKernelHead.load(Model, path)
    pca_ref.same(back.landmarks, head.landmarks, "landmarks")
    assert back.gamma == head.gamma and back.level == "structure" and back.dim == 128 and back.names == ["gap"] and back.head.lev0 == head.head.lev0
    for key in rbf_ref.HEAD_ARRAYS:
        pca_ref.same(getattr(back.head, key), getattr(head.head, key), key)
    head.check_model(Model)
    narrow = so.default_config("qm9")
    narrow["model"]["dense_out"] = 64

    class Other:
        config = narrow

    with pytest.raises(ValueError, match="does not fit"):
        LatentKernelHead.load(Other, path)
    with pytest.raises(ValueError, match="does not fit"):
        head.check_model(Other)
    # finish: std in fp64 on the host, support the largest feature
    phi = np.float32([[0.1, 0.9] + [0.0] * 14, [0.0] * 16])
    out = head.finish(np.zeros((2, 1), np.float32), np.float32([[0.0], [3.0]]), phi)
    assert np.array_equal(out["support"], np.float32([0.9, 0.0])) and out["std"][1, 0] == np.float32(np.sqrt(head.head.sigma2[0] * 4.0))
    assert out["std"][0, 0] == np.float32(np.sqrt(head.head.sigma2[0]))


def test_python_layer_raises_before_any_upload(hip_lib):
    from scann import _hip
    from scann.models import LatentHead, LatentKernelHead
    from scann.models import latent_index as li

    for bad in (0, 1025, -3, True, 2.5, "many", np.array([0.5, 1.5]), np.array([[0, 1]]), np.array([0, 0]), np.array([0, 99]), np.array([], np.int64)):
        with pytest.raises(ValueError, match="landmarks"):
            li.kernel_landmarks_arg(bad, 50)
    assert li.kernel_landmarks_arg(7, 50) == (7, None) and li.kernel_landmarks_arg(np.int64(1024), 5)[0] == 1024
    m, pos = li.kernel_landmarks_arg([3, 1, 2], 50)
    assert m == 3 and pos.dtype == np.int64 and pos.tolist() == [3, 1, 2]
    for bad in ("cv", 0.0, -1.0, np.nan, np.inf, [1.0] * 9, [], [[1.0]], True, None, [1.0, -2.0], 1e-30):
        with pytest.raises(ValueError, match="bandwidth"):
            li.kernel_bandwidth_arg(bad)
    assert li.kernel_bandwidth_arg("loo") is None and li.kernel_bandwidth_arg(2).tolist() == [2.0] and len(li.kernel_bandwidth_arg([1, 2, 3, 4, 5, 6, 7, 8])) == 8
    for bad_r2 in (0.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="covering radius"):
            li.kernel_bandwidths("loo", bad_r2)
    assert li.kernel_bandwidths(3.0, 0.0).tolist() == [3.0]
    assert np.array_equal(li.kernel_bandwidths("loo", 4.0), 2.0 * np.sqrt(np.array(rbf_ref.FACTORS)))
    inner = LatentHead(np.zeros(4, np.float32), np.zeros(1, np.float32), np.zeros((1, 4), np.float32), np.eye(4, dtype=np.float32)[:2],
                       np.ones((1, 2), np.float32), 0.1, np.ones(1), np.ones(1), "structure")
    Z = np.ones((4, 9), np.float32)
    assert LatentKernelHead(Z, 0.5, inner, "structure").dim == 9
    for kw in (dict(landmarks=np.ones((5, 9), np.float32)), dict(gamma=0.0), dict(gamma=np.nan), dict(head="h"), dict(level="bond"), dict(dim=8),
               dict(names=["a", "b"]), dict(landmarks=np.full((4, 9), np.nan, np.float32))):
        a = dict(landmarks=Z, gamma=0.5, head=inner, level="structure", dim=None, names=None)
        a.update(kw)
        with pytest.raises(ValueError):
            LatentKernelHead(**a)
    with pytest.raises(ValueError, match="landmark 2, column 1"):
        z = Z.copy()
        z[2, 1] = -np.inf
        _hip.check_rbf_args(z, 1.0)


def test_cli_takes_the_kernel_head_flags(tmp_path):
    spec = importlib.util.spec_from_file_location("predict_model_cli", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    np.save(tmp_path / "t.npy", np.zeros((5, 2), np.float32))
    a = cli.parser().parse_args(["some_dir", "--fit-kernel-head", str(tmp_path / "t.npy"), "--landmarks", "3", "--kernel-head-level", "atom",
                                 "--kernel-head-out", "kh.npz"])
    assert (a.fit_kernel_head, a.landmarks, a.kernel_head_level, a.kernel_head_out, a.kernel_head) == (str(tmp_path / "t.npy"), 3, "atom", "kh.npz", "")
    assert cli.check_kernel_head_flags(a).shape == (5, 2) and cli.check_kernel_head_flags(a).dtype == np.float32
    d = cli.parser().parse_args(["some_dir"])
    assert (d.fit_kernel_head, d.landmarks, d.kernel_head_level, d.kernel_head_out, d.kernel_head) == ("", 256, "structure", "", "")
    assert cli.check_kernel_head_flags(d) is None
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--kernel-head-level", "bond"])
    np.save(tmp_path / "wide.npy", np.zeros((5, 17), np.float32))
    open(tmp_path / "kh.npz", "wb").close()
    t = str(tmp_path / "t.npy")
    # bad arguments end before the model's folder -- which does not exist -- is read
    for bad in (["--fit-kernel-head", str(tmp_path / "none.npy")], ["--fit-kernel-head", str(tmp_path / "wide.npy")], ["--kernel-head", str(tmp_path / "none.npz")],
                ["--kernel-head-out", "x.npz"], ["--fit-kernel-head", t, "--kernel-head", str(tmp_path / "kh.npz")],
                ["--fit-kernel-head", t, "--landmarks", "0"], ["--fit-kernel-head", t, "--landmarks", "1025"], ["--fit-kernel-head", t, "--landmarks", "5"]):
        with pytest.raises(SystemExit):
            cli.main(cli.parser().parse_args([str(tmp_path / "no_such_model")] + bad))
    src = open(spec.origin).read()
    assert "kernel_head_{}.pickle" in src and "fit_kernel_head" in src and "predict_kernel_head" in src
