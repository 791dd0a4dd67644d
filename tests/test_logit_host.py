"""Host tests of the classification head on a latent index (scann_index_logit_pass / scann_logit_head_batch, the twin
scann_logit_pass_host, LatentIndex.fit_class_head, LatentClassHead, HipModel.fit_class_head / predict_class_head): the twin against the
NumPy restatement of the definition (tests/logit_ref.py), bit for bit, either side of a block and of a span, with more than 64 logit
columns, folds, planted NaN / inf components and unlabelled rows, and under threading; facts that hold whatever the twin does; the
argument checks; the optimiser on the host route against an fp64 Newton fit; LatentClassHead's save / load; header, ctypes table and
library agree; predict_model.py takes --fit-class-head / --class-head.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import abi_checks
import logit_ref
import pca_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, dim, C, M, F): N either side of a block (128) and of a span (4,096); dim 1, 3, 130; C 2, 3, 16; M C = 80 > 64; F 0, 2, 4; the last
# is above the twin's threshold for threading over the spans
CASES = [(1, 1, 2, 1, 0), (127, 3, 3, 2, 2), (129, 130, 16, 5, 4), (4095, 3, 2, 3, 4), (4097, 1, 3, 2, 2), (4097, 130, 3, 4, 0),
         (9000, 64, 2, 20, 4)]


@pytest.mark.parametrize("case", CASES, ids=["N%d_d%d_C%d_M%d_F%d" % c for c in CASES])
def test_twin_equals_the_definition(hip_lib, case):
    from scann import _hip

    rows, lab, mean, U, fold, F, pof = logit_ref.random_pass(*case, seed=case[0])
    got = _hip.logit_pass_host(rows, lab, mean, U, fold, F, pof)
    want = logit_ref.logit_pass(rows, lab, mean, U, fold, F, pof)
    logit_ref.same_pass(got, want, str(case))
    N = case[0]
    if N >= 100:
        assert 0 < got["n"] < N and np.isnan(got["prob"]).any() and np.isfinite(got["prob"]).any()
        assert (got["stats"][:, 0, 0] + got["stats"][:, 1, 0] == got["n"]).all()
    # without prob nothing else changes
    logit_ref.same_pass(_hip.logit_pass_host(rows, lab, mean, U, fold, F), {k: v for k, v in want.items() if k != "prob"}, "no prob")


def test_a_fold_whose_training_rows_lack_a_class(hip_lib):
    """class 2 lives at even positions only: the model that holds out fold 0 of 2 never trains on it"""
    from scann import _hip

    rows, lab, mean, U, _, _, _ = logit_ref.random_pass(300, 5, 3, 3, 0, seed=3, planted=False)
    lab = (np.arange(300) % 2).astype(np.int32)
    lab[::4] = 2
    fold, pof = np.array([0, 1, -1], np.int32), np.array([0, 1], np.int32)
    got = _hip.logit_pass_host(rows, lab, mean, U, fold, 2, pof)
    logit_ref.same_pass(got, logit_ref.logit_pass(rows, lab, mean, U, fold, 2, pof), "a class missing")
    assert got["stats"][0, 0, 0] == 150 and got["stats"][0, 1, 0] == 150 and np.isfinite(got["grad"]).all()
    # the missing class's gradient is minus the sum of its probabilities' terms: its intercept entry is negative
    assert got["grad"][0, 2, 5] < 0 and got["grad"][1, 2, 5] != got["grad"][0, 2, 5]


def test_all_rows_unlabelled_gives_zeros(hip_lib):
    from scann import _hip

    rows, lab, mean, U, fold, F, pof = logit_ref.random_pass(200, 4, 3, 3, 2, seed=5)
    lab[:] = -1
    got = _hip.logit_pass_host(rows, lab, mean, U, fold, F, pof)
    assert got["n"] == 0 and not got["grad"].any() and not got["stats"].any() and np.isnan(got["prob"]).all()
    empty = _hip.logit_pass_host(np.zeros((0, 4), np.float32), np.zeros(0, np.int32), mean, U, fold, F, pof)
    assert empty["n"] == 0 and not empty["grad"].any() and not empty["stats"].any() and empty["prob"].shape == (0, 3)


@pytest.mark.parametrize("C", [2, 4, 16])
def test_at_zero_weights_every_probability_is_one_over_c(hip_lib, C):
    """independent of the twin: at U = 0 every p_k is (float)(1.0f / C), a power of two here, so every sum is exact"""
    from scann import _hip

    N, dim, F = 1000, 7, 4
    rows, lab, mean, _, _, _, _ = logit_ref.random_pass(N, dim, C, 1, 0, seed=C, planted=False)
    lab[::7] = -1
    U = np.zeros((F + 1, C, dim + 1), np.float32)
    fold = np.array(list(range(F)) + [-1], np.int32)
    got = _hip.logit_pass_host(rows, lab, mean, U, fold, F, np.arange(F, dtype=np.int32))
    p = np.float32(1.0) / np.float32(C)
    counted = lab >= 0
    assert got["n"] == counted.sum() and (got["prob"][counted] == p).all() and np.isnan(got["prob"][~counted]).all()
    pos = np.arange(N) % F
    for j, f in enumerate(fold):
        train = counted & (pos != f)
        count = np.bincount(lab[train], minlength=C).astype(np.float64)
        assert np.array_equal(got["grad"][j, :, dim], count - train.sum() * float(p)), j
        assert got["stats"][j, 0, 0] == train.sum() and got["stats"][j, 0, 1] == count[0]  # all logits equal: class 0 is "the largest"
        held = counted & (pos == f)
        assert got["stats"][j, 1, 0] == held.sum() and got["stats"][j, 1, 1] == (lab[held] == 0).sum()
        b = float(np.float32(C - 1) * p * p + (np.float32(1) - p) * (np.float32(1) - p))  # exact: powers of two
        assert got["stats"][j, 0, 2] == train.sum() * b


def test_header_and_python_agree(hip_lib):
    import ctypes as C

    from scann import _hip

    abi_checks.declared("int scann_index_logit_pass(scann_handle_t* h, scann_index_t* pool, const int32_t* labels /* [N] */, int32_t C, "
                        "const float* mean /* [dim] */, const float* weights /* [M][C][dim + 1] */, int32_t M, const int32_t* fold /* [M] */, int32_t F, "
                        "const int32_t* prob_of_fold /* [max(F,1)] or NULL */, int64_t* n_used, double* grad /* [M][C][dim + 1] */, "
                        "double* stats /* [M][2][3] */, float* prob /* [N * C] or NULL */);",
                        "int scann_logit_pass_host(const float* rows, int64_t n, int64_t dim, const int32_t* labels, int32_t C, const float* mean, "
                        "const float* weights, int32_t M, const int32_t* fold, int32_t F, const int32_t* prob_of_fold, int64_t* n_used, double* grad, "
                        "double* stats, float* prob);",
                        "int scann_logit_head_batch(scann_handle_t* h, scann_dbatch_t* db, int32_t level, const float* mean /* [dim] */, "
                        "const float* weights /* [C][dim + 1] */, int32_t C, float* y, float* ga, float* prob /* [n * C] */);",
                        "#define SCANN_LOGIT_MAX_CLASSES 16", "#define SCANN_LOGIT_MAX_MODELS 64")
    assert _hip.LOGIT_MAX_CLASSES == 16 and _hip.LOGIT_MAX_MODELS == 64
    P, I, L = C.c_void_p, C.c_int32, C.c_int64
    sig = abi_checks.signatures({
        "scann_index_logit_pass": (C.c_int, [P, P, P, I, P, P, I, P, I, P, P, P, P, P]),
        "scann_logit_pass_host": (C.c_int, [P, L, L, P, I, P, P, I, P, I, P, P, P, P, P]),
        "scann_logit_head_batch": (C.c_int, [P, P, I, P, P, I, P, P, P])})
    for name in sig:
        assert hasattr(hip_lib, name), name


def test_null_and_bad_arguments_are_errors_not_crashes(hip_lib):
    import ctypes as C

    from scann import _hip

    P = _hip._ptr
    rows, lab, mean, U, fold, F, pof = logit_ref.random_pass(6, 3, 3, 3, 2, seed=0, planted=False)
    n = C.c_int64(0)
    grad, stats, prob = np.zeros((3, 3, 4)), np.zeros((3, 2, 3)), np.zeros((6, 3), np.float32)

    def call(rows=rows, N=6, dim=3, lab=lab, Cn=3, mean=mean, U=U, M=3, fold=fold, F=2, pof=pof, n=n, grad=grad, stats=stats, prob=prob):
        return hip_lib.scann_logit_pass_host(P(rows), N, dim, P(lab), Cn, P(mean), P(U), M, P(fold), F, P(pof), None if n is None else C.byref(n),
                                             P(grad), P(stats), P(prob))

    assert call() == 0 and n.value == 6
    assert call(prob=None, pof=None) == 0
    bad_lab, low_lab = lab.copy(), lab.copy()
    bad_lab[4], low_lab[0] = 3, -2
    for bad in (dict(rows=None), dict(lab=None), dict(mean=None), dict(U=None), dict(fold=None), dict(n=None), dict(grad=None), dict(stats=None),
                dict(pof=None), dict(N=-1), dict(dim=0), dict(Cn=1), dict(Cn=17), dict(M=0), dict(M=65), dict(F=1), dict(F=17), dict(F=-1),
                dict(fold=np.array([0, 2, -1], np.int32)), dict(fold=np.array([-2, 0, 1], np.int32)), dict(F=0),
                dict(pof=np.array([0, 3], np.int32)), dict(pof=np.array([-2, 0], np.int32)), dict(mean=np.float32([0, np.nan, 0])),
                dict(U=np.full_like(U, np.inf)), dict(lab=bad_lab), dict(lab=low_lab)):
        assert call(**bad) == -1, bad
    assert call(N=0, rows=None, lab=None) == 0 and n.value == 0 and not grad.any() and not stats.any()  # an empty pool: zeros
    assert hip_lib.scann_index_logit_pass(None, None, P(lab), 3, P(mean), P(U), 3, P(fold), 2, P(pof), C.byref(n), P(grad), P(stats), P(prob)) == -1
    assert hip_lib.scann_logit_head_batch(None, None, 2, P(mean), P(U), 3, None, None, P(prob)) == -1
    # the Python checks name the argument
    good = dict(mean=mean, weights=U, fold=fold, folds=2, prob_of_fold=pof, dim=3)
    out = _hip.check_logit_args(**good)
    assert [a.dtype for a in (out[0], out[1], out[2], out[4])] == [np.float32, np.float32, np.int32, np.int32] and out[3] == 2
    for kw, word in ((dict(mean=mean[:2]), "mean"), (dict(weights=U[:, :, :3]), "weights"), (dict(weights=U[:, :1]), "weights"),
                     (dict(weights=np.zeros((65, 3, 4))), "weights"), (dict(weights=np.zeros((1, 17, 4))), "weights"), (dict(weights="x"), "weights"),
                     (dict(mean=np.float32([0, np.inf, 0])), "mean holds a non-finite"), (dict(weights=np.full_like(U, np.nan)), "weights holds a non-finite"),
                     (dict(folds=1), "folds"), (dict(folds=17), "folds"), (dict(folds=2.0), "folds"), (dict(fold=[0, 2, -1]), "fold"),
                     (dict(fold=[0, 1]), "fold"), (dict(fold=[0.5, 0, 1]), "fold"), (dict(prob_of_fold=[0, 3]), "prob_of_fold"),
                     (dict(prob_of_fold=[0]), "prob_of_fold"), (dict(folds=0), "fold")):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            _hip.check_logit_args(**args)
    assert _hip.check_class_labels([0, -1, 2], 3, 3).dtype == np.int32
    for bad, C_, word in (([0, 3, 1], 3, r"labels\[1\] = 3"), ([0, -2], 2, r"labels\[1\] = -2"), ([0.0, 1.0], 2, "labels"), ([[0, 1]], 2, "labels"),
                          ([0, 1], 1, "C must"), ([0, 1], 17, "C must"), ([0, 1, 1], 2, "labels hold 3 rows")):
        with pytest.raises(ValueError, match=word):
            _hip.check_class_labels(bad, C_, 2 if "hold" in word else None)
    with pytest.raises(ValueError, match="rows of shape"):
        _hip.logit_pass_host(np.zeros(3), lab, mean, U)


# ---- the optimiser, with the host twin as the pass ----

def test_fit_separates_the_planted_classes(hip_lib):
    """3 classes on 600 x 16 rows, centres 8 e_k and unit noise: pairwise distances of 11.3 sigma.  The fp64 Newton fit of the same
    objective reaches cross-validated accuracy 1.0 -- the condition the inputs are chosen for --, and so does the product's host route"""
    rows, lab = logit_ref.planted(600, 16, 3, 8.0, seed=0)
    s0 = float(np.linalg.eigvalsh(np.cov(rows.astype(np.float64).T))[-1])
    assert logit_ref.newton_cv_accuracy(rows, lab, 3, 1e-3 * s0, 4) == 1.0
    res, head = logit_ref.host_fit(rows, lab)
    print("planted: l2 %.4g cv_accuracy %.4f cv_brier %.3g cv_log_loss %.3g iterations %d passes %d %s" % (
        res["l2"], res["cv_accuracy"], res["cv_brier"], res["cv_log_loss"], res["iterations"], res["passes"], res["stopped"]))
    assert res["cv_accuracy"] == 1.0 and res["fit_accuracy"] == 1.0 and res["converged"] and res["n_rows"] == 600
    assert np.array_equal(res["cv_confusion"], np.diag(np.bincount(lab))) and np.array_equal(res["class_count"], np.bincount(lab))
    assert res["cv_probability"].shape == (600, 3) and res["cv_probability"].dtype == np.float32 and res["weights"].shape == (3, 16)
    assert np.array_equal(np.argmax(res["cv_probability"], axis=1), lab) and res["cv_log_loss"] < 0.01 and res["cv_brier"] < 1e-3
    assert list(res["classes"]) == [0, 1, 2] and len(res["path"]["l2"]) == len(res["path"]["cv_brier"]) <= 6
    assert res["l2"] == res["path"]["l2"][int(np.argmin(res["path"]["cv_brier"]))]  # the least held-out Brier sum wins
    # the head's own arithmetic on new rows of the same classes
    new_rows, new_lab = logit_ref.planted(90, 16, 3, 8.0, seed=1)
    from scann import _hip
    prob = _hip.logit_pass_host(new_rows, np.zeros(90, np.int32), head.mean, head.weights[None], None, 0, [0])["prob"]
    out = head.finish(prob)
    assert np.array_equal(out["label"], new_lab) and (out["confidence"] > 0.99).all() and (out["entropy"] < 0.05).all() and (out["entropy"] >= 0).all()


OVERLAP_GAP = 7.640e-10  # per row, measured by the fp64 yardstick logit_ref.lbfgs64_gap on this case (profiles/logit_fit.txt)


def test_fit_reaches_the_optimum_of_an_overlapping_case(hip_lib):
    """2,000 x 16, 3 classes 1.5 sigma apart per axis, l2 = 1e-3 s_0, tol 1e-5: the objective at the returned weights, evaluated in fp64
    NumPy, is no larger than at W = 0 and lies above the fp64 Newton optimum by at most 4 x the per-row gap OVERLAP_GAP -- what an
    fp64 L-BFGS with exact gradients leaves at the same stopping rule (logit_ref.lbfgs64_gap; the table is profiles/logit_fit.txt); fp32
    rounding in the pass moves the figure by about that much between seeds.  Measured for the host route: 7.635e-10."""
    from scann import _hip

    rows, lab = logit_ref.planted(2000, 16, 3, 1.5, seed=0)
    mo = _hip.moments_host(rows)
    s0 = _hip.sym_eig(mo["cov"])[0][0]
    l2 = 1e-3 * s0
    fit = logit_ref.host_fit(rows, lab, l2=l2, folds=0, max_iter=200, tol=1e-5, raw=True)
    f = logit_ref.objective(rows, lab, fit["U"].astype(np.float64), l2, mo["mean"])
    f0 = logit_ref.objective(rows, lab, np.zeros((3, 17)), l2, mo["mean"])
    f_star = logit_ref.objective(rows, lab, logit_ref.newton_fit(rows, lab, 3, l2, mo["mean"]), l2, mo["mean"])
    gap = (f - f_star) / 2000
    print("overlapping: f(0)/n %.6f f/n %.6f f*/n %.6f gap/row %.3e iterations %d passes %d %s" % (
        f0 / 2000, f / 2000, f_star / 2000, gap, fit["iterations"], fit["passes"], fit["stopped"]))
    assert fit["stopped"] == "converged" and fit["passes"] <= fit["iterations"] + 3
    assert f <= f0
    assert -1e-12 <= gap <= 4 * OVERLAP_GAP, gap


def test_fit_arguments_raise_value_errors(hip_lib):
    from scann.models import latent_index as li

    rows, lab = logit_ref.planted(40, 4, 3, 4.0, seed=2)
    lab7 = lab * 7 + 3  # classes 3, 10, 17
    idx, classes = li.class_labels_arg(lab7, None, 40)
    assert list(classes) == [3, 10, 17] and np.array_equal(idx, lab) and idx.dtype == np.int32
    idx, classes = li.class_labels_arg(np.where(lab == 1, -1, lab7), [17, 3], 40)
    assert list(classes) == [17, 3] and np.array_equal(idx, np.where(lab == 1, -1, np.where(lab == 2, 0, 1)))
    for kw, word in ((dict(labels=lab[:5]), "labels hold 5 rows"), (dict(labels=lab.astype(np.float32)), "labels must be an integer"),
                     (dict(labels=np.zeros(40, np.int32)), "2 .. 16 classes"), (dict(labels=np.arange(40)), "2 .. 16 classes"),
                     (dict(classes=[0, 1]), r"labels\[\d+\] = 2 is neither"), (dict(classes=[0, 0, 1]), "distinct"),
                     (dict(classes=[0, -1, 1]), "distinct"), (dict(classes=[0, 1, 2, 3]), "class 3 .label 3. has no row"),
                     (dict(l2="loo"), "l2"), (dict(l2=-1.0), "l2"), (dict(l2=[1.0] * 9), "l2"), (dict(l2=np.nan), "l2"), (dict(folds=1), "folds"),
                     (dict(folds=17), "folds"), (dict(folds=0), "folds=0"), (dict(folds=0, l2=[1.0, 2.0]), "folds=0"), (dict(folds=16, labels=np.where(np.arange(40) < 12, -1, lab)), "at least 32 rows"),
                     (dict(max_iter=0), "max_iter"), (dict(max_iter=2.5), "max_iter"), (dict(tol=0), "tol"), (dict(tol="x"), "tol")):
        args = dict(labels=lab)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            logit_ref.host_fit(rows, **args)
    # a class whose rows all hold a non-finite component: found by the first pass
    broken = rows.copy()
    broken[lab == 2, 1] = np.nan
    with pytest.raises(ValueError, match="class 2 .label 2. has no row that counts"):
        logit_ref.host_fit(broken, lab, l2=1.0, folds=0)
    # one strength without folds: the cv entries are NaN, nothing else is missing
    res, head = logit_ref.host_fit(rows, lab, l2=0.5, folds=0)
    assert np.isnan(res["cv_accuracy"]) and np.isnan(res["cv_log_loss"]) and np.isnan(res["cv_probability"]).all() and res["l2"] == 0.5
    assert res["fit_accuracy"] > 0.9 and head.c == 3 and head.weights.shape == (3, 5)


def test_class_head_saves_loads_and_checks(hip_lib, tmp_path):
    from scann.models import LatentClassHead, LatentHead

    class Model:
        config = {"model": {"dense_out": 4, "global_dim": 9}}

    rng = np.random.default_rng(0)
    head = LatentClassHead(rng.standard_normal(4), rng.standard_normal((3, 5)), [5, 2, 9], 0.25, "structure", 4)
    head.check_model(Model)
    head.save(str(tmp_path / "ch.npz"))
    back = LatentClassHead.load(Model, str(tmp_path / "ch.npz"))
    for name in ("mean", "weights", "classes"):
        pca_ref.same(getattr(back, name), getattr(head, name), name)
    assert (back.l2, back.level, back.dim, back.c) == (0.25, "structure", 4, 3)
    out = head.finish(np.float32([[0.5, 0.5, 0.0], [0.0, 0.0, 1.0], [0.2, 0.7, 0.1]]))
    assert list(out["label"]) == [5, 9, 2] and list(out["confidence"]) == [np.float32(0.5), 1.0, np.float32(0.7)]
    assert abs(out["entropy"][0] - np.log(2)) < 1e-6 and out["entropy"][1] == 0 and out["entropy"].dtype == np.float32
    for args, word in (((np.zeros(4), np.zeros((3, 4)), [0, 1, 2], 1.0, "structure", 4), "weights"),
                       ((np.zeros(4), np.zeros((3, 5)), [0, 1], 1.0, "structure", 4), "classes"),
                       ((np.zeros(4), np.zeros((3, 5)), [0, 1, 1], 1.0, "structure", 4), "classes"),
                       ((np.zeros(4), np.zeros((3, 5)), [0, 1, 2], 1.0, "bond", 4), "level"),
                       ((np.zeros(5), np.zeros((3, 6)), [0, 1, 2], 1.0, "structure", 4), "mean"),
                       ((np.zeros(4), np.full((3, 5), np.nan), [0, 1, 2], 1.0, "structure", 4), "non-finite"),
                       ((np.zeros(4), np.zeros((1, 5)), [0], 1.0, "structure", 4), "weights")):
        with pytest.raises(ValueError, match=word):
            LatentClassHead(*args)
    atom = LatentClassHead(np.zeros(4), np.zeros((2, 5)), [0, 1], 1.0, "atom", 4)
    with pytest.raises(ValueError, match="does not fit"):
        atom.check_model(Model)
    atom.save(str(tmp_path / "atom.npz"))
    with pytest.raises(ValueError, match="does not fit"):
        LatentClassHead.load(Model, str(tmp_path / "atom.npz"))
    np.savez(open(tmp_path / "other.npz", "wb"), mean=np.zeros(4))
    with pytest.raises(ValueError, match="not a saved LatentClassHead"):
        LatentClassHead.load(Model, str(tmp_path / "other.npz"))
    assert LatentHead is not LatentClassHead


def test_cli_takes_the_class_head_flags(tmp_path):
    spec = importlib.util.spec_from_file_location("predict_model_cli", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    np.save(tmp_path / "l.npy", np.array([0, 1, 1, -1, 0, 2]))
    a = cli.parser().parse_args(["some_dir", "--fit-class-head", str(tmp_path / "l.npy"), "--class-head-level", "atom", "--class-head-out", "ch.npz"])
    assert (a.fit_class_head, a.class_head_level, a.class_head_out, a.class_head) == (str(tmp_path / "l.npy"), "atom", "ch.npz", "")
    assert cli.check_class_head_flags(a).shape == (6,) and cli.check_class_head_flags(a).dtype == np.int64
    d = cli.parser().parse_args(["some_dir"])
    assert (d.fit_class_head, d.class_head_level, d.class_head_out, d.class_head) == ("", "structure", "", "") and cli.check_class_head_flags(d) is None
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--class-head-level", "bond"])
    np.save(tmp_path / "float.npy", np.zeros(5, np.float32))
    np.save(tmp_path / "one.npy", np.zeros(5, np.int64))
    np.save(tmp_path / "wide.npy", np.zeros((5, 2), np.int64))
    np.save(tmp_path / "many.npy", np.arange(40))
    open(tmp_path / "ch.npz", "wb").close()
    # bad arguments end before the model's folder -- which does not exist -- is read
    for bad in (["--fit-class-head", str(tmp_path / "none.npy")], ["--fit-class-head", str(tmp_path / "float.npy")],
                ["--fit-class-head", str(tmp_path / "one.npy")], ["--fit-class-head", str(tmp_path / "wide.npy")],
                ["--fit-class-head", str(tmp_path / "many.npy")], ["--class-head", str(tmp_path / "none.npz")], ["--class-head-out", "x.npz"],
                ["--fit-class-head", str(tmp_path / "l.npy"), "--class-head", str(tmp_path / "ch.npz")]):
        with pytest.raises(SystemExit):
            cli.main(cli.parser().parse_args([str(tmp_path / "no_such_model")] + bad))
    src = open(spec.origin).read()
    assert "class_head_{}.pickle" in src and "fit_class_head" in src and "predict_class_head" in src
