"""Host tests of the prototypes and criticisms of a latent index (scann_index_prototypes / scann_index_criticisms, the twins
scann_prototypes_host / scann_criticisms_host, LatentIndex.prototypes, LatentIndex.mmd's host half, LatentPrototypes): the twins against
the restatement of the definition from the full term matrix (tests/proto_ref.py) in every integer, with the certificate that each pick
is the exact argmax of the greedy objective; duplicates, coincident rows, non-finite rows, the empty pool; the range cap and the weight
range; independence of the thread count; the planted clusters end to end; the MMD of two samples against its exact rational; header,
ctypes table and library agree; LatentPrototypes' round trip; the host route of LatentIndex.prototypes; the CLI flags.  No GPU."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import abi_checks
import kcenter_ref
import peaks_cpu
import peaks_ref
import proto_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED_SEED = 0  # checked with the twin below before it was committed
ONE = 2 ** 30


def same_as_reference(rows, m, gamma, dist2, crit=4, what=""):
    """the twins equal the restated definition in every integer, in both witness modes; returns the twin's dict"""
    from scann import _hip
    from scann.models import latent_index as li

    got = _hip.prototypes_host(rows, m, gamma)
    ref = proto_ref.prototypes(rows, m, dist2, _hip.rbf_weight, gamma)
    c = got["count"]
    assert c == len(ref["position"]) == min(m, ref["n"]), what
    assert got["position"][:c].tolist() == ref["position"] and got["score"][:c].tolist() == ref["score"], what
    assert got["b_at_pick"][:c].tolist() == ref["b_at_pick"] and got["A"].tolist() == ref["A"] and got["B"].tolist() == ref["B"], what
    assert (got["position"][c:] == -1).all() and (got["score"][c:] == 0).all() and (got["b_at_pick"][c:] == 0).all(), what
    assert got["position"].dtype == np.int32 and all(got[k].dtype == np.int64 for k in ("score", "b_at_pick", "A", "B"))
    el = [i for i in range(len(rows)) if ref["A"][i] >= 0]
    if c:
        curve = proto_ref.mmd_curve(ref["T"], el, ref["position"])
        mmd2 = li.prototypes_mmd2(got["A"], got["position"][:c], got["b_at_pick"][:c])
        assert np.allclose(mmd2, [float(x) for x in curve], rtol=1e-12, atol=1e-18), what
        assert all(x >= 0 for x in curve)
    for witness in ("under", "both") if c else ():
        W, weight = proto_ref.weights(ref["A"], ref["B"], c, witness)
        W2, wit, weight2 = li.prototypes_weights(got["A"], got["B"], c, witness)
        assert W2.tolist() == W and weight2.tolist() == weight and max(weight, default=0) < 2 ** 31, what
        assert all(wit[i] == W[i] / (ref["n"] * c * ONE) for i in el) and np.isnan(wit[[i for i in range(len(rows)) if i not in el]]).all()
        gc = _hip.criticisms_host(rows, weight2, got["position"][:c], crit, gamma)
        rc = proto_ref.criticisms(rows, weight, ref["position"], crit, dist2, _hip.rbf_weight, gamma)
        k = gc["count"]
        assert gc["position"][:k].tolist() == rc["position"] and gc["score"][:k].tolist() == rc["score"], (what, witness)
        assert (gc["position"][k:] == -1).all() and (gc["score"][k:] == 0).all()
    return got


@pytest.mark.parametrize("n,dim", [(1, 1), (2, 3), (100, 3), (100, 128), (257, 1), (257, 130)])
def test_twin_equals_the_definition_on_small_integer_rows(hip_lib, n, dim):
    rows = peaks_ref.small_integer_rows(n, dim, seed=n + dim)
    for m in (1, 5, n + 3) if n <= 100 else (9,):
        got = same_as_reference(rows, m, 0.02, kcenter_ref.exact_dist2, what="n %d dim %d m %d" % (n, dim, m))
        assert got["position"][0] == int(np.argmax(got["A"])) and got["score"][0] == got["A"].max()  # the densest row, the lowest position


@pytest.mark.parametrize("n,dim", [(1, 130), (2, 1), (100, 130), (257, 3), (257, 128)])
def test_twin_equals_the_definition_on_random_rows(hip_lib, n, dim):
    """the distances are the chain's (scann_knn_distsq_matrix): no fp32 operation is restated"""
    from scann import _hip

    rng = np.random.default_rng(n * 5 + dim)
    rows = (rng.standard_normal((n, dim)) * rng.uniform(0.1, 3, dim)).astype(np.float32)
    d2 = _hip.knn_dist2_matrix(rows, rows)
    gamma = float(np.float32(4.0 / max(float(np.median(d2)), 1e-3)))
    for m in (1, 7, n + 3) if n <= 100 else (12,):
        same_as_reference(rows, m, gamma, _hip.knn_dist2_matrix, what="n %d dim %d m %d" % (n, dim, m))


@pytest.mark.parametrize("n,dim", [(30, 3), (100, 7)])
def test_every_pick_is_the_argmax_of_the_objective(hip_lib, n, dim):
    from scann import _hip

    rows = peaks_ref.small_integer_rows(n, dim, seed=n)
    rows[n // 2] = rows[1]
    got = _hip.prototypes_host(rows, 8, 0.05)
    proto_ref.certificate(rows, got["position"][:got["count"]], kcenter_ref.exact_dist2, _hip.rbf_weight, 0.05)


def test_exact_duplicates_tie_by_position_and_fall_behind(hip_lib):
    from scann import _hip

    rows = peaks_ref.small_integer_rows(60, 6, seed=1)
    first = int(_hip.prototypes_host(rows, 1, 0.1)["position"][0])
    dup = (first + 17) % 60
    rows[dup] = rows[first]
    lo, hi = min(first, dup), max(first, dup)
    got = same_as_reference(rows, 60, 0.1, kcenter_ref.exact_dist2)
    n, A = 60, got["A"]
    assert A[lo] == A[hi] and got["position"][0] == lo  # equal scores: the lower position is picked
    at = {int(p): s for s, p in enumerate(got["position"])}
    assert at[hi] > 0
    # at pick 1 the duplicate's score is the pick's own score at pick 0, plus A once more, less n times the 2^30 it shares with the pick
    ref = proto_ref.prototypes(rows, 2, kcenter_ref.exact_dist2, _hip.rbf_weight, 0.1)
    score_hi_at_1 = 2 * int(A[hi]) - n * ref["T"][hi][lo]
    assert ref["T"][hi][lo] == ONE and score_hi_at_1 == int(got["score"][0]) + int(A[hi]) - n * ONE
    # and a duplicate of a criticism scores 0: it is never picked
    weight = np.ones(60, np.int64)
    c = _hip.criticisms_host(rows, weight, None, 60, 0.1)
    picked = c["position"][:c["count"]].tolist()
    assert picked[0] == 0 and (lo in picked) != (hi in picked) and c["count"] < 60 and (c["score"][:c["count"]] > 0).all()


def test_all_coincident_rows(hip_lib):
    rows = np.tile(peaks_ref.small_integer_rows(1, 5, seed=3), (40, 1))
    got = same_as_reference(rows, 6, 0.5, kcenter_ref.exact_dist2)
    assert got["position"].tolist() == [0, 1, 2, 3, 4, 5] and (got["A"] == 40 * ONE).all() and (got["B"] == 6 * ONE).all()
    assert (got["score"] == 40 * ONE).all() and got["b_at_pick"].tolist() == [s * ONE for s in range(6)]


def test_rows_with_nan_and_inf(hip_lib):
    rows = peaks_ref.small_integer_rows(50, 4, seed=4)
    rows[7, 1] = np.nan
    rows[20, 0] = np.inf
    rows[21, 3] = -np.inf
    got = same_as_reference(rows, 53, 0.1, kcenter_ref.exact_dist2)
    assert got["count"] == 47 and not {7, 20, 21} & set(got["position"].tolist())
    assert (got["A"][[7, 20, 21]] == -1).all() and (got["B"][[7, 20, 21]] == 0).all()


def test_the_empty_pool(hip_lib):
    from scann import _hip

    got = _hip.prototypes_host(np.zeros((0, 3), np.float32), 4, 0.5)
    assert got["count"] == 0 and (got["position"] == -1).all() and got["A"].shape == (0,)
    c = _hip.criticisms_host(np.zeros((0, 3), np.float32), np.zeros(0, np.int64), None, 2, 0.5)
    assert c["count"] == 0 and (c["position"] == -1).all()


def test_the_range_cap_names_both_numbers(hip_lib):
    from scann import _hip

    rows = np.zeros((65537, 1), np.float32)
    with pytest.raises(ValueError, match="65537 rows times m = 65536 pass 2\\^32"):
        _hip.prototypes_host(rows, 65536, 0.5)
    P = _hip._ptr
    pos = np.full(4, 7, np.int32)
    assert hip_lib.scann_prototypes_host(P(rows), 65537, 1, 65536, 0.5, P(pos), None, None, None, None) == -1 and (pos == 7).all()  # before any work
    assert hip_lib.scann_prototypes_host(P(rows), 4, 1, 2 ** 30 + 1, 0.5, P(pos), None, None, None, None) == -1
    assert hip_lib.scann_prototypes_host(P(rows), 4, 1, 4, 0.5, P(pos), None, None, None, None) == 4  # (N m = 2^32 itself is allowed: not run here)


def test_criticism_arguments_out_of_range_are_refused(hip_lib):
    from scann import _hip

    rows = peaks_ref.small_integer_rows(6, 2, seed=0)
    w = np.ones(6, np.int64)
    for bad, word in ((np.array([1, 1, 2 ** 31 + 1, 1, 1, 1]), "0 .. 2\\^31"), (np.array([1, -1, 1, 1, 1, 1]), "0 .. 2\\^31"), (np.ones(5, np.int64), "one integer per row"),
                      (np.ones(6), "one integer per row")):
        with pytest.raises(ValueError, match=word):
            _hip.criticisms_host(rows, bad, None, 2, 0.5)
    with pytest.raises(ValueError, match="exclude"):
        _hip.criticisms_host(rows, w, [6], 2, 0.5)
    with pytest.raises(ValueError, match="c must"):
        _hip.criticisms_host(rows, w, None, 0, 0.5)
    with pytest.raises(ValueError, match="gamma"):
        _hip.criticisms_host(rows, w, None, 2, 0.0)
    with pytest.raises(ValueError, match="m must"):
        _hip.prototypes_host(rows, 0, 0.5)
    P = _hip._ptr
    pos, far, ex = np.full(2, 7, np.int32), np.array([1, 1, 2 ** 31 + 1, 1, 1, 1], np.int64), np.array([6], np.int32)
    assert hip_lib.scann_criticisms_host(P(rows), 6, 2, P(far), None, 0, 2, 0.5, P(pos), None) == -1  # the C twin refuses them itself
    assert hip_lib.scann_criticisms_host(P(rows), 6, 2, P(w), P(ex), 1, 2, 0.5, P(pos), None) == -1 and (pos == 7).all()
    w[3] = 2 ** 31
    assert _hip.criticisms_host(rows, w, None, 1, 0.5)["position"][0] == 3  # the largest weight allowed


THREAD_SCRIPT = """
import os, sys
if sys.argv[2] == "one":
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})  # before the library starts a thread: it sees one CPU
sys.path[:0] = [%r, %r]
import numpy as np
import peaks_ref
from scann import _hip
rows = peaks_ref.small_integer_rows(40000, 104, seed=8)  # 40,000 x 104: above the fold's threshold for threading
out = _hip.prototypes_host(rows[:2000], 20, 0.01)   # the density pass threads here ...
big = _hip.criticisms_host(rows, np.arange(40000) %% 97 + 1, None, 3, 0.01)   # ... and the fold here
np.savez(sys.argv[1], cpus=len(os.sched_getaffinity(0)), cpos=big["position"], cscore=big["score"], **out)
"""


def test_twins_do_not_depend_on_the_thread_count(hip_lib, tmp_path):
    """one process whose runtime sees 1 CPU against one that sees them all"""
    script = tmp_path / "run.py"
    script.write_text(THREAD_SCRIPT % (os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "tests")))
    outs = []
    for cpus in ("one", "all"):
        path = str(tmp_path / ("out_%s.npz" % cpus))
        subprocess.run([sys.executable, str(script), path, cpus], check=True)
        with np.load(path) as z:
            outs.append({k: z[k] for k in z.files})
    assert outs[0]["cpus"] == 1 and outs[1]["cpus"] == len(os.sched_getaffinity(0))
    for k in ("position", "score", "b_at_pick", "A", "B", "cpos", "cscore"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert outs[0]["count"] == 20 and (outs[0]["cpos"] >= 0).all()


def test_planted_clusters(hip_lib):
    """four Gaussian clusters of 600 / 300 / 100 / 30 rows, ten prototypes: their shares follow the clusters' mass, the criticisms fall in
    the cluster no prototype covers, and the MMD curve does not rise"""
    from scann.models import latent_index as li

    rows, planted = proto_ref.planted(PLANTED_SEED)
    res, pr = li.prototypes_rows_host(rows, 10, criticisms=5)
    counts = np.bincount(planted[res["position"]], minlength=4)
    share = 10 * np.array(proto_ref.PLANTED_SIZES) / len(rows)
    print("bandwidth %.4g, prototypes per cluster %s (mass %s), criticisms in %s, mmd2 %s" % (
        res["bandwidth"], counts, share, planted[res["criticism_position"]], res["mmd2"]))
    assert counts.tolist() == [6, 3, 1, 0] and (np.abs(counts - share) <= 1).all()
    assert res["count"] == 10 and (np.diff(res["mmd2"]) <= 0).all() and (res["mmd2"] > 0).all()
    assert len(res["criticism_position"]) == 5 and (planted[res["criticism_position"]] == 3).all()
    assert (res["criticism_witness"] > 0).all() and res["size"].sum() == len(rows) and len(res["witness"]) == len(rows)
    assert np.array_equal(planted[res["position"]][res["nearest_prototype"]], planted) or (planted[res["position"]][res["nearest_prototype"]] == planted).mean() > 0.96
    # three prototypes cover the two large clusters only: every criticism falls in the larger of the two left out
    three, _ = li.prototypes_rows_host(rows, 3, criticisms=5, bandwidth=res["bandwidth"])
    assert np.bincount(planted[three["position"]], minlength=4).tolist() == [2, 1, 0, 0] and (planted[three["criticism_position"]] == 2).all()
    assert np.array_equal(three["position"], res["position"][:3]) and np.array_equal(three["mmd2"], res["mmd2"][:3])  # greedy: a prefix
    assert pr.m == 10 and pr.rows.shape == (10, 16) and np.array_equal(pr.rows, rows[res["position"]]) and len(pr.criticism_ids) == 5


def test_mmd_of_two_samples(hip_lib):
    """two samples of one distribution score below two of shifted distributions; the value is the restatement's exact rational"""
    from scann import _hip
    from scann.models import latent_index as li

    rng = np.random.default_rng(5)
    a, b = (rng.standard_normal((n, 6)).astype(np.float32) for n in (150, 120))
    c = b + np.float32(1.5)
    c[7, 2] = np.nan  # left out on its side
    gamma = _hip.rbf_gamma(2.0)

    def sums(x, y):
        return _hip.density_host(y, x, gamma)  # the rows of x under the pool y

    same, _, num, den = li.mmd_of_sums(sums(a, a), sums(b, b), sums(b, a))
    want = proto_ref.mmd_two(a, b, _hip.knn_dist2_matrix, _hip.rbf_weight, gamma)
    assert Fraction(num, den) == want and same == float(want)
    ok = np.isfinite(c).all(1)
    shifted, wit, num, den = li.mmd_of_sums(sums(a, a), sums(c, c[ok]), sums(c, a))
    assert Fraction(num, den) == proto_ref.mmd_two(a, c[ok], _hip.knn_dist2_matrix, _hip.rbf_weight, gamma)
    assert 0 <= same < 0.03 and shifted > 0.2 and np.isnan(wit[7]) and (wit[ok] < 0).mean() > 0.9  # b's rows lie where a is thin
    with pytest.raises(ValueError, match="MMD needs"):
        li.mmd_of_sums([-1], [5], [5])


def test_header_and_python_agree(hip_lib):
    abi_checks.declared("int64_t scann_index_prototypes(scann_handle_t* h, scann_index_t* pool, int64_t m, float gamma, int32_t* pos, int64_t* ids, "
                        "int32_t* atoms,",
                        "int64_t* score, int64_t* b_at_pick /* [m] */, int64_t* A /* [N] or NULL */, int64_t* B /* [N] or NULL */);",
                        "int64_t scann_index_criticisms(scann_handle_t* h, scann_index_t* pool, const int64_t* weight /* [N] */, const int32_t* exclude,",
                        "int64_t scann_prototypes_host(const float* rows, int64_t n, int64_t dim, int64_t m, float gamma, int32_t* pos, int64_t* score,",
                        "int64_t scann_criticisms_host(const float* rows, int64_t n, int64_t dim, const int64_t* weight, const int32_t* exclude, "
                        "int64_t n_exclude,",
                        "score_i = (s + 1) A_i - n B_i", "(score descending, position ascending)", "The calls require N m <= 2^32",
                        "An ineligible row gets A = -1", "Cmax_i = max(Cmax_i, t(i, pick))")
    P, L, F = C.c_void_p, C.c_int64, C.c_float
    sig = abi_checks.signatures({
        "scann_index_prototypes": (L, [P, P, L, F, P, P, P, P, P, P, P]),
        "scann_index_criticisms": (L, [P, P, P, P, L, L, F, P, P, P, P]),
        "scann_prototypes_host": (L, [P, L, L, L, F, P, P, P, P, P]),
        "scann_criticisms_host": (L, [P, L, L, P, P, L, L, F, P, P])})
    for name in sig:
        assert hasattr(hip_lib, name), name


def test_the_step_kernel_uses_no_scratch(hip_lib):
    from scann import _hip

    kernels = {n: v for n, v in abi_checks.device_kernels(_hip.LIB_PATH).items() if "proto_step_kernel" in n}
    assert len(kernels) == 2, sorted(kernels)  # the sum fold and the max fold
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0 and vgprs <= 128, (name, scratch, vgprs)  # 128 VGPRs: four workgroups of 256 lanes per CU


def test_prototypes_save_load_and_check(hip_lib, tmp_path):
    from scann.models import LatentPrototypes

    class Model:
        config = {"model": {"dense_out": 4, "global_dim": 9}}

    rows = np.arange(12, dtype=np.float32).reshape(3, 4)
    crows = rows[:2] + 100
    pr = LatentPrototypes(rows, [10, 11, 12], [-1, -1, -1], crows, [20, 21], [-1, -1], 1.5, "structure", 4)
    pr.check_model(Model)
    pr.save(str(tmp_path / "p.npz"))
    back = LatentPrototypes.load(Model, str(tmp_path / "p.npz"))
    for key in ("rows", "ids", "atoms", "criticism_rows", "criticism_ids", "criticism_atoms"):
        assert np.array_equal(getattr(back, key), getattr(pr, key)) and getattr(back, key).dtype == getattr(pr, key).dtype, key
    assert (back.bandwidth, back.level, back.dim, back.m) == (1.5, "structure", 4, 3)
    none = LatentPrototypes(rows, [10, 11, 12], [0, 1, 2], np.zeros((0, 4)), [], [], 2.0, "structure")
    assert none.criticism_rows.shape == (0, 4) and none.dim == 4
    for args, word in (((rows, [10, 11], [-1, -1, -1], crows, [20, 21], [-1, -1], 1.5, "structure", 4), "one entry per row"),
                       ((rows, [10, 11, 12], [-1, -1, -1], crows, [20, 21], [-1, -1], 0.0, "structure", 4), "bandwidth"),
                       ((rows, [10, 11, 12], [-1, -1, -1], crows, [20, 21], [-1, -1], 1.5, "bond", 4), "level"),
                       ((rows, [10, 11, 12], [-1, -1, -1], crows, [20, 21], [-1, -1], 1.5, "structure", 5), "rows must"),
                       ((np.full_like(rows, np.inf), [10, 11, 12], [-1, -1, -1], crows, [20, 21], [-1, -1], 1.5, "structure", 4), "non-finite")):
        with pytest.raises(ValueError, match=word):
            LatentPrototypes(*args)
    atom = LatentPrototypes(rows, [10, 11, 12], [0, 1, 2], crows, [20, 21], [3, 4], 1.5, "atom", 4)
    with pytest.raises(ValueError, match="does not fit"):
        atom.check_model(Model)
    atom.save(str(tmp_path / "a.npz"))
    with pytest.raises(ValueError, match="does not fit"):
        LatentPrototypes.load(Model, str(tmp_path / "a.npz"))
    from scann.models import LatentPeaks

    with pytest.raises(ValueError, match="not a saved"):
        LatentPrototypes.load(Model, _saved_peaks(tmp_path, LatentPeaks))


def _saved_peaks(tmp_path, LatentPeaks):
    path = str(tmp_path / "peaks.npz")
    LatentPeaks(np.zeros(3, np.int32), np.arange(3), np.arange(3), [0], 1.5, "structure", 4).save(path)
    return path


def test_the_host_route_of_an_index(hip_lib):
    """LatentIndex.prototypes(route="host") on a model without a GPU: the index's search gives the bandwidth, the twins the loops -- the
    result of prototypes_rows_host on the same rows, names included"""
    from scann.models import LatentIndex
    from scann.models import latent_index as li

    rows, planted = proto_ref.planted(1)
    rows = np.ascontiguousarray(rows[:400, :4])
    model = peaks_cpu.RowsModel(dense_out=4)
    index = LatentIndex(model, "structure").add_rows(rows[:150], ids=np.arange(150) + 1000).add_rows(rows[150:], ids=np.arange(150, 400) + 1000)
    res, pr = index.prototypes(7, criticisms=3, route="host")
    want, _ = li.prototypes_rows_host(rows, 7, criticisms=3)
    assert sorted(res) == sorted(want)
    for key in ("position", "score", "b_at_pick", "A", "B", "criticism_position", "criticism_score", "nearest_prototype", "size", "mmd2", "witness"):
        assert np.array_equal(res[key], want[key], equal_nan=key == "witness"), key
    assert res["bandwidth"] == want["bandwidth"] and res["gamma"] == want["gamma"] and res["n_eligible"] == 400
    assert np.array_equal(res["id"], res["position"] + 1000) and (res["atom"] == -1).all()
    assert np.array_equal(res["criticism_id"], res["criticism_position"] + 1000)
    assert pr.level == "structure" and pr.dim == 4 and np.array_equal(pr.ids, res["id"]) and np.array_equal(pr.rows, rows[res["position"]])
    plain, _ = index.prototypes(7, bandwidth=res["bandwidth"], assign=False, route="host")
    assert "size" not in plain and len(plain["criticism_position"]) == 0 and np.array_equal(plain["position"], res["position"])
    for kw, word in ((dict(m=0), "m must"), (dict(m=2, criticisms=-1), "criticisms"), (dict(m=2, bandwidth="wide"), "bandwidth"),
                     (dict(m=2, neighbours=0), "neighbours"), (dict(m=2, witness="over"), "witness"), (dict(m=2, route="gpu"), "route"),
                     (dict(m=2, assign="yes"), "assign"), (dict(m=2 ** 31), "2\\^32")):
        with pytest.raises(ValueError, match=word):
            index.prototypes(**kw)
    with pytest.raises(ValueError, match="at least 1 row"):
        LatentIndex(model, "structure").prototypes(2, bandwidth=1.0, route="host")


def test_cli_takes_the_prototypes_flags():
    spec = importlib.util.spec_from_file_location("predict_model_cli", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parser().parse_args(["some_dir", "--prototypes", "12", "--criticisms", "5", "--prototypes-level", "structure", "--prototypes-bandwidth", "2.5",
                                 "--prototypes-out", "protos.npz", "--nearest-prototype", "saved.npz"])
    assert (a.prototypes, a.criticisms, a.prototypes_level, a.prototypes_bandwidth, a.prototypes_out, a.nearest_prototype) == (
        12, 5, "structure", 2.5, "protos.npz", "saved.npz")
    d = cli.parser().parse_args(["some_dir"])
    assert (d.prototypes, d.criticisms, d.prototypes_level, d.prototypes_bandwidth, d.prototypes_out, d.nearest_prototype) == (0, 0, "atom", 0.0, "", "")
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--prototypes-level", "bond"])
    for bad in (["--prototypes", "-1"], ["--criticisms", "3"], ["--prototypes-out", "x.npz"], ["--prototypes-bandwidth", "2"],
                ["--prototypes", "2", "--prototypes-bandwidth", "-1"], ["--prototypes", "2", "--criticisms", "-1"]):  # before the model's folder is read
        with pytest.raises(SystemExit):
            cli.main(cli.parser().parse_args(["no_such_model_dir"] + bad))
