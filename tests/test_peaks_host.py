"""Host tests of the density-peak clustering and the kernel density of a latent index (scann_index_density / scann_index_peaks, the twins
scann_density_host / scann_peaks_host, LatentIndex.density_peaks, LatentPeaks): the twins against the NumPy restatement of the definition
(tests/peaks_ref.py) in integers and bit for bit, with ties, coincident rows, tiny pools, non-finite rows, skipped positions and weights
that vanish; independence of the thread count; the planted blobs and the two crescents end to end; the argument checks; header, ctypes
table and library agree; LatentPeaks' round trip; the host route of LatentIndex.density_peaks.  No GPU."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import abi_checks
import kcenter_ref
import peaks_cpu
import peaks_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CRESCENT_SEED = 0  # checked with the reference below before it was committed


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def same_as_reference(rows, gamma, what=""):
    """the twin's self-join equals the restated definition, and passes its certificate; returns the twin's dict"""
    from scann import _hip

    got = _hip.peaks_host(rows, gamma)
    sums, parent, delta2, _ = peaks_ref.peaks(rows, kcenter_ref.exact_dist2, _hip.rbf_weight, gamma)
    assert [int(s) for s in got["sum"]] == sums, what
    assert np.array_equal(got["parent"], parent), what
    assert np.array_equal(bits(got["delta2"]), bits(delta2)), what
    assert got["sum"].dtype == np.int64 and got["parent"].dtype == np.int32 and got["delta2"].dtype == np.float32
    peaks_ref.certificate(rows, got["sum"], got["parent"], got["delta2"], kcenter_ref.exact_dist2)
    return got


@pytest.mark.parametrize("n,dim", [(1, 3), (2, 5), (9, 1), (37, 7), (130, 20), (257, 130)])
@pytest.mark.parametrize("gamma", [0.01, 0.3])
def test_twin_equals_the_definition_on_small_integer_rows(hip_lib, n, dim, gamma):
    rows = peaks_ref.small_integer_rows(n, dim, seed=n + dim)
    got = same_as_reference(rows, gamma, "n %d dim %d" % (n, dim))
    assert (got["sum"] >= 0).all() and int((got["parent"] < 0).sum()) == 1
    # the same sums as arbitrary queries with their own positions left out, and with nothing left out one term of 2^30 more
    from scann import _hip

    assert np.array_equal(_hip.density_host(rows, rows, gamma, np.arange(n)), got["sum"])
    assert np.array_equal(_hip.density_host(rows, rows, gamma), got["sum"] + 2 ** 30)


def test_exact_duplicates_tie_by_position(hip_lib):
    rows = peaks_ref.small_integer_rows(40, 6, seed=1)
    rows[7] = rows[3]
    rows[21] = rows[3]
    rows[30] = rows[12]
    got = same_as_reference(rows, 0.1)
    s = got["sum"]
    assert s[3] == s[7] == s[21] and s[12] == s[30]
    # equal sums: the earlier row is above the later one, so a duplicate's parent is its earlier copy at distance 0
    assert got["parent"][7] == 3 and got["parent"][21] == 3 and got["parent"][30] == 12
    assert got["delta2"][7] == 0 and got["delta2"][21] == 0 and got["delta2"][30] == 0


def test_all_coincident_rows(hip_lib):
    rows = np.tile(np.array([[2.0, -1.0, 3.0]], np.float32), (70, 1))
    got = same_as_reference(rows, 0.5)
    assert (got["sum"] == 69 * 2 ** 30).all()  # every term is exactly 2^30 at distance 0
    assert got["parent"][0] == -1 and got["delta2"][0] == np.inf
    assert (got["parent"][1:] == 0).all() and (got["delta2"][1:] == 0).all()


def test_empty_and_tiny_pools(hip_lib):
    from scann import _hip

    empty = _hip.peaks_host(np.zeros((0, 4), np.float32), 0.5)
    assert empty["sum"].shape == (0,) and empty["parent"].shape == (0,) and empty["delta2"].shape == (0,)
    one = same_as_reference(np.array([[1.0, 2.0]], np.float32), 0.5)
    assert one["sum"][0] == 0 and one["parent"][0] == -1 and one["delta2"][0] == np.inf
    two = same_as_reference(np.array([[0.0, 0.0], [1.0, 1.0]], np.float32), 0.5)
    assert two["sum"][0] == two["sum"][1] == 2 ** 29  # 2^(-2 * 0.5)
    assert list(two["parent"]) == [-1, 0] and two["delta2"][1] == 2.0
    # an empty pool gives zeros for finite queries and -1 for the others
    q = np.array([[1.0, 2.0], [np.nan, 0.0]], np.float32)
    assert list(_hip.density_host(np.zeros((0, 2), np.float32), q, 0.5)) == [0, -1]
    assert _hip.density_host(q[:1], np.zeros((0, 2), np.float32), 0.5).shape == (0,)


def test_rows_with_nan_and_inf(hip_lib):
    rows = peaks_ref.small_integer_rows(50, 5, seed=4)
    rows[4, 2] = np.nan
    rows[17, 0] = np.inf
    rows[33, 4] = -np.inf
    got = same_as_reference(rows, 0.05)
    for i in (4, 17, 33):
        assert got["sum"][i] == -1 and got["parent"][i] == -1 and got["delta2"][i] == np.inf
    assert not np.isin(got["parent"], [4, 17, 33]).any()
    # the eligible rows' results are those of the pool without the others
    keep = np.array([i for i in range(50) if i not in (4, 17, 33)])
    from scann import _hip

    clean = _hip.peaks_host(rows[keep], 0.05)
    assert np.array_equal(clean["sum"], got["sum"][keep]) and np.array_equal(bits(clean["delta2"]), bits(got["delta2"][keep]))
    assert np.array_equal(np.where(clean["parent"] >= 0, keep[np.maximum(clean["parent"], 0)], -1), got["parent"][keep])


def test_density_of_queries_with_skipped_positions(hip_lib):
    from scann import _hip

    rows = peaks_ref.small_integer_rows(90, 9, seed=5)
    rows[13, 1] = np.nan
    q = peaks_ref.small_integer_rows(21, 9, seed=6)
    q[2] = rows[40]
    q[5, 3] = np.inf
    for skip in (None, np.full(21, -1), np.arange(21) * 4, np.array([40] * 21), np.arange(21) + 1000):
        got = _hip.density_host(rows, q, 0.02, skip)
        want = peaks_ref.density(rows, q, kcenter_ref.exact_dist2, _hip.rbf_weight, 0.02, skip)
        assert [int(s) for s in got] == want
        assert got[5] == -1
    with_own = _hip.density_host(rows, q, 0.02)
    assert with_own[2] - _hip.density_host(rows, q, 0.02, np.full(21, 40))[2] == 2 ** 30  # q[2] lies on row 40


def test_far_weights_vanish(hip_lib):
    """a gamma at which every pair at distance > 0 weighs 0: only coincident rows count, and parents still follow the distances"""
    from scann import _hip

    rows = peaks_ref.small_integer_rows(30, 4, seed=7)
    rows[9] = rows[2]
    got = same_as_reference(rows, 200.0)
    assert _hip.rbf_weight(np.float32(1.0), 200.0) == 0
    want = np.zeros(30, np.int64)
    want[[2, 9]] = 2 ** 30
    assert np.array_equal(got["sum"], want)
    assert got["parent"][2] == -1 and got["parent"][9] == 2
    assert (got["parent"][got["sum"] == 0] >= 0).all()  # zeros tie by position: each follows its nearest row above it


THREAD_SCRIPT = """
import os, sys
if sys.argv[2] == "one":
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})  # before the library starts a thread: it sees one CPU
sys.path[:0] = [%r, %r]
import numpy as np
import peaks_ref
from scann import _hip
rows = peaks_ref.small_integer_rows(700, 24, seed=8)  # 700^2 pairs of 24 columns: above the twin's threshold for threading
out = _hip.peaks_host(rows, 0.01)
np.savez(sys.argv[1], density=_hip.density_host(rows, rows[:300] + 1, 0.01), cpus=len(os.sched_getaffinity(0)), **out)
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
    for k in ("sum", "parent", "density"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert np.array_equal(bits(outs[0]["delta2"]), bits(outs[1]["delta2"]))
    rows = peaks_ref.small_integer_rows(700, 24, seed=8)
    peaks_ref.certificate(rows, outs[0]["sum"], outs[0]["parent"], outs[0]["delta2"], kcenter_ref.exact_dist2)


def test_host_assembly_equals_its_restatement(hip_lib):
    from scann import _hip
    from scann.models import latent_index as li

    rows = peaks_ref.small_integer_rows(120, 5, seed=9)
    rows[8] = rows[1]
    rows[50, 0] = np.nan
    rows[60], rows[61] = np.float32(3e19), np.float32(-3e19)  # finite; every distance overflows: sums of 0 and parents at +inf
    r = _hip.peaks_host(rows, 0.05)
    assert r["sum"][60] == 0 and r["sum"][61] == 0 and r["parent"][60] >= 0 and r["delta2"][60] == np.inf and r["delta2"][61] == np.inf
    dens = np.ldexp(r["sum"].astype(np.float64), -30) / 119
    for kw in (dict(k=1), dict(k=4), dict(k=119), dict(min_density=float(np.median(dens[dens >= 0])), min_delta=2.0), dict(min_density=0.0, min_delta=0.0),
               dict(min_density=1e9, min_delta=0.0)):
        got = li.peaks_assemble(r["sum"], r["parent"], r["delta2"], **kw)
        want = peaks_ref.assemble(r["sum"], r["parent"], r["delta2"], **kw)
        for key in ("label", "centre_position", "size"):
            assert np.array_equal(got[key], want[key]), (kw, key)
        for key in ("density", "delta", "decision"):
            assert np.array_equal(got[key].view(np.uint64), want[key].view(np.uint64)), (kw, key)
        root = int(np.nonzero((r["parent"] < 0) & (r["sum"] >= 0))[0][0])
        assert got["centre_position"][0] == root and got["label"][root] == 0 and got["label"][50] == -1
        assert got["decision"][0] == np.inf and np.isfinite(got["decision"][1:]).all() and (np.diff(got["decision"][1:]) <= 0).all()
        assert got["size"].sum() == 119 and got["n_eligible"] == 119
    assert len(li.peaks_assemble(r["sum"], r["parent"], r["delta2"], min_density=1e9, min_delta=0.0)["centre_position"]) == 1  # the root alone
    with pytest.raises(ValueError, match="k = 120"):
        li.peaks_assemble(r["sum"], r["parent"], r["delta2"], k=120)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_blobs_are_recovered(hip_lib, seed):
    """300 / 120 / 60 rows in 3 of 128 columns at 0.5 x, 1 x and 2 x the automatic bandwidth: every label is the planted one, and the
    three centres lie one per blob"""
    from scann.models import latent_index as li

    rows, planted = peaks_ref.blobs(seed)
    auto, _ = li.density_peaks_rows_host(rows, k=3)
    for f in (0.5, 1.0, 2.0):
        res, pk = li.density_peaks_rows_host(rows, k=3, bandwidth=auto["bandwidth"] * f)
        print("seed %d, %.1f x h = %.4f: sizes %s, decision %s" % (seed, f, res["bandwidth"], res["size"], res["decision"][:5]))
        assert sorted(planted[res["centre_position"]]) == [0, 1, 2]
        assert np.array_equal(planted[res["centre_position"]][res["label"]], planted)  # every row carries its blob's centre
        assert sorted(res["size"]) == [60, 120, 300] and res["label"][res["centre_position"][0]] == 0
        assert res["decision"][2] > 2.0 * res["decision"][3]  # the gap in the decision graph says three
        assert np.array_equal(pk.label, res["label"]) and pk.k == 3 and len(pk) == 480
    by_threshold, _ = li.density_peaks_rows_host(rows, bandwidth=auto["bandwidth"], min_density=0.0, min_delta=6.0)  # blobs are 17 apart
    assert np.array_equal(by_threshold["label"], auto["label"])


def test_crescents_need_density_peaks(hip_lib):
    """two interleaved crescents of 800 integer rows in 16 columns (the committed seed): density peaks at the automatic bandwidth label
    every row right, in the twin and in the restated definition alike; Lloyd's k-means with k = 2 cannot"""
    from scann import _hip
    from scann.models import latent_index as li

    rows, planted = peaks_ref.crescents(CRESCENT_SEED)
    res, _ = li.density_peaks_rows_host(rows, k=2)
    share = peaks_ref.matches(res["label"], planted)
    sums, parent, delta2, _ = peaks_ref.peaks(rows, kcenter_ref.exact_dist2, _hip.rbf_weight, res["gamma"])
    ref = peaks_ref.assemble(sums, parent, delta2, k=2)
    worst = 0.0
    for s in range(5):
        init = rows[np.random.default_rng(s).choice(len(rows), 2, replace=False)]
        worst = max(worst, peaks_ref.matches(_hip.kmeans_host(rows, init, 100)["label"], planted))
    print("h^2 %.2f: density peaks %.4f, reference %.4f, k-means at best %.4f" % (
        res["bandwidth"] ** 2, share, peaks_ref.matches(ref["label"], planted), worst))
    assert share == 1.0
    assert np.array_equal(ref["label"], res["label"]) and [int(s) for s in res["sum"]] == sums
    assert worst < 0.9
    assert 35.0 < res["bandwidth"] ** 2 < 60.0


def test_argument_errors_name_the_argument(hip_lib):
    from scann import _hip
    from scann.models import latent_index as li

    rows = peaks_ref.small_integer_rows(20, 4, seed=3)
    nan, inf = float("nan"), float("inf")
    for g in (0.0, -1.0, nan, inf, "x", True, 1e-60):
        with pytest.raises(ValueError, match="gamma"):
            _hip.peaks_host(rows, g)
        with pytest.raises(ValueError, match="gamma"):
            _hip.density_host(rows, rows, g)
    with pytest.raises(ValueError, match="rows"):
        _hip.peaks_host(rows[0], 0.5)
    with pytest.raises(ValueError, match="q must"):
        _hip.density_host(rows, rows[:, :3], 0.5)
    with pytest.raises(ValueError, match="q must"):
        _hip.density_host(rows, "abc", 0.5)
    for skip in (np.zeros(19, np.int64), np.zeros(20), np.zeros((20, 1), np.int32), np.full(20, 2 ** 40)):
        with pytest.raises(ValueError, match="skip_pos"):
            _hip.density_host(rows, rows, 0.5, skip)
    for kw, word in ((dict(), "exactly one"), (dict(k=2, min_density=0.1, min_delta=1.0), "exactly one"), (dict(min_density=0.1), "together"),
                     (dict(k=0), "k must"), (dict(k=2.5), "k must"), (dict(k=True), "k must"), (dict(k=21), "k = 21"),
                     (dict(min_density=-1.0, min_delta=1.0), "min_density"), (dict(min_density=0.0, min_delta=nan), "min_delta"),
                     (dict(k=2, bandwidth="wide"), "bandwidth"), (dict(k=2, bandwidth=0.0), "bandwidth"), (dict(k=2, bandwidth=-1.0), "bandwidth"),
                     (dict(k=2, neighbours=0), "neighbours"), (dict(k=2, neighbours=32), "neighbours"), (dict(k=2, neighbours=2.0), "neighbours")):
        with pytest.raises(ValueError, match=word):
            li.density_peaks_rows_host(rows, **kw)
    with pytest.raises(ValueError, match="route"):
        li.peaks_fit_args(2, "auto", 31, None, None, "gpu")
    bad = rows.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):  # the automatic bandwidth inherits neighbour_graph's refusal ...
        li.density_peaks_rows_host(bad, k=2)
    assert li.density_peaks_rows_host(bad, k=2, bandwidth=2.0)[0]["label"][3] == -1  # ... a given one does not need it
    with pytest.raises(ValueError, match="automatic bandwidth"):
        li.density_peaks_rows_host(np.zeros((10, 3), np.float32), k=1)


def test_the_c_twins_refuse_bad_arguments_themselves(hip_lib):
    """the twins' own checks, behind Python's: SCANN_ERR_INVALID (-1), nothing written"""
    from scann import _hip

    P = _hip._ptr
    rows = peaks_ref.small_integer_rows(10, 3, seed=2)
    sums, parent, delta2 = np.full(10, 7, np.int64), np.full(10, 7, np.int32), np.full(10, 7, np.float32)

    def peaks(rows=P(rows), n=10, dim=3, gamma=0.5, sums=P(sums), parent=P(parent), delta2=P(delta2)):
        return hip_lib.scann_peaks_host(rows, n, dim, gamma, sums, parent, delta2)

    def density(rows=P(rows), n=10, dim=3, q=P(rows), nq=10, gamma=0.5, sums=P(sums)):
        return hip_lib.scann_density_host(rows, n, dim, q, nq, None, gamma, sums)

    for kw in (dict(rows=None), dict(n=-1), dict(n=2 ** 31), dict(dim=0), dict(gamma=0.0), dict(gamma=-2.0), dict(gamma=float("nan")),
               dict(gamma=float("inf")), dict(sums=None), dict(parent=None), dict(delta2=None)):
        assert peaks(**kw) == -1, kw
    for kw in (dict(rows=None), dict(n=-1), dict(dim=0), dict(q=None), dict(nq=-1), dict(gamma=0.0), dict(gamma=float("nan")), dict(sums=None)):
        assert density(**kw) == -1, kw
    assert (sums == 7).all() and (parent == 7).all() and (delta2 == 7).all()
    assert peaks() == 0 and density(nq=0, q=None, sums=None) == 0 and peaks(n=0, rows=None, sums=None, parent=None, delta2=None) == 0


def test_header_and_python_agree(hip_lib):
    from scann import _hip

    abi_checks.declared("int scann_index_density(scann_handle_t* h, scann_index_t* pool, const float* q /* host [nq * dim] */, int64_t nq, "
                        "const int32_t* skip_pos /* [nq] or NULL */, float gamma, int64_t* sums /* [nq] */);",
                        "int scann_index_peaks(scann_handle_t* h, scann_index_t* pool, float gamma, int64_t* sums /* [N] */, int32_t* parent /* [N] */, "
                        "float* delta2 /* [N] */);",
                        "int scann_index_density_batch(scann_handle_t* h, scann_index_t* idx, scann_dbatch_t* db, int32_t level, float gamma, float* y, "
                        "float* ga, int64_t* sums);",
                        "int scann_density_host(const float* rows, int64_t n, int64_t dim, const float* q, int64_t nq, const int32_t* skip_pos, "
                        "float gamma, int64_t* sums);",
                        "int scann_peaks_host(const float* rows, int64_t n, int64_t dim, float gamma, int64_t* sums, int32_t* parent, float* delta2);",
                        "t = llrintf(ldexpf(w, 30)), round to nearest even", "row j is ABOVE row i iff S_j > S_i, or S_j == S_i and j < i",
                        "(dist2 ascending, position ascending)", "An ineligible query gets S = -1", "the parents form a tree", "#define SCANN_ABI_VERSION 1")
    assert hip_lib.scann_abi_version() == 1
    P, I, L, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    sig = abi_checks.signatures({
        "scann_index_density": (C.c_int, [P, P, P, L, P, F, P]),
        "scann_index_peaks": (C.c_int, [P, P, F, P, P, P]),
        "scann_index_density_batch": (C.c_int, [P, P, P, I, F, P, P, P]),
        "scann_density_host": (C.c_int, [P, L, L, P, L, P, F, P]),
        "scann_peaks_host": (C.c_int, [P, L, L, F, P, P, P])})
    for name in sig:
        assert hasattr(hip_lib, name), name


def test_peaks_save_load_and_check(hip_lib, tmp_path):
    from scann.models import LatentPeaks

    class Model:
        config = {"model": {"dense_out": 4, "global_dim": 9}}

    label = np.array([0, 1, 1, -1, 0, 2, 1], np.int32)
    pk = LatentPeaks(label, np.arange(7) + 10, np.full(7, -1), [4, 2, 5], 1.5, "structure", 4)
    pk.check_model(Model)
    pk.save(str(tmp_path / "p.npz"))
    back = LatentPeaks.load(Model, str(tmp_path / "p.npz"))
    for key in ("label", "ids", "atoms", "centre_position"):
        assert np.array_equal(getattr(back, key), getattr(pk, key)) and getattr(back, key).dtype == getattr(pk, key).dtype, key
    assert (back.bandwidth, back.level, back.dim, back.k, len(back)) == (1.5, "structure", 4, 3, 7)
    # labels of the positions a k = 1 search reports, any shape; -1 stays -1
    assert np.array_equal(back.label_of(np.array([[5], [3], [-1], [0]])), [[2], [-1], [-1], [0]])
    for bad in (np.array([7]), np.array([-2]), np.array([0.5])):
        with pytest.raises(ValueError, match="position"):
            back.label_of(bad)
    for args, word in (((label, np.arange(6), np.arange(7), [4, 2, 5], 1.5, "structure", 4), "ids"),
                       ((label, np.arange(7), np.arange(7), [4, 2, 7], 1.5, "structure", 4), "centre_position"),
                       ((label, np.arange(7), np.arange(7), [4, 2], 1.5, "structure", 4), "label"),
                       ((label, np.arange(7), np.arange(7), [4, 2, 5], 0.0, "structure", 4), "bandwidth"),
                       ((label, np.arange(7), np.arange(7), [4, 2, 5], 1.5, "bond", 4), "level")):
        with pytest.raises(ValueError, match=word):
            LatentPeaks(*args)
    atom = LatentPeaks(label, np.arange(7), np.arange(7), [4, 2, 5], 1.5, "atom", 4)
    with pytest.raises(ValueError, match="does not fit"):
        atom.check_model(Model)
    atom.save(str(tmp_path / "a.npz"))
    with pytest.raises(ValueError, match="does not fit"):
        LatentPeaks.load(Model, str(tmp_path / "a.npz"))


def test_the_host_route_of_an_index(hip_lib):
    """LatentIndex.density_peaks(route="host") on a model without a GPU: the index's search gives the bandwidth, the twins the passes --
    the result of density_peaks_rows_host on the same rows, names included"""
    from scann.models import LatentIndex
    from scann.models import latent_index as li

    rows, planted = peaks_ref.blobs(3)
    rows = np.ascontiguousarray(rows[:, [5, 40, 99, 0]])
    model = peaks_cpu.RowsModel(dense_out=4)
    index = LatentIndex(model, "structure").add_rows(rows[:200], ids=np.arange(200) + 1000).add_rows(rows[200:], ids=np.arange(200, 480) + 1000)
    res, pk = index.density_peaks(k=3, route="host")
    want, _ = li.density_peaks_rows_host(rows, k=3)
    for key in ("label", "parent", "sum", "centre_position", "size"):
        assert np.array_equal(res[key], want[key]), key
    assert res["bandwidth"] == want["bandwidth"] and res["gamma"] == want["gamma"]
    assert np.array_equal(res["centre_id"], res["centre_position"] + 1000) and (res["centre_atom"] == -1).all()
    assert np.array_equal(planted[res["centre_position"]][res["label"]], planted)
    assert pk.level == "structure" and pk.dim == 4 and np.array_equal(pk.ids, np.arange(480) + 1000)
    with pytest.raises(AssertionError, match="without a GPU"):
        index.density_peaks(k=3, bandwidth=1.0)  # the device route asks the device
    with pytest.raises(ValueError, match="exactly one"):
        index.density_peaks()
    with pytest.raises(ValueError, match="at least 1 row"):
        LatentIndex(model, "structure").density_peaks(k=1, bandwidth=1.0, route="host")


def test_cli_takes_the_peaks_flags():
    spec = importlib.util.spec_from_file_location("predict_model_cli", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parser().parse_args(["some_dir", "--peaks", "4", "--peaks-level", "structure", "--peaks-bandwidth", "2.5", "--peaks-out", "peaks.npz",
                                 "--density", "index.npz", "--density-bandwidth", "1.5"])
    assert (a.peaks, a.peaks_level, a.peaks_bandwidth, a.peaks_out, a.density, a.density_bandwidth) == (4, "structure", 2.5, "peaks.npz", "index.npz", 1.5)
    d = cli.parser().parse_args(["some_dir"])
    assert (d.peaks, d.peaks_level, d.peaks_bandwidth, d.peaks_out, d.density, d.density_bandwidth) == (0, "atom", 0.0, "", "", 0.0)
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--peaks-level", "bond"])
    for bad in (["--peaks", "-1"], ["--peaks-out", "x.npz"], ["--peaks-bandwidth", "2"], ["--peaks", "2", "--peaks-bandwidth", "-1"],
                ["--density", "index.npz"], ["--density-bandwidth", "2"]):  # before the model's folder is read
        with pytest.raises(SystemExit):
            cli.main(cli.parser().parse_args(["no_such_model_dir"] + bad))
