"""Host tests of the silhouette of a labelled latent index (scann_index_silhouette's twin scann_silhouette_host, LatentIndex.silhouette's
host route, cluster_scores, choose_k): the twin against the NumPy restatement of the definition (tests/silhouette_ref.py) bit for bit --
unlabelled rows, an empty cluster, a singleton, non-finite and coincident rows, both metrics, a qpos subset, thread counts --; against
scikit-learn's silhouette_samples on fp64 copies; the range error and the chosen shift; the argument checks; choose_k on planted blobs;
header, ctypes table and library agree.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import abi_checks
import silhouette_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("euclidean", "sqeuclidean")


def twin_equals_reference(rows, lab, n_clusters, metric, qpos=None, what=""):
    from scann import _hip

    shift = sr.shift_for(rows, metric)
    got = _hip.silhouette_host(rows, lab, n_clusters, qpos, metric, shift, table=True)
    sr.same(got, sr.silhouette(rows, lab, n_clusters, qpos, metric == "sqeuclidean", shift), what)
    assert got["count"].dtype == np.int64 and got["sums"].dtype == np.int64 and got["other"].dtype == np.int32
    return got, shift


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [3, 130])
@pytest.mark.parametrize("N", [1, 2, 65, 700])
def test_twin_equals_the_definition(hip_lib, N, dim, metric):
    from scann import _hip

    rows, lab = sr.pathological_case(N, dim)
    full, shift = twin_equals_reference(rows, lab, 5, metric, what="N %d dim %d %s" % (N, dim, metric))
    cnt = sr.counting_rows(rows, lab)
    assert full["count"][3] == 0 and full["count"].sum() == cnt.sum()
    assert np.isnan(full["a"][~cnt]).all() and (full["other"][~cnt] == -1).all() and (full["sums"][~cnt] == -1).all()
    if N >= 2:
        assert full["count"][4] == 1 and full["a"][N - 1] == 0.0        # the singleton
    if N >= 60:
        assert (full["sums"][cnt, 3] == 0).all() and not (full["other"][cnt] == 3).any()  # the empty cluster is nobody's neighbour
        assert np.isfinite(full["b"][cnt]).all() and np.array_equal(full["sums"][40], full["sums"][47])  # coincident rows of one cluster
        # a subset of the queries, in any order and with a repeat, gives the rows of the full answer
        q = np.array([N - 1, 0, 10, 41, 41, 5, 64], np.int32)
        part, _ = twin_equals_reference(rows, lab, 5, metric, q, "a qpos subset")
        for key in ("a", "b", "other", "sums"):
            assert np.array_equal(part[key], full[key][q], equal_nan=key in "ab"), key
        # the thread count is no part of the result
        one = _hip.silhouette_host(rows, lab, 5, None, metric, shift, table=True, threads=1)
        many = _hip.silhouette_host(rows, lab, 5, None, metric, shift, table=True, threads=16)
        for key in one:
            assert one[key].tobytes() == many[key].tobytes() == full[key].tobytes(), key


@pytest.mark.parametrize("metric", METRICS)
def test_copies_of_a_cluster_tie_to_the_lower_label(hip_lib, metric):
    """small integers: clusters 1 and 3 are copies of each other, so from cluster 0 and 2 both are equally far: b names cluster 1"""
    rng = np.random.default_rng(4)
    base = rng.integers(-4, 5, (30, 6)).astype(np.float32)
    near = rng.integers(-4, 5, (20, 6)).astype(np.float32) + np.float32(40.0)
    far = rng.integers(-4, 5, (9, 6)).astype(np.float32) - np.float32(300.0)
    rows = np.concatenate([near, base, far, base])
    lab = np.concatenate([np.zeros(20), np.ones(30), np.full(9, 2), np.full(30, 3)]).astype(np.int32)
    got, _ = twin_equals_reference(rows, lab, 4, metric)
    assert np.array_equal(got["sums"][:20, 1], got["sums"][:20, 3])
    assert (got["other"][:20] == 1).all() and (got["other"][50:59] == 1).all()
    assert (got["other"][20:50] == 3).all() and (got["b"][20:50] <= got["a"][20:50] * 30 / 29).all()  # the copy is as near as the own cluster
    assert (got["other"][59:] == 1).all()
    # all rows coincident: every distance 0, every silhouette 0 by the rule for max(a, b) == 0
    from scann.models import latent_index as li

    same = np.tile(base[:1], (10, 1))
    r = li.silhouette_rows_host(same, np.arange(10) % 2, metric=metric)
    assert (r["a"] == 0).all() and (r["b"] == 0).all() and (r["silhouette"] == 0).all() and r["score"] == 0.0 and r["shift"] == 126


def test_one_cluster_and_no_counting_row(hip_lib):
    from scann.models import latent_index as li

    rows, _ = sr.pathological_case(65, 3)
    r = li.silhouette_rows_host(rows, np.zeros(65, np.int32), table=True)
    fin = np.isfinite(rows).all(axis=1)
    assert np.isnan(r["b"]).all() and (r["other"] == -1).all() and (r["a"][fin] > 0).all() and np.isnan(r["silhouette"]).all()
    assert np.isnan(r["score"]) and r["size"].tolist() == [int(fin.sum())] and (r["sums"][fin] > 0).all()
    r = li.silhouette_rows_host(rows, np.full(65, -1), n_clusters=3)
    assert np.isnan(r["a"]).all() and r["size"].tolist() == [0, 0, 0] and np.isnan(r["cluster_score"]).all()
    r = li.silhouette_rows_host(np.zeros((0, 4), np.float32), np.zeros(0, np.int32))
    assert r["position"].shape == (0,) and r["size"].tolist() == [0] and np.isnan(r["score"])


SKLEARN_SETS = [dict(n_per=250, dim=8, k=4, seed=1), dict(n_per=175, dim=130, k=4, seed=2, spread=0.3),
                dict(n_per=300, dim=5, k=3, seed=3, spread=0.01, offset=100.0)]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", SKLEARN_SETS)
def test_rows_agree_with_scikit_learn(hip_lib, case, metric):
    """|s - s_sklearn| <= 2e-5 for every row, dim <= 130, against silhouette_samples on fp64 copies of the fp32 rows.  The bound is
    derived, not measured: each term carries at most about (dim + 3) 2^-24 relative error from the fp32 chain and the root, plus 2^-31 of
    the largest term from the fixed point, and s at most doubles it: 2 x 133 x 6e-8 = 1.6e-5.  A NumPy restatement measured 1.3e-6 at
    worst over three 700-1,000-row sets, one of them offset by 100 with spread 0.01."""
    metrics = pytest.importorskip("sklearn.metrics")
    from scann.models import latent_index as li

    rows, lab = sr.blobs(**case)
    r = li.silhouette_rows_host(rows, lab, metric=metric)
    want = metrics.silhouette_samples(rows.astype(np.float64), lab, metric=metric)
    err = np.abs(r["silhouette"] - want)
    print("%s %s: %d rows, shift %d, worst |ds| %.3g, min |s| %.3g, score %.6f" % (case, metric, len(rows), r["shift"], err.max(), np.abs(want).min(),
                                                                                  r["score"]))
    assert np.abs(want).min() > 0.05  # the rows are far from where s could change sign
    assert err.max() <= 2e-5
    assert abs(r["score"] - want.mean()) <= 2e-5 and np.array_equal(r["position"], np.arange(len(rows)))
    for c in range(case["k"]):
        assert abs(r["cluster_score"][c] - want[lab == c].mean()) <= 2e-5
    # a sample: the sampled rows' values are those of the full answer, the positions the generator's, sorted
    s = li.silhouette_rows_host(rows, lab, sample=50, seed=7, metric=metric)
    pos = np.sort(np.random.default_rng(7).choice(len(rows), 50, replace=False))
    assert np.array_equal(s["position"], pos) and np.array_equal(s["silhouette"], r["silhouette"][pos]) and s["shift"] == r["shift"]
    e = li.silhouette_rows_host(rows, lab, sample=pos[::-1].copy(), metric=metric)
    assert np.array_equal(e["silhouette"], r["silhouette"][pos[::-1]]) and e["score"] == s["score"]


def spanning_rows(dim=3):
    """rows that span the bound their column ranges give: every column is +-0.99, so f_j = 0 and the largest distance, 1.98 sqrt(dim),
    is more than half of the power of two above the bound 2 sqrt(dim)"""
    a = np.float32(0.99)
    rows = np.array([[a] * dim, [-a] * dim] * 20, np.float32)
    return rows, (np.arange(40) // 2 % 2).astype(np.int32)


@pytest.mark.parametrize("metric", METRICS)
def test_range_error_and_the_chosen_shift(hip_lib, metric):
    from scann import _hip
    from scann.models import latent_index as li

    rows, lab = spanning_rows()
    shift = sr.shift_for(rows, metric)
    assert shift == (28 if metric == "euclidean" else 26)
    ok = _hip.silhouette_host(rows, lab, 2, None, metric, shift, table=True)
    sr.same(ok, sr.silhouette(rows, lab, 2, None, metric == "sqeuclidean", shift))
    assert 2 ** 29 < ok["sums"].max() // 10 <= 2 ** 30                 # (ten rows of a cluster are at the far end) the largest term is within a factor of two of the 2^30 aimed at
    assert li.silhouette_rows_host(rows, lab, metric=metric)["shift"] == shift
    for s in (shift + 2, 126):
        with pytest.raises(_hip.ScannHipError, match="RANGE"):
            _hip.silhouette_host(rows, lab, 2, None, metric, s)
        with pytest.raises(sr.OutOfRange):
            sr.silhouette(rows, lab, 2, None, metric == "sqeuclidean", s)
    # exactly 2^31 is still a term: two rows at distance 2 (4 squared) with shift 30 (29)
    pair = np.array([[1.0, 0.0], [-1.0, 0.0], [1.0, 0.0]], np.float32)
    edge = 30 if metric == "euclidean" else 29
    r = _hip.silhouette_host(pair, [0, 1, 0], 2, None, metric, edge, table=True)
    assert r["sums"].tolist() == [[0, 2 ** 31], [2 ** 32, 0], [0, 2 ** 31]]
    with pytest.raises(_hip.ScannHipError, match="RANGE"):
        _hip.silhouette_host(pair, [0, 1, 0], 2, None, metric, edge + 1)
    # a distance that overflows is out of range at any shift, and the automatic shift refuses such rows by name
    big = np.array([[3e19, 0.0], [-3e19, 0.0], [0.0, 1.0]], np.float32)
    with pytest.raises(_hip.ScannHipError, match="RANGE"):
        _hip.silhouette_host(big, [0, 1, 0], 2, None, metric, -126)
    with pytest.raises(ValueError, match="not finite in fp32"):
        li.silhouette_rows_host(big, [0, 1, 0], metric=metric)
    # rows that do not count raise nothing: their terms are no terms of the call
    big[0, 0], big[1, 1] = 1e19, np.nan     # (4e19 from row 1, which no longer counts; 1e19 from row 2: its square is finite)
    assert _hip.silhouette_host(big, [0, 1, 0], 2, None, metric, -126)["count"].tolist() == [2, 0]


def test_argument_errors_name_the_argument(hip_lib):
    from scann import _hip
    from scann.models import latent_index as li

    rows, lab = sr.pathological_case(65, 3)
    for shift in (-127, 127, 1.0, True, None):
        with pytest.raises(ValueError, match="shift"):
            _hip.silhouette_host(rows, lab, 5, None, "euclidean", shift)
    for bad in (lab[:-1], lab.astype(np.float32), lab[:, None], "abc"):
        with pytest.raises(ValueError, match="labels"):
            _hip.silhouette_host(rows, bad, 5)
    with pytest.raises(ValueError, match=r"labels\[64\] = 4 outside -1 \.\. 3"):
        _hip.silhouette_host(rows, lab, 4)
    low = lab.copy()
    low[7] = -2
    with pytest.raises(ValueError, match=r"labels\[7\] = -2"):
        _hip.silhouette_host(rows, low, 5)
    for c in (0, 1025, 2.0, True):
        with pytest.raises(ValueError, match="n_clusters"):
            _hip.silhouette_host(rows, np.zeros(65, np.int32), c)
    with pytest.raises(ValueError, match="at most 1024 clusters"):
        li.silhouette_rows_host(rows, np.arange(65) * 16)       # labels up to 1024: 1025 clusters
    for q, word in ((np.array([0, 65]), r"qpos\[1\] = 65"), (np.array([-1]), r"qpos\[0\] = -1"), (np.zeros((2, 2), np.int32), "qpos"),
                    (np.array([0.5]), "qpos")):
        with pytest.raises(ValueError, match=word):
            _hip.silhouette_host(rows, lab, 5, q)
    with pytest.raises(ValueError, match="metric"):
        _hip.silhouette_host(rows, lab, 5, None, "cosine")
    with pytest.raises(ValueError, match="threads"):
        _hip.silhouette_host(rows, lab, 5, threads=-1)
    with pytest.raises(ValueError, match="rows"):
        _hip.silhouette_host(rows[0], lab, 5)
    for kw, word in ((dict(sample=0), "sample"), (dict(sample=2.5), "sample"), (dict(sample=True), "sample"), (dict(sample=[0, 65]), r"sample\[1\] = 65"),
                     (dict(sample=60), "only"), (dict(seed=-1), "seed"), (dict(metric="l1"), "metric"), (dict(n_clusters=4), "labels")):
        with pytest.raises(ValueError, match=word):
            li.silhouette_rows_host(rows, lab, **kw)
    with pytest.raises(ValueError, match="route"):
        li.silhouette_route("gpu")
    for ks in ((), (0, 2), (2, 1025), (2.5,), 3, "ab"):
        with pytest.raises(ValueError, match="ks"):
            li.choose_k_rows_host(rows, ks)


def test_the_c_twin_refuses_bad_arguments_itself(hip_lib):
    """the twin's own checks, behind Python's: SCANN_ERR_INVALID (-1)"""
    from scann import _hip

    P = _hip._ptr
    rows, lab = sr.pathological_case(65, 3)
    lab = lab.astype(np.int32)
    cnt, a, b, other = np.full(5, 7, np.int64), np.full(65, 7.0), np.full(65, 7.0), np.full(65, 7, np.int32)
    q = np.array([1, 2], np.int32)

    def call(rows=P(rows), n=65, dim=3, labels=P(lab), c=5, qpos=None, nq=0, shift=0, threads=0, counts=P(cnt), a=P(a), b=P(b), other=P(other)):
        return hip_lib.scann_silhouette_host(rows, n, dim, labels, c, qpos, nq, 0, shift, threads, counts, a, b, other, None)

    bad_q, bad_lab = np.array([1, 65], np.int32), np.where(np.arange(65) == 9, 5, lab).astype(np.int32)
    for kw in (dict(rows=None), dict(n=-1), dict(dim=0), dict(labels=None), dict(c=0), dict(c=1025), dict(shift=127), dict(shift=-127),
               dict(threads=-1), dict(counts=None), dict(a=None), dict(b=None), dict(other=None), dict(qpos=P(q), nq=-1),
               dict(qpos=P(bad_q), nq=2), dict(labels=P(bad_lab))):
        assert call(**kw) == -1, kw
    assert (cnt == 7).all() and (a == 7).all() and (other == 7).all()
    assert call() == 0 and call(qpos=P(q), nq=2) == 0 and call(n=0, rows=None, labels=None, a=None, b=None, other=None) == 0
    assert cnt.tolist() == [0, 0, 0, 0, 0]


def test_header_and_python_agree(hip_lib):
    from scann import _hip

    flat = abi_checks.header()
    abi_checks.declared("int scann_index_silhouette(scann_handle_t* h, scann_index_t* pool, const int32_t* labels /* host [N], -1 .. C-1 */, int32_t C, "
                        "const int32_t* qpos /* host [nq] positions, or NULL: all N rows */, int64_t nq, int32_t squared, int32_t shift, "
                        "int64_t* counts /* [C] */, double* a /* [nq] */, double* b /* [nq] */, int32_t* other /* [nq] */, "
                        "int64_t* sums /* [nq * C] or NULL */);",
                        "int scann_silhouette_host(const float* rows, int64_t n, int64_t dim, const int32_t* labels, int32_t C, const int32_t* qpos, "
                        "int64_t nq, int32_t squared, int32_t shift, int32_t threads, int64_t* counts, double* a, double* b, int32_t* other, int64_t* sums);",
                        "t = llrintf(ldexpf(e, shift)), round to nearest even", "ties to the lower c", "a qpos subset gives the rows of the full answer",
                        "No tree is part of the definition", "#define SCANN_ABI_VERSION 1")
    P, I, L = C.c_void_p, C.c_int32, C.c_int64
    sig = abi_checks.signatures({
        "scann_index_silhouette": (C.c_int, [P, P, P, I, P, L, I, I, P, P, P, P, P]),
        "scann_silhouette_host": (C.c_int, [P, L, L, P, I, P, L, I, I, I, P, P, P, P, P])})
    for name in sig:
        assert hasattr(hip_lib, name), name
    assert _hip.KMEANS_MAX_K == 1024 and "#define SCANN_KMEANS_MAX_K 1024" in flat


def fp64_cluster_result(rows, lab, k):
    """a ``cluster``-shaped result in fp64: the exact means as centres, fp64 distances"""
    rows = rows.astype(np.float64)
    centre = np.stack([rows[lab == c].mean(axis=0) for c in range(k)])
    d = np.sqrt(((rows - centre[lab]) ** 2).sum(axis=1))
    return {"label": lab, "distance": d, "centre": centre, "size": np.bincount(lab, minlength=k), "inertia": float((d ** 2).sum())}


def test_cluster_scores_agree_with_scikit_learn(hip_lib):
    metrics = pytest.importorskip("sklearn.metrics")
    from scann.models import latent_index as li

    for case, k in ((dict(n_per=200, dim=7, k=4, seed=5, spread=0.4), 4), (dict(n_per=90, dim=30, k=6, seed=6, spread=1.5), 6)):
        rows, planted = sr.blobs(**case)
        lab = (planted + (np.arange(len(rows)) % 11 == 0)) % k      # not the best labelling: some rows sit in the wrong cluster
        got = li.cluster_scores(fp64_cluster_result(rows, lab, k))
        ch = metrics.calinski_harabasz_score(rows.astype(np.float64), lab)
        db = metrics.davies_bouldin_score(rows.astype(np.float64), lab)
        print("CH %.12g against %.12g, DB %.12g against %.12g" % (got["calinski_harabasz"], ch, got["davies_bouldin"], db))
        assert abs(got["calinski_harabasz"] - ch) <= 1e-9 * ch and abs(got["davies_bouldin"] - db) <= 1e-9 * db
    # from a k-means result: the fp32 centres and distances carry the same indices to fp32 accuracy; an empty cluster is left out
    res = li.cluster_rows_host(rows, 6)
    got = li.LatentIndex.cluster_scores(res)
    ch = metrics.calinski_harabasz_score(rows.astype(np.float64), res["label"])
    db = metrics.davies_bouldin_score(rows.astype(np.float64), res["label"])
    assert abs(got["calinski_harabasz"] - ch) <= 1e-4 * ch and abs(got["davies_bouldin"] - db) <= 1e-4 * db
    res = fp64_cluster_result(rows, lab, k)
    res["size"] = np.append(res["size"], 0)
    res["centre"] = np.concatenate([res["centre"], np.zeros((1, 30))])
    assert li.cluster_scores(res) == li.cluster_scores(fp64_cluster_result(rows, lab, k))
    one = li.cluster_scores(fp64_cluster_result(rows, np.zeros(len(rows), np.int64), 1))
    assert np.isnan(one["calinski_harabasz"]) and np.isnan(one["davies_bouldin"])


def test_choose_k_finds_the_planted_blobs(hip_lib):
    from scann.models import latent_index as li

    rows, planted = sr.blobs(n_per=200, dim=6, k=4, seed=11, spread=0.1)
    r = li.choose_k_rows_host(rows, (8, 2, 3, 4, 6, 4))
    print("k %s score %s CH %s DB %s" % (r["k"], np.round(r["score"], 4), np.round(r["calinski_harabasz"], 1), np.round(r["davies_bouldin"], 3)))
    assert r["k"].tolist() == [2, 3, 4, 6, 8] and r["best_k"] == 4 and r["score"].argmax() == 2
    assert r["best"]["size"].tolist() == [200] * 4 and r["silhouette"]["score"] == r["score"][2] > 0.8
    # each planted blob is one cluster
    assert len(set(zip(planted.tolist(), r["best"]["label"].tolist()))) == 4
    assert r["calinski_harabasz"].argmax() == 2 and r["davies_bouldin"].argmin() == 2 and r["converged"].all()
    assert (np.diff(r["inertia"]) < 0).all() and [len(s) for s in r["size"]] == [2, 3, 4, 6, 8]
    # every entry is what the single calls give
    res = li.cluster_rows_host(rows, 6)
    sil = li.silhouette_rows_host(rows, res["label"], n_clusters=6)
    assert r["score"][3] == sil["score"] and r["inertia"][3] == res["inertia"]
    # a sampled sweep picks the same k
    s = li.choose_k_rows_host(rows, (2, 3, 4, 6, 8), sample=100, seed=3)
    assert s["best_k"] == 4 and len(s["silhouette"]["position"]) == 100 and abs(s["score"][2] - r["score"][2]) < 0.05


def test_choose_k_ties_go_to_the_smaller_k(hip_lib):
    from scann.models import latent_index as li

    scores = {2: float("nan"), 3: 0.5, 5: 0.7, 7: 0.7, 9: 0.1}
    res = {"label": np.zeros(4, np.int32), "distance": np.zeros(4), "centre": np.zeros((1, 2)), "size": np.array([4]), "inertia": 0.0, "n_iter": 1,
           "converged": True}
    r = li.choose_k_run(lambda k: dict(res, k=k), lambda lab, k: {"score": scores[k]}, [2, 3, 5, 7, 9])
    assert r["best_k"] == 5 and r["best"]["k"] == 5 and np.isnan(r["score"][0])
    r = li.choose_k_run(lambda k: dict(res, k=k), lambda lab, k: {"score": float("nan")}, [2, 3])
    assert r["best_k"] == 2
    # two k with bit-equal scores from real rows: k = 1 twice is one k; the copies of a clustering score alike
    rows, _ = sr.blobs(n_per=40, dim=3, k=2, seed=1)
    assert li.choose_k_rows_host(rows, (1, 1))["k"].tolist() == [1] and np.isnan(li.choose_k_rows_host(rows, (1,))["score"][0])
