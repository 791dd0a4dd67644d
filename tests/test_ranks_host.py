"""Host tests of the exact neighbour ranks and the map scores on top of them (scann_index_ranks' twin scann_ranks_host;
LatentIndex.map_quality's host route map_quality_rows_host; choose_perplexity_rows_host): the twin against the NumPy restatement of the
definition (tests/rank_ref.py) byte for byte -- coincident rows beyond the probe count, non-finite rows, an overflowing distance, probes
that are -1, the query itself, ineligible or repeated, a shuffled qpos with repeats, thread counts --; the permutation and the search's
places; trustworthiness and continuity against scikit-learn on tie-free rows; curves, means and samples; the argument checks; the header;
choose_perplexity on planted blobs.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import abi_checks
import rank_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dim", [2, 3, 130])
@pytest.mark.parametrize("N", [1, 2, 3, 65, 300])
def test_twin_equals_the_definition(hip_lib, N, dim):
    from scann import _hip

    rows = rr.pathological_pool(N, dim)
    for m in (1, 31, 32):
        probe = rr.probe_lists(N, N, m, seed=m)
        got = _hip.ranks_host(rows, probe, dist2=True)
        rr.same(got, rr.ranks(rows, probe), "N %d dim %d m %d" % (N, dim, m))
        assert "dist2" not in _hip.ranks_host(rows, probe) and _hip.ranks_host(rows, probe)["rank"].tobytes() == got["rank"].tobytes()
        none = (probe < 0) | (probe == np.arange(N)[:, None]) | ~rr.eligible(rows)[np.maximum(probe, 0)] | ~rr.eligible(rows)[:, None]
        assert (got["rank"][none] == -1).all() and np.isposinf(got["dist2"][none]).all() and (got["rank"][~none] >= 0).all()
    if N >= 65:
        # qpos shuffled with repeats: the rows of the full answer, in the order asked
        q = np.random.default_rng(N + dim).integers(0, N, 90).astype(np.int32)
        q[:6] = [10, 11, 61, 62, 20, 20]
        probe = rr.probe_lists(N, 90, 31, seed=5, qpos=q)
        part = _hip.ranks_host(rows, probe, q, dist2=True)
        rr.same(part, rr.ranks(rows, probe, q), "a qpos subset")
        assert (part["rank"][:2] == -1).all()                                    # ineligible queries
        d = _hip.ranks_host(rows, np.array([[62, 61]], np.int32), np.array([61], np.int32), dist2=True)
        assert np.isposinf(d["dist2"][0, 0]) and d["rank"][0, 0] >= 0 and d["rank"][0, 1] == -1  # +inf is an ordinary distance


def test_ties_beyond_the_probe_count(hip_lib):
    """40 coincident rows: from inside the run every other row of it is at distance 0, and the positions alone rank them"""
    from scann import _hip

    rows = rr.pathological_pool(70, 3)
    run = np.arange(20, 60, dtype=np.int32)
    q = np.array([20, 37, 59, 5], np.int32)
    probe = np.stack([run[:32], run[8:], np.full(32, 44, np.int32), run[:32]])
    got = _hip.ranks_host(rows, probe, q, dist2=True)
    rr.same(got, rr.ranks(rows, probe, q), "the coincident run")
    assert got["rank"][0].tolist() == [-1] + list(range(31))                     # seen from 20: 21 has rank 0
    assert got["rank"][1].tolist() == [r - 20 - (r > 37) if r != 37 else -1 for r in run[8:]]
    assert (got["rank"][2] == 44 - 20).all() and (got["dist2"][:3][got["rank"][:3] >= 0] == 0).all()   # the same probe 32 times
    assert np.array_equal(np.diff(got["rank"][3]), np.ones(31)) and len(set(got["dist2"][3].tolist())) == 1  # equal distance from outside


def test_thread_count_does_not_enter(hip_lib):
    from scann import _hip

    rows = rr.pathological_pool(300, 130)
    probe = rr.probe_lists(300, 300, 31, seed=2)
    one = _hip.ranks_host(rows, probe, threads=1, dist2=True)
    for threads in (3, 16):
        rr.same(_hip.ranks_host(rows, probe, threads=threads, dist2=True), one, "%d threads" % threads)


def test_all_other_rows_form_a_permutation(hip_lib):
    from scann import _hip

    rows = rr.pathological_pool(300, 3)
    n_el = int(rr.eligible(rows).sum())
    for i in (0, 20, 45, 61, 299):
        probe = rr.all_others(300, i)
        r = _hip.ranks_host(rows, probe, np.full(len(probe), i, np.int32))["rank"].reshape(-1)
        assert sorted(r[r >= 0].tolist()) == list(range(n_el - 1)) and (r < 0).sum() == probe.size - (n_el - 1), i


def test_the_search_places_have_their_ranks(hip_lib):
    from scann import _hip
    from scann.models import latent_index as li

    rng = np.random.default_rng(4)
    rows = rng.standard_normal((300, 20)).astype(np.float32)
    rows[100:140] = rows[100]                                                   # 40 coincident rows: the dropped place is not always the row's own
    pos, d2 = li.neighbour_graph_host(rows)
    got = _hip.ranks_host(rows, pos, dist2=True)
    assert (got["rank"] == np.arange(31)).all() and got["dist2"].tobytes() == d2.tobytes()


# ---- the scores ----

@pytest.fixture(scope="module")
def tie_free():
    X = rr.tie_free_rows(300, 3, 1000, seed=1)
    Y = rr.tie_free_rows(300, 2, 1000, seed=2, base=X[:, :2], jitter=300)
    return X, Y


def test_trustworthiness_and_continuity_are_scikit_learns(hip_lib, tie_free):
    """On tie-free integer rows every distance is exact in fp32 and fp64, so scikit-learn's ordering is the definition's.  Measured with
    this construction: the difference is 0.0 at every k, trustworthiness 0.81 .. 0.85, continuity 0.91 .. 0.93"""
    from sklearn.manifold import trustworthiness

    from scann.models import latent_index as li

    X, Y = tie_free
    assert rr.has_no_ties(X) and rr.has_no_ties(Y)                              # the precondition, on the input
    for k in (1, 5, 15, 31):
        q = li.map_quality_rows_host(X, Y, k=k)
        t, c = trustworthiness(X.astype(np.float64), Y.astype(np.float64), n_neighbors=k), trustworthiness(
            Y.astype(np.float64), X.astype(np.float64), n_neighbors=k)
        print("k %d: trustworthiness %.15f (sklearn %+.3e), continuity %.15f (sklearn %+.3e)" % (k, q["trustworthiness"], t - q["trustworthiness"],
                                                                                               q["continuity"], c - q["continuity"]))
        assert abs(q["trustworthiness"] - t) <= 1e-12 and abs(q["continuity"] - c) <= 1e-12, k
        assert 0.5 < q["trustworthiness"] < 1.0 and 0.5 < q["continuity"] < 1.0


def test_scores_are_the_formulas_on_the_restated_ranks(hip_lib, tie_free):
    from scann.models import latent_index as li

    X, Y = tie_free
    pos_x, pos_y = li.neighbour_graph_host(X)[0], li.neighbour_graph_host(Y)[0]
    want_latent, want_map = rr.ranks(X, pos_y)["rank"], rr.ranks(Y, pos_x)["rank"]
    q = li.map_quality_rows_host(X, Y, k=7)
    assert np.array_equal(q["rank_latent"], want_latent) and np.array_equal(q["rank_map"], want_map)
    ref = rr.scores(want_latent, want_map, 300, 7)
    for key, v in ref.items():
        assert np.allclose(q[key], v, rtol=0, atol=1e-13), key
    assert np.array_equal(q["false_neighbours"], (want_latent[:, :7] >= 7).sum(axis=1))
    assert np.array_equal(q["missed_neighbours"], (want_map[:, :7] >= 7).sum(axis=1))
    assert q["false_neighbours"].sum() == q["missed_neighbours"].sum()          # the two k-neighbour graphs have as many edges
    assert q["lcmc"] == q["neighbour_overlap"] - 7 / 299.0 and q["k"] == 7 and q["n_rows"] == 300
    ks = np.arange(1, 32)
    rnx = (299 * q["qnx_curve"] - ks) / (299 - ks)
    assert abs(q["rnx_auc"] - np.sum(rnx / ks) / np.sum(1.0 / ks)) <= 1e-15
    # a map that is the rows themselves is perfect
    same = li.map_quality_rows_host(X, X, k=15)
    assert same["trustworthiness"] == 1.0 and same["continuity"] == 1.0 and same["neighbour_overlap"] == 1.0 and same["rnx_auc"] == 1.0
    assert not same["false_neighbours"].any() and (same["rank_latent"] == np.arange(31)).all()


def test_curves_means_and_samples(hip_lib, tie_free):
    from scann.models import latent_index as li

    X, Y = tie_free
    full = li.map_quality_rows_host(X, Y, k=15)
    assert full["ks"].tolist() == list(range(1, 32)) and full["position"].tolist() == list(range(300))
    for k in (1, 2, 15, 30, 31):
        at = li.map_quality_rows_host(X, Y, k=k)
        for name, curve in (("trustworthiness", "trustworthiness_curve"), ("continuity", "continuity_curve"), ("neighbour_overlap", "qnx_curve")):
            assert at[name] == full[curve][k - 1] == at[curve][k - 1], (name, k)
    for name in ("trustworthiness", "continuity", "overlap"):
        total = full["neighbour_overlap" if name == "overlap" else name]
        assert abs(np.mean(full["row_" + name]) - total) <= 1e-14, name
    for sample in (40, np.array([299, 0, 17, 17, 3], np.int32)):
        part = li.map_quality_rows_host(X, Y, k=15, sample=sample, seed=3)
        p = part["position"]
        assert len(p) == (40 if isinstance(sample, int) else 5)
        for key in ("row_trustworthiness", "row_continuity", "row_overlap", "false_neighbours", "missed_neighbours", "rank_latent", "rank_map"):
            assert part[key].tobytes() == full[key][p].tobytes(), key
        assert abs(part["trustworthiness"] - np.mean(full["row_trustworthiness"][p])) <= 1e-14
    assert np.array_equal(li.map_quality_rows_host(X, Y, sample=40, seed=3)["position"], li.map_quality_rows_host(X, X, sample=40, seed=3)["position"])
    # the graph handed in is the graph computed; a result dict and a tuple are read like an array
    graph = li.neighbour_graph_host(X)
    for coords in ({"coords": Y}, {"coordinates": Y}, ({"coords": Y}, None)):
        again = li.map_quality_rows_host(X, coords, k=15, graph=graph)
        assert all(np.asarray(again[key]).tobytes() == np.asarray(v).tobytes() for key, v in full.items())
    # a small index: K = N - 2, and the curves end where 2N - 3k' - 1 is no longer positive
    small = li.map_quality_rows_host(X[:9], Y[:9], k=2)
    assert small["ks"].tolist() == list(range(1, 8)) and np.isfinite(small["trustworthiness_curve"][:5]).all()
    assert np.isnan(small["trustworthiness_curve"][5:]).all() and np.isfinite(small["qnx_curve"]).all()


def test_argument_errors_name_the_argument(hip_lib, tie_free):
    from scann import _hip
    from scann.models import latent_index as li

    X, Y = tie_free
    rows = X[:20]
    ok = np.zeros((20, 3), np.int32)
    for probe, q, word in ((np.zeros((20, 33), np.int32), None, "m 33 outside 1 .. 32"), (np.zeros((20, 0), np.int32), None, "m 0 outside"),
                           (np.zeros((19, 3), np.int32), None, r"shape \[20, m\]"), (np.zeros((20, 3), np.float32), None, "integer positions"),
                           (np.where(np.arange(60).reshape(20, 3) == 7, 20, 0), None, r"probe\[7\] = 20 outside -1 .. 19"),
                           (np.where(np.arange(60).reshape(20, 3) == 8, -2, 0), None, r"probe\[8\] = -2 outside -1 .. 19"),
                           (ok[:2], np.array([3, 20]), r"qpos\[1\] = 20 outside 0 .. 19"), (ok[:2], np.array([[3, 2]]), "one-dimensional")):
        with pytest.raises(ValueError, match=word):
            _hip.ranks_host(rows, probe, q)
    with pytest.raises(ValueError, match="threads"):
        _hip.ranks_host(rows, ok, threads=-1)
    with pytest.raises(ValueError, match="rows of shape"):
        _hip.ranks_host(rows[0], ok)
    # the C twin refuses by itself
    lib, P = hip_lib, _hip._ptr
    out = np.full((20, 3), 7, np.int32)
    bad = ok.copy()
    bad[4, 1] = 20
    assert lib.scann_ranks_host(P(rows), 20, 3, None, 0, P(ok), 0, 0, P(out), None) == -1
    assert lib.scann_ranks_host(P(rows), 20, 3, None, 0, P(bad), 3, 0, P(out), None) == -1
    assert lib.scann_ranks_host(P(rows), 20, 3, None, 0, None, 3, 0, P(out), None) == -1
    assert lib.scann_ranks_host(P(rows), 20, 3, None, 0, P(ok), 3, 0, None, None) == -1
    assert lib.scann_ranks_host(P(rows), 20, 3, P(np.array([20], np.int32)), 1, P(ok), 3, 0, P(out), None) == -1
    assert (out == 7).all()
    assert lib.scann_ranks_host(P(rows), 0, 3, None, 0, None, 3, 0, None, None) == 0          # an empty pool
    assert lib.scann_ranks_host(P(rows), 20, 3, None, 0, P(ok), 3, 0, P(out), None) == 0 and (out[1:] >= 0).all()
    # the scores
    for kw, word in ((dict(k=0), "k must be"), (dict(k=32), "k must be"), (dict(k=True), "k must be"), (dict(k=1.5), "k must be"),
                     (dict(sample=0), "sample"), (dict(sample=[300]), "sample"), (dict(sample=301), "only 300 rows"), (dict(seed=-1), "seed")):
        with pytest.raises(ValueError, match=word):
            li.map_quality_rows_host(X, Y, **kw)
    with pytest.raises(ValueError, match="2N - 3k - 1"):
        li.map_quality_rows_host(X[:9], Y[:9], k=6)
    with pytest.raises(ValueError, match="k must be an integer in 1 .. 7"):
        li.map_quality_rows_host(X[:9], Y[:9], k=8)
    with pytest.raises(ValueError, match="one row per row"):
        li.map_quality_rows_host(X, Y[:-1])
    with pytest.raises(ValueError, match="coords: row 5 has a non-finite"):
        li.map_quality_rows_host(X, np.where(np.arange(300)[:, None] == 5, np.nan, Y))
    with pytest.raises(ValueError, match="non-finite component"):
        li.map_quality_rows_host(np.where(np.arange(300)[:, None] == 5, np.inf, X), Y)
    with pytest.raises(ValueError, match="coords"):
        li.map_quality_rows_host(X, {"y": Y})
    for ps in ([], [10, 5], [5, 5], [1], [16], "a"):
        with pytest.raises(ValueError, match="perplexities"):
            li.choose_perplexity_rows_host(X, ps)


def test_header_and_python_agree(hip_lib):
    from scann import _hip

    abi_checks.declared("int scann_index_ranks(scann_handle_t* h, scann_index_t* pool, const int32_t* qpos /* host [nq] positions, or NULL: all N rows, nq "
                        "ignored */, int64_t nq, const int32_t* probe /* host [nq * m] positions, -1: unused */, int32_t m, int32_t* rank /* [nq * m] */, "
                        "float* dist2 /* [nq * m] or NULL */);",
                        "int scann_ranks_host(const float* rows, int64_t n, int64_t dim, const int32_t* qpos, int64_t nq, const int32_t* probe, int32_t m, "
                        "int32_t threads, int32_t* rank, float* dist2);",
                        "a row is eligible iff all its components are finite", "exactly the chain of scann_knn_distsq with row i as q",
                        "dist2 ascending, then position ascending", "strictly less than j's key", "the nearest other row has rank 0",
                        "gets rank -1 and dist2 +inf", "equal probes get equal ranks", "a qpos subset gives the rows of the full answer",
                        "leave-self-out answer from scann_index_query has rank p", "a permutation of 0 .. n_eligible - 2",
                        "on the query slicing or on a thread count", "#define SCANN_RANKS_MAX_PROBES 32", "#define SCANN_RANKS_SLICE 262144",
                        "#define SCANN_ABI_VERSION 1")
    P, I, L = C.c_void_p, C.c_int32, C.c_int64
    sig = abi_checks.signatures({
        "scann_index_ranks": (C.c_int, [P, P, P, L, P, I, P, P]),
        "scann_ranks_host": (C.c_int, [P, L, L, P, L, P, I, I, P, P])})
    for name in sig:
        assert hasattr(hip_lib, name), name
    assert _hip.RANKS_MAX_PROBES == 32 and _hip.RANKS_SLICE == 262144


# ---- the sweep over perplexities ----

def test_choose_perplexity_on_planted_blobs(hip_lib):
    import silhouette_ref as sr
    from scann.models import latent_index as li

    rows, _ = sr.blobs(40, 6, 2, seed=8)
    table, emb = li.choose_perplexity_rows_host(rows, [5, 10], k=10, iterations=(30, 60))
    assert table["perplexity"] == [5.0, 10.0, "linear"] and all(len(table[c]) == 3 for c in li.MAP_QUALITY_COLUMNS + ("kl",))
    assert np.isnan(table["kl"][2]) and np.isfinite(table["kl"][:2]).all() and (table["neighbour_overlap"] > 0).all()
    best = int(np.argmax(table["neighbour_overlap"][:2]))                        # (argmax: the first among equals, i.e. the lower perplexity)
    assert table["best_perplexity"] == table["perplexity"][best] == emb.perplexity
    assert np.array_equal(emb.coordinates, table["best"]["coords"]) and table["quality"]["neighbour_overlap"] == table["neighbour_overlap"][best]
    # every row of the table is the score of that map by itself, the graph shared or not
    for i, p in enumerate((5, 10)):
        res, _ = li.embed_rows_host(rows, perplexity=p, iterations=(30, 60))
        q = li.map_quality_rows_host(rows, res, k=10)
        assert all(q[c] == table[c][i] for c in li.MAP_QUALITY_COLUMNS) and res["kl"] == table["kl"][i]
    # the tie rule, on maps that score alike: the lower perplexity stays
    same = {c: 0.5 for c in li.MAP_QUALITY_COLUMNS}
    t, e = li.choose_perplexity_run(lambda p: ({"coords": p, "kl": 0.0}, p), lambda c: dict(same), lambda: None, [3.0, 7.0, 9.0])
    assert t["best_perplexity"] == 3.0 and e == 3.0
    t, e = li.choose_perplexity_run(lambda p: ({"coords": p, "kl": 0.0}, p),
                                    lambda c: dict(same, neighbour_overlap=0.9 if c in (7.0, 9.0) else 0.5), lambda: None, [3.0, 7.0, 9.0])
    assert t["best_perplexity"] == 7.0 and e == 7.0 and t["perplexity"] == [3.0, 7.0, 9.0, "linear"]
