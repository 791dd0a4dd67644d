"""Host tests of the k-means clustering (scann_index_kmeans / scann_kmeans_host, LatentIndex.cluster, LatentClustering, HipModel.cluster /
assign): the host twin against the NumPy restatement of the definition (tests/kmeans_ref.py) over the kernel's distance chain and, on
small-integer rows with many ties, over the chain restated in NumPy alone; planted cases (NaN / inf rows, equal initial centres, all rows equal, k = N, k = 1, max_iter = 0, the
stop rule, columns of very different scale); invariance under a permutation of the rows; header, ctypes table and library agree; null
and bad arguments; the kernels use no scratch and keep out of the other kernels' name census; the Python layer on a stand-in engine;
predict_model.py takes --cluster.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import abi_checks
import kmeans_ref
import scann_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_host(rows, init, max_iter, stop=0, dist2=None, label=""):
    """scann_kmeans_host == the NumPy restatement: labels, dist2 bits, centre bits, sizes, n_iter, converged; and the certificate"""
    from scann import _hip

    got = _hip.kmeans_host(rows, init, max_iter, stop)
    want = kmeans_ref.kmeans(rows, init, max_iter, stop, dist2 or _hip.knn_dist2_matrix)
    kmeans_ref.same(got, want, label)
    kmeans_ref.certificate(rows, got, dist2 or _hip.knn_dist2_matrix, stop)
    assert got["dist2"].dtype == np.float32 and got["centre"].dtype == np.float32 and got["centre"].shape == np.shape(init)
    assert got["n_iter"] <= max_iter
    return got


# ---- the host twin against the restated definition ----

@pytest.mark.parametrize("N,dim,k", [(100, 128, 7), (255, 1, 2), (257, 130, 5), (1000, 3, 64)])
def test_host_twin_against_the_definition_on_random_rows(hip_lib, N, dim, k):
    from scann import _hip

    rng = np.random.default_rng(N * 7 + dim * 3 + k)
    rows = rng.standard_normal((N, dim)).astype(np.float32)
    rows[N // 2:N // 2 + 4] = rows[3]  # ties
    init = rows[_hip.kcenter_host(rows, None, k)["position"]]
    got = check_host(rows, init, 8, label="random N %d dim %d k %d" % (N, dim, k))
    assert got["n_iter"] >= 2  # the update really ran
    for max_iter in (0, 1, 3):
        check_host(rows, init, max_iter, label="random, max_iter %d" % max_iter)
    check_host(rows, init, 8, stop=N // 20, label="random, stop")


@pytest.mark.parametrize("dim", [1, 3, 33])
def test_host_twin_on_small_integers_against_numpy_alone(hip_lib, dim):
    """small-integer rows, many exact ties, and a reference that needs nothing of the library: the chain in NumPy alone"""
    rng = np.random.default_rng(dim)
    rows = rng.integers(-4, 5, (400, dim)).astype(np.float32)
    for k in (1, 5, 40):
        init = rows[rng.choice(400, k, replace=False)]
        check_host(rows, init, 6, dist2=kmeans_ref.fma_dist2, label="integers dim %d k %d" % (dim, k))


def within_bound_of_the_mean(rows, member, centre, e):
    """the update's value before its last rounding, ldexp(S / n, e_j - 30) in fp64, lies within 2^(e_j - 31) of the fp64 mean in every
    column, and the centre is that value rounded to fp32"""
    S = kmeans_ref.quantise(rows[member], e).sum(axis=0, dtype=np.int64)
    v = np.ldexp(S.astype(np.float64) / np.float64(member.sum()), (e - 30).astype(np.int32))
    mean = rows[member].astype(np.float64).mean(axis=0)
    assert np.all(np.abs(v - mean) <= np.ldexp(1.0, (e - 31).astype(np.int32))), (v, mean, e)
    assert np.array_equal(_bits(centre), _bits(v.astype(np.float32)))


def planted_cases():
    """(name, rows, init, max_iter, stop_changed, check(result)) -- shared with tests/test_gpu_cluster.py"""
    rng = np.random.default_rng(11)
    cases = []

    # NaN / +-inf rows get -1 / +inf and move no centre
    rows = (rng.standard_normal((120, 16)) * 3).astype(np.float32)
    clean = rows.copy()
    bad = [3, 58, 90]
    rows[3, 8] = np.nan
    rows[58, 0] = np.inf
    rows[90, 15] = -np.inf
    init = rows[[0, 10, 20, 30]]

    def non_finite(r, rows=rows, clean=clean, bad=bad, init=init):
        from scann import _hip

        assert np.all(r["label"][bad] == -1) and np.all(np.isposinf(r["dist2"][bad])) and r["size"].sum() == len(rows) - len(bad)
        keep = np.setdiff1d(np.arange(len(rows)), bad)
        alone = _hip.kmeans_host(clean[keep], init, 8)  # the same rows without the three
        assert np.array_equal(_bits(r["centre"]), _bits(alone["centre"])) and np.array_equal(r["label"][keep], alone["label"])
        assert r["n_iter"] == alone["n_iter"]
    cases.append(("non-finite rows", rows, init, 8, 0, non_finite))

    # two equal initial centres: in the assignment to them the higher index stays empty (size 0), and the update leaves it unchanged.
    # (From then on it differs from its moved twin and may win rows: so the loop is cut at t = 0 and at t = 1.)
    rows = rng.standard_normal((200, 5)).astype(np.float32)
    init = rows[[4, 9, 4, 30]]

    def twins0(r, init=init):
        assert r["size"][2] == 0 and not np.any(r["label"] == 2) and np.array_equal(_bits(r["centre"]), _bits(init)) and r["size"][0] > 0
    cases.append(("equal initial centres, t = 0", rows, init, 0, 0, twins0))

    def twins1(r, init=init):
        assert r["n_iter"] == 1 and np.array_equal(_bits(r["centre"][2]), _bits(init[2])) and not np.array_equal(_bits(r["centre"][0]), _bits(init[0]))
    cases.append(("equal initial centres, one update", rows, init, 1, 0, twins1))

    # all rows equal
    rows = np.tile(np.float32([1.5, -2.0, 0.25]), (150, 1))
    init = np.float32([[0, 0, 0], [1.5, -2.0, 0.25], [1.5, -2.0, 0.25]])

    def equal(r, rows=rows):
        assert np.all(r["label"] == 1) and not r["dist2"].any() and r["size"].tolist() == [0, 150, 0] and r["converged"]
        assert np.array_equal(_bits(r["centre"][1]), _bits(rows[0]))
    cases.append(("all rows equal", rows, init, 8, 0, equal))

    # k = N: every row its own centre
    rows = rng.standard_normal((37, 6)).astype(np.float32)

    def own(r, rows=rows):
        assert r["label"].tolist() == list(range(37)) and np.all(r["size"] == 1) and r["converged"] and r["n_iter"] == 1
        # the mean of one row is the row on the grid of the integer sums: at most 2^(e_j - 31) off in column j
        step = np.ldexp(1.0, (kmeans_ref.exponents(rows) - 31).astype(np.int32))
        assert np.all(np.abs(r["centre"].astype(np.float64) - rows) <= step) and np.all(r["dist2"] <= (step ** 2).sum() * (1 + 2.0 ** -20))
    cases.append(("k = N", rows, rows.copy(), 8, 0, own))

    # k = 1: the centre is the mean after one update
    rows = rng.standard_normal((300, 4)).astype(np.float32)

    def one(r, rows=rows):
        assert np.all(r["label"] == 0) and r["n_iter"] == 1 and r["converged"] and r["size"].tolist() == [300]
        assert np.allclose(r["centre"][0], rows.astype(np.float64).mean(axis=0), rtol=0, atol=2.0 ** -20)
    cases.append(("k = 1", rows, rows[:1].copy(), 8, 0, one))

    # max_iter = 0: a pure assignment to the given centres
    rows = rng.standard_normal((260, 7)).astype(np.float32)
    init = rows[[1, 100, 200]]

    def pure(r, init=init):
        assert r["n_iter"] == 0 and not r["converged"] and np.array_equal(_bits(r["centre"]), _bits(init)) and r["size"].sum() == 260
    cases.append(("max_iter = 0", rows, init, 0, 0, pure))

    # stop_changed large enough to stop at t = 1 (changed_0 = N > stop; changed_1 <= N - 1)
    def early(r):
        assert r["n_iter"] == 1 and r["converged"]
    cases.append(("stop at t = 1", rows, init, 8, 259, early))

    # stop_changed >= N: stops at t = 0, converged
    def at_once(r, init=init):
        assert r["n_iter"] == 0 and r["converged"] and np.array_equal(_bits(r["centre"]), _bits(init))
    cases.append(("stop at t = 0", rows, init, 8, 260, at_once))

    # columns of very different scale: each column's centre lands within 2^(e_j - 31) of the fp64 mean
    rows = rng.standard_normal((500, 3)).astype(np.float32)
    rows[:, 0] *= np.float32(1e-6)
    rows[:, 2] *= np.float32(1e6)
    init = rows[[0, 1, 2, 3]]

    def scales(r, rows=rows):
        e = kmeans_ref.exponents(rows)
        assert e[0] < -15 and e[2] > 15 and r["n_iter"] >= 1
        assert r["converged"]  # so label_t == label_{t-1}: the centres are U of the returned labels
        for c in range(4):
            assert r["size"][c] > 0
            within_bound_of_the_mean(rows, r["label"] == c, r["centre"][c], e)
    cases.append(("column scales", rows, init, 30, 0, scales))
    return cases


def test_planted_cases(hip_lib):
    for name, rows, init, max_iter, stop, check in planted_cases():
        check(check_host(rows, init, max_iter, stop, label=name))


def test_integer_sums_are_within_their_bound_of_the_fp64_mean(hip_lib):
    """one update of the twin from a known labelling, columns of scales 1e-15 .. 1e-3 beside one of scale 1: the header's bound"""
    from scann import _hip

    rng = np.random.default_rng(5)
    rows = (rng.standard_normal((4000, 6)) * np.float32([1e-15, 1, 1e-3, 3e-9, 1e-12, 1e-7])).astype(np.float32)
    label = (np.arange(4000) % 3).astype(np.int32)
    rows[:, 1] = np.float32(label) - 1 + rows[:, 1] * np.float32(0.01)  # column 1 decides the label: near -1, 0 and 1
    init = np.zeros((3, 6), np.float32)
    init[:, 1] = [-1, 0, 1]
    e = kmeans_ref.exponents(rows)
    first = _hip.kmeans_host(rows, init, 0)
    assert np.array_equal(first["label"], label)
    got = _hip.kmeans_host(rows, init, 1)
    assert got["n_iter"] == 1
    for c in range(3):
        within_bound_of_the_mean(rows, label == c, got["centre"][c], e)


def test_result_does_not_depend_on_the_order_of_the_rows(hip_lib):
    from scann import _hip

    rng = np.random.default_rng(21)
    rows = rng.standard_normal((700, 20)).astype(np.float32)
    rows[300:305] = rows[2]
    init = rows[_hip.kcenter_host(rows, None, 9)["position"]]
    base = _hip.kmeans_host(rows, init, 10)
    assert base["n_iter"] >= 2
    for seed in range(3):
        perm = np.random.default_rng(seed).permutation(len(rows))
        p = _hip.kmeans_host(rows[perm], init, 10)
        assert np.array_equal(p["label"], base["label"][perm]) and np.array_equal(_bits(p["dist2"]), _bits(base["dist2"][perm]))
        assert np.array_equal(_bits(p["centre"]), _bits(base["centre"])) and np.array_equal(p["size"], base["size"]) and p["n_iter"] == base["n_iter"]


def test_empty_pool_and_no_eligible_row(hip_lib):
    from scann import _hip

    init = np.float32([[1, 2], [3, 4]])
    e = _hip.kmeans_host(np.zeros((0, 2), np.float32), init, 4)
    assert e["n_iter"] == 0 and e["converged"] and np.array_equal(e["centre"], init) and not e["size"].any() and e["label"].shape == (0,)
    e = check_host(np.full((3, 2), np.nan, np.float32), init, 4, label="no eligible row")
    assert e["n_iter"] == 0 and e["converged"] and np.all(e["label"] == -1) and np.array_equal(e["centre"], init)


# ---- ABI ----

def test_header_ctypes_and_library_agree(hip_lib):
    import ctypes as C

    from scann import _hip

    h = abi_checks.header()
    abi_checks.declared("int64_t scann_index_kmeans(scann_handle_t* h, scann_index_t* pool, int32_t k, const float* init /* [k * dim] or NULL */, "
                        "const int32_t* init_pos /* [k] positions in pool, or NULL */, int32_t max_iter, int64_t stop_changed, "
                        "int32_t* labels /* [N] */, float* dist2 /* [N] or NULL */, float* centres /* [k * dim] */, "
                        "int64_t* sizes /* [k] or NULL */, int32_t* converged /* or NULL */);",
                        "int64_t scann_kmeans_host(const float* rows, int64_t n, int64_t dim, int32_t k, const float* init, int32_t max_iter, "
                        "int64_t stop_changed, int32_t* labels, float* dist2, float* centres, int64_t* sizes, int32_t* converged);",
                        "#define SCANN_KMEANS_MAX_K 1024")
    assert "#define SCANN_ABI_VERSION 1" in h and hip_lib.scann_abi_version() == 1
    assert _hip.KMEANS_MAX_K == 1024
    P = C.c_void_p
    sig = abi_checks.signatures({
        "scann_index_kmeans": (C.c_int64, [P, P, C.c_int32, P, P, C.c_int32, C.c_int64, P, P, P, P, P]),
        "scann_kmeans_host": (C.c_int64, [P, C.c_int64, C.c_int64, C.c_int32, P, C.c_int32, C.c_int64, P, P, P, P, P])})
    assert hasattr(hip_lib, "scann_index_kmeans") and hasattr(hip_lib, "scann_kmeans_host")


def test_null_and_bad_arguments_are_errors_not_crashes(hip_lib):
    from scann import _hip

    P = _hip._ptr
    rows = np.arange(6, dtype=np.float32).reshape(3, 2)
    init = rows[:2].copy()
    lab, d2, cen, size = np.zeros(3, np.int32), np.zeros(3, np.float32), np.zeros((2, 2), np.float32), np.zeros(2, np.int64)
    assert hip_lib.scann_index_kmeans(None, None, 2, P(init), None, 3, 0, P(lab), P(d2), P(cen), P(size), None) == -1
    assert hip_lib.scann_index_kmeans(None, None, 2, None, None, 3, 0, None, None, None, None, None) == -1
    k = hip_lib.scann_kmeans_host
    assert k(None, 3, 2, 2, P(init), 3, 0, P(lab), P(d2), P(cen), P(size), None) == -1     # rows null
    assert k(P(rows), 3, 2, 2, None, 3, 0, P(lab), P(d2), P(cen), P(size), None) == -1     # init null
    assert k(P(rows), 3, 2, 2, P(init), 3, 0, None, P(d2), P(cen), P(size), None) == -1    # labels null
    assert k(P(rows), 3, 2, 2, P(init), 3, 0, P(lab), P(d2), None, P(size), None) == -1    # centres null
    assert k(P(rows), 3, 0, 2, P(init), 3, 0, P(lab), P(d2), P(cen), P(size), None) == -1  # dim < 1
    assert k(P(rows), -1, 2, 2, P(init), 3, 0, P(lab), P(d2), P(cen), P(size), None) == -1
    assert k(P(rows), 3, 2, 0, P(init), 3, 0, P(lab), P(d2), P(cen), P(size), None) == -1  # k < 1
    assert k(P(rows), 3, 2, 1025, P(init), 3, 0, P(lab), P(d2), P(cen), P(size), None) == -1
    assert k(P(rows), 3, 2, 2, P(init), -1, 0, P(lab), P(d2), P(cen), P(size), None) == -1
    assert k(P(rows), 3, 2, 2, P(init), 3, -1, P(lab), P(d2), P(cen), P(size), None) == -1
    bad = init.copy()
    bad[1, 0] = np.nan
    assert k(P(rows), 3, 2, 2, P(bad), 3, 0, P(lab), P(d2), P(cen), P(size), None) == -1   # a non-finite initial centre
    assert k(P(rows), 3, 2, 2, P(init), 3, 0, P(lab), None, P(cen), None, None) >= 0       # dist2, sizes, converged may be null
    assert lab.tolist() == [0, 1, 1]
    for kw in (dict(max_iter=-1), dict(max_iter=2.5), dict(max_iter=True), dict(max_iter=None), dict(max_iter=3, stop_changed=-1),
               dict(max_iter=3, stop_changed=0.5)):
        with pytest.raises(ValueError):
            _hip.kmeans_host(rows, init, **kw)
    for bad_init in (bad, np.zeros((2, 3), np.float32), np.zeros((0, 2), np.float32), np.zeros(2, np.float32), np.zeros((1025, 2), np.float32), "x"):
        with pytest.raises(ValueError):
            _hip.kmeans_host(rows, bad_init, 3)
    for kw in (dict(k=0), dict(k=1025), dict(k=2.0), dict(k=True), dict(k=None)):
        with pytest.raises(ValueError):
            _hip.check_kmeans_args(kw["k"], 3, 0)
    assert _hip.check_kmeans_args(np.int64(4), np.int32(0), 7) == (4, 0, 7)


def test_kmeans_kernels_use_no_scratch_and_keep_their_names_apart(hip_lib):
    """the kernels of csrc/scann_kmeans.hip spill nothing, read from the built library's kernel descriptors; their names stay out of
    the name census the other host tests take"""
    from scann import _hip

    kern = {n: v for n, v in abi_checks.device_kernels(_hip.LIB_PATH).items() if "kmeans_" in n}
    for want in ("kmeans_prepare_kernel", "kmeans_gather_kernel", "kmeans_assign_kernel", "kmeans_sum_kernel", "kmeans_finalise_kernel"):
        assert sum(want in n for n in kern) == 1, (want, sorted(kern))
    assert len(kern) == 5, sorted(kern)
    for name, (scratch, vgpr) in kern.items():
        assert scratch == 0, (name, scratch, vgpr)
        for other in ("knn_", "kcenter_", "rollout_", "ablate_", "input_grad_kernel"):
            assert other not in name, name


# ---- the Python layer against a stand-in engine ----

def _model(cfg):
    """test_knn_host's stand-in engine (rows [s, 0, ...] per structure, [s, a, 0, ...] per atom), with index_select and index_kmeans
    answered by the NumPy restatements"""
    import kcenter_ref
    import test_knn_host as tk

    class StandIn(tk._StandIn):
        def index_select(self, pool_ix, ref_ix, m, stop_dist2=0.0):
            self.calls.append(("select", m, stop_dist2))
            pos, rad, cnt = kcenter_ref.select(pool_ix.rows, None, m, stop_dist2, kcenter_ref.exact_dist2)
            return {"position": pos, "id": pos.astype(np.int64), "atom": pos * 0 - 1, "radius2": rad, "count": cnt}

        def index_names(self, ix):
            return ix.ids.copy(), ix.atoms.copy()

        def index_kmeans(self, ix, init, max_iter=50, stop_changed=0):
            a = np.asarray(init)
            self.calls.append(("kmeans", "positions" if a.dtype.kind in "iu" else "centres", len(a), max_iter, stop_changed))
            cen = ix.rows[a] if a.dtype.kind in "iu" else a
            return kmeans_ref.kmeans(ix.rows, cen, max_iter, stop_changed, kmeans_ref.fma_dist2)

    m = tk._model(cfg)
    m.engine = StandIn(m.config)
    return m


def _batch(n=5, seed=2):
    cfg = so.default_config("qm9")
    inputs, _ = so.pad_batch(*so.synth_dataset(n, seed), g_update=True)
    return cfg, inputs


def test_python_layer_raises_before_any_upload(tmp_path):
    from scann.models import LatentClustering

    cfg, inputs = _batch(4)
    m = _model(cfg)
    for kw in (dict(k=0), dict(k=1025), dict(k=2.5), dict(k=None), dict(k=True), dict(k=2, max_iter=-1), dict(k=2, max_iter=1.5),
               dict(k=2, stop_changed=-1), dict(k=2, level="bond"), dict(k=2, batch_size=0), dict(k=2, init="random"),
               dict(k=2, init=np.full((2, 128), np.nan, np.float32)), dict(k=2, init=np.zeros((2, 5), np.float32))):
        with pytest.raises(ValueError):
            m.cluster(inputs, **kw)
    with pytest.raises(ValueError):
        m.assign(inputs, np.zeros((2, 128), np.float32))  # no LatentClustering
    with pytest.raises(ValueError):
        m.assign(inputs, LatentClustering(np.zeros((2, 64), np.float32), "atom"))  # another width
    with pytest.raises(ValueError):
        m.assign(inputs, LatentClustering(np.zeros((2, 128), np.float32), "atom"), batch_size=0)
    for bad in (dict(centres=np.zeros((0, 4), np.float32), level="atom"), dict(centres=np.zeros(4, np.float32), level="atom"),
                dict(centres=np.zeros((2, 4), np.float32), level="bond"), dict(centres=np.full((2, 4), np.inf, np.float32), level="atom"),
                dict(centres=np.zeros((2, 4), np.float32), level="atom", dim=5)):
        with pytest.raises(ValueError):
            LatentClustering(**bad)
    assert m.engine.uploads == 0 and not m.engine.calls and m.engine.created == 0
    pool = m.build_index(inputs)  # rows [s, 0, ...], s = 0 .. 3
    up = m.engine.uploads
    m.engine.calls.clear()
    for kw in (dict(k=0), dict(k=2, max_iter=-1), dict(k=2, stop_changed=-3), dict(k=2, init="farthest"), dict(k=2, init=[0, 1, 2]),
               dict(k=2, init=[0, 4]), dict(k=2, init=[-1, 2]), dict(k=2, init=np.zeros((3, 128), np.float32)),
               dict(k=2, init=np.zeros((2, 127), np.float32)), dict(k=2, init=np.full((2, 128), np.inf, np.float32))):
        with pytest.raises(ValueError):
            pool.cluster(**kw)
    assert not m.engine.calls
    with pytest.raises(ValueError):
        pool.cluster(5)  # 5 clusters need 5 eligible rows: the index has 4
    assert [c[0] for c in m.engine.calls] == ["select"]
    other = _model(so.default_config("qm9"))
    with pytest.raises(ValueError):
        other.cluster(pool, 2)  # another model's index
    cfg2 = so.default_config("qm9")
    cfg2["model"]["dense_out"] = 64
    LatentClustering(np.zeros((2, 128), np.float32), "structure").save(str(tmp_path / "c.npz"))
    with pytest.raises(ValueError):
        LatentClustering.load(_model(cfg2), str(tmp_path / "c.npz"))
    assert m.engine.uploads == up


def test_python_layer_init_forms_medoids_inertia_and_temporary_index():
    cfg, inputs = _batch(6)
    m = _model(cfg)
    pool = m.build_index(inputs, ids=[10, 11, 12, 13, 14, 15])  # rows [s, 0, ...], s = 0 .. 5
    m.engine.calls.clear()
    # "kcenter": the positions select(2) picks (0, then the farthest, 5) go to the call as positions
    r = pool.cluster(2)
    assert [c[:3] for c in m.engine.calls] == [("select", 2, 0.0), ("kmeans", "positions", 2)] and m.engine.calls[-1][3:] == (50, 0)
    assert sorted(r) == ["centre", "converged", "distance", "inertia", "label", "medoid_atom", "medoid_id", "medoid_position", "n_iter", "size"]
    assert r["label"].tolist() == [0, 0, 0, 1, 1, 1] and r["size"].tolist() == [3, 3] and r["converged"] and r["n_iter"] == 1
    assert r["centre"][:, 0].tolist() == [1.0, 4.0] and not r["centre"][:, 1:].any()
    assert r["distance"].dtype == np.float32 and r["distance"].tolist() == [1.0, 0.0, 1.0, 1.0, 0.0, 1.0] and r["inertia"] == 4.0
    assert r["medoid_position"].tolist() == [1, 4] and r["medoid_id"].tolist() == [11, 14] and r["medoid_atom"].tolist() == [-1, -1]
    assert r["label"].dtype == np.int32 and r["medoid_position"].dtype == np.int32 and r["medoid_id"].dtype == np.int64
    # positions, and centres: the same clustering
    for init, form in ((np.array([0, 5]), "positions"), ([0, 5], "positions"), (pool.rows()[0][[0, 5]], "centres")):
        q = pool.cluster(2, init=init, max_iter=7, stop_changed=0)
        assert m.engine.calls[-1] == ("kmeans", form, 2, 7, 0)
        assert np.array_equal(q["label"], r["label"]) and np.array_equal(q["centre"], r["centre"])
    # an empty cluster has no medoid; ties between members go to the earlier position
    init = np.zeros((3, 128), np.float32)
    init[0, 0], init[1, 0], init[2, 0] = 2.5, 2.5, 100.0
    q = pool.cluster(3, init=init, max_iter=0)
    assert q["label"].tolist() == [0] * 6 and q["size"].tolist() == [6, 0, 0]
    assert q["medoid_position"].tolist() == [2, -1, -1] and q["medoid_id"].tolist() == [12, -1, -1] and q["medoid_atom"].tolist() == [-1, -1, -1]
    assert q["n_iter"] == 0 and not q["converged"] and q["inertia"] == 2 * (6.25 + 2.25 + 0.25)
    # data instead of an index: indexed for the call, freed afterwards; atom level by default
    import test_knn_host as tk
    freed = []
    orig = tk._Ix.free
    tk._Ix.free = lambda self: freed.append(self)
    try:
        created = m.engine.created
        m.engine.seen = 0
        res, clustering = m.cluster(inputs, 2, batch_size=4)
        assert m.engine.created == created + 1 and len(freed) == 1
        assert clustering.level == "atom" and clustering.dim == 128 and clustering.k == 2 and np.array_equal(clustering.centres, res["centre"])
        assert res["size"].sum() == len(res["label"]) and np.all(res["medoid_atom"] >= 0)
        m.engine.seen = 0
        res, clustering = m.cluster(inputs, 2, level="structure", ids=[10, 11, 12, 13, 14, 15])
        assert len(freed) == 2 and clustering.level == "structure" and np.array_equal(res["label"], r["label"]) and res["medoid_id"].tolist() == [11, 14]
        res, clustering = m.cluster(pool, 2, level="atom")  # an index: its level counts
        assert len(freed) == 2 and clustering.level == "structure"
    finally:
        tk._Ix.free = orig


def test_clustering_save_load_and_assign_goes_through_nearest(tmp_path):
    from scann.models import LatentClustering
    from scann.models.scann_model import SCANN

    cfg, inputs = _batch(6)
    m = _model(cfg)
    pool = m.build_index(inputs)
    res, clustering = m.cluster(pool, 2)
    path = str(tmp_path / "kinds.npz")
    clustering.save(path)
    assert os.listdir(tmp_path) == ["kinds.npz"]
    loaded = LatentClustering.load(m, path)
    assert loaded.level == "structure" and loaded.dim == 128 and np.array_equal(_bits(loaded.centres), _bits(clustering.centres))
    m.engine.calls.clear()
    m.engine.seen = 0
    created = m.engine.created
    a = m.assign(inputs, loaded, batch_size=4)
    # one index of the centres, then nearest with k = 1, batch by batch
    assert m.engine.created == created + 1
    assert [c[0] for c in m.engine.calls] == ["query", "query"] and all(c[2] == 1 for c in m.engine.calls)
    assert sorted(a) == ["cluster", "distance", "predict_property"]
    assert a["cluster"].dtype == np.int32 and a["cluster"].tolist() == res["label"].tolist()
    assert a["distance"].dtype == np.float32 and a["distance"].tolist() == res["distance"].tolist() and a["predict_property"].shape == (6, 1)
    m.engine.seen = 0
    m.assign(inputs, loaded)
    assert m.engine.created == created + 1  # the centres' index is kept
    # atom level: padded atoms get -1 / 0
    m.engine.seen = 0
    res, atoms = m.cluster(inputs, 3, level="atom")
    m.engine.seen = 0
    a = m.assign(inputs, atoms)
    mask = np.asarray(inputs["atom_mask"]).reshape(6, -1) > 0
    assert a["cluster"].shape == mask.shape and np.array_equal(a["cluster"][mask], res["label"]) and np.all(a["cluster"][~mask] == -1)
    assert not a["distance"][~mask].any()
    # the facade passes through; predict_property in the target's units
    s = SCANN.__new__(SCANN)
    s.model = m
    s.mean, s.std = 2.0, -0.5
    m.engine.seen = 0
    b = s.assign(inputs, atoms)
    assert np.array_equal(b["cluster"], a["cluster"]) and np.array_equal(b["predict_property"], a["predict_property"] * -0.5 + 2.0)
    r2, c2 = s.cluster(pool, 2)
    assert np.array_equal(r2["label"], m.cluster(pool, 2)[0]["label"]) and isinstance(c2, LatentClustering)


def test_predict_model_cli_takes_cluster():
    pytest.importorskip("sklearn")
    spec = importlib.util.spec_from_file_location("predict_model_cli_cluster", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parser().parse_args(["some_dir", "--cluster", "30", "--cluster-level", "structure", "--cluster-iter", "9", "--cluster-out", "kinds.npz"])
    assert a.cluster == 30 and a.cluster_level == "structure" and a.cluster_iter == 9 and a.cluster_out == "kinds.npz"
    d = cli.parser().parse_args(["some_dir"])
    assert d.cluster == 0 and d.cluster_level == "atom" and d.cluster_iter == 50 and d.cluster_out == ""
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--cluster-level", "bond"])
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--cluster", "many"])
    for bad in (["--cluster", "-3"], ["--cluster", "1025"], ["--cluster", "3", "--cluster-iter", "-1"]):
        with pytest.raises(SystemExit):
            cli.main(cli.parser().parse_args(["some_dir"] + bad))
