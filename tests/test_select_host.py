"""Host tests of the greedy k-center selection (scann_index_select / scann_kcenter_host, LatentIndex.select, HipModel.select_diverse):
the host twin against the NumPy restatement of the definition (tests/kcenter_ref.py) over the kernel's distance chain and over exact
small-integer distances; planted cases (duplicates last with radius 0, NaN / inf rows never picked, all rows equal, m > N, an empty
reference, a reference row with a NaN, the stop rule); radius2 non-increasing; invariance under a permuted reference; header, ctypes
table and library agree; null arguments; the kernels use no scratch and keep out of the other kernels' name census; the Python layer on
a stand-in engine; predict_model.py takes --select.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import abi_checks
import kcenter_ref
import scann_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_host(rows, ref, m, stop=0.0, dist2=None, label=""):
    """scann_kcenter_host == the NumPy restatement, positions and radius2 bit for bit, tails included"""
    from scann import _hip

    got = _hip.kcenter_host(rows, ref, m, stop)
    pos, rad, cnt = kcenter_ref.select(rows, ref, m, stop, dist2 or _hip.knn_dist2_matrix)
    assert got["count"] == cnt, (label, got["count"], cnt)
    assert got["position"].dtype == np.int32 and got["radius2"].dtype == np.float32 and got["position"].shape == (m,)
    assert np.array_equal(got["position"], pos), label
    assert np.array_equal(_bits(got["radius2"]), _bits(rad)), label
    assert np.all(got["position"][cnt:] == -1) and np.all(np.isposinf(got["radius2"][cnt:]))
    r = got["radius2"][:cnt]
    assert np.all(r[1:] <= r[:-1]), label  # non-increasing
    return got


# ---- the host twin against the restated definition ----

@pytest.mark.parametrize("dim", [1, 3, 128, 130])
@pytest.mark.parametrize("with_ref", [False, True])
def test_host_twin_against_the_definition_on_random_rows(hip_lib, dim, with_ref):
    from scann import _hip

    rng = np.random.default_rng(dim * 2 + with_ref)
    n = 300
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows[50:60] = rows[7]  # duplicates
    ref = rng.standard_normal((40, dim)).astype(np.float32) if with_ref else None
    for m in (1, 17, n, n + 5):
        got = check_host(rows, ref, m, label="random dim %d m %d" % (dim, m))
        assert got["count"] == min(m, n)
        kcenter_ref.certificate(rows, ref, got["position"], got["radius2"], got["count"], _hip.knn_dist2_matrix, m=m)
    if not with_ref:
        assert check_host(rows, None, 3)["position"][0] == 0 and np.isposinf(check_host(rows, None, 3)["radius2"][0])


@pytest.mark.parametrize("dim", [1, 3, 64])
def test_host_twin_on_small_integers_where_numpy_is_exact(hip_lib, dim):
    """small-integer rows: plain NumPy squares and sums are the chain exactly, so the reference needs nothing of the library"""
    rng = np.random.default_rng(dim)
    rows = rng.integers(-8, 9, (200, dim)).astype(np.float32)
    ref = rng.integers(-8, 9, (30, dim)).astype(np.float32)
    for r in (None, ref):
        for m in (1, 40, 250):
            check_host(rows, r, m, dist2=kcenter_ref.exact_dist2, label="integers dim %d" % dim)
    # many ties: the order by position decides
    check_host(rows, ref, 60, stop=4.0, dist2=kcenter_ref.exact_dist2, label="integers, stop")


def planted(rng, dim=16, n=120):
    """rows with exact duplicates, a NaN row, a +inf row and a -inf row; -> (rows, positions of the non-finite rows, duplicates of row 5)"""
    rows = (rng.standard_normal((n, dim)) * 3).astype(np.float32)
    dup = [40, 77, 101]
    rows[dup] = rows[5]
    bad = [3, 58, 90]
    rows[3, dim // 2] = np.nan
    rows[58, 0] = np.inf
    rows[90, dim - 1] = -np.inf
    return rows, bad, dup


def test_duplicates_last_and_non_finite_rows_never(hip_lib):
    rng = np.random.default_rng(11)
    rows, bad, dup = planted(rng)
    n = len(rows)
    got = check_host(rows, None, n + 10, label="planted")
    cnt = got["count"]
    assert cnt == n - len(bad)  # every eligible row, once
    pos, r2 = got["position"][:cnt], got["radius2"][:cnt]
    assert not set(bad) & set(pos.tolist()) and len(set(pos.tolist())) == cnt
    # the duplicates of row 5 (and 5 itself): one of them at a positive radius, the others at the very end with radius 0, by position
    group = [5] + dup
    first = [p for p in pos if p in group][0]
    rest = sorted(p for p in group if p != first)
    assert first == 5 and pos[-3:].tolist() == rest and not r2[-3:].any() and np.all(r2[:-3] > 0)
    # with a reference that contains row 5 all four come last
    got = check_host(rows, rows[5:6] + 0, n, label="planted, reference")
    assert got["position"][got["count"] - 4:got["count"]].tolist() == sorted(group) and not got["radius2"][got["count"] - 4:got["count"]].any()


def test_all_rows_equal_m_beyond_n_and_empty_inputs(hip_lib):
    from scann import _hip

    rows = np.tile(np.float32([1.5, -2.0, 0.25]), (9, 1))
    got = check_host(rows, None, 12, label="all equal")
    assert got["count"] == 9 and got["position"][:9].tolist() == list(range(9))
    assert np.isposinf(got["radius2"][0]) and not got["radius2"][1:9].any()
    assert check_host(rows, None, 12, stop=1e-6)["count"] == 1  # the second pick's radius 0 lies below the threshold
    # an empty reference is no reference: first pick position 0, radius +inf
    a = _hip.kcenter_host(rows, np.zeros((0, 3), np.float32), 2)
    assert a["position"].tolist() == [0, 1] and np.isposinf(a["radius2"][0])
    # an empty pool returns 0
    e = _hip.kcenter_host(np.zeros((0, 3), np.float32), None, 4)
    assert e["count"] == 0 and np.all(e["position"] == -1) and np.all(np.isposinf(e["radius2"]))
    # a pool of non-finite rows only: nothing to pick
    e = _hip.kcenter_host(np.full((3, 2), np.nan, np.float32), None, 4)
    assert e["count"] == 0


def test_reference_rows_with_nan_are_ignored_and_its_order_does_not_matter(hip_lib):
    from scann import _hip

    rng = np.random.default_rng(3)
    rows = rng.standard_normal((150, 20)).astype(np.float32)
    ref = rng.standard_normal((25, 20)).astype(np.float32)
    base = check_host(rows, ref, 30, label="reference")
    dirty = np.concatenate([ref[:10], np.full((1, 20), 1.0, np.float32), ref[10:]])
    dirty[10, 4] = np.nan
    got = check_host(rows, dirty, 30, label="reference with a NaN row")
    assert np.array_equal(got["position"], base["position"]) and np.array_equal(_bits(got["radius2"]), _bits(base["radius2"]))
    # a reference of NaN rows only: as without a reference
    none = check_host(rows, None, 5)
    only = check_host(rows, np.full((2, 20), np.nan, np.float32), 5, label="NaN reference")
    assert np.array_equal(only["position"], none["position"]) and np.isposinf(only["radius2"][0])
    for seed in range(3):
        perm = np.random.default_rng(seed).permutation(len(ref))
        p = _hip.kcenter_host(rows, ref[perm], 30)
        assert np.array_equal(p["position"], base["position"]) and np.array_equal(_bits(p["radius2"]), _bits(base["radius2"]))


def test_stop_rule_ends_exactly_before_the_first_radius_below_it(hip_lib):
    rng = np.random.default_rng(8)
    rows = rng.standard_normal((200, 12)).astype(np.float32)
    ref = rng.standard_normal((10, 12)).astype(np.float32)
    full = check_host(rows, ref, 200, label="no stop")
    r2 = full["radius2"]
    for cut in (1, 2, 50, 199):
        if not r2[cut] < r2[cut - 1]:
            continue
        # a threshold between radius2[cut - 1] and radius2[cut]: exactly `cut` picks; at radius2[cut - 1] itself (not below it) as well
        for stop in (np.float32(0.5) * (r2[cut - 1] + r2[cut]), r2[cut - 1]):
            got = check_host(rows, ref, 200, stop=float(stop), label="stop %g" % stop)
            assert got["count"] == cut and np.array_equal(got["position"][:cut], full["position"][:cut])
            assert np.array_equal(_bits(got["radius2"][:cut]), _bits(r2[:cut]))
    assert check_host(rows, ref, 200, stop=float(np.nextafter(r2[0], np.float32(np.inf))))["count"] == 0
    assert check_host(rows, ref, 200, stop=-3.0)["count"] == 200  # <= 0: no threshold
    # without a reference the first radius is +inf: never below a threshold
    assert check_host(rows, None, 200, stop=1e30)["count"] == 1


# ---- ABI ----

def test_header_ctypes_and_library_agree(hip_lib):
    import ctypes as C

    from scann import _hip

    h = abi_checks.header()
    abi_checks.declared("int64_t scann_index_select(scann_handle_t* h, scann_index_t* pool, scann_index_t* reference /* or NULL */, int64_t m, "
                        "float stop_dist2, int32_t* pos, int64_t* ids, int32_t* atoms, float* radius2);",
                        "int64_t scann_kcenter_host(const float* rows, int64_t n, const float* ref, int64_t nr, int64_t dim, int64_t m, "
                        "float stop_dist2, int32_t* pos, float* radius2);")
    assert "#define SCANN_ABI_VERSION 1" in h and hip_lib.scann_abi_version() == 1
    P = C.c_void_p
    sig = abi_checks.signatures({
        "scann_index_select": (C.c_int64, [P, P, P, C.c_int64, C.c_float, P, P, P, P]),
        "scann_kcenter_host": (C.c_int64, [P, C.c_int64, P, C.c_int64, C.c_int64, C.c_int64, C.c_float, P, P])})
    assert hasattr(hip_lib, "scann_index_select") and hasattr(hip_lib, "scann_kcenter_host")


def test_null_and_bad_arguments_are_errors_not_crashes(hip_lib):
    from scann import _hip

    pos, r2 = np.zeros(4, np.int32), np.zeros(4, np.float32)
    rows = np.zeros((3, 2), np.float32)
    assert hip_lib.scann_index_select(None, None, None, 4, 0.0, None, None, None, None) == -1
    assert hip_lib.scann_index_select(None, None, None, 4, 0.0, _hip._ptr(pos), None, None, _hip._ptr(r2)) == -1
    k = hip_lib.scann_kcenter_host
    assert k(None, 3, None, 0, 2, 4, 0.0, _hip._ptr(pos), _hip._ptr(r2)) == -1          # rows null
    assert k(_hip._ptr(rows), 3, None, 0, 2, 4, 0.0, None, _hip._ptr(r2)) == -1         # pos null
    assert k(_hip._ptr(rows), 3, None, 2, 2, 4, 0.0, _hip._ptr(pos), None) == -1        # ref null with nr > 0
    assert k(_hip._ptr(rows), 3, None, 0, 2, 0, 0.0, _hip._ptr(pos), None) == -1        # m < 1
    assert k(_hip._ptr(rows), 3, None, 0, 0, 4, 0.0, _hip._ptr(pos), None) == -1        # dim < 1
    assert k(_hip._ptr(rows), -1, None, 0, 2, 4, 0.0, _hip._ptr(pos), None) == -1
    assert k(_hip._ptr(rows), 3, None, 0, 2, 4, float("nan"), _hip._ptr(pos), None) == -1
    assert k(_hip._ptr(rows), 3, None, 0, 2, 4, 0.0, _hip._ptr(pos), None) == 3          # radius2 may be null
    assert pos.tolist() == [0, 1, 2, -1]
    assert k(None, 0, None, 0, 2, 4, 0.0, _hip._ptr(pos), _hip._ptr(r2)) == 0 and np.all(pos == -1) and np.all(np.isposinf(r2))
    for bad in (dict(m=0), dict(m=-2), dict(m=2.5), dict(m=True), dict(m=None), dict(m=3, stop_dist2=float("nan")), dict(m=3, stop_dist2="x")):
        with pytest.raises(ValueError):
            _hip.kcenter_host(rows, None, **bad)
    with pytest.raises(ValueError):
        _hip.kcenter_host(rows, np.zeros((2, 3), np.float32), 2)


def test_kcenter_kernels_use_no_scratch_and_keep_their_names_apart(hip_lib):
    """the kernels of csrc/scann_select.hip spill nothing, read from the built library's kernel descriptors; their names stay out of
    the name census the other host tests take"""
    from scann import _hip

    kern = {n: v for n, v in abi_checks.device_kernels(_hip.LIB_PATH).items() if "kcenter_" in n}
    assert len(kern) == 2 and sum("kcenter_step_kernel" in n for n in kern) == 1 and sum("kcenter_prepare_kernel" in n for n in kern) == 1, sorted(kern)
    for name, (scratch, vgpr) in kern.items():
        assert scratch == 0, (name, scratch, vgpr)
        for other in ("knn_", "rollout_", "ablate_", "input_grad_kernel"):
            assert other not in name, name


# ---- the Python layer against a stand-in engine ----

def _model(cfg):
    """test_knn_host's stand-in engine (rows [s, 0, ...] per structure, [s, a, 0, ...] per atom), with index_select answered by the
    NumPy restatement over exact distances"""
    import test_knn_host as tk

    class StandIn(tk._StandIn):
        selects = 0

        def index_select(self, pool_ix, ref_ix, m, stop_dist2=0.0):
            self.selects += 1
            self.calls.append(("select", m, stop_dist2))
            pos, rad, cnt = kcenter_ref.select(pool_ix.rows, None if ref_ix is None else ref_ix.rows, m, stop_dist2, kcenter_ref.exact_dist2)
            ok = pos >= 0
            return {"position": pos, "id": np.where(ok, pool_ix.ids[np.maximum(pos, 0)], -1).astype(np.int64),
                    "atom": np.where(ok, pool_ix.atoms[np.maximum(pos, 0)], -1).astype(np.int32), "radius2": rad, "count": cnt}

    m = tk._model(cfg)
    m.engine = StandIn(m.config)
    return m


def _batch(n=5, seed=2):
    cfg = so.default_config("qm9")
    inputs, _ = so.pad_batch(*so.synth_dataset(n, seed), g_update=True)
    return cfg, inputs


def test_python_layer_raises_before_any_upload():
    from scann.models import LatentIndex

    cfg, inputs = _batch(4)
    m = _model(cfg)
    for kw in (dict(m=0), dict(m=-1), dict(m=2.5), dict(m=None), dict(m=True), dict(m=2, stop_distance=-1.0), dict(m=2, stop_distance=float("nan")),
               dict(m=2, stop_distance="far"), dict(m=2, level="bond"), dict(m=2, batch_size=0)):
        with pytest.raises(ValueError):
            m.select_diverse(inputs, **kw)
    with pytest.raises(ValueError):
        m.select_diverse(inputs, 2, reference=inputs)  # the pool itself
    assert m.engine.uploads == 0 and not m.engine.calls and m.engine.created == 0
    pool = m.build_index(inputs)
    atoms = m.build_index(inputs, level="atom")
    up = m.engine.uploads
    m.engine.calls.clear()
    for kw in (dict(m=0), dict(m=2, stop_distance=-0.5), dict(m=2, stop_distance=float("nan")), dict(m=2, reference=pool),
               dict(m=2, reference=atoms), dict(m=2, reference="an index")):
        with pytest.raises(ValueError):
            pool.select(**kw)
    other = _model(so.default_config("qm9"))
    foreign = other.build_index(inputs)
    with pytest.raises(ValueError):
        pool.select(2, reference=foreign)  # another model's
    with pytest.raises(ValueError):
        m.select_diverse(foreign, 2)
    with pytest.raises(ValueError):
        m.select_diverse(pool, 2, reference=atoms)  # another level
    cfg2 = so.default_config("qm9")
    cfg2["model"]["dense_out"] = 64
    narrow = LatentIndex(_model(cfg2), "structure")
    narrow.model = m  # (what a caller could do by hand: the width still gives it away)
    with pytest.raises(ValueError):
        pool.select(2, reference=narrow)
    assert m.engine.uploads == up and not m.engine.calls and m.engine.selects == 0


def test_python_layer_sqrt_truncation_and_temporary_indices():
    cfg, inputs = _batch(5)
    m = _model(cfg)
    pool = m.build_index(inputs, ids=[10, 11, 12, 13, 14])  # rows [s, 0, ...], s = 0 .. 4
    r = pool.select(3)
    assert sorted(r) == ["atom", "count", "neighbor_id", "position", "radius"]
    # position 0 first (radius inf), then the farthest (4, squared distance 16), then 2 (4)
    assert r["count"] == 3 and r["position"].tolist() == [0, 4, 2] and r["neighbor_id"].tolist() == [10, 14, 12] and r["atom"].tolist() == [-1, -1, -1]
    assert r["radius"].dtype == np.float32 and np.array_equal(r["radius"], np.float32([np.inf, 4.0, 2.0]))
    assert r["position"].dtype == np.int32 and r["neighbor_id"].dtype == np.int64
    # m beyond the rows: cut to the picks made
    r = pool.select(9)
    assert r["count"] == 5 and all(len(r[k]) == 5 for k in ("position", "neighbor_id", "atom", "radius"))
    # stop_distance is squared in fp32 for the call, and ends the run before the first radius below it
    r = pool.select(9, stop_distance=1.5)
    assert m.engine.calls[-1] == ("select", 9, 2.25) and r["position"].tolist() == [0, 4, 2] and len(r["radius"]) == 3
    assert pool.select(9, stop_distance=None)["count"] == 5 and m.engine.calls[-1] == ("select", 9, 0.0)
    # data instead of indices: indexed for the call (pool and reference), freed afterwards
    freed = []
    import test_knn_host as tk
    orig = tk._Ix.free
    tk._Ix.free = lambda self: freed.append(self)
    try:
        created = m.engine.created
        m.engine.seen = 0
        r = m.select_diverse(inputs, 2, reference=pool, batch_size=2)
        assert m.engine.created == created + 1 and len(freed) == 1
        # (the stand-in numbers the structures of later uploads on: the temporary pool's rows are s = 0 .. 4 again after seen = 0)
        assert r["count"] == 2 and not r["radius"].any()  # every row is in the reference: radius 0, by position
        assert r["position"].tolist() == [0, 1]
        m.engine.seen = 0
        r = m.select_diverse(inputs, 2, level="atom")
        assert m.engine.created == created + 2 and len(freed) == 2 and r["count"] == 2 and r["atom"][0] == 0
    finally:
        tk._Ix.free = orig


def test_scann_facade_passes_through():
    from scann.models.scann_model import SCANN

    cfg, inputs = _batch(4)
    s = SCANN.__new__(SCANN)
    s.model = _model(cfg)
    s.mean, s.std = 2.0, -0.5
    pool = s.build_index(inputs)
    a, b = s.select_diverse(pool, 3), s.model.select_diverse(pool, 3)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_predict_model_cli_takes_select():
    pytest.importorskip("sklearn")
    spec = importlib.util.spec_from_file_location("predict_model_cli_select", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parser().parse_args(["some_dir", "--select", "30", "--select-level", "atom", "--select-reference", "train.npz"])
    assert a.select == 30 and a.select_level == "atom" and a.select_reference == "train.npz"
    d = cli.parser().parse_args(["some_dir"])
    assert d.select == 0 and d.select_level == "structure" and d.select_reference == ""
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--select-level", "bond"])
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--select", "many"])
    with pytest.raises(SystemExit):
        cli.main(cli.parser().parse_args(["some_dir", "--select", "-3"]))
