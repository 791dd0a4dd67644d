"""Host tests of the Shapley values of atoms for the global pooling (scann_shapley, HipModel.atom_shapley): the permutation generator
(scann_shapley_permutation) against its NumPy restatement and for uniformity; the reference of tests/shapley_ref.py against itself -- the
mean over all n! walks equals the subset formula, efficiency, and v(S) for |S| >= 2 equals ablate_ref's insertion entries; the host
reduction (scann_shapley_reduce_host) against its NumPy restatement bit for bit; the C header, the ctypes table and the library agree; null
and bad arguments are errors; the Python layer refuses bad arguments before anything is uploaded, re-pads and de-normalises (stand-in
engine); the kernels of csrc/scann_shapley.hip use no scratch; predict_model.py takes --shapley.  No GPU."""
import importlib.util
import math
import os
import types

import numpy as np
import pytest

import abi_checks
import ablate_ref
import shapley_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the generator ----

def test_generator_gives_permutations_equal_to_the_restatement(hip_lib):
    from scann import _hip

    for n in range(1, 71):
        for seed, key, p in ((0, 0, 0), (7, 3, 5), (2 ** 64 - 1, 2 ** 63 + 11, 1000), (123456789, n, n)):
            got = _hip.shapley_permutation(seed, key, p, n)
            assert got.dtype == np.int32 and sorted(got.tolist()) == list(range(n)), (n, seed, key, p)
            assert np.array_equal(got, sr.permutation(seed, key, p, n)), (n, seed, key, p)


def test_generator_depends_on_seed_key_walk_and_size_only(hip_lib):
    from scann import _hip

    a = _hip.shapley_permutation(5, 9, 2, 40)
    assert np.array_equal(a, _hip.shapley_permutation(5, 9, 2, 40))
    # a buffer with other contents, other calls in between: the same walk
    out = np.full(40, -7, np.int32)
    _hip.shapley_permutation(1, 1, 1, 13)
    hip_lib.scann_shapley_permutation(5, 9, 2, 40, _hip._ptr(out))
    assert np.array_equal(out, a)
    for other in ((6, 9, 2, 40), (5, 10, 2, 40), (5, 9, 3, 40)):
        assert not np.array_equal(a, _hip.shapley_permutation(*other)), other
    assert not np.array_equal(a[:39], _hip.shapley_permutation(5, 9, 2, 39))
    # nothing is written for n <= 0, p < 0 or a null buffer
    out[:] = -7
    hip_lib.scann_shapley_permutation(5, 9, 2, 0, _hip._ptr(out))
    hip_lib.scann_shapley_permutation(5, 9, -1, 40, _hip._ptr(out))
    hip_lib.scann_shapley_permutation(5, 9, 2, 40, None)
    assert np.all(out == -7)


def test_generator_is_uniform_over_positions(hip_lib):
    """20,000 draws at n = 5 (walks p = 0 .. 199 of keys 0 .. 99): the count of every atom in every position within 5 standard deviations of
    uniform -- a binomial (N, 1 / 5)"""
    from scann import _hip

    n, N = 5, 20000
    count = np.zeros((n, n), dtype=np.int64)
    for key in range(100):
        for p in range(200):
            w = _hip.shapley_permutation(42, key, p, n)
            count[w, np.arange(n)] += 1
    sd = math.sqrt(N * (1 / n) * (1 - 1 / n))
    dev = np.abs(count - N / n) / sd
    print("largest deviation %.2f standard deviations" % dev.max())
    assert count.sum() == N * n and dev.max() <= 5.0, count


# ---- the reference against itself ----

def _rows(case, dtype=np.float64):
    cfg, w, inputs = sr.config_and_inputs(**(sr.CASES[case] if isinstance(case, str) else case))
    z, mol = ablate_ref.after_lc(cfg, w, inputs, dtype)
    return cfg, w, z, mol


@pytest.mark.parametrize("case", ["sizes", "sizes_no_ga_norm", dict(data="sizes", target="e_b")], ids=["sizes", "sizes_no_ga_norm", "sizes_e_b"])
def test_mean_over_all_walks_is_the_subset_formula_and_efficiency(case):
    cfg, w, z, mol = _rows(case)
    done = 0
    for s in range(len(mol) - 1):
        n = int(mol[s + 1] - mol[s])
        if n not in (2, 3, 5):
            continue
        zs = z[mol[s]:mol[s + 1]]
        v = sr.all_subsets(cfg, w, zs, np.float64)
        assert np.all(np.isfinite(v)), (case, n, v)
        phi = sr.exact_shapley(v)
        perms = sr.all_permutations(n)
        vals, base = sr.prefix_values(cfg, w, zs, np.array([0, n]), perms, np.float64)
        assert np.allclose(vals, sr.walk_values(v, perms), rtol=1e-12, atol=0)
        sh, se, full = sr.reduce(vals, perms, np.array([0, n]), base)
        scale = np.abs(phi).max()
        assert np.max(np.abs(sh - phi)) <= 1e-12 * scale, (case, n, sh, phi)
        # efficiency, on both
        assert abs(phi.sum() - (v[-1] - v[0])) <= 1e-12 * np.abs(v).max()
        assert abs(sh.sum() - (full[0] - base[0])) <= 1e-12 * np.abs(v).max()
        assert base[0] == v[0] and abs(full[0] - v[-1]) <= 1e-14 * abs(v[-1])
        done += 1
    assert done == 3


@pytest.mark.parametrize("case", ["sizes", "sizes_no_ga_norm"])
def test_values_of_two_atoms_and_more_are_the_insertion_entries(case):
    """along any order, v of the first k >= 2 atoms is ablate_ref's insertion entry k - 1; below, the convention: finite where the
    reference's use_ga_norm arithmetic is NaN -- except the one-atom structure, whose only set is the full one"""
    cfg, w, z, mol = _rows(case)
    rng = np.random.default_rng(4)
    order = np.concatenate([rng.permutation(int(n)) for n in np.diff(mol)]).astype(np.int32)
    vals, base = sr.prefix_values(cfg, w, z, mol, order[None], np.float64)
    with np.errstate(all="ignore"):
        ins, y = ablate_ref.ablate(cfg, w, z, mol, "insertion", order, np.float64)
    first = np.zeros(len(order), dtype=bool)
    first[mol[:-1]] = True
    # (to 1e-12: the oracle's einsum adds in another order for another number of kept sets per call)
    assert np.allclose(vals[0][~first], ins[~first], rtol=1e-12, atol=0)
    norm = cfg["model"]["use_ga_norm"]
    assert np.all(np.isnan(ins[first]) == norm)
    one = np.diff(mol) == 1
    assert np.array_equal(np.isnan(vals[0][first]), one & norm)
    assert np.all(np.isfinite(base))
    # the convention is the arithmetic without use_ga_norm: there the insertion entries agree from the first on
    if not norm:
        assert np.allclose(vals[0], ins, rtol=1e-12, atol=0)
    # ... and a single kept atom pools to its own row: v({i}) = head(k_i)
    s = 3
    zs = z[mol[s]:mol[s + 1]]
    wd = {k: np.asarray(v_, dtype=np.float64) for k, v_ in w.items()}
    import scann_oracle as so
    key = so.dense(zs, wd, "global_attention/key", np.dtype(np.float64))
    hk = ablate_ref.head(cfg, wd, key, np.dtype(np.float64))[:, 0]
    v1 = sr.v_sets(cfg, wd, zs, np.eye(len(zs), dtype=bool), np.dtype(np.float64))
    assert np.allclose(v1, hk, rtol=1e-12, atol=1e-14)
    assert np.isclose(base[s], ablate_ref.head(cfg, wd, np.zeros((1, key.shape[1])), np.dtype(np.float64))[0, 0], rtol=1e-13)


# ---- the host reduction ----

def _random_walks(rng, sizes, P):
    mol = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    perms = np.empty((P, mol[-1]), np.int32)
    for p in range(P):
        for s, n in enumerate(sizes):
            perms[p, mol[s]:mol[s + 1]] = rng.permutation(n)
    values = rng.standard_normal((P, mol[-1])).astype(np.float32) * np.float32(3.0)
    return mol, perms, values, rng.standard_normal(len(sizes))


@pytest.mark.parametrize("P", [1, 2, 7])
def test_host_reduce_equals_the_restatement_bit_for_bit(hip_lib, P):
    from scann import _hip

    rng = np.random.default_rng(100 + P)
    sizes = [1, 2, 0, 5, 33, 7]
    mol, perms, values, base = _random_walks(rng, sizes, P)
    values[:, mol[5]:mol[6]][P // 2, 3] = np.nan  # a NaN row: structure 5 only
    values[:, mol[1]] = np.inf
    sh, se, full = _hip.shapley_reduce_host(values, perms, mol, base)
    rsh, rse, rfull = sr.reduce(values, perms, mol, base)
    assert np.array_equal(_bits(sh), _bits(rsh)) and np.array_equal(_bits(se), _bits(rse)) and np.array_equal(_bits(full), _bits(rfull))
    assert np.all(np.isnan(sh[mol[5]:mol[6]]) == np.isin(np.arange(7), [perms[P // 2, mol[5] + 3], perms[P // 2, mol[5] + 4]]))
    assert np.all(np.isfinite(sh[mol[3]:mol[5]])) and full[2] == base[2]
    if P == 1:
        assert np.all(np.isnan(se))
    else:
        assert np.all(np.isfinite(se[mol[3]:mol[5]]))
        # efficiency of the reduction itself
        for s in (0, 3, 4):
            scale = max(float(np.abs(values[:, mol[s]:mol[s + 1]]).max()), abs(float(base[s])))
            assert abs(sh[mol[s]:mol[s + 1]].sum() - (full[s] - base[s])) <= 1e-9 * scale


# ---- ABI ----

def test_header_ctypes_and_library_agree(hip_lib):
    import ctypes as C

    from scann import _hip

    h = abi_checks.header()
    abi_checks.declared("int scann_shapley(scann_handle_t* h, scann_dbatch_t* db, int32_t n_perm, uint64_t seed, const uint64_t* keys, "
                        "const int32_t* perms_in, float* y, float* ga, double* shapley, double* stderr_out, double* baseline, double* full, "
                        "float* values, int32_t* perms_out);",
                        "int scann_shapley_profile(scann_handle_t* h, scann_dbatch_t* db, int32_t n_perm, uint64_t seed, const uint64_t* keys, float* ms);",
                        "void scann_shapley_permutation(uint64_t seed, uint64_t key, int32_t p, int32_t n, int32_t* out);",
                        "int scann_shapley_reduce_host(const float* values, const int32_t* perms, const int32_t* mol_offset, int32_t n_struct, "
                        "int32_t n_perm, const double* baseline, double* shapley, double* stderr_out, double* full);")
    assert "#define SCANN_ABI_VERSION 1" in h and hip_lib.scann_abi_version() == 1
    P = C.c_void_p
    sig = abi_checks.signatures({
        "scann_shapley": (C.c_int, [P, P, C.c_int32, C.c_uint64, P, P, P, P, P, P, P, P, P, P]),
        "scann_shapley_profile": (C.c_int, [P, P, C.c_int32, C.c_uint64, P, P]),
        "scann_shapley_permutation": (None, [C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, P]),
        "scann_shapley_reduce_host": (C.c_int, [P, P, P, C.c_int32, C.c_int32, P, P, P, P])})
    for n in ("scann_shapley", "scann_shapley_profile", "scann_shapley_permutation", "scann_shapley_reduce_host"):
        assert hasattr(hip_lib, n), n


def test_null_and_bad_arguments_are_errors_not_crashes(hip_lib):
    from scann import _hip

    assert hip_lib.scann_shapley(None, None, 8, 0, None, None, None, None, None, None, None, None, None, None) == -1
    assert hip_lib.scann_shapley_profile(None, None, 8, 0, None, None) == -1
    mol = np.array([0, 2, 5], np.int32)
    perms = np.array([[0, 1, 2, 0, 1]], np.int32)
    values = np.zeros((1, 5), np.float32)
    base, full = np.zeros(2), np.zeros(2)
    sh, se = np.zeros(5), np.zeros(5)
    r = hip_lib.scann_shapley_reduce_host
    p = _hip._ptr
    assert r(p(values), p(perms), p(mol), 2, 1, p(base), p(sh), p(se), p(full)) == 0
    assert r(None, p(perms), p(mol), 2, 1, p(base), p(sh), p(se), p(full)) == -1
    assert r(p(values), None, p(mol), 2, 1, p(base), p(sh), p(se), p(full)) == -1
    assert r(p(values), p(perms), None, 2, 1, p(base), p(sh), p(se), p(full)) == -1
    assert r(p(values), p(perms), p(mol), 2, 1, None, p(sh), p(se), p(full)) == -1
    assert r(p(values), p(perms), p(mol), 2, 1, p(base), None, p(se), p(full)) == -1
    assert r(p(values), p(perms), p(mol), 2, 0, p(base), p(sh), p(se), p(full)) == -1   # n_perm < 1
    assert r(p(values), p(perms), p(mol), -1, 1, p(base), p(sh), p(se), p(full)) == -1
    bad = perms.copy()
    bad[0, 1] = 2  # outside its two-atom structure
    assert r(p(values), p(bad), p(mol), 2, 1, p(base), p(sh), p(se), p(full)) == -1
    assert r(None, None, p(mol[:1]), 0, 3, p(base), p(sh), p(se), p(full)) == 0  # no structures: nothing to read
    with pytest.raises(ValueError):
        _hip.shapley_reduce_host(values, perms[:, :4], mol, base)
    with pytest.raises(_hip.ScannHipError):
        _hip.shapley_reduce_host(values, bad, mol, base)


def test_shapley_kernels_use_no_scratch_and_keep_their_names_apart(hip_lib):
    """the kernels of csrc/scann_shapley.hip spill nothing, read from the built library's kernel descriptors; their names stay out of the
    name census the other host tests take"""
    from scann import _hip

    kern = {n: v for n, v in abi_checks.device_kernels(_hip.LIB_PATH).items() if "shapley_" in n}
    assert len(kern) == 4, sorted(kern)
    assert sum("shapley_walk_kernel" in n for n in kern) == 2 and sum("gen_shapley_walk_kernel" in n for n in kern) == 1
    assert sum("shapley_pair_kernel" in n for n in kern) == 1 and sum("shapley_reduce_kernel" in n for n in kern) == 1
    for name, (scratch, vgpr) in kern.items():
        assert scratch == 0, (name, scratch, vgpr)
        for other in ("knn_", "rollout_", "ablate_", "input_grad_kernel", "kcenter_", "kmeans_", "pca_", "match_"):
            assert other not in name, name


# ---- the Python layer against a stand-in engine ----

class _StandIn:
    """the Engine surface atom_shapley uses: y = 10 + s, ga = local atom index, shapley = key + local / 1000, stderr = 0.5 local,
    baseline = -key, full = 2 key"""
    training = True  # (padded inputs go through the host packer: the stand-in reads mol_offset)

    def __init__(self):
        self.uploads, self.calls, self.seen = 0, [], 0

    def num_streams(self):
        return 2

    def upload(self, packed):
        self.uploads += 1
        return types.SimpleNamespace(packed=packed, free=lambda: None, release=lambda: None)

    def shapley(self, rb, permutations, seed=0, keys=None, perms=None, want_values=False):
        p = rb.packed
        self.calls.append((permutations, seed, np.asarray(keys).tolist(), p.n_struct))
        cnt = np.diff(p.mol_offset)
        local = (np.arange(p.n_atom) - np.repeat(p.mol_offset[:-1], cnt)).astype(np.float64)
        k = np.asarray(keys, dtype=np.float64)
        out = {"y": (10.0 + np.arange(p.n_struct) + self.seen).astype(np.float32), "ga": local.astype(np.float32),
               "shapley": np.repeat(k, cnt) + local / 1000, "stderr": 0.5 * local, "baseline": -k, "full": 2 * k}
        self.seen += p.n_struct
        return out


def _model(cfg):
    return abi_checks.stand_in_model(cfg, lambda config: _StandIn())


def _batch(n=5):
    import scann_oracle as so

    cfg = so.default_config("qm9")
    inputs, _ = so.pad_batch(*so.synth_dataset(n, 2), g_update=True)
    return cfg, inputs


@pytest.mark.parametrize("kw", [dict(permutations=0), dict(permutations=-4), dict(permutations=2.5), dict(permutations=None),
                                dict(permutations="many"), dict(seed=-1), dict(seed=1.5), dict(seed=None), dict(keys=[1, 2]),
                                dict(keys=[0.5, 1.0, 2.0]), dict(keys=[0, -1, 2]), dict(batch_size=0), dict(batch_size=-3)])
def test_bad_arguments_raise_before_any_upload(kw):
    cfg, inputs = _batch(3)
    m = _model(cfg)
    with pytest.raises(ValueError):
        m.atom_shapley(inputs, **kw)
    assert m.engine.uploads == 0 and not m.engine.calls


def test_repadding_keys_and_slicing():
    cfg, inputs = _batch(5)
    m = _model(cfg)
    r = m.atom_shapley(inputs, permutations=16, seed=9, batch_size=2)
    # keys default to the structure's position in the inputs, whatever the chunking
    assert m.engine.calls == [(16, 9, [0, 1], 2), (16, 9, [2, 3], 2), (16, 9, [4], 1)]
    amask = np.asarray(inputs["atom_mask"]).reshape(5, -1) != 0
    B, M = amask.shape
    assert sorted(r) == ["baseline", "full", "global_attention", "shapley", "stderr", "y"]
    for k in ("y", "baseline", "full"):
        assert r[k].shape == (B, 1) and r[k].dtype == np.float64, k
    for k in ("global_attention", "shapley", "stderr"):
        assert r[k].shape == (B, M, 1) and r[k].dtype == np.float64, k
    for b in range(B):
        pos = np.nonzero(amask[b])[0]
        n = len(pos)
        assert np.array_equal(r["shapley"][b, pos, 0], b + np.arange(n) / 1000) and np.array_equal(r["stderr"][b, pos, 0], 0.5 * np.arange(n))
        assert np.array_equal(r["global_attention"][b, pos, 0], np.arange(n))
        for k in ("global_attention", "shapley", "stderr"):
            assert np.all(r[k][b, ~amask[b], 0] == 0), k
        assert r["y"][b, 0] == 10.0 + b and r["baseline"][b, 0] == -b and r["full"][b, 0] == 2 * b
    one = _model(cfg).atom_shapley(inputs, permutations=16, seed=9, batch_size=64)
    for k in r:
        assert np.array_equal(r[k], one[k]), k
    m2 = _model(cfg)
    m2.atom_shapley(inputs, permutations=3, keys=[7, 7, 8, 2 ** 40, 0], batch_size=4)
    assert m2.engine.calls == [(3, 0, [7, 7, 8, 2 ** 40], 4), (3, 0, [0], 1)]


def test_scann_facade_passes_through_and_denormalises():
    from scann.models.scann_model import SCANN

    cfg, inputs = _batch(3)
    s = SCANN.__new__(SCANN)
    s.model = _model(cfg)
    s.mean, s.std = 2.0, -0.5
    raw = _model(cfg).atom_shapley(inputs, permutations=4, seed=3, keys=[5, 6, 7])
    got = s.atom_shapley(inputs, permutations=4, seed=3, keys=[5, 6, 7], batch_size=2)
    assert s.model.engine.calls == [(4, 3, [5, 6], 2), (4, 3, [7], 1)]
    for k in ("shapley", "stderr"):
        assert np.array_equal(got[k], raw[k] * -0.5), k
    for k in ("y", "baseline", "full"):
        assert np.array_equal(got[k], raw[k] * -0.5 + 2.0), k
    assert np.array_equal(got["global_attention"], raw["global_attention"])


def test_predict_model_cli_takes_shapley():
    pytest.importorskip("sklearn")
    spec = importlib.util.spec_from_file_location("predict_model_cli_shapley", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parser().parse_args(["some_dir", "--shapley", "256", "--shapley-seed", "3"])
    assert a.shapley == 256 and a.shapley_seed == 3
    a = cli.parser().parse_args(["some_dir"])
    assert a.shapley == 0 and a.shapley_seed == 0 and a.contributions == ""
