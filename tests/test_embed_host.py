"""Host tests of the neighbour embedding of a latent index (scann_embed_iterate, the twin scann_embed_iterate_host, neighbour_graph_host,
embed_affinities, embed_rows_host, LatentEmbedding): the twin against the NumPy restatement of the definition (tests/embed_ref.py), bit
for bit, either side of a block; independence of the thread count; a call split in two; the argument checks; the affinities; the
gradient against the fp64 dense gradient of the objective; header, ctypes table and library agree; the planted blobs end to end.  No GPU."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import abi_checks
import embed_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N", [2, 127, 129, 300])
def test_twin_equals_the_definition(hip_lib, N):
    from scann import _hip

    st = embed_ref.random_state(N, seed=N)
    for ex, mom in ((12.0, 0.5), (1.0, 0.8)):
        got = _hip.embed_iterate_host(*st, 3, ex, mom, 200.0, want_grad=True)
        embed_ref.same_state(got, embed_ref.iterate_n(*st, 3, ex, mom, 200.0), "N %d, exaggeration %g" % (N, ex))
        assert np.isfinite(got["y"]).all() and got["z"] > 0
    # the inputs are not touched, and without the gradient nothing else changes
    y_before = st[3].copy()
    plain = _hip.embed_iterate_host(*st, 3, 1.0, 0.8, 200.0)
    assert np.array_equal(st[3], y_before) and "grad" not in plain
    embed_ref.same_state(plain, got, "no grad", keys=("y", "u", "gain"))


def test_no_iteration_returns_its_inputs(hip_lib):
    from scann import _hip

    st = embed_ref.random_state(50, seed=1)
    got = _hip.embed_iterate_host(*st, 0, 12.0, 0.5, 200.0, want_grad=True)
    assert got["z"] == 0.0 and not got["grad"].any()
    for k, a in zip(("y", "u", "gain"), st[3:]):
        assert np.array_equal(got[k].view(np.uint32), a.view(np.uint32))


def test_six_iterations_equal_three_and_three(hip_lib):
    from scann import _hip

    st = embed_ref.random_state(300, seed=7)
    whole = _hip.embed_iterate_host(*st, 6, 4.0, 0.5, 150.0, want_grad=True)
    half = _hip.embed_iterate_host(*st, 3, 4.0, 0.5, 150.0)
    both = _hip.embed_iterate_host(*st[:3], half["y"], half["u"], half["gain"], 3, 4.0, 0.5, 150.0, want_grad=True)
    embed_ref.same_state(both, whole, "3 + 3")


THREAD_SCRIPT = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import embed_ref
from scann import _hip
st = embed_ref.random_state(2500, seed=3, most=8)  # 2500^2 pairs: above the twin's threshold for threading
out = _hip.embed_iterate_host(*st, 2, 12.0, 0.5, 200.0, want_grad=True)
np.savez(sys.argv[1], z=np.float64(out["z"]), **{k: out[k] for k in ("y", "u", "gain", "grad")})
"""


def test_twin_does_not_depend_on_the_thread_count(hip_lib, tmp_path):
    """OMP_NUM_THREADS 1 against 16, each in a process of its own"""
    script = tmp_path / "run.py"
    script.write_text(THREAD_SCRIPT % (os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "tests")))
    outs = []
    for n in ("1", "16"):
        path = str(tmp_path / ("out%s.npz" % n))
        subprocess.run([sys.executable, str(script), path], check=True, env=dict(os.environ, OMP_NUM_THREADS=n))
        with np.load(path) as z:
            outs.append({k: z[k] for k in z.files})
    embed_ref.same_state(outs[0], outs[1], "OMP_NUM_THREADS 1 against 16")
    assert np.isfinite(outs[0]["y"]).all() and outs[0]["z"] > 0


def test_argument_errors_name_the_argument(hip_lib):
    from scann import _hip

    rf, col, p, y, u, gain = embed_ref.random_state(40, seed=2)
    assert rf[-1] > 4

    def run(rf=rf, col=col, p=p, y=y, u=u, gain=gain, n_iter=1, ex=12.0, mom=0.5, lr=200.0):
        return _hip.embed_iterate_host(rf, col, p, y, u, gain, n_iter, ex, mom, lr)

    def changed(a, at, v):
        b = np.array(a)
        b[at] = v
        return b

    own = int(np.nonzero(np.diff(rf))[0][0])  # a row with an entry
    nan, inf = float("nan"), float("inf")
    for word, kw in (("y", dict(y=y[:, :1])), ("N", dict(y=y[:1], u=u[:1], gain=gain[:1], rf=rf[:2])), ("row_first", dict(rf=rf[:-1])),
                     ("row_first", dict(rf=changed(rf, 0, 1))), ("row_first", dict(rf=changed(rf, 1, rf[-1] + 5))),
                     ("col", dict(col=changed(col, 3, 40))), ("col", dict(col=changed(col, 3, -1))),
                     ("own row", dict(col=changed(col, rf[own], own))), ("col", dict(col=col[:-1])),
                     ("p", dict(p=changed(p, 2, -1e-3))), ("p", dict(p=changed(p, 2, nan))), ("p", dict(p=changed(p, 2, inf))), ("p", dict(p=p[:-1])),
                     ("y", dict(y=changed(y, (5, 1), nan))), ("u", dict(u=changed(u, (5, 0), inf))), ("gain", dict(gain=changed(gain, (0, 0), nan))),
                     ("u", dict(u=u[:-1])), ("n_iter", dict(n_iter=-1)), ("n_iter", dict(n_iter=100001)), ("n_iter", dict(n_iter=2.5)),
                     ("exaggeration", dict(ex=0.0)), ("exaggeration", dict(ex=nan)), ("exaggeration", dict(ex=inf)),
                     ("lr", dict(lr=0.0)), ("lr", dict(lr=-1.0)), ("lr", dict(lr=inf)),
                     ("momentum", dict(mom=1.0)), ("momentum", dict(mom=-0.1)), ("momentum", dict(mom=nan))):
        with pytest.raises(ValueError, match=word):
            run(**kw)
    big = np.zeros((_hip.EMBED_MAX_ROWS + 1, 2), np.float32)
    with pytest.raises(ValueError, match="N"):
        _hip.embed_iterate_host(np.zeros(len(big) + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), big, big, big, 0)


def test_the_c_call_refuses_bad_arguments_itself(hip_lib):
    """the twin's own checks, behind Python's: SCANN_ERR_INVALID (-1), nothing written"""
    from scann import _hip

    P = _hip._ptr
    rf, col, p, y, u, gain = embed_ref.random_state(20, seed=4)
    z = C.c_double(7.0)

    def call(N=20, rf=rf, col=col, p=p, y=y, u=u, gain=gain, n_iter=1, ex=12.0, mom=0.5, lr=200.0, z=C.byref(z)):
        return hip_lib.scann_embed_iterate_host(N, P(rf), P(col), P(p), P(y), P(u), P(gain), n_iter, ex, mom, lr, z, None)

    before = y.copy()
    bad_col = col.copy()
    bad_col[0] = 20
    bad_p = p.copy()
    bad_p[1] = -1.0
    bad_y = y.copy()
    bad_y[3, 0] = np.inf
    for kw in (dict(rf=None), dict(col=None), dict(p=None), dict(y=None), dict(u=None), dict(gain=None), dict(z=None), dict(N=1),
               dict(N=_hip.EMBED_MAX_ROWS + 1), dict(rf=rf + 1), dict(rf=rf[::-1].copy()), dict(col=bad_col), dict(p=bad_p), dict(y=bad_y),
               dict(n_iter=-1), dict(n_iter=100001), dict(ex=0.0), dict(ex=float("nan")), dict(lr=0.0), dict(lr=float("inf")), dict(mom=1.0),
               dict(mom=-0.5)):
        assert call(**kw) == -1, kw
    assert np.array_equal(y, before) and z.value == 7.0


def test_header_and_python_agree(hip_lib):
    from scann import _hip

    abi_checks.declared("int scann_embed_iterate(scann_handle_t* h, int64_t N, const int64_t* row_first /* [N + 1] */, const int32_t* col /* [E] */, "
                        "const float* p /* [E] */, float* y /* [N * 2] in/out */, float* u /* [N * 2] in/out */, float* gain /* [N * 2] in/out */, "
                        "int32_t n_iter, float exaggeration, float momentum, float lr, double* z_out, float* grad_out /* [N * 2] or NULL */);",
                        "int scann_embed_iterate_host(int64_t N, const int64_t* row_first, const int32_t* col, const float* p, float* y, float* u, "
                        "float* gain, int32_t n_iter, float exaggeration, float momentum, float lr, double* z_out, float* grad_out);",
                        "#define SCANN_EMBED_MAX_ROWS 262144", "#define SCANN_ABI_VERSION 1")
    assert _hip.EMBED_MAX_ROWS == 262144 and hip_lib.scann_abi_version() == 1
    P, I, L, F, D = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.POINTER(C.c_double)
    sig = abi_checks.signatures({
        "scann_embed_iterate": (C.c_int, [P, L, P, P, P, P, P, P, I, F, F, F, D, P]),
        "scann_embed_iterate_host": (C.c_int, [L, P, P, P, P, P, P, I, F, F, F, D, P])})
    for name in sig:
        assert hasattr(hip_lib, name), name


def test_affinities_have_the_perplexity_and_are_symmetric(hip_lib):
    from scann.models import latent_index as li

    rng = np.random.default_rng(0)
    rows = rng.standard_normal((400, 12)).astype(np.float32)
    rows[:50] *= 0.05  # a dense knot among sparse rows
    pos, d2 = li.neighbour_graph_host(rows)
    assert pos.shape == d2.shape == (400, 31) and (np.diff(d2, axis=1) >= 0).all() and (pos != np.arange(400)[:, None]).all()
    for perp in (2, 10, 15, 7.5):
        P = li.embed_conditional(d2, perp)
        H = -(P * np.log(np.where(P > 0, P, 1.0))).sum(axis=1)
        assert np.allclose(P.sum(axis=1), 1.0, rtol=0, atol=1e-12) and (P >= 0).all()
        assert np.abs(np.exp(H) / perp - 1.0).max() < 1e-6, (perp, np.abs(np.exp(H) / perp - 1.0).max())
    rf, col, p = li.embed_affinities(d2, pos, 10)
    assert p.dtype == np.float32 and col.dtype == np.int32 and rf.dtype == np.int64 and rf[0] == 0 and rf[-1] == len(col) == len(p)
    assert abs(float(p.astype(np.float64).sum()) - 1.0) < 1e-6 and (p >= 0).all()
    row = np.repeat(np.arange(400), np.diff(rf))
    assert (row != col).all() and len(col) >= 400 * 31
    for i in range(400):
        assert (np.diff(col[rf[i]:rf[i + 1]]) > 0).all()  # ascending, no duplicate
    dense = np.zeros((400, 400), np.float32)
    dense[row, col] = p
    assert np.array_equal(dense, dense.T)
    stored = np.zeros((400, 400), bool)
    stored[np.repeat(np.arange(400), 31), pos.ravel()] = True
    assert np.array_equal(dense > 0, stored | stored.T)  # the union of the edges, nothing else
    for bad in (1.9, 15.5, 0, float("nan"), "ten", True):
        with pytest.raises(ValueError, match="perplexity"):
            li.embed_rows_host(rows, perplexity=bad)


def test_identical_rows_get_finite_uniform_weights(hip_lib):
    from scann.models import latent_index as li

    rows = np.tile(np.arange(6, dtype=np.float32), (40, 1))
    pos, d2 = li.neighbour_graph_host(rows)
    assert not d2.any() and pos.shape == (40, 31)
    # among equal distances the search's order is the position's; the row itself is dropped where it appears, else the last place
    assert np.array_equal(pos[0], np.arange(1, 32)) and np.array_equal(pos[39], np.arange(31)) and np.array_equal(pos[5], np.delete(np.arange(32), 5))
    P = li.embed_conditional(d2, 10)
    assert np.array_equal(P, np.full((40, 31), 1.0 / 31))
    rf, col, p = li.embed_affinities(d2, pos, 10)
    assert np.isfinite(p).all() and (p > 0).all() and abs(float(p.astype(np.float64).sum()) - 1.0) < 1e-6
    equal_far = np.full((3, 31), 9.0, np.float32)  # all-equal, not zero
    assert np.array_equal(li.embed_conditional(equal_far, 2), np.full((3, 31), 1.0 / 31))


def test_gradient_against_the_fp64_dense_gradient(hip_lib):
    """The twin's gradient must lie within max(1e-6 of the largest component, 2 x the error of the fp32 NumPy restatement on the same
    input) of the fp64 dense gradient of the objective."""
    from scann import _hip

    for N, spread, ex in ((300, 1.0, 1.0), (300, 10.0, 12.0), (129, 1e-4, 12.0)):
        st = embed_ref.random_state(N, seed=11, spread=spread, symmetric=True)
        got = _hip.embed_iterate_host(*st, 1, ex, 0.5, 200.0, want_grad=True)["grad"].astype(np.float64)
        ref32 = embed_ref.iterate(*st, ex, 0.5, 200.0)["grad"].astype(np.float64)
        exact = embed_ref.dense_gradient(*st[:4], ex)
        top = np.abs(exact).max()
        err, err32 = np.abs(got - exact).max(), np.abs(ref32 - exact).max()
        print("N %d spread %g exaggeration %g: largest component %.3e, twin error %.3e (%.3e of it), restatement error %.3e" % (
            N, spread, ex, top, err, err / top, err32))
        assert err <= max(1e-6 * top, 2.0 * err32)


def test_embedding_saves_loads_and_checks(hip_lib, tmp_path):
    from scann.models import LatentEmbedding

    class Model:
        config = {"model": {"dense_out": 4, "global_dim": 9}}

    rng = np.random.default_rng(0)
    emb = LatentEmbedding(rng.standard_normal((7, 2)), np.arange(7) + 10, np.full(7, -1), 10, "structure", 4)
    emb.check_model(Model)
    emb.save(str(tmp_path / "e.npz"))
    back = LatentEmbedding.load(Model, str(tmp_path / "e.npz"))
    assert np.array_equal(back.coordinates, emb.coordinates) and np.array_equal(back.ids, emb.ids) and np.array_equal(back.atoms, emb.atoms)
    assert (back.perplexity, back.level, back.dim, len(back)) == (10.0, "structure", 4, 7)
    for args, word in (((np.zeros((7, 3)), np.arange(7), np.arange(7), 10, "structure", 4), "coordinates"),
                       ((np.zeros((7, 2)), np.arange(6), np.arange(7), 10, "structure", 4), "ids"),
                       ((np.zeros((7, 2)), np.arange(7), np.arange(7), 40, "structure", 4), "perplexity"),
                       ((np.zeros((7, 2)), np.arange(7), np.arange(7), 10, "bond", 4), "level"),
                       ((np.full((7, 2), np.nan), np.arange(7), np.arange(7), 10, "structure", 4), "finite")):
        with pytest.raises(ValueError, match=word):
            LatentEmbedding(*args)
    atom = LatentEmbedding(np.zeros((7, 2)), np.arange(7), np.arange(7), 10, "atom", 4)
    with pytest.raises(ValueError, match="does not fit"):
        atom.check_model(Model)
    atom.save(str(tmp_path / "a.npz"))
    with pytest.raises(ValueError, match="does not fit"):
        LatentEmbedding.load(Model, str(tmp_path / "a.npz"))
    # placing: the weighted mean of the neighbours' map rows, the nearest row reported
    out = emb.place(np.array([[2, 3, 4]]), np.array([[0.0, 4.0, 4.0]], np.float32))
    assert out["nearest_position"][0] == 2 and out["nearest_id"][0] == 12 and out["nearest_distance"][0] == 0.0
    assert np.allclose(out["coords"][0], emb.coordinates[[2, 3, 4]].mean(axis=0))  # three neighbours, perplexity 10: uniform


def test_planted_blobs_end_to_end_on_the_host(hip_lib):
    from scann.models import latent_index as li

    rows, labels = embed_ref.blobs(0)
    res, emb = li.embed_rows_host(rows, perplexity=10, iterations=(100, 200))
    share = embed_ref.blob_share(res["coords"], labels)
    print("kl %.4f -> %.4f, share %.4f, z %.6g" % (res["kl_init"], res["kl"], share, res["z"]))
    assert res["kl"] < 0.5 * res["kl_init"]
    assert share >= 0.98
    assert res["coords"].shape == (600, 2) and res["coords"].dtype == np.float32 and np.array_equal(emb.coordinates, res["coords"])
    assert res["neighbor_position"].shape == (600, 31) and len(emb) == 600 and emb.perplexity == 10.0
    assert np.abs(res["coords"].astype(np.float64).mean(axis=0)).max() < 1e-3  # centred
    again, _ = li.embed_rows_host(rows, perplexity=10, iterations=(100, 200))
    assert np.array_equal(again["coords"].view(np.uint32), res["coords"].view(np.uint32)) and again["kl"] == res["kl"]
    with pytest.raises(ValueError, match="iterations"):
        li.embed_rows_host(rows, iterations=(100,))
    with pytest.raises(ValueError, match="learning_rate"):
        li.embed_rows_host(rows, learning_rate="fast")
    with pytest.raises(ValueError, match="exaggeration"):
        li.embed_rows_host(rows, exaggeration=0)


def test_cli_takes_the_embed_flags():
    spec = importlib.util.spec_from_file_location("predict_model_cli", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parser().parse_args(["some_dir", "--embed", "--embed-level", "atom", "--embed-perplexity", "5", "--embed-out", "map.npz"])
    assert (a.embed, a.embed_level, a.embed_perplexity, a.embed_out) == (True, "atom", 5.0, "map.npz")
    d = cli.parser().parse_args(["some_dir"])
    assert (d.embed, d.embed_level, d.embed_perplexity, d.embed_out) == (False, "structure", 10.0, "")
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--embed-level", "bond"])
    for bad in (["--embed", "--embed-perplexity", "40"], ["--embed-out", "x.npz"]):  # before the model's folder is read
        with pytest.raises(SystemExit):
            cli.main(cli.parser().parse_args(["no_such_model_dir"] + bad))
