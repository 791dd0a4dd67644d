"""Host tests of the crystal batches (tests/crystal_batches.py): neighbour lists that repeat an atom and point at the atom itself.

1. Pins: every batch is what its name says -- self-loops, repeated (atom, neighbour) pairs, atoms with more incoming edges than their
   structure has atoms, an atom with edges of its own that no edge points at -- and the upload picks the tile height and the chunk tiles
   tests/test_gpu_crystal.py expects, against tests/size_batches.py's thresholds.
2. The references agree on these graphs before a kernel is compared with them: the padded NumPy oracle and the packed torch graph in
   fp64, the rollout reference against its dense restatement (parallel edges add), input_grad_ref against finite differences, the MC
   masks of parallel edges.
3. The committed lattice fixture is what our own Voronoi builder gives (needs SciPy).
4. The native list walker and the packed slicers give the bytes of pad_batch + pack_inputs.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import crystal_batches as cb
import scann_oracle as so
import size_batches as sb

SMALL = [n for n in cb.DATA if n != "cells_large"]  # every batch the padded oracle runs in a moment
ONE_ATOM = ("cells_small_1atom", "lattices")         # batches with one-atom cells: use_ga_norm=False models only


def config(name, g_update=True, **over):
    return cb.config(g_update, use_ga_norm=name not in ONE_ATOM, **over)


# ---- 1. pins ----

@pytest.mark.parametrize("name", list(cb.DATA))
def test_every_batch_is_a_multigraph_with_self_loops_on_the_intended_tiles(name):
    pk, _ = cb.packed(name)
    deg = np.diff(pk.edge_offset)
    st = cb.graph_stats(pk)
    rows, chunk_tiles = sb.upload_tile_rows(pk)
    print(name, "structures %d atoms %d edges %d max degree %d tile rows %d chunk tiles %d" % (pk.n_struct, pk.n_atom, pk.n_edge, deg.max(), rows, chunk_tiles), st)
    assert st["self_loops"] > 0 and st["repeats"] > 0 and st["in_over"] > 0, st
    want_rows, n_big, (lo, hi) = cb.PLAN[name]
    assert rows == want_rows and lo <= int(deg.max()) <= hi and int((deg > 64).sum()) == n_big
    assert chunk_tiles == int(((deg[deg > 64] + 63) // 64).sum())
    if name == "lattices":  # the Voronoi relation is symmetric: every atom is pointed at as often as it points
        row = np.repeat(np.arange(pk.n_atom), deg)
        assert np.array_equal(np.bincount(pk.edge_col, minlength=pk.n_atom), deg) and st["unseen"] == 0
        assert np.array_equal(np.sort(row * pk.n_atom + pk.edge_col), np.sort(pk.edge_col.astype(np.int64) * pk.n_atom + row))
    else:
        assert st["unseen"] > 0, st
    # the switches each batch is built for
    if name in ("cells_small", "cells_small_1atom", "lattices", "cells_deg16"):
        assert pk.n_edge <= sb.EDGE_TILE_32_MAX_EDGES and int(deg.max()) <= sb.EDGE_TILE_32_MAX_DEGREE
        # the attention backward is fused into edge_bwd_kernel<1, true> up to FUSE_ATTN_MAX_DEGREE: cells_deg16 and lattices
        assert (int(deg.max()) <= sb.FUSE_ATTN_MAX_DEGREE) == (name in ("cells_deg16", "lattices"))
    if name == "cells_large":
        last = sum(len(lst) for lst in cb.cells_large_data()[1][-1])
        assert pk.n_edge - last <= sb.EDGE_TILE_32_MAX_EDGES < pk.n_edge and int(deg.max()) <= sb.FUSE_ATTN_MAX_DEGREE  # the fewest cells
        assert sb.small_cuts(pk)[0] != (0, pk.n_struct)
    if name == "cells_deg40":
        assert sorted(deg[deg > sb.EDGE_TILE_32_MAX_DEGREE].tolist()) == [sb.EDGE_TILE_32_MAX_DEGREE + 1, 40] and pk.n_edge <= sb.EDGE_TILE_32_MAX_EDGES
    if name == "cells_chunked":
        mid = pk.n_struct // 2
        a0 = int(pk.mol_offset[mid])
        assert deg[a0:a0 + 3].tolist() == [65, 130, 64] and int(pk.mol_offset[mid + 1]) == a0 + 3
        for a in range(a0, a0 + 3):  # every chunk of the atom gathers the structure's one to three rows
            for e0 in range(int(pk.edge_offset[a]), int(pk.edge_offset[a + 1]), 64):
                cols = set(pk.edge_col[e0:min(e0 + 64, int(pk.edge_offset[a + 1]))].tolist())
                assert 1 <= len(cols) <= 3 and cols <= {a0, a0 + 1, a0 + 2}
    if name in ONE_ATOM:
        assert (np.diff(pk.mol_offset) == 1).any()
    else:
        assert np.diff(pk.mol_offset).min() >= 2
    assert int(pk.atomic.min()) >= 1 and int(pk.atomic.max()) <= 94


def test_the_lattice_fixture_holds_the_table():
    """edges per atom, edges to the atom itself, distinct neighbours of the seven cells"""
    arr = cb.lattice_arrays()
    want = {"fcc_Cu": ([12], 12, [1]), "bcc_Fe": ([14], 14, [1]), "hcp_Mg": ([12, 12], 12, [2, 2]), "NaCl": ([6, 6], 0, [1, 1]),
            "diamond_C": ([4, 4], 0, [1, 1]), "CsCl": ([8, 8], 0, [1, 1]), "SrTiO3": ([12, 6, 14, 14, 14], 0, [3, 3, 4, 4, 4])}
    for name in cb.LATTICE_NAMES:
        d = arr[name]
        off, idx = d["offset"], d["index"]
        deg = np.diff(off).tolist()
        own = sum(int((idx[off[a]:off[a + 1]] == a).sum()) for a in range(len(deg)))
        distinct = [len(set(idx[off[a]:off[a + 1]].tolist())) for a in range(len(deg))]
        assert (deg, own, distinct) == want[name], (name, deg, own, distinct)
        assert all(v.dtype != object for v in d.values()) and d["index"].max() < len(d["Z"])
    assert arr["hcp_Mg"]["index"][:12].tolist().count(0) == 6  # six in-plane images of the atom itself, six of the other site
    assert os.path.getsize(cb.FIXTURE) < 16 << 10


def test_the_lattice_fixture_is_what_the_voronoi_builder_gives():
    pytest.importorskip("scipy")
    spec = importlib.util.spec_from_file_location("_make_lattice_cells", os.path.join(os.path.dirname(cb.FIXTURE), "make_lattice_cells.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.NAMES == cb.LATTICE_NAMES
    new, old = gen.neighbour_arrays(), cb.lattice_arrays()
    for name in cb.LATTICE_NAMES:
        for k in ("Z", "offset", "index"):
            assert np.array_equal(new[name][k], old[name][k]), (name, k)
        for k in ("angle", "ratio", "distance"):
            assert np.max(np.abs(new[name][k] - old[name][k])) <= 1e-6, (name, k)


# ---- 2. the references on these graphs ----

@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
@pytest.mark.parametrize("name", SMALL)
def test_padded_oracle_and_packed_torch_graph_agree_in_fp64(name, g_update):
    torch_ref = pytest.importorskip("torch_ref")
    cfg, w = config(name, g_update)
    inputs, _ = cb.padded(name, g_update)
    pk, _ = cb.packed(name, g_update)
    inter = {}
    y64, ga64 = so.forward(cfg, w, inputs, np.float64, intermediates=inter)
    yt, gat = torch_ref.forward_packed(cfg, w, pk)
    amask = inputs["atom_mask"][..., 0] != 0
    e_y, e_ga = float(np.max(np.abs(y64 - yt))), float(np.max(np.abs(ga64[..., 0][amask] - gat)))
    y32, ga32 = so.forward(cfg, w, inputs, np.float32)
    print("%s %s: oracle against torch, fp64: y %.1e ga %.1e; fp32 oracle against fp64: y %.1e ga %.1e" % (
        name, "g_update" if g_update else "base", e_y, e_ga, np.max(np.abs(y32 - y64)), np.max(np.abs(ga32 - ga64))))
    assert e_y <= 1e-12 and e_ga <= 1e-12, (e_y, e_ga)
    assert np.isfinite(y64).all()
    # the rollout reference on the oracle's maps: rows sum to 1, and the row gather equals the dense matrices in which parallel edges add
    import rollout_ref

    maps = [inter["attn_local_%d" % (k + 1)] for k in range(cfg["model"]["n_attention"])]
    R, attr = rollout_ref.rollout(inputs, maps, ga64)
    assert np.max(np.abs(R.sum(-1)[amask] - 1.0)) <= 1e-12 and np.max(np.abs(attr[..., 0].sum(1) - 1.0)) <= 1e-12
    assert np.max(np.abs(R - rollout_ref.dense_rollout(inputs, maps))) <= 1e-12


def test_rollout_reference_adds_parallel_edges_and_keeps_self_loops():
    """fcc Cu (twelve edges of one atom to itself) rolls out to [[1]]; NaCl's six parallel edges add up to the
    one weight of a two-atom chain"""
    cfg, w = config("lattices")
    inputs, _ = cb.padded("lattices")
    import rollout_ref

    inter = {}
    so.forward(cfg, w, inputs, np.float64, intermediates=inter)
    maps = [inter["attn_local_%d" % (k + 1)] for k in range(2)]
    R, _ = rollout_ref.rollout(inputs, maps)
    fcc, nacl = cb.LATTICE_NAMES.index("fcc_Cu"), cb.LATTICE_NAMES.index("NaCl")
    assert abs(R[fcc, 0, 0] - 1.0) <= 1e-15 and not R[fcc, 1:].any()
    T = np.array([[0.5, 0.5], [0.5, 0.5]])  # residual 0.5, every edge of either atom to the other: the six weights sum to 1
    assert np.max(np.abs(R[nacl, :2, :2] - T @ T)) <= 1e-14


@pytest.mark.parametrize("name,over", [("cells_small", {}), ("cells_small", dict(g_update=False)), ("lattices", {}), ("lattices", dict(g_update=False))],
                         ids=["cells_small-g_update", "cells_small-base", "lattices-g_update", "lattices-base"])
def test_input_gradient_reference_matches_finite_differences(name, over):
    """the rule of test_input_grads_host.test_reference_matches_directional_finite_differences on per-edge leaves whose edges share
    their (atom, neighbour) pair"""
    torch_ref = pytest.importorskip("torch_ref")
    import input_grad_ref
    from test_input_grads_host import FIELD, _as64

    cfg, w = config(name, **over)
    pk, _ = cb.packed(name, cfg["model"]["g_update"])
    y, grads = input_grad_ref.input_grads(cfg, w, pk)
    y0, _ = torch_ref.forward_packed(cfg, w, _as64(pk))
    assert np.allclose(y, y0.ravel(), rtol=1e-12, atol=1e-12)
    rng = np.random.default_rng(7)
    seg = np.repeat(np.repeat(np.arange(pk.n_struct), np.diff(pk.mol_offset)), np.diff(pk.edge_offset))
    h = 1e-5
    for leaf, g in grads.items():
        x = getattr(_as64(pk), FIELD[leaf])
        assert np.abs(g).max() > 0, leaf
        for _ in range(2):
            v = rng.standard_normal(x.shape)
            yp, _ = torch_ref.forward_packed(cfg, w, _as64(pk, **{FIELD[leaf]: x + h * v}))
            ym, _ = torch_ref.forward_packed(cfg, w, _as64(pk, **{FIELD[leaf]: x - h * v}))
            fd = (yp.ravel() - ym.ravel()) / (2 * h)
            an = np.bincount(seg, weights=g * v, minlength=pk.n_struct)
            assert np.abs(fd - an).max() <= 1e-6 * max(np.abs(an).max(), 1e-3), (leaf, fd, an)


def test_mc_reference_masks_differ_between_edges_of_one_pair(monkeypatch):
    """the attention-dropout masks are keyed by the edge, not by (atom, neighbour): the twelve self-loops of fcc Cu draw twelve
    elements each; a sample of the reference under them is finite and is not the plain forward"""
    torch_ref = pytest.importorskip("torch_ref")
    import mc_ref

    cfg, w = config("lattices", use_drop=True)
    pk, _ = cb.packed("lattices")
    keys = np.arange(pk.n_struct, dtype=np.uint64) + np.uint64(77)
    scales = mc_ref.attn_scales(pk, 5, 0, keys, 8, 2, 0.5)
    fcc = cb.LATTICE_NAMES.index("fcc_Cu")
    e0, e1 = int(pk.edge_offset[pk.mol_offset[fcc]]), int(pk.edge_offset[pk.mol_offset[fcc + 1]])
    assert e1 - e0 == 12 and len(set(pk.edge_col[e0:e1].tolist())) == 1
    assert 0 < (scales[0][e0:e1] == 0).sum() < 96 and not np.array_equal(scales[0][e0:e1], scales[1][e0:e1])
    y, ga = mc_ref.sample_ref(cfg, w, pk, 5, 0, keys, 0.1, 0.05, monkeypatch)
    y0, _ = torch_ref.forward_packed(cfg, w, pk)
    assert np.isfinite(y).all() and np.abs(y - y0.ravel()).max() > 1e-6


# ---- 4. packers ----

@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
@pytest.mark.parametrize("name", ["cells_small", "lattices"])
def test_list_walker_and_slicers_give_the_host_packers_bytes(name, g_update):
    from scann import _hip
    from scann.utils import DataIterator, PackedDataset

    de, dn = cb.DATA[name]()
    ref, targets = cb.packed(name, g_update)
    fields = ("atomic", "mol_offset", "edge_offset", "edge_col", "edge_dist", "edge_weight")

    def same(got, want, what):
        for f in fields:
            a, b = np.asarray(getattr(got, f)), np.asarray(getattr(want, f))
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, f)

    n = len(de)
    whole, t = PackedDataset(de, dn, batch_size=n, g_update=g_update)[0]
    same(whole, ref, "PackedDataset, one batch")
    assert np.array_equal(np.asarray(t, np.float32), targets)
    inputs, _ = DataIterator(de, dn, batch_size=n, g_update=g_update)[0]
    same(_hip.pack_inputs(inputs), ref, "DataIterator + pack_inputs")
    ds = PackedDataset(de, dn, batch_size=4, g_update=g_update)
    parts = [ds[i][0] for i in range(len(ds))]
    for i, p in enumerate(parts):
        same(p, _hip.slice_packed(ref, 4 * i, min(4 * i + 4, n)), "PackedDataset batch %d against slice_packed" % i)
    same(_hip.concat_packed(parts), ref, "concat_packed of the batches")
    same(_hip.concat_packed([_hip.slice_packed(ref, s, s + 1) for s in range(n)]), ref, "concat_packed of single structures")
