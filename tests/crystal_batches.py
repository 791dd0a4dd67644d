"""Seeded batches whose neighbour lists are what a crystal's are: multigraphs with self-loops.  The reference stores the index of the
periodic SITE behind every Voronoi facet, whichever image the facet belongs to (so does scann/utils/voronoi_neighbor.py), so a small
unit cell lists one neighbour several times and lists the atom itself: fcc Cu is one atom with twelve edges to itself.  Every other
batch of the suite (so.synth_dataset, tests/size_batches.py) is a simple graph.

Shared by tests/test_crystal_host.py, which pins that every batch is what its name says and that the references agree on it, and
tests/test_gpu_crystal.py, which compares the kernels with those references.  The thresholds are size_batches' (not restated).  Test-only."""
import functools
import os

import numpy as np

import scann_oracle as so
import size_batches as sb

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lattice_cells.npz")
LATTICE_NAMES = ("fcc_Cu", "bcc_Fe", "hcp_Mg", "NaCl", "diamond_C", "CsCl", "SrTiO3")  # tests/golden/make_lattice_cells.py
ANGLE, DISTANCE = (0.4, 3.5), (1.5, 6.0)  # so.synth_dataset's mp2018 ranges


# ---- datasets: (data_energy, data_neighbor) object arrays like so.synth_dataset ----

def cell(rng, degrees, unseen=False):
    """one structure of len(degrees) atoms, Z in 1..94; atom a has degrees[a] edges whose neighbour is drawn with replacement from ALL
    atoms of the structure, itself included: ([atomic numbers, target], neighbour lists).  unseen: all but the last atom, which then
    has edges of its own and none that points at it -- an empty segment of the reverse adjacency (with a draw from all atoms that
    happens in no batch of this size: no seed out of 300 gave one)"""
    A = len(degrees)
    Z = rng.integers(1, 95, size=A)
    atoms = []
    for a in range(A):
        d = int(degrees[a])
        js = rng.integers(0, A - 1 if unseen else A, size=d)
        ang, dist = rng.uniform(*ANGLE, size=d), rng.uniform(*DISTANCE, size=d)
        atoms.append([[int(Z[j]), int(j), float(ang[k]), float(ang[k] / ang.max()), float(dist[k])] for k, j in enumerate(js)])
    return [[int(z) for z in Z], float(rng.normal())], atoms


UNSEEN_SIZE = 8  # cells of this many atoms are drawn with cell(unseen=True)


def one_cell(seed, i, sizes, lo, hi):
    """cell i of cells(.., seed, sizes, lo, hi): it does not depend on how many cells are drawn"""
    rng = np.random.default_rng([seed, i])
    A = sizes[i % len(sizes)]
    return cell(rng, rng.integers(lo, hi + 1, size=A), unseen=A == UNSEEN_SIZE)


def as_dataset(structs):
    de, dn = np.empty(len(structs), dtype=object), np.empty(len(structs), dtype=object)
    for i, (e, n) in enumerate(structs):
        de[i], dn[i] = e, n
    return de, dn


def cells(n, seed, sizes, lo, hi):
    """n structures of sizes[i % len(sizes)] atoms, every atom with lo..hi edges (cell)"""
    return as_dataset([one_cell(seed, i, sizes, lo, hi) for i in range(n)])


SMALL_SIZES = (2, 3, 8, 5, 4, 6, 7)
SMALL_1ATOM_SIZES = (2, 1, 8, 5, 1, 6, 3)


@functools.lru_cache(maxsize=None)
def cells_small_data():
    """14 cells of 2 - 8 atoms, 4 - 24 edges per atom: 32-row edge tiles, above FUSE_ATTN_MAX_DEGREE"""
    return cells(14, 3, SMALL_SIZES, 4, 24)


@functools.lru_cache(maxsize=None)
def cells_small_1atom_data():
    """the same with one-atom cells (every edge a self-loop) among them: for use_ga_norm=False models"""
    return cells(14, 0, SMALL_1ATOM_SIZES, 4, 24)


@functools.lru_cache(maxsize=None)
def cells_deg16_data():
    """14 cells of 2 - 8 atoms, 4 - 16 edges per atom: the fused attention backward on 32-row tiles"""
    return cells(14, 1, SMALL_SIZES, 4, sb.FUSE_ATTN_MAX_DEGREE)


@functools.lru_cache(maxsize=None)
def cells_large_data():
    """the fewest cells of 2 - 8 atoms and 4 - 16 edges per atom that put n_edge past EDGE_TILE_32_MAX_EDGES: 64-row tiles by edge count"""
    structs, edges = [], 0
    while edges <= sb.EDGE_TILE_32_MAX_EDGES:
        structs.append(one_cell(5, len(structs), SMALL_SIZES, 4, sb.FUSE_ATTN_MAX_DEGREE))
        edges += sum(len(lst) for lst in structs[-1][1])
    return as_dataset(structs)


def flanked(seed, degrees, n=6):
    """a cell of the given degrees in the middle of n ordinary cells (2 - 8 atoms, 4 - 16 edges per atom)"""
    return sb.flanked(cell(np.random.default_rng([seed, 1 << 20]), degrees), cells(n, seed, SMALL_SIZES, 4, sb.FUSE_ATTN_MAX_DEGREE))


DEG40_DEGREES = (sb.EDGE_TILE_32_MAX_DEGREE + 1, 40)
CHUNKED_DEGREES = (65, 130, 64)


@functools.lru_cache(maxsize=None)
def cells_deg40_data():
    """a two-atom cell whose atoms have 33 and 40 edges, between ordinary cells: 64-row tiles by degree, no chunk tiles"""
    return flanked(2, DEG40_DEGREES)


@functools.lru_cache(maxsize=None)
def cells_chunked_data():
    """a three-atom cell whose atoms have 65, 130 and 64 edges, between ordinary cells: two atoms' chunk tiles, every chunk of which
    gathers the same one to three rows"""
    return flanked(4, CHUNKED_DEGREES)


@functools.lru_cache(maxsize=None)
def cells_small_ring_data():
    """cells_small with a ring / aromatic flag pair per atom (use_ring: the general embedding)"""
    de, dn = cells_small_data()
    rng = np.random.default_rng(8)
    return as_dataset([([e[0], e[1], rng.integers(0, 2, size=(len(e[0]), 2)).astype("int32")], n) for e, n in zip(de, dn)])


def lattice_arrays(path=FIXTURE):
    """name -> dict(Z, offset, index, angle, ratio, distance) of the committed fixture"""
    with np.load(path, allow_pickle=False) as z:
        return {name: {k: z["%s/%s" % (name, k)] for k in ("Z", "offset", "index", "angle", "ratio", "distance")} for name in LATTICE_NAMES}


def lists_of(arr):
    """one structure's arrays -> ([atomic numbers, target], neighbour lists)"""
    Z, off = arr["Z"], arr["offset"]
    atoms = [[[int(Z[arr["index"][e]]), int(arr["index"][e]), float(arr["angle"][e]), float(arr["ratio"][e]), float(arr["distance"][e])]
              for e in range(off[a], off[a + 1])] for a in range(len(Z))]
    return [[int(z) for z in Z], 0.1 * float(len(Z)) - 0.2], atoms


@functools.lru_cache(maxsize=None)
def lattices_data():
    """the seven unit cells of tests/golden/lattice_cells.npz, in LATTICE_NAMES' order: our own Voronoi builder's lists"""
    arrays = lattice_arrays()
    return as_dataset([lists_of(arrays[name]) for name in LATTICE_NAMES])


DATA = {"cells_small": cells_small_data, "cells_small_1atom": cells_small_1atom_data, "cells_deg16": cells_deg16_data,
        "cells_large": cells_large_data, "cells_deg40": cells_deg40_data, "cells_chunked": cells_chunked_data, "lattices": lattices_data}
RING_DATA = {"cells_small": cells_small_ring_data}

# what each batch is: (edge-tile height, atoms with chunk tiles, range of the largest degree)
PLAN = {
    "cells_small": (32, 0, (sb.FUSE_ATTN_MAX_DEGREE + 1, 24)),
    "cells_small_1atom": (32, 0, (sb.FUSE_ATTN_MAX_DEGREE + 1, 24)),
    "cells_deg16": (32, 0, (sb.FUSE_ATTN_MAX_DEGREE, sb.FUSE_ATTN_MAX_DEGREE)),
    "cells_large": (64, 0, (sb.FUSE_ATTN_MAX_DEGREE, sb.FUSE_ATTN_MAX_DEGREE)),
    "cells_deg40": (64, 0, (40, 40)),
    "cells_chunked": (64, 2, (130, 130)),
    "lattices": (32, 0, (14, 14)),
}


# ---- batches ----

def config(g_update=True, L=2, **over):
    """(config, weights): the crystal configuration (95 species, gaussian_d 6) with L LocalAttention layers"""
    cfg = so.default_config("mp2018")
    cfg["model"].update(n_attention=L, g_update=g_update, **over)
    return cfg, so.init_weights(cfg, 3, perturb=True)


def padded(name, g_update=True, use_ring=False):
    """the padded Keras input dict and targets of the batch `name`"""
    return sb.padded((RING_DATA if use_ring else DATA)[name](), g_update, use_ring)


def packed(name, g_update=True, use_ring=False):
    """(PackedBatch, targets) of the batch `name`"""
    return sb.packed((RING_DATA if use_ring else DATA)[name](), g_update, use_ring)


def padded_general(name, g_update=True):
    """padded(name, use_ring=True) with the atomic numbers replaced by 92 seeded 0 / 1 features each (feature cgcnn), as
    test_gpu_input_grads.setup builds them"""
    inputs, targets = padded(name, g_update, use_ring=True)
    inputs["atomic"] = np.random.default_rng(5).integers(0, 2, size=(101, 92)).astype("float32")[inputs["atomic"]]
    return inputs, targets


def graph_stats(pk):
    """what makes a batch a crystal's: dict(self_loops, repeats, in_over -- atoms whose in-degree exceeds their structure's atom count,
    unseen -- atoms with edges of their own that no edge points at)"""
    deg = np.diff(pk.edge_offset).astype(np.int64)
    row = np.repeat(np.arange(pk.n_atom), deg)
    col = np.asarray(pk.edge_col, np.int64)
    size = np.repeat(np.diff(pk.mol_offset), np.diff(pk.mol_offset))
    indeg = np.bincount(col, minlength=pk.n_atom)
    pairs = row * pk.n_atom + col
    return dict(self_loops=int((row == col).sum()), repeats=int(len(pairs) - len(np.unique(pairs))),
                in_over=int((indeg > size).sum()), unseen=int(((indeg == 0) & (deg > 0)).sum()))
