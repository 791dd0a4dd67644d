"""Seeded batches on the large side of the launch code's size switches, shared by tests/test_sizes_host.py (which pins that they
cross what they are meant to cross) and tests/test_gpu_sizes.py, tests/test_gpu_mc_sizes.py, tests/test_gpu_output_sizes.py,
tests/test_gpu_parity.py and tests/test_gpu_input_grad_sizes.py (which compare the kernels on them with references; the last one also
takes the ring / cgcnn variants below, pinned by tests/test_input_grad_sizes_host.py); and batches past 2^31 bytes per tensor, up to the
upload limit, for tests/test_gpu_large_rows.py.

The launch code picks a template instantiation, tile height, partial-sum partition or reduction kernel by row count; the
constants below restate those thresholds, each next to the source line it mirrors.  If a threshold moves, the host test fails
instead of the GPU tests quietly running the small side again.  Test-only."""
import functools

import numpy as np

import scann_oracle as so

# ---- thresholds (csrc/) ----
FUSED_TILE_ROWS_32_MAX = 32 * 768     # scann_train_slots.h fused_split: rn_bwd_kernel<2> / edge_bwd_kernel<2,..> above (rows)
EDGE_TILE_32_MAX_EDGES = 32 * 1024    # scann_batch.cpp upload_impl `small`: 32-row edge tiles only while E <= this ...
EDGE_TILE_32_MAX_DEGREE = 32          # ... and no atom has more neighbours (else planned again at 64 rows)
FUSE_ATTN_MAX_DEGREE = 16             # scann_train_host.cpp Bwd::fuse_attn (also needs 32-row tiles); attn_bwd16_kernel up to this
ATOM_TILE_32_MAX = 32 * 1024          # scann_kernels.hip launch_atom: atom_kernel<.., 2, ..> (64-row tiles) above (atoms)
ATTN_APW16_ATOMS = 4096               # scann_train_slots.h attn_apw16: one atom per wave up to this many atoms, 2 to 8 above
WGRAD_FOUR_CHUNKS_MAX = 4 * 64 * 80   # scann_train_slots.h wgrad_chunks: 4 chunks of 64 rows per slab up to this, more above
WGRAD_REDUCE4_BYTES = 24 << 20        # scann_train.hip wgrad_flush: wgrad_reduce4_kernel at >= this many bytes of partial slots
WGRAD_SLOT_BYTES = 128 * 128 * 4      # one partial slot of a 128 x 128 weight gradient
LN_BWD_ONE_GROUP_MAX = 32 * 1536      # scann_train_slots.h ln_bwd_groups: one 32-row group per workgroup up to this, >= 2 above (rows)
GEN_LN_64_ROWS_MAX = 512 * 64         # scann_generic_train.hip gen_ln_chunks: <= 64 rows per chunk up to this, more above
UPLOAD_MAX_ATOMS = 60000 // (5 * 4)   # scann_batch.cpp upload_impl: 5 floats of LDS per atom of the largest structure (3,000)
GEN_BWD_MAX_ATOMS = (65536 // 8 - 4) // 3  # scann_train_host.cpp gen_backward: (3 n + 4) doubles <= 64 KiB (2,729)
UPLOAD_MAX_ROWS = (1 << 32) // (128 * 4) - 1   # scann_batch.cpp upload_impl: max(atoms, edges) * 128 * 4 < 2^32 (8,388,607 rows)
SIGNED_OFFSET_ROWS = (1 << 31) // (128 * 4)    # above this many rows a [rows, 128] fp32 tensor passes 2^31 bytes (4,194,304)


def wgrad_chunks(rows):
    """scann_train_slots.h wgrad_chunks"""
    tiles = (rows + 63) // 64
    return max(min(4, tiles), (tiles + 79) // 80)


def wgrad_slabs(rows):
    """scann_train_slots.h wgrad_slabs"""
    c = wgrad_chunks(rows)
    return (rows + 64 * c - 1) // (64 * c)


def layer_wgrad_bytes(n_atom, n_edge):
    """partial-slot bytes of the 128 x 128 weight gradients one g_update LocalAttention + ResidualNorm layer hands to wgrad_flush:
    dense_1, dense_2, query and filter_geo's W1 / W3 over atom rows, key and filter_geo's W2 over edge rows (scann_train_host.cpp)"""
    return (5 * wgrad_slabs(n_atom) + 2 * wgrad_slabs(n_edge)) * WGRAD_SLOT_BYTES


# what each batch is built to cross: lower bounds on atoms / edges, the range of the largest degree, the edge-tile height
LARGE = {
    # edge_bwd_kernel<2, ..>, 64-row edge tiles, > 4 wgrad chunks per slab on the edge rows; degree > 16: attn_bwd_kernel
    "mp2018_b128": dict(atoms=3000, edges=max(EDGE_TILE_32_MAX_EDGES, WGRAD_FOUR_CHUNKS_MAX), degree=(FUSE_ATTN_MAX_DEGREE + 1, 24),
                        tile_rows=64),
    # 64-row edge tiles with every degree <= 16: the unfused attn_bwd16_kernel, 2 atoms per wave
    "qm9_b260": dict(atoms=ATTN_APW16_ATOMS, edges=EDGE_TILE_32_MAX_EDGES, degree=(1, FUSE_ATTN_MAX_DEGREE), tile_rows=64),
    # the same with ring features (use_ring: the general embedding -- an embed launch, no per-species tables) on 64-row edge tiles
    "qm9_ring_b260": dict(atoms=ATTN_APW16_ATOMS, edges=EDGE_TILE_32_MAX_EDGES, degree=(1, FUSE_ATTN_MAX_DEGREE), tile_rows=64),
    # rn_bwd_kernel<2>, atom_kernel<.., 2, ..>, 8 atoms per wave, two ln_bwd row groups on the edge rows, gen_ln_chunks > 64 rows
    "sparse_atoms": dict(atoms=max(ATOM_TILE_32_MAX, GEN_LN_64_ROWS_MAX, 7 * ATTN_APW16_ATOMS), edges=LN_BWD_ONE_GROUP_MAX,
                         degree=(1, FUSE_ATTN_MAX_DEGREE), tile_rows=64),
    # one structure at the upload / plain-backward limits (its size is checked on the PackedBatch: the device reports no maximum)
    "giant": dict(atoms=0, edges=0, degree=(12, 12), tile_rows=None),
}


def crosses(name, atoms, edges, max_degree, tile_rows, big_atoms):
    """a batch of these counts is on the large side of every switch LARGE[name] names (and has no chunked atoms)"""
    want = LARGE[name]
    lo, hi = want["degree"]
    ok = atoms > want["atoms"] and edges > want["edges"] and lo <= max_degree <= hi and big_atoms == 0
    ok = ok and (want["tile_rows"] is None or tile_rows == want["tile_rows"])
    if name == "sparse_atoms":
        ok = ok and layer_wgrad_bytes(atoms, edges) >= WGRAD_REDUCE4_BYTES
    return ok


def small_side(atoms, edges):
    """a (sub-)batch this small runs the small side of every switch: 32-row atom / edge / fused tiles, one atom per wave, four wgrad
    chunks per slab, one ln_bwd row group, no wgrad_reduce4_kernel (a layer's seven gradients and the readout's four, counted as atom rows)"""
    return (atoms <= ATTN_APW16_ATOMS and edges <= WGRAD_FOUR_CHUNKS_MAX and
            (9 * wgrad_slabs(atoms) + 2 * wgrad_slabs(edges)) * WGRAD_SLOT_BYTES < WGRAD_REDUCE4_BYTES)


def small_cuts(pk):
    """contiguous runs of whole structures that each sit on the small side of every switch (small_side)"""
    mol, eoff = pk.mol_offset.astype(np.int64), pk.edge_offset.astype(np.int64)
    cuts, lo = [], 0
    for hi in range(1, pk.n_struct + 1):
        if not small_side(int(mol[hi] - mol[lo]), int(eoff[mol[hi]] - eoff[mol[lo]])):
            assert hi - 1 > lo
            cuts.append((lo, hi - 1))
            lo = hi - 1
    cuts.append((lo, pk.n_struct))
    return cuts


# ---- datasets: (data_energy, data_neighbor) object arrays like so.synth_dataset ----

@functools.lru_cache(maxsize=None)
def mp2018_b128_data():
    """configs[3]'s batch of 128 synthetic crystals: ~3.2 k atoms, ~43 k edges, up to 24 neighbours"""
    return so.synth_dataset(128, 1, "mp2018")


@functools.lru_cache(maxsize=None)
def qm9_b260_data():
    """260 QM9-like molecules: 4,779 atoms, 35,837 edges, up to 12 neighbours"""
    return so.synth_dataset(260, 1)


@functools.lru_cache(maxsize=None)
def qm9_ring_b260_data():
    """260 QM9-like molecules with a ring / aromatic flag per atom (the generator draws them between the molecules, so the graphs are
    not those of qm9_b260): 4,742 atoms, 35,569 edges, up to 12 neighbours"""
    return so.synth_dataset(260, 1, use_ring=True)


@functools.lru_cache(maxsize=None)
def sparse_atoms_data():
    """1,900 QM9-like molecules, each atom's neighbour list cut to its first 0 - 3 entries: 34,231 atoms (isolated ones among
    them), 51,255 edges, up to 3 neighbours"""
    de, dn = so.synth_dataset(1900, 1)
    rng = np.random.default_rng(0)
    cut = np.empty(len(dn), dtype=object)
    for i, atoms in enumerate(dn):
        cut[i] = [lst[:int(rng.integers(0, 4))] for lst in atoms]
    return de, cut


@functools.lru_cache(maxsize=None)
def giant_data(n_atoms):
    """one structure of `n_atoms` atoms with 12 neighbours each, between two ordinary molecules.  (No atom has atom 1000 as a
    neighbour: in the padded layout index 1000 is the reference's empty-slot sentinel, datagenerator.py:82-90.)"""
    de, dn = so.synth_dataset(2, 5)
    rng = np.random.default_rng(n_atoms)
    Z = rng.choice([1, 6, 7, 8], n_atoms)
    nb = []
    for a in range(n_atoms):
        others = np.setdiff1d(np.arange(n_atoms), [a, 1000])
        js = rng.choice(others, 12, replace=False)
        ang, dist = rng.uniform(0.4, 3.5, 12), rng.uniform(0.9, 4.0, 12)
        nb.append([[int(Z[j]), int(j), float(ang[k]), float(ang[k] / ang.max()), float(dist[k])] for k, j in enumerate(js)])
    de3, dn3 = np.empty(3, dtype=object), np.empty(3, dtype=object)
    de3[0], dn3[0] = de[0], dn[0]
    de3[1], dn3[1] = [[int(z) for z in Z], float(rng.normal())], nb
    de3[2], dn3[2] = de[1], dn[1]
    return de3, dn3


def hub_structure(rng, n_atoms, degrees):
    """one structure of `n_atoms` atoms in which atom a has degrees[a] neighbours and every other atom 0 to 8:
    ([atomic numbers, target], neighbour lists)"""
    nb = []
    for a in range(n_atoms):
        d = degrees.get(a, int(rng.integers(0, 9)))
        js = rng.choice(np.delete(np.arange(n_atoms), a), d, replace=False)
        ang = rng.uniform(0.4, 3.5, size=d)
        nb.append([[6, int(j), float(ang[k]), float(ang[k] / ang.max()), float(rng.uniform(0.9, 4.0))] for k, j in enumerate(js)])
    return [[int(z) for z in rng.choice([1, 6, 7, 8], n_atoms)], 0.0], nb


def flanked(big, flank):
    """the structure `big` in the middle of the molecules of the dataset `flank`"""
    de, dn = flank
    n, mid = len(de), len(de) // 2
    de2, dn2 = np.empty(n + 1, dtype=object), np.empty(n + 1, dtype=object)
    for i in range(n):
        de2[i + (i >= mid)], dn2[i + (i >= mid)] = de[i], dn[i]
    de2[mid], dn2[mid] = big
    return de2, dn2


CHUNKED_DEGREES = {0: 219, 1: 65, 7: 128, 8: 129, 9: 64, 100: 200, 219: 70}  # six atoms above 64 (chunk tiles), one at 64
DEG40_DEGREES = {5: 40, 30: EDGE_TILE_32_MAX_DEGREE + 1}                     # nothing above 64: no chunk tiles


@functools.lru_cache(maxsize=None)
def chunked_data():
    """a 220-atom structure whose atoms 0, 1, 7, 8, 100 and 219 have 65 to 219 neighbours -- chunk tiles, merged by
    edge_merge_kernel, on 64-row edge tiles -- between two small molecules"""
    return flanked(hub_structure(np.random.default_rng(11), 220, CHUNKED_DEGREES), so.synth_dataset(2, 3))


@functools.lru_cache(maxsize=None)
def deg40_data():
    """a 48-atom structure with one atom of 40 neighbours and one of exactly 33 -- more than EDGE_TILE_32_MAX_DEGREE: a few hundred
    edges on 64-row edge tiles, no chunk tiles -- in the middle of six QM9-like molecules"""
    return flanked(hub_structure(np.random.default_rng(40), 48, DEG40_DEGREES), so.synth_dataset(6, 3))


# ---- batches: (PackedBatch, targets) ----

def padded(data, g_update=True, use_ring=False):
    """the padded Keras input dict and targets of a dataset (so.pad_batch)"""
    return so.pad_batch(*data, g_update=g_update, use_ring=use_ring)


def packed(data, g_update=True, use_ring=False):
    from scann import _hip

    inputs, targets = padded(data, g_update, use_ring)
    return _hip.pack_inputs(inputs), np.asarray(targets, np.float32)


def mp2018_b128(g_update=True):
    return packed(mp2018_b128_data(), g_update)


def qm9_b260(g_update=True):
    return packed(qm9_b260_data(), g_update)


def qm9_ring_b260(g_update=True):
    return packed(qm9_ring_b260_data(), g_update, use_ring=True)


def sparse_atoms(g_update=True):
    return packed(sparse_atoms_data(), g_update)


def giant(n_atoms, g_update=True):
    return packed(giant_data(n_atoms), g_update)


def chunked(g_update=True):
    return packed(chunked_data(), g_update)


def deg40(g_update=True):
    return packed(deg40_data(), g_update)


# ---- the general embedding's inputs on these batches (tests/test_gpu_input_grad_sizes.py) ----

CHUNKED_RING_SEED = 23


def with_cgcnn(pk):
    """`pk` with 92 seeded 0 / 1 features per atom in place of its atomic numbers (feature cgcnn): rng(5), as
    test_gpu_input_grads.setup seeds its table"""
    from scann import _hip

    feat = np.random.default_rng(5).integers(0, 2, size=(pk.n_atom, 92)).astype(np.float32)
    return _hip.PackedBatch(None, pk.mol_offset, pk.edge_offset, pk.edge_col, pk.edge_dist, pk.edge_weight, ring=pk.ring, cgcnn=feat)


def with_ring(pk, seed):
    """`pk` with a seeded ring / aromatic flag pair per atom (use_ring), for structures whose generator draws none"""
    from scann import _hip

    ring = np.random.default_rng(seed).integers(0, 2, size=(pk.n_atom, 2)).astype(np.float32)
    return _hip.PackedBatch(pk.atomic, pk.mol_offset, pk.edge_offset, pk.edge_col, pk.edge_dist, pk.edge_weight, ring=ring, cgcnn=pk.cgcnn)


def qm9_b260_cgcnn(g_update=True):
    pk, targets = qm9_b260(g_update)
    return with_cgcnn(pk), targets


def chunked_ring(g_update=True):
    """`chunked` with ring flags: chunk tiles under the general embedding"""
    pk, targets = chunked(g_update)
    return with_ring(pk, CHUNKED_RING_SEED), targets


def small_general(g_update=True):
    """8 QM9-like molecules with ring flags and cgcnn features (use_ring + feature cgcnn): the batch test_gpu_input_grads.setup(n=8,
    use_ring=True, feature="cgcnn") builds, on 32-row tiles"""
    from scann import _hip

    de, dn = so.synth_dataset(8, 1, use_ring=True)
    inputs, targets = so.pad_batch(de, dn, g_update, use_ring=True)
    inputs["atomic"] = np.random.default_rng(5).integers(0, 2, size=(101, 92)).astype("float32")[inputs["atomic"]]
    return _hip.pack_inputs(inputs), np.asarray(targets, np.float32)


def upload_tile_rows(pk):
    """the edge-tile height scann_batch_upload picks (scann_batch.cpp upload_impl), from the host planner"""
    from scann import _hip

    small = 0 < pk.n_edge <= EDGE_TILE_32_MAX_EDGES
    rows, _, part, _ = _hip.plan_tiles(pk, 32 if small else 64)
    if small and int(np.diff(pk.edge_offset).max()) > EDGE_TILE_32_MAX_DEGREE:
        rows, _, part, _ = _hip.plan_tiles(pk, 64)
    return rows, int((part >= 0).sum())


# ---- batches whose [rows, 128] tensors pass 2^31 bytes, up to the upload limit (tests/test_gpu_large_rows.py) ----
# Each is a seeded batch above tiled with _hip.concat_packed (NumPy only): (PackedBatch, replicas, the small batch it is made of).
# A replica's rows in the large batch are the small batch's rows shifted by r * n_atom / r * n_edge, so every per-replica result of
# the large batch reshapes to [replicas, ...] against the small batch forwarded alone.

LIMIT_FILLER_ATOMS, LIMIT_REPLICAS = 230, 234  # qm9_at_limit: 234 x 35,837 = 8,385,858 edges, the filler brings the other 2,749


def replicated(small, n):
    from scann import _hip

    return _hip.concat_packed([small] * n)


def qm9_x118(g_update=True):
    """qm9_b260 118 times: 563,922 atoms, 4,228,766 edges -- the edge tensors pass 2^31 bytes, the atom tensors do not"""
    small, _ = qm9_b260(g_update)
    return replicated(small, 118), 118, small


def sparse_x123(g_update=True):
    """sparse_atoms 123 times: 4,210,413 atoms (isolated ones among them), 6,304,365 edges -- atom and edge tensors pass 2^31 bytes"""
    small, _ = sparse_atoms(g_update)
    return replicated(small, 123), 123, small


@functools.lru_cache(maxsize=None)
def limit_filler_data(extra=0):
    """one structure of 230 atoms: 229 with 12 neighbours each and one with 1 + `extra` -- 2,749 + `extra` edges, every degree given"""
    degrees = {a: 12 for a in range(LIMIT_FILLER_ATOMS - 1)}
    degrees[LIMIT_FILLER_ATOMS - 1] = 1 + extra
    de, dn = np.empty(1, dtype=object), np.empty(1, dtype=object)
    de[0], dn[0] = hub_structure(np.random.default_rng(2749), LIMIT_FILLER_ATOMS, degrees)
    return de, dn


def limit_filler(g_update=True, extra=0):
    """the filler structure alone: PackedBatch"""
    return packed(limit_filler_data(extra), g_update)[0]


def qm9_at_limit(g_update=True, extra=0):
    """qm9_b260 234 times, then the filler structure: n_edge is exactly UPLOAD_MAX_ROWS (+ `extra`).  The filler is last: its edge rows
    are the last rows below 2^32 bytes, and the spare row behind them ends 4 bytes below 2^32"""
    from scann import _hip

    small, _ = qm9_b260(g_update)
    return _hip.concat_packed([small] * LIMIT_REPLICAS + [limit_filler(g_update, extra)]), LIMIT_REPLICAS, small


def qm9_over_limit(g_update=True):
    """qm9_at_limit with one more edge in the filler: the first batch scann_batch_upload refuses"""
    return qm9_at_limit(g_update, extra=1)
