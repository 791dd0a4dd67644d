"""Host: the filled edge-tile plan of the inference edge kernels (scann_plan_tiles_filled, scann_pack.cpp) -- a tile's atoms need not be
a contiguous range of the batch.  What the kernels rely on: the atom order is a permutation that never leaves a structure; in that order
every atom's edges are contiguous and in their order; the tiles partition the atoms and the edges of that order within the two limits;
the plan never has more tiles than the contiguous one (it IS the contiguous one where best-fit does not win, and wherever an atom is
chunked).  And what it is for: 5 % fewer tiles on QM9-shaped launches of 10 and 16 batches, 10 % on crystals (bench.py's generators)."""
import numpy as np
import pytest

import size_batches as sb

ROWS_ATOMS = [(64, 24), (32, 24), (64, 5), (32, 3)]


def packed_of(degrees_per_structure):
    """a PackedBatch whose structure s has one atom per entry of degrees_per_structure[s], with that many neighbours (atoms of its own
    structure, round robin)"""
    from scann import _hip

    mol, eoff, col = [0], [0], []
    for degs in degrees_per_structure:
        a0, n = mol[-1], len(degs)
        for i, d in enumerate(degs):
            col += [a0 + (i + 1 + k) % n for k in range(d)]
            eoff.append(eoff[-1] + d)
        mol.append(a0 + n)
    A, E = mol[-1], eoff[-1]
    rng = np.random.default_rng(A + E)
    return _hip.PackedBatch(rng.choice([1, 6, 7, 8], A).astype(np.int32), np.asarray(mol, np.int32), np.asarray(eoff, np.int32),
                            np.asarray(col, np.int32), rng.uniform(0.9, 4.0, E).astype(np.float32), rng.uniform(0.1, 1.0, E).astype(np.float32))


def hand_built_32():
    """32-row tiles, one structure, degrees 20, 0, 20, 12, 32, 12: the contiguous plan is [20, 0] [20, 12] [32] [12], four tiles; best
    fit is [32, 0] [20, 12] [20, 12], three -- the atom of exactly 32 neighbours fills a tile's rows and the isolated atom still fits"""
    return packed_of([[20, 0, 20, 12, 32, 12]])


def check_plan(pk, rows, atoms):
    """every property the kernels rely on; returns (filled, n_tiles, n_contiguous)"""
    from scann import _hip

    rows_c, tiles_c, part_c, _ = _hip.plan_tiles(pk, rows, atoms)
    filled, atom_row, toff, tiles = _hip.plan_tiles_filled(pk, rows, atoms)
    A, E = pk.n_atom, pk.n_edge
    deg = np.diff(pk.edge_offset)
    # a permutation that maps every structure onto itself
    assert np.array_equal(np.sort(atom_row), np.arange(A))
    for s in range(pk.n_struct):
        a0, a1 = int(pk.mol_offset[s]), int(pk.mol_offset[s + 1])
        assert np.array_equal(np.sort(atom_row[a0:a1]), np.arange(a0, a1)), s
    # the offsets in tile order are those of the permuted degrees: an atom's edges are one contiguous run of its own length, and the
    # copy the upload makes (edge k of the atom -> toff + k) keeps their order
    assert toff[0] == 0 and toff[-1] == E and np.array_equal(np.diff(toff), deg[atom_row])
    src = np.concatenate([np.arange(pk.edge_offset[r], pk.edge_offset[r + 1]) for r in atom_row]) if E else np.zeros(0, np.int64)
    assert np.array_equal(np.sort(src), np.arange(E))
    for k in range(A):
        run = src[toff[k]:toff[k + 1]]
        assert np.array_equal(run, np.arange(pk.edge_offset[atom_row[k]], pk.edge_offset[atom_row[k] + 1]))
    # the tiles partition the tile-order atoms and edges, within the limits (a chunked atom's tiles -- the contiguous plan, which such
    # a batch gets -- share their atom and partition the edges alone)
    assert tiles[0, 0] == 0 and tiles[0, 2] == 0 and tiles[-1, 1] == A and tiles[-1, 3] == E
    assert np.array_equal(tiles[1:, 2], tiles[:-1, 3])
    n_atoms, n_edges = tiles[:, 1] - tiles[:, 0], tiles[:, 3] - tiles[:, 2]
    assert n_atoms.min() >= 1 and n_atoms.max() <= atoms and n_edges.max() <= rows_c
    if (part_c < 0).all():
        assert np.array_equal(tiles[1:, 0], tiles[:-1, 1])
        assert np.array_equal(tiles[:, 2], toff[tiles[:, 0]]) and np.array_equal(tiles[:, 3], toff[tiles[:, 1]])
    else:
        assert not filled
    # equal degrees keep their relative order inside a structure
    struct_of = np.repeat(np.arange(pk.n_struct), np.diff(pk.mol_offset))
    for s in range(pk.n_struct):
        a0, a1 = int(pk.mol_offset[s]), int(pk.mol_offset[s + 1])
        order = atom_row[a0:a1]
        for d in np.unique(deg[a0:a1]):
            same = order[deg[order] == d]
            assert np.all(np.diff(same) > 0), (s, d)
    assert np.array_equal(struct_of[atom_row], struct_of)
    # never more tiles than the contiguous plan; the identity where it is not fewer
    assert len(tiles) <= len(tiles_c)
    if filled:
        assert len(tiles) < len(tiles_c) and (part_c < 0).all()
    else:
        assert np.array_equal(atom_row, np.arange(A)) and np.array_equal(toff, pk.edge_offset) and np.array_equal(tiles, tiles_c)
    return filled, len(tiles), len(tiles_c)


def reference_plan(pk, rows, atoms):
    """the rule, restated: per structure the remaining atom of the largest degree that fits the open tile, the lowest row among equals;
    none fits, or the tile has its atoms: close it and take the largest; the open tile carries over.  -> (order, tiles closed)"""
    deg = np.diff(pk.edge_offset)
    order, n_tiles, used, held = [], 1, 0, 0
    for s in range(pk.n_struct):
        left = list(range(int(pk.mol_offset[s]), int(pk.mol_offset[s + 1])))
        while left:
            fit = [a for a in left if deg[a] <= rows - used] if held < atoms else []
            if not fit:
                n_tiles, used, held = n_tiles + 1, 0, 0
                fit = left
            best = max(deg[a] for a in fit)
            a = min(a for a in fit if deg[a] == best)
            left.remove(a)
            order.append(a)
            used, held = used + int(deg[a]), held + 1
    return np.asarray(order), n_tiles


def test_hand_built_32_row_case_saves_one_tile(hip_lib):
    from scann import _hip

    pk = hand_built_32()
    filled, n, n_c = check_plan(pk, 32, 24)
    _, atom_row, toff, tiles = _hip.plan_tiles_filled(pk, 32, 24)
    assert filled and (n, n_c) == (3, 4)
    assert atom_row.tolist() == [4, 1, 0, 3, 2, 5] and tiles.tolist() == [[0, 2, 0, 32], [2, 4, 32, 64], [4, 6, 64, 96]]
    assert toff.tolist() == [0, 32, 32, 52, 64, 84, 96]
    assert sb.upload_tile_rows(pk) == (32, 0)


@pytest.mark.parametrize("name", ["qm9_b260", "qm9_ring_b260", "mp2018_b128", "sparse_atoms", "deg40"])
@pytest.mark.parametrize("rows,atoms", ROWS_ATOMS)
def test_plan_properties_on_the_size_batches(hip_lib, name, rows, atoms):
    pk = getattr(sb, name)()[0]
    filled, n, n_c = check_plan(pk, rows, atoms)
    print(name, rows, atoms, filled, n, n_c)
    if int(np.diff(pk.edge_offset).max()) <= rows:
        from scann import _hip

        order, n_ref = reference_plan(pk, rows, atoms)
        _, atom_row, _, tiles = _hip.plan_tiles_filled(pk, rows, atoms)
        if filled:
            assert np.array_equal(atom_row, order) and len(tiles) == n_ref
        else:
            assert n_ref >= n_c


def test_chunked_atoms_get_the_identity(hip_lib):
    """an atom of more than `rows` neighbours (chunk tiles in the contiguous plan): the identity, whatever best-fit would save"""
    pk = sb.chunked()[0]
    for rows in (32, 64):
        filled, n, n_c = check_plan(pk, rows, 24)
        assert not filled and n == n_c
    pk = sb.deg40()[0]
    assert not check_plan(pk, 32, 24)[0]  # 40 > 32: chunked at 32 rows
    pk = packed_of([[20, 0, 20, 12, 33, 12]])
    assert not check_plan(pk, 32, 24)[0] and check_plan(pk, 64, 24)[1] <= 2


def test_best_fit_that_loses_gets_the_identity(hip_lib):
    """32-row tiles, degrees 15, 9, 6, 12, 12, 6: the caller's order packs [15, 9, 6] [12, 12, 6] = 30 + 30, two tiles; best fit takes
    [15, 12], then [12, 9, 6] and is left with the last 6 -- three.  The plan is the caller's"""
    pk = packed_of([[15, 9, 6, 12, 12, 6]])
    order, n_ref = reference_plan(pk, 32, 24)
    assert n_ref == 3
    filled, n, n_c = check_plan(pk, 32, 24)
    assert not filled and (n, n_c) == (2, 2)
    # ... and a tie (best fit needs as many tiles as the caller's order) is the identity too: "fewer", not "as few"
    pk = packed_of([[16, 16, 16, 16]])
    assert not check_plan(pk, 32, 24)[0]


def test_open_tile_carries_over_into_the_next_structure(hip_lib):
    from scann import _hip

    """[10, 3] [20, 7, 12] [5, 30] at 32 rows: the caller's order needs [10, 3] [20, 7] [12, 5] [30]; best fit [10, 3 | 12, 7] [20 | 5]
    [30] -- the first tile takes two atoms of the second structure, the second tile one of the third"""
    pk = packed_of([[10, 3], [20, 7, 12], [5, 30]])
    filled, atom_row, toff, tiles = _hip.plan_tiles_filled(pk, 32, 24)
    assert check_plan(pk, 32, 24) == (True, 3, 4)
    assert atom_row.tolist() == [0, 1, 4, 3, 2, 5, 6] and tiles[:, :2].tolist() == [[0, 4], [4, 6], [6, 7]]
    assert np.array_equal(atom_row, reference_plan(pk, 32, 24)[0])


def bench_group(kind, n_batches):
    import bench
    from scann import _hip

    rng = np.random.default_rng(1000)
    make = bench.synth_packed_crystals if kind == "mp2018" else bench.synth_packed_batch
    return _hip.concat_packed([make(rng, 128) for _ in range(n_batches)])


@pytest.mark.parametrize("kind,n_batches,cap", [("qm9", 10, 0.955), ("qm9", 16, 0.955), ("mp2018", 10, 0.91), ("mp2018", 16, 0.91)])
def test_fewer_tiles_on_the_benchmark_launches(hip_lib, kind, n_batches, cap):
    """bench.py's generators, seed 1000, 64-row tiles of at most 24 atoms: filled / contiguous tiles"""
    from scann import _hip

    pk = bench_group(kind, n_batches)
    _, tiles_c, _, _ = _hip.plan_tiles(pk, 64, 24)
    filled, atom_row, toff, tiles = _hip.plan_tiles_filled(pk, 64, 24)
    ratio = len(tiles) / len(tiles_c)
    print("%s x %d: %d edges, ceil(E / 64) = %d, %d -> %d tiles, ratio %.4f" % (kind, n_batches, pk.n_edge, -(-pk.n_edge // 64), len(tiles_c),
                                                                              len(tiles), ratio))
    assert filled and ratio <= cap, ratio
    assert np.array_equal(np.sort(atom_row), np.arange(pk.n_atom)) and np.array_equal(np.diff(toff), np.diff(pk.edge_offset)[atom_row])
    n_edges = tiles[:, 3] - tiles[:, 2]
    assert n_edges.max() <= 64 and (tiles[:, 1] - tiles[:, 0]).max() <= 24
