"""CPU: the batches of tests/size_batches.py cross the size switches they are built for, so that tests/test_gpu_sizes.py does not
quietly run the small side again if a threshold moves or the generator changes; and the thresholds restated there still match the
source lines they cite."""
import os
import re

import numpy as np
import pytest

import size_batches as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scann--material_amd", "csrc")


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_thresholds_match_the_launch_code():
    """each constant against the expression of the line it mirrors"""
    slots = src("scann_train_slots.h")  # the training backward's partitions, stated once for launcher and bound
    assert "inline Split fused_split(int rows) { return split(rows, rows <= 32 * 768 ? 32 : 64); }" in slots
    assert "fused_split(a.n_atom)" in src("scann_train_fused.hip") and "fused_split(a.n_edge)" in src("scann_train_fused.hip")
    assert sb.FUSED_TILE_ROWS_32_MAX == 32 * 768
    batch = src("scann_batch.cpp")
    assert "const bool small = E > 0 && E <= 32 * 1024;" in batch and "if (small && max_degree > 32) {" in batch
    assert "if ((size_t)max_atoms * 5 * sizeof(float) > 60000)" in batch
    assert sb.UPLOAD_MAX_ATOMS == 3000 and 3000 * 5 * 4 <= 60000 < 3001 * 5 * 4
    assert "if ((uint64_t)std::max(A, E) * D * 4 >= (1ull << 32))" in batch and "constexpr int D = 128;" in src("scann_internal.h")
    assert "scann_batch_upload: more than 8,388,607 atoms or edges in one batch; split it" in batch
    assert sb.UPLOAD_MAX_ROWS == 8388607 and sb.UPLOAD_MAX_ROWS * 128 * 4 < 1 << 32 <= (sb.UPLOAD_MAX_ROWS + 1) * 128 * 4
    assert sb.SIGNED_OFFSET_ROWS == 4194304 and sb.SIGNED_OFFSET_ROWS * 128 * 4 == 1 << 31
    assert "db->tile_rows == 32 && db->n_big == 0 && db->max_degree <= 16" in src("scann_train_host.cpp")
    assert "((size_t)3 * db->max_atoms + 4) * sizeof(double) > 65536" in src("scann_train_host.cpp")
    assert sb.GEN_BWD_MAX_ATOMS == 2729 and (3 * 2729 + 4) * 8 <= 65536 < (3 * 2730 + 4) * 8
    assert "const int rows = a.n_atom <= 32 * 1024 ? 32 : 64;" in src("scann_kernels.hip")
    train = src("scann_train.hip")
    assert "return std::min(8, std::max(1, (n_atom + 4095) / 4096));" in slots and "attn_bwd_apw(n_atom, max_degree)" in train
    assert "return std::max(std::min(4, tiles), (tiles + 79) / 80);" in slots and "wgrad_chunks(" not in train
    assert len(re.findall(r"bytes >= \(\(size_t\)24 << 20\)", train)) == 1 and "bytes < ((size_t)24 << 20)" in train
    assert "return std::min(32, std::max(1, (rows + 32 * 1536 - 1) / (32 * 1536)));" in slots and "ln_bwd_groups(rows)" in train
    assert "int gen_ln_chunks(int rows) { return std::max(1, std::min(512, (rows + 63) / 64)); }" in src("scann_generic_train.hip")
    # the training forward of the plain-fp32 path refuses what its backward cannot run
    assert "if (kp && ((size_t)3 * db->max_atoms + 4) * sizeof(double) > 65536)" in src("scann_forward.cpp")


def test_wgrad_partition_restatement():
    assert [sb.wgrad_chunks(r) for r in (1, 64, 256, 20480, 20481, 43462)] == [1, 1, 4, 4, 5, 9]
    for rows in (1, 63, 64, 4000, 20480, 20481, 43462, 51255):
        c, s = sb.wgrad_chunks(rows), sb.wgrad_slabs(rows)
        assert s <= 80 and s * 64 * c >= rows > (s - 1) * 64 * c


@pytest.mark.parametrize("name", ["mp2018_b128", "qm9_b260", "qm9_ring_b260", "sparse_atoms"])
def test_size_batches_cross_their_thresholds(hip_lib, name):
    pk, targets = getattr(sb, name)()
    deg = np.diff(pk.edge_offset)
    rows, n_big = sb.upload_tile_rows(pk)
    assert len(targets) == pk.n_struct and np.isfinite(targets).all()
    assert n_big == 0 and rows == 64
    assert sb.crosses(name, pk.n_atom, pk.n_edge, int(deg.max()), rows, n_big), (pk.n_atom, pk.n_edge, int(deg.max()))
    assert not sb.small_side(pk.n_atom, pk.n_edge)
    # the measured sizes (a changed generator shows here first)
    assert (pk.n_struct, pk.n_atom, pk.n_edge, int(deg.max())) == {
        "mp2018_b128": (128, 3252, 43462, 24), "qm9_b260": (260, 4779, 35837, 12), "qm9_ring_b260": (260, 4742, 35569, 12),
        "sparse_atoms": (1900, 34231, 51255, 3)}[name]
    if name == "qm9_ring_b260":
        assert pk.ring is not None and np.asarray(pk.ring).shape == (pk.n_atom, 2)
    if name == "sparse_atoms":
        assert (deg == 0).sum() > 1000 and sb.layer_wgrad_bytes(pk.n_atom, pk.n_edge) >= sb.WGRAD_REDUCE4_BYTES
    if name == "mp2018_b128":
        assert sb.wgrad_chunks(pk.n_edge) > 4 and pk.n_edge % (64 * sb.wgrad_chunks(pk.n_edge)) != 0  # the last chunk is partial


@pytest.mark.parametrize("g_update", [True, False])
def test_deg40_is_on_64_row_edge_tiles_by_its_degree_alone(hip_lib, g_update):
    """few edges, no chunk tiles: only `max_degree > 32` sends it to 64-row tiles -- and each part of it alone is where
    tests/test_gpu_mc_sizes.py expects it (the flanking molecules on 32 rows, the structure itself on 64)"""
    from scann.parallel import slice_packed

    pk, targets = sb.deg40(g_update)
    deg = np.diff(pk.edge_offset)
    mid = pk.n_struct // 2
    a0, a1 = int(pk.mol_offset[mid]), int(pk.mol_offset[mid + 1])
    assert pk.n_struct == 7 and len(targets) == 7 and a1 - a0 == 48
    assert 0 < pk.n_edge <= 2048 < sb.EDGE_TILE_32_MAX_EDGES and pk.n_atom <= sb.ATOM_TILE_32_MAX
    assert sorted(deg[a0:a1])[-2:] == [sb.EDGE_TILE_32_MAX_DEGREE + 1, 40] and sorted(deg[a0:a1])[-3] <= 8
    assert max(deg[:a0].max(), deg[a1:].max()) <= 12
    assert sb.upload_tile_rows(pk) == (64, 0)
    assert sb.upload_tile_rows(slice_packed(pk, 0, mid)) == (32, 0) and sb.upload_tile_rows(slice_packed(pk, mid + 1, pk.n_struct)) == (32, 0)
    assert sb.upload_tile_rows(slice_packed(pk, mid, mid + 1)) == (64, 0)


@pytest.mark.parametrize("g_update", [True, False])
def test_chunked_has_chunk_tiles(hip_lib, g_update):
    """six atoms above 64 neighbours: chunk tiles (part >= 0) on 64-row tiles, in the batch and in the structure alone"""
    from scann.parallel import slice_packed

    pk, targets = sb.chunked(g_update)
    deg = np.diff(pk.edge_offset)
    a0 = int(pk.mol_offset[1])
    assert pk.n_struct == 3 and len(targets) == 3 and int(pk.mol_offset[2]) - a0 == 220
    assert {a: int(deg[a0 + a]) for a in sb.CHUNKED_DEGREES} == sb.CHUNKED_DEGREES
    assert int((deg > 64).sum()) == 6 and pk.n_edge <= sb.EDGE_TILE_32_MAX_EDGES
    rows, n_chunk = sb.upload_tile_rows(pk)
    # 219, 65, 128, 129, 200, 70 neighbours in chunks of at most 64
    assert rows == 64 and n_chunk == sum((d + 63) // 64 for d in sb.CHUNKED_DEGREES.values() if d > 64) == 17
    assert sb.upload_tile_rows(slice_packed(pk, 0, 1)) == (32, 0) and sb.upload_tile_rows(slice_packed(pk, 2, 3)) == (32, 0)
    assert sb.upload_tile_rows(slice_packed(pk, 1, 2)) == (64, n_chunk)


@pytest.mark.parametrize("n", [sb.GEN_BWD_MAX_ATOMS, sb.GEN_BWD_MAX_ATOMS + 1, sb.UPLOAD_MAX_ATOMS, sb.UPLOAD_MAX_ATOMS + 1])
def test_giant_structure_batches(hip_lib, n):
    pk, targets = sb.giant(n)
    sizes = np.diff(pk.mol_offset)
    deg = np.diff(pk.edge_offset)
    assert pk.n_struct == 3 and sizes[1] == n and sizes.max() == n and len(targets) == 3
    assert (deg[sizes[0]:sizes[0] + n] == 12).all()
    rows, n_big = sb.upload_tile_rows(pk)
    assert n_big == 0 and sb.crosses("giant", pk.n_atom, pk.n_edge, int(deg.max()), rows, n_big)


def test_sub_batches_of_the_split_sum_are_small(hip_lib):
    """every sub-batch test_gpu_sizes cuts is planned at 32 rows, on the small side"""
    from scann import _hip
    from scann.parallel import slice_packed

    for name in ("mp2018_b128", "qm9_b260", "sparse_atoms"):
        pk, _ = getattr(sb, name)()
        cuts = sb.small_cuts(pk)
        assert cuts[0][0] == 0 and cuts[-1][1] == pk.n_struct and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
        assert len(cuts) >= 2
        for lo, hi in cuts:
            sub = slice_packed(pk, lo, hi)
            assert sb.small_side(sub.n_atom, sub.n_edge) and sb.upload_tile_rows(sub) == (32, 0), (name, lo, hi)
            assert _hip.plan_tiles(sub, 32)[0] == 32


def _is_replicated(big, n, small, a0=0, e0=0):
    """structures / atoms / edges of `big` from atom a0 / edge e0 on are `small` n times over, each replica's indices shifted by its rows"""
    A, E, B = small.n_atom, small.n_edge, small.n_struct
    a_shift = (a0 + A * np.arange(n, dtype=np.int64))[:, None]
    e_shift = (e0 + E * np.arange(n, dtype=np.int64))[:, None]
    s0 = int(np.searchsorted(big.mol_offset, a0))
    ok = np.array_equal(big.mol_offset[s0 + 1:s0 + 1 + n * B].reshape(n, B), small.mol_offset[1:][None] + a_shift)
    ok = ok and np.array_equal(big.edge_offset[a0 + 1:a0 + 1 + n * A].reshape(n, A), small.edge_offset[1:][None] + e_shift)
    ok = ok and np.array_equal(big.edge_col[e0:e0 + n * E].reshape(n, E), small.edge_col[None] + a_shift)
    ok = ok and np.array_equal(big.atomic[a0:a0 + n * A].reshape(n, A), np.broadcast_to(small.atomic, (n, A)))
    for name in ("edge_dist", "edge_weight"):
        ok = ok and np.array_equal(getattr(big, name)[e0:e0 + n * E].reshape(n, E), np.broadcast_to(getattr(small, name), (n, E)))
    return bool(ok)


@pytest.mark.parametrize("g_update", [True, False])
def test_replicated_batches_pass_two_to_the_31_bytes(hip_lib, g_update):
    """qm9_x118: only the edge tensors pass 2^31 bytes; sparse_x123: atom and edge tensors both; neither reaches the upload limit; both
    stay on 64-row tiles without chunk tiles, and every replica is the small batch with its rows shifted"""
    from scann import _hip

    big, n, small = sb.qm9_x118(g_update)
    assert n == 118 and (small.n_struct, small.n_atom, small.n_edge) == (260, 4779, 35837)
    assert (big.n_struct, big.n_atom, big.n_edge) == (118 * 260, 563922, 4228766)
    assert big.n_atom < sb.SIGNED_OFFSET_ROWS < big.n_edge <= sb.UPLOAD_MAX_ROWS
    assert big.n_edge * 128 * 4 > 1 << 31 and big.n_edge * 256 * 4 > 1 << 32  # (the 256-wide case: past 2^32 bytes)
    assert _is_replicated(big, n, small) and sb.upload_tile_rows(big) == (64, 0)
    assert _hip.plan_tiles_filled(big, 64, 24)[0]  # (best fit saves tiles: a second forward runs on the filled plan)
    big, n, small = sb.sparse_x123(g_update)
    assert n == 123 and (small.n_struct, small.n_atom, small.n_edge) == (1900, 34231, 51255)
    assert (big.n_struct, big.n_atom, big.n_edge) == (123 * 1900, 4210413, 6304365)
    assert sb.SIGNED_OFFSET_ROWS < big.n_atom < big.n_edge <= sb.UPLOAD_MAX_ROWS
    assert int((np.diff(big.edge_offset) == 0).sum()) > 123 * 1000
    assert _is_replicated(big, n, small) and sb.upload_tile_rows(big) == (64, 0)
    assert not _hip.plan_tiles_filled(big, 64, 24)[0]  # (degrees 0 .. 3: the atom limit closes the tiles of either plan)


@pytest.mark.parametrize("g_update", [True, False])
def test_limit_batches_sit_on_either_side_of_the_upload_limit(hip_lib, g_update):
    """qm9_at_limit: exactly UPLOAD_MAX_ROWS edges, the filler structure (229 atoms of 12 neighbours, one of 1) last, so that its rows are
    the last below 2^32 bytes and the spare row behind them ends 4 bytes short of 2^32; qm9_over_limit: one edge more"""
    from scann import _hip
    from scann.parallel import slice_packed

    big, n, small = sb.qm9_at_limit(g_update)
    assert n == 234 and n * small.n_edge == 8385858
    assert big.n_struct == 234 * 260 + 1 and big.n_atom == 234 * 4779 + 230 and big.n_edge == sb.UPLOAD_MAX_ROWS
    assert (big.n_edge + 1) * 128 * 4 == 1 << 32  # (the spare row: bytes [2^32 - 512, 2^32))
    assert big.n_edge * 64 * 4 == (1 << 31) - 256  # (the 64-wide case: the last row of an [E, 64] tensor is the last below 2^31 bytes)
    assert _is_replicated(big, n, small) and sb.upload_tile_rows(big) == (64, 0) and _hip.plan_tiles_filled(big, 64, 24)[0]
    filler, last = sb.limit_filler(g_update), slice_packed(big, big.n_struct - 1, big.n_struct)
    deg = np.diff(filler.edge_offset)
    assert filler.n_struct == 1 and filler.n_atom == 230 and filler.n_edge == 2749
    assert (deg[:229] == 12).all() and deg[229] == 1
    assert _is_replicated(last, 1, filler)
    over, n2, _ = sb.qm9_over_limit(g_update)
    assert n2 == 234 and over.n_edge == sb.UPLOAD_MAX_ROWS + 1 and over.n_atom == big.n_atom and over.n_struct == big.n_struct
    assert np.diff(over.edge_offset)[-1] == 2 and _is_replicated(over, n2, small)
    assert np.array_equal(over.edge_offset[:-1], big.edge_offset[:-1])
