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
    assert "static int fused_tile_rows(int rows) { return rows <= 32 * 768 ? 32 : 64; }" in src("scann_train_fused.hip")
    assert sb.FUSED_TILE_ROWS_32_MAX == 32 * 768
    batch = src("scann_batch.cpp")
    assert "const bool small = E > 0 && E <= 32 * 1024;" in batch and "if (small && max_degree > 32) {" in batch
    assert "if ((size_t)max_atoms * 5 * sizeof(float) > 60000)" in batch
    assert sb.UPLOAD_MAX_ATOMS == 3000 and 3000 * 5 * 4 <= 60000 < 3001 * 5 * 4
    assert "db->tile_rows == 32 && db->n_big == 0 && db->max_degree <= 16" in src("scann_train_host.cpp")
    assert "((size_t)3 * db->max_atoms + 4) * sizeof(double) > 65536" in src("scann_train_host.cpp")
    assert sb.GEN_BWD_MAX_ATOMS == 2729 and (3 * 2729 + 4) * 8 <= 65536 < (3 * 2730 + 4) * 8
    assert "const int rows = a.n_atom <= 32 * 1024 ? 32 : 64;" in src("scann_kernels.hip")
    train = src("scann_train.hip")
    assert "return std::min(8, std::max(1, (n_atom + 4095) / 4096));" in train
    assert "return std::max(std::min(4, tiles), (tiles + 79) / 80);" in train
    assert len(re.findall(r"bytes >= \(\(size_t\)24 << 20\)", train)) == 1 and "bytes < ((size_t)24 << 20)" in train
    assert "return std::min(32, std::max(1, (rows + 32 * 1536 - 1) / (32 * 1536)));" in train
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
