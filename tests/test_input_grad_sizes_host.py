"""CPU: what tests/test_gpu_input_grad_sizes.py takes for granted -- the ring / cgcnn variants of the size batches are what the GPU
tests take them for, no batch of its table has a structure whose reference is not finite, and the per-structure normalisation shows a
small structure's error undiluted."""
import zlib

import numpy as np
import pytest

import size_batches as sb
import test_gpu_input_grad_sizes as igs
import test_gpu_input_grads as ig


def test_general_embedding_variants_are_what_they_are_named(hip_lib):
    """cgcnn64_base: qm9_b260's graph with [n_atom, 92] 0 / 1 features and no atomic numbers; ring64: [n_atom, 2] flags; chunked_ring:
    seeded flags on `chunked`, still 17 chunk tiles on 64 rows under the host planner; small_general: both inputs on 32-row tiles.
    The drawn features are pinned by checksum"""
    from scann.parallel import slice_packed

    base, _ = sb.qm9_b260(False)
    pk, targets = sb.qm9_b260_cgcnn(False)
    assert pk.atomic is None and pk.ring is None and pk.cgcnn.shape == (base.n_atom, 92) and pk.cgcnn.dtype == np.float32
    assert set(np.unique(pk.cgcnn)) == {0.0, 1.0} and len(targets) == pk.n_struct == 260
    for k in ("mol_offset", "edge_offset", "edge_col", "edge_dist", "edge_weight"):
        assert np.array_equal(getattr(pk, k), getattr(base, k)), k
    assert sb.upload_tile_rows(pk) == (64, 0)
    assert sb.crosses("qm9_b260", pk.n_atom, pk.n_edge, int(np.diff(pk.edge_offset).max()), 64, 0)
    sub = slice_packed(pk, 3, 5)
    assert sub.atomic is None and np.array_equal(sub.cgcnn, pk.cgcnn[pk.mol_offset[3]:pk.mol_offset[5]])
    assert zlib.crc32(pk.cgcnn.tobytes()) == CRC["qm9_b260_cgcnn"]

    ring, _ = sb.qm9_ring_b260()
    assert ring.ring.shape == (ring.n_atom, 2) and set(np.unique(ring.ring)) == {0.0, 1.0} and ring.cgcnn is None

    plain, _ = sb.chunked()
    pk, targets = sb.chunked_ring()
    assert pk.ring.shape == (pk.n_atom, 2) and set(np.unique(pk.ring)) == {0.0, 1.0} and pk.cgcnn is None and len(targets) == 3
    assert np.array_equal(pk.atomic, plain.atomic) and np.array_equal(pk.edge_col, plain.edge_col)
    assert sb.upload_tile_rows(pk) == sb.upload_tile_rows(plain) == (64, 17)
    assert 0.3 < pk.ring.mean() < 0.7 and zlib.crc32(pk.ring.tobytes()) == CRC["chunked_ring"]

    pk, targets = sb.small_general()
    assert pk.n_struct == 8 and len(targets) == 8 and pk.atomic is None
    assert pk.ring.shape == (pk.n_atom, 2) and pk.cgcnn.shape == (pk.n_atom, 92)
    assert sb.upload_tile_rows(pk) == (32, 0) and sb.small_side(pk.n_atom, pk.n_edge)
    assert zlib.crc32(pk.cgcnn.tobytes()) == CRC["small_general"]


CRC = {"qm9_b260_cgcnn": 1580619626, "chunked_ring": 1998904840, "small_general": 1047933743}  # zlib.crc32 of the float32 bytes


class _Cache(dict):
    def __call__(self, key, make):
        if key not in self:
            self[key] = make()
        return self[key]


def sampled_structures(pk):
    """the first and the last structure, the smallest, the largest, and the one with the most atoms without a neighbour"""
    sizes = np.diff(pk.mol_offset)
    lone = np.add.reduceat((np.diff(pk.edge_offset) == 0).astype(np.int64), pk.mol_offset[:-1].astype(np.int64))
    return sorted({0, pk.n_struct - 1, int(np.argmin(sizes)), int(np.argmax(sizes)), int(np.argmax(lone))})


@pytest.mark.parametrize("case", list(igs.CASES))
def test_no_structure_of_the_table_has_an_undefined_reference(hip_lib, case):
    """The per-structure check of the GPU module may skip no structure, and counts an empty gradient as equal: so no batch of its table
    may have a one-atom structure (y = NaN under use_ga_norm) or a structure without edges.  The fp64 reference (y and every leaf) of
    sampled structures -- among them the smallest, the 2-atom crystal 122 of mp2018_b128 -- is finite; the GPU module asserts the same of
    the whole batch's reference where it computes it"""
    import input_grad_ref
    from scann.parallel import slice_packed

    cfg, w, pk, targets, _ = igs.case_of(_Cache(), case)
    assert cfg["model"]["use_ga_norm"] and len(targets) == pk.n_struct
    mol = pk.mol_offset.astype(np.int64)
    sizes, edges = np.diff(mol), np.diff(pk.edge_offset.astype(np.int64)[mol])
    assert sizes.min() >= 2 and edges.min() >= 1, (int(sizes.min()), int(edges.min()))
    if case.startswith("mp"):
        assert int(np.argmin(sizes)) == 122 and sizes[122] == 2
    if case.startswith("sparse"):
        assert int((np.diff(pk.edge_offset) == 0).sum()) == 8577
    for s in sampled_structures(pk):
        y, ref = input_grad_ref.input_grads(cfg, w, slice_packed(pk, s, s + 1))
        assert set(ref) == set(ig.wrt_of(cfg))
        assert np.isfinite(y).all() and all(np.isfinite(r).all() for r in ref.values()), (case, s)
        assert all(np.abs(r).max() > 0 for r in ref.values()), (case, s)


def test_structure_errors_are_normalised_by_the_structure_itself(hip_lib):
    """three structures of 2, 3 and 2 atoms with 2, 5 and 3 edges (one atom without a neighbour); the middle one's gradients are 1e-4
    of the others'.  A perturbation of one of ITS edges by 1 % of its own largest entry shows as 1e-2 on that structure and nowhere
    else, where errors() -- normalised by the batch -- sees 1e-6"""
    from scann import _hip

    mol = [0, 2, 5, 7]
    eoff = [0, 1, 2, 4, 4, 7, 9, 10]
    col = [1, 0, 3, 4, 2, 2, 3, 6, 5, 5]
    pk = _hip.PackedBatch(np.ones(7, np.int32), mol, eoff, col, np.ones(10, np.float32), np.ones(10, np.float32))
    rng = np.random.default_rng(0)
    scale_e = np.array([1.0] * 2 + [1e-4] * 5 + [1.0] * 3)
    scale_a = np.array([1.0] * 2 + [1e-4] * 3 + [1.0] * 2)
    ref = {"neighbor_distance": rng.uniform(0.5, 1.0, 10) * scale_e, "neighbor_weight": rng.uniform(0.5, 1.0, 10) * scale_e,
           "atomic": rng.uniform(0.5, 1.0, (7, 92)) * scale_a[:, None]}
    zero = ig.structure_errors(ref, ref, pk)
    assert all(v.shape == (3,) and not v.any() for v in zero.values())
    got = {k: v.copy() for k, v in ref.items()}
    top = np.abs(ref["neighbor_distance"][2:7]).max()
    got["neighbor_distance"][4] += 0.01 * top
    got["atomic"][3, 17] -= 0.02 * np.abs(ref["atomic"][2:5]).max()
    e = ig.structure_errors(got, ref, pk)
    assert np.allclose(e["neighbor_distance"], [0, 0.01, 0], rtol=1e-9, atol=0) and not e["neighbor_weight"].any()
    assert np.allclose(e["atomic"], [0, 0.02, 0], rtol=1e-9, atol=0)
    assert ig.errors(got, ref)["neighbor_distance"] < 2e-6  # (diluted by the batch maximum)
    # every structure's figure is its own: worst entry over its own largest reference entry
    got = {k: v * (1 + 1e-3) for k, v in ref.items()}
    e = ig.structure_errors(got, ref, pk)
    assert all(np.allclose(v, 1e-3, rtol=1e-6) for v in e.values())
    # a structure without edges counts as equal in the edge leaves and does not shift its neighbours' rows
    lone = _hip.PackedBatch(np.ones(4, np.int32), [0, 2, 3, 4], [0, 1, 2, 2, 2], [1, 0], np.ones(2, np.float32), np.ones(2, np.float32))
    r = {"neighbor_weight": np.array([1.0, 2.0]), "ring_aromatic": np.ones((4, 2))}
    g = {"neighbor_weight": np.array([1.0, 2.2]), "ring_aromatic": np.ones((4, 2)) + np.array([0, 0, 0, 0.5])[:, None]}
    e = ig.structure_errors(g, r, lone)
    assert np.allclose(e["neighbor_weight"], [0.1, 0, 0]) and np.allclose(e["ring_aromatic"], [0, 0, 0.5])
