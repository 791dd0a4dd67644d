"""CPU tests of the local-attention / representation outputs' host side: the packed -> padded scatter against the oracle's own padded
arrays (the 0 and 1/N conventions of the reference's fp32 softmax included), the per-structure split predict_dataset uses, and the
validation of output names."""
import numpy as np
import pytest

import scann_oracle as so


def _batch_with_corners(seed=3):
    """A QM9-shaped padded batch with an isolated real atom, padded atoms and padded neighbour slots."""
    de, dn = so.synth_dataset(7, seed)
    inputs, _ = so.pad_batch(de, dn, True)
    inputs = {k: np.array(v) for k, v in inputs.items()}
    inputs["neighbor_mask"][2, 1, :] = False  # atom 1 of structure 2 loses every neighbour
    return inputs


def _packed_of(padded_attn, inputs):
    """what the kernels return for one layer: the weights of the real slots of real atoms, in np.nonzero order"""
    em = inputs["neighbor_mask"] & (inputs["atom_mask"][..., 0] != 0)[:, :, None]
    return padded_attn.transpose(0, 2, 3, 1)[em]  # [B,H,M,N] -> [n_edge, H]


def test_local_attention_scatter_reproduces_the_oracles_padded_maps():
    from scann import _hip

    cfg = so.default_config("qm9")
    w = so.init_weights(cfg, 1234, perturb=True)
    inputs = _batch_with_corners()
    inter = {}
    so.forward(cfg, w, inputs, np.float32, intermediates=inter)
    amask = inputs["atom_mask"][..., 0] != 0
    em = inputs["neighbor_mask"] & amask[:, :, None]
    N = em.shape[2]
    for k in range(cfg["model"]["n_attention"]):
        ref = inter["attn_local_%d" % (k + 1)]  # [B, H, M, N]: the oracle's attn_local_<k+1> is local_attention_<k>
        got = _hip.repad_local_attention(_packed_of(ref, inputs), inputs["atom_mask"], inputs["neighbor_mask"])
        assert got.shape == ref.shape and got.dtype == np.float32
        assert np.array_equal(got, ref), k  # bit for bit: the scatter adds nothing the graph does not give
        # the conventions themselves, as the oracle's fp32 graph gives them
        has = em.any(-1)
        assert np.all(got.transpose(0, 2, 1, 3)[~has] == np.float32(1.0) / np.float32(N))  # padded and isolated atoms: 1/N
        assert not got.transpose(0, 2, 3, 1)[has[:, :, None] & ~em].any()  # masked slots of atoms with a neighbour: exactly 0
    assert (~em.any(-1) & amask).any() and (~amask).any()  # the batch has both corners
    z = _hip.repad_atoms(inter["after_Lc"][amask], inputs["atom_mask"])
    assert np.array_equal(z, inter["after_Lc"] * amask[..., None]) and not z[~amask].any()  # padded atoms: 0
    with pytest.raises(ValueError):
        _hip.repad_local_attention(np.zeros((3, 8), np.float32), inputs["atom_mask"], inputs["neighbor_mask"])


def test_per_structure_split_matches_each_batchs_padded_layout():
    """predict_dataset's split of a fused group: structure s's array is the padded array of its own dataset batch, row s."""
    from scann import _hip
    from scann.models.scann_model import HipModel

    de, dn = so.synth_dataset(11, 8)
    counts = [4, 4, 3]  # a fused group of three dataset batches
    batches, parts = [], []
    b0 = 0
    for c in counts:
        inputs, _ = so.pad_batch(de[b0:b0 + c], dn[b0:b0 + c], True)
        batches.append(inputs)
        parts.append(_hip.pack_inputs(inputs))
        b0 += c
    pk = _hip.concat_packed(parts)
    rng = np.random.default_rng(0)
    packed = {"local_attention_1": rng.random((pk.n_edge, 8), dtype=np.float32),
              "after_Lc": rng.random((pk.n_atom, 128), dtype=np.float32),
              "bf_property": rng.random((pk.n_struct, 128), dtype=np.float32)}
    per = {n: [] for n in packed}
    HipModel._split_outputs(None, packed, pk, counts, per)
    assert all(len(v) == 11 for v in per.values())
    s = e0 = a0 = 0
    for inputs, part in zip(batches, parts):
        attn = _hip.repad_local_attention(packed["local_attention_1"][e0:e0 + part.n_edge], inputs["atom_mask"], inputs["neighbor_mask"])
        z = _hip.repad_atoms(packed["after_Lc"][a0:a0 + part.n_atom], inputs["atom_mask"])
        for i in range(part.n_struct):
            assert np.array_equal(per["local_attention_1"][s], attn[i])
            assert np.array_equal(per["after_Lc"][s], z[i])
            assert np.array_equal(per["bf_property"][s], packed["bf_property"][s])
            s += 1
        e0 += part.n_edge
        a0 += part.n_atom


def test_output_names_are_validated():
    from scann.models.scann_model import _output_selection

    names, layers, z, bf = _output_selection(["bf_property", "local_attention_2", "predict_property", "local_attention_0", "after_Lc"], 3)
    assert names == ["bf_property", "local_attention_2", "predict_property", "local_attention_0", "after_Lc"]
    assert layers == [0, 2] and z and bf
    assert _output_selection("global_attention", 3) == (["global_attention"], [], False, False)
    for bad in (["local_attention_3"], ["local_attention_-1"], ["local_attention_01"], ["local_attention_x"], ["attn"],
                ["After_Lc"], [3]):
        with pytest.raises(ValueError):
            _output_selection(bad, 3)
