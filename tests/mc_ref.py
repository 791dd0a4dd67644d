"""NumPy twin of the Monte Carlo dropout masks of scann_predict_mc (csrc/scann_internal.h: mc_seed, drop_scale) and the torch fp64
restatement of one MC sample built on tests/torch_ref.forward_packed: its two Dropout(0.1) masks are substituted with the
structure-local ones, the attention-weight masks passed as attn_scale.  Test-only."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
DROP_TAG_EMBED, DROP_TAG_ATTN = 1000, 2000


def _mix(z):
    """splitmix64 finaliser on uint64 arrays"""
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def mc_seed(seed, t, key):
    """mc_seed(seed, t, key) elementwise (key may be an array)"""
    key = np.asarray(key, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = _mix(np.uint64(int(seed) & M64) + np.uint64(GOLDEN) * np.uint64(int(t) + 1))
        return _mix(z + np.uint64(GOLDEN) * (key + np.uint64(1)))


def drop_scale(seed, tag, idx, p):
    """drop_scale(seed, tag, idx, p) elementwise: seed and idx uint64 arrays of one shape (or broadcastable)"""
    seed = np.asarray(seed, dtype=np.uint64)
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = seed + np.uint64(GOLDEN) * (idx + np.uint64(1)) + (np.uint64(tag) << np.uint64(48))
        z = _mix(z)
    u = (z >> np.uint64(40)).astype(np.float64) / 16777216.0
    p32 = np.float32(p)
    return np.where(u < p32, 0.0, float(np.float32(1.0) / (np.float32(1.0) - p32)))


def atom_struct(pk):
    return np.repeat(np.arange(pk.n_struct), np.diff(pk.mol_offset))


def local_drop_twin(pk, t, keys, d):
    """a drop_scale_np stand-in for torch_ref.forward_packed: its (seed, tag, global index atom * d + column, p) calls answered with the
    structure-local masks of sample t"""
    s_of = atom_struct(pk)
    a0 = np.asarray(pk.mol_offset)[s_of]
    ks = np.asarray(keys, dtype=np.uint64)[s_of]

    def twin(seed, tag, idx, p):
        idx = np.asarray(idx, dtype=np.uint64)
        atom = (idx // np.uint64(d)).astype(np.int64)
        col = idx - atom.astype(np.uint64) * np.uint64(d)
        local = (atom - a0[atom]).astype(np.uint64) * np.uint64(d) + col
        return drop_scale(mc_seed(seed, t, ks[atom]), tag, local, p)

    return twin


def attn_scales(pk, seed, t, keys, H, L, p):
    """per layer [E, H] attention-weight factors of sample t (None when p == 0)"""
    if p == 0:
        return None
    s_of = atom_struct(pk)
    eoff = np.asarray(pk.edge_offset)
    row = np.repeat(np.arange(pk.n_atom), np.diff(eoff))
    e0 = eoff[np.asarray(pk.mol_offset)[s_of[row]]]
    local = (np.arange(pk.n_edge) - e0).astype(np.uint64)
    sd = mc_seed(seed, t, np.asarray(keys, dtype=np.uint64)[s_of[row]])
    hh = np.arange(H, dtype=np.uint64)
    return [drop_scale(sd[:, None], DROP_TAG_ATTN + l, local[:, None] * np.uint64(H) + hh[None, :], p) for l in range(L)]


def sample_ref(cfg, w, pk, seed, t, keys, p_drop, p_attn, monkeypatch):
    """y [B] of MC sample t in fp64 (torch_ref.forward_packed with the structure-local masks)"""
    import torch_ref

    m = cfg["model"]
    monkeypatch.setattr(torch_ref, "drop_scale_np", local_drop_twin(pk, t, keys, m["local_dim"]))
    y, ga = torch_ref.forward_packed(cfg, w, pk, "float64", drop=(seed, p_drop) if p_drop > 0 else None,
                                     attn_scale=attn_scales(pk, seed, t, keys, m["num_head"], m["n_attention"], p_attn))
    return np.asarray(y, np.float64).ravel(), np.asarray(ga, np.float64).ravel()
