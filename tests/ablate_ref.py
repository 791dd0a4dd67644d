"""Reference for the ablated poolings (scann_ablate_pooling / HipModel.atom_contributions): the prediction of a structure when atom_mask
is 1 on a kept set S of its atoms and 0 elsewhere.  In the reference graph atom_mask feeds nothing but GlobalAttention
(scann_model.py:329-447), so from the after_Lc rows of ONE forward (oracle.forward(..., intermediates=...)) each kept set is
oracle.global_attention with the edited mask and oracle.dense for the two head layers.  tests/test_ablate_host.py checks this shortcut
against the literal recipe: oracle.forward on inputs whose atom_mask is edited.  Packed layout throughout: per-atom arrays [n_atom]
with structure s at mol_offset[s]:mol_offset[s + 1].  Test-only."""
import numpy as np

import scann_oracle as so
from analysis_checks import rel_err

MODES = ("leave_one_out", "deletion", "insertion")


def kept_set(mode, n, order, e):
    """bool [n]: the atoms kept by entry e of a structure of n atoms; order = its atom indices by rank"""
    keep = np.ones(n, dtype=bool)
    if mode == "leave_one_out":
        keep[e] = False
    elif mode == "deletion":  # entry k - 1: all but the k highest-ranked
        keep[order[:e + 1]] = False
    elif mode == "insertion":  # entry k - 1: the k highest-ranked only
        keep[:] = False
        keep[order[:e + 1]] = True
    else:
        raise ValueError(mode)
    return keep


def after_lc(config, weights, inputs, dtype):
    """packed after_Lc rows [n_atom, global_dim] of the oracle's forward, and mol_offset"""
    inter = {}
    so.forward(config, weights, inputs, dtype, intermediates=inter)
    amask = np.asarray(inputs["atom_mask"]).reshape(inter["after_Lc"].shape[:2]) != 0
    return inter["after_Lc"][amask], np.concatenate([[0], np.cumsum(amask.sum(1))]).astype(np.int64)


def head(config, w, rep, dt):
    out = so.dense(so.dense(rep, w, "bf_property", dt, "swish"), w, "predict_property", dt)  # scann_model.py:437-447
    if config.get("hyper", {}).get("target") == "e_b":
        out = np.maximum(out, dt.type(0))  # mrelu (custom_layers.py:15); a NaN stays one
    return out


def pooled(config, w, z, keep, dt):
    """y [V] of one structure for V kept sets: z [n, dg] after_Lc rows, keep [V, n] bool"""
    V = keep.shape[0]
    zz = np.broadcast_to(z.astype(dt)[None], (V,) + z.shape)
    _, rep = so.global_attention(w, config["model"], zz, keep.astype(dt)[..., None], dt)
    return head(config, w, rep, dt)[:, 0]


def ablate(config, weights, z, mol_offset, mode, order, dtype, entries=None):
    """(ablated [n_atom], y [n_struct]) in `dtype`: entry e of structure s at mol_offset[s] + e, y = the full pooling from the same rows.
    order [n_atom]: structure-local atom index by rank (the GPU's; unused for leave_one_out).  entries: {s: [e, ...]} to compute only
    those (the others stay NaN), for structures too large to ablate entry by entry on the CPU."""
    dt = np.dtype(dtype)
    w = {k: np.asarray(v).astype(dt) for k, v in weights.items()}
    n_struct = len(mol_offset) - 1
    out = np.full(int(mol_offset[-1]), np.nan, dtype=dt)
    y = np.empty(n_struct, dtype=dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(n_struct):
            o0, o1 = int(mol_offset[s]), int(mol_offset[s + 1])
            n = o1 - o0
            zs = np.asarray(z[o0:o1])
            y[s] = pooled(config, w, zs, np.ones((1, n), dtype=bool), dt)[0]
            es = list(range(n)) if entries is None else list(entries.get(s, []))
            if not es:
                continue
            keep = np.stack([kept_set(mode, n, np.asarray(order[o0:o1]), e) for e in es])
            out[o0 + np.asarray(es)] = pooled(config, w, zs, keep, dt)
    return out, y


def check_order(order, ga, mol_offset):
    """order is a permutation of each structure's atoms, ga[order] is non-increasing, equal scores in ascending index (a NaN score -- the
    one-atom structure under use_ga_norm -- ranks last)"""
    for s in range(len(mol_offset) - 1):
        o0, o1 = int(mol_offset[s]), int(mol_offset[s + 1])
        o = np.asarray(order[o0:o1])
        assert sorted(o.tolist()) == list(range(o1 - o0)), (s, o)
        g = np.asarray(ga[o0:o1], dtype=np.float64)
        g = np.where(np.isnan(g), -np.inf, g)[o]
        assert np.all(g[:-1] >= g[1:]), (s, g)
        tie = g[:-1] == g[1:]
        assert np.all(o[:-1][tie] < o[1:][tie]), (s, o, g)


def check_ablated(got, ref64, ref32, label=""):
    """the bound: rel_err(gpu, ref64) <= max(1e-4, 2 * rel_err(ref32, ref64)) over the finite entries of ref64, and the non-finite positions
    equal to the fp32 oracle's.  Prints the figures, then asserts.  Returns (gpu error, fp32 oracle's error)."""
    got, ref64, ref32 = np.asarray(got), np.asarray(ref64), np.asarray(ref32)
    fin = np.isfinite(ref64)
    e_gpu = rel_err(got[fin], ref64[fin]) if fin.any() else 0.0
    e_32 = rel_err(ref32[fin], ref64[fin]) if fin.any() else 0.0
    print("ablated %s: gpu %.3e  fp32 oracle %.3e  bound %.3e  non-finite gpu %d / fp32 oracle %d of %d"
          % (label, e_gpu, e_32, max(1e-4, 2 * e_32), int((~np.isfinite(got)).sum()), int((~np.isfinite(ref32)).sum()), got.size))
    assert np.array_equal(~np.isfinite(got), ~np.isfinite(ref32)), (label, np.nonzero(~np.isfinite(got))[0], np.nonzero(~np.isfinite(ref32))[0])
    assert e_gpu <= max(1e-4, 2 * e_32), (label, e_gpu, e_32)
    return e_gpu, e_32
