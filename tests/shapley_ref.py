"""Reference for the Shapley values of a structure's atoms for the global pooling (scann_shapley / HipModel.atom_shapley), built on
tests/ablate_ref.py: the game's value v(S) from the after_Lc rows of one forward -- oracle.global_attention with atom_mask = 1 on S and the
two head layers -- in fp32 and fp64.  For |S| <= 1 of a structure of several atoms the oracle runs on a copy of the configuration with
use_ga_norm = False (the game's convention where the reference's arithmetic is 0 / 0); the full set keeps the model's arithmetic, so a
one-atom structure under use_ga_norm is NaN as its forward is.  On top of v: the prefix values of given walks, the exact Shapley value by
the subset formula (n <= 5), and NumPy restatements of the permutation recipe (scann_internal.h) and of the fp64 reduction.  Packed
layout: per-atom arrays [n_atom], structure s at mol_offset[s]:mol_offset[s + 1]; walks [P, n_atom], structure-local atom by position.
Also the size fixture of the GPU tests.  Test-only."""
import copy
import itertools
import math

import numpy as np

import ablate_ref
import scann_oracle as so
from ablate_ref import rel_err  # noqa: F401

SIZES = [1, 2, 3, 5, 31, 32, 33, 65]  # the 32-entry tile edge and the 64-lane edge
M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def sizes_data(sizes=SIZES, seed=17, max_neighbours=8):
    """one structure per entry of `sizes`, every atom with at most `max_neighbours` random neighbours (all others, if fewer)"""
    rng = np.random.default_rng(seed)
    de, dn = np.empty(len(sizes), dtype=object), np.empty(len(sizes), dtype=object)
    for s, n in enumerate(sizes):
        Z = rng.choice([1, 6, 7, 8], n)
        nb = []
        for a in range(n):
            others = np.array([j for j in range(n) if j != a], dtype=np.int64)
            js = np.sort(rng.choice(others, min(max_neighbours, len(others)), replace=False)) if len(others) else others
            ang, dist = rng.uniform(0.4, 3.5, len(js)), rng.uniform(0.9, 4.0, len(js))
            nb.append([[int(Z[j]), int(j), float(ang[k]), float(ang[k] / ang.max()), float(dist[k])] for k, j in enumerate(js)])
        de[s], dn[s] = [[int(z) for z in Z], float(rng.normal())], nb
    return de, dn


# ---- the game ----

def _no_norm(config):
    c = copy.deepcopy(config)
    c["model"]["use_ga_norm"] = False
    return c


def v_sets(config, w, z, keep, dt):
    """v(S) [V] of one structure for V kept sets: z [n, dg] after_Lc rows, keep [V, n] bool; w already in dt"""
    keep = np.asarray(keep, dtype=bool)
    n = keep.shape[1]
    out = np.empty(keep.shape[0], dtype=dt)
    small = (keep.sum(1) <= 1) & (n > 1)
    with np.errstate(all="ignore"):
        if small.any():
            out[small] = ablate_ref.pooled(_no_norm(config), w, z, keep[small], dt)
        if (~small).any():
            out[~small] = ablate_ref.pooled(config, w, z, keep[~small], dt)
    return out


def _weights(weights, dt):
    return {k: np.asarray(v).astype(dt) for k, v in weights.items()}


def baseline(config, weights, z, dtype):
    """v(empty): the literal empty pooling under use_ga_norm = False (rep = 0), i.e. the head on a zero representation"""
    dt = np.dtype(dtype)
    w = _weights(weights, dt)
    with np.errstate(all="ignore"):
        return ablate_ref.pooled(_no_norm(config), w, np.asarray(z)[:1], np.zeros((1, 1), dtype=bool), dt)[0]


def prefix_values(config, weights, z, mol_offset, perms, dtype):
    """(values [P, n_atom], baseline [n_struct]) in `dtype`: values[p, mol_offset[s] + j] = v of the first j + 1 atoms of walk p"""
    dt = np.dtype(dtype)
    w = _weights(weights, dt)
    perms = np.asarray(perms)
    P = perms.shape[0]
    values = np.empty(perms.shape, dtype=dt)
    base = np.empty(len(mol_offset) - 1, dtype=dt)
    for s in range(len(mol_offset) - 1):
        o0, o1 = int(mol_offset[s]), int(mol_offset[s + 1])
        n = o1 - o0
        zs = np.asarray(z[o0:o1])
        base[s] = baseline(config, weights, zs, dt)
        keep = np.zeros((P, n, n), dtype=bool)
        for p in range(P):
            pos = np.empty(n, dtype=np.int64)
            pos[perms[p, o0:o1]] = np.arange(n)
            keep[p] = pos[None, :] <= np.arange(n)[:, None]
        values[:, o0:o1] = v_sets(config, w, zs, keep.reshape(P * n, n), dt).reshape(P, n)
    return values, base


def all_subsets(config, weights, z, dtype):
    """v of every subset of one structure (n <= 5): [2^n] indexed by the bit mask of S, bit i = atom i; entry 0 = the baseline"""
    dt = np.dtype(dtype)
    n = len(z)
    assert n <= 5
    keep = np.array([[(m >> i) & 1 for i in range(n)] for m in range(1 << n)], dtype=bool)
    v = np.empty(1 << n, dtype=dt)
    v[1:] = v_sets(config, _weights(weights, dt), np.asarray(z), keep[1:], dt)
    v[0] = baseline(config, weights, z, dt)
    return v


def exact_shapley(v):
    """the subset formula on all_subsets' table, fp64: phi_i = sum over S without i of |S|! (n - |S| - 1)! / n! (v(S + i) - v(S))"""
    v = np.asarray(v, dtype=np.float64)
    n = int(round(math.log2(len(v))))
    phi = np.zeros(n)
    for i in range(n):
        for m in range(1 << n):
            if (m >> i) & 1:
                continue
            k = bin(m).count("1")
            phi[i] += math.factorial(k) * math.factorial(n - k - 1) / math.factorial(n) * (v[m | (1 << i)] - v[m])
    return phi


def all_permutations(n):
    return np.array(list(itertools.permutations(range(n))), dtype=np.int32)


def walk_values(v, perms):
    """the prefix values [P, n] of walks of one structure read from all_subsets' table"""
    perms = np.asarray(perms)
    masks = np.cumsum(1 << perms.astype(np.int64), axis=1)
    return np.asarray(v)[masks]


# ---- the permutation recipe and the reduction, restated ----

def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def permutation(seed, key, p, n):
    """scann_internal.h's shapley_permutation in Python integers"""
    base = _mix((_mix((seed + GOLD * (p + 1)) & M64) + GOLD * (key + 1)) & M64)
    out = list(range(n))
    for i in range(n - 1, 0, -1):
        u = _mix((base + GOLD * (i + 1)) & M64) >> 32
        k = (u * (i + 1)) >> 32
        out[i], out[k] = out[k], out[i]
    return np.array(out, dtype=np.int32)


def sampled_perms(seed, keys, mol_offset, P):
    """[P, n_atom]: the walks scann_shapley samples"""
    out = np.empty((P, int(mol_offset[-1])), dtype=np.int32)
    for s in range(len(mol_offset) - 1):
        o0, o1 = int(mol_offset[s]), int(mol_offset[s + 1])
        for p in range(P):
            out[p, o0:o1] = permutation(seed, int(keys[s]) if keys is not None else 0, p, o1 - o0)
    return out


def reduce(values, perms, mol_offset, base):
    """(shapley [n_atom], stderr [n_atom], full [n_struct]) in fp64 as scann_shapley defines them: marginals of fp32 (or any) values as
    doubles, sums over the walks in order, two passes"""
    values, perms = np.asarray(values), np.asarray(perms)
    P, A = values.shape
    sh, se, full = np.empty(A), np.empty(A), np.empty(len(mol_offset) - 1)
    with np.errstate(all="ignore"):
        for s in range(len(mol_offset) - 1):
            o0, o1 = int(mol_offset[s]), int(mol_offset[s + 1])
            n = o1 - o0
            if n == 0:
                full[s] = np.float64(base[s])
                continue
            v = values[:, o0:o1].astype(np.float64)
            prev = np.concatenate([np.full((P, 1), np.float64(base[s])), v[:, :-1]], axis=1)
            m_pos = v - prev  # by position
            m = np.empty((P, n))
            m[np.arange(P)[:, None], perms[:, o0:o1]] = m_pos  # by atom
            tot, f = np.zeros(n), np.float64(0)
            for p in range(P):
                tot = tot + m[p]
                f = f + v[p, n - 1]
            mean = tot / np.float64(P)
            ss = np.zeros(n)
            for p in range(P):
                d = m[p] - mean
                ss = ss + d * d
            sh[o0:o1] = mean
            se[o0:o1] = np.sqrt(ss / np.float64(P - 1) / np.float64(P))
            full[s] = f / np.float64(P)
    return sh, se, full


def check_values(got, ref64, ref32, label=""):
    """the project's bound (ablate_ref.check_ablated): rel_err(gpu, ref64) <= max(1e-4, 2 * rel_err(ref32, ref64)) over the finite entries,
    the non-finite positions equal to the fp32 oracle's"""
    return ablate_ref.check_ablated(np.asarray(got).reshape(-1), np.asarray(ref64).reshape(-1), np.asarray(ref32).reshape(-1), label)


# ---- the fixtures of the GPU tests (and of tools/shapley_parity.py) ----

CASES = {
    "sizes": dict(data="sizes"),
    "sizes_no_ga_norm": dict(data="sizes", use_ga_norm=False),
    "qm9": dict(n=8),
    "e_b": dict(n=8, target="e_b"),
    "base": dict(n=8, g_update=False),
    "generic": dict(n=8, local_dim=64, num_head=4, global_dim=96, dense_out=80),
}
P_TEST = 8  # walks per structure in every case


def config_and_inputs(kind="qm9", n=8, seed=5, L=2, target=None, data=None, **over):
    """(config, weights, padded inputs) of one case: an L = 2 model, QM9-shaped structures or the size fixture"""
    cfg = so.default_config(kind)
    cfg["model"]["n_attention"] = L
    cfg["model"].update(over)
    if target:
        cfg["hyper"]["target"] = target
    w = so.init_weights(cfg, 3, perturb=True)
    de, dn = sizes_data() if data == "sizes" else so.synth_dataset(n, seed, kind=kind)
    inputs, _ = so.pad_batch(de, dn, g_update=cfg["model"]["g_update"])
    return cfg, w, inputs
