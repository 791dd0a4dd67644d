"""GPU: a row's result does not depend on the height of its atom tile.  launch_atom (scann_kernels.hip) runs the ResidualNorm launches of a
plain inference forward -- MODE 0 of layers 1 .. L-1 and MODE 2 in front of the readout -- on 32- / 64-row tiles (atom_kernel) or on
96- / 128-row tiles (atom_wide_kernel); SCANN_ATOM_ROWS, read when the handle is made, forces a height where the launch has that
instantiation.  With an L = 2 g_update model both wide launches run in every forward.  Handles made under SCANN_ATOM_ROWS = 32, 64, 96
and 128 (no such instantiation is shipped: the automatic choice) must return the same bytes -- every structure's y, every atom's
GlobalAttention score -- on batches whose atom counts lie on both sides of every tile edge: 1, 31, 33, 95, 96, 97, 127, 129, 193 and
301 atoms.  The batches are small synthetic molecules behind a one-atom structure and a molecule with an isolated atom.  The automatic
choice is compared with 32 rows on launches of 25 k, 33 k and 50 k atoms: on a 256-CU device 64, 96 and again 64 rows."""
import functools
import os

import numpy as np
import pytest

import scann_oracle as so
from test_gpu_mc_sizes import same_bits

pytestmark = pytest.mark.gpu

L = 2
ATOMS = [1, 31, 33, 95, 96, 97, 127, 129, 193, 301]
HEIGHTS = ("0", "32", "64", "96", "128")  # 0: automatic


def molecule(rng, n_atoms, isolated=()):
    """one structure as a PackedBatch: every atom 1 to 6 neighbours among the others, those of `isolated` (and a lone atom) none"""
    from scann import _hip

    deg = [0 if a in isolated or n_atoms == 1 else int(rng.integers(1, min(6, n_atoms - 1) + 1)) for a in range(n_atoms)]
    col = [rng.choice(np.delete(np.arange(n_atoms), a), d, replace=False) for a, d in enumerate(deg)]
    n_edge = int(sum(deg))
    return _hip.PackedBatch(rng.choice([1, 6, 7, 8, 9], n_atoms), [0, n_atoms], np.concatenate([[0], np.cumsum(deg)]),
                            np.concatenate(col).astype(np.int64) if n_edge else np.zeros(0, np.int64),
                            rng.uniform(0.9, 4.0, n_edge), rng.uniform(0.4, 3.5, n_edge))


@functools.lru_cache(maxsize=None)
def batch_of(total):
    """a batch of `total` atoms: a one-atom structure, a molecule one of whose atoms is isolated, then molecules of up to 19 atoms"""
    from scann import _hip

    rng = np.random.default_rng(total)
    parts, left = [molecule(rng, 1)], total - 1
    first = True
    while left > 0:
        n = min(left, int(rng.integers(9, 20)))
        if left - n == 1:  # (no second one-atom structure by accident)
            n += 1
        parts.append(molecule(rng, n, isolated=(n // 2,) if first and n > 2 else ()))
        first = False
        left -= n
    pk = _hip.concat_packed(parts)
    assert pk.n_atom == total and pk.n_struct == len(parts)
    if total > 2:
        assert (np.diff(pk.edge_offset)[1:] == 0).any() and int(pk.mol_offset[1]) == 1
    return pk


@pytest.fixture(scope="module")
def models(hip_lib):
    """{height: handle made under SCANN_ATOM_ROWS = height} of one L = 2 g_update model"""
    from scann.models.scann_model import HipModel

    cfg = so.default_config("qm9")
    cfg["model"].update(n_attention=L, g_update=True)
    w = so.init_weights(cfg, 3, perturb=True)
    out, old = {}, os.environ.get("SCANN_ATOM_ROWS")
    try:
        for rows in HEIGHTS:
            os.environ["SCANN_ATOM_ROWS"] = rows
            out[rows] = HipModel(cfg, w, device=0, infer=True)
    finally:
        if old is None:
            os.environ.pop("SCANN_ATOM_ROWS", None)
        else:
            os.environ["SCANN_ATOM_ROWS"] = old
    return out


def forward(model, pk, outputs=False):
    from scann import _hip

    eng = model.engine
    rb = eng.upload(pk)
    try:
        if outputs:
            eng.set_outputs((), after_lc=True)
        eng.forward_resident(rb, 0)
        y, ga = eng.download(rb)
        z = eng.read_output(rb, _hip.OUT_AFTER_LC) if outputs else None
    finally:
        if outputs:
            eng.set_outputs()
        rb.free()
    assert y.shape == (pk.n_struct,) and ga.shape == (pk.n_atom,)
    # (the reference graph itself gives a one-atom structure NaN -- oracle/scann_oracle.py does too; its bytes are compared like any others)
    many = np.diff(pk.mol_offset) > 1
    assert np.isfinite(y[many]).all() and np.isfinite(ga[np.repeat(many, np.diff(pk.mol_offset))]).all()
    return y, ga, z


@pytest.mark.parametrize("total", ATOMS)
def test_tile_height_does_not_change_a_row(models, total):
    """y of every structure and the GlobalAttention score of every atom: the bytes of the 32-row handle on the 96- and 128-row ones"""
    pk = batch_of(total)
    y32, ga32, _ = forward(models["32"], pk)
    for rows in ("64", "96", "128", "0"):
        y, ga, _ = forward(models[rows], pk)
        same_bits("%d atoms, %s rows: y" % (total, rows), y, y32, pk, "structure")
        same_bits("%d atoms, %s rows: ga" % (total, rows), ga, ga32, pk, "atom")


@pytest.mark.parametrize("total", [25000, 33000, 50000])
def test_automatic_height_of_large_launches_does_not_change_a_row(models, total):
    """the first structures of one 50,000-atom batch that hold at least `total` atoms: beyond three 32-row tiles per CU the automatic choice
    leaves 32 rows (scann_kernels.hip atom_tile_rows) -- the forced-32 handle's bytes"""
    from scann import _hip

    big = batch_of(50000)
    n = int(np.searchsorted(big.mol_offset, total))
    pk = _hip.slice_packed(big, 0, n)
    assert total <= pk.n_atom < total + 20
    y32, ga32, _ = forward(models["32"], pk)
    y, ga, _ = forward(models["0"], pk)
    same_bits("%d atoms, automatic: y" % pk.n_atom, y, y32, pk, "structure")
    same_bits("%d atoms, automatic: ga" % pk.n_atom, ga, ga32, pk, "atom")


def test_a_launch_without_a_wide_instantiation_falls_back(models):
    """after_Lc selected: the readout's launch stores z (atom_kernel's ZOUT instantiation, which has no wide form) and runs at the
    automatic height under a forced 96, beside a 96-row layer launch: y, the scores and after_Lc are the 32-row handle's bytes, and
    y / the scores those of the forward without the output"""
    pk = batch_of(193)
    y32, ga32, z32 = forward(models["32"], pk, outputs=True)
    y, ga, z = forward(models["96"], pk, outputs=True)
    assert z.shape == (pk.n_atom, 128) and np.abs(z).max() > 0
    same_bits("after_Lc selected under 96 rows: y", y, y32, pk, "structure")
    same_bits("after_Lc selected under 96 rows: ga", ga, ga32, pk, "atom")
    same_bits("after_Lc selected under 96 rows: after_Lc", z, z32)
    y0, ga0, _ = forward(models["96"], pk)
    same_bits("with and without after_Lc: y", y, y0, pk, "structure")
    same_bits("with and without after_Lc: ga", ga, ga0, pk, "atom")
