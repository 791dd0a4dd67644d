"""GPU: the selected inference outputs -- every LocalAttention layer's attention weights, after_Lc, bf_property -- on the far side of
the launch code's switches: 64-row edge tiles without chunk tiles (by degree and by edge count, the first layer fed from the per-species
tables), 64-row atom tiles, the general embedding (use_ring / feature cgcnn), the exact-fp32 instantiations on 64-row and chunk tiles,
the plain-fp32 kernels above 64 neighbours and on a large batch, SCANN_SPECIES_TABLES=0.  tests/test_gpu_outputs.py runs the 32-row side.

Every oracle comparison is test_gpu_outputs.check_against_oracle(fp64_bound=True) on the padded-array call: rel_err(gpu, fp64) <=
max(RTOL, 2 rel_err(fp32 oracle, fp64)), masked slots exactly 0, rows without a neighbour exactly 1 / N, row sums within 1e-6 of 1.
The oracle's own fp32 error against fp64 on deg40, qm9_b260 and sparse_atoms is 1.5e-7 to 3.8e-6 over the four outputs, so the bound is
RTOL = 1e-4 throughout.  Each test uploads its PackedBatch once, asserts from batch_info that the batch is on the side it is meant to be,
runs the forward on that resident batch, and requires the padded-array call (one launch sequence) to return the same bytes.  The
batches are those of tests/size_batches.py (tests/test_sizes_host.py pins their plans without a GPU); the oracle's intermediates are
computed once per (batch, config).  The measured errors and bounds are collected in PARITY_LINES (tools/outputs_parity.py writes them
to profiles/outputs_parity.txt)."""
import numpy as np
import pytest

import rollout_ref
import scann_oracle as so
import size_batches as sb
from test_gpu_mc_sizes import BRANCH, W64, expect_rows, same_bits
from test_gpu_outputs import RTOL, all_names, check_against_oracle, oracle_outputs, rel_err

pytestmark = pytest.mark.gpu

L = 2
PARITY_LINES = []  # "case  output  rel_err  bound" of every oracle comparison this module has run


@pytest.fixture(scope="module")
def cache():
    """key -> value, computed on first use for the whole module"""
    store = {}

    def get(key, make):
        if key not in store:
            store[key] = make()
        return store[key]

    return get


def out_config(g_update=True, widths=None, **over):
    cfg = so.default_config("qm9")
    cfg["model"].update(n_attention=L, g_update=g_update, **over)
    if widths:
        cfg["model"].update(widths)
        cfg["model"]["n_atoms"] = 100
    return cfg, so.init_weights(cfg, 3, perturb=True)


def new_model(cfg, w, monkeypatch=None, **env):
    """a handle made with `env` set around its constructor (the switches are read when the handle is made)"""
    from scann.models.scann_model import HipModel

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model = HipModel(cfg, w, device=0, infer=True)
    for k in env:
        monkeypatch.delenv(k)
    return model


def batch(cache, name, g_update=True):
    """(padded inputs, PackedBatch) of the size batch `name`"""
    def make():
        inputs, _ = sb.padded(getattr(sb, name + "_data")(), g_update, use_ring=name == "qm9_ring_b260")
        return inputs, getattr(sb, name)(g_update)[0]

    return cache(("batch", name, g_update), make)


def refs_of(cache, key, cfg, w, inputs):
    """(fp32, fp64) oracle outputs of (batch, config) `key`, once for the module; check_against_oracle leaves them as they are after
    its first call (it writes the fp32 graph's 1 / N convention into the fp64 maps' rows without a neighbour)"""
    return cache(("oracle",) + key, lambda: (oracle_outputs(cfg, w, inputs), oracle_outputs(cfg, w, inputs, np.float64)))


def run_outputs(model, pk, expect):
    """{name: packed output} plus "y" and "ga" of one forward of `pk` with every output selected, on the batch uploaded once, after
    `expect(info)` has asserted which side of the switches it is on"""
    from scann import _hip

    eng = model.engine
    rb = eng.upload(pk)
    try:
        expect(eng.batch_info(rb))
        eng.set_outputs(range(L), after_lc=True, bf_property=True)
        eng.forward_resident(rb, 0)
        y, ga = eng.download(rb)
        out = {"local_attention_%d" % k: eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, k) for k in range(L)}
        out["after_Lc"] = eng.read_output(rb, _hip.OUT_AFTER_LC)
        out["bf_property"] = eng.read_output(rb, _hip.OUT_BF_PROPERTY)
        out["y"], out["ga"] = y, ga
    finally:
        eng.set_outputs()
        rb.free()
    cfg = model.config["model"]
    assert out["local_attention_0"].shape == (pk.n_edge, cfg["num_head"]) and out["after_Lc"].shape == (pk.n_atom, cfg["global_dim"])
    assert out["bf_property"].shape == (pk.n_struct, cfg["dense_out"])
    return out


def padded_outputs(model, inputs, names, packed, monkeypatch):
    """predict(padded arrays, outputs=names) as ONE launch sequence (no pipeline of chunks, which would cut the batch back to the
    small side): the packed outputs of the resident run, byte for byte, at the real slots"""
    from scann import _hip
    from scann.models.scann_model import HipModel

    monkeypatch.setattr(HipModel, "BIG_PREDICT", 1 << 30)
    nb = np.shape(inputs["neighbors"])
    assert nb[0] * nb[1] * max(1, nb[2]) <= HipModel.BIG_SLOTS
    got = model.predict(inputs, outputs=names)
    for n, g in zip(names, got):
        if n.startswith("local_attention_"):
            want = _hip.repad_local_attention(packed[n], inputs["atom_mask"], inputs["neighbor_mask"])
        elif n == "after_Lc":
            want = _hip.repad_atoms(packed[n], inputs["atom_mask"])
        else:
            want = packed[n]
        same_bits("padded call against the resident batch: " + n, g, want)
    return got


def check_oracle(label, cfg, w, inputs, got, refs):
    """check_against_oracle under the fp64 bound; the figures go to PARITY_LINES before anything is asserted"""
    names, measured = all_names(cfg), []
    try:
        check_against_oracle(cfg, w, inputs, got, names, fp64_bound=True, refs=refs, measured=measured)
    finally:
        for n, e, bound in measured:
            line = "%-40s %-18s %-12.3e %.3e" % (label, n, e, bound)
            print(line)
            PARITY_LINES.append(line)
    assert [m[0] for m in measured] == names


def against_oracle(label, cache, key, cfg, w, model, inputs, pk, expect, monkeypatch):
    """the whole rule of this module for one handle and batch; returns the packed outputs"""
    packed = run_outputs(model, pk, expect)
    names = all_names(cfg)
    got = padded_outputs(model, inputs, names, packed, monkeypatch)
    check_oracle(label, cfg, w, inputs, got, refs_of(cache, key, cfg, w, inputs))
    return packed


def agree(label, a, b, names, tol):
    """two implementations of one graph: every output of `a` within `tol` of `b`'s (rel_err), and not the same arithmetic"""
    for n in names:
        e = rel_err(a[n], b[n])
        print("%s %s: %.3e" % (label, n, e))
        assert e <= tol, (label, n, e)
    assert any(not np.array_equal(a[n], b[n]) for n in names), label


# ---- 1., 2. 64-row edge tiles without chunk tiles, the first layer fed from the per-species tables ----

@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
def test_64_row_edge_tiles_by_degree_match_the_oracle(hip_lib, monkeypatch, cache, g_update):
    """deg40 (a 40- and a 33-neighbour atom, one isolated atom, no chunk tiles).  g_update: edge_kernel<true, 2, .., ATTN> piece-major
    with fuse_basis and species0 (no atom launch before layer 0); base: the row-major edge_kernel<false, 2, .., ATTN>"""
    inputs, pk = batch(cache, "deg40", g_update)
    deg = np.diff(pk.edge_offset)
    assert pk.n_edge <= sb.EDGE_TILE_32_MAX_EDGES and sb.EDGE_TILE_32_MAX_DEGREE < int(deg.max()) <= 64 and (deg == 0).any()
    cfg, w = out_config(g_update)
    against_oracle("deg40 " + BRANCH[g_update], cache, ("deg40", g_update), cfg, w, new_model(cfg, w), inputs, pk, expect_rows(64),
                   monkeypatch)


@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
def test_64_row_edge_tiles_by_edge_count_match_the_oracle(hip_lib, monkeypatch, cache, g_update):
    """qm9_b260 (4,779 atoms, 35,837 edges, degrees up to 12): the same instantiations as by degree, on 560 full tiles of many atoms
    each, with 32-row atom tiles in front of them"""
    inputs, pk = batch(cache, "qm9_b260", g_update)
    assert pk.n_edge > sb.EDGE_TILE_32_MAX_EDGES and int(np.diff(pk.edge_offset).max()) <= sb.EDGE_TILE_32_MAX_DEGREE
    cfg, w = out_config(g_update)
    against_oracle("qm9_b260 " + BRANCH[g_update], cache, ("qm9_b260", g_update), cfg, w, new_model(cfg, w), inputs, pk, expect_rows(64),
                   monkeypatch)


# ---- 3. 64-row atom tiles ----

def test_64_row_atom_tiles_match_the_oracle(hip_lib, monkeypatch, cache):
    """sparse_atoms (34,231 atoms, 8,577 of them isolated, padded N = 3): atom_kernel<.., 2, ..> in mode 2 writes after_Lc through
    AtomArgs::out_z, the last of its 535 tiles holding 55 rows; the isolated atoms' attention rows are 1 / 3"""
    inputs, pk = batch(cache, "sparse_atoms")
    assert inputs["neighbors"].shape[2] == 3 and int((np.diff(pk.edge_offset) == 0).sum()) == 8577
    cfg, w = out_config()
    model = new_model(cfg, w)
    packed = against_oracle("sparse_atoms g_update", cache, ("sparse_atoms", True), cfg, w, model, inputs, pk,
                            expect_rows(64, atoms_above=sb.ATOM_TILE_32_MAX), monkeypatch)
    # the packed call: n_atom rows, the partial last tile's among them
    z = model.predict(pk, outputs=["after_Lc"])[0]
    tail = pk.n_atom % 64
    assert z.shape == (pk.n_atom, cfg["model"]["global_dim"]) and 0 < tail < 64
    z_pad = model.predict(inputs, outputs=["after_Lc"])[0]  # (BIG_PREDICT is still lifted: one launch sequence)
    amask = inputs["atom_mask"][..., 0] != 0
    same_bits("after_Lc, the last %d rows" % tail, z[-tail:], z_pad[amask][-tail:])
    same_bits("after_Lc, packed call", z, packed["after_Lc"])
    assert np.abs(z[-tail:]).max() > 0


# ---- 4. the general embedding ----

GENERAL = {"ring": dict(n=8, use_ring=True), "cgcnn": dict(n=10, feature="cgcnn"), "ring+cgcnn": dict(n=12, use_ring=True, feature="cgcnn")}


@pytest.mark.parametrize("case", list(GENERAL))
def test_general_embedding_matches_the_oracle(hip_lib, monkeypatch, cache, case):
    """use_ring / feature cgcnn: general_embed -- embed_kernel writes c0, no per-species tables, an atom launch in front of layer 0's
    edge_kernel<true, 1, .., ATTN> (fused basis); 32-row tiles"""
    import test_gpu_input_grads as ig

    cfg, w, inputs, pk, model = ig.setup(L=L, **GENERAL[case])
    assert (pk.ring is not None) == ("ring" in case) and (pk.cgcnn is not None) == ("cgcnn" in case)
    against_oracle("general " + case, cache, ("general", case), cfg, w, model, inputs, pk, expect_rows(32), monkeypatch)


def test_general_embedding_on_64_row_edge_tiles_matches_the_oracle(hip_lib, monkeypatch, cache):
    """qm9_ring_b260 (260 ring molecules, 35,569 edges): general_embed in front of edge_kernel<true, 2, .., ATTN> with the fused basis
    and no species tables"""
    inputs, pk = batch(cache, "qm9_ring_b260")
    assert pk.ring is not None and pk.n_edge > sb.EDGE_TILE_32_MAX_EDGES
    cfg, w = out_config(use_ring=True)
    against_oracle("qm9_ring_b260 g_update", cache, ("qm9_ring_b260", True), cfg, w, new_model(cfg, w), inputs, pk, expect_rows(64),
                   monkeypatch)


# ---- 5. exact fp32 ----

@pytest.mark.parametrize("name", ["chunked", "deg40"])
def test_exact_fp32_kernels_match_the_oracle_and_the_split_fp16_ones(hip_lib, monkeypatch, cache, name):
    """SCANN_EXACT=1: basis_kernel and the row-major EX instantiations edge_kernel<true, 2, .., ATTN, EX> / atom_kernel<.., EX> -- on
    chunked with six atoms' chunk tiles finished by attn_merge_kernel, on deg40 without.  Two implementations of one graph: every
    output also within 2 RTOL of the split-fp16 handle's"""
    inputs, pk = batch(cache, name)
    expect = expect_rows(64, big_atoms=6 if name == "chunked" else 0)
    cfg, w = out_config()
    exact = new_model(cfg, w, monkeypatch, SCANN_EXACT="1")
    got = against_oracle("%s g_update exact" % name, cache, (name, True), cfg, w, exact, inputs, pk, expect, monkeypatch)
    assert exact.engine.exact_reruns() == 0  # (exact from the start, not a re-run)
    fast = against_oracle("%s g_update split-fp16" % name, cache, (name, True), cfg, w, new_model(cfg, w), inputs, pk, expect, monkeypatch)
    agree("%s exact against split-fp16" % name, got, fast, all_names(cfg), 2 * RTOL)


# ---- 6. plain fp32 ----

@pytest.mark.parametrize("name", ["chunked", "qm9_b260"])
def test_plain_fp32_kernels_match_the_oracle(hip_lib, monkeypatch, cache, name):
    """run_forward_generic: SCANN_GENERIC=1 at 128 / 8 and the 64 / 4 / 96 / 32 widths -- gen_attn_kernel at max_degree 219 (chunked)
    and over 35,837 edges (qm9_b260).  At 128 / 8 every output is also within 2 RTOL of the MFMA handle's"""
    inputs, pk = batch(cache, name)
    expect = expect_rows(64, big_atoms=6 if name == "chunked" else 0)
    cfg, w = out_config()
    plain = new_model(cfg, w, monkeypatch, SCANN_GENERIC="1")
    got = against_oracle("%s g_update plain" % name, cache, (name, True), cfg, w, plain, inputs, pk, expect, monkeypatch)
    fast = run_outputs(new_model(cfg, w), pk, expect)
    agree("%s plain against mfma" % name, got, fast, all_names(cfg), 2 * RTOL)
    cfg4, w4 = out_config(widths=W64)
    got4 = against_oracle("%s g_update 64x4" % name, cache, (name, True, "64x4"), cfg4, w4, new_model(cfg4, w4), inputs, pk, expect,
                          monkeypatch)
    assert got4["local_attention_1"].shape[1] == 4 and got4["after_Lc"].shape[1] == 96 and got4["bf_property"].shape[1] == 32


# ---- 7. species tables off ----

def test_outputs_without_the_species_tables_are_the_same_bytes(hip_lib, monkeypatch, cache):
    """SCANN_SPECIES_TABLES=0 (fused basis, an atom launch in front of layer 0) against the default handle (species0), on qm9_b260
    (64-row tiles) and on 16 of its molecules (32-row): every output the same bytes -- the promise of
    test_first_layer_computes_its_geometry_rows_itself for y and the GA scores, extended to the outputs -- and y / GA with outputs
    requested the bytes of a plain predict"""
    from scann import _hip

    _, pk = batch(cache, "qm9_b260")
    cfg, w = out_config()
    tables, launch = new_model(cfg, w), new_model(cfg, w, monkeypatch, SCANN_SPECIES_TABLES="0")
    # (slices carry no padding information: predict returns the packed GA scores for them)
    for label, p, expect in (("qm9_b260", _hip.slice_packed(pk, 0, pk.n_struct), expect_rows(64)),
                             ("16 molecules", _hip.slice_packed(pk, 0, 16), expect_rows(32))):
        a, b = run_outputs(tables, p, expect), run_outputs(launch, p, expect)
        for n in all_names(cfg) + ["y", "ga"]:
            same_bits("%s, tables off: %s" % (label, n), b[n], a[n])
        for model, got in ((tables, a), (launch, b)):
            y, ga = model.predict(p)
            same_bits(label + ": y with outputs requested", got["y"], y[:, 0])
            same_bits(label + ": ga with outputs requested", got["ga"], np.ravel(ga))


# ---- 8. a structure does not depend on its batch ----

@pytest.mark.parametrize("g_update", [True, False], ids=["g_update", "base"])
@pytest.mark.parametrize("name", ["deg40", "chunked"])
def test_a_structure_gets_the_same_outputs_beside_one_that_forces_64_row_tiles(hip_lib, cache, name, g_update):
    """deg40 / chunked: the flanking molecules alone run on 32-row edge tiles and must give the bytes they get in the mixed batch (64
    rows); the large structure alone stays on 64 rows (and its chunk tiles) and must give the bytes it gets behind other structures.
    DESIGN.md, "Tile height follows the launch": "Per row the arithmetic is the same instruction sequence in both, so results do not
    depend on the choice"; "Determinism": "A row's result must not depend on where in a tile (or batch) it lands"."""
    from scann import _hip

    _, pk = batch(cache, name, g_update)
    n_big = 6 if name == "chunked" else 0
    cfg, w = out_config(g_update)
    model = new_model(cfg, w)
    whole = run_outputs(model, pk, expect_rows(64, big_atoms=n_big))
    mid = pk.n_struct // 2
    for lo, hi, expect in ((0, mid, expect_rows(32)), (mid, mid + 1, expect_rows(64, big_atoms=n_big)), (mid + 1, pk.n_struct, expect_rows(32))):
        got = run_outputs(model, _hip.slice_packed(pk, lo, hi), expect)
        a0, a1 = int(pk.mol_offset[lo]), int(pk.mol_offset[hi])
        e0, e1 = int(pk.edge_offset[a0]), int(pk.edge_offset[a1])
        label = "%s %s structures [%d, %d) " % (name, BRANCH[g_update], lo, hi)
        for k in range(L):
            same_bits(label + "local_attention_%d" % k, got["local_attention_%d" % k], whole["local_attention_%d" % k][e0:e1])
        same_bits(label + "after_Lc", got["after_Lc"], whole["after_Lc"][a0:a1])
        same_bits(label + "bf_property", got["bf_property"], whole["bf_property"][lo:hi])
        same_bits(label + "y", got["y"], whole["y"][lo:hi], pk, "structure", lo)
        same_bits(label + "ga", got["ga"], whole["ga"][a0:a1], pk, "atom", a0)


# ---- 9. consumers ----

def test_rollout_reads_the_maps_of_64_row_edge_tiles(hip_lib, cache):
    """attention_rollout on deg40: the rollout kernels compose the maps edge_kernel<true, 2, .., ATTN> left in the batch's output block
    -- against tests/rollout_ref.py in fp64 on the GPU's own maps, under test_gpu_rollout.check_kernel's derived bound"""
    import test_gpu_rollout as tr

    inputs, pk = batch(cache, "deg40")
    cfg, w = out_config()
    model = new_model(cfg, w)
    rb = model.engine.upload(pk)
    expect_rows(64)(model.engine.batch_info(rb))
    rb.free()
    got = model.attention_rollout(inputs)
    check = tr.check_kernel(got, cfg, inputs, tr.gpu_maps(model, cfg, inputs), "deg40 rollout")
    amask, em = rollout_ref.masks(inputs)
    assert int(em.sum(-1).max()) == 40 and check[0] <= check[1]


def test_atom_index_holds_the_after_lc_rows_of_64_row_atom_tiles(hip_lib, cache):
    """build_index(level="atom") over sparse_atoms as one batch: the index keeps the rows atom_kernel<.., 2, ..> wrote through out_z,
    the bytes predict(outputs=["after_Lc"]) returns for the same batch"""
    _, pk = batch(cache, "sparse_atoms")
    cfg, w = out_config()
    model = new_model(cfg, w)
    rb = model.engine.upload(pk)
    expect_rows(64, atoms_above=sb.ATOM_TILE_32_MAX)(model.engine.batch_info(rb))
    rb.free()
    ix = model.build_index(pk, level="atom", batch_size=pk.n_struct)
    rows, ids, atoms = ix.rows()
    z = model.predict(pk, outputs=["after_Lc"])[0]
    assert rows.shape == (pk.n_atom, cfg["model"]["global_dim"])
    same_bits("the index's rows against after_Lc", rows, z)
    cnt = np.diff(pk.mol_offset)
    assert np.array_equal(ids, np.repeat(np.arange(pk.n_struct), cnt)) and np.array_equal(atoms, np.concatenate([np.arange(c) for c in cnt]))
