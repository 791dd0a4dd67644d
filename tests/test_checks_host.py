"""The shared checks of tests/analysis_checks.py and tests/abi_checks.py have teeth: driven with a small fake engine and model (plain
Python objects that hold NumPy arrays), the honest fake passes, and every variant that breaks exactly one invariant makes the helper
raise AssertionError.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import abi_checks
import scann_oracle as so
from analysis_checks import padded, same_arrays, steady_memory, training_twin, untouched

MiB = 1 << 20


class _Batch:
    def __init__(self, packed):
        self.packed, self.y, self.ga, self.block, self.freed = packed, None, None, {}, False

    def free(self):
        self.freed = True


class _Index:
    def __init__(self, dim):
        self.rows, self.freed = np.zeros((0, dim), np.float32), False

    def __len__(self):
        return len(self.rows)

    def free(self):
        self.freed = True


class FakeEngine:
    """an engine whose forward is a few NumPy lines on its weights; ``analysis`` is the call under test, and ``fault`` names the one
    thing it (or a training step after it) does that it should not"""

    def __init__(self, w, fault=None):
        self.w = {k: np.array(v, np.float32) for k, v in w.items()}
        self.fault, self.sel, self.free_bytes, self.grads, self.adam, self.loss_bias = fault, set(), 1000 * MiB, None, np.float32(0), 0.0

    # -- inference --
    def get_weights(self):
        return {k: v.copy() for k, v in self.w.items()}

    def set_outputs(self, attn_layers=(), after_lc=False, bf_property=False):
        from scann import _hip

        self.sel = {(_hip.OUT_LOCAL_ATTENTION, int(k)) for k in attn_layers} | ({(_hip.OUT_AFTER_LC, 0)} if after_lc else set()) | \
            ({(_hip.OUT_BF_PROPERTY, 0)} if bf_property else set())

    def upload(self, packed):
        return _Batch(packed)

    def _values(self, p):
        from scann import _hip

        a = np.arange(p.n_atom, dtype=np.float32)[:, None]
        return {(_hip.OUT_LOCAL_ATTENTION, 1): np.tile(self.w["a"][:8], (p.n_edge, 1)), (_hip.OUT_AFTER_LC, 0): a * self.w["a"][None, :] + self.w["b"][0],
                (_hip.OUT_BF_PROPERTY, 0): np.tile(self.w["b"], (p.n_struct, 1))}

    def forward_resident(self, rb, also=()):
        from scann import _hip

        p = rb.packed
        v = self._values(p)
        rb.y = np.arange(p.n_struct, dtype=np.float32) * self.w["a"][0] + self.w["b"][1]
        rb.ga = v[(_hip.OUT_AFTER_LC, 0)][:, 0].copy()
        rb.block = {k: v[k] for k in self.sel | set(also)}

    def download(self, rb):
        return rb.y.copy(), rb.ga.copy()

    def read_output(self, rb, what, layer=0):
        from scann import _hip

        if (what, layer) not in rb.block:
            raise _hip.ScannHipError(-1, "output not selected")
        return rb.block[(what, layer)].copy()

    def index_create(self, dim):
        return _Index(dim)

    def index_add_batch(self, ix, rb, level):
        self.forward_resident(rb, also=[(level, 0)])  # the call's own forward: the handle's selection and the level
        ix.rows = np.concatenate([ix.rows, rb.block[(level, 0)]])

    def index_read(self, ix):
        return ix.rows.copy(), np.arange(len(ix), dtype=np.int64), np.full(len(ix), -1, np.int32)

    def index_query(self, ix, q, k):
        d = ((q[:, None, :].astype(np.float64) - ix.rows[None, :, :]) ** 2).sum(-1).astype(np.float32)
        pos = np.argsort(d, axis=1, kind="stable")[:, :k].astype(np.int32)
        return {"dist2": np.take_along_axis(d, pos, axis=1), "position": pos}

    def device_memory(self):
        return self.free_bytes, 2000 * MiB

    # -- the call under test --
    def analysis(self, rb=None, pool=None):
        from scann import _hip

        f = self.fault
        if f == "weight":
            self.w["a"].view(np.uint32)[3] ^= 1
        elif f == "row":
            pool.rows.view(np.uint8)[5] ^= 1
        elif f == "y":
            rb.y[0] += 1
        elif f == "selected":
            rb.block[(_hip.OUT_AFTER_LC, 0)][1, 1] += 1
        elif f == "unselected":
            rb.block[(_hip.OUT_BF_PROPERTY, 0)] = np.zeros((rb.packed.n_struct, 128), np.float32)
        elif f == "leak":
            self.free_bytes -= 5 * MiB
        elif f == "grad":
            self.grads["a"].view(np.uint32)[0] ^= 1
        elif f == "step":
            self.loss_bias = 1.0
        elif f == "adam":
            self.adam = np.float32(1)
        return {"value": np.float32([1, 2, 3])}

    # -- training --
    def train_begin(self):
        self.grads = {k: np.zeros_like(v) for k, v in self.w.items()}

    def train_step(self, rb, targets, lr, dropout=0.0, seed=0):
        loss = float(self.w["a"][0]) + seed + self.loss_bias
        for k in self.w:
            self.grads[k] = np.float32(seed) * np.sign(self.w[k]) + np.float32(targets.sum())
            self.w[k] = self.w[k] - np.float32(lr) * (self.grads[k] + self.adam)
        return loss

    def get_grads(self):
        return {k: v.copy() for k, v in self.grads.items()}


class FakeModel:
    fault = None

    def __init__(self, cfg, w, device=0, infer=False, deterministic=False):
        self.engine = FakeEngine(w, None if infer else type(self).fault)

    def predict(self, data, outputs=None):
        from scann import _hip

        eng = self.engine
        rb = eng.upload(_hip.pack_inputs(data))
        keys = {"local_attention_1": (_hip.OUT_LOCAL_ATTENTION, 1), "after_Lc": (_hip.OUT_AFTER_LC, 0)}
        v = eng._values(rb.packed)
        if outputs is not None:
            return [v[keys[n]] for n in outputs]
        eng.forward_resident(rb)
        return eng.download(rb)


def faulty(fault):
    return type("Faulty", (FakeModel,), {"fault": fault})


@pytest.fixture(scope="module")
def case():
    cfg = so.default_config("qm9")
    rng = np.random.default_rng(0)
    w = {"a": rng.standard_normal(128).astype(np.float32), "b": rng.standard_normal(128).astype(np.float32)}
    return cfg, w, padded("qm9", 3, 0, cfg)


def run_untouched(model, data, times=3):
    with untouched(model, data) as u:
        first = u.eng.analysis(u.rb, u.pool)
        u.repeat(lambda: u.eng.analysis(u.rb, u.pool), lambda r: same_arrays(r, first, "repeat"), times, 16 * MiB)


# ---- untouched ----

def test_untouched_passes_on_the_honest_engine(case):
    cfg, w, data = case
    model = FakeModel(cfg, w)
    run_untouched(model, data)
    assert model.engine.sel == set()


@pytest.mark.parametrize("fault", ["weight", "row", "y", "selected", "unselected", "leak"])
def test_untouched_catches_one_broken_invariant(case, fault):
    cfg, w, data = case
    model = faulty(fault)(cfg, w)
    with pytest.raises(AssertionError):
        run_untouched(model, data, times=4)  # (the leak: 4 x 5 MiB pass the 16 MiB slack)
    assert model.engine.sel == set()  # the selection is taken back on this way out as well


def test_untouched_takes_the_selection_back_when_the_body_raises(case):
    cfg, w, data = case
    model = FakeModel(cfg, w)
    with pytest.raises(RuntimeError, match="the body"):
        with untouched(model, data) as u:
            assert u.eng.sel  # something is selected in here
            raise RuntimeError("the body")
    assert model.engine.sel == set()


def test_check_inside_the_body_sees_what_a_later_forward_would_hide(case):
    cfg, w, data = case
    model = faulty("selected")(cfg, w)
    with untouched(model, data) as u:
        u.eng.analysis(u.rb, u.pool)
        with pytest.raises(AssertionError):
            u.check()
        u.reforward()  # the block is the forward's again: the exit alone would not have seen it


# ---- steady_memory ----

def test_steady_memory(case):
    cfg, w, data = case
    eng = FakeEngine(w)
    seen = []
    assert steady_memory(eng, seen.append, 5, 16 * MiB) == 1000 * MiB and seen == [0, 1, 2, 3, 4]
    eng.fault = "leak"
    steady_memory(eng, lambda rep: eng.analysis(), 3, 16 * MiB)  # 15 MiB
    with pytest.raises(AssertionError):
        steady_memory(eng, lambda rep: eng.analysis(), 4, 16 * MiB)  # 20 MiB


# ---- training_twin ----

def twin_calls(seen):
    def calls(train_model, rb, inference):
        train_model.engine.analysis(rb)
        inf_model, rb2 = inference()
        assert inference() == (inf_model, rb2)  # built once
        same_arrays(inf_model.engine.get_weights(), train_model.engine.get_weights(), "the inference handle has the current weights")
        seen.append((train_model, rb2))
    return calls


def test_training_twin_passes_on_the_honest_engine(case):
    from scann import _hip

    cfg, w, data = case
    seen = []
    training_twin(cfg, w, _hip.pack_inputs(data), twin_calls(seen), model_class=FakeModel)
    assert len(seen) == 1 and seen[0][1].freed  # the calls ran on one handle only; the inference batch was freed
    assert not np.array_equal(seen[0][0].engine.w["a"], w["a"])  # (the steps did move the weights)


@pytest.mark.parametrize("fault", ["grad", "weight", "step", "adam"])
def test_training_twin_catches_one_broken_invariant(case, fault):
    from scann import _hip

    cfg, w, data = case
    with pytest.raises(AssertionError):
        training_twin(cfg, w, _hip.pack_inputs(data), twin_calls([]), model_class=faulty(fault))


# ---- same_arrays ----

def test_same_arrays():
    a = {"x": np.float32([1, 2]), "n": np.int32([3])}
    same_arrays(a, {k: v.copy() for k, v in a.items()})
    for other in ({"x": np.float32([1, 2])}, {"x": np.float64([1, 2]), "n": np.int32([3])}, {"x": np.float32([[1, 2]]), "n": np.int32([3])},
                  {"x": np.float32([1, -2]), "n": np.int32([3])}, {"x": np.float32([1, 2]), "n": np.int32([3]), "more": np.zeros(1)}):
        with pytest.raises(AssertionError):
            same_arrays(a, other)
    same_arrays({"x": np.float32([np.nan])}, {"x": np.float32([np.nan])})  # bytes, not values
    with pytest.raises(AssertionError):
        same_arrays({"x": np.float32([0.0])}, {"x": np.float32([-0.0])})


# ---- abi_checks ----

def test_declared_and_signatures(hip_lib):
    P = C.c_void_p
    abi_checks.declared("int scann_index_create(scann_handle_t* h, int32_t dim, scann_index_t** out);", "#define SCANN_ABI_VERSION 1")
    with pytest.raises(AssertionError):
        abi_checks.declared("int scann_index_create(scann_handle_t* h, int64_t dim, scann_index_t** out);")
    sig = abi_checks.signatures({"scann_index_create": (C.c_int, [P, C.c_int32, C.POINTER(P)])})
    assert "scann_index_free" in sig  # the whole table comes back
    for wrong in ((C.c_int, [P, C.c_int64, C.POINTER(P)]), (C.c_int64, [P, C.c_int32, C.POINTER(P)]), (C.c_int, [P, C.c_int32])):
        with pytest.raises(AssertionError):
            abi_checks.signatures({"scann_index_create": wrong})
    with pytest.raises(AssertionError):
        abi_checks.signatures({"scann_no_such_call": (C.c_int, [P])})
    assert abi_checks.header() is abi_checks.header()


def test_device_kernels_takes_a_library_apart_once(hip_lib, monkeypatch):
    from scann import _hip

    runs = []
    real = abi_checks._read_device_kernels
    monkeypatch.setattr(abi_checks, "_KERNELS", {})
    monkeypatch.setattr(abi_checks, "_read_device_kernels", lambda path: runs.append(path) or real(path))
    first = abi_checks.device_kernels(_hip.LIB_PATH)
    assert abi_checks.device_kernels(_hip.LIB_PATH) is first and len(runs) == 1 and len(first) > 10
    assert all(isinstance(s, int) and isinstance(v, int) for s, v in first.values())


def test_device_kernels_does_not_remember_a_skip(tmp_path, monkeypatch):
    lib = tmp_path / "lib.so"
    lib.write_bytes(b"x")
    runs = []

    def skips(path):
        runs.append(path)
        pytest.skip("no tools")

    monkeypatch.setattr(abi_checks, "_KERNELS", {})
    monkeypatch.setattr(abi_checks, "_read_device_kernels", skips)
    for _ in range(2):
        with pytest.raises(pytest.skip.Exception):
            abi_checks.device_kernels(str(lib))
    assert len(runs) == 2
    monkeypatch.setattr(abi_checks, "_read_device_kernels", lambda path: {"k": (0, 1)})
    assert abi_checks.device_kernels(str(lib)) == {"k": (0, 1)}
    lib.write_bytes(b"xy")  # another size: read again
    monkeypatch.setattr(abi_checks, "_read_device_kernels", lambda path: {"k": (0, 2)})
    assert abi_checks.device_kernels(str(lib)) == {"k": (0, 2)}


def test_stand_in_model():
    cfg = so.default_config("qm9")
    m = abi_checks.stand_in_model(cfg, lambda config: ("engine", config["model"]["dense_out"]))
    assert m.engine == ("engine", 128) and "ring_aromatic" not in m.input_names
    cfg["model"]["use_ring"] = True
    assert "ring_aromatic" in abi_checks.stand_in_model(cfg, lambda config: None, ring=True).input_names
    assert "ring_aromatic" not in abi_checks.stand_in_model(cfg, lambda config: None).input_names
