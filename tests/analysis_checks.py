"""What the GPU tests of the analyses share: the builders of a model, a batch and an index, and the three invariants every analysis is
held to, each stated once.

untouched      an analysis call leaves an inference handle alone: index rows, the batch's last y, the selected outputs, the
               unselected one, the weights and the predictions are where they were, and repeated calls stay within a device-memory bound
training_twin  an analysis call leaves a training handle alone: gradients, weights, the following step and the weights after it are
               those of a twin handle that never made the call
steady_memory  repeated calls do not eat device memory

Which call, which host twin and which comparison of results is the test's own business.  Nothing here runs at import time."""
import contextlib

import numpy as np

import scann_oracle as so


# ---- builders ----

def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def padded(kind, n, seed, cfg):
    inputs, _ = so.pad_batch(*so.synth_dataset(n, seed, kind=kind), g_update=cfg["model"]["g_update"])
    return {k: np.array(v) for k, v in inputs.items()}


def setup(kind="qm9", n=24, seed=0, infer=True, **over):
    """as tests/test_gpu_rollout.py::setup builds its model and batch"""
    from scann.models.scann_model import HipModel

    cfg = so.default_config(kind)
    cfg["model"].update(over)
    w = so.init_weights(cfg, 1234, perturb=True)
    return cfg, w, padded(kind, n, seed, cfg), HipModel(cfg, w, device=0, infer=infer)


def amask_of(inputs):
    return np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0


def make_index(eng, rows, ids=None, atoms=None):
    ix = eng.index_create(rows.shape[1])
    if len(rows):
        eng.index_add(ix, rows, ids, atoms)
    return ix


def random_rows(N, dim, seed=None):
    """columns of very different scale and offset, a few duplicated rows"""
    rng = np.random.default_rng(N * 7 + dim * 3 if seed is None else seed)
    rows = (rng.standard_normal((N, dim)) * rng.uniform(0.01, 30, dim) + rng.standard_normal(dim) * 5).astype(np.float32)
    if N >= 100:
        rows[N // 2:N // 2 + 4] = rows[3]
    return rows


SUBNORMAL = np.float32(2.0 ** -149)  # the smallest fp32 above zero


def subnormal_column(rng, n):
    """n values k * 2^-149, 1 <= k < 400: frexp's exponent of the largest takes the subnormal branch, and no mean of them is zero"""
    return rng.integers(1, 400, n).astype(np.float32) * SUBNORMAL


def scan_edge_rows():
    """The smallest indexes that reach every edge of the eligibility scan the prepare kernels share (csrc/scann_prim.h: 8 lanes per row, 32
    rows per pass, 32 columns per trip of a lane): 1, 31, 32 and 33 rows -- the pass boundary from both sides --; widths 1 and 5 -- strides 4
    and 8, lanes without a column -- and 32 and 36 -- the last lane's columns, and a second trip.  From 31 rows on, +inf stands in column
    0 of row 0 and NaN in the last column of the last row; from width 5 on, -inf in the last column of row 1 (a NaN distance never
    qualifies whatever the scan said, an infinite one does), and column 1 holds subnormals only.  Yields (label, rows)."""
    for n in (1, 31, 32, 33):
        for dim in (1, 5, 32, 36):
            rng = np.random.default_rng(100 * n + dim)
            rows = (rng.standard_normal((n, dim)) * 3).astype(np.float32)
            if dim >= 5:
                rows[:, 1] = subnormal_column(rng, n)
            if n >= 31:
                rows[0, 0] = np.inf
                rows[n - 1, dim - 1] = np.nan
                if dim >= 5:
                    rows[1, dim - 1] = -np.inf
            yield "scan edges, N %d dim %d" % (n, dim), rows


def rel_err(got, ref):
    """tests/test_gpu_outputs.py's"""
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    scale = max(float(np.sqrt(np.mean(ref * ref))), 1e-30)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), scale)))


# ---- comparisons ----

def same_arrays(got, want, label=""):
    """two dicts of arrays: the same keys, and under each key the same dtype, shape and bytes"""
    assert sorted(got) == sorted(want), (label, sorted(got), sorted(want))
    for key, b in want.items():
        a, b = np.asarray(got[key]), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (label, key, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (label, key)


def _same_tuple(got, want, label):
    assert len(got) == len(want), label
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (label, i)


def steady_memory(eng, call, times, slack_bytes):
    """``call(rep)`` for rep = 0 .. times - 1 takes at most ``slack_bytes`` from the device: repeated calls get their workspace from the
    block cache.  The caller makes the first call itself, before this.  Returns the free bytes before the loop."""
    free0, _ = eng.device_memory()
    for rep in range(times):
        call(rep)
    free1, _ = eng.device_memory()
    assert free0 - free1 <= slack_bytes, (free0, free1)
    return free0


# ---- an inference handle is left alone ----

class _Untouched:
    """what ``untouched`` hands its body: ``eng``; ``rb``, the resident batch after its forward; ``pool``, an index of the batch's
    after_Lc rows; ``rows``, what index_read gave for it (rows, ids, atoms); ``y_first``, the batch's y"""

    def __init__(self, model, data):
        from scann import _hip

        self._hip, self.eng = _hip, model.engine
        eng = self.eng
        self.rb = eng.upload(_hip.pack_inputs(data))
        eng.forward_resident(self.rb)
        self.y_first, _ = eng.download(self.rb)
        self._sel0 = [eng.read_output(self.rb, _hip.OUT_LOCAL_ATTENTION, 1), eng.read_output(self.rb, _hip.OUT_AFTER_LC)]
        self._unselected_is_unreadable()
        self.pool = eng.index_create(self._sel0[1].shape[1])
        eng.index_add_batch(self.pool, self.rb, _hip.OUT_AFTER_LC)
        self.reforward()  # the call above ran a forward with after_Lc selected; the batch's block is the handle's own again
        self.rows = eng.index_read(self.pool)
        self._near = self.rows[0][:9] + np.float32(0.01)
        self._q0 = eng.index_query(self.pool, self._near, 3)
        self._memory = None

    def _unselected_is_unreadable(self):
        try:
            self.eng.read_output(self.rb, self._hip.OUT_BF_PROPERTY)
        except self._hip.ScannHipError:
            return
        raise AssertionError("bf_property is not selected, and the batch's block gives it")

    def reforward(self):
        """a plain forward and download of the batch, as after a ..._batch call that ran a forward with a selection of its own"""
        self.eng.forward_resident(self.rb)
        self.eng.download(self.rb)

    def repeat(self, call, same, times, slack_bytes):
        """``same(call())`` ``times`` times within ``slack_bytes`` of device memory; the first call is the body's, before this"""
        self._memory = (steady_memory(self.eng, lambda rep: same(call()), times, slack_bytes), slack_bytes)

    def check(self):
        """the index, the batch's last y and the outputs of its last forward are where they were.  The exit runs this; a body that goes
        on to forward the batch again (reforward, a ..._batch call) runs it before that, while it still says something."""
        _hip, eng = self._hip, self.eng
        assert len(self.pool) == len(self.rows[0])
        _same_tuple(eng.index_read(self.pool), self.rows, "index rows")
        same_arrays(eng.index_query(self.pool, self._near, 3), self._q0, "a search of the index")
        y_again, _ = eng.download(self.rb)
        assert np.array_equal(_bits(y_again), _bits(self.y_first))
        assert np.array_equal(_bits(eng.read_output(self.rb, _hip.OUT_LOCAL_ATTENTION, 1)), _bits(self._sel0[0]))
        assert np.array_equal(_bits(eng.read_output(self.rb, _hip.OUT_AFTER_LC)), _bits(self._sel0[1]))
        self._unselected_is_unreadable()

    def _close(self):
        self.check()
        self.rb.free()
        self.pool.free()
        if self._memory is not None:  # nothing was taken from the device that did not come back
            free0, slack = self._memory
            assert free0 - self.eng.device_memory()[0] <= slack, (free0, self.eng.device_memory()[0])


@contextlib.contextmanager
def untouched(model, data):
    """The frame of every test_nothing_else_changes.  Entry: predictions and weights recorded, local_attention_1 and after_Lc selected,
    the batch uploaded and forwarded, an index built from its after_Lc rows, the batch forwarded again.  The body makes the analysis's
    calls.  Clean exit: _Untouched.check, then the weights, predict(outputs=...) and predict are bit for bit what they were.  The
    selection is taken back whether the body raises or not."""
    eng = model.engine
    names = ["local_attention_1", "after_Lc"]
    before = model.predict(data, outputs=names)
    y0, ga0 = model.predict(data)
    w0 = eng.get_weights()
    eng.set_outputs([1], after_lc=True)
    try:
        u = _Untouched(model, data)
        yield u
        u._close()
    finally:
        eng.set_outputs()
    same_arrays(eng.get_weights(), w0, "weights")
    after = model.predict(data, outputs=names)
    assert len(after) == len(before) and all(np.array_equal(_bits(x), _bits(y_)) for x, y_ in zip(before, after))
    y1, ga1 = model.predict(data)
    assert np.array_equal(_bits(y0), _bits(y1)) and np.array_equal(_bits(ga0), _bits(ga1))


# ---- a training handle is left alone ----

def training_twin(cfg, w, pk, calls, model_class=None):
    """The frame of every test_training_handle.  Two deterministic training handles take two steps each (seeds 3 and 4) on ``pk``.
    ``calls(train_model, rb, inference)`` runs on the first only; ``inference()`` gives (model, rb2): an inference HipModel with the
    training handle's current weights and ``pk`` resident on it, built on first use.  Then both give their gradients and weights,
    take a third step (seed 5; the Adam state enters it) and give their weights again: all four equal, bit for bit and key by key."""
    if model_class is None:
        from scann.models.scann_model import HipModel as model_class
    targets = np.linspace(-1, 1, pk.n_struct).astype(np.float32)
    res = []
    for makes_the_calls in (True, False):
        model = model_class(cfg, w, device=0, deterministic=True)
        eng = model.engine
        eng.train_begin()
        rb = eng.upload(pk)
        eng.train_step(rb, targets, 1e-3, dropout=0.1, seed=3)
        eng.train_step(rb, targets, 1e-3, dropout=0.1, seed=4)
        if makes_the_calls:
            made = []

            def inference():
                if not made:
                    inf = model_class(cfg, eng.get_weights(), device=0, infer=True)
                    made.append((inf, inf.engine.upload(pk)))
                return made[0]

            calls(model, rb, inference)
            for _, rb2 in made:
                rb2.free()
        grads, weights = eng.get_grads(), eng.get_weights()
        step = eng.train_step(rb, targets, 1e-3, dropout=0.1, seed=5)
        res.append((grads, weights, step, eng.get_weights()))
        rb.free()
    (ga, wa, sa, wa2), (gb, wb, sb, wb2) = res
    same_arrays(ga, gb, "gradients")
    same_arrays(wa, wb, "weights")
    assert sa == sb, (sa, sb)
    same_arrays(wa2, wb2, "weights after the following step")
