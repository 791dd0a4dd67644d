"""GPU tests of the paths the searches over a latent-space index share on the host (csrc/scann_search.h).

1. Windows of the index's own rows that start just before, on and just behind a storage-chunk boundary: ``index_query_rows`` and
   ``index_within_rows`` equal ``index_read`` of the window followed by ``index_query`` / ``index_within`` in every byte, without a
   partition and with one, and the two layouts answer alike.
2. Every refusal of scann_index_query, _query_rows, _query_batch, _within, _within_rows, _within_batch and _add_batch through ctypes, one
   call per wrong argument and, for the batch entry points, per pair of wrong arguments: the status and the handle's error text, as
   literals.  The order of an entry point's checks decides which of two wrong arguments a caller hears about; no call launches a kernel.
   (The "empty query" of the batch entry points is not among them: scann_batch_upload refuses an empty batch, so none reaches them.)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from analysis_checks import setup  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(hip_lib):
    cfg, w, inputs, m = setup(n=4, seed=1)
    m.inputs4 = inputs
    yield m
    m.engine.close()


# ---- 1. windows across a chunk boundary ----

CHUNK = 16384  # rows of a storage chunk at 1,024 columns (64 MiB of rows)
N_ROWS = 16400  # two chunks; the last window, rows 16,385 .. 16,392, still lies inside


def bytes_equal(a, b, label):
    assert a.keys() == b.keys(), label
    for key in a:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (label, key)


def without_own(w, first):
    """index_within's result without the hit of query i at position first + i, as index_within_rows counts"""
    query = np.repeat(np.arange(len(w["count"])), w["count"])
    keep = w["position"] != first + query
    count = np.bincount(query[keep], minlength=len(w["count"])).astype(np.int64)
    out = {"count": count, "first": np.concatenate(([0], np.cumsum(count))).astype(np.int64), "total": int(keep.sum())}
    for key in ("dist2", "position", "id", "atom"):
        out[key] = w[key][keep]
    return out


def test_windows_across_a_chunk_boundary(model):
    eng = model.engine
    rng = np.random.default_rng(61)
    rows = np.zeros((N_ROWS, 1024), np.float32)
    rows[:, :6] = rng.integers(0, 4, (N_ROWS, 6))  # 4,096 grid points: every row has copies, every distance ties
    ix = eng.index_create(1024)
    eng.index_add(ix, rows, ids=np.arange(N_ROWS, dtype=np.int64) // 3, atoms=(np.arange(N_ROWS) % 5).astype(np.int32))
    k, r2 = 8, 1.0
    answers = {}
    try:
        for layout, cells in (("no partition", 0), ("7 cells", 7)):
            eng.index_partition(ix, cells, 4)
            for first in (CHUNK - 1, CHUNK, CHUNK + 1):
                for n in (1, 2, 8):
                    label = "%s, rows %d .. %d" % (layout, first, first + n)
                    window = eng.index_read(ix, first, n)[0]
                    assert window.tobytes() == rows[first:first + n].tobytes(), label
                    near = eng.index_query_rows(ix, first, n, k)
                    bytes_equal(near, eng.index_query(ix, window, k), label + ": query_rows")
                    hits = eng.index_within_rows(ix, first, n, r2)
                    bytes_equal(hits, without_own(eng.index_within(ix, window, r2), first), label + ": within_rows")
                    assert hits["total"] > 0 and len(np.unique(near["dist2"])) < near["dist2"].size, label  # (ties did occur)
                    if cells:
                        bytes_equal(near, answers[first, n][0], label + ": query_rows against no partition")
                        bytes_equal(hits, answers[first, n][1], label + ": within_rows against no partition")
                    else:
                        answers[first, n] = near, hits
    finally:
        ix.free()


# ---- 2. the refusals ----

def refusals(model):
    """{label: (status, the handle's error text)} of every refused call"""
    from scann import _hip

    eng, lib = model.engine, model.engine.lib
    bare = _hip.Engine(eng.cfg, device=0)  # a handle whose weights were never loaded
    packed = _hip.pack_inputs(model.inputs4)
    made = []

    def index(e, dim, n):
        ix = e.index_create(dim)
        if n:
            e.index_add(ix, np.zeros((n, dim), np.float32))
        made.append(ix)
        return ix

    q = np.zeros((3, 128), np.float32)
    d, counts, tot = np.zeros(3 * 32, np.float32), np.zeros(64, np.int64), np.zeros(1, np.int64)
    qp, dp, cp, tp = q.ctypes.data, d.ctypes.data, counts.ctypes.data, tot.ctypes.data
    AT, BF = _hip.OUT_AFTER_LC, _hip.OUT_BF_PROPERTY
    out = {}
    try:
        ix, narrow, ixb = index(eng, 128, 10), index(eng, 64, 10), index(bare, 128, 10)
        rb, rbb = eng.upload(packed), bare.upload(packed)
        made += [rb, rbb]
        H, X, R = eng._h, ix._h, rb._h

        def note(label, handle, status):
            assert label not in out, label
            out[label] = (int(status), (lib.scann_last_error(handle) or b"").decode())

        def query(label, h=H, x=X, q=qp, nq=3, k=5, dist2=dp):
            note("query: " + label, h, lib.scann_index_query(h, x, q, nq, None, k, dist2, None, None, None))

        def query_rows(label, h=H, x=X, first=0, n=2, k=5, dist2=dp):
            note("query_rows: " + label, h, lib.scann_index_query_rows(h, x, first, n, k, dist2, None, None, None))

        def query_batch(label, h=H, x=X, b=R, level=AT, k=5, dist2=dp):
            note("query_batch: " + label, h, lib.scann_index_query_batch(h, x, b, level, None, k, None, None, dist2, None, None, None))

        def within(label, h=H, x=X, q=qp, nq=3, r2=1.0, cap=0, c=cp, t=tp, dist2=None):
            note("within: " + label, h, lib.scann_index_within(h, x, q, nq, None, r2, cap, c, t, dist2, None, None, None))

        def within_rows(label, h=H, x=X, first=0, n=2, upper=0, r2=1.0, cap=0, c=cp, t=tp, dist2=None):
            note("within_rows: " + label, h, lib.scann_index_within_rows(h, x, first, n, upper, r2, cap, c, t, dist2, None, None, None))

        def within_batch(label, h=H, x=X, b=R, level=AT, r2=1.0, cap=0, c=cp, t=tp, dist2=None):
            note("within_batch: " + label, h, lib.scann_index_within_batch(h, x, b, level, None, r2, cap, None, None, c, t, dist2, None, None, None))

        def add_batch(label, h=H, x=X, b=R, level=AT):
            note("add_batch: " + label, h, lib.scann_index_add_batch(h, x, b, level, None))

        for call in (query, query_rows, query_batch, within, within_rows, within_batch, add_batch):
            call("null handle", h=None)
            call("null index", x=None)
            call("index of another handle", x=ixb._h)
        for call in (query, query_rows, query_batch):
            for k in (0, 33):
                call("k %d" % k, k=k)
            call("null dist2", dist2=None)
        for call in (query, within):
            call("null q", q=None)
            call("nq 0", nq=0)
        query("too many queries", nq=(0x7fffffff // 32) + 1)
        within("too many queries", nq=0x80000000)
        for call in (query_rows, within_rows):
            call("first -1", first=-1)
            call("n 0", n=0)
            call("past the end", first=5, n=6)
        for call in (within, within_rows, within_batch):
            call("null counts", c=None)
            call("null total", t=None)
            call("radius2 NaN", r2=float("nan"))
            call("radius2 -1", r2=-1.0)
            call("cap -1", cap=-1)
            call("cap above the limit", cap=(1 << 30) + 1)
            call("cap 0 with dist2", dist2=dp)
        within_rows("upper 2", upper=2)
        for call in (query_batch, within_batch, add_batch):
            call("null batch", b=None)
            call("level 7", level=7)
            call("an index of 64 columns", x=narrow._h, level=BF)
            call("weights not loaded", h=bare._h, x=ixb._h, b=rbb._h)
            call("weights not loaded, level 7", h=bare._h, x=ixb._h, b=rbb._h, level=7)
            call("weights not loaded, null batch", h=bare._h, x=ixb._h, b=None)
        # pairs of wrong arguments at the two searches of a batch
        query_batch("level 7, k 0", level=7, k=0)
        query_batch("level 7, null dist2", level=7, dist2=None)
        query_batch("k 0, null dist2", k=0, dist2=None)
        within_batch("level 7, radius2 -1", level=7, r2=-1.0)
        within_batch("level 7, null counts", level=7, c=None)
        within_batch("radius2 -1, cap -1", r2=-1.0, cap=-1)
        unloaded = dict(h=bare._h, x=ixb._h, b=rbb._h)
        query_batch("weights not loaded, k 0", k=0, **unloaded)
        query_batch("weights not loaded, null dist2", dist2=None, **unloaded)
        query_batch("weights not loaded, level 7, k 0", level=7, k=0, **unloaded)
        within_batch("weights not loaded, radius2 -1", r2=-1.0, **unloaded)
        within_batch("weights not loaded, null counts", c=None, **unloaded)
        within_batch("weights not loaded, level 7, radius2 -1", level=7, r2=-1.0, **unloaded)
        assert len(ix) == 10 and len(ixb) == 10  # nothing was added
    finally:
        for x in reversed(made):
            x.free()
        bare.close()
    return out


# what the library answered before the searches shared their host pieces, recorded by this function
EXPECTED = {
    'query: null handle': (-1, 'scann_index_query: null argument'),
    'query: null index': (-1, 'scann_index_query: null argument'),
    'query: index of another handle': (-1, 'scann_index_query: the index belongs to another handle'),
    'query_rows: null handle': (-1, 'scann_index_query_rows: null argument'),
    'query_rows: null index': (-1, 'scann_index_query_rows: null argument'),
    'query_rows: index of another handle': (-1, 'scann_index_query_rows: the index belongs to another handle'),
    'query_batch: null handle': (-1, 'scann_index_query_batch: null argument'),
    'query_batch: null index': (-1, 'scann_index_query_batch: null argument'),
    'query_batch: index of another handle': (-1, 'scann_index_query_batch: the index belongs to another handle'),
    'within: null handle': (-1, 'scann_index_within: null argument'),
    'within: null index': (-1, 'scann_index_within: null argument'),
    'within: index of another handle': (-1, 'scann_index_within: the index belongs to another handle'),
    'within_rows: null handle': (-1, 'scann_index_within_rows: null argument'),
    'within_rows: null index': (-1, 'scann_index_within_rows: null argument'),
    'within_rows: index of another handle': (-1, 'scann_index_within_rows: the index belongs to another handle'),
    'within_batch: null handle': (-1, 'scann_index_within_batch: null argument'),
    'within_batch: null index': (-1, 'scann_index_within_batch: null argument'),
    'within_batch: index of another handle': (-1, 'scann_index_within_batch: the index belongs to another handle'),
    'add_batch: null handle': (-1, 'scann_index_add_batch: null argument'),
    'add_batch: null index': (-1, 'scann_index_add_batch: null argument'),
    'add_batch: index of another handle': (-1, 'scann_index_add_batch: the index belongs to another handle'),
    'query: k 0': (-1, 'scann_index_query: k 0 outside 1 .. 32'),
    'query: k 33': (-1, 'scann_index_query: k 33 outside 1 .. 32'),
    'query: null dist2': (-1, 'scann_index_query: dist2 is null'),
    'query_rows: k 0': (-1, 'scann_index_query_rows: k 0 outside 1 .. 32'),
    'query_rows: k 33': (-1, 'scann_index_query_rows: k 33 outside 1 .. 32'),
    'query_rows: null dist2': (-1, 'scann_index_query_rows: dist2 is null'),
    'query_batch: k 0': (-1, 'scann_index_query_batch: k 0 outside 1 .. 32'),
    'query_batch: k 33': (-1, 'scann_index_query_batch: k 33 outside 1 .. 32'),
    'query_batch: null dist2': (-1, 'scann_index_query_batch: dist2 is null'),
    'query: null q': (-1, 'scann_index_query: an empty query'),
    'query: nq 0': (-1, 'scann_index_query: an empty query'),
    'within: null q': (-1, 'scann_index_within: an empty query'),
    'within: nq 0': (-1, 'scann_index_within: an empty query'),
    'query: too many queries': (-1, 'scann_index_query: too many queries in one call'),
    'within: too many queries': (-1, 'scann_index_within: too many queries in one call'),
    'query_rows: first -1': (-1, 'scann_index_query_rows: rows -1 .. 1 of 10'),
    'query_rows: n 0': (-1, 'scann_index_query_rows: rows 0 .. 0 of 10'),
    'query_rows: past the end': (-1, 'scann_index_query_rows: rows 5 .. 11 of 10'),
    'within_rows: first -1': (-1, 'scann_index_within_rows: rows -1 .. 1 of 10'),
    'within_rows: n 0': (-1, 'scann_index_within_rows: rows 0 .. 0 of 10'),
    'within_rows: past the end': (-1, 'scann_index_within_rows: rows 5 .. 11 of 10'),
    'within: null counts': (-1, 'scann_index_within: counts or total is null'),
    'within: null total': (-1, 'scann_index_within: counts or total is null'),
    'within: radius2 NaN': (-1, 'scann_index_within: radius2 must be >= 0 (+inf allowed) and not NaN'),
    'within: radius2 -1': (-1, 'scann_index_within: radius2 must be >= 0 (+inf allowed) and not NaN'),
    'within: cap -1': (-1, 'scann_index_within: cap -1 outside 0 .. 1073741824'),
    'within: cap above the limit': (-1, 'scann_index_within: cap 1073741825 outside 0 .. 1073741824'),
    'within: cap 0 with dist2': (-1, 'scann_index_within: cap 0 is the count-only call, its entry arrays must be null'),
    'within_rows: null counts': (-1, 'scann_index_within_rows: counts or total is null'),
    'within_rows: null total': (-1, 'scann_index_within_rows: counts or total is null'),
    'within_rows: radius2 NaN': (-1, 'scann_index_within_rows: radius2 must be >= 0 (+inf allowed) and not NaN'),
    'within_rows: radius2 -1': (-1, 'scann_index_within_rows: radius2 must be >= 0 (+inf allowed) and not NaN'),
    'within_rows: cap -1': (-1, 'scann_index_within_rows: cap -1 outside 0 .. 1073741824'),
    'within_rows: cap above the limit': (-1, 'scann_index_within_rows: cap 1073741825 outside 0 .. 1073741824'),
    'within_rows: cap 0 with dist2': (-1, 'scann_index_within_rows: cap 0 is the count-only call, its entry arrays must be null'),
    'within_batch: null counts': (-1, 'scann_index_within_batch: counts or total is null'),
    'within_batch: null total': (-1, 'scann_index_within_batch: counts or total is null'),
    'within_batch: radius2 NaN': (-1, 'scann_index_within_batch: radius2 must be >= 0 (+inf allowed) and not NaN'),
    'within_batch: radius2 -1': (-1, 'scann_index_within_batch: radius2 must be >= 0 (+inf allowed) and not NaN'),
    'within_batch: cap -1': (-1, 'scann_index_within_batch: cap -1 outside 0 .. 1073741824'),
    'within_batch: cap above the limit': (-1, 'scann_index_within_batch: cap 1073741825 outside 0 .. 1073741824'),
    'within_batch: cap 0 with dist2': (-1, 'scann_index_within_batch: cap 0 is the count-only call, its entry arrays must be null'),
    'within_rows: upper 2': (-1, 'scann_index_within_rows: upper must be 0 or 1, got 2'),
    'query_batch: null batch': (-1, 'scann_index_query_batch: null argument'),
    'query_batch: level 7': (-1, 'scann_index_query_batch: level must be SCANN_OUT_BF_PROPERTY or SCANN_OUT_AFTER_LC, got 7'),
    'query_batch: an index of 64 columns': (-1, "scann_index_query_batch: the index holds rows of 64 columns, the model's dense_out is 128"),
    'query_batch: weights not loaded': (-5, 'scann_index_query_batch: weights not loaded'),
    'query_batch: weights not loaded, level 7': (-1, 'scann_index_query_batch: level must be SCANN_OUT_BF_PROPERTY or SCANN_OUT_AFTER_LC, got 7'),
    'query_batch: weights not loaded, null batch': (-1, 'scann_index_query_batch: null argument'),
    'within_batch: null batch': (-1, 'scann_index_within_batch: null argument'),
    'within_batch: level 7': (-1, 'scann_index_within_batch: level must be SCANN_OUT_BF_PROPERTY or SCANN_OUT_AFTER_LC, got 7'),
    'within_batch: an index of 64 columns': (-1, "scann_index_within_batch: the index holds rows of 64 columns, the model's dense_out is 128"),
    'within_batch: weights not loaded': (-5, 'scann_index_within_batch: weights not loaded'),
    'within_batch: weights not loaded, level 7': (-1, 'scann_index_within_batch: level must be SCANN_OUT_BF_PROPERTY or SCANN_OUT_AFTER_LC, got 7'),
    'within_batch: weights not loaded, null batch': (-1, 'scann_index_within_batch: null argument'),
    'add_batch: null batch': (-1, 'scann_index_add_batch: null argument'),
    'add_batch: level 7': (-1, 'scann_index_add_batch: level must be SCANN_OUT_BF_PROPERTY or SCANN_OUT_AFTER_LC, got 7'),
    'add_batch: an index of 64 columns': (-1, "scann_index_add_batch: the index holds rows of 64 columns, the model's dense_out is 128"),
    'add_batch: weights not loaded': (-5, 'scann_index_add_batch: weights not loaded'),
    'add_batch: weights not loaded, level 7': (-1, 'scann_index_add_batch: level must be SCANN_OUT_BF_PROPERTY or SCANN_OUT_AFTER_LC, got 7'),
    'add_batch: weights not loaded, null batch': (-1, 'scann_index_add_batch: null argument'),
    'query_batch: level 7, k 0': (-1, 'scann_index_query_batch: k 0 outside 1 .. 32'),
    'query_batch: level 7, null dist2': (-1, 'scann_index_query_batch: level must be SCANN_OUT_BF_PROPERTY or SCANN_OUT_AFTER_LC, got 7'),
    'query_batch: k 0, null dist2': (-1, 'scann_index_query_batch: k 0 outside 1 .. 32'),
    'within_batch: level 7, radius2 -1': (-1, 'scann_index_within_batch: level must be SCANN_OUT_BF_PROPERTY or SCANN_OUT_AFTER_LC, got 7'),
    'within_batch: level 7, null counts': (-1, 'scann_index_within_batch: level must be SCANN_OUT_BF_PROPERTY or SCANN_OUT_AFTER_LC, got 7'),
    'within_batch: radius2 -1, cap -1': (-1, 'scann_index_within_batch: radius2 must be >= 0 (+inf allowed) and not NaN'),
    'query_batch: weights not loaded, k 0': (-1, 'scann_index_query_batch: k 0 outside 1 .. 32'),
    'query_batch: weights not loaded, null dist2': (-1, 'scann_index_query_batch: dist2 is null'),
    'query_batch: weights not loaded, level 7, k 0': (-1, 'scann_index_query_batch: k 0 outside 1 .. 32'),
    'within_batch: weights not loaded, radius2 -1': (-1, 'scann_index_within_batch: radius2 must be >= 0 (+inf allowed) and not NaN'),
    'within_batch: weights not loaded, null counts': (-1, 'scann_index_within_batch: counts or total is null'),
    'within_batch: weights not loaded, level 7, radius2 -1': (-1, 'scann_index_within_batch: level must be SCANN_OUT_BF_PROPERTY or SCANN_OUT_AFTER_LC, got 7'),
}


def test_every_refusal_keeps_its_status_and_text(model):
    got = refusals(model)
    assert got.keys() == EXPECTED.keys()
    wrong = {label: (got[label], EXPECTED[label]) for label in EXPECTED if got[label] != EXPECTED[label]}
    assert not wrong, wrong
