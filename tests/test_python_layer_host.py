"""Host tests of the steps the analysis Python layer states once: the saved-result base of latent_index.py (the keys, dtypes and shapes
of every ``.npz``, the mismatch messages, files without a ``kind``), the SCANN facade built from its table (HipModel's signatures, the
one de-normalised key) and HipModel's "index or data" scope (an index built for a call is freed, also on an error; one passed in never).
Every expected key list and message is a literal taken from the code before the base existed.  No GPU."""
import inspect
import types

import numpy as np
import pytest

import test_knn_host as tk

F4, F8, I4, I8 = "<f4", "<f8", "<i4", "<i8"


def _rows(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


_HEAD = {"mean": _rows(1, 4, 0)[0], "tmean": np.float32([0.5]), "weights": _rows(1, 4, 1), "components": _rows(2, 4, 2), "scale": _rows(1, 2, 3),
         "lev0": np.array(0.25), "sigma2": np.array([0.125]), "l2": np.array([1e-3]), "level": np.array("structure"),
         "dim": np.array(4, dtype=np.int64), "names": np.array(["gap"], dtype=np.str_)}
# the inner head of the kernel head regresses on its 3 features; the landmarks have the model's width
_KERNEL = {"landmarks": _rows(3, 4, 4), "gamma": np.array(0.75, dtype=np.float32), "mean": _rows(1, 3, 5)[0], "tmean": np.float32([0.5]),
           "weights": _rows(1, 3, 6), "components": _rows(2, 3, 7), "scale": _rows(1, 2, 8), "lev0": np.array(0.25), "sigma2": np.array([0.125]),
           "l2": np.array([1e-3]), "level": np.array("structure"), "dim": np.array(4, dtype=np.int64), "names": np.array(["gap"], dtype=np.str_)}
_LEVEL = {"level": np.array("structure"), "dim": np.array(4, dtype=np.int64)}

# class name -> (noun of the mismatch message, the file as np.savez gets it, {key: (dtype, shape)} of a saved file)
SAVED = {
    "LatentHead": ("head", _HEAD,
                   {"mean": (F4, (4,)), "tmean": (F4, (1,)), "weights": (F4, (1, 4)), "components": (F4, (2, 4)), "scale": (F4, (1, 2)), "lev0": (F8, ()),
                    "sigma2": (F8, (1,)), "l2": (F8, (1,)), "level": ("<U9", ()), "dim": (I8, ()), "names": ("<U3", (1,))}),
    "LatentClassHead": ("head", dict(_LEVEL, mean=_rows(1, 4, 9)[0], weights=_rows(2, 5, 10), classes=np.array([3, 7]), l2=np.array(0.5),
                                     kind=np.array("class_head")),
                        {"mean": (F4, (4,)), "weights": (F4, (2, 5)), "classes": (I8, (2,)), "l2": (F8, ()), "level": ("<U9", ()), "dim": (I8, ()),
                         "kind": ("<U10", ())}),
    "LatentKernelHead": ("kernel head", _KERNEL,
                         {"landmarks": (F4, (3, 4)), "gamma": (F4, ()), "mean": (F4, (3,)), "tmean": (F4, (1,)), "weights": (F4, (1, 3)),
                          "components": (F4, (2, 3)), "scale": (F4, (1, 2)), "lev0": (F8, ()), "sigma2": (F8, (1,)), "l2": (F8, (1,)),
                          "level": ("<U9", ()), "dim": (I8, ()), "names": ("<U3", (1,))}),
    "LatentProjection": ("projection", dict(_LEVEL, mean=_rows(1, 4, 11)[0], components=_rows(2, 4, 12), variance=np.array([2.0, 0.5]),
                                            noise_floor=np.array(1e-6)),
                         {"mean": (F4, (4,)), "components": (F4, (2, 4)), "variance": (F8, (2,)), "noise_floor": (F8, ()), "level": ("<U9", ()),
                          "dim": (I8, ())}),
    "LatentClustering": ("clustering", dict(_LEVEL, centres=_rows(3, 4, 13)), {"centres": (F4, (3, 4)), "level": ("<U9", ()), "dim": (I8, ())}),
    "LatentEmbedding": ("embedding", dict(_LEVEL, coordinates=_rows(3, 2, 14), ids=np.array([5, 6, 7]), atoms=np.int32([-1, -1, -1]),
                                          perplexity=np.array(5.0)),
                        {"coordinates": (F4, (3, 2)), "ids": (I8, (3,)), "atoms": (I4, (3,)), "perplexity": (F8, ()), "level": ("<U9", ()),
                         "dim": (I8, ())}),
    "LatentPeaks": ("density-peak clustering", dict(_LEVEL, label=np.int32([0, 1, -1]), ids=np.array([5, 6, 7]), atoms=np.int32([-1, -1, -1]),
                                                    centre_position=np.int32([0, 1]), bandwidth=np.array(1.5)),
                    {"label": (I4, (3,)), "ids": (I8, (3,)), "atoms": (I4, (3,)), "centre_position": (I4, (2,)), "bandwidth": (F8, ()),
                     "level": ("<U9", ()), "dim": (I8, ())}),
    "LatentHierarchy": ("hierarchy", dict(_LEVEL, a=np.int32([0, 1]), b=np.int32([1, 2]), w=np.float32([1.0, 4.0]), core2=np.float32([0, 0, 0]),
                                          ids=np.array([5, 6, 7]), atoms=np.int32([-1, -1, -1]), min_samples=np.array(0, dtype=np.int64),
                                          lone_position=np.array(-1, dtype=np.int64)),
                        {"a": (I4, (2,)), "b": (I4, (2,)), "w": (F4, (2,)), "core2": (F4, (3,)), "ids": (I8, (3,)), "atoms": (I4, (3,)),
                         "min_samples": (I8, ()), "lone_position": (I8, ()), "level": ("<U9", ()), "dim": (I8, ())}),
}


def _width(dense_out):
    """what the saved results ask of a model: its configuration"""
    return types.SimpleNamespace(config={"model": {"dense_out": dense_out, "global_dim": 6}})


def _written(tmp_path, name, drop=()):
    path = str(tmp_path / (name + ".npz"))
    with open(path, "wb") as f:
        np.savez(f, **{k: v for k, v in SAVED[name][1].items() if k not in drop})
    return path


@pytest.mark.parametrize("name", sorted(SAVED))
def test_saved_file_keys_dtypes_shapes_and_values(tmp_path, name):
    import scann.models.latent_index as li

    cls, (_, given, layout) = getattr(li, name), SAVED[name]
    obj = cls.load(_width(4), _written(tmp_path, name))
    assert type(obj) is cls and obj.level == "structure" and obj.dim == 4
    path = str(tmp_path / "again.npz")
    obj.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(layout)
        assert {k: (z[k].dtype.str, z[k].shape) for k in z.files} == layout
        for k in z.files:
            assert np.array_equal(z[k], given[k]), k
    back = cls.load(_width(4), path)
    assert type(back) is cls and back.level == "structure" and back.dim == 4


@pytest.mark.parametrize("name", sorted(SAVED))
def test_mismatch_messages(tmp_path, name):
    import scann.models.latent_index as li

    cls, noun = getattr(li, name), SAVED[name][0]
    path = _written(tmp_path, name)
    obj = cls.load(_width(4), path)
    obj.check_model(_width(4))
    with pytest.raises(ValueError) as e:
        obj.check_model(_width(3))
    assert str(e.value) == "a structure-level %s of 4 columns does not fit a model whose dense_out is 3" % noun
    with pytest.raises(ValueError) as e:
        cls.load(_width(3), path)
    assert str(e.value) == "%s: a structure-level %s of 4 columns does not fit a model whose dense_out is 3" % (path, noun)
    # a level no model has: the width reads -1
    bad = str(tmp_path / "bad.npz")
    with open(bad, "wb") as f:
        np.savez(f, **dict(SAVED[name][1], level=np.array("bond")))
    with pytest.raises(ValueError) as e:
        cls.load(_width(4), bad)
    assert str(e.value) == "%s: a bond-level %s of 4 columns does not fit a model whose global_dim is -1" % (bad, noun)


def test_index_load_shares_the_message(tmp_path):
    from scann.models import LatentIndex

    path = str(tmp_path / "ix.npz")
    with open(path, "wb") as f:
        np.savez(f, rows=_rows(2, 4, 0), ids=np.array([0, 1]), atoms=np.int32([-1, -1]), level=np.array("structure"), dim=np.array(4, dtype=np.int64))
    m = _width(3)
    m.engine = types.SimpleNamespace(index_create=lambda dim: pytest.fail("an index was created"))
    with pytest.raises(ValueError) as e:
        LatentIndex.load(m, path)
    assert str(e.value) == "%s: a structure-level index of 4 columns does not fit a model whose dense_out is 3" % path


@pytest.mark.parametrize("name", sorted(SAVED))
def test_files_without_a_kind(tmp_path, name):
    """a class head demands its tag; every other class loads a file that has none, as the files written before the tag existed"""
    import scann.models.latent_index as li

    cls = getattr(li, name)
    path = _written(tmp_path, name, drop=("kind",))
    with np.load(path) as z:
        assert "kind" not in z.files
    if name == "LatentClassHead":
        with pytest.raises(ValueError) as e:
            cls.load(_width(4), path)
        assert str(e.value) == "%s: not a saved LatentClassHead" % path
        other = _written(tmp_path, "LatentHead")  # (another class's file is no class head either)
        with pytest.raises(ValueError) as e:
            cls.load(_width(4), other)
        assert str(e.value) == "%s: not a saved LatentClassHead" % other
    else:
        assert type(cls.load(_width(4), path)) is cls


def test_clustering_load_checks_the_centres_shape(tmp_path):
    from scann.models import LatentClustering

    path = str(tmp_path / "c.npz")
    with open(path, "wb") as f:
        np.savez(f, centres=_rows(3, 5, 0), level=np.array("structure"), dim=np.array(4, dtype=np.int64))
    with pytest.raises(ValueError) as e:
        LatentClustering.load(_width(4), path)
    assert str(e.value) == "%s: a structure-level clustering of 4 columns does not fit a model whose dense_out is 4" % path


# ---- the facade ----

HAND_WRITTEN = ("input_gradients", "atom_contributions", "atom_shapley", "predict_uncertainty")


def test_facade_table_covers_the_analysis_methods():
    from scann.models.scann_model import FACADE, SCANN, HipModel

    names = [n for n, _ in FACADE]
    assert len(set(names)) == len(names) == 25 and not set(names) & set(HAND_WRITTEN)
    assert {k for _, k in FACADE} == {None, "predict_property", "y"}
    for n in names + list(HAND_WRITTEN):
        assert callable(getattr(SCANN, n)) and callable(getattr(HipModel, n)), n


def test_facade_signatures_are_hipmodels():
    from scann.models.scann_model import FACADE, SCANN, HipModel

    for name, key in FACADE:
        assert inspect.signature(getattr(SCANN, name)) == inspect.signature(getattr(HipModel, name)), name
        doc = getattr(SCANN, name).__doc__
        first = "HipModel.%s as it is." % name if key is None else \
            "HipModel.%s with ``%s`` in the units of the target (times std plus mean, as predict_data)." % (name, key)
        assert doc.splitlines()[0] == first and getattr(HipModel, name).__doc__ in doc, name
        assert getattr(SCANN, name).__qualname__ == "SCANN." + name
    # a default of HipModel is the facade's: there is one place to change it
    assert inspect.signature(SCANN.fit_embedding).parameters["iterations"].default == (250, 500)
    assert inspect.signature(SCANN.density_peaks).parameters["neighbours"].default == 31


def test_facade_denormalises_exactly_the_declared_key():
    from scann.models.scann_model import FACADE, SCANN

    class Model:
        def __init__(self):
            self.seen = []

        def __getattr__(self, name):
            def call(*args, **kwargs):
                self.seen.append((name, args, kwargs))
                return self.result
            return call

    s = SCANN.__new__(SCANN)
    s.model, s.mean, s.std = Model(), 2.0, -0.5
    for name, key in FACADE:
        fixed = {"predict_property": np.float32([[1.0], [3.0]]), "y": np.float32([[2.0], [4.0]]), "distance": np.float32([0.5, 0.25]),
                 "label": np.array([1, 0])}
        s.model.result = dict(fixed) if key is not None else (dict(fixed), "artefact")
        got = getattr(s, name)("inputs", "second", batch_size=3)
        assert s.model.seen[-1] == (name, ("inputs", "second"), {"batch_size": 3}), name
        if key is None:
            assert got is s.model.result, name
            continue
        assert got is s.model.result and sorted(got) == sorted(fixed), name
        assert got[key].dtype == np.float32 or got[key].dtype == np.float64
        assert np.array_equal(got[key], fixed[key] * -0.5 + 2.0), name
        for k in fixed:
            assert k == key or got[k] is fixed[k], (name, k)


# ---- "a LatentIndex, or data to index for this call" ----

N = 6


def _targets():
    return np.arange(N, dtype=np.float32)


# the 12 methods: (HipModel method, the LatentIndex method it runs on the index, the call on ``data`` [and ``other`` data])
OWNED = (
    ("cluster", "cluster", lambda m, d, o: m.cluster(d, 2, level="structure")),
    ("choose_k", "choose_k", lambda m, d, o: m.choose_k(d, [2, 3], level="structure")),
    ("fit_projection", "pca", lambda m, d, o: m.fit_projection(d)),
    ("fit_embedding", "embed", lambda m, d, o: m.fit_embedding(d)),
    ("map_quality", "map_quality", lambda m, d, o: m.map_quality(d, np.zeros((N, 2), np.float32))),
    ("choose_perplexity", "choose_perplexity", lambda m, d, o: m.choose_perplexity(d, [5])),
    ("density_peaks", "density_peaks", lambda m, d, o: m.density_peaks(d, level="structure", k=2)),
    ("hierarchy", "hierarchy", lambda m, d, o: m.hierarchy(d, level="structure")),
    ("fit_head", "fit_head", lambda m, d, o: m.fit_head(d, _targets())),
    ("fit_kernel_head", "fit_kernel_head", lambda m, d, o: m.fit_kernel_head(d, _targets(), landmarks=2)),
    ("fit_class_head", "fit_class_head", lambda m, d, o: m.fit_class_head(d, np.arange(N) % 2, folds=2)),
    ("select_diverse", "select", lambda m, d, o: m.select_diverse(d, 2, reference=o)),
)
RESULT = {"cluster": {"centre": np.zeros((2, 128), np.float32)}, "choose_k": {"best": {"centre": np.zeros((2, 128), np.float32)}},
          "hierarchy": ({}, "hierarchy")}


def _setup(monkeypatch, inner, fail):
    from scann.models import LatentIndex

    cfg, inputs = tk._batch(N)
    other = dict(inputs)  # (the same structures as another object: select_diverse refuses the pool itself as the reference)
    m = tk._model(cfg)
    ran = []

    def stub(self, *args, **kwargs):
        ran.append(self)
        assert isinstance(self, LatentIndex) and self.model is m and len(self) == N
        if fail:
            raise RuntimeError("the analysis failed")
        return RESULT.get(inner, ("result", "artefact"))

    monkeypatch.setattr(LatentIndex, inner, stub)
    return m, inputs, other, ran


@pytest.mark.parametrize("method,inner,call", OWNED, ids=[o[0] for o in OWNED])
def test_an_index_built_for_the_call_is_freed(monkeypatch, method, inner, call):
    m, inputs, other, ran = _setup(monkeypatch, inner, fail=False)
    call(m, inputs, other)
    own = 2 if method == "select_diverse" else 1
    assert len(ran) == 1 and m.engine.created == own and m.engine.freed == own


@pytest.mark.parametrize("method,inner,call", OWNED, ids=[o[0] for o in OWNED])
def test_an_index_built_for_the_call_is_freed_on_an_error(monkeypatch, method, inner, call):
    m, inputs, other, ran = _setup(monkeypatch, inner, fail=True)
    with pytest.raises(RuntimeError, match="the analysis failed"):
        call(m, inputs, other)
    own = 2 if method == "select_diverse" else 1
    assert len(ran) == 1 and m.engine.created == own and m.engine.freed == own


@pytest.mark.parametrize("method,inner,call", OWNED, ids=[o[0] for o in OWNED])
def test_an_index_passed_in_is_never_freed(monkeypatch, method, inner, call):
    for fail in (False, True):
        m, inputs, other, ran = _setup(monkeypatch, inner, fail)
        ix, ref = m.build_index(inputs), m.build_index(other)
        if fail:
            with pytest.raises(RuntimeError, match="the analysis failed"):
                call(m, ix, ref)
        else:
            call(m, ix, ref)
        assert ran == [ix] and m.engine.created == 2 and m.engine.freed == 0


def test_select_diverse_frees_the_pool_when_the_reference_cannot_be_indexed(monkeypatch):
    """the second ``with`` fails on entry: the first index is still freed"""
    m, inputs, other, ran = _setup(monkeypatch, "select", fail=False)
    build = m.build_index

    def build_once(data, **kw):
        if data is other:
            raise RuntimeError("the reference cannot be indexed")
        return build(data, **kw)

    m.build_index = build_once
    with pytest.raises(RuntimeError, match="the reference cannot be indexed"):
        m.select_diverse(inputs, 2, reference=other)
    assert not ran and m.engine.created == 1 and m.engine.freed == 1


def test_the_level_in_force_and_the_flat_order():
    from scann.models import scann_model as sm

    cfg, inputs = tk._batch(3)
    m = tk._model(cfg)
    ix = m.build_index(inputs, level="atom")
    assert sm._level_of(ix, "structure") == "atom" and sm._level_of(inputs, "structure") == "structure"
    per = [np.float32([[1], [2]]), np.float32([[3]])]
    assert np.array_equal(sm._flat_per_structure(per, "atom", "targets", np.float32), np.float32([[1], [2], [3]]))
    assert np.array_equal(sm._flat_per_structure([np.array([1, 2]), np.array([0])], "atom", "labels"), [1, 2, 0])
    assert sm._flat_per_structure(per, "structure", "targets", np.float32) is per
    flat = np.float32([1, 2, 3])
    assert sm._flat_per_structure(flat, "atom", "targets", np.float32) is flat
    with pytest.raises(ValueError) as e:
        sm._flat_per_structure([np.float32([1, 2]), ["a"]], "atom", "targets", np.float32)
    assert str(e.value) == "targets must be a flat array in packed order or one array per structure"
    with pytest.raises(ValueError) as e:
        sm._expect("x", type(ix), "index")
    assert str(e.value) == "index must be a LatentIndex, got 'str'"
