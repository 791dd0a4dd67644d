"""Latent-space index: the learned representations of a set of structures kept on the GPU, searched for the nearest ones of a query.

The mean Euclidean distance of a structure's last hidden representation (``bf_property``) to its k nearest training structures is an
uncertainty / applicability-domain measure that needs one forward and no retraining (Janet, Duan, Yang, Nandy, Kulik, Chem. Sci. 2019);
at the atom level (``after_Lc``) the neighbours say which local structures of the training set an atom's environment resembles.  The rows
stay on the device (scann_index_*, include/scann_hip.h); the search is exact, in the difference form, under the total order (distance,
then position), so a query's answer depends on the query and the index contents only."""
from __future__ import annotations

import functools
import math

import numpy as np

from .. import _hip

LEVELS = ("structure", "atom")


def level_dim(config, level):
    """Width of the rows of ``level`` in a model configuration: dense_out (structure, ``bf_property``) or global_dim (atom, ``after_Lc``);
    ValueError for another level."""
    if level not in LEVELS:
        raise ValueError("level must be one of %s, got %r" % (", ".join(LEVELS), level))
    return int(config["model"]["dense_out" if level == "structure" else "global_dim"])


def batch_jobs(model, data, bs, upload_padded=None):
    """(upload, n_struct) per chunk of ``data``: a padded dict or a ``PackedBatch`` cut ``bs`` structures at a time, or a dataset -- any
    sequence of ``(PackedBatch | padded dict, target)`` -- batch by batch.  THE chunker of every batched call (HipModel._run_chunks).
    ``upload_padded``: what uploads a padded chunk (default: the model's own choice of packer, HipModel._upload_padded)."""
    eng = model.engine
    upload_padded = upload_padded or model._upload_padded
    if isinstance(data, _hip.PackedBatch):
        B = data.n_struct
        for i in range(0, B, bs):
            yield functools.partial(eng.upload, _hip.slice_packed(data, i, min(i + bs, B))), min(i + bs, B) - i
    elif isinstance(data, dict):
        B = int(np.shape(data["neighbors"])[0])
        sliced = {k: np.asarray(v) for k, v in data.items() if k in model.input_names}
        for i in range(0, B, bs):
            yield functools.partial(upload_padded, {k: v[i:i + bs] for k, v in sliced.items()}), min(i + bs, B) - i
    else:
        for i in range(len(data)):
            item, _ = data[i]
            if isinstance(item, _hip.PackedBatch):
                yield functools.partial(eng.upload, item), item.n_struct
            else:
                yield functools.partial(upload_padded, item), int(np.shape(item["neighbors"])[0])


def count_structures(data):
    if isinstance(data, _hip.PackedBatch):
        return data.n_struct
    if isinstance(data, dict):
        return int(np.shape(data["neighbors"])[0])
    n = 0
    for i in range(len(data)):
        item, _ = data[i]
        n += item.n_struct if isinstance(item, _hip.PackedBatch) else int(np.shape(item["neighbors"])[0])
    return n


def stop_dist2_of(stop_distance):
    """``stop_distance`` of a selection as the squared fp32 threshold the C call takes (None: 0, no threshold); ValueError for a
    negative or NaN one."""
    if stop_distance is None:
        return 0.0
    try:
        stop = float(stop_distance)
    except (TypeError, ValueError):
        raise ValueError("stop_distance must be None or a number >= 0, got %r" % (stop_distance,)) from None
    if not stop >= 0.0:
        raise ValueError("stop_distance must be None or a number >= 0, got %r" % (stop_distance,))
    return float(np.float32(stop) * np.float32(stop))


def radius2_of(radius):
    """``radius`` of a radius search as the squared fp32 threshold the C calls take, squared in fp32 the way ``stop_dist2_of`` does it
    (inf stays inf); ValueError for a negative or NaN one or for no number."""
    try:
        r = float(radius)
    except (TypeError, ValueError):
        raise ValueError("radius must be a number >= 0, got %r" % (radius,)) from None
    if isinstance(radius, bool) or not r >= 0.0:
        raise ValueError("radius must be a number >= 0, got %r" % (radius,))
    return float(np.float32(r) * np.float32(r))


def within_result(r, count_only):
    """What ``LatentIndex.within`` returns, from the engine's dict of a radius search"""
    out = {"count": r["count"], "first": r["first"]}
    if not count_only:
        out.update({"position": r["position"], "id": r["id"], "atom": r["atom"], "dist2": r["dist2"],
                    "distance": np.sqrt(r["dist2"])})  # (correctly rounded on the host, as nearest reports distances)
    return out


def duplicates_chunk_arg(chunk):
    """``chunk`` of ``LatentIndex.duplicates``: the rows of one self-join call, an integer >= 1; ValueError otherwise"""
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or int(chunk) < 1:
        raise ValueError("chunk must be an integer >= 1, got %r" % (chunk,))
    return int(chunk)


def duplicate_groups(i, j, dist2, n_rows):
    """``LatentIndex.duplicates``' dict from the pairs (i < j) of a self-join over ``n_rows`` rows.  The components come from a union-find
    written with arrays: every pair hooks the greater of its two roots to the lesser, then every row's pointer is shortened to its
    root, until no pair joins two roots; a root is therefore always its component's least position."""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    group = np.arange(n_rows, dtype=np.int64)
    while len(i):
        gi, gj = group[i], group[j]
        if np.array_equal(gi, gj):
            break
        np.minimum.at(group, np.maximum(gi, gj), np.minimum(gi, gj))
        while True:
            up = group[group]
            if np.array_equal(up, group):
                break
            group = up
    roots, sizes = np.unique(group, return_counts=True)
    return {"pairs": np.stack([i, j], axis=1).astype(np.int32).reshape(-1, 2), "distance": np.sqrt(np.asarray(dist2, np.float32)),
            "group": group.astype(np.int32), "n_groups": int(len(roots)), "sizes": sizes.astype(np.int64),
            "keep": group == np.arange(n_rows)}


def explained_ratio(w):
    """The share of every eigenvalue in the total variance, fp64: negative eigenvalues (rounding noise of a rank-deficient covariance)
    count as 0, and the divisor is the fp64 sum of the others times 1 + (d + 2) * 2^-52 = 1 + (2 d + 4) * 2^-53.  The d - 1 adds of that
    sum, a quotient, and the d - 1 adds of a sum of the ratios each err by at most 2^-53 relative, fewer than 2 d roundings along any
    path, so with that divisor the ratios, or any part of them, sum to at most 1 in fp64 whatever the order of the adds; dividing by
    one number keeps them non-increasing.  All zeros if no eigenvalue is positive."""
    w = np.maximum(np.asarray(w, dtype=np.float64), 0.0)
    total = float(w.sum())
    if not total > 0.0:
        return np.zeros(len(w))
    return w / (total * (1.0 + (len(w) + 2) * 2.0 ** -52))


def width_mismatch(noun, level, dim, config, path=None):
    """THE message for rows of ``level`` and ``dim`` columns that are not ``config``'s, ``path``: in front for a file"""
    return "%sa %s-level %s of %d columns does not fit a model whose %s is %d" % (
        "" if path is None else "%s: " % (path,), level, noun, dim, "dense_out" if level == "structure" else "global_dim",
        level_dim(config, level) if level in LEVELS else -1)


# how a scalar field of a saved result is boxed for np.savez and unboxed for the constructor
AS_FLOAT = (np.array, float)
AS_FLOAT32 = (lambda v: np.array(v, dtype=np.float32), float)
AS_INT = (lambda v: np.array(v, dtype=np.int64), int)
AS_NAMES = (lambda v: np.array(v, dtype=np.str_), lambda a: [str(x) for x in a])


def saved_fields(*fields, of=""):
    """A saved result's FIELDS from a declaration: "key" for an array attribute saved as it is, ("key", AS_...) for a scalar;
    ``of``: the attribute that holds them ("head." for an inner head's).  -> ((key, attribute path, box, unbox), ...)"""
    return tuple((f, of + f, None, None) if isinstance(f, str) else (f[0], of + f[0]) + f[1] for f in fields)


class SavedResult:
    """What the results a fit leaves behind share: they belong to one ``level`` of a model and to rows of ``dim`` columns, fit every
    model whose level has that width, and are saved as one ``.npz`` without pickle.  A subclass declares ``NOUN`` (what the mismatch
    message calls it), ``FIELDS`` (``saved_fields``, in the order of its constructor's arguments; ``level`` and ``dim`` follow them),
    and where it differs: ``KIND`` (a tag the file carries and ``load`` demands), ``saved_fits`` (a further check of a loaded file
    against ``dim``) and ``from_saved`` (a constructor that takes the fields in another order)."""
    NOUN, FIELDS, KIND = None, (), None

    def check_model(self, model):
        """ValueError unless the result has the width of ``model``'s level"""
        if level_dim(model.config, self.level) != self.dim:
            raise ValueError(width_mismatch(self.NOUN, self.level, self.dim, model.config))

    def save(self, path):
        """An ``.npz`` of the fields, level and dim (written to exactly ``path``; no pickle)."""
        out = {}
        for key, attr, box, _ in self.FIELDS:
            v = functools.reduce(getattr, attr.split("."), self)
            out[key] = v if box is None else box(v)
        out.update(level=np.array(self.level), dim=np.array(self.dim, dtype=np.int64))
        if self.KIND is not None:
            out["kind"] = np.array(self.KIND)
        with open(path, "wb") as f:
            np.savez(f, **out)

    @classmethod
    def load(cls, model, path):
        """The saved result; ValueError if the file is of another kind, or if its level's width is not this model's."""
        with np.load(path, allow_pickle=False) as z:
            if cls.KIND is not None and ("kind" not in z.files or str(z["kind"]) != cls.KIND):
                raise ValueError("%s: not a saved %s" % (path, cls.__name__))
            level, dim = str(z["level"]), int(z["dim"])
            v = {key: z[key] if unbox is None else unbox(z[key]) for key, _, _, unbox in cls.FIELDS}
        if level not in LEVELS or level_dim(model.config, level) != dim or not cls.saved_fits(v, dim):
            raise ValueError(width_mismatch(cls.NOUN, level, dim, model.config, path))
        return cls.from_saved(v, level, dim)

    @classmethod
    def saved_fits(cls, v, dim):
        return True

    @classmethod
    def from_saved(cls, v, level, dim):
        return cls(*v.values(), level, dim)


def auto_cells(n_rows):
    """The cells ``LatentIndex.partition(cells="auto")`` asks for: one per 2,048 rows, at most 1,024 -- about 32 tiles to a cell, so that
    the centre distances (cells / rows of a full search) and the pad entries (at most one tile per cell) both stay near 1/2048 of the index."""
    return min(_hip.KMEANS_MAX_K, max(1, int(n_rows) // 2048))


class LatentIndex:
    """Rows of one level of one model on its GPU.  ``level``: "structure" (one ``bf_property`` row per structure) or "atom" (one
    ``after_Lc`` row per real atom).  Every row carries the id of its structure and, at atom level, the atom's index within it."""

    def __init__(self, model, level="structure"):
        self.dim = level_dim(model.config, level)
        self.level = level
        self.model = model
        self._ix = model.engine.index_create(self.dim)
        self._n_struct = 0  # structures given so far: where the default ids of the next add start

    def check_model(self, model):
        """ValueError unless the index lives on ``model``'s GPU handle and holds rows of its level's width"""
        if self.model is not model or level_dim(model.config, self.level) != self.dim:
            raise ValueError("the index was built for another model: it lives on that model's GPU handle (%s level, %d columns)" % (
                self.level, self.dim))

    def __len__(self):
        return len(self._ix)

    def add(self, data, ids=None, batch_size=None):
        """Append the rows of ``data`` -- a padded dict, a ``PackedBatch`` or a dataset as ``predict_dataset`` takes it -- computed by one
        forward per batch and copied device to device.  ``ids``: one per structure (default: continuing from the structures the index
        was given so far, i.e. 0 .. n-1 for a fresh one).  Returns self."""
        n = count_structures(data)
        if ids is None:
            ids = np.arange(n, dtype=np.int64) + self._n_struct
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if ids.shape[0] != n:
            raise ValueError("%d structures need %d ids, got %d" % (n, n, ids.shape[0]))
        eng, lvl = self.model.engine, _hip.KNN_LEVELS[self.level]
        self.model._run_chunks(data, batch_size, lambda rb, s0, s1: eng.index_add_batch(self._ix, rb, lvl, ids[s0:s1]))
        self._n_struct += n
        return self

    def add_rows(self, rows, ids=None, atoms=None):
        """Append host rows [n, dim] with their ids (default: their positions) and atoms (default: -1)."""
        self.model.engine.index_add(self._ix, rows, ids, atoms)
        return self

    def rows(self):
        """(rows [n, dim] fp32, ids [n] int64, atoms [n] int32) copied back from the device, in insertion order."""
        return self.model.engine.index_read(self._ix)

    def names(self):
        """(ids [n] int64, atoms [n] int32) of every row, from the host copies the index keeps: nothing is read from the device."""
        return self.model.engine.index_names(self._ix)

    def segments(self):
        """(first int64, count int32, id int64) of the index's segments -- its maximal runs of consecutive rows with one id, i.e. the
        structures of an atom-level index, numbered in position order -- from the host copies the index keeps."""
        return self.model.engine.index_segments(self._ix)

    def partition(self, cells="auto", max_iter=8):
        """Partition the index into cells so that every nearest-row search over it -- ``nearest``, ``place``, ``attach``, the reference
        pass of ``select``, the neighbour graph under ``embed``, ``density_peaks``, ``hierarchy`` and ``map_quality`` -- skips the cells
        out of reach (scann_index_partition).  The answers stay the brute-force answers in every byte; the cell-ordered copy doubles the
        index's device memory, and adding rows drops it.  ``cells``: 1 .. _hip.KMEANS_MAX_K, or "auto" = ``auto_cells(len(self))``;
        ``max_iter``: Lloyd rounds that refine the farthest-point centres.  Returns {"cells": cells in use, "tiles": 64-row tiles of the
        copy, "pad": its pad entries, "largest": rows of the largest cell, "pad_share": pad / (64 tiles)}."""
        if isinstance(cells, str):
            if cells != "auto":
                raise ValueError('cells must be "auto" or an integer in 1 .. %d, got %r' % (_hip.KMEANS_MAX_K, cells))
            cells = auto_cells(len(self))
        cells, max_iter = _hip.check_cells_args(cells, max_iter)
        info = self.model.engine.index_partition(self._ix, cells, max_iter)
        info["pad_share"] = info["pad"] / (64.0 * info["tiles"]) if info["tiles"] else 0.0
        return info

    def drop_partition(self):
        """Free the partition, if there is one: searches compare every row again.  Returns self."""
        self.model.engine.index_partition(self._ix, 0, 0)
        return self

    def partition_args(self):
        """(cells, max_iter) the partition was built with, or None without one, as the index itself knows them
        (scann_index_partition_args).  An engine that has no such call -- the CPU stand-ins of the tests, never ``Engine`` -- has no
        partitions."""
        ask = getattr(self.model.engine, "index_partition_args", None)
        cells, max_iter = ask(self._ix) if ask else (0, 0)
        return (cells, max_iter) if cells else None

    def search_stats(self):
        """The last search over this index: {"total": (128-query group, 64-row tile) pairs a full search visits, "seeds", "visited",
        "groups", "visited_share": visited / total}; without a partition visited == total."""
        st = self.model.engine.index_search_stats(self._ix)
        st["visited_share"] = st["visited"] / st["total"] if st["total"] else 1.0
        return st

    def within(self, rows, radius, exclude_ids=None, max_pairs=1 << 24, count_only=False):
        """Which rows of this index lie within Euclidean distance ``radius`` of every host query vector of ``rows`` [nq, dim]: the exact
        radius search on the GPU (scann_index_within).  Where ``nearest`` always answers k rows, this answers as many as there are,
        possibly none: the ball count of a prediction, or whether a test structure has a training twin.  ``radius`` is squared in fp32
        and compared with the fp32 distance chain, inclusively; ``np.inf`` is allowed.  ``exclude_ids`` [nq]: rows whose id equals the
        query's are skipped.  Returns {"count" int64 [nq], "first" int64 [nq + 1], "position" int32, "id" int64, "atom" int32, "dist2",
        "distance" fp32 [total]}: query i's hits are entries first[i] .. first[i + 1] - 1, in the order (distance, position), so the
        result depends on the queries, the index and the radius only, in every byte.  ``count_only``: counts and "first" alone, nothing
        else is allocated.  More than ``max_pairs`` hits in all, or bad arguments, raise ValueError."""
        r2 = radius2_of(radius)
        _hip.check_within_args(r2, max_pairs)
        r = self.model.engine.index_within(self._ix, rows, r2, query_ids=exclude_ids, max_pairs=max_pairs, count_only=count_only)
        return within_result(r, count_only)

    def duplicates(self, radius, max_pairs=1 << 24, chunk=65536, route="device"):
        """The near-duplicate groups of this index: every unordered pair of rows within Euclidean distance ``radius`` (the self-join of
        scann_index_within_rows with ``upper`` = 1, ``chunk`` rows at a time, each pair listed once) and the connected components of
        those pairs, by a union-find on the host.  Returns {"pairs" int32 [P, 2] (i < j, ordered by i, then distance, then j),
        "distance" fp32 [P], "group" int32 [N] -- the least position of the row's component; a row without a partner is its own group --,
        "n_groups", "sizes" int64 [n_groups] (by ascending group), "keep" bool [N] -- true at each group's least position: the dedup
        mask}.  ``route`` "host" runs the host twin on the rows read back: the same bytes.  More than ``max_pairs`` pairs, or bad
        arguments, raise ValueError."""
        r2 = radius2_of(radius)
        _, max_pairs, _ = _hip.check_within_args(r2, max_pairs)
        chunk = duplicates_chunk_arg(chunk)
        if route not in ("device", "host"):
            raise ValueError('route must be "device" or "host", got %r' % (route,))
        eng, N = self.model.engine, len(self)
        host_rows = self.rows()[0] if route == "host" and N else None
        pi, pj, pd, found = [], [], [], 0
        for first in range(0, N, chunk):
            n = min(chunk, N - first)
            if route == "host":
                r = _hip.within_host(host_rows, host_rows[first:first + n], r2, query_pos=np.arange(first, first + n, dtype=np.int32), upper=1,
                                     max_pairs=max_pairs - found)
            else:
                r = eng.index_within_rows(self._ix, first, n, r2, upper=1, max_pairs=max_pairs - found)
            found += r["total"]
            pi.append(np.repeat(np.arange(first, first + n, dtype=np.int32), r["count"]))
            pj.append(r["position"])
            pd.append(r["dist2"])
        return duplicate_groups(np.concatenate(pi) if pi else np.zeros(0, np.int32), np.concatenate(pj) if pj else np.zeros(0, np.int32),
                                np.concatenate(pd) if pd else np.zeros(0, np.float32), N)

    def save(self, path):
        """An ``.npz`` of rows, ids, atoms, level and dim (written to exactly ``path``), and of the partition's arguments if the index
        has one: the build is deterministic, so ``load`` rebuilds the same layout."""
        rows, ids, atoms = self.rows()
        part = self.partition_args()
        extra = {"partition": np.array(part, dtype=np.int64)} if part else {}
        with open(path, "wb") as f:
            np.savez(f, rows=rows, ids=ids, atoms=atoms, level=np.array(self.level), dim=np.array(self.dim, dtype=np.int64), **extra)

    @classmethod
    def load(cls, model, path):
        """The saved index uploaded to ``model``'s GPU; ValueError if its level's width is not this model's."""
        with np.load(path, allow_pickle=False) as z:
            level, dim = str(z["level"]), int(z["dim"])
            rows, ids, atoms = z["rows"], z["ids"], z["atoms"]
            part = tuple(int(v) for v in z["partition"]) if "partition" in z.files else (0, 0)
        if level_dim(model.config, level) != dim or rows.ndim != 2 or rows.shape[1] != dim:
            raise ValueError(width_mismatch("index", level, dim, model.config, path))
        ix = cls(model, level)
        if len(rows):
            ix.add_rows(rows, ids, atoms)
        ix._n_struct = int(ids.max()) + 1 if len(ids) else 0  # default ids of later adds do not collide
        if part[0] and len(rows):
            ix.partition(part[0], part[1])
        return ix

    def select(self, m, reference=None, stop_distance=None):
        """The ``m`` most diverse rows of this index by greedy k-center (farthest-point) selection on the GPU: repeatedly the row whose
        distance to every row of ``reference`` (a ``LatentIndex`` of the same model, level and width; None: nothing is labelled yet) and
        to every row already taken is largest, ties to the earlier position; rows with a non-finite component are never taken.
        ``stop_distance``: selection ends before the first pick nearer than this to what is covered already (None: no threshold).
        Returns {"position" int32, "neighbor_id" int64 (the structure ids), "atom" int32, "radius" fp32 -- the covering radius at each
        pick, non-increasing, ``inf`` for a first pick without a reference --, "count"}, every array cut to the picks made.  A bad ``m``,
        a negative or NaN ``stop_distance`` or an unfit reference raise ValueError before any device call."""
        m, _ = _hip.check_select_args(m, 0.0)
        stop2 = stop_dist2_of(stop_distance)
        if reference is not None:
            if reference is self:
                raise ValueError("the reference is the pool itself: every row would be at distance 0")
            if not isinstance(reference, LatentIndex):
                raise ValueError("reference must be a LatentIndex or None, got %r" % (type(reference).__name__,))
            if reference.model is not self.model or reference.level != self.level or reference.dim != self.dim:
                raise ValueError("the reference is a %s-level index of %d columns%s, the pool a %s-level index of %d" % (
                    reference.level, reference.dim, "" if reference.model is self.model else " of another model", self.level, self.dim))
        r = self.model.engine.index_select(self._ix, None if reference is None else reference._ix, m, stop2)
        n = int(r["count"])
        return {"position": r["position"][:n], "neighbor_id": r["id"][:n], "atom": r["atom"][:n],
                "radius": np.sqrt(r["radius2"][:n]), "count": n}  # (correctly rounded on the host, as nearest reports distances)

    def cluster(self, k, init="kcenter", max_iter=50, stop_changed=0):
        """k-means over the rows of this index on the GPU (scann_index_kmeans): which kinds of row the model distinguishes, and which
        kind each row is.  The result depends on the index contents and the initial centres only, bit for bit.  ``init``: "kcenter" --
        the rows ``self.select(k)`` picks, a deterministic farthest-point seeding; ValueError if fewer than ``k`` rows are eligible --,
        an integer array of ``k`` positions in the index, or a finite float array [k, dim].  The loop ends when at most ``stop_changed``
        rows changed their label or after ``max_iter`` updates; rows with a non-finite component get label -1 and count for nothing.
        Returns {"label" int32 [N], "distance" fp32 [N] (to the row's centre; inf for label -1), "centre" fp32 [k, dim], "size" int64
        [k], "n_iter", "converged", "inertia" (the fp64 sum of the squared distances of the labelled rows), "medoid_position" int32,
        "medoid_id" int64, "medoid_atom" int32 [k]: per cluster its member row nearest the centre, ties to the earlier position, -1 for
        an empty cluster -- the cluster explained by an example}.  Bad arguments raise ValueError before any device call."""
        k, max_iter, stop_changed = _hip.check_kmeans_args(k, max_iter, stop_changed)
        eng = self.model.engine
        if isinstance(init, str):
            if init != "kcenter":
                raise ValueError('init must be "kcenter", %d positions or an array [%d, %d], got %r' % (k, k, self.dim, init))
            picks = eng.index_select(self._ix, None, k, 0.0)
            if picks["count"] < k:
                raise ValueError("k = %d clusters need %d rows without a non-finite component, the index has %d" % (k, k, picks["count"]))
            init = picks["position"]
        else:
            a = np.asarray(init)
            if a.dtype.kind in "iu" and a.ndim == 1:
                if a.shape[0] != k or (k and (a.min() < 0 or a.max() >= len(self))):
                    raise ValueError("init must name %d positions in 0 .. %d, got %d of them in %s .. %s" % (
                        k, len(self) - 1, a.shape[0], a.min() if a.size else "-", a.max() if a.size else "-"))
                init = a
            else:
                init = _hip.check_kmeans_init(init, self.dim)
                if init.shape[0] != k:
                    raise ValueError("init holds %d centres, k is %d" % (init.shape[0], k))
        r = eng.index_kmeans(self._ix, init, max_iter, stop_changed)
        ids, atoms = eng.index_names(self._ix)  # (host copies: the rows stay on the device)
        return cluster_result(r, ids, atoms, k)

    def silhouette(self, labels, sample=None, seed=0, metric="euclidean", route="device", table=False, n_clusters=None):
        """How good a labelling of this index's rows is, row by row and as a whole: the silhouette (Rousseeuw 1987).  For a row, ``a`` is
        its mean distance to the other rows of its own cluster and ``b`` the least mean distance to the rows of any other cluster;
        s = (b - a) / max(a, b) lies in [-1, 1], near 1 for a row well inside its cluster, near 0 for a row between two, and ``other``
        names the second one.  Every mean is over all rows of the index, from one exact pass over all pairs on the GPU
        (scann_index_silhouette), defined to the bit, so the result depends on the index contents and the arguments only.
        ``labels``: an integer array [N], -1 for noise or unlabelled -- ``cluster(k)["label"]``, ``density_peaks(...)[0]["label"]``, the
        labels of ``LatentHierarchy.clusters()``; at most 1024 clusters (``n_clusters``: their number, default the largest label + 1).
        A row counts if it has a label >= 0 and no non-finite component.  ``sample``: None -- every row --, an integer m -- m counting
        positions drawn without replacement by ``np.random.default_rng(seed)``, then sorted: the sampled rows' values are exact, only
        the mean is sampled --, or an array of positions.  ``metric``: "euclidean" or "sqeuclidean".  ``route`` "host" runs the host
        twin on the rows read back: the same bits.  Returns {"position" int32 [n], "silhouette", "a", "b" fp64 [n] (silhouette 0 for the
        row of a one-row cluster and where a and b are both 0; NaN where the row does not count or there is no other cluster), "other"
        int32 [n], "size" int64 [C] (the counting rows per cluster), "score" (the fp64 mean of the finite silhouettes, positions
        ascending; NaN without any), "cluster_score" fp64 [C], "shift" (of the pass's fixed point, chosen from the index's column
        ranges: ``silhouette_shift``), "metric", and with ``table`` "sums" int64 [n, C]}.  Bad arguments raise ValueError before any
        device call."""
        eng = self.model.engine
        route = silhouette_route(route)
        if route == "host":
            return silhouette_rows_host(self.rows()[0], labels, sample=sample, seed=seed, metric=metric, table=table, n_clusters=n_clusters)
        labels, C_, _, _, _ = _hip.check_silhouette_args(labels, len(self), n_clusters, None, metric, 0)
        sample = silhouette_sample_arg(sample, seed, len(self))

        def moments():
            try:
                return eng.index_moments(self._ix)
            except _hip.ScannHipError:
                return None  # fewer than two rows without a non-finite component: no pair, no term

        def counting():
            labelled = labels >= 0
            size = eng.index_silhouette(self._ix, labels, C_, np.zeros(0, np.int32), metric, 0)["count"]
            if int(size.sum()) == int(labelled.sum()):
                return labelled  # (the usual case: nothing is read back)
            return labelled & np.isfinite(self.rows()[0]).all(axis=1)

        return silhouette_run(lambda q, shift: eng.index_silhouette(self._ix, labels, C_, q, metric, shift, table), moments, counting,
                              labels, C_, sample, seed, metric)

    @staticmethod
    def cluster_scores(result):
        """``cluster_scores(result)`` of this module: the Calinski-Harabasz and the Davies-Bouldin index of a ``cluster`` result."""
        return cluster_scores(result)

    def choose_k(self, ks, sample=None, seed=0, metric="euclidean", route="device", **cluster_args):
        """How many kinds of row the model distinguishes: ``cluster(k, **cluster_args)`` and ``silhouette`` of its labels for every k
        of ``ks``, and the k with the highest silhouette score, ties to the smaller k.  ``sample``, ``seed``, ``metric``: as
        ``silhouette`` takes them (an integer sample is drawn anew, with the same seed, among each clustering's counting rows).
        ``route`` "host" runs the host twins of both on the rows read back: the same bits.  Returns {"k" int64 [n_k] (ascending, each
        once), "score", "inertia", "calinski_harabasz", "davies_bouldin" fp64 [n_k], "n_iter" int64 [n_k], "converged" bool [n_k],
        "size" (a list of int64 arrays), "best_k", "best" (the best k's ``cluster`` result) and "silhouette" (its ``silhouette``
        result)}.  Bad arguments raise ValueError before any device call."""
        ks = choose_k_arg(ks)
        route = silhouette_route(route)
        if route == "host":
            rows = self.rows()[0]
            ids, atoms = self.names()
            return choose_k_run(lambda k: cluster_rows_host(rows, k, ids=ids, atoms=atoms, **cluster_args),
                                lambda lab, k: silhouette_rows_host(rows, lab, sample=sample, seed=seed, metric=metric, n_clusters=k), ks)
        _hip.check_silhouette_args(np.zeros(len(self), np.int32), len(self), None, None, metric, 0)
        silhouette_sample_arg(sample, seed, len(self))
        return choose_k_run(lambda k: self.cluster(k, **cluster_args),
                            lambda lab, k: self.silhouette(lab, sample=sample, seed=seed, metric=metric, n_clusters=k), ks)

    def pca(self, m=None):
        """The principal-component map of this index's rows, mean and covariance computed on the GPU (scann_index_moments) and
        bit-reproducible: they depend on the index contents only.  Rows with a non-finite component count for nothing.  The covariance
        is decomposed on the host (``_hip.sym_eig``: cyclic Jacobi, fp64) and the rows are projected on the device onto the ``m``
        leading components (None: all ``dim``).  Returns ``(result, projection)``: {"mean" fp32 [dim], "components" fp32 [m, dim],
        "variance" fp64 [m] (the eigenvalues, descending), "explained_variance_ratio" fp64 [m] (``explained_ratio``: each eigenvalue,
        negative ones as 0, over the sum of them all, the divisor rounded up so that the ratios are non-increasing and their fp64 sum
        never exceeds 1), "total_variance" (the trace), "rank" (eigenvalues above the noise floor of the integer moments), "noise_floor", "n_rows" (the
        rows that counted), "coordinates" fp32 [N, m], "mahalanobis" fp32 [N] (over the ``m`` components; those at or below the noise
        floor are left out), "distance_to_mean" fp32 [N]} -- NaN for every row whose distance to the mean is not finite, as it is for a
        row with a non-finite component -- and the ``LatentProjection`` that ``HipModel.project`` takes.  A bad ``m`` raises ValueError
        before any device call; so do fewer than 2 usable rows."""
        m = self.dim if m is None else m
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= int(m) <= self.dim:
            raise ValueError("m must be an integer in 1 .. %d, got %r" % (self.dim, m))
        m = int(m)
        if len(self) < 2:
            raise ValueError("a covariance needs at least 2 rows, the index has %d" % len(self))
        eng = self.model.engine
        try:
            mo = eng.index_moments(self._ix)
        except _hip.ScannHipError as e:
            if e.code == -1:
                raise ValueError(str(e)) from None
            raise
        w, v, _ = _hip.sym_eig(mo["cov"])
        noise = float(self.dim) * 2.0 ** (2 * int(mo["col_exp"].max()) - mo["bits"] + 2)
        total = float(np.trace(mo["cov"]))
        proj = LatentProjection(mo["mean"], v[:m].astype(np.float32), w[:m], noise, self.level, self.dim)
        out = self.project(proj)
        out.update({"mean": proj.mean, "components": proj.components, "variance": proj.variance, "total_variance": total,
                    "explained_variance_ratio": explained_ratio(w)[:m], "rank": int((w > noise).sum()),
                    "noise_floor": noise, "n_rows": mo["n"]})
        return out, proj

    def project(self, projection):
        """This index's own rows through a ``LatentProjection``, on the device where they lie (scann_index_project): {"coordinates" fp32
        [N, m], "mahalanobis" fp32 [N], "distance_to_mean" fp32 [N]}; NaN for every row whose distance to the mean is not finite."""
        if not isinstance(projection, LatentProjection):
            raise ValueError("projection must be a LatentProjection, got %r" % (type(projection).__name__,))
        if projection.level != self.level or projection.dim != self.dim:
            raise ValueError("a %s-level projection of %d columns does not fit a %s-level index of %d" % (
                projection.level, projection.dim, self.level, self.dim))
        r = self.model.engine.index_project(self._ix, projection.mean, projection.components, projection.scale)
        return projection.finish(r)

    def fit_head(self, targets, l2="loo", names=None):
        """A linear readout head for ``targets`` ([N] or [N, K], K <= 16, one row per row of this index; NaN: unlabelled) on the frozen
        rows: ridge regression in the principal axes of the rows, the strength chosen per target by exact leave-one-out.  The moments of
        [rows | targets] (scann_index_fit_moments) and the leave-one-out residuals of every row at every strength
        (scann_index_ridge_loo) are computed on the GPU and depend on the index contents and the targets only, bit for bit; the X-X
        covariance is decomposed on the host (``_hip.sym_eig``).  Components at or below the noise floor of the integer moments
        (``pca``'s) are left out.  ``l2``: "loo" -- the grid max(s_0 10^(-l/2), noise floor), l = 0 .. 16, s_0 the largest eigenvalue --,
        one number, or a sequence of at most 32.  Per target the strength with the least leave-one-out sum of squares wins, ties to
        the larger.  Returns ``(result, head)``: {"l2" [K], "loo_rmse", "loo_mae", "loo_r2", "fit_rmse", "dof", "sigma2" [K],
        "n_rows", "loo_prediction" fp32 [N, K] (t - r; NaN for rows that do not count), "weights" fp32 [K, dim], "names", "path":
        {"l2" [L], "loo_rmse" [L, K], "dof" [L]}} and the ``LatentHead`` that ``HipModel.predict_head`` takes.  Bad arguments raise
        ValueError before any device call; so do fewer than 3 usable rows and a covariance without a component above the noise floor."""
        t = _hip.check_head_targets(targets, len(self))
        K = t.shape[1]
        names = ["target_%d" % k for k in range(K)] if names is None else [str(x) for x in names]
        if len(names) != K:
            raise ValueError("names: %d for %d targets" % (len(names), K))
        grid = head_grid(l2)
        if len(self) < 3:
            raise ValueError("a head needs at least 3 rows, the index has %d" % len(self))
        eng, dim = self.model.engine, self.dim
        try:
            mo = eng.index_fit_moments(self._ix, t)
        except _hip.ScannHipError as e:
            if e.code == -1:
                raise ValueError(str(e)) from None
            raise
        fit = head_closed_form(mo, dim, grid)
        n = fit["n"]
        first = eng.index_ridge_loo(self._ix, t, fit["mean"], fit["tmean"], fit["components"], fit["scale"], fit["coef"], fit["lev0"])
        pick = head_pick(first["sse"], fit["l2"])
        second = eng.index_ridge_loo(self._ix, t, fit["mean"], fit["tmean"], fit["components"], fit["scale"], fit["coef"], fit["lev0"], pick)
        return head_result(fit, second, pick, t, names, self.level, dim)

    def fit_kernel_head(self, targets, landmarks=256, bandwidth="loo", l2="loo", names=None):
        """A nonlinear readout head for ``targets`` (as ``fit_head`` takes them) on the frozen rows: ridge regression on the Gaussian
        features phi_c(x) = exp(-|x - z_c|^2 / 2 h^2) to m landmarks -- kernel ridge regression with a fixed basis, i.e. sparse Gaussian
        process regression --, the features computed on the GPU (scann_index_rbf_features) into a temporary index on which exactly
        ``fit_head``'s sequence runs.  ``landmarks``: a count m (the first m picks of ``select(m + 1)``; the next pick's radius is their
        covering radius R) or an integer array of positions in the index (R: the largest distance of a row to them).  ``bandwidth``:
        "loo" -- h^2 = R^2 {1, 2, 4, 8, 16, 32} --, one positive distance h or a sequence of at most 8.  The bandwidth with the least
        sum over the targets of leave-one-out sse / total sum of squares wins (targets without variance skipped), ties to the larger
        h; one bandwidth serves all targets, the ridge strength stays per target (``l2`` as in ``fit_head``).  Returns ``(result,
        head)``: ``fit_head``'s keys with "weights" [K, m] over the features, "bandwidth", "landmark_position", "landmark_id",
        "landmark_atom", "covering_radius", "bandwidth_path": {"bandwidth" [G], "loo_rmse", "loo_r2" [G, K]}, and the
        ``LatentKernelHead`` that ``HipModel.predict_kernel_head`` takes.  Bad arguments raise ValueError before any device call; so
        do fewer usable rows than landmarks + 1 and a covering radius of 0, before any feature pass."""
        t = _hip.check_head_targets(targets, len(self))
        K = t.shape[1]
        names = ["target_%d" % k for k in range(K)] if names is None else [str(x) for x in names]
        if len(names) != K:
            raise ValueError("names: %d for %d targets" % (len(names), K))
        grid = head_grid(l2)
        m, positions = kernel_landmarks_arg(landmarks, len(self))
        kernel_bandwidth_arg(bandwidth)
        if len(self) < 3:
            raise ValueError("a head needs at least 3 rows, the index has %d" % len(self))
        eng = self.model.engine
        if positions is None:
            sel = eng.index_select(self._ix, None, m + 1, 0.0)
            if sel["count"] < m + 1:
                raise ValueError("a kernel head needs more usable rows than landmarks: %d landmarks, %d rows without a non-finite component" % (
                    m, sel["count"]))
            positions, R2 = sel["position"][:m].copy(), float(sel["radius2"][m])
            Z = np.concatenate([eng.index_read(self._ix, int(p), 1)[0] for p in positions])
        else:
            Z = np.concatenate([eng.index_read(self._ix, int(p), 1)[0] for p in positions])
            _hip.check_rbf_args(Z, 1.0, self.dim)  # (a landmark must be a finite row)
            ref = eng.index_create(self.dim)
            try:
                eng.index_add(ref, Z)
                sel = eng.index_select(self._ix, ref, 1, 0.0)
            finally:
                ref.free()
            R2 = float(sel["radius2"][0]) if sel["count"] >= 1 else 0.0
        hs = kernel_bandwidths(bandwidth, R2)
        ids, atoms = eng.index_names(self._ix)

        def run(gamma):
            feat = eng.index_rbf_features(self._ix, Z, gamma)
            try:
                try:
                    mo = eng.index_fit_moments(feat, t)
                except _hip.ScannHipError as e:
                    if e.code == -1:
                        raise ValueError(str(e)) from None
                    raise
                fit = head_closed_form(mo, m, grid)
                args = (feat, t, fit["mean"], fit["tmean"], fit["components"], fit["scale"], fit["coef"], fit["lev0"])
                pick = head_pick(eng.index_ridge_loo(*args)["sse"], fit["l2"])
                return fit, eng.index_ridge_loo(*args, pick), pick
            finally:
                feat.free()

        return kernel_head_result(run, hs, Z, R2, positions, ids, atoms, t, names, self.level, self.dim)

    def fit_class_head(self, labels, l2="cv", folds=4, max_iter=100, tol=1e-4, classes=None):
        """A classification head for ``labels`` (integers [N], one per row of this index; -1: unlabelled) on the frozen rows:
        multinomial logistic regression (softmax, 2 .. 16 classes) in the principal axes of the rows, the ridge strength chosen by
        ``folds``-fold cross-validation (the fold of a row is its position mod ``folds``).  Every pass over the rows -- for all strengths
        and folds at once, each model's log-likelihood gradient and score sums (scann_index_logit_pass) -- runs on the GPU and depends
        on the index contents and the arguments only, bit for bit; the optimiser (``class_head_fit``: L-BFGS in fp64 on the host, which
        needs gradients only) is deterministic given them.  ``classes``: the label values in the order of the head's classes (None: the
        distinct labels other than -1, ascending).  ``l2``: "cv" -- the grid max(s_0 10^-l, noise floor), l = 0 .. 5, s_0 the largest
        eigenvalue --, one number, or a sequence of at most 8; ``folds`` 0 (one ``l2`` value only: no folds are fitted) or 2 .. 16.
        The strength with the least held-out Brier sum wins, ties to the larger; the head is the all-rows model at that strength.
        Returns ``(result, head)``: {"l2", "cv_accuracy", "cv_brier", "cv_log_loss" (fp64 on the host from the held-out probability of
        the true class: this one statistic goes through the host's ``log``), "cv_confusion" [C, C] (true class, predicted class),
        "fit_accuracy", "class_count" [C], "n_rows", "cv_probability" fp32 [N, C] (held out; NaN for rows that do not count),
        "weights" fp32 [C, dim], "intercept" fp32 [C], "iterations", "converged", "stopped", "passes", "classes", "path": {"l2",
        "cv_accuracy", "cv_brier", "converged"}} and the ``LatentClassHead`` that ``HipModel.predict_class_head`` takes.  With
        ``folds=0`` the cv entries are NaN.  Bad arguments raise ValueError before any device call: fewer than 2 classes present, a
        class without a labelled row, fewer labelled rows than 2 per fold, bad ``folds``, ``l2``, ``max_iter`` or ``tol``; a class
        whose rows all have a non-finite component raises it after the first pass."""
        lab, classes = class_labels_arg(labels, classes, len(self))
        grid, folds, max_iter, tol = class_fit_args(l2, folds, max_iter, tol)
        class_count_check(np.bincount(lab[lab >= 0], minlength=len(classes)), classes, folds)
        eng = self.model.engine
        try:
            mo = eng.index_moments(self._ix)
        except _hip.ScannHipError as e:
            if e.code == -1:
                raise ValueError(str(e)) from None
            raise

        def run_pass(weights, fold, prob_of_fold=None):
            return eng.index_logit_pass(self._ix, lab, mo["mean"], weights, fold, folds, prob_of_fold)

        fit = class_head_fit(run_pass, mo, lab, len(classes), grid, folds, max_iter, tol)
        return class_head_result(fit, lab, classes, self.level, self.dim)

    def embed(self, perplexity=10, iterations=(250, 500), exaggeration=12.0, learning_rate="auto", route="device", graph=None):
        """The neighbour embedding (t-SNE) of this index's rows in two dimensions: the map that keeps neighbourhoods, where ``pca`` draws
        the linear one.  The repulsion between all pairs of rows is computed exactly on the GPU (scann_embed_iterate), so the map depends
        on the index contents and the arguments only, bit for bit.  Each row's 31 nearest other rows come from the index's exact search
        (``neighbour_graph``), their affinities from ``embed_affinities`` at ``perplexity`` (2 .. 15).  The initial layout is ``pca(2)``'s
        coordinates scaled so that the first column's standard deviation is 1e-4, with zero velocity and unit gains.  Two calls of the
        iteration follow: ``iterations[0]`` with ``exaggeration`` and momentum 0.5, then ``iterations[1]`` with exaggeration 1 and
        momentum 0.8, both with ``learning_rate`` ("auto": max(200, N / 12)).  ``route`` "host" runs the host twin instead of the
        device: the same bits.  Returns ``(result, embedding)``: {"coords" fp32 [N, 2], "kl_init", "kl" (the Kullback-Leibler divergence
        over the stored edges, fp64 on the host, of the initial and of the final layout, each with its own Z from one more iteration
        whose result is dropped), "z", "neighbor_position" int32 [N, K], "neighbor_dist2" fp32 [N, K], "n_edges", "learning_rate"} and
        the ``LatentEmbedding`` that ``HipModel.place`` takes.  Bad arguments, an index above 262,144 rows, fewer rows than the
        perplexity needs and rows with a non-finite component raise ValueError; the arguments are checked before any GPU work.
        ``graph``: the ``(position, dist2)`` of ``neighbour_graph`` for these rows where the caller has it already (``choose_perplexity``
        computes it once for all its maps)."""
        perplexity, iterations, exaggeration, route = embed_fit_args(perplexity, iterations, exaggeration, learning_rate, route)
        N = len(self)
        if N > _hip.EMBED_MAX_ROWS:
            raise ValueError("the index has %d rows, an embedding takes at most %d: thin it first with select(m), or embed the medoids of "
                             "cluster(k)" % (N, _hip.EMBED_MAX_ROWS))
        if N - 1 <= perplexity or N < 3:
            raise ValueError("perplexity %g needs more than %d rows, the index has %d" % (perplexity, int(perplexity) + 1, N))
        lr = max(200.0, N / 12.0) if isinstance(learning_rate, str) else float(learning_rate)
        eng = self.model.engine
        pca, _ = self.pca(2)
        y0 = embed_initial_layout(pca["coordinates"])
        pos, d2 = neighbour_graph(self) if graph is None else graph
        row_first, col, p = embed_affinities(d2, pos, perplexity)
        if route == "device":
            step = functools.partial(eng.embed_iterate, row_first, col, p)
        else:
            step = functools.partial(_hip.embed_iterate_host, row_first, col, p)
        ids, atoms = eng.index_names(self._ix)
        return embed_run(step, y0, row_first, col, p, iterations, exaggeration, lr, pos, d2, ids, atoms, perplexity, self.level, self.dim)

    def density_peaks(self, k=None, bandwidth="auto", neighbours=31, min_density=None, min_delta=None, route="device"):
        """Density-peak clustering of this index's rows (Rodriguez & Laio 2014): a clustering that needs neither a number of clusters
        nor round ones.  A row is a cluster centre if it is denser than its surroundings and far from anything denser; every other row
        follows its nearest denser row.  The Gaussian kernel density of every row and its nearest denser row come from two exact passes
        over all pairs on the GPU (scann_index_peaks), defined to the bit, so the result depends on the index contents and the arguments
        only.  ``bandwidth``: the kernel width h, a positive number, or "auto": h^2 is the median over the rows of the squared distance
        to the ``neighbours``-th nearest other row (1 .. 31, capped at N - 1; ``neighbour_graph``, whose ValueError for a row with a
        non-finite component it inherits).  Centres: the first ``k`` rows under (density x delta descending, position ascending), or --
        with ``min_density`` and ``min_delta`` instead of ``k`` -- the rows at or above both thresholds plus the densest row.  Clusters
        are numbered in density order of their centres (the densest row's is 0); rows with a non-finite component get label -1.
        ``route`` "host" runs the host twin on the rows read back: the same bits.  Returns ``(result, peaks)``: {"label" int32 [N],
        "density" fp64 [N] (the mean kernel weight to the other eligible rows; NaN for label -1), "delta" fp64 [N] (the distance to the
        nearest denser row, inf for the densest), "parent" int32 [N], "sum" int64 [N], "centre_position" int32, "centre_id" int64,
        "centre_atom" int32, "size" int64 per cluster, "decision" (density x delta sorted descending: the gap in it tells how many
        clusters there are), "bandwidth", "gamma", "n_eligible"} and the ``LatentPeaks`` that labels the neighbours ``nearest(k=1)``
        finds.  Bad arguments raise ValueError before any device call."""
        k, neighbours, min_density, min_delta, route = peaks_fit_args(k, bandwidth, neighbours, min_density, min_delta, route)
        N = len(self)
        if N < 1:
            raise ValueError("density peaks need at least 1 row, the index has 0")
        eng = self.model.engine
        if isinstance(bandwidth, str):
            _, d2 = neighbour_graph(self)
            h = peaks_auto_bandwidth(d2, neighbours)
        else:
            h = float(bandwidth)
        gamma = _hip.rbf_gamma(h)
        r = eng.index_peaks(self._ix, gamma) if route == "device" else _hip.peaks_host(self.rows()[0], gamma)
        ids, atoms = eng.index_names(self._ix)  # (host copies: the rows stay on the device)
        return peaks_result(r, ids, atoms, k, min_density, min_delta, h, gamma, self.level, self.dim)

    def prototypes(self, m, criticisms=0, bandwidth="auto", neighbours=31, witness="under", assign=True, route="device"):
        """The ``m`` rows that stand for all of this index, and the rows those do not stand for: MMD-critic (Kim, Khanna & Koyejo 2016).
        Prototypes are picked greedily so that the Gaussian kernel mean of the picked set matches the kernel mean of the index; the
        greedy loop runs on the GPU in exact integers (scann_index_prototypes), so the picks depend on the index contents, the bandwidth
        and ``m`` only, bit for bit, and the first pick is the densest row.  ``criticisms``: that many rows where the two kernel means
        still differ most, picked greedily with kernel suppression so that they do not repeat each other (scann_index_criticisms);
        ``witness`` "under" weighs a row by how far the prototypes under-represent it, "both" by the absolute difference (the paper's
        rule).  ``bandwidth``: the kernel width h, a positive number, or "auto" as in ``density_peaks``.  ``route`` "host" runs the host
        twins on the rows read back: the same bits.  Returns ``(result, prototypes)``: {"position" int32, "id" int64, "atom" int32,
        "score", "b_at_pick" int64 [m'], "mmd2" fp64 [m'] (the squared MMD between the index and the first 1 .. m' prototypes),
        "witness" fp64 [N] (mean kernel weight to the index less that to the prototypes; NaN for a row with a non-finite component),
        "A", "B" int64 [N], "count", "n_eligible", "criticism_position", "criticism_id", "criticism_atom", "criticism_score",
        "criticism_witness", "bandwidth", "gamma", and with ``assign`` and m' <= 1024 "nearest_prototype" int32 [N] and "size" int64
        [m']} and the ``LatentPrototypes`` that holds the picked rows.  Bad arguments raise ValueError before any device call."""
        m, criticisms, neighbours, witness, assign, route = prototypes_fit_args(m, criticisms, bandwidth, neighbours, witness, assign, route)
        N = len(self)
        if N < 1:
            raise ValueError("prototypes need at least 1 row, the index has 0")
        _hip.check_prototypes_args(m, 1.0, N)
        eng, ix = self.model.engine, self._ix
        h = peaks_auto_bandwidth(neighbour_graph(self)[1], neighbours) if isinstance(bandwidth, str) else float(bandwidth)

        def rows_at(pos):
            return np.concatenate([eng.index_read(ix, int(p), 1)[0] for p in pos] + [np.zeros((0, self.dim), np.float32)])

        if route == "device":
            proto, crit = functools.partial(eng.index_prototypes, ix), functools.partial(eng.index_criticisms, ix)
            assign_to = (lambda pos: eng.index_kmeans(ix, pos, 0, 0)) if assign else None
        else:
            rows = self.rows()[0]
            proto, crit = functools.partial(_hip.prototypes_host, rows), functools.partial(_hip.criticisms_host, rows)
            assign_to = (lambda pos: _hip.kmeans_host(rows, rows[pos], 0, 0)) if assign else None
        return prototypes_run(proto, crit, assign_to, lambda: eng.index_names(ix), rows_at, m, criticisms, h, witness, self.level, self.dim)

    def mmd(self, other, bandwidth, chunk=65536):
        """The squared maximum mean discrepancy between this index and ``other`` (a ``LatentIndex`` of the same model, level and
        width) under the Gaussian kernel of width ``bandwidth``: dataset shift in one number.  mmd2 = mean k(a, a') + mean k(b, b') -
        2 mean k(a, b), every mean over all pairs of rows without a non-finite component, the row itself included.  The self terms come
        from the two self-joins, the cross term from the density of ``other``'s rows under this index (``chunk`` host queries at a
        time): integer sums, so the value is exact and order-free.  Returns {"mmd2", "witness" fp64 [len(other)] (mean kernel weight of
        each row of ``other`` to this index less that to ``other``), "numerator", "denominator" (Python integers), "bandwidth"}."""
        if not isinstance(other, LatentIndex) or other.model is not self.model or other.level != self.level or other.dim != self.dim:
            raise ValueError("other must be a %s-level LatentIndex of %d columns of the same model" % (self.level, self.dim))
        if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or int(chunk) < 1:
            raise ValueError("chunk must be an integer >= 1, got %r" % (chunk,))
        gamma = _hip.rbf_gamma(bandwidth)
        eng = self.model.engine

        def self_sums(index):  # the row itself counts: + 2^30 on the eligible rows
            S = eng.index_peaks(index._ix, gamma)["sum"] if len(index) else np.zeros(0, np.int64)
            return np.where(S >= 0, S + PROTO_ONE, -1)

        q = other.rows()[0]
        cross = [eng.index_density(self._ix, q[i:i + int(chunk)], gamma) for i in range(0, len(q), int(chunk))]
        mmd2, wit, num, den = mmd_of_sums(self_sums(self), self_sums(other), np.concatenate(cross + [np.zeros(0, np.int64)]))
        return {"mmd2": mmd2, "witness": wit, "numerator": num, "denominator": den, "bandwidth": float(bandwidth)}

    def hierarchy(self, min_samples=5, route="device"):
        """The hierarchical clustering of this index's rows: how the kinds nest, and which rows belong to none.  Single linkage
        (``min_samples`` 0) and density-based hierarchical clustering (HDBSCAN, Campello et al. 2013; ``min_samples`` 1 .. 31) both rest
        on the minimum spanning tree of the complete graph over the rows, the second with the mutual-reachability weight
        max(dist2, core2_i, core2_j), core2_i the squared distance to the ``min_samples``-th nearest other row without a non-finite
        component (``hierarchy_core2`` over ``neighbour_graph``: the exact search's bits).  The tree is built exactly on the GPU by
        Boruvka rounds of all-pairs passes (scann_index_mst) and is unique under the edge order (w, min, max), so it depends on the index
        contents and ``min_samples`` only, bit for bit.  ``route`` "host" runs the host twins on the rows read back: the same bits.
        Returns ``(result, hierarchy)``: {"a", "b" int32 [n_edges], "w" fp32 [n_edges] (the edges in the edge order, a < b),
        "core2" fp32 [N] (None for ``min_samples`` 0), "rounds" (device route), "n_eligible"} and the ``LatentHierarchy`` with
        ``linkage()``, ``cut(...)`` and ``clusters(min_cluster_size)``.  Rows with a non-finite component are in no edge and get label
        -1 everywhere.  Bad arguments and an index above 262,144 rows raise ValueError before any device call."""
        min_samples, route = hierarchy_fit_args(min_samples, route)
        N = len(self)
        if N > _hip.MST_MAX_ROWS:
            raise ValueError("the index has %d rows, a hierarchy takes at most %d: thin it first with select(m), or cluster the medoids of "
                             "cluster(k)" % (N, _hip.MST_MAX_ROWS))
        eng = self.model.engine
        rows = self.rows()[0] if (min_samples or route == "host") else None
        core2 = None
        if min_samples:
            elig = np.isfinite(rows).all(axis=1)
            if route == "host":
                graph = lambda x: neighbour_graph_host(x, strict=False)  # noqa: E731
            elif elig.all():
                graph = lambda x: neighbour_graph(self, strict=False)  # noqa: E731
            else:
                def graph(x):  # the search over the rows that count, on the device like the rest
                    sub = LatentIndex(self.model, self.level)
                    try:
                        return neighbour_graph(sub.add_rows(x), strict=False)
                    finally:
                        sub.free()
            core2 = hierarchy_core2(rows, min_samples, graph, elig)
        r = eng.index_mst(self._ix, core2) if route == "device" else _hip.mst_host(rows, core2)
        ids, atoms = eng.index_names(self._ix)  # (host copies: the rows stay on the device)
        lone = -1
        if N and not len(r["a"]):  # no edge: no eligible row, or one -- the rows tell
            lone = hierarchy_lone_row(self.rows()[0] if rows is None else rows)
        return hierarchy_result(r, core2, N, ids, atoms, min_samples, self.level, self.dim, lone)

    def map_quality(self, coords, k=15, sample=None, seed=0, route="device", graph=None):
        """Whether a map of this index's rows can be believed: the rank-based scores of ``coords`` -- fp32 [N, c] in position order, a
        ``LatentEmbedding`` of this index, or the result of ``embed`` / ``pca`` -- against the rows themselves (Venna & Kaski 2001; Lee
        & Verleysen 2009).  Each row's 31 nearest other rows in latent space (``neighbour_graph``, or the ``graph`` = (position, dist2)
        that ``embed`` returned) and on the map (the same search on a temporary index of the coordinates) are ranked in the OTHER
        space by one exact pass over all pairs on the GPU each (scann_index_ranks), defined to the bit; the scores are fp64 NumPy on
        those integers.  With rho the 0-based rank, K = min(31, N - 2) and the first k places of a row's lists:
          row_trustworthiness = 1 - 2 / (k (2N - 3k - 1)) * the sum over its map-neighbours of max(0, rho_latent + 1 - k),
          row_continuity likewise over its latent-neighbours with rho_map,  row_overlap = #(map-neighbours with rho_latent < k) / k,
        "trustworthiness", "continuity" and "neighbour_overlap" their means over the scored rows (formed from the integer totals);
        "ks" 1 .. K with "trustworthiness_curve", "continuity_curve" (NaN where 2N - 3k' - 1 <= 0) and "qnx_curve" the same at every
        k'; "lcmc" = neighbour_overlap - k / (N - 1); "rnx_auc" the 1/k'-weighted mean of ((N - 1) Q_NX(k') - k') / (N - 1 - k');
        "false_neighbours" / "missed_neighbours" int32 per row: its map-neighbours that are no latent-neighbours, and the reverse;
        "rank_latent" / "rank_map" int32 [n, K] the ranks themselves; "position" the scored rows, "k", "n_rows".
        ``sample``: None, m rows drawn with ``seed`` or positions (the silhouette's rule): those rows are scored exactly against all
        rows.  ``route`` "host" runs the twins on the rows read back: the same bytes.  ValueError for k outside 1 .. K, 2N - 3k - 1
        <= 0, coordinates of the wrong length or not finite -- before any GPU work -- and for rows with a non-finite component."""
        route = silhouette_route(route)
        coords = map_coords_arg(coords, self)
        if route == "host":
            return map_quality_rows_host(self.rows()[0], coords, k=k, sample=sample, seed=seed, graph=graph)
        N = len(self)
        k = map_quality_k_arg(k, N)
        sample = silhouette_sample_arg(sample, seed, N)
        eng = self.model.engine
        low = _CoordIndex(self.model, coords)
        try:
            return map_quality_run(lambda: neighbour_graph(self) if graph is None else graph, lambda: neighbour_graph(low),
                                   lambda probe, q: eng.index_ranks(self._ix, probe, q)["rank"],
                                   lambda probe, q: eng.index_ranks(low._ix, probe, q)["rank"], N, k, sample, seed)
        finally:
            low.free()

    def choose_perplexity(self, perplexities, k=15, sample=None, seed=0, **embed_args):
        """Which perplexity draws the most faithful map: ``embed`` at every perplexity of ``perplexities`` (ascending, distinct), each
        map scored by ``map_quality`` at ``k``, and ``pca(2)`` scored as the row "linear".  The latent neighbour graph is computed once
        and shared by the maps and the scores.  Returns ``(table, embedding)``: {"perplexity" (a list, "linear" last),
        "neighbour_overlap", "trustworthiness", "continuity", "lcmc", "rnx_auc", "kl" fp64 arrays (kl NaN for "linear"),
        "best_perplexity", "best" (the best map's ``embed`` result) and "quality" (its ``map_quality``)} and the ``LatentEmbedding``
        with the greatest neighbour_overlap, ties to the lower perplexity.  ``embed_args``: ``embed``'s other arguments."""
        perplexities = choose_perplexity_arg(perplexities)
        map_quality_k_arg(k, len(self))
        silhouette_sample_arg(sample, seed, len(self))
        graph = neighbour_graph(self)
        return choose_perplexity_run(lambda p: self.embed(perplexity=p, graph=graph, **embed_args),
                                     lambda c: self.map_quality(c, k=k, sample=sample, seed=seed, graph=graph,
                                                                route=embed_args.get("route", "device")),
                                     lambda: self.pca(2)[0]["coordinates"], perplexities)

    def place(self, rows, embedding):
        """Host ``rows`` [n, dim] on an existing map of this index (``embedding``, as ``embed`` returned it for these rows): each row's
        31 nearest index rows from the exact search, conditional weights calibrated to the embedding's perplexity
        (``embed_conditional``), coordinates their weighted mean in fp64.  {"coords" fp32 [n, 2], "nearest_position" int32 [n],
        "nearest_id" int64 [n], "nearest_atom" int32 [n], "nearest_distance" fp32 [n]}."""
        embedding.check_index(self)
        k = min(EMBED_NEIGHBOURS, len(self))
        r = self.model.engine.index_query(self._ix, rows, k)
        return embedding.place(r["position"], r["dist2"])

    def free(self):
        self._ix.free()


def cluster_result(r, ids, atoms, k):
    """``LatentIndex.cluster``'s dict from the k-means call's result ``r`` and the rows' names"""
    label, d2 = r["label"], r["dist2"]
    medoid = np.full(k, -1, np.int32)
    member = np.nonzero(label >= 0)[0]
    least = np.full(k, np.inf, np.float32)
    np.minimum.at(least, label[member], d2[member])
    nearest = member[d2[member] == least[label[member]]]  # the members at their cluster's least dist2, positions ascending
    cluster, first = np.unique(label[nearest], return_index=True)
    medoid[cluster] = nearest[first]  # ... and of those the first position
    has = medoid >= 0
    return {"label": label, "distance": np.sqrt(d2),  # (correctly rounded on the host, as nearest reports distances)
            "centre": r["centre"], "size": r["size"], "n_iter": int(r["n_iter"]), "converged": bool(r["converged"]),
            "inertia": float(d2[member].astype(np.float64).sum()), "medoid_position": medoid,
            "medoid_id": np.where(has, ids[np.maximum(medoid, 0)], -1).astype(np.int64),
            "medoid_atom": np.where(has, atoms[np.maximum(medoid, 0)], -1).astype(np.int32)}


def cluster_rows_host(rows, k, init="kcenter", max_iter=50, stop_changed=0, ids=None, atoms=None):
    """``LatentIndex.cluster`` without a GPU: the host twins (``_hip.kcenter_host``, ``_hip.kmeans_host``) on ``rows`` [N, dim]; the
    same dict, bit for bit.  ``ids`` default to the positions, ``atoms`` to -1."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[1] < 1:
        raise ValueError("rows must be [N, dim], got shape %s" % (rows.shape,))
    k, max_iter, stop_changed = _hip.check_kmeans_args(k, max_iter, stop_changed)
    N, dim = rows.shape
    if isinstance(init, str):
        if init != "kcenter":
            raise ValueError('init must be "kcenter", %d positions or an array [%d, %d], got %r' % (k, k, dim, init))
        picks = _hip.kcenter_host(rows, None, k, 0.0)
        if picks["count"] < k:
            raise ValueError("k = %d clusters need %d rows without a non-finite component, the rows have %d" % (k, k, picks["count"]))
        init = rows[picks["position"]]
    else:
        a = np.asarray(init)
        if a.dtype.kind in "iu" and a.ndim == 1:
            if a.shape[0] != k or (k and (a.min() < 0 or a.max() >= N)):
                raise ValueError("init must name %d positions in 0 .. %d, got %d of them" % (k, N - 1, a.shape[0]))
            init = rows[a]
        else:
            init = _hip.check_kmeans_init(init, dim)
            if init.shape[0] != k:
                raise ValueError("init holds %d centres, k is %d" % (init.shape[0], k))
    ids = np.arange(N, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    atoms = np.full(N, -1, np.int32) if atoms is None else np.asarray(atoms, np.int32)
    return cluster_result(_hip.kmeans_host(rows, init, max_iter, stop_changed), ids, atoms, k)


def silhouette_route(route):
    if route not in ("device", "host"):
        raise ValueError('route must be "device" or "host", got %r' % (route,))
    return route


def silhouette_sample_arg(sample, seed, n_rows):
    """``sample`` of a silhouette checked: None, an integer m >= 1 (returned as int) or int32 positions; ValueError otherwise"""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or int(seed) < 0:
        raise ValueError("seed must be an integer >= 0, got %r" % (seed,))
    if sample is None:
        return None
    if isinstance(sample, bool):
        raise ValueError("sample must be None, an integer >= 1 or an array of positions, got %r" % (sample,))
    if isinstance(sample, (int, np.integer)):
        if int(sample) < 1:
            raise ValueError("sample must be None, an integer >= 1 or an array of positions, got %r" % (sample,))
        return int(sample)
    try:
        pos = np.ascontiguousarray(sample)
    except (TypeError, ValueError):
        raise ValueError("sample must be None, an integer >= 1 or an array of positions") from None
    if pos.dtype.kind not in "iu" or pos.ndim != 1:
        raise ValueError("sample must be None, an integer >= 1 or a one-dimensional array of integer positions, got %s of shape %s" % (
            pos.dtype, pos.shape))
    if pos.size and (int(pos.min()) < 0 or int(pos.max()) >= int(n_rows)):
        bad = int(np.flatnonzero((pos < 0) | (pos >= int(n_rows)))[0])
        raise ValueError("sample[%d] = %d outside 0 .. %d" % (bad, int(pos[bad]), int(n_rows) - 1))
    return pos.astype(np.int32)


def silhouette_values(a, b, own_size):
    """s = (b - a) / max(a, b) in fp64: 0 for the row of a one-row cluster and where max is 0, NaN where a or b is (the row does not
    count, or there is no other cluster)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    top = np.maximum(a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (b - a) / top
    s = np.where(np.isfinite(top) & ((top == 0.0) | (np.asarray(own_size) == 1)), 0.0, s)
    return np.where(np.isnan(a) | np.isnan(b), np.nan, s)


def silhouette_run(run_pass, moments, counting, labels, n_clusters, sample, seed, metric):
    """The host work around a silhouette pass, shared by the device and the host route.  ``run_pass(qpos or None, shift)`` is the pass,
    ``moments()`` the column statistics of the rows (None with fewer than two eligible rows), ``counting()`` the bool mask of the rows
    that count (asked for only when an integer sample has to be drawn)."""
    mo = moments()
    shift = 0 if mo is None else _hip.silhouette_shift(mo["col_exp"], np.diagonal(mo["cov"]), metric)
    N = len(labels)
    if sample is None:
        qpos, position = None, np.arange(N, dtype=np.int32)
    elif isinstance(sample, int):
        pool = np.flatnonzero(counting())
        if sample > len(pool):
            raise ValueError("sample = %d, but only %d rows count (a label >= 0 and no non-finite component)" % (sample, len(pool)))
        position = np.sort(np.random.default_rng(seed).choice(pool, sample, replace=False)).astype(np.int32)
        qpos = position
    else:
        qpos = position = sample
    r = run_pass(qpos, shift)
    size = r["count"]
    lab = labels[position]
    s = silhouette_values(r["a"], r["b"], size[np.maximum(lab, 0)])
    order = np.argsort(position, kind="stable")
    fin = np.isfinite(s[order])
    score = float(np.sum(s[order][fin], dtype=np.float64) / fin.sum()) if fin.any() else float("nan")
    per = np.full(n_clusters, np.nan, np.float64)
    for c in np.unique(lab[order][fin]):
        v = s[order][fin][lab[order][fin] == c]
        per[c] = float(np.sum(v, dtype=np.float64) / len(v))
    out = {"position": position, "silhouette": s, "a": r["a"], "b": r["b"], "other": r["other"], "size": size, "score": score,
           "cluster_score": per, "shift": shift, "metric": metric}
    if "sums" in r:
        out["sums"] = r["sums"]
    return out


def silhouette_rows_host(rows, labels, sample=None, seed=0, metric="euclidean", table=False, n_clusters=None):
    """``LatentIndex.silhouette`` without a GPU: the host twin (``_hip.silhouette_host``) on ``rows`` [N, dim]; the same dict, bit for
    bit."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[1] < 1:
        raise ValueError("rows must be [N, dim], got shape %s" % (rows.shape,))
    labels, C_, _, _, _ = _hip.check_silhouette_args(labels, len(rows), n_clusters, None, metric, 0)
    sample = silhouette_sample_arg(sample, seed, len(rows))

    def moments():
        try:
            return _hip.moments_host(rows)
        except ValueError:
            return None

    return silhouette_run(lambda q, shift: _hip.silhouette_host(rows, labels, C_, q, metric, shift, table), moments,
                          lambda: (labels >= 0) & np.isfinite(rows).all(axis=1), labels, C_, sample, seed, metric)


def cluster_scores(result):
    """The two cheap companions of the silhouette from a ``cluster`` result, in fp64 NumPy, no device work: {"calinski_harabasz":
    [B / (k - 1)] / [W / (n - k)] with W the inertia and B the sum over the clusters of size x the squared distance of the centre to the
    size-weighted mean of the centres (higher is better; 1 where W is 0), "davies_bouldin": the mean over the clusters of the largest
    (s_c + s_d) / |centre_c - centre_d|, s_c the mean distance of cluster c's rows to its centre (lower is better)}.  Empty clusters
    are left out; NaN with fewer than two clusters or no more rows than clusters.  It reads "label", "distance", "centre", "size" and
    "inertia", in whatever precision they come."""
    size = np.asarray(result["size"], np.float64)
    centre = np.asarray(result["centre"], np.float64)
    label = np.asarray(result["label"])
    dist = np.asarray(result["distance"], np.float64)
    has = size > 0
    k, n = int(has.sum()), float(size.sum())
    if k < 2 or n <= k:
        return {"calinski_harabasz": float("nan"), "davies_bouldin": float("nan")}
    mean = (size[has, None] * centre[has]).sum(axis=0) / n
    between = float((size[has] * ((centre[has] - mean) ** 2).sum(axis=1)).sum())
    within = float(result["inertia"])
    ch = 1.0 if within == 0.0 else between * (n - k) / (within * (k - 1.0))
    member = label >= 0
    spread = np.bincount(label[member], weights=dist[member], minlength=len(size))[has] / size[has]
    gap = np.sqrt(((centre[has][:, None, :] - centre[has][None, :, :]) ** 2).sum(axis=2))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (spread[:, None] + spread[None, :]) / gap
    ratio[~np.isfinite(ratio)] = 0.0  # coincident centres and the diagonal count for nothing, as in scikit-learn
    np.fill_diagonal(ratio, 0.0)
    return {"calinski_harabasz": float(ch), "davies_bouldin": float(ratio.max(axis=1).mean())}


def choose_k_arg(ks):
    """``ks`` of ``choose_k`` checked: the distinct k ascending; ValueError unless they are integers in 1 .. 1024, at least one"""
    try:
        arr = np.asarray(list(ks))
    except TypeError:
        raise ValueError("ks must be a sequence of integers in 1 .. %d, got %r" % (_hip.KMEANS_MAX_K, ks)) from None
    if arr.ndim != 1 or not arr.size or arr.dtype.kind not in "iu" or arr.min() < 1 or arr.max() > _hip.KMEANS_MAX_K:
        raise ValueError("ks must be a sequence of integers in 1 .. %d, at least one, got %r" % (_hip.KMEANS_MAX_K, ks))
    return [int(k) for k in np.unique(arr)]


def choose_k_run(cluster, silhouette, ks):
    """``choose_k``'s table from ``cluster(k)`` and ``silhouette(labels, k)`` over the ascending ``ks``"""
    rows, best = [], None
    for k in ks:
        res = cluster(k)
        sil = silhouette(res["label"], k)
        extra = cluster_scores(res)
        rows.append((k, sil["score"], res["inertia"], extra["calinski_harabasz"], extra["davies_bouldin"], res["n_iter"], res["converged"],
                     res["size"]))
        if best is None or (sil["score"] == sil["score"] and not best[1]["score"] >= sil["score"]):  # ties stay with the smaller k
            best = (res, sil, k)
    return {"k": np.array([r[0] for r in rows], np.int64), "score": np.array([r[1] for r in rows], np.float64),
            "inertia": np.array([r[2] for r in rows], np.float64), "calinski_harabasz": np.array([r[3] for r in rows], np.float64),
            "davies_bouldin": np.array([r[4] for r in rows], np.float64), "n_iter": np.array([r[5] for r in rows], np.int64),
            "converged": np.array([r[6] for r in rows], bool), "size": [r[7] for r in rows], "best_k": best[2], "best": best[0],
            "silhouette": best[1]}


def choose_k_rows_host(rows, ks, sample=None, seed=0, metric="euclidean", **cluster_args):
    """``LatentIndex.choose_k`` without a GPU: the host twins on ``rows`` [N, dim]; the same dict, bit for bit (``cluster_args`` may
    carry ``ids`` and ``atoms``)."""
    ks = choose_k_arg(ks)
    return choose_k_run(lambda k: cluster_rows_host(rows, k, **cluster_args),
                        lambda lab, k: silhouette_rows_host(rows, lab, sample=sample, seed=seed, metric=metric, n_clusters=k), ks)


def head_grid(l2):
    """``l2`` of ``fit_head`` checked: "loo" -> None (the default grid, which needs the eigenvalues), else the fp64 values; ValueError
    for anything else"""
    if isinstance(l2, str):
        if l2 != "loo":
            raise ValueError('l2 must be "loo", a number >= 0 or a sequence of them, got %r' % (l2,))
        return None
    try:
        g = np.atleast_1d(np.asarray(l2, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError('l2 must be "loo", a number >= 0 or a sequence of them, got %r' % (l2,)) from None
    if isinstance(l2, bool) or g.ndim != 1 or not 1 <= g.shape[0] <= _hip.HEAD_MAX_LAMBDA or not np.isfinite(g).all() or (g < 0).any():
        raise ValueError("l2 must hold 1 .. %d finite values >= 0, got %r" % (_hip.HEAD_MAX_LAMBDA, l2))
    return g


def head_closed_form(mo, dim, grid=None):
    """The moments of [rows | targets] ({"n", "mean", "cov", "col_exp", "bits"}) -> what the leave-one-out pass takes, in fp64 and cast
    to fp32 at the end: the eigen-decomposition of the X-X block (``_hip.sym_eig``), the components above the noise floor, and per
    strength lambda_l  beta_lkc = g_kc / (s_c + lambda_l), g_k = V c_xy,k;  S_lc = 1 / sqrt((n - 1)(s_c + lambda_l));  lev0 = 1 / n.
    ValueError for fewer than 3 rows or no component above the floor."""
    n = int(mo["n"])
    if n < 3:
        raise ValueError("a head needs at least 3 rows without a non-finite component or target, got %d" % n)
    cov = np.asarray(mo["cov"], dtype=np.float64)
    w, v, _ = _hip.sym_eig(cov[:dim, :dim])
    noise = float(dim) * 2.0 ** (2 * int(np.asarray(mo["col_exp"])[:dim].max()) - int(mo["bits"]) + 2)
    m = int((w > noise).sum())
    if m < 1:
        raise ValueError("no component of the rows' covariance lies above its noise floor %.3g: nothing to regress on" % noise)
    s, V = w[:m], v[:m]
    if grid is None:
        grid = np.maximum(s[0] * 10.0 ** (-np.arange(17) / 2.0), noise)
        grid = grid[np.concatenate([[True], grid[1:] != grid[:-1]])]  # (non-increasing: duplicates are neighbours)
    grid = np.asarray(grid, dtype=np.float64)
    g = (V @ cov[:dim, dim:]).T  # [K, m]
    den = s[None, :] + grid[:, None]  # [L, m]
    with np.errstate(divide="ignore", invalid="ignore"):
        beta = g[None, :, :] / den[:, None, :]
        scale = 1.0 / np.sqrt((n - 1.0) * den)
    out = {"n": n, "m": m, "noise_floor": noise, "variance": s, "l2": grid, "beta": beta, "V": V, "lev0": 1.0 / n,
           "mean": np.asarray(mo["mean"][:dim], np.float32), "tmean": np.asarray(mo["mean"][dim:], np.float32),
           "components": V.astype(np.float32), "scale": scale.astype(np.float32), "coef": beta.astype(np.float32),
           "tvar": np.diag(cov)[dim:].copy()}
    for name in ("scale", "coef"):
        if not np.isfinite(out[name]).all():
            raise ValueError("l2 is too small for this index: %s is not finite in fp32" % name)
    return out


def head_pick(sse, l2):
    """Per target the strength with the least leave-one-out sum of squares (NaN counts as inf), ties to the larger lambda: int32 [K]"""
    sse = np.where(np.isnan(sse), np.inf, np.asarray(sse, dtype=np.float64))
    order = np.lexsort((-np.asarray(l2, dtype=np.float64), ))  # larger lambda first
    pick = np.zeros(sse.shape[1], np.int32)
    for k in range(sse.shape[1]):
        col = sse[order, k]
        pick[k] = order[int(np.argmin(col))]  # (argmin: the first of equals, i.e. the larger lambda)
    return pick


def head_result(fit, loo, pick, t, names, level, dim):
    """``fit_head``'s ``(result, head)`` from the closed form, the second leave-one-out pass and the picks"""
    n, K = fit["n"], len(pick)
    kk = np.arange(K)
    sse, sae, sse_fit = loo["sse"][pick, kk], loo["sae"][pick, kk], loo["sse_fit"][pick, kk]
    W = np.einsum("kc,cj->kj", fit["beta"][pick, kk, :], fit["V"])  # fp64
    sigma2 = sse / n
    tss = fit["tvar"] * (n - 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = 1.0 - sse / tss
    head = LatentHead(fit["mean"], fit["tmean"], W.astype(np.float32), fit["components"], fit["scale"][pick], fit["lev0"], sigma2, fit["l2"][pick],
                      level, dim, names)
    result = {"l2": fit["l2"][pick], "loo_rmse": np.sqrt(sse / n), "loo_mae": sae / n, "loo_r2": r2, "fit_rmse": np.sqrt(sse_fit / n),
              "dof": loo["dof"][pick], "sigma2": sigma2, "n_rows": n, "loo_prediction": (t - loo["resid"]).astype(np.float32),
              "weights": head.weights, "names": list(names),
              "path": {"l2": fit["l2"], "loo_rmse": np.sqrt(loo["sse"] / n), "dof": loo["dof"]}}
    return result, head


class LatentHead(SavedResult):
    """A linear readout head on one level of one model, as ``LatentIndex.fit_head`` fits it: prediction_k = tmean_k + (x - mean) . W_k
    and leverage_k = lev0 + sum_c ((x - mean) . V_c scale_kc)^2, so that std_k = sqrt(sigma2_k (1 + leverage_k)) is the predictive
    standard deviation of Bayesian linear regression.  mean [dim], tmean [K], weights [K, dim], components [m, dim], scale [K, m] fp32;
    sigma2, l2 [K] fp64."""
    NOUN = "head"
    FIELDS = saved_fields("mean", "tmean", "weights", "components", "scale", ("lev0", AS_FLOAT), "sigma2", "l2", ("names", AS_NAMES))

    def __init__(self, mean, tmean, weights, components, scale, lev0, sigma2, l2, level, dim=None, names=None):
        if level not in LEVELS:
            raise ValueError("level must be one of %s, got %r" % (", ".join(LEVELS), level))
        self.mean, self.components, _ = _hip.check_pca_args(mean, components, None, dim)
        try:
            self.tmean = np.ascontiguousarray(tmean, dtype=np.float32)
            self.weights = np.ascontiguousarray(weights, dtype=np.float32)
            self.scale = np.ascontiguousarray(scale, dtype=np.float32)
            self.sigma2 = np.ascontiguousarray(sigma2, dtype=np.float64)
            self.l2 = np.ascontiguousarray(l2, dtype=np.float64)
            self.lev0 = float(lev0)
        except (TypeError, ValueError):
            raise ValueError("tmean, weights, scale, sigma2 and l2 must be arrays of numbers and lev0 a number") from None
        K, d, m = self.tmean.shape[0] if self.tmean.ndim == 1 else 0, self.mean.shape[0], self.components.shape[0]
        if not 1 <= K <= _hip.HEAD_MAX_TARGETS:
            raise ValueError("tmean must hold 1 .. %d values, got shape %s" % (_hip.HEAD_MAX_TARGETS, self.tmean.shape))
        for name, a, shape in (("weights", self.weights, (K, d)), ("scale", self.scale, (K, m)), ("sigma2", self.sigma2, (K,)), ("l2", self.l2, (K,))):
            if a.shape != shape:
                raise ValueError("%s must have shape %s, got %s" % (name, shape, a.shape))
        for name, a in (("tmean", self.tmean), ("weights", self.weights), ("scale", self.scale), ("lev0", np.float64(self.lev0))):
            if not np.isfinite(a).all():
                raise ValueError("%s holds a non-finite value" % name)
        if np.isnan(self.sigma2).any() or (self.sigma2 < 0).any():
            raise ValueError("sigma2 must be >= 0")
        self.level, self.dim = level, int(d)
        self.names = ["target_%d" % k for k in range(K)] if names is None else [str(x) for x in names]
        if len(self.names) != K:
            raise ValueError("names: %d for %d targets" % (len(self.names), K))

    @property
    def k(self):
        return int(self.tmean.shape[0])

    @classmethod
    def from_saved(cls, v, level, dim):
        names = v.pop("names")  # (the constructor takes them last)
        return cls(*v.values(), level, dim, names)

    def finish(self, pred, lev):
        """the device's pred and lev [n, K] as {"prediction", "std", "leverage"}: the square root taken on the host in fp64"""
        with np.errstate(invalid="ignore"):
            std = np.sqrt(self.sigma2[None, :] * (1.0 + lev.astype(np.float64))).astype(np.float32)
        return {"prediction": pred, "std": std, "leverage": lev}


CLASS_L2_DECADES = 6      # l2="cv": max(s_0 10^-l, noise floor), l = 0 .. 5
CLASS_MAX_L2 = 8
CLASS_MEMORY = 8          # curvature pairs L-BFGS keeps
CLASS_MAX_SHRINKS = 8     # secant shrinks of one line search
CLASS_SLACK = 1e-6        # a step is accepted when the directional derivative at the new point is <= CLASS_SLACK |the one at the old point|


def class_labels_arg(labels, classes, n_rows):
    """``labels`` and ``classes`` of ``fit_class_head`` checked: (int32 [N] class indices with -1 for unlabelled, int64 [C] class values);
    ValueError otherwise"""
    a = np.asarray(labels)
    if a.dtype.kind not in "iu" or a.ndim != 1:
        raise ValueError("labels must be an integer array of shape [N], got %s %s" % (a.dtype, a.shape))
    if a.shape[0] != int(n_rows):
        raise ValueError("labels hold %d rows, the index %d" % (a.shape[0], int(n_rows)))
    a = a.astype(np.int64)
    if classes is None:
        cl = np.unique(a[a != -1])
    else:
        try:
            cl = np.asarray(classes)
        except (TypeError, ValueError):
            raise ValueError("classes must be a sequence of distinct integers other than -1") from None
        if cl.dtype.kind not in "iu" or cl.ndim != 1 or len(np.unique(cl)) != len(cl) or (cl == -1).any():
            raise ValueError("classes must be a sequence of distinct integers other than -1, got %r" % (classes,))
        cl = cl.astype(np.int64)
    if not 2 <= len(cl) <= _hip.LOGIT_MAX_CLASSES:
        raise ValueError("a classification head needs 2 .. %d classes, the labels%s hold %d" % (
            _hip.LOGIT_MAX_CLASSES, "" if classes is None else " and classes", len(cl)))
    order = np.argsort(cl, kind="stable")
    at = np.minimum(np.searchsorted(cl[order], a), len(cl) - 1)
    known = cl[order][at] == a
    bad = np.nonzero(~known & (a != -1))[0]
    if bad.size:
        raise ValueError("labels[%d] = %d is neither -1 nor one of the classes" % (bad[0], int(a[bad[0]])))
    return np.ascontiguousarray(np.where(known, order[at], -1), dtype=np.int32), cl


def class_fit_args(l2, folds, max_iter, tol):
    """``l2``, ``folds``, ``max_iter`` and ``tol`` of ``fit_class_head`` checked: (None for "cv" or the fp64 strengths, folds, max_iter,
    tol); ValueError otherwise"""
    if isinstance(l2, str):
        if l2 != "cv":
            raise ValueError('l2 must be "cv", a number >= 0 or a sequence of at most %d, got %r' % (CLASS_MAX_L2, l2))
        grid = None
    else:
        try:
            grid = np.atleast_1d(np.asarray(l2, dtype=np.float64))
        except (TypeError, ValueError):
            raise ValueError('l2 must be "cv", a number >= 0 or a sequence of at most %d, got %r' % (CLASS_MAX_L2, l2)) from None
        if isinstance(l2, bool) or grid.ndim != 1 or not 1 <= grid.shape[0] <= CLASS_MAX_L2 or not np.isfinite(grid).all() or (grid < 0).any():
            raise ValueError("l2 must hold 1 .. %d finite values >= 0, got %r" % (CLASS_MAX_L2, l2))
    if isinstance(folds, bool) or not isinstance(folds, (int, np.integer)) or not (int(folds) == 0 or 2 <= int(folds) <= _hip.LOGIT_MAX_FOLDS):
        raise ValueError("folds must be 0 or an integer in 2 .. %d, got %r" % (_hip.LOGIT_MAX_FOLDS, folds))
    if int(folds) == 0 and (grid is None or len(grid) != 1):
        raise ValueError("folds=0 fits no folds, so l2 must be one number, got %r" % (l2,))
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or not 1 <= int(max_iter) <= 100000:
        raise ValueError("max_iter must be an integer in 1 .. 100000, got %r" % (max_iter,))
    try:
        tol_f = float(tol)
    except (TypeError, ValueError):
        raise ValueError("tol must be a number > 0, got %r" % (tol,)) from None
    if isinstance(tol, bool) or not (tol_f > 0.0 and np.isfinite(tol_f)):
        raise ValueError("tol must be a number > 0, got %r" % (tol,))
    return grid, int(folds), int(max_iter), tol_f


def class_count_check(count, classes, folds):
    """ValueError for a class without a row, or fewer rows than 2 per fold"""
    for k, c in enumerate(count):
        if c < 1:
            raise ValueError("class %d (label %d) has no row that counts" % (k, int(classes[k])))
    if int(np.sum(count)) < 2 * max(int(folds), 1):
        raise ValueError("%d folds need at least %d rows that count, got %d" % (folds, 2 * max(int(folds), 1), int(np.sum(count))))


def class_head_fit(run_pass, mo, lab, n_classes, grid, folds, max_iter, tol):
    """The optimiser of ``fit_class_head``, deterministic given the passes' outputs.  ``run_pass(weights fp32 [M, C, dim + 1], fold int32
    [M], prob_of_fold=None)`` is ``Engine.index_logit_pass`` on the index, or ``_hip.logit_pass_host`` on the same rows: the host route.
    ``mo``: the rows' moments (``index_moments`` / ``moments_host``); their covariance is decomposed (``_hip.sym_eig``) and components at
    or below the noise floor are dropped, as ``head_closed_form`` does.  One model per (strength, fold) and one on all rows per
    strength; model j minimises  sum_i nll_i + (n - 1) l2_j / 2 |W|^2,  W [C, m] in principal-axis coordinates, the intercept
    unpenalised, n the rows that count.  L-BFGS (memory 8, fp64) per model, all models advancing in lockstep with one pass per round
    (64 models at most per call).  The initial inverse Hessian is the diagonal 1 / ((n - 1)(s_c / 2 + l2)), 2 / n for the intercept:
    Boehning's bound, valid for every fold because the all-row Gram matrix dominates every subset's.  Weights go to the device as U = W V
    cast to fp32, gradients come back as V grad_x.  A step t (first 1) is accepted when the directional derivative at the new point is <=
    CLASS_SLACK times the size of the one at the old point: the objective is convex, so up to that slack it did not rise along the step,
    and no loss value is needed.  Otherwise t shrinks by the secant of the two directional derivatives, at most 8 times; then the model
    stops with stopped="line_search".  Converged: max |grad| / n_train <= tol.  A non-finite gradient raises ValueError."""
    C = int(n_classes)
    dim = int(np.asarray(mo["mean"]).shape[0])
    cov = np.asarray(mo["cov"], dtype=np.float64)
    w, v, _ = _hip.sym_eig(cov)
    noise = float(dim) * 2.0 ** (2 * int(np.asarray(mo["col_exp"]).max()) - int(mo["bits"]) + 2)
    m = int((w > noise).sum())
    if m < 1:
        raise ValueError("no component of the rows' covariance lies above its noise floor %.3g: nothing to classify on" % noise)
    s, V = w[:m], v[:m]
    if grid is None:
        grid = np.maximum(s[0] * 10.0 ** (-np.arange(CLASS_L2_DECADES, dtype=np.float64)), noise)
        grid = grid[np.concatenate([[True], grid[1:] != grid[:-1]])]  # (non-increasing: duplicates are neighbours)
    grid = np.asarray(grid, dtype=np.float64)
    L, F = len(grid), int(folds)
    model_l2 = np.repeat(grid, F + 1)
    model_fold = np.tile(np.concatenate([np.arange(F), [-1]]), L).astype(np.int32)
    M = L * (F + 1)
    mean = np.ascontiguousarray(mo["mean"], dtype=np.float32)
    passes = 0

    def to_device(X):  # [.., C, m + 1] principal-axis weights and intercept -> U fp32 [.., C, dim + 1]
        U = np.concatenate([X[..., :m] @ V, X[..., m:]], axis=-1)
        with np.errstate(over="ignore"):
            U = U.astype(np.float32)
        if not np.isfinite(U).all():
            raise ValueError("the weights left the range of fp32: l2 is too small for this index")
        return U

    def evaluate(idx, X):  # the passes of models idx at X [len(idx), C, m + 1] -> (log-likelihood gradient in principal axes, stats, n)
        nonlocal passes
        g, st, n = np.zeros((len(idx), C, m + 1)), np.zeros((len(idx), 2, 3)), 0
        for a in range(0, len(idx), _hip.LOGIT_MAX_MODELS):
            b = min(len(idx), a + _hip.LOGIT_MAX_MODELS)
            r = run_pass(to_device(X[a:b]), model_fold[idx[a:b]])
            passes += 1
            g[a:b, :, :m] = r["grad"][:, :, :dim] @ V.T
            g[a:b, :, m] = r["grad"][:, :, dim]
            st[a:b], n = r["stats"], int(r["n"])
        return g, st, n

    everyone = np.arange(M)
    X = np.zeros((M, C, m + 1))
    g_ll, stats, n = evaluate(everyone, X)
    p0 = float(np.float32(1.0) / np.float32(C))  # every probability at U = 0
    j_all = F  # the first strength's all-rows model
    count = np.rint(g_ll[j_all, :, m] + stats[j_all, 0, 0] * p0).astype(np.int64)
    class_count_check(count, np.arange(C), F)
    pen = (n - 1.0) * model_l2  # [M]
    h0 = np.empty((M, C, m + 1))
    h0[:, :, :m] = 1.0 / ((n - 1.0) * (s[None, None, :] / 2.0 + model_l2[:, None, None]))
    h0[:, :, m] = 2.0 / n

    def objective_grad(idx, X, g_ll):
        g = -g_ll
        g[:, :, :m] += pen[idx, None, None] * X[:, :, :m]
        if not np.isfinite(g).all():
            raise ValueError("a gradient is not finite (model %d): l2 is too small for this index, or the logits overflow fp32" % (
                idx[int(np.nonzero(~np.isfinite(g).all(axis=(1, 2)))[0][0])]))
        return g

    G = objective_grad(everyone, X, g_ll)
    n_train = stats[:, 0, 0].copy()
    state = [{"S": [], "Y": [], "d": None, "t": 1.0, "dd0": 0.0, "it": 0, "shrinks": 0, "stopped": None} for _ in range(M)]

    def direction(j):  # the two-loop recursion with the diagonal h0
        st, q = state[j], G[j].ravel().copy()
        al = []
        for sv, yv in zip(reversed(st["S"]), reversed(st["Y"])):
            a = float(sv @ q) / float(yv @ sv)
            al.append(a)
            q -= a * yv
        q *= h0[j].ravel()
        for (sv, yv), a in zip(zip(st["S"], st["Y"]), reversed(al)):
            q += (a - float(yv @ q) / float(yv @ sv)) * sv
        d = -q
        dd = float(G[j].ravel() @ d)
        if not dd < 0.0:  # (cannot happen with positive curvature pairs; start again from the diagonal)
            st["S"], st["Y"] = [], []
            d = -h0[j].ravel() * G[j].ravel()
            dd = float(G[j].ravel() @ d)
        st["d"], st["dd0"], st["t"], st["shrinks"] = d, dd, 1.0, 0

    def settle(j):  # after a new point: converged, out of iterations, or the next direction
        st = state[j]
        if float(np.abs(G[j]).max()) / max(n_train[j], 1.0) <= tol:
            st["stopped"] = "converged"
        elif st["it"] >= max_iter:
            st["stopped"] = "max_iter"
        else:
            direction(j)

    for j in range(M):
        settle(j)
    while True:
        idx = np.array([j for j in range(M) if state[j]["stopped"] is None], dtype=np.int64)
        if not len(idx):
            break
        trial = np.stack([X[j] + (state[j]["t"] * state[j]["d"]).reshape(C, m + 1) for j in idx])
        g_ll, st_new, _ = evaluate(idx, trial)
        g_new = objective_grad(idx, trial, g_ll)
        for a, j in enumerate(idx):
            st = state[j]
            dd1 = float(g_new[a].ravel() @ st["d"])
            if dd1 <= CLASS_SLACK * abs(st["dd0"]):
                sv, yv = st["t"] * st["d"], (g_new[a] - G[j]).ravel()
                if float(yv @ sv) > 0.0:
                    st["S"], st["Y"] = (st["S"] + [sv])[-CLASS_MEMORY:], (st["Y"] + [yv])[-CLASS_MEMORY:]
                X[j], G[j], stats[j], n_train[j] = trial[a], g_new[a], st_new[a], st_new[a, 0, 0]
                st["it"] += 1
                settle(j)
            elif st["shrinks"] >= CLASS_MAX_SHRINKS:
                st["stopped"] = "line_search"
            else:
                st["shrinks"] += 1
                st["t"] *= -st["dd0"] / (dd1 - st["dd0"])
    # selection: the least held-out Brier sum over the folds, ties to the larger strength
    conv = np.array([st["stopped"] == "converged" for st in state]).reshape(L, F + 1)
    held = stats[:, 1, :].reshape(L, F + 1, 3)[:, :F, :].sum(axis=1)  # [L, 3]: rows, hits, brier
    pick = 0
    if F:
        brier = np.where(np.isnan(held[:, 2]), np.inf, held[:, 2])
        order = np.argsort(-grid, kind="stable")
        pick = int(order[int(np.argmin(brier[order]))])  # (argmin: the first of equals, i.e. the larger strength)
    sel = np.arange(pick * (F + 1), (pick + 1) * (F + 1))
    prob = None
    if F:
        prob = run_pass(to_device(X[sel]), model_fold[sel], np.arange(F, dtype=np.int32))["prob"]
        passes += 1
    head_model = int(sel[-1])
    with np.errstate(divide="ignore", invalid="ignore"):
        path = {"l2": grid, "cv_accuracy": held[:, 1] / held[:, 0] if F else np.full(L, np.nan),
                "cv_brier": held[:, 2] / held[:, 0] if F else np.full(L, np.nan), "converged": conv.all(axis=1)}
    return {"n": n, "m": m, "mean": mean, "U": to_device(X[head_model]), "W": X[head_model].copy(), "V": V, "variance": s,
            "l2": float(grid[pick]), "pick": pick, "path": path, "stats": stats[head_model].copy(), "prob": prob, "class_count": count,
            "iterations": int(state[head_model]["it"]), "converged": bool(conv[pick].all()), "stopped": state[head_model]["stopped"],
            "passes": passes, "folds": F, "noise_floor": noise}


def class_head_result(fit, lab, classes, level, dim):
    """``fit_class_head``'s ``(result, head)`` from the optimiser's output"""
    C, N, F = len(classes), len(lab), fit["folds"]
    U = fit["U"]
    head = LatentClassHead(fit["mean"], U, classes, fit["l2"], level, dim)
    pick = fit["pick"]
    prob = fit["prob"] if F else np.full((N, C), np.nan, np.float32)
    confusion = np.zeros((C, C), np.int64)
    log_loss = float("nan")
    if F:
        ok = ~np.isnan(prob).any(axis=1) & (lab >= 0)
        pred = np.argmax(prob[ok], axis=1)  # (the first of equals)
        np.add.at(confusion, (lab[ok], pred), 1)
        with np.errstate(divide="ignore"):
            log_loss = float(-np.log(prob[ok, lab[ok]].astype(np.float64)).mean()) if ok.any() else float("nan")
    st = fit["stats"]
    result = {"l2": fit["l2"], "cv_accuracy": float(fit["path"]["cv_accuracy"][pick]), "cv_brier": float(fit["path"]["cv_brier"][pick]),
              "cv_log_loss": log_loss, "cv_confusion": confusion, "fit_accuracy": float(st[0, 1] / st[0, 0]),
              "class_count": fit["class_count"], "n_rows": fit["n"], "cv_probability": prob, "weights": np.ascontiguousarray(U[:, :dim]),
              "intercept": np.ascontiguousarray(U[:, dim]), "iterations": fit["iterations"], "converged": fit["converged"],
              "stopped": fit["stopped"], "passes": fit["passes"], "classes": np.asarray(classes, np.int64), "path": fit["path"]}
    return result, head


class LatentClassHead(SavedResult):
    """A classification head on one level of one model, as ``LatentIndex.fit_class_head`` fits it: the logits a_k = intercept_k + (x -
    mean) . W_k and their softmax.  mean [dim], weights [C, dim + 1] fp32 (the intercept in the last column), classes int64 [C] (the label
    value of every class), l2 the strength it was fitted with."""
    NOUN, KIND = "head", "class_head"  # (the tag tells its file from a LatentHead's, whose keys it shares in part)
    FIELDS = saved_fields("mean", "weights", "classes", ("l2", AS_FLOAT))

    def __init__(self, mean, weights, classes, l2, level, dim=None):
        if level not in LEVELS:
            raise ValueError("level must be one of %s, got %r" % (", ".join(LEVELS), level))
        try:
            w = np.ascontiguousarray(weights, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError("weights must be an array of numbers") from None
        if w.ndim != 2:
            raise ValueError("weights must have shape [C, dim + 1], got %s" % (w.shape,))
        self.mean, w3, _, _, _ = _hip.check_logit_args(mean, w[None], None, 0, None, dim)
        self.weights = w3[0]
        cl = np.asarray(classes)
        if cl.dtype.kind not in "iu" or cl.shape != (w.shape[0],) or len(np.unique(cl)) != len(cl):
            raise ValueError("classes must hold %d distinct integers, got %r" % (w.shape[0], classes))
        self.classes = cl.astype(np.int64)
        try:
            self.l2 = float(l2)
        except (TypeError, ValueError):
            raise ValueError("l2 must be a number, got %r" % (l2,)) from None
        self.level, self.dim = level, int(self.mean.shape[0])

    @property
    def c(self):
        return int(self.weights.shape[0])

    def finish(self, prob):
        """the device's probabilities [n, C] as {"probability", "label" (the class value of the largest, the first of equals),
        "confidence" (that probability), "entropy" (nats; fp64 on the host, 0 log 0 = 0)}"""
        p = prob.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ent = -np.where(p > 0, p * np.log(p), np.where(np.isnan(p), np.nan, 0.0)).sum(axis=1)
        best = np.argmax(np.where(np.isnan(prob), -np.inf, prob), axis=1) if len(prob) else np.zeros(0, np.int64)
        return {"probability": prob, "label": self.classes[best], "confidence": prob[np.arange(len(prob)), best].astype(np.float32),
                "entropy": ent.astype(np.float32)}


KERNEL_BANDWIDTH_FACTORS = (1.0, 2.0, 4.0, 8.0, 16.0, 32.0)  # bandwidth="loo": h^2 over the squared covering radius
KERNEL_MAX_BANDWIDTHS = 8


def kernel_landmarks_arg(landmarks, n_rows):
    """``landmarks`` of ``fit_kernel_head`` checked: (m, None) for a count, (m, positions int64 [m]) for an integer array of distinct
    positions in 0 .. n_rows - 1; ValueError otherwise"""
    top = _hip.RBF_MAX_LANDMARKS
    if isinstance(landmarks, (int, np.integer)) and not isinstance(landmarks, bool):
        if not 1 <= int(landmarks) <= top:
            raise ValueError("landmarks must be a count in 1 .. %d or an array of positions, got %r" % (top, landmarks))
        return int(landmarks), None
    a = np.asarray(landmarks)
    if a.dtype.kind not in "iu" or a.ndim != 1 or not 1 <= a.shape[0] <= top:
        raise ValueError("landmarks must be a count in 1 .. %d or an array of as many integer positions, got %r" % (top, landmarks))
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= int(n_rows) or len(np.unique(a)) != len(a):
        raise ValueError("landmarks must name distinct positions in 0 .. %d, got %d of them in %d .. %d" % (int(n_rows) - 1, len(a), a.min(), a.max()))
    return int(a.shape[0]), a


def kernel_bandwidth_arg(bandwidth):
    """``bandwidth`` of ``fit_kernel_head`` checked: None for "loo", else the fp64 distances [G], 1 <= G <= 8, each with a valid gamma
    (``_hip.rbf_gamma``); ValueError otherwise"""
    what = '"loo", a positive distance or a sequence of at most %d' % KERNEL_MAX_BANDWIDTHS
    if isinstance(bandwidth, str):
        if bandwidth != "loo":
            raise ValueError("bandwidth must be %s, got %r" % (what, bandwidth))
        return None
    try:
        h = np.atleast_1d(np.asarray(bandwidth, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError("bandwidth must be %s, got %r" % (what, bandwidth)) from None
    if isinstance(bandwidth, bool) or h.ndim != 1 or not 1 <= h.shape[0] <= KERNEL_MAX_BANDWIDTHS:
        raise ValueError("bandwidth must be %s, got %r" % (what, bandwidth))
    for x in h:
        _hip.rbf_gamma(x)
    return h


def kernel_bandwidths(bandwidth, R2):
    """The bandwidths to try, fp64 [G]: the caller's, or for "loo" sqrt(R2 f) over KERNEL_BANDWIDTH_FACTORS with R2 the squared
    covering radius of the landmarks (fp32, as the selection reports it); ValueError for "loo" with an R2 that is 0 or not finite"""
    h = kernel_bandwidth_arg(bandwidth)
    if h is not None:
        return h
    if not (np.isfinite(R2) and R2 > 0.0):
        raise ValueError("the landmarks' squared covering radius is %r: every other usable row coincides with a landmark (or lies "
                         "infinitely far), so there is no scale for a bandwidth" % (R2,))
    h = np.sqrt(float(R2) * np.asarray(KERNEL_BANDWIDTH_FACTORS, dtype=np.float64))
    for x in h:
        _hip.rbf_gamma(x)
    return h


def kernel_head_result(run, hs, Z, R2, positions, ids, atoms, t, names, level, dim):
    """``fit_kernel_head``'s ``(result, head)``: ``run(gamma)`` -> (closed form, second leave-one-out pass, picks) on the features of
    one bandwidth, tried for every bandwidth of ``hs``; the score is the fp64 sum over the targets with variance of sse / tss, the
    least wins, ties to the larger h."""
    G, K = len(hs), t.shape[1]
    kk = np.arange(K)
    path = {"bandwidth": np.asarray(hs, dtype=np.float64).copy(), "loo_rmse": np.zeros((G, K)), "loo_r2": np.zeros((G, K))}
    best = None
    for g in np.argsort(-path["bandwidth"], kind="stable"):  # larger h first: a later one must be strictly better
        gamma = _hip.rbf_gamma(hs[g])
        fit, loo, pick = run(gamma)
        n = fit["n"]
        sse, tss = loo["sse"][pick, kk], fit["tvar"] * (n - 1.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            path["loo_rmse"][g], path["loo_r2"][g] = np.sqrt(sse / n), 1.0 - sse / tss
        score = sum(float(sse[k]) / float(tss[k]) for k in range(K) if tss[k] != 0)  # fp64, the targets in order
        score = np.inf if np.isnan(score) else score
        if best is None or score < best[0]:
            best = (score, g, gamma, fit, loo, pick)
    _, g, gamma, fit, loo, pick = best
    result, inner = head_result(fit, loo, pick, t, names, level, Z.shape[0])
    head = LatentKernelHead(Z, gamma, inner, level, dim, names)
    positions = np.asarray(positions)
    result.update({"bandwidth": float(hs[g]), "landmark_position": positions.astype(np.int32), "landmark_id": np.asarray(ids)[positions],
                   "landmark_atom": np.asarray(atoms)[positions], "covering_radius": float(np.sqrt(np.float64(R2))), "bandwidth_path": path})
    return result, head


class LatentKernelHead(SavedResult):
    """A ridge head on the Gaussian features of one level of one model, as ``LatentIndex.fit_kernel_head`` fits it: phi_c(x) =
    2^(-|x - z_c|^2 gamma) to the landmarks z [m, dim], and ``head`` -- a ``LatentHead`` over the m features (its ``dim`` is m):
    prediction_k = tmean_k + (phi - mean) . W_k, leverage_k as there, std_k = sqrt(sigma2_k (1 + leverage_k)), the predictive standard
    deviation of sparse Gaussian process regression with this basis.  ``gamma`` is the fp32 value log2(e) / (2 h^2) the device uses."""
    NOUN = "kernel head"
    # one flat file: the inner head's fields (all but its names) at top level beside the landmarks
    FIELDS = saved_fields("landmarks", ("gamma", AS_FLOAT32)) + saved_fields(
        "mean", "tmean", "weights", "components", "scale", ("lev0", AS_FLOAT), "sigma2", "l2", of="head.") + saved_fields(("names", AS_NAMES))

    def __init__(self, landmarks, gamma, head, level, dim=None, names=None):
        if level not in LEVELS:
            raise ValueError("level must be one of %s, got %r" % (", ".join(LEVELS), level))
        if not isinstance(head, LatentHead):
            raise ValueError("head must be a LatentHead over the features, got %r" % (type(head).__name__,))
        self.landmarks, self.gamma = _hip.check_rbf_args(landmarks, gamma, dim)
        if head.dim != self.landmarks.shape[0]:
            raise ValueError("the head regresses on %d features, there are %d landmarks" % (head.dim, self.landmarks.shape[0]))
        self.head, self.level, self.dim = head, level, int(self.landmarks.shape[1])
        self.names = list(head.names) if names is None else [str(x) for x in names]
        if len(self.names) != head.k:
            raise ValueError("names: %d for %d targets" % (len(self.names), head.k))

    @property
    def k(self):
        return self.head.k

    @property
    def m(self):
        return int(self.landmarks.shape[0])

    @property
    def bandwidth(self):
        """h of exp(-d^2 / 2 h^2), from the stored gamma"""
        return float(np.sqrt(np.log2(np.e) / (2.0 * self.gamma)))

    @classmethod
    def from_saved(cls, v, level, dim):
        landmarks, gamma, names = v.pop("landmarks"), v.pop("gamma"), v.pop("names")
        return cls(landmarks, gamma, LatentHead(*v.values(), level, None, names), level, dim, names)

    def finish(self, pred, lev, phi):
        """the device's pred, lev [n, K] and phi [n, m] as {"prediction", "std", "leverage", "support"}: support is the largest
        feature of the row -- how close it lies to its nearest landmark, in [0, 1]"""
        out = self.head.finish(pred, lev)
        out["support"] = phi.max(axis=1) if phi.shape[0] else np.zeros(0, np.float32)
        return out


class LatentProjection(SavedResult):
    """A principal-component map of one level of one model: mean [dim], components [m, dim] (fp32, rows), their variances (fp64) and the
    noise floor below which a variance cannot be told from 0.  ``scale`` [m] fp32 is 1 / sqrt(variance) above the floor and 0 at or
    below it, so such a component adds nothing to the Mahalanobis distance; ``rank`` counts the components above it."""
    NOUN = "projection"
    FIELDS = saved_fields("mean", "components", "variance", ("noise_floor", AS_FLOAT))

    def __init__(self, mean, components, variance, noise_floor, level, dim=None):
        if level not in LEVELS:
            raise ValueError("level must be one of %s, got %r" % (", ".join(LEVELS), level))
        self.mean, self.components, _ = _hip.check_pca_args(mean, components, None, dim)
        try:
            self.variance = np.ascontiguousarray(variance, dtype=np.float64)
            self.noise_floor = float(noise_floor)
        except (TypeError, ValueError):
            raise ValueError("variance must be an array of numbers and noise_floor a number") from None
        if self.variance.shape != (self.components.shape[0],) or not np.isfinite(self.variance).all():
            raise ValueError("variance must hold one finite value per component (%d), got shape %s" % (self.components.shape[0], self.variance.shape))
        if not self.noise_floor >= 0.0 or not np.isfinite(self.noise_floor):
            raise ValueError("noise_floor must be a finite number >= 0, got %r" % (noise_floor,))
        self.level, self.dim = level, int(self.mean.shape[0])
        above = self.variance > self.noise_floor
        self.scale = np.where(above, 1.0 / np.sqrt(np.where(above, self.variance, 1.0)), 0.0).astype(np.float32)
        self.rank = int(above.sum())

    @property
    def m(self):
        return int(self.components.shape[0])

    def finish(self, r):
        """the device's {"coords", "md2", "dist2"} as the rows the callers report: square roots taken on the host (correctly rounded, as
        ``nearest`` reports distances), NaN where the distance to the mean is not finite"""
        bad = ~np.isfinite(r["dist2"])
        coords, md, dist = r["coords"].copy(), np.sqrt(r["md2"]), np.sqrt(r["dist2"])
        coords[bad], md[bad], dist[bad] = np.nan, np.nan, np.nan
        return {"coordinates": coords, "mahalanobis": md, "distance_to_mean": dist}


class LatentClustering(SavedResult):
    """The centres of a clustering of one level of one model: what ``HipModel.assign`` assigns new inputs to."""
    NOUN = "clustering"
    FIELDS = saved_fields("centres")

    def __init__(self, centres, level, dim=None):
        centres = np.ascontiguousarray(centres, dtype=np.float32)
        if level not in LEVELS:
            raise ValueError("level must be one of %s, got %r" % (", ".join(LEVELS), level))
        if centres.ndim != 2 or not 1 <= centres.shape[0] <= _hip.KMEANS_MAX_K or (dim is not None and centres.shape[1] != int(dim)):
            raise ValueError("centres must be an array of 1 .. %d rows%s, got shape %s" % (
                _hip.KMEANS_MAX_K, "" if dim is None else " of %d columns" % int(dim), centres.shape))
        if not np.isfinite(centres).all():
            raise ValueError("centres hold a non-finite value")
        self.centres, self.level, self.dim = centres, level, int(centres.shape[1])
        self._index = None  # the centres as an index on a model's GPU (index_on)

    @property
    def k(self):
        return int(self.centres.shape[0])

    @classmethod
    def saved_fits(cls, v, dim):
        return v["centres"].ndim == 2 and v["centres"].shape[1] == dim

    def index_on(self, model):
        """The centres as a ``LatentIndex`` on ``model``'s GPU, centre c at position c with id c (built once per model and kept)."""
        self.check_model(model)
        if self._index is None or self._index.model is not model:
            self.free()
            self._index = LatentIndex(model, self.level).add_rows(self.centres)
        return self._index

    def free(self):
        if self._index is not None:
            self._index.free()
        self._index = None


EMBED_NEIGHBOURS = 31       # neighbours of a row in the affinity graph: one search with k = 32 less the row itself
EMBED_PERPLEXITY = (2, 15)  # the perplexities 31 neighbours carry
EMBED_BISECTIONS = 64       # steps of the precision search, fixed
EMBED_BETA_CAP = 2.0 ** 40  # the largest precision, in units of 1 / (the row's mean shifted squared distance)


def embed_fit_args(perplexity, iterations, exaggeration, learning_rate, route):
    """The arguments of ``LatentIndex.embed`` checked: (perplexity, (n_early, n_late), exaggeration, route); ValueError otherwise"""
    try:
        perp = float(perplexity)
    except (TypeError, ValueError):
        raise ValueError("perplexity must be a number in %d .. %d, got %r" % (EMBED_PERPLEXITY + (perplexity,))) from None
    if isinstance(perplexity, bool) or not EMBED_PERPLEXITY[0] <= perp <= EMBED_PERPLEXITY[1]:
        raise ValueError("perplexity must be a number in %d .. %d, got %r" % (EMBED_PERPLEXITY + (perplexity,)))
    try:
        its = tuple(iterations)
    except TypeError:
        raise ValueError("iterations must be two integers in 0 .. %d, got %r" % (_hip.EMBED_MAX_ITER, iterations)) from None
    if len(its) != 2 or any(isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= _hip.EMBED_MAX_ITER for n in its):
        raise ValueError("iterations must be two integers in 0 .. %d, got %r" % (_hip.EMBED_MAX_ITER, iterations))
    try:
        ex = float(exaggeration)
    except (TypeError, ValueError):
        raise ValueError("exaggeration must be a finite number > 0, got %r" % (exaggeration,)) from None
    if isinstance(exaggeration, bool) or not (math.isfinite(ex) and ex > 0):
        raise ValueError("exaggeration must be a finite number > 0, got %r" % (exaggeration,))
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise ValueError('learning_rate must be "auto" or a finite number > 0, got %r' % (learning_rate,))
    else:
        try:
            lr = float(learning_rate)
        except (TypeError, ValueError):
            raise ValueError('learning_rate must be "auto" or a finite number > 0, got %r' % (learning_rate,)) from None
        if isinstance(learning_rate, bool) or not (math.isfinite(lr) and lr > 0):
            raise ValueError('learning_rate must be "auto" or a finite number > 0, got %r' % (learning_rate,))
    if route not in ("device", "host"):
        raise ValueError('route must be "device" or "host", got %r' % (route,))
    return perp, (int(its[0]), int(its[1])), ex, route


def neighbour_graph(index, chunk=4096, strict=True):
    """For every row of ``index`` its nearest other rows -- 31, or all others in a smaller index --: (position int32 [N, K], dist2 fp32
    [N, K]), nearest first.  The rows are searched ``chunk`` at a time, where they lie on the device, with k = 32 and no id skipping
    (``Engine.index_query_rows``, the bits of ``Engine.index_read`` + ``Engine.index_query``, which is what an engine without that call
    is asked for: the CPU stand-ins of the tests only, the route is never taken with ``Engine``): bits and total order are the search's.  From a row's answer its own position is
    dropped where it appears, otherwise (33 or more coincident rows) the last place.  ValueError for a row with a non-finite component
    (``strict`` False: no such check, an overflowed distance stays +inf; ``hierarchy`` passes rows without a non-finite component)."""
    eng, ix = index.model.engine, index._ix
    N = len(index)
    k = min(EMBED_NEIGHBOURS + 1, N)
    if k < 2:
        raise ValueError("a neighbour graph needs at least 2 rows, the index has %d" % N)
    pos, d2 = np.empty((N, k - 1), np.int32), np.empty((N, k - 1), np.float32)
    for a in range(0, N, int(chunk)):
        b = min(N, a + int(chunk))
        r = eng.index_query_rows(ix, a, b - a, k) if hasattr(eng, "index_query_rows") else eng.index_query(ix, eng.index_read(ix, a, b - a)[0], k)
        own = r["position"] == np.arange(a, b, dtype=np.int32)[:, None]
        drop = np.where(own.any(axis=1), own.argmax(axis=1), k - 1)
        keep = np.ones((b - a, k), bool)
        keep[np.arange(b - a), drop] = False
        pos[a:b] = r["position"][keep].reshape(b - a, k - 1)
        d2[a:b] = r["dist2"][keep].reshape(b - a, k - 1)
    if strict and ((pos < 0).any() or not np.isfinite(d2).all()):
        raise ValueError("row %d has no %d neighbours at a finite distance: rows with a non-finite component cannot be embedded" % (
            int(np.nonzero((pos < 0).any(axis=1) | ~np.isfinite(d2).all(axis=1))[0][0]), k - 1))
    return pos, d2


def neighbour_graph_host(rows, chunk=1024, strict=True):
    """``neighbour_graph`` of host rows [N, dim] without a GPU: the search's distances (``_hip.knn_dist2_matrix``) ranked by (distance,
    position), the search's total order, so the same bits and places."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    N = rows.shape[0]
    k = min(EMBED_NEIGHBOURS + 1, N)
    if rows.ndim != 2 or k < 2:
        raise ValueError("a neighbour graph needs rows [N, dim] with N >= 2, got shape %s" % (rows.shape,))
    pos, d2 = np.empty((N, k - 1), np.int32), np.empty((N, k - 1), np.float32)
    for a in range(0, N, int(chunk)):
        b = min(N, a + int(chunk))
        d = _hip.knn_dist2_matrix(rows[a:b], rows)
        order = np.argsort(d, axis=1, kind="stable")[:, :k]  # (stable: equal distances stay in position order)
        own = order == np.arange(a, b)[:, None]
        drop = np.where(own.any(axis=1), own.argmax(axis=1), k - 1)
        keep = np.ones((b - a, k), bool)
        keep[np.arange(b - a), drop] = False
        pos[a:b] = order[keep].reshape(b - a, k - 1)
        d2[a:b] = np.take_along_axis(d, order, axis=1)[keep].reshape(b - a, k - 1)
    if strict and not np.isfinite(d2).all():
        raise ValueError("row %d has no %d neighbours at a finite distance: rows with a non-finite component cannot be embedded" % (
            int(np.nonzero(~np.isfinite(d2).all(axis=1))[0][0]), k - 1))
    return pos, d2


def embed_rows_host(rows, perplexity=10, iterations=(250, 500), exaggeration=12.0, learning_rate="auto", ids=None, atoms=None, level="structure",
                    graph=None):
    """``LatentIndex.embed`` of host rows [N, dim] entirely on the host, no GPU: the twins of the moments, the projection, the search's
    distances and the iteration -- bit for bit what an index holding these rows gives by either route."""
    perplexity, iterations, exaggeration, _ = embed_fit_args(perplexity, iterations, exaggeration, learning_rate, "host")
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[1] < 2:
        raise ValueError("rows must have shape [N, dim] with dim >= 2, got %s" % (rows.shape,))
    N, dim = rows.shape
    if N > _hip.EMBED_MAX_ROWS:
        raise ValueError("%d rows, an embedding takes at most %d" % (N, _hip.EMBED_MAX_ROWS))
    if N - 1 <= perplexity or N < 3:
        raise ValueError("perplexity %g needs more than %d rows, got %d" % (perplexity, int(perplexity) + 1, N))
    lr = max(200.0, N / 12.0) if isinstance(learning_rate, str) else float(learning_rate)
    mo = _hip.moments_host(rows)
    _, v, _ = _hip.sym_eig(mo["cov"])
    y0 = embed_initial_layout(_hip.project_host(rows, mo["mean"], v[:2].astype(np.float32))["coords"])
    pos, d2 = neighbour_graph_host(rows) if graph is None else graph
    row_first, col, p = embed_affinities(d2, pos, perplexity)
    ids = np.arange(N, dtype=np.int64) if ids is None else ids
    atoms = np.full(N, -1, np.int32) if atoms is None else atoms
    step = functools.partial(_hip.embed_iterate_host, row_first, col, p)
    return embed_run(step, y0, row_first, col, p, iterations, exaggeration, lr, pos, d2, ids, atoms, perplexity, level, dim)


def embed_conditional(dist2, perplexity):
    """The conditional distribution of every row over its K neighbours, fp64 [n, K]: p_j = exp(-beta d_j) / sum, d_j the squared
    distance less the row's least one, beta found per row by ``EMBED_BISECTIONS`` = 64 steps -- doubling until the entropy falls below
    log(perplexity), then halving the bracket -- in units of 1 / (the row's mean d; 1 if that is 0) and capped at ``EMBED_BETA_CAP`` =
    2^40 of them.  A row whose distances are all equal has the entropy log K at every beta, ends at the cap and stays uniform and
    finite; so does a row of zeros.  ValueError unless the perplexity lies below K."""
    d = np.asarray(dist2, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] < 2 or not np.isfinite(d).all():
        raise ValueError("dist2 must be a finite array [n, K] with K >= 2, got shape %s" % (d.shape,))
    perp = float(perplexity)
    if not 1.0 < perp < d.shape[1]:
        raise ValueError("perplexity %g must lie above 1 and below the %d neighbours" % (perp, d.shape[1]))
    d = d - d.min(axis=1, keepdims=True)
    scale = d.mean(axis=1, keepdims=True)
    d = d / np.where(scale > 0, scale, 1.0)
    target = math.log(perp)
    n = d.shape[0]
    lo, hi, beta = np.zeros((n, 1)), np.full((n, 1), np.inf), np.ones((n, 1))
    for _ in range(EMBED_BISECTIONS):
        w = np.exp(-beta * d)
        s = w.sum(axis=1, keepdims=True)  # >= 1: the nearest neighbour's weight is 1
        H = np.log(s) + beta * (d * w).sum(axis=1, keepdims=True) / s
        high = H > target  # too flat: a larger beta
        lo = np.where(high, beta, lo)
        hi = np.where(high, hi, beta)
        beta = np.minimum(np.where(np.isinf(hi), beta * 2.0, (lo + hi) / 2.0), EMBED_BETA_CAP)
    w = np.exp(-beta * d)
    return w / w.sum(axis=1, keepdims=True)


def embed_affinities(dist2, pos, perplexity):
    """The symmetric affinities of a neighbour graph (``neighbour_graph``'s position and dist2 [N, K]) as the iteration takes them:
    ``(row_first int64 [N + 1], col int32 [E], p fp32 [E])``, CSR with columns ascending over the union of the edges i -> j and j -> i,
    p_ij = (float)((p_j|i + p_i|j) / (2 N)) from ``embed_conditional`` in fp64 (an edge stored one way only has the other term 0)."""
    pos = np.asarray(pos)
    if pos.dtype.kind not in "iu" or pos.ndim != 2 or pos.shape != np.shape(dist2):
        raise ValueError("pos must be an integer array of dist2's shape %s, got %s %s" % (np.shape(dist2), pos.dtype, pos.shape))
    N, K = pos.shape
    own = np.arange(N, dtype=np.int64)[:, None]
    if (pos < 0).any() or (pos >= N).any() or (pos == own).any():
        raise ValueError("pos must hold positions in 0 .. %d other than the row's own" % (N - 1))
    P = embed_conditional(dist2, perplexity)
    i, j = np.broadcast_to(own, (N, K)).ravel(), pos.astype(np.int64).ravel()
    key = np.concatenate([i * N + j, j * N + i])
    val = np.concatenate([P.ravel(), P.ravel()])
    order = np.argsort(key, kind="stable")
    key, val = key[order], val[order]
    first = np.concatenate([[True], key[1:] != key[:-1]])
    start = np.nonzero(first)[0]
    total = np.add.reduceat(val, start)  # (one or two terms per edge: no order to speak of)
    edge = key[start]
    row, col = edge // N, (edge % N).astype(np.int32)
    row_first = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=N), out=row_first[1:])
    return row_first, col, (total / (2.0 * N)).astype(np.float32)


def embed_initial_layout(coords):
    """``pca(2)``'s coordinates [N, 2] scaled so that the first column's standard deviation is 1e-4, fp32; mean and variance are exactly
    rounded sums (``math.fsum``), the scaling one fp64 product per value.  ValueError for a non-finite coordinate or no spread."""
    c = np.asarray(coords, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != 2:
        raise ValueError("coords must have shape [N, 2], got %s" % (c.shape,))
    if not np.isfinite(c).all():
        raise ValueError("row %d has a non-finite component: it cannot be embedded" % int(np.nonzero(~np.isfinite(c).all(axis=1))[0][0]))
    mean = math.fsum(c[:, 0]) / len(c)
    std = math.sqrt(math.fsum((c[:, 0] - mean) ** 2) / len(c))
    if not std > 0.0:
        raise ValueError("the rows have no spread along their first principal axis: nothing to embed")
    return (c * (1e-4 / std)).astype(np.float32)


def embed_kl(coords, row_first, col, p, z):
    """The Kullback-Leibler divergence of a layout over the stored edges, fp64: sum of p log(p / q) with q = 1 / ((1 + |y_i - y_j|^2) z),
    edges with p = 0 left out."""
    y = np.asarray(coords, dtype=np.float64)
    row = np.repeat(np.arange(len(y)), np.diff(row_first))
    pv = np.asarray(p, dtype=np.float64)
    live = pv > 0
    diff = y[row[live]] - y[np.asarray(col)[live]]
    q = 1.0 / ((1.0 + (diff * diff).sum(axis=1)) * float(z))
    return float(np.sum(pv[live] * np.log(pv[live] / q)))


def embed_run(step, y0, row_first, col, p, iterations, exaggeration, lr, pos, d2, ids, atoms, perplexity, level, dim):
    """``LatentIndex.embed`` behind the graph: the two phases through ``step(y, u, gain, n_iter, exaggeration, momentum, lr)`` --
    ``Engine.embed_iterate`` or ``_hip.embed_iterate_host`` with the graph bound -- and the result"""
    u, gain = np.zeros_like(y0), np.ones_like(y0)
    z_init = step(y0, u, gain, 1, 1.0, 0.8, lr)["z"]  # (the Z of the layout the call starts from; its step is dropped)
    st = step(y0, u, gain, iterations[0], exaggeration, 0.5, lr)
    st = step(st["y"], st["u"], st["gain"], iterations[1], 1.0, 0.8, lr)
    z = step(st["y"], st["u"], st["gain"], 1, 1.0, 0.8, lr)["z"]
    coords = st["y"]
    if not np.isfinite(coords).all():
        raise ValueError("the embedding left the range of fp32: the learning rate %g is too large for this index" % lr)
    emb = LatentEmbedding(coords, ids, atoms, perplexity, level, dim)
    result = {"coords": coords, "kl_init": embed_kl(y0, row_first, col, p, z_init), "kl": embed_kl(coords, row_first, col, p, z), "z": z,
              "neighbor_position": pos, "neighbor_dist2": d2, "n_edges": int(row_first[-1]), "learning_rate": float(np.float32(lr))}
    return result, emb


class LatentEmbedding(SavedResult):
    """A neighbour embedding of one level of one model, as ``LatentIndex.embed`` fits it: the map coordinates fp32 [N, 2] of the index's
    rows in position order, their ids and atoms, and the perplexity new rows are placed with."""
    NOUN = "embedding"
    FIELDS = saved_fields("coordinates", "ids", "atoms", ("perplexity", AS_FLOAT))

    def __init__(self, coordinates, ids, atoms, perplexity, level, dim):
        if level not in LEVELS:
            raise ValueError("level must be one of %s, got %r" % (", ".join(LEVELS), level))
        try:
            self.coordinates = np.ascontiguousarray(coordinates, dtype=np.float32)
            self.ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
            self.atoms = np.ascontiguousarray(atoms, dtype=np.int32).reshape(-1)
            self.perplexity = float(perplexity)
        except (TypeError, ValueError):
            raise ValueError("coordinates, ids and atoms must be arrays of numbers and perplexity a number") from None
        n = self.coordinates.shape[0]
        if self.coordinates.ndim != 2 or self.coordinates.shape[1] != 2 or n < 2 or not np.isfinite(self.coordinates).all():
            raise ValueError("coordinates must be a finite array [N, 2] with N >= 2, got shape %s" % (self.coordinates.shape,))
        if self.ids.shape != (n,) or self.atoms.shape != (n,):
            raise ValueError("ids %s and atoms %s must hold one entry per row (%d)" % (self.ids.shape, self.atoms.shape, n))
        if not EMBED_PERPLEXITY[0] <= self.perplexity <= EMBED_PERPLEXITY[1]:
            raise ValueError("perplexity must lie in %d .. %d, got %r" % (EMBED_PERPLEXITY + (perplexity,)))
        self.level, self.dim = level, int(dim)

    def __len__(self):
        return int(self.coordinates.shape[0])

    def check_index(self, index):
        """ValueError unless ``index`` can be the one the embedding maps: its level, width and number of rows"""
        if not isinstance(index, LatentIndex):
            raise ValueError("index must be a LatentIndex, got %r" % (type(index).__name__,))
        if index.level != self.level or index.dim != self.dim or len(index) != len(self):
            raise ValueError("a %s-level embedding of %d rows of %d columns does not map a %s-level index of %d rows of %d" % (
                self.level, len(self), self.dim, index.level, len(index), index.dim))

    def place(self, position, dist2):
        """New rows from their nearest index rows ([n, k] positions and squared distances, nearest first): ``LatentIndex.place``'s dict.
        With fewer neighbours than the perplexity needs (a tiny index) the weights are uniform."""
        position, dist2 = np.asarray(position), np.asarray(dist2, dtype=np.float32)
        n, k = position.shape
        if (position < 0).any() or not np.isfinite(dist2).all():
            raise ValueError("row %d has no %d index rows at a finite distance" % (
                int(np.nonzero((position < 0).any(axis=1) | ~np.isfinite(dist2).all(axis=1))[0][0]), k))
        w = embed_conditional(dist2, self.perplexity) if n and k > self.perplexity else np.full((n, k), 1.0 / max(k, 1))
        coords = np.einsum("nk,nkc->nc", w, self.coordinates[position].astype(np.float64)).astype(np.float32)
        first = position[:, 0]
        return {"coords": coords, "nearest_position": first.astype(np.int32), "nearest_id": self.ids[first], "nearest_atom": self.atoms[first],
                "nearest_distance": np.sqrt(dist2[:, 0])}  # (correctly rounded on the host, as nearest reports distances)


PEAKS_NEIGHBOURS = EMBED_NEIGHBOURS  # the farthest neighbour the automatic bandwidth can look at: what ``neighbour_graph`` returns


class _CoordIndex:
    """Map coordinates [N, c] as a temporary index on ``model``'s GPU handle, with what ``neighbour_graph`` asks of an index"""

    def __init__(self, model, coords):
        self.model = model
        self._ix = model.engine.index_create(coords.shape[1])
        try:
            model.engine.index_add(self._ix, coords)
        except Exception:
            self._ix.free()
            raise

    def __len__(self):
        return len(self._ix)

    def free(self):
        self._ix.free()


def map_coords_arg(coords, index=None, n_rows=None):
    """The coordinates of a map as fp32 [N, c]: an array, a ``LatentEmbedding`` (checked against ``index``), the result dict of
    ``embed`` ("coords") or ``pca`` ("coordinates"), or the pair either returns; ValueError unless they are finite and one per row"""
    if isinstance(coords, tuple) and len(coords) == 2 and isinstance(coords[0], dict):
        coords = coords[0]
    if isinstance(coords, LatentEmbedding):
        if index is not None:
            coords.check_index(index)
        coords = coords.coordinates
    elif isinstance(coords, dict):
        if "coords" not in coords and "coordinates" not in coords:
            raise ValueError('a result dict must hold "coords" (embed) or "coordinates" (pca)')
        coords = coords["coords"] if "coords" in coords else coords["coordinates"]
    try:
        c = np.ascontiguousarray(coords, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("coords must be an array of numbers [N, c]") from None
    n = len(index) if index is not None else n_rows
    if c.ndim != 2 or c.shape[1] < 1 or c.shape[1] > 1024 or (n is not None and c.shape[0] != int(n)):
        raise ValueError("coords must have shape [%s, c] with c in 1 .. 1024, one row per row of the index, got %s" % (
            "N" if n is None else int(n), c.shape))
    if not np.isfinite(c).all():
        raise ValueError("coords: row %d has a non-finite component" % int(np.nonzero(~np.isfinite(c).all(axis=1))[0][0]))
    return c


def map_quality_k_arg(k, n_rows):
    """``k`` of ``map_quality`` checked against the number of rows: 1 .. K = min(31, N - 2) with 2N - 3k - 1 > 0; ValueError otherwise"""
    K = min(EMBED_NEIGHBOURS, int(n_rows) - 2)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= K:
        raise ValueError("k must be an integer in 1 .. %d (min(%d, N - 2) with N = %d rows), got %r" % (K, EMBED_NEIGHBOURS, int(n_rows), k))
    if 2 * int(n_rows) - 3 * int(k) - 1 <= 0:
        raise ValueError("k = %d is too large for %d rows: the scores need 2N - 3k - 1 > 0" % (int(k), int(n_rows)))
    return int(k)


def map_quality_scores(rank_latent, rank_map, n_rows, k):
    """The scores of ``map_quality`` from the ranks, fp64 NumPy on integers: ``rank_latent`` int [n, K] the latent-space ranks of every
    scored row's map-neighbours, nearest first, ``rank_map`` the map ranks of its latent-neighbours"""
    rl, rm = np.asarray(rank_latent, np.int64), np.asarray(rank_map, np.int64)
    n, K = rl.shape
    N = int(n_rows)

    def at(r, kk):  # the integer penalties and hits of every row at kk
        head = r[:, :kk]
        return np.maximum(head + 1 - kk, 0).sum(axis=1), (head < kk).sum(axis=1)

    def coef(kk):
        return 2.0 / (kk * (2.0 * N - 3.0 * kk - 1.0)) if 2 * N - 3 * kk - 1 > 0 else float("nan")

    ks = np.arange(1, K + 1, dtype=np.int64)
    t_curve, c_curve, q_curve = np.empty(K), np.empty(K), np.empty(K)
    for kk in range(1, K + 1):
        pen_l, hit_l = at(rl, kk)
        pen_m, _ = at(rm, kk)
        t_curve[kk - 1] = 1.0 - coef(kk) * (float(int(pen_l.sum())) / n)
        c_curve[kk - 1] = 1.0 - coef(kk) * (float(int(pen_m.sum())) / n)
        q_curve[kk - 1] = float(int(hit_l.sum())) / (n * kk)
    pen_l, hit_l = at(rl, k)
    pen_m, hit_m = at(rm, k)
    kf = ks.astype(np.float64)
    rnx = ((N - 1) * q_curve - kf) / (N - 1 - kf)
    return {"k": int(k), "n_rows": N, "ks": ks,
            "row_trustworthiness": 1.0 - coef(k) * pen_l.astype(np.float64), "row_continuity": 1.0 - coef(k) * pen_m.astype(np.float64),
            "row_overlap": hit_l.astype(np.float64) / k,
            "trustworthiness": float(t_curve[k - 1]), "continuity": float(c_curve[k - 1]), "neighbour_overlap": float(q_curve[k - 1]),
            "trustworthiness_curve": t_curve, "continuity_curve": c_curve, "qnx_curve": q_curve,
            "lcmc": float(q_curve[k - 1] - k / (N - 1.0)), "rnx_auc": float(np.sum(rnx / kf) / np.sum(1.0 / kf)),
            "false_neighbours": (k - hit_l).astype(np.int32), "missed_neighbours": (k - hit_m).astype(np.int32),
            "rank_latent": rl.astype(np.int32), "rank_map": rm.astype(np.int32)}


def map_quality_run(graph_latent, graph_map, ranks_latent, ranks_map, n_rows, k, sample, seed):
    """The host work around the two rank passes of ``map_quality``, shared by the device and the host route.  ``graph_latent()`` and
    ``graph_map()`` give the neighbour graphs (position [N, >= K], dist2) of the two spaces, ``ranks_latent(probe, qpos or None)`` and
    ``ranks_map`` the ranks of ``probe`` [n, K] in each."""
    N = int(n_rows)
    K = min(EMBED_NEIGHBOURS, N - 2)
    if sample is None:
        qpos, position = None, np.arange(N, dtype=np.int32)
    elif isinstance(sample, int):
        if sample > N:
            raise ValueError("sample = %d, but there are only %d rows" % (sample, N))
        qpos = position = np.sort(np.random.default_rng(seed).choice(N, sample, replace=False)).astype(np.int32)
    else:
        qpos = position = sample
    pos_latent = np.ascontiguousarray(np.asarray(graph_latent()[0])[position, :K], dtype=np.int32)
    pos_map = np.ascontiguousarray(np.asarray(graph_map()[0])[position, :K], dtype=np.int32)
    if pos_latent.shape != (len(position), K):
        raise ValueError("graph must hold the positions [%d, >= %d] of neighbour_graph, got %s" % (N, K, np.shape(graph_latent()[0])))
    rank_latent, rank_map = ranks_latent(pos_map, qpos), ranks_map(pos_latent, qpos)
    if (rank_latent < 0).any() or (rank_map < 0).any():
        raise ValueError("row %d has a non-finite component: the map of such rows cannot be scored" % int(
            position[np.nonzero((rank_latent < 0).any(axis=1) | (rank_map < 0).any(axis=1))[0][0]]))
    out = map_quality_scores(rank_latent, rank_map, N, k)
    out["position"] = position
    return out


def map_quality_rows_host(rows, coords, k=15, sample=None, seed=0, graph=None):
    """``LatentIndex.map_quality`` without a GPU: the host twins (``neighbour_graph_host``, ``_hip.ranks_host``) on ``rows`` [N, dim]
    and ``coords`` [N, c]; the same dict, bit for bit."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[1] < 1:
        raise ValueError("rows must be [N, dim], got shape %s" % (rows.shape,))
    coords = map_coords_arg(coords, n_rows=len(rows))
    k = map_quality_k_arg(k, len(rows))
    sample = silhouette_sample_arg(sample, seed, len(rows))
    return map_quality_run(lambda: neighbour_graph_host(rows) if graph is None else graph, lambda: neighbour_graph_host(coords),
                           lambda probe, q: _hip.ranks_host(rows, probe, q)["rank"],
                           lambda probe, q: _hip.ranks_host(coords, probe, q)["rank"], len(rows), k, sample, seed)


def choose_perplexity_arg(perplexities):
    """``perplexities`` of ``choose_perplexity`` checked: a non-empty ascending list of distinct perplexities (each as ``embed`` takes it)"""
    try:
        ps = [float(p) for p in perplexities]
    except (TypeError, ValueError):
        raise ValueError("perplexities must be a list of numbers in %d .. %d, got %r" % (EMBED_PERPLEXITY + (perplexities,))) from None
    if not ps or any(isinstance(p, bool) for p in perplexities) or any(not EMBED_PERPLEXITY[0] <= p <= EMBED_PERPLEXITY[1] for p in ps) or any(
            b <= a for a, b in zip(ps, ps[1:])):
        raise ValueError("perplexities must be an ascending list of distinct numbers in %d .. %d, got %r" % (EMBED_PERPLEXITY + (perplexities,)))
    return ps


MAP_QUALITY_COLUMNS = ("neighbour_overlap", "trustworthiness", "continuity", "lcmc", "rnx_auc")


def choose_perplexity_run(embed, quality, linear, perplexities):
    """``choose_perplexity``'s table from ``embed(perplexity)``, ``quality(coords)`` and ``linear()`` (the coordinates of ``pca(2)``)
    over the ascending ``perplexities``"""
    table = {name: [] for name in MAP_QUALITY_COLUMNS + ("kl",)}
    best = None
    for p in perplexities:
        res, emb = embed(p)
        q = quality(res["coords"])
        for name in MAP_QUALITY_COLUMNS:
            table[name].append(q[name])
        table["kl"].append(res["kl"])
        if best is None or q["neighbour_overlap"] > best[2]["neighbour_overlap"]:  # (ascending: among equal scores the lower stays)
            best = (p, res, q, emb)
    q = quality(linear())
    for name in MAP_QUALITY_COLUMNS:
        table[name].append(q[name])
    table["kl"].append(float("nan"))
    out = {name: np.asarray(v, np.float64) for name, v in table.items()}
    out.update({"perplexity": list(perplexities) + ["linear"], "best_perplexity": best[0], "best": best[1], "quality": best[2]})
    return out, best[3]


def choose_perplexity_rows_host(rows, perplexities, k=15, sample=None, seed=0, **embed_args):
    """``LatentIndex.choose_perplexity`` of host rows [N, dim] entirely on the host, no GPU: the same table and embedding, bit for bit"""
    perplexities = choose_perplexity_arg(perplexities)
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[1] < 2:
        raise ValueError("rows must have shape [N, dim] with dim >= 2, got %s" % (rows.shape,))
    map_quality_k_arg(k, len(rows))
    silhouette_sample_arg(sample, seed, len(rows))
    graph = neighbour_graph_host(rows)

    def linear():
        mo = _hip.moments_host(rows)
        _, v, _ = _hip.sym_eig(mo["cov"])
        return _hip.project_host(rows, mo["mean"], v[:2].astype(np.float32))["coords"]

    return choose_perplexity_run(lambda p: embed_rows_host(rows, perplexity=p, graph=graph, **embed_args),
                                 lambda c: map_quality_rows_host(rows, c, k=k, sample=sample, seed=seed, graph=graph), linear, perplexities)


def peaks_fit_args(k, bandwidth, neighbours, min_density, min_delta, route):
    """The arguments of ``LatentIndex.density_peaks`` checked: (k or None, neighbours, min_density, min_delta, route); ValueError
    otherwise, naming the argument"""
    if (k is None) == (min_density is None and min_delta is None):
        raise ValueError("exactly one of k and the thresholds (min_density, min_delta) must be given")
    if k is None and (min_density is None or min_delta is None):
        raise ValueError("min_density and min_delta must be given together")
    if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 1):
        raise ValueError("k must be an integer >= 1, got %r" % (k,))
    out = []
    for name, v in (("min_density", min_density), ("min_delta", min_delta)):
        if v is None:
            out.append(None)
            continue
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError("%s must be a number >= 0, got %r" % (name, v)) from None
        if isinstance(v, bool) or not f >= 0:
            raise ValueError("%s must be a number >= 0, got %r" % (name, v))
        out.append(f)
    if isinstance(bandwidth, str):
        if bandwidth != "auto":
            raise ValueError('bandwidth must be "auto" or a positive number, got %r' % (bandwidth,))
    else:
        _hip.rbf_gamma(bandwidth)
    if isinstance(neighbours, bool) or not isinstance(neighbours, (int, np.integer)) or not 1 <= int(neighbours) <= PEAKS_NEIGHBOURS:
        raise ValueError("neighbours must be an integer in 1 .. %d, got %r" % (PEAKS_NEIGHBOURS, neighbours))
    if route not in ("device", "host"):
        raise ValueError('route must be "device" or "host", got %r' % (route,))
    return None if k is None else int(k), int(neighbours), out[0], out[1], route


def peaks_auto_bandwidth(dist2, neighbours):
    """The automatic kernel width from a neighbour graph's squared distances [N, K], nearest first: h^2 is the median over the rows of
    the squared distance to the ``neighbours``-th nearest other row (capped at K), in fp64.  ValueError if that median is 0."""
    d2 = np.asarray(dist2, dtype=np.float64)
    h2 = float(np.median(d2[:, min(int(neighbours), d2.shape[1]) - 1]))
    if not (h2 > 0.0 and math.isfinite(h2)):
        raise ValueError("the automatic bandwidth is %r: more than half of the rows have %d coincident neighbours; give bandwidth a number" % (
            math.sqrt(h2) if h2 >= 0 else h2, min(int(neighbours), d2.shape[1])))
    return math.sqrt(h2)


def peaks_assemble(S, parent, delta2, k=None, min_density=None, min_delta=None):
    """The host half of the density-peak clustering, fp64, O(N log N): from the device's sums, parents and squared distances the
    densities, the decision values, the centres and the labels.  density_i = 2^-30 S_i / n_eligible; delta_i = sqrt(delta2_i); g_i =
    2^-30 S_i delta_i, +inf outright for the root (the eligible row without a parent) and 0 outright for any other row with S_i = 0 (its
    delta may be +inf: an overflowed distance).  Centres: the first ``k`` rows under (g
    descending, position ascending), or the rows with density >= min_density and delta >= min_delta plus the root; clusters numbered in
    density order (S descending, position ascending) of their centres; rows visited in density order, a non-centre takes its parent's
    label; ineligible rows (S < 0) get -1.  {"label", "density", "delta", "g", "centre_position", "size", "decision", "n_eligible"}."""
    S = np.asarray(S, dtype=np.int64)
    parent = np.asarray(parent, dtype=np.int32)
    N = S.shape[0]
    pos = np.arange(N)
    elig = S >= 0
    n_el = int(elig.sum())
    w = np.ldexp(S.astype(np.float64), -30)
    with np.errstate(invalid="ignore", divide="ignore"):
        density = np.where(elig, w / max(n_el, 1), np.nan)
        delta = np.where(elig, np.sqrt(np.asarray(delta2, dtype=np.float64)), np.inf)
        root = elig & (parent < 0)
        g = np.where(root, np.inf, np.where(elig, np.where(S == 0, 0.0, w * np.where(root, 0.0, delta)), -np.inf))  # (S = 0: 0, never 0 * inf)
    if n_el and int(root.sum()) != 1:
        raise ValueError("the parents do not form a tree: %d eligible rows have none" % int(root.sum()))
    order = np.lexsort((pos, -S))[:n_el]  # the density order: S descending, position ascending; the ineligible rows (S = -1) come last
    by_g = np.lexsort((pos, -g))[:n_el]
    if k is not None:
        if k > n_el:
            raise ValueError("k = %d clusters need %d rows without a non-finite component, there are %d" % (k, k, n_el))
        is_centre = np.zeros(N, bool)
        is_centre[by_g[:k]] = True
    else:
        is_centre = root | (elig & (density >= min_density) & (delta >= min_delta))
    centres = order[is_centre[order]]  # in density order: the root first
    number = np.full(N, -1, np.int32)
    number[centres] = np.arange(len(centres), dtype=np.int32)
    label = np.full(N, -1, np.int32)
    for i in order.tolist():
        label[i] = number[i] if is_centre[i] else label[parent[i]]
    return {"label": label, "density": density, "delta": delta, "g": g, "centre_position": centres.astype(np.int32),
            "size": np.bincount(label[label >= 0], minlength=len(centres)).astype(np.int64), "decision": g[by_g], "n_eligible": n_el}


def peaks_result(r, ids, atoms, k, min_density, min_delta, h, gamma, level, dim):
    """``LatentIndex.density_peaks``'s ``(result, peaks)`` from the passes' dict {"sum", "parent", "delta2"}"""
    a = peaks_assemble(r["sum"], r["parent"], r["delta2"], k, min_density, min_delta)
    c = a["centre_position"]
    result = {"label": a["label"], "density": a["density"], "delta": a["delta"], "parent": r["parent"], "sum": r["sum"], "centre_position": c,
              "centre_id": np.asarray(ids, dtype=np.int64)[c], "centre_atom": np.asarray(atoms, dtype=np.int32)[c], "size": a["size"],
              "decision": a["decision"], "bandwidth": float(h), "gamma": float(gamma), "n_eligible": a["n_eligible"]}
    return result, LatentPeaks(a["label"], ids, atoms, c, h, level, dim)


def density_peaks_rows_host(rows, k=None, bandwidth="auto", neighbours=31, min_density=None, min_delta=None, ids=None, atoms=None,
                            level="structure"):
    """``LatentIndex.density_peaks`` of host rows [N, dim] entirely on the host, no GPU: the twins of the search's distances and of the
    two passes -- bit for bit what an index holding these rows gives by either route."""
    k, neighbours, min_density, min_delta, _ = peaks_fit_args(k, bandwidth, neighbours, min_density, min_delta, "host")
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] < 1:
        raise ValueError("rows must have shape [N, dim] with N >= 1, got %s" % (rows.shape,))
    N, dim = rows.shape
    h = peaks_auto_bandwidth(neighbour_graph_host(rows)[1], neighbours) if isinstance(bandwidth, str) else float(bandwidth)
    gamma = _hip.rbf_gamma(h)
    ids = np.arange(N, dtype=np.int64) if ids is None else ids
    atoms = np.full(N, -1, np.int32) if atoms is None else atoms
    return peaks_result(_hip.peaks_host(rows, gamma), ids, atoms, k, min_density, min_delta, h, gamma, level, dim)


def density_of_sums(sums, n_rows):
    """The kernel density a density sum stands for, fp64: 2^-30 S / n_rows (the mean kernel weight to the index's rows); NaN for S < 0
    (a query with a non-finite component) and for an empty index."""
    S = np.asarray(sums, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(S >= 0, np.ldexp(S.astype(np.float64), -30) / (n_rows if n_rows > 0 else np.nan), np.nan)


class LatentPeaks(SavedResult):
    """A density-peak clustering of one level of one model, as ``LatentIndex.density_peaks`` fits it: the label of every row of the
    index in position order, the rows' ids and atoms, the centres' positions and the kernel width.  A new structure takes the label of
    its nearest index row: ``label_of(position)`` with the positions ``nearest(k=1)`` reports."""
    NOUN = "density-peak clustering"
    FIELDS = saved_fields("label", "ids", "atoms", "centre_position", ("bandwidth", AS_FLOAT))

    def __init__(self, label, ids, atoms, centre_position, bandwidth, level, dim):
        if level not in LEVELS:
            raise ValueError("level must be one of %s, got %r" % (", ".join(LEVELS), level))
        try:
            self.label = np.ascontiguousarray(label, dtype=np.int32).reshape(-1)
            self.ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
            self.atoms = np.ascontiguousarray(atoms, dtype=np.int32).reshape(-1)
            self.centre_position = np.ascontiguousarray(centre_position, dtype=np.int32).reshape(-1)
            self.bandwidth = float(bandwidth)
        except (TypeError, ValueError):
            raise ValueError("label, ids, atoms and centre_position must be arrays of integers and bandwidth a number") from None
        n, k = self.label.shape[0], self.centre_position.shape[0]
        if self.ids.shape != (n,) or self.atoms.shape != (n,):
            raise ValueError("ids %s and atoms %s must hold one entry per row (%d)" % (self.ids.shape, self.atoms.shape, n))
        if k and (self.centre_position.min() < 0 or self.centre_position.max() >= n):
            raise ValueError("centre_position must name rows in 0 .. %d" % (n - 1))
        if n and (self.label.min() < -1 or self.label.max() >= k):
            raise ValueError("label must lie in -1 .. %d (one less than the number of centres)" % (k - 1))
        if not (self.bandwidth > 0 and math.isfinite(self.bandwidth)):
            raise ValueError("bandwidth must be a positive number, got %r" % (bandwidth,))
        self.level, self.dim = level, int(dim)

    def __len__(self):
        return int(self.label.shape[0])

    @property
    def k(self):
        return int(self.centre_position.shape[0])

    def label_of(self, position):
        """The labels of index rows by position (any shape, int32): what ``nearest(k=1)``'s positions stand for; -1 for position -1."""
        p = np.asarray(position)
        if p.dtype.kind not in "iu" or (p.size and (p.min() < -1 or p.max() >= len(self))):
            raise ValueError("position must hold integers in -1 .. %d" % (len(self) - 1))
        return np.where(p >= 0, self.label[np.maximum(p, 0)], -1).astype(np.int32)


PROTO_ONE = 1 << 30  # the fixed-point weight term of two coincident rows


def prototypes_fit_args(m, criticisms, bandwidth, neighbours, witness, assign, route):
    """The arguments of ``LatentIndex.prototypes`` checked: (m, criticisms, neighbours, witness, assign, route); ValueError otherwise,
    naming the argument"""
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) < 1:
        raise ValueError("m must be an integer >= 1, got %r" % (m,))
    if isinstance(criticisms, bool) or not isinstance(criticisms, (int, np.integer)) or int(criticisms) < 0:
        raise ValueError("criticisms must be an integer >= 0, got %r" % (criticisms,))
    if isinstance(bandwidth, str):
        if bandwidth != "auto":
            raise ValueError('bandwidth must be "auto" or a positive number, got %r' % (bandwidth,))
    else:
        _hip.rbf_gamma(bandwidth)
    if isinstance(neighbours, bool) or not isinstance(neighbours, (int, np.integer)) or not 1 <= int(neighbours) <= PEAKS_NEIGHBOURS:
        raise ValueError("neighbours must be an integer in 1 .. %d, got %r" % (PEAKS_NEIGHBOURS, neighbours))
    if witness not in ("under", "both"):
        raise ValueError('witness must be "under" or "both", got %r' % (witness,))
    if not isinstance(assign, (bool, np.bool_)):
        raise ValueError("assign must be True or False, got %r" % (assign,))
    if route not in ("device", "host"):
        raise ValueError('route must be "device" or "host", got %r' % (route,))
    return int(m), int(criticisms), int(neighbours), witness, bool(assign), route


def prototypes_weights(A, B, n_picks, witness="under"):
    """The host half between the two selections, in exact integers: from the prototype call's A and B [N] and its number of picks m'
    the witness numerators W_i = m' A_i - n B_i (|W| < 2^63: the range cap), the witness function W_i / (n m' 2^30) in fp64 (NaN for
    an ineligible row) and the criticism weights: max(W, 0) ("under": the rows the prototypes under-represent) or |W| ("both", the
    paper's rule), shifted right until the largest has 31 bits; an ineligible row weighs 0.  -> (W int64, witness fp64, weight int64)"""
    A, B = np.asarray(A, dtype=np.int64), np.asarray(B, dtype=np.int64)
    elig = A >= 0
    n = int(elig.sum())
    W = np.where(elig, int(n_picks) * A - n * B, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        wit = np.where(elig, W.astype(np.float64) / float(max(n * int(n_picks), 1) * PROTO_ONE), np.nan)
    aw = np.maximum(W, 0) if witness == "under" else np.abs(W)
    top = int(aw.max()) if aw.size else 0
    return W, wit, aw >> max(0, top.bit_length() - 31)


def prototypes_mmd2(A, position, b_at_pick):
    """The squared MMD between the pool and the first s prototypes, s = 1 .. m', from the prototype call's integers: T = sum A_i over
    the eligible rows, SA_s = sum of A over the first s picks, K_s = K_{s-1} + 2 b_at_pick_s + 2^30;
    mmd2[s] = (s^2 T - 2 n s SA_s + n^2 K_s) / (n^2 s^2 2^30), numerator and denominator Python integers, one true division."""
    A = np.asarray(A, dtype=np.int64)
    elig = A >= 0
    n, T = int(elig.sum()), sum(int(x) for x in A[elig])
    out, SA, K = [], 0, 0
    for s, (p, b) in enumerate(zip(np.asarray(position).tolist(), np.asarray(b_at_pick).tolist()), 1):
        SA += int(A[p])
        K += 2 * int(b) + PROTO_ONE
        out.append((s * s * T - 2 * n * s * SA + n * n * K) / (n * n * s * s * PROTO_ONE))
    return np.array(out, dtype=np.float64)


def prototypes_run(proto, crit, assign_to, names, rows_at, m, criticisms, h, witness, level, dim):
    """``LatentIndex.prototypes``'s ``(result, prototypes)``: ``proto(m, gamma)`` and ``crit(weight, exclude, c, gamma)`` are the two
    selections (the device calls or their twins), ``assign_to(positions)`` the labelling pass or None, ``names()`` the rows' (ids, atoms),
    ``rows_at(positions)`` their rows"""
    gamma = _hip.rbf_gamma(h)
    r = proto(m, gamma)
    mp = int(r["count"])
    pos = r["position"][:mp]
    ids, atoms = names()
    ids, atoms = np.asarray(ids, dtype=np.int64), np.asarray(atoms, dtype=np.int32)
    W, wit, weight = prototypes_weights(r["A"], r["B"], max(mp, 1), witness)
    result = {"position": pos, "id": ids[pos], "atom": atoms[pos], "score": r["score"][:mp], "b_at_pick": r["b_at_pick"][:mp],
              "mmd2": prototypes_mmd2(r["A"], pos, r["b_at_pick"][:mp]), "witness": wit, "A": r["A"], "B": r["B"], "count": mp,
              "n_eligible": int((r["A"] >= 0).sum()), "bandwidth": float(h), "gamma": float(gamma)}
    cpos = np.zeros(0, np.int32)
    if criticisms and mp:
        c = crit(weight, pos, criticisms, gamma)
        cpos = c["position"][:int(c["count"])]
        result["criticism_score"] = c["score"][:len(cpos)]
    else:
        result["criticism_score"] = np.zeros(0, np.int64)
    result.update(criticism_position=cpos, criticism_id=ids[cpos], criticism_atom=atoms[cpos], criticism_witness=wit[cpos])
    if assign_to is not None and 1 <= mp <= _hip.KMEANS_MAX_K:
        a = assign_to(pos)
        result.update(nearest_prototype=a["label"], size=a["size"])
    protos = LatentPrototypes(rows_at(pos), ids[pos], atoms[pos], rows_at(cpos), ids[cpos], atoms[cpos], h, level, dim) if mp else None
    return result, protos


def prototypes_rows_host(rows, m, criticisms=0, bandwidth="auto", neighbours=31, witness="under", assign=True, ids=None, atoms=None,
                         level="structure"):
    """``LatentIndex.prototypes`` of host rows [N, dim] entirely on the host, no GPU: the twins of the search's distances, of the two
    selections and of the labelling pass -- bit for bit what an index holding these rows gives by either route."""
    m, criticisms, neighbours, witness, assign, _ = prototypes_fit_args(m, criticisms, bandwidth, neighbours, witness, assign, "host")
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] < 1:
        raise ValueError("rows must have shape [N, dim] with N >= 1, got %s" % (rows.shape,))
    N, dim = rows.shape
    _hip.check_prototypes_args(m, 1.0, N)
    h = peaks_auto_bandwidth(neighbour_graph_host(rows)[1], neighbours) if isinstance(bandwidth, str) else float(bandwidth)
    ids = np.arange(N, dtype=np.int64) if ids is None else ids
    atoms = np.full(N, -1, np.int32) if atoms is None else atoms
    return prototypes_run(functools.partial(_hip.prototypes_host, rows), functools.partial(_hip.criticisms_host, rows),
                          (lambda pos: _hip.kmeans_host(rows, rows[pos], 0, 0)) if assign else None, lambda: (ids, atoms),
                          lambda pos: rows[pos], m, criticisms, h, witness, level, dim)


def mmd_of_sums(Sa, Sb, cross):
    """The squared MMD between two samples a and b and b's witness from integer density sums: Sa [na] the sums of a's rows under a (the
    row itself included), Sb [nb] of b's under b, cross [nb] of b's under a; -1 marks a row with a non-finite component, left out.
    mmd2 = Ta / na^2 + Tb / nb^2 - 2 X / (na nb), all over 2^30: one true division of Python integers.  witness_j = mean k(b_j, a) -
    mean k(b_j, b) in fp64, NaN for a row left out.  -> (mmd2, witness [nb], numerator, denominator)"""
    Sa, Sb, X = (np.asarray(v, dtype=np.int64) for v in (Sa, Sb, cross))
    ea, eb = Sa >= 0, Sb >= 0
    na, nb = int(ea.sum()), int(eb.sum())
    if na < 1 or nb < 1:
        raise ValueError("the MMD needs a row without a non-finite component on either side, there are %d and %d" % (na, nb))
    Ta, Tb, Tx = (sum(int(x) for x in v) for v in (Sa[ea], Sb[eb], X[eb]))
    num, den = Ta * nb * nb + Tb * na * na - 2 * Tx * na * nb, na * na * nb * nb * PROTO_ONE
    with np.errstate(invalid="ignore"):
        wit = np.where(eb, X.astype(np.float64) / (na * float(PROTO_ONE)) - Sb.astype(np.float64) / (nb * float(PROTO_ONE)), np.nan)
    return num / den, wit, num, den


class LatentPrototypes(SavedResult):
    """The prototypes and criticisms of one level of one model, as ``LatentIndex.prototypes`` picks them: their rows, ids and atoms and
    the kernel width.  ``index_on(model)`` holds the prototype rows as an index, prototype p at position p: a prediction is explained
    by the nearest of them (``HipModel.nearest_prototype``)."""
    NOUN = "prototype set"
    KIND = "prototypes"
    FIELDS = saved_fields("rows", "ids", "atoms", "criticism_rows", "criticism_ids", "criticism_atoms", ("bandwidth", AS_FLOAT))

    def __init__(self, rows, ids, atoms, criticism_rows, criticism_ids, criticism_atoms, bandwidth, level, dim=None):
        if level not in LEVELS:
            raise ValueError("level must be one of %s, got %r" % (", ".join(LEVELS), level))
        try:
            self.rows = np.ascontiguousarray(rows, dtype=np.float32)
            self.ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
            self.atoms = np.ascontiguousarray(atoms, dtype=np.int32).reshape(-1)
            self.criticism_ids = np.ascontiguousarray(criticism_ids, dtype=np.int64).reshape(-1)
            self.criticism_atoms = np.ascontiguousarray(criticism_atoms, dtype=np.int32).reshape(-1)
            self.bandwidth = float(bandwidth)
            width = self.rows.shape[1] if self.rows.ndim == 2 else -1
            self.criticism_rows = np.ascontiguousarray(criticism_rows, dtype=np.float32).reshape(len(self.criticism_ids), max(width, 1))
        except (TypeError, ValueError, IndexError):
            raise ValueError("rows and criticism_rows must be arrays of numbers of one width with one id and one atom per row, and "
                             "bandwidth a number") from None
        m = self.rows.shape[0]
        if self.rows.ndim != 2 or m < 1 or width < 1 or (dim is not None and width != int(dim)):
            raise ValueError("rows must be an array of at least 1 row%s, got shape %s" % ("" if dim is None else " of %d columns" % int(dim), self.rows.shape))
        if self.ids.shape != (m,) or self.atoms.shape != (m,) or self.criticism_atoms.shape != self.criticism_ids.shape:
            raise ValueError("ids and atoms must hold one entry per row")
        if not np.isfinite(self.rows).all() or not np.isfinite(self.criticism_rows).all():
            raise ValueError("rows hold a non-finite value")
        if not (self.bandwidth > 0 and math.isfinite(self.bandwidth)):
            raise ValueError("bandwidth must be a positive number, got %r" % (bandwidth,))
        self.level, self.dim = level, int(width)
        self._index = None  # the prototype rows as an index on a model's GPU (index_on)

    @property
    def m(self):
        return int(self.rows.shape[0])

    @classmethod
    def saved_fits(cls, v, dim):
        return v["rows"].ndim == 2 and v["rows"].shape[1] == dim

    def index_on(self, model):
        """The prototype rows as a ``LatentIndex`` on ``model``'s GPU, prototype p at position p under its id and atom (built once per
        model and kept)."""
        self.check_model(model)
        if self._index is None or self._index.model is not model:
            self.free()
            self._index = LatentIndex(model, self.level).add_rows(self.rows, self.ids, self.atoms if self.level == "atom" else None)
        return self._index

    def free(self):
        if self._index is not None:
            self._index.free()
        self._index = None


HIER_MAX_SAMPLES = EMBED_NEIGHBOURS  # the farthest neighbour a core distance can look at: what ``neighbour_graph`` returns


def hierarchy_fit_args(min_samples, route):
    """The arguments of ``LatentIndex.hierarchy`` checked: (min_samples, route); ValueError otherwise, naming the argument"""
    if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) or not 0 <= int(min_samples) <= HIER_MAX_SAMPLES:
        raise ValueError("min_samples must be an integer in 0 .. %d, got %r" % (HIER_MAX_SAMPLES, min_samples))
    if route not in ("device", "host"):
        raise ValueError('route must be "device" or "host", got %r' % (route,))
    return int(min_samples), route


def check_min_cluster_size(min_cluster_size):
    if isinstance(min_cluster_size, bool) or not isinstance(min_cluster_size, (int, np.integer)) or int(min_cluster_size) < 2:
        raise ValueError("min_cluster_size must be an integer >= 2, got %r" % (min_cluster_size,))
    return int(min_cluster_size)


def hierarchy_core2(rows, min_samples, graph, elig=None):
    """The squared core distances, fp32 [N]: for a row without a non-finite component the search's dist2 to its ``min_samples``-th
    nearest OTHER such row -- its farthest one where there are fewer, 0 where it is alone --, and 0 for the other rows (they are in no
    edge).  ``graph(rows of the eligible) -> (position, dist2 [n, K])`` is ``neighbour_graph`` / ``neighbour_graph_host`` without the
    finiteness check."""
    rows = np.asarray(rows, dtype=np.float32)
    elig = np.isfinite(rows).all(axis=1) if elig is None else elig
    core2 = np.zeros(rows.shape[0], np.float32)
    if int(elig.sum()) >= 2:
        _, d2 = graph(rows if elig.all() else np.ascontiguousarray(rows[elig]))
        core2[elig] = d2[:, min(int(min_samples), d2.shape[1]) - 1]
    return core2


def hierarchy_lone_row(rows):
    """the position of the one row without a non-finite component, -1 if there is none or more than one"""
    elig = np.flatnonzero(np.isfinite(np.asarray(rows, dtype=np.float32)).all(axis=1)) if len(rows) else np.zeros(0, np.int64)
    return int(elig[0]) if len(elig) == 1 else -1


def hierarchy_result(r, core2, n_rows, ids, atoms, min_samples, level, dim, lone_position=-1):
    """``LatentIndex.hierarchy``'s ``(result, hierarchy)`` from the tree's dict {"a", "b", "w"}; ``lone_position``: the one eligible row
    of a tree without edges, -1 if there is none"""
    h = LatentHierarchy(r["a"], r["b"], r["w"], core2, n_rows, ids, atoms, min_samples, level, dim, lone_position)
    result = {"a": h.a, "b": h.b, "w": h.w, "core2": h.core2 if min_samples else None, "n_eligible": h.n_eligible}
    if "rounds" in r:
        result["rounds"] = r["rounds"]
    return result, h


def hierarchy_rows_host(rows, min_samples=5, ids=None, atoms=None, level="structure"):
    """``LatentIndex.hierarchy`` of host rows [N, dim] entirely on the host, no GPU: the twins of the search's distances and of the
    tree -- bit for bit what an index holding these rows gives by either route."""
    min_samples, _ = hierarchy_fit_args(min_samples, "host")
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[1] < 1:
        raise ValueError("rows must have shape [N, dim], got %s" % (rows.shape,))
    N, dim = rows.shape
    if N > _hip.MST_MAX_ROWS:
        raise ValueError("%d rows, a hierarchy takes at most %d" % (N, _hip.MST_MAX_ROWS))
    core2 = hierarchy_core2(rows, min_samples, lambda x: neighbour_graph_host(x, strict=False)) if min_samples else None
    ids = np.arange(N, dtype=np.int64) if ids is None else ids
    atoms = np.full(N, -1, np.int32) if atoms is None else atoms
    r = _hip.mst_host(rows, core2)
    return hierarchy_result(r, core2, N, ids, atoms, min_samples, level, dim, -1 if len(r["a"]) else hierarchy_lone_row(rows))


def _number_by_least_member(raw, n_rows):
    """raw labels (any integers >= 0, -1: none) renumbered 0, 1, .. in the order of each label's least member position: (label int32
    [n_rows], the raw label of every new number)"""
    raw = np.asarray(raw, dtype=np.int64)
    pos = np.flatnonzero(raw >= 0)
    label = np.full(n_rows, -1, np.int32)
    if not len(pos):
        return label, np.zeros(0, np.int64)
    uniq, first = np.unique(raw[pos], return_index=True)  # first: the least position among each label's members (pos ascends)
    order = np.argsort(first, kind="stable")
    number = np.empty(len(uniq), np.int64)
    number[order] = np.arange(len(uniq))
    label[pos] = number[np.searchsorted(uniq, raw[pos])]
    return label, uniq[order]


class LatentHierarchy(SavedResult):
    """The hierarchical clustering of one level of one model, as ``LatentIndex.hierarchy`` builds it: the N - 1 edges of the minimum
    spanning tree in the edge order (w ascending, then the positions), the squared core distances, the rows' ids and atoms.  Everything
    derived from it -- ``linkage``, ``cut``, ``clusters`` -- is deterministic fp64 NumPy on the sorted edges.  The rows that count
    (the eligible ones: no non-finite component) are the rows the edges name; a tree without edges has none, or the one at
    ``lone_position``.  The other rows get label -1 everywhere."""
    NOUN = "hierarchy"
    FIELDS = saved_fields("a", "b", "w", "core2", "ids", "atoms", ("min_samples", AS_INT), ("lone_position", AS_INT))

    def __init__(self, a, b, w, core2, n_rows, ids, atoms, min_samples, level, dim, lone_position=-1):
        if level not in LEVELS:
            raise ValueError("level must be one of %s, got %r" % (", ".join(LEVELS), level))
        try:
            self.a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
            self.b = np.ascontiguousarray(b, dtype=np.int32).reshape(-1)
            self.w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
            self.ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
            self.atoms = np.ascontiguousarray(atoms, dtype=np.int32).reshape(-1)
            n = int(n_rows)
            self.core2 = np.zeros(n, np.float32) if core2 is None else np.ascontiguousarray(core2, dtype=np.float32).reshape(-1)
            self.min_samples = int(min_samples)
        except (TypeError, ValueError):
            raise ValueError("a, b, ids and atoms must be arrays of integers, w and core2 arrays of numbers") from None
        m = self.a.shape[0]
        if self.b.shape != (m,) or self.w.shape != (m,):
            raise ValueError("a %s, b %s and w %s must hold one entry per edge" % (self.a.shape, self.b.shape, self.w.shape))
        if self.ids.shape != (n,) or self.atoms.shape != (n,) or self.core2.shape != (n,):
            raise ValueError("ids %s, atoms %s and core2 %s must hold one entry per row (%d)" % (self.ids.shape, self.atoms.shape, self.core2.shape, n))
        if m and (self.a.min() < 0 or self.b.max() >= n or not (self.a < self.b).all()):
            raise ValueError("every edge must name rows a < b in 0 .. %d" % (n - 1))
        if m and (not (self.w >= 0).all() or not (np.diff(self.w) >= 0).all()):
            raise ValueError("w must be non-negative and ascending")
        self.level, self.dim, self.n_rows = level, int(dim), n
        # the rows that count, and the merges: cluster n_eligible + e joins the clusters of a[e] and b[e] (union-find over the edges)
        in_tree = np.zeros(n, bool)
        in_tree[self.a], in_tree[self.b] = True, True
        self.lone_position = int(lone_position)
        if self.lone_position != -1:
            if m or not 0 <= self.lone_position < n:
                raise ValueError("lone_position names the one eligible row of a tree without edges, in 0 .. %d; got %d with %d edges" % (
                    n - 1, self.lone_position, m))
            in_tree[self.lone_position] = True
        self.leaf_position = np.flatnonzero(in_tree).astype(np.int32)
        ne = self.n_eligible = len(self.leaf_position)
        if m != max(ne - 1, 0):
            raise ValueError("%d edges over %d rows are no spanning tree" % (m, ne))
        leaf = np.full(n, -1, np.int64)
        leaf[self.leaf_position] = np.arange(ne)
        top = list(range(ne))  # union-find over leaves; top[root] = the cluster id the set carries
        up = list(range(ne))
        size = [1] * ne
        left, right, count = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64)

        def find(x):
            r = x
            while up[r] != r:
                r = up[r]
            while up[x] != r:
                up[x], x = r, up[x]
            return r

        for e, (x, y) in enumerate(zip(leaf[self.a].tolist(), leaf[self.b].tolist())):
            rx, ry = find(x), find(y)
            if rx == ry:
                raise ValueError("the edges close a cycle at edge %d" % e)
            cx, cy = top[rx], top[ry]
            left[e], right[e] = min(cx, cy), max(cx, cy)
            if size[rx] < size[ry]:
                rx, ry = ry, rx
            up[ry] = rx
            size[rx] += size[ry]
            top[rx] = ne + e
            count[e] = size[rx]
        self._left, self._right, self._count = left, right, count

    def __len__(self):
        return self.n_rows

    @classmethod
    def from_saved(cls, v, level, dim):
        return cls(v["a"], v["b"], v["w"], v["core2"], len(v["ids"]), v["ids"], v["atoms"], v["min_samples"], level, dim, v["lone_position"])

    def linkage(self):
        """The dendrogram in SciPy's layout, fp64 [n - 1, 4], n the rows that count: merge e joins the clusters of a[e] and b[e] in edge
        order at height sqrt(w[e]); columns: the two cluster ids (the smaller first), the height, the rows of the new cluster n + e.
        Leaf i is the i-th row that count in position order (``leaf_position``; the position itself when all rows count).  Usable with
        ``scipy.cluster.hierarchy.dendrogram`` as it is."""
        return np.stack([self._left.astype(np.float64), self._right.astype(np.float64), np.sqrt(self.w.astype(np.float64)),
                         self._count.astype(np.float64)], axis=1) if len(self.w) else np.zeros((0, 4))

    def cut(self, height=None, k=None):
        """The flat clustering of a cut through the dendrogram, int32 [N]: with ``height`` the merges at sqrt(w) <= height are made, with
        ``k`` the first n - k merges (k clusters; 1 <= k <= n).  Clusters are numbered by their least member position; rows that do not
        count get -1."""
        if (height is None) == (k is None):
            raise ValueError("exactly one of height and k must be given")
        ne, m = self.n_eligible, len(self.w)
        if k is not None:
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= max(ne, 1):
                raise ValueError("k must be an integer in 1 .. %d, got %r" % (max(ne, 1), k))
            n_merge = max(ne - int(k), 0)
        else:
            try:
                hgt = float(height)
            except (TypeError, ValueError):
                raise ValueError("height must be a number >= 0, got %r" % (height,)) from None
            if isinstance(height, bool) or not hgt >= 0:
                raise ValueError("height must be a number >= 0, got %r" % (height,))
            n_merge = int(np.searchsorted(np.sqrt(self.w.astype(np.float64)), hgt, side="right"))
        # the cluster of every leaf after n_merge merges: the nodes ne + e, e < n_merge, top-down
        owner = np.arange(ne + m, dtype=np.int64)
        for e in range(n_merge - 1, -1, -1):
            owner[self._left[e]] = owner[self._right[e]] = owner[ne + e]
        raw = np.full(self.n_rows, -1, np.int64)
        raw[self.leaf_position] = owner[:ne]
        return _number_by_least_member(raw, self.n_rows)[0]

    def clusters(self, min_cluster_size):
        """HDBSCAN's condensed tree and excess-of-mass selection on the dendrogram.  lambda = 1 / sqrt(w); a zero-weight merge takes the
        largest lambda of the merges with w > 0, or 1 if there is none, which keeps every stability finite.  Walking down from the root,
        a split whose two sides both hold >= ``min_cluster_size`` rows makes two new clusters born at the split's lambda; otherwise the
        rows of a side below ``min_cluster_size`` fall out of the cluster at that lambda and the other side carries it on.
        stability(c) = the sum over the rows of c of (lambda_leave - lambda_birth), a row that passes into a child cluster leaving at the
        child's birth.  Bottom-up, a cluster is selected iff its stability >= the sum of its children's selected totals; the root is
        never selected.  {"label" int32 [N] (-1: noise; clusters numbered by least member position), "probability" fp64 [N]
        (lambda_leave over the largest lambda_leave of the row's cluster, capped at 1; 0 for noise), "persistence" fp64 per cluster (its
        stability), "birth2" fp32 per cluster (the squared level w at which it joins its parent), "exemplar" int32 per cluster (the
        member of largest lambda_leave, least position on ties), "size" int64 per cluster, "lambda" fp64 [N] (lambda_leave; NaN for rows
        that do not count)}."""
        mcs = check_min_cluster_size(min_cluster_size)
        N, ne, m = self.n_rows, self.n_eligible, len(self.w)
        out = {"label": np.full(N, -1, np.int32), "probability": np.zeros(N), "persistence": np.zeros(0), "birth2": np.zeros(0, np.float32),
               "exemplar": np.zeros(0, np.int32), "size": np.zeros(0, np.int64), "lambda": np.full(N, np.nan)}
        if m == 0:
            return out
        w64 = self.w.astype(np.float64)
        with np.errstate(divide="ignore"):
            lam = 1.0 / np.sqrt(w64)
        lam[w64 == 0] = lam[w64 > 0].max() if (w64 > 0).any() else 1.0
        left, right = self._left.tolist(), self._right.tolist()
        size = [1] * ne + self._count.tolist()
        lam_l, w_l = lam.tolist(), self.w.tolist()
        c_parent, c_birth, c_birth2 = [-1], [0.0], [float("inf")]  # cluster 0 is the root
        c_stab, c_children = [0.0], [[]]
        p_cluster, p_lambda = [0] * ne, [0.0] * ne
        stack = [(ne + m - 1, 0)]
        while stack:
            node, c = stack.pop()
            e = node - ne
            l, r, la = left[e], right[e], lam_l[e]
            if size[l] >= mcs and size[r] >= mcs:
                for side in (l, r):
                    k = len(c_parent)
                    c_parent.append(c), c_birth.append(la), c_birth2.append(w_l[e]), c_stab.append(0.0), c_children.append([])
                    c_children[c].append(k)
                    c_stab[c] += size[side] * (la - c_birth[c])
                    stack.append((side, k))
                continue
            for side in (l, r):
                if size[side] >= mcs:
                    stack.append((side, c))
                    continue
                c_stab[c] += size[side] * (la - c_birth[c])
                todo = [side]  # the side's rows fall out of c here
                while todo:
                    x = todo.pop()
                    if x < ne:
                        p_cluster[x], p_lambda[x] = c, la
                    else:
                        todo.append(left[x - ne]), todo.append(right[x - ne])
        # excess of mass, bottom-up: children carry larger numbers than their parents
        n_c = len(c_parent)
        chosen, total = [False] * n_c, [0.0] * n_c
        for c in range(n_c - 1, 0, -1):
            below = sum(total[k] for k in c_children[c])
            if c_stab[c] >= below:
                chosen[c], total[c] = True, c_stab[c]
            else:
                total[c] = below
        owner = [-1] * n_c  # the selected cluster at or above c that no selected cluster lies above
        for c in range(1, n_c):
            owner[c] = owner[c_parent[c]] if owner[c_parent[c]] >= 0 else (c if chosen[c] else -1)
        raw = np.full(N, -1, np.int64)
        raw[self.leaf_position] = np.asarray(owner, dtype=np.int64)[np.asarray(p_cluster, dtype=np.int64)]
        label, which = _number_by_least_member(raw, N)
        lam_row = np.full(N, np.nan)
        lam_row[self.leaf_position] = p_lambda
        k = len(which)
        top = np.zeros(k)
        member = label >= 0
        np.maximum.at(top, label[member], lam_row[member])
        prob = np.zeros(N)
        with np.errstate(invalid="ignore", divide="ignore"):
            prob[member] = np.where(top[label[member]] > 0, np.minimum(lam_row[member] / top[label[member]], 1.0), 1.0)
        exemplar = np.full(k, -1, np.int32)
        for i in np.flatnonzero(member)[::-1].tolist():  # descending positions: the least position among the largest stays
            if lam_row[i] == top[label[i]]:
                exemplar[label[i]] = i
        out.update(label=label, probability=prob, persistence=np.asarray(c_stab)[which], birth2=np.asarray(c_birth2, dtype=np.float32)[which],
                   exemplar=exemplar, size=np.bincount(label[member], minlength=k).astype(np.int64))
        out["lambda"] = lam_row
        return out

    def attach_labels(self, position, dist2, clusters):
        """The labels of new rows from their nearest index row (``position``, ``dist2`` as ``nearest(k=1)`` / scann_index_query_batch
        report them) under ``clusters`` (what ``clusters(min_cluster_size)`` returned): the label of the nearest row r, or -1 if r is
        noise, if there is no r, or if max(dist2, core2[r]) >= birth2[label] -- the new row would lie outside the cluster at the level
        where the cluster is born."""
        p = np.asarray(position)
        d = np.asarray(dist2, dtype=np.float32)
        if p.dtype.kind not in "iu" or p.shape != d.shape or (p.size and (p.min() < -1 or p.max() >= len(self))):
            raise ValueError("position must hold integers in -1 .. %d and dist2 one distance each" % (len(self) - 1))
        q = np.maximum(p, 0)
        lab = np.where(p >= 0, clusters["label"][q], -1).astype(np.int32) if len(self) else np.full(p.shape, -1, np.int32)
        if len(self) and len(clusters["birth2"]):
            reach = np.maximum(d, self.core2[q])
            lab = np.where((lab >= 0) & ~(reach < clusters["birth2"][np.maximum(lab, 0)]), -1, lab).astype(np.int32)
        return lab
