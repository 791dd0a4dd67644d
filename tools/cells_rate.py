#!/usr/bin/env python3
"""Cost of the nearest-row search over an index partitioned into cells (scann_index_partition) beside the full search of the same rows
in the same run, on one box:
    python tools/cells_rate.py [--small] [out.txt]
Two row sets of 128 columns: rows around 40 centres in shuffled order (tools/mst_rate.py's set) and unstructured Gaussian rows, the
worst case; N = 16,384, 131,072 and 2,400,000 (--small: the first only).  The full search is the route of an index without a partition,
reached through an unpartitioned twin index of the same rows.  One process, host clock around synchronous calls, warm, min / median of
three, the two routes alternating.  Prints (and appends to out.txt):
  (a) LatentIndex.partition(cells): build time, cells, tiles, pad share;
  (b) Engine.index_query of 2,304 host queries -- 128 QM9-shaped molecules of 18 atoms: rows of the set, perturbed -- at k = 1, 5 and 32:
      full, partitioned, the visited share of (128-query group, 64-row tile) pairs, and whether both answers agree in every byte;
  (c) the neighbour graph (neighbour_graph, k = 32 self-queries, 4,096 at a time) at 16,384 and 131,072 rows, both routes;
  (d) the cells sweep at 131,072 rows that settles cells="auto": (b) at k = 5 and (c) for several cell counts;
  (e) LatentIndex.density_peaks and LatentIndex.hierarchy end to end at 131,072 rows, with and without a partition;
  (f) Engine.index_select against a partitioned reference at 131,072 rows.
In (b) and (d) the partitioned index is timed twice: with the fall-back rule off (SCANN_CELLS_FALLBACK=off: the list route whatever the
plan keeps, which is what settles the rule) and as shipped; (g) sweeps k on the Gaussian rows with the rule off."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
argv = sys.argv[1:]
args = [a for a in argv if not a.startswith("--")]
out_path = args[0] if args else None
D = 128


def say(line):
    print(line, flush=True)
    if out_path:
        open(out_path, "a").write(line + "\n")


def timed_pair(f, g, runs=3):
    """f and g alternating: (min, median) of each"""
    tf, tg = [], []
    for r in range(runs):
        for fn, t in ((f, tf), (g, tg)):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
    return (min(tf), float(np.median(tf))), (min(tg), float(np.median(tg)))


import scann_oracle as so
from scann.models import LatentIndex
from scann.models import latent_index as li
from scann.models.scann_model import HipModel

cfg = so.default_config("qm9")
model = HipModel(cfg, so.init_weights(cfg, 3, perturb=True), device=0, infer=True)
eng = model.engine


def make_rows(kind, N, seed=7):
    rng = np.random.default_rng(seed)
    if kind == "40 centres":
        centres = 4.0 * rng.standard_normal((40, D), dtype=np.float32)
        return centres[rng.integers(0, 40, N)] + rng.standard_normal((N, D), dtype=np.float32)
    return rng.standard_normal((N, D), dtype=np.float32)


def index_of(rows):
    lat = LatentIndex(model, "atom")
    for i in range(0, len(rows), 1 << 18):
        lat.add_rows(rows[i:i + (1 << 18)])
    return lat


def same(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def route(rule_on):
    """the fall-back rule of the pruned route (csrc/scann_cells.h) as shipped, or off: the list route whatever the plan keeps"""
    if rule_on:
        os.environ.pop("SCANN_CELLS_FALLBACK", None)
    else:
        os.environ["SCANN_CELLS_FALLBACK"] = "off"


def query_line(tag, plain, cut, q, k):
    route(False)
    a, b = eng.index_query(plain._ix, q, k), eng.index_query(cut._ix, q, k)  # warm, and the answers
    st = cut.search_stats()
    tp, tc = timed_pair(lambda: eng.index_query(plain._ix, q, k), lambda: eng.index_query(cut._ix, q, k))
    route(True)
    c = eng.index_query(cut._ix, q, k)
    fell = cut.search_stats()["visited"] == cut.search_stats()["total"] + cut.search_stats()["seeds"]
    _, tr = timed_pair(lambda: eng.index_query(plain._ix, q, k), lambda: eng.index_query(cut._ix, q, k))
    say("    %s k = %2d: full %8.2f / %8.2f ms, list route %8.2f / %8.2f ms (%.2f x), kept %5.1f %% of %d pairs (%d seeds); as shipped "
        "%8.2f / %8.2f ms (%.2f x, %s), answers %s" % (
            tag, k, tp[0] * 1e3, tp[1] * 1e3, tc[0] * 1e3, tc[1] * 1e3, tp[0] / tc[0], 100.0 * st["visited_share"], st["total"], st["seeds"],
            tr[0] * 1e3, tr[1] * 1e3, tp[0] / tr[0], "fell back" if fell else "list route",
            "equal in every byte" if same(a, b) and same(a, c) else "DIFFER"))


def graph_line(tag, plain, cut):
    ga, gb = li.neighbour_graph(plain, strict=False), li.neighbour_graph(cut, strict=False)
    st = cut.search_stats()
    tp, tc = timed_pair(lambda: li.neighbour_graph(plain, strict=False), lambda: li.neighbour_graph(cut, strict=False), runs=2)
    say("    %s neighbour graph: full %9.1f / %9.1f ms, partitioned %9.1f / %9.1f ms (%.2f x), last chunk visited %5.1f %%, graphs %s" % (
        tag, tp[0] * 1e3, tp[1] * 1e3, tc[0] * 1e3, tc[1] * 1e3, tp[0] / tc[0], 100.0 * st["visited_share"],
        "equal in every byte" if all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(ga, gb)) else "DIFFER"))


sizes = (16384,) if "--small" in argv else (16384, 131072, 2400000)
for kind in ("40 centres", "gaussian"):
    for N in sizes:
        rows = make_rows(kind, N)
        rng = np.random.default_rng(1)
        q = rows[rng.integers(0, N, 2304)] + np.float32(0.3) * rng.standard_normal((2304, D), dtype=np.float32)
        plain, cut = index_of(rows), index_of(rows)
        cells = li.auto_cells(N)
        cut.partition(cells)  # warm
        t0 = time.perf_counter()
        info = cut.partition(cells)
        t_build = time.perf_counter() - t0
        say("%s, N = %d rows x %d columns" % (kind, N, D))
        say("(a) partition(cells=%d): %9.1f ms; %d cells, %d tiles, pad share %.3f, largest cell %d rows" % (
            cells, t_build * 1e3, info["cells"], info["tiles"], info["pad_share"], info["largest"]))
        say("(b) Engine.index_query, 2,304 host queries:")
        for k in (1, 5, 32):
            query_line("", plain, cut, q, k)
        if N <= 131072:
            say("(c)")
            graph_line("", plain, cut)
        if N == 131072:
            say("(d) the cells sweep:")
            for c in (8, 64, 256, 1024):
                t0 = time.perf_counter()
                info = cut.partition(c)
                t_build = time.perf_counter() - t0
                say("  cells = %d (build %.0f ms, pad share %.3f):" % (c, t_build * 1e3, info["pad_share"]))
                query_line("  ", plain, cut, q, 5)
                graph_line("  ", plain, cut)
            cut.partition(cells)
            say("(f) Engine.index_select of 8 rows from the same rows as a pool against this index as the reference (128 passes of 1,024 "
                "queries, k = 1, the distances left on the device; the pruned route waits for the host in every pass):")
            pool = index_of(rows)
            eng.index_select(pool._ix, plain._ix, 8), eng.index_select(pool._ix, cut._ix, 8)
            tp, tc = timed_pair(lambda: eng.index_select(pool._ix, plain._ix, 8), lambda: eng.index_select(pool._ix, cut._ix, 8), runs=2)
            say("    full reference %9.1f / %9.1f ms, partitioned reference %9.1f / %9.1f ms (%.2f x)" % (
                tp[0] * 1e3, tp[1] * 1e3, tc[0] * 1e3, tc[1] * 1e3, tp[0] / tc[0]))
            pool.free()
            say("(e) end to end, without / with a partition:")
            for name, call in (("density_peaks(k=40)", lambda ix: ix.density_peaks(k=40)), ("hierarchy(min_samples=5)", lambda ix: ix.hierarchy(min_samples=5))):
                call(plain), call(cut)
                tp, tc = timed_pair(lambda: call(plain), lambda: call(cut), runs=2)
                say("    %s: %9.1f / %9.1f ms without, %9.1f / %9.1f ms with (%.2f x)" % (name, tp[0] * 1e3, tp[1] * 1e3, tc[0] * 1e3, tc[1] * 1e3,
                                                                                         tp[0] / tc[0]))
        if kind == "gaussian" and N == 131072:
            say("(g) the list route where it visits every tile, by k (rule off), against the full search:")
            route(False)
            for k in (1, 2, 3, 5, 7, 8, 12, 16, 24, 32):
                eng.index_query(plain._ix, q, k), eng.index_query(cut._ix, q, k)
                tp, tc = timed_pair(lambda: eng.index_query(plain._ix, q, k), lambda: eng.index_query(cut._ix, q, k))
                say("    k = %2d: full %8.2f ms, list route %8.2f ms (%.2f x)" % (k, tp[0] * 1e3, tc[0] * 1e3, tp[0] / tc[0]))
            route(True)
        plain.free()
        cut.free()
