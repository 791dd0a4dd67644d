#!/usr/bin/env python3
"""CLI with the reference's interface (predict_model.py:95-100): load ``<trained_model>/config.yaml`` and
``<trained_model>/models/model_<target>.h5`` in infer mode, predict the whole dataset, pickle GA scores and
predictions next to the model.  ``--outputs after_Lc,local_attention_2,bf_property`` also pickles each named output as
``<name>_<target>.pickle``: one array per structure, laid out as the padded predict of its batch returns it.
``--mc-samples T [--mc-seed S]`` also pickles Monte Carlo dropout estimates as ``mc_<target>.pickle``: a dict with the de-normalised
mean and standard deviation of the prediction per structure and the mean and standard deviation of its GA scores (one [M, 1] array
per structure, as ga_scores), each structure keyed by its index in the dataset.
``--rollout [--rollout-residual R] [--rollout-head K]`` also pickles the attention rollout as ``rollout_<target>.pickle``: one unpadded dict
per structure with ``attribution`` [n] (the GA scores traced back to the atoms through the local-attention layers) and ``rollout`` [n, n].
``--nearest K [--nearest-level atom] [--nearest-index FILE]`` also pickles ``nearest_<target>.pickle``: one unpadded dict per structure
with the K nearest structures of the dataset in the model's latent space (``neighbor_id``: dataset indices, the structure itself left
out; ``distance``; ``latent_distance``: their mean, an uncertainty measure), or per atom at ``--nearest-level atom`` (``neighbor_atom``
as well).  With ``--nearest-index FILE`` a saved ``LatentIndex``, for example of the training set, is searched and nothing is left out.
``--match K [--match-measure chamfer|hausdorff|cover] [--match-index FILE]`` pickles ``match_<target>.pickle``: per structure the K
structures of the dataset (or of a saved atom-level index) made of the most similar local structures, and which atom matches which.
``--pair K [--pair-shortlist S] [--pair-measure chamfer|hausdorff|cover] [--pair-index FILE]`` pickles ``pair_<target>.pickle``: the same
question answered one to one -- the S candidates of ``--match`` reranked by the exact pairing of their atoms with the structure's, and
per neighbour a true atom map.
``--select M [--select-level atom] [--select-reference FILE]`` also pickles ``selected_<target>.pickle``: one dict with the M most
diverse structures of the dataset (or atoms, at ``--select-level atom``) by greedy k-center selection in the model's latent space, in
pick order (``neighbor_id``: dataset indices; ``atom``; ``radius``: the covering radius at each pick; ``position``; ``count``).  With
``--select-reference FILE``, a saved ``LatentIndex`` of what is labelled already, they are the dataset's structures farthest from it.
``--cluster K [--cluster-level atom|structure] [--cluster-iter N] [--cluster-out FILE]`` clusters the dataset's atoms (or structures)
in the model's latent space by k-means on the GPU, prints the sizes, ``n_iter`` / ``converged`` / inertia and each cluster's medoid
(dataset index and atom), pickles the result as ``clusters_<target>.pickle`` and, with ``--cluster-out``, saves the centres as a
``LatentClustering`` (.npz) that ``SCANN.assign`` takes.
``--cluster-sweep 2,4,8,16,32,64 [--cluster-level atom|structure] [--cluster-sample M] [--cluster-iter N] [--cluster-out FILE]`` chooses
the number of clusters: k-means for every k of the list, each scored by the silhouette of its labels (every mean distance over all rows,
exact on the GPU and bit-reproducible; ``--cluster-sample M``: the score is the mean over M sampled rows).  It prints the table -- score,
inertia, Calinski-Harabasz, Davies-Bouldin, converged per k -- and the best k, pickles the table with the best k's clustering as
``cluster_sweep_<target>.pickle`` and, with ``--cluster-out``, saves the best k's centres as a ``LatentClustering`` (.npz).
``--project M [--project-level atom|structure] [--project-out FILE]`` maps the dataset's structures (or atoms) onto the M leading
principal components of the model's latent space (mean and covariance on the GPU, bit-reproducible), prints the rank and the explained
variance, pickles the result -- coordinates, Mahalanobis distance and distance to the mean per row, with the rows' dataset indices and
atoms -- as ``projection_<target>.pickle`` and, with ``--project-out``, saves the map as a ``LatentProjection`` (.npz) that
``SCANN.project`` takes.
``--fit-head TARGETS.npy [--head-level atom|structure] [--head-out FILE]`` fits a linear readout head for another property on the frozen
latent space: ``TARGETS.npy`` holds [N] or [N, K] values (K <= 16, NaN: unlabelled), one row per structure of the dataset in dataset
order, or per atom in packed order.  Ridge regression with the strength chosen by exact leave-one-out on the GPU; prints the
leave-one-out table, pickles the result with the rows' dataset indices and atoms as ``head_<target>.pickle`` and, with ``--head-out``,
saves the head as a ``LatentHead`` (.npz).  ``--head FILE`` evaluates a saved head over the dataset instead and pickles one unpadded dict
per structure (prediction, std, leverage) as ``head_<target>.pickle``.
``--fit-kernel-head TARGETS.npy [--landmarks M] [--kernel-head-level atom|structure] [--kernel-head-out FILE]`` fits a nonlinear readout
head instead: ridge regression on Gaussian features to M landmarks of the latent space (default 256; the most diverse rows), features,
moments and leave-one-out on the GPU, the bandwidth chosen by leave-one-out.  It prints the bandwidth path and the leave-one-out table,
pickles the result as ``kernel_head_<target>.pickle`` and, with ``--kernel-head-out``, saves the head as a ``LatentKernelHead`` (.npz).
``--kernel-head FILE`` evaluates a saved one over the dataset and pickles one unpadded dict per structure (prediction, std, leverage,
support) as ``kernel_head_<target>.pickle``.
``--fit-class-head LABELS.npy [--class-head-level atom|structure] [--class-head-out FILE]`` fits a classification head instead:
multinomial logistic regression of integer labels (one per structure, or per atom in dataset order; -1: unlabelled) on the frozen latent
space, the ridge strength chosen by 4-fold cross-validation, every pass over the rows on the GPU.  It prints the cross-validation table,
pickles the result as ``class_head_<target>.pickle`` and, with ``--class-head-out``, saves the head as a ``LatentClassHead`` (.npz).
``--class-head FILE`` evaluates a saved one over the dataset and pickles one unpadded dict per structure (probability, label, confidence,
entropy) as ``class_head_<target>.pickle``.
``--embed [--embed-level atom|structure] [--embed-perplexity P] [--embed-out FILE]`` draws the neighbour embedding (t-SNE) of the
dataset's rows in two dimensions, the pair repulsion computed exactly on the GPU and the map bit-reproducible.  It prints the divergence
before and after, pickles the result (coordinates, ids, atoms, neighbour lists) as ``embedding_<target>.pickle`` and, with ``--embed-out``,
saves the map as a ``LatentEmbedding`` (.npz) for ``SCANN.place``.
``--map-quality K`` adds to what ``--embed`` or ``--project 2`` prints and pickles whether the map can be believed: trustworthiness,
continuity and the neighbourhood overlap at K neighbours, from exact neighbour ranks computed on the GPU (key "quality" of the pickle).
``--embed-sweep 5,10,15`` draws the map at every perplexity of the list, scores each and the linear map beside them, prints the table,
pickles it as ``embed_sweep_<target>.pickle`` and, with ``--embed-out``, saves the map with the greatest neighbourhood overlap.
``--peaks K [--peaks-level atom|structure] [--peaks-bandwidth H] [--peaks-out FILE]`` clusters the dataset's atoms (or structures) by
density peaks -- no round clusters are assumed; both passes over all pairs run on the GPU, bit-reproducible --, prints the bandwidth, the
leading decision values and each cluster's size and centre, pickles the result as ``peaks_<target>.pickle`` and, with ``--peaks-out``,
saves the labels as a ``LatentPeaks`` (.npz).  ``--density FILE [--density-bandwidth H]`` pickles ``density_<target>.pickle``: per structure
the Gaussian kernel density of its row (or of its atoms' rows) under a saved ``LatentIndex``, for example of the training set.
``--prototypes M [--criticisms C] [--prototypes-level atom|structure] [--prototypes-bandwidth H] [--prototypes-out FILE]`` picks the M atoms
(or structures) that stand for the whole dataset in latent space and the C that those do not stand for (MMD-critic; both greedy loops run
on the GPU in exact integers, bit-reproducible), prints them with the MMD curve, pickles the result as ``prototypes_<target>.pickle`` and,
with ``--prototypes-out``, saves the picked rows as a ``LatentPrototypes`` (.npz).  ``--nearest-prototype FILE`` loads such a file and
pickles ``nearest_prototype_<target>.pickle``: per structure its (or its atoms') nearest prototype and the distance to it.
``--hierarchy MIN_CLUSTER_SIZE [--hierarchy-level atom|structure] [--hierarchy-min-samples 5] [--hierarchy-out FILE]`` clusters the dataset's
atoms (or structures) hierarchically (HDBSCAN; single linkage with ``--hierarchy-min-samples 0``) on the exact minimum spanning tree,
built on the GPU and bit-reproducible: it prints the tree's size and each cluster's size, persistence and exemplar, and how many rows are
noise, pickles the result as ``hierarchy_<target>.pickle`` and, with ``--hierarchy-out``, saves the tree as a ``LatentHierarchy`` (.npz)
and the rows it was built on beside it as ``FILE.index.npz``.  ``--attach FILE --attach-min-cluster-size N`` loads both and pickles
``attach_<target>.pickle``: per structure the label of its row (or of its atoms' rows) under that hierarchy, -1 for noise.
``--duplicates RADIUS [--duplicates-level atom] [--duplicates-out FILE]`` finds the dataset's near-duplicate groups: the structures (or
atoms) whose rows lie within RADIUS of each other in the model's latent space, by the exact radius search on the GPU.  It prints the
number of groups and of redundant rows and pickles the groups (pairs, distances, group per row, the dedup mask ``keep``, and the rows'
dataset indices and atoms) as ``duplicates_<target>.pickle``, or as FILE.  ``--within RADIUS --within-index FILE`` is the leakage report:
it prints how many of the dataset's structures have a row of the saved ``LatentIndex`` FILE, for example of the training set, within
RADIUS, and pickles one dict per structure (count, neighbor_id, distance, position) as ``within_<target>.pickle``.
``--with <dir2>,<dir3>`` runs those trained models (one architecture) in one model set with ``<trained_model>`` over its dataset: each
writes the energy_pre_<target>.pickle / ga_scores_<target>.pickle it would write alone, into its own folder, and when all targets agree
``ensemble_<target>.pickle`` (next to ``<trained_model>``) holds the mean and standard deviation (ddof 1) of the de-normalised predictions."""
import argparse
import os
import pickle
import sys

import numpy as np
import yaml
from sklearn.metrics import mean_absolute_error, r2_score

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "scann--material_amd"))
from scann.models import SCANN  # noqa: E402


def main_with(args, make_set=None):
    """--with: the models of one architecture over the first model's dataset, every batch through one model set.  Each member's ground
    truth and de-normalisation are its own run's: its dataset is prepared from its own config.yaml (its target's values, normalised with
    its own statistics when hyper.scaler is set), so its pickles are the ones ``predict_model.py <its dir>`` writes.  ``make_set(dirs)``:
    the model set (default ``ModelSet(dirs)``)."""
    from scann.models import ModelSet

    dirs = [args.trained_model] + [d for d in args.with_models.split(",") if d]
    configs = [yaml.safe_load(open(os.path.join(d, "config.yaml"))) for d in dirs]
    for d, c in zip(dirs[1:], configs[1:]):  # one dataset, batched alike (the GA scores are padded per batch)
        for k in ("data_energy_path", "data_nei_path", "batch_size"):
            if c["hyper"].get(k) != configs[0]["hyper"].get(k):
                raise SystemExit("--with: %s has hyper.%s = %r, %s has %r; the models of a set run over one dataset"
                                 % (d, k, c["hyper"].get(k), dirs[0], configs[0]["hyper"].get(k)))
    runs = []
    for c in configs:
        run = SCANN(c, mode="data")
        run.prepare_dataset(split=False)
        runs.append(run)
    data = runs[0].dataIter
    ms = make_set(dirs) if make_set is not None else ModelSet(dirs)
    K = len(dirs)
    raw, gas = [[] for _ in range(K)], [[] for _ in range(K)]
    for b in range(len(data)):
        inputs, _ = data[b]
        r = ms.predict(inputs)
        for m in range(K):
            raw[m].append(r["predict_property"][m][:, 0])
            gas[m] += list(r["global_attention"][m])
    preds = []
    for m, (d, run) in enumerate(zip(dirs, runs)):
        t, dm = run.config["hyper"]["target"], run.dataIter
        # main()'s arithmetic: the member's float32 targets as its dataset batches them, its predictions de-normalised with its own mean / std
        y = list(np.array([float(dm.data_energy[i][1]) * dm.converter for i in dm.indexes], "float32"))
        struct_energy = list(np.concatenate(raw[m]) * run.std + run.mean)
        preds.append(struct_energy)
        print("%s (%s): R2 %s, MAE %s" % (d, t, r2_score(struct_energy, y), mean_absolute_error(struct_energy, y)))
        print("Save prediction and GA score to", d)
        pickle.dump(gas[m], open(os.path.join(d, "ga_scores_{}.pickle".format(t)), "wb"))
        pickle.dump([y, struct_energy], open(os.path.join(d, "energy_pre_{}.pickle".format(t)), "wb"))
    targets = [run.config["hyper"]["target"] for run in runs]
    if K >= 2 and len(set(targets)) == 1:
        p = np.asarray(preds, dtype=np.float64)
        pickle.dump({"mean": list(p.mean(axis=0)), "std": list(p.std(axis=0, ddof=1))},
                    open(os.path.join(args.trained_model, "ensemble_{}.pickle".format(targets[0])), "wb"))


def main(args):
    if args.with_models:
        return main_with(args)
    if args.nearest and not 1 <= args.nearest <= 32:
        raise SystemExit("--nearest: K must lie in 1 .. 32, got %d" % args.nearest)
    if not 0 <= args.nearest_cells <= 1024:
        raise SystemExit("--nearest-cells: C must lie in 0 .. 1024 (0: no partition), got %d" % args.nearest_cells)
    if args.match and not 1 <= args.match <= 32:
        raise SystemExit("--match: K must lie in 1 .. 32, got %d" % args.match)
    if args.pair and not 1 <= args.pair <= 32:
        raise SystemExit("--pair: K must lie in 1 .. 32, got %d" % args.pair)
    if args.pair and not args.pair <= args.pair_shortlist <= 32:
        raise SystemExit("--pair-shortlist: S must lie in K = %d .. 32, got %d" % (args.pair, args.pair_shortlist))
    if args.select < 0:
        raise SystemExit("--select: M must be >= 1, got %d" % args.select)
    if args.cluster and not 1 <= args.cluster <= 1024:
        raise SystemExit("--cluster: K must lie in 1 .. 1024, got %d" % args.cluster)
    if args.cluster_iter < 0:
        raise SystemExit("--cluster-iter: N must be >= 0, got %d" % args.cluster_iter)
    check_within_flags(args)
    sweep = check_sweep_flags(args)
    head_targets = check_head_flags(args)
    kernel_head_targets = check_kernel_head_flags(args)
    class_labels = check_class_head_flags(args)
    embed_sweep = check_embed_flags(args)
    check_peaks_flags(args)
    check_prototypes_flags(args)
    check_hierarchy_flags(args)
    config = yaml.safe_load(open(os.path.join(args.trained_model, "config.yaml")))
    if args.project:  # (0: the flag was not given)
        width = int(config["model"]["dense_out" if args.project_level == "structure" else "global_dim"])
        if not 1 <= args.project <= width:
            raise SystemExit("--project: M must lie in 1 .. %d, the width of the %s level, got %d" % (width, args.project_level, args.project))
    target = config["hyper"]["target"]
    print("Load pretrained weight for target ", target)
    scann = SCANN(config, os.path.join(args.trained_model, "models", "model_{}.h5".format(target)), mode="infer")
    print("Load data for trained model: ", config["hyper"]["data_energy_path"])
    scann.prepare_dataset(split=False)
    # the reference loops predict_data over the batches (predict_model.py:49-62); the same per-batch results come out of the
    # pipelined dataset path (batches fused per launch sequence, uploads / launches / downloads overlapped over the streams)
    data = scann.dataIter
    names = [n for n in (args.outputs or "").split(",") if n]
    if names:
        yp, ga, yt, extra = scann.model.predict_dataset(data, want_ga=True, outputs=names)
    else:
        yp, ga, yt = scann.model.predict_dataset(data, want_ga=True)
    struct_energy = list(np.asarray(yp) * scann.std + scann.mean)   # predict_data's de-normalisation (scann_model.py:315-319)
    y = list(yt)
    # GA scores in the reference's shape: one [M, 1] array per structure, M = largest structure of ITS batch (zeros behind the
    # structure's own atoms: the softmax of the -1e9 mask)
    counts = [len(data.data_energy[i][0]) for i in data.indexes]
    off = np.concatenate([[0], np.cumsum(counts)])
    ga_scores = []
    for b0 in range(0, len(counts), data.batch_size):
        sel = range(b0, min(len(counts), b0 + data.batch_size))
        m = max(counts[i] for i in sel)
        for i in sel:
            a = np.zeros((m, 1), dtype=np.float32)
            a[:counts[i], 0] = ga[off[i]:off[i + 1]]
            ga_scores.append(a)
    print(len(y))
    print(r2_score(struct_energy, y), mean_absolute_error(struct_energy, y))
    print("Save prediction and GA score")
    pickle.dump(ga_scores, open(os.path.join(args.trained_model, "ga_scores_{}.pickle".format(target)), "wb"))
    pickle.dump([y, struct_energy], open(os.path.join(args.trained_model, "energy_pre_{}.pickle".format(target)), "wb"))
    for n in names:
        pickle.dump(extra[n], open(os.path.join(args.trained_model, "{}_{}.pickle".format(n, target)), "wb"))
    if args.mc_samples:
        print("Monte Carlo dropout: %d samples per structure" % args.mc_samples)
        mc = {"mean": [], "std": [], "ga_mean": [], "ga_std": []}
        for b in range(len(data)):
            inputs, _ = data[b]
            sel = data.indexes[b * data.batch_size:(b + 1) * data.batch_size]
            r = scann.predict_uncertainty(inputs, samples=args.mc_samples, seed=args.mc_seed, keys=sel)
            mc["mean"] += list(r["predict_property"][:, 0])
            mc["std"] += list(r["predict_property_std"][:, 0])
            mc["ga_mean"] += list(r["global_attention"])
            mc["ga_std"] += list(r["global_attention_std"])
        pickle.dump(mc, open(os.path.join(args.trained_model, "mc_{}.pickle".format(target)), "wb"))
    if args.contributions:
        print("Per-atom contributions:", args.contributions)
        per = []
        for b in range(len(data)):
            inputs, _ = data[b]
            r = scann.atom_contributions(inputs, mode=args.contributions)
            amask = np.asarray(inputs["atom_mask"]).reshape(r["order"].shape) != 0
            for i in range(len(amask)):  # unpadded: one entry per real atom of the structure
                d = {k: v[i][amask[i]] for k, v in r.items() if k != "y"}
                d["y"] = float(r["y"][i, 0])
                # order: indices into the structure's own atoms (the padded positions of real atoms, counted)
                d["order"] = (np.cumsum(amask[i]) - 1)[d["order"]].astype(np.int32)
                per.append(d)
        pickle.dump(per, open(os.path.join(args.trained_model, "contributions_{}.pickle".format(target)), "wb"))
    if args.shapley:
        print("Shapley values of the atoms for the global pooling: %d permutations, seed %d" % (args.shapley, args.shapley_seed))
        per, at = [], 0
        for b in range(len(data)):
            inputs, _ = data[b]
            nb = len(np.asarray(inputs["atom_mask"]))
            # keys: the structure's position in the dataset, so that the batching changes nothing
            r = scann.atom_shapley(inputs, permutations=args.shapley, seed=args.shapley_seed, keys=np.arange(at, at + nb))
            at += nb
            amask = np.asarray(inputs["atom_mask"]).reshape(r["shapley"].shape[:2]) != 0
            for i in range(len(amask)):  # unpadded: one entry per real atom of the structure
                d = {k: r[k][i][amask[i]][:, 0] for k in ("shapley", "stderr", "global_attention")}
                d.update({k: float(r[k][i, 0]) for k in ("y", "baseline", "full")})
                per.append(d)
        pickle.dump(per, open(os.path.join(args.trained_model, "shapley_{}.pickle".format(target)), "wb"))
    if args.rollout:
        print("Attention rollout: residual %g, %s" % (args.rollout_residual, "head mean" if args.rollout_head < 0 else "head %d" % args.rollout_head))
        per = []
        for b in range(len(data)):
            inputs, _ = data[b]
            r = scann.attention_rollout(inputs, residual=args.rollout_residual, head=None if args.rollout_head < 0 else args.rollout_head)
            amask = np.asarray(inputs["atom_mask"]).reshape(r["rollout"].shape[:2]) != 0
            for i in range(len(amask)):  # unpadded: the structure's own atoms
                per.append({"attribution": r["atom_attribution"][i][amask[i], 0], "rollout": r["rollout"][i][np.ix_(amask[i], amask[i])]})
        pickle.dump(per, open(os.path.join(args.trained_model, "rollout_{}.pickle".format(target)), "wb"))
    if args.nearest:
        from scann.models import LatentIndex

        if args.nearest_index:
            index = LatentIndex.load(scann.model, args.nearest_index)
            if args.nearest_cells and len(index):
                index.partition(args.nearest_cells)
            print("Nearest %d rows of %s (%s level, %d rows)" % (args.nearest, args.nearest_index, index.level, len(index)))
        else:  # the dataset itself, every structure queried with its own dataset index left out
            index = scann.build_index(data, level=args.nearest_level, ids=data.indexes, cells=args.nearest_cells or None)
            print("Nearest %d of the dataset's own %d rows (%s level), leave-one-out" % (args.nearest, len(index), index.level))
        per = nearest_records(scann, data, index, args.nearest, exclude=not args.nearest_index)
        if index.partition_args():  # (of the last batch's search)
            print("Nearest: %d cells, %.1f %% of the (query group, row tile) pairs visited" % (
                index.partition_args()[0], 100.0 * index.search_stats()["visited_share"]))
        index.free()
        pickle.dump(per, open(os.path.join(args.trained_model, "nearest_{}.pickle".format(target)), "wb"))
    if args.match:
        from scann.models import LatentIndex

        if args.match_index:
            index = LatentIndex.load(scann.model, args.match_index)
            if index.level != "atom":
                raise SystemExit("--match-index: %s is a %s-level index, matching needs an atom-level one" % (args.match_index, index.level))
            print("Match: %d nearest structures of %s (%d atom rows), %s" % (args.match, args.match_index, len(index), args.match_measure))
        else:  # the dataset itself, every structure queried with its own dataset index left out
            index = scann.build_index(data, level="atom", ids=data.indexes)
            print("Match: %d nearest of the dataset's own structures (%d atom rows), %s, leave-one-out" % (args.match, len(index), args.match_measure))
        try:
            per = match_records(scann, data, index, args.match, args.match_measure, exclude=not args.match_index)
        except ValueError as e:  # (a structure above the atom limit)
            index.free()
            raise SystemExit("--match: %s" % e) from None
        index.free()
        pickle.dump(per, open(os.path.join(args.trained_model, "match_{}.pickle".format(target)), "wb"))
    if args.pair:
        from scann.models import LatentIndex

        if args.pair_index:
            index = LatentIndex.load(scann.model, args.pair_index)
            if index.level != "atom":
                raise SystemExit("--pair-index: %s is a %s-level index, pairing needs an atom-level one" % (args.pair_index, index.level))
            print("Pair: %d of the %d nearest structures of %s (%d atom rows), %s" % (args.pair, args.pair_shortlist, args.pair_index, len(index),
                                                                                      args.pair_measure))
        else:  # the dataset itself, every structure queried with its own dataset index left out
            index = scann.build_index(data, level="atom", ids=data.indexes)
            print("Pair: %d of the %d nearest of the dataset's own structures (%d atom rows), %s, leave-one-out" % (
                args.pair, args.pair_shortlist, len(index), args.pair_measure))
        try:
            per = pair_records(scann, data, index, args.pair, args.pair_shortlist, args.pair_measure, exclude=not args.pair_index)
        except ValueError as e:  # (a structure above the atom limit)
            index.free()
            raise SystemExit("--pair: %s" % e) from None
        index.free()
        pickle.dump(per, open(os.path.join(args.trained_model, "pair_{}.pickle".format(target)), "wb"))
    if args.duplicates is not None:
        pool = scann.build_index(data, level=args.duplicates_level, ids=data.indexes)
        dup = pool.duplicates(args.duplicates)
        dup["id"], dup["atom"] = pool.names()
        pool.free()
        print("Duplicates within %g (%s level): %d rows, %d pairs, %d groups, %d redundant rows" % (
            args.duplicates, args.duplicates_level, len(dup["group"]), len(dup["pairs"]), dup["n_groups"], len(dup["group"]) - dup["n_groups"]))
        pickle.dump(dup, open(args.duplicates_out or os.path.join(args.trained_model, "duplicates_{}.pickle".format(target)), "wb"))
    if args.within is not None:
        from scann.models import LatentIndex

        index = LatentIndex.load(scann.model, args.within_index)
        if index.level != "structure":
            raise SystemExit("--within-index: %s is a %s-level index, the leakage report needs a structure-level one" % (args.within_index, index.level))
        r = scann.within(data, index, args.within)
        print("Within %g of %s (%d rows): %d of %d structures have an indexed row within the radius" % (
            args.within, args.within_index, len(index), int((r["count"] > 0).sum()), len(r["count"])))
        index.free()
        first = r["first"]
        per = [{"predict_property": float(r["predict_property"][i, 0]), "count": int(r["count"][i])} for i in range(len(r["count"]))]
        for i, d in enumerate(per):
            d.update({n: r[n][first[i]:first[i + 1]] for n in ("neighbor_id", "distance", "position")})
        pickle.dump(per, open(os.path.join(args.trained_model, "within_{}.pickle".format(target)), "wb"))
    if args.select:
        from scann.models import LatentIndex

        reference = LatentIndex.load(scann.model, args.select_reference) if args.select_reference else None
        level = reference.level if reference is not None else args.select_level
        pool = scann.build_index(data, level=level, ids=data.indexes)
        print("Select %d of the dataset's %d rows (%s level)%s" % (args.select, len(pool), level, ", farthest from the %d rows of %s" % (
            len(reference), args.select_reference) if reference is not None else ""))
        sel = scann.select_diverse(pool, args.select, reference=reference)
        pool.free()
        if reference is not None:
            reference.free()
        pickle.dump(sel, open(os.path.join(args.trained_model, "selected_{}.pickle".format(target)), "wb"))
    if args.cluster:
        pool = scann.build_index(data, level=args.cluster_level, ids=data.indexes)
        print("Cluster the dataset's %d rows (%s level) into %d clusters" % (len(pool), args.cluster_level, args.cluster))
        res, clustering = scann.cluster(pool, args.cluster, max_iter=args.cluster_iter)
        pool.free()
        print("n_iter %d, converged %s, inertia %.6g" % (res["n_iter"], res["converged"], res["inertia"]))
        for c in range(args.cluster):
            print("cluster %4d: size %8d, medoid id %d atom %d" % (c, res["size"][c], res["medoid_id"][c], res["medoid_atom"][c]))
        pickle.dump(res, open(os.path.join(args.trained_model, "clusters_{}.pickle".format(target)), "wb"))
        if args.cluster_out:
            clustering.save(args.cluster_out)
        clustering.free()
    if sweep:
        pool = scann.build_index(data, level=args.cluster_level, ids=data.indexes)
        print("Choose the number of clusters of the dataset's %d rows (%s level) among %s" % (len(pool), args.cluster_level, sweep))
        try:
            table, clustering = scann.choose_k(pool, sweep, sample=args.cluster_sample or None, max_iter=args.cluster_iter)
        except ValueError as e:
            raise SystemExit("--cluster-sweep: %s" % e)
        finally:
            pool.free()
        print("     k  silhouette       inertia  Calinski-Harabasz  Davies-Bouldin  converged")
        for i, k in enumerate(table["k"]):
            print("%6d  %10.6f  %12.6g  %17.6g  %14.6g  %s" % (k, table["score"][i], table["inertia"][i], table["calinski_harabasz"][i],
                                                              table["davies_bouldin"][i], bool(table["converged"][i])))
        print("best k %d, sizes %s" % (table["best_k"], table["best"]["size"].tolist()))
        pickle.dump(table, open(os.path.join(args.trained_model, "cluster_sweep_{}.pickle".format(target)), "wb"))
        if args.cluster_out:
            clustering.save(args.cluster_out)
        clustering.free()
    if args.project:
        pool = scann.build_index(data, level=args.project_level, ids=data.indexes)
        print("Map the dataset's %d rows (%s level) onto %d principal components" % (len(pool), args.project_level, args.project))
        try:
            res, projection = scann.fit_projection(pool, m=args.project)
        except ValueError as e:  # (fewer than 2 usable rows)
            pool.free()
            raise SystemExit("--project: %s" % e) from None
        res["id"], res["atom"] = pool.names()
        print("n_rows %d, rank %d, total variance %.6g, explained variance ratio %s" % (
            res["n_rows"], res["rank"], res["total_variance"], " ".join("%.4f" % r for r in res["explained_variance_ratio"])))
        if args.map_quality and args.project == 2:
            res["quality"] = print_map_quality(scann, pool, res["coordinates"], args.map_quality, "--project")
        pickle.dump(res, open(os.path.join(args.trained_model, "projection_{}.pickle".format(target)), "wb"))
        if args.project_out:
            projection.save(args.project_out)
        pool.free()
    if head_targets is not None:
        pool = scann.build_index(data, level=args.head_level, ids=data.indexes)
        print("Fit a head for %d target(s) on the dataset's %d rows (%s level)" % (head_targets.shape[1], len(pool), args.head_level))
        try:
            res, head = scann.fit_head(pool, head_targets)
        except ValueError as e:  # (the number of rows, too few labelled ones)
            pool.free()
            raise SystemExit("--fit-head: %s" % e) from None
        res["id"], res["atom"] = pool.names()
        print("n_rows %d" % res["n_rows"])
        print("%-12s %12s %12s %12s %10s %12s %8s" % ("target", "l2", "loo_rmse", "loo_mae", "loo_r2", "fit_rmse", "dof"))
        for k, name in enumerate(res["names"]):
            print("%-12s %12.6g %12.6g %12.6g %10.6f %12.6g %8.2f" % (name, res["l2"][k], res["loo_rmse"][k], res["loo_mae"][k], res["loo_r2"][k],
                                                                   res["fit_rmse"][k], res["dof"][k]))
        pickle.dump(res, open(os.path.join(args.trained_model, "head_{}.pickle".format(target)), "wb"))
        if args.head_out:
            head.save(args.head_out)
        pool.free()
    if args.head:
        from scann.models import LatentHead

        try:
            head = LatentHead.load(scann.model, args.head)
        except ValueError as e:
            raise SystemExit("--head: %s" % e) from None
        print("Evaluate the head of %s (%s level, %d targets: %s)" % (args.head, head.level, head.k, ", ".join(head.names)))
        pickle.dump(head_records(scann, data, head), open(os.path.join(args.trained_model, "head_{}.pickle".format(target)), "wb"))
    if kernel_head_targets is not None:
        pool = scann.build_index(data, level=args.kernel_head_level, ids=data.indexes)
        print("Fit a kernel head for %d target(s) on the dataset's %d rows (%s level, %d landmarks)" % (
            kernel_head_targets.shape[1], len(pool), args.kernel_head_level, args.landmarks))
        try:
            res, head = scann.fit_kernel_head(pool, kernel_head_targets, landmarks=args.landmarks)
        except ValueError as e:  # (the number of rows, too few labelled ones, fewer usable rows than landmarks)
            pool.free()
            raise SystemExit("--fit-kernel-head: %s" % e) from None
        res["id"], res["atom"] = pool.names()
        print("n_rows %d, covering radius %.6g, bandwidth %.6g" % (res["n_rows"], res["covering_radius"], res["bandwidth"]))
        for g, h in enumerate(res["bandwidth_path"]["bandwidth"]):
            print("bandwidth %12.6g  loo_r2 %s" % (h, " ".join("%10.6f" % x for x in res["bandwidth_path"]["loo_r2"][g])))
        print("%-12s %12s %12s %12s %10s %12s %8s" % ("target", "l2", "loo_rmse", "loo_mae", "loo_r2", "fit_rmse", "dof"))
        for k, name in enumerate(res["names"]):
            print("%-12s %12.6g %12.6g %12.6g %10.6f %12.6g %8.2f" % (name, res["l2"][k], res["loo_rmse"][k], res["loo_mae"][k], res["loo_r2"][k],
                                                                   res["fit_rmse"][k], res["dof"][k]))
        pickle.dump(res, open(os.path.join(args.trained_model, "kernel_head_{}.pickle".format(target)), "wb"))
        if args.kernel_head_out:
            head.save(args.kernel_head_out)
        pool.free()
    if args.kernel_head:
        from scann.models import LatentKernelHead

        try:
            head = LatentKernelHead.load(scann.model, args.kernel_head)
        except ValueError as e:
            raise SystemExit("--kernel-head: %s" % e) from None
        print("Evaluate the kernel head of %s (%s level, %d landmarks, %d targets: %s)" % (args.kernel_head, head.level, head.m, head.k, ", ".join(head.names)))
        pickle.dump(head_records(scann, data, head, kernel=True), open(os.path.join(args.trained_model, "kernel_head_{}.pickle".format(target)), "wb"))
    if class_labels is not None:
        pool = scann.build_index(data, level=args.class_head_level, ids=data.indexes)
        print("Fit a classification head on the dataset's %d rows (%s level)" % (len(pool), args.class_head_level))
        try:
            res, head = scann.fit_class_head(pool, class_labels)
        except ValueError as e:  # (the number of rows, too few labelled ones, a class without rows)
            pool.free()
            raise SystemExit("--fit-class-head: %s" % e) from None
        res["id"], res["atom"] = pool.names()
        print("n_rows %d, classes %s, counts %s" % (res["n_rows"], " ".join(str(c) for c in res["classes"]), " ".join(str(c) for c in res["class_count"])))
        print("%12s %12s %12s %10s" % ("l2", "cv_accuracy", "cv_brier", "converged"))
        for i, l2 in enumerate(res["path"]["l2"]):
            print("%12.6g %12.6f %12.6g %10s" % (l2, res["path"]["cv_accuracy"][i], res["path"]["cv_brier"][i], bool(res["path"]["converged"][i])))
        print("l2 %.6g: cv_accuracy %.6f, cv_brier %.6g, cv_log_loss %.6g, fit_accuracy %.6f, %d iterations, %d passes, %s" % (
            res["l2"], res["cv_accuracy"], res["cv_brier"], res["cv_log_loss"], res["fit_accuracy"], res["iterations"], res["passes"], res["stopped"]))
        pickle.dump(res, open(os.path.join(args.trained_model, "class_head_{}.pickle".format(target)), "wb"))
        if args.class_head_out:
            head.save(args.class_head_out)
        pool.free()
    if args.class_head:
        from scann.models import LatentClassHead

        try:
            head = LatentClassHead.load(scann.model, args.class_head)
        except ValueError as e:
            raise SystemExit("--class-head: %s" % e) from None
        print("Evaluate the classification head of %s (%s level, classes %s)" % (args.class_head, head.level, " ".join(str(c) for c in head.classes)))
        pickle.dump(class_head_records(scann, data, head), open(os.path.join(args.trained_model, "class_head_{}.pickle".format(target)), "wb"))
    if args.embed:
        pool = scann.build_index(data, level=args.embed_level, ids=data.indexes)
        print("Embed the dataset's %d rows (%s level, perplexity %g)" % (len(pool), args.embed_level, args.embed_perplexity))
        try:
            res, emb = scann.fit_embedding(pool, perplexity=args.embed_perplexity)
        except ValueError as e:  # (too many or too few rows, a row with a non-finite component)
            pool.free()
            raise SystemExit("--embed: %s" % e) from None
        res["id"], res["atom"] = pool.names()
        print("n_rows %d, %d edges, learning rate %g: kl %.6f -> %.6f, z %.6g" % (
            len(emb), res["n_edges"], res["learning_rate"], res["kl_init"], res["kl"], res["z"]))
        if args.map_quality:
            res["quality"] = print_map_quality(scann, pool, res, args.map_quality, "--embed")
        pickle.dump(res, open(os.path.join(args.trained_model, "embedding_{}.pickle".format(target)), "wb"))
        if args.embed_out:
            emb.save(args.embed_out)
        pool.free()
    if embed_sweep:
        pool = scann.build_index(data, level=args.embed_level, ids=data.indexes)
        print("Choose the perplexity of the map of the dataset's %d rows (%s level) among %s" % (len(pool), args.embed_level, embed_sweep))
        try:
            table, emb = scann.choose_perplexity(pool, embed_sweep, k=args.map_quality or 15)
        except ValueError as e:
            raise SystemExit("--embed-sweep: %s" % e) from None
        finally:
            pool.free()
        print("perplexity  neighbour overlap  trustworthiness  continuity      LCMC  R_NX area        kl")
        for i, p in enumerate(table["perplexity"]):
            print("%10s  %17.6f  %15.6f  %10.6f  %8.6f  %9.6f  %8.6f" % (p if isinstance(p, str) else "%g" % p, table["neighbour_overlap"][i],
                                                                        table["trustworthiness"][i], table["continuity"][i], table["lcmc"][i],
                                                                        table["rnx_auc"][i], table["kl"][i]))
        print("best perplexity %g" % table["best_perplexity"])
        pickle.dump(table, open(os.path.join(args.trained_model, "embed_sweep_{}.pickle".format(target)), "wb"))
        if args.embed_out:
            emb.save(args.embed_out)
    if args.peaks:
        pool = scann.build_index(data, level=args.peaks_level, ids=data.indexes)
        print("Density peaks of the dataset's %d rows (%s level), %d clusters" % (len(pool), args.peaks_level, args.peaks))
        try:
            res, peaks = scann.density_peaks(pool, k=args.peaks, bandwidth=args.peaks_bandwidth or "auto")
        except ValueError as e:  # (too few rows, a row with a non-finite component under the automatic bandwidth)
            pool.free()
            raise SystemExit("--peaks: %s" % e) from None
        print("bandwidth %.6g, %d eligible rows; decision values: %s" % (
            res["bandwidth"], res["n_eligible"], " ".join("%.6g" % g for g in res["decision"][:args.peaks + 3])))
        for c in range(len(res["size"])):
            print("cluster %4d: size %8d, centre id %d atom %d" % (c, res["size"][c], res["centre_id"][c], res["centre_atom"][c]))
        res["id"], res["atom"] = pool.names()
        pickle.dump(res, open(os.path.join(args.trained_model, "peaks_{}.pickle".format(target)), "wb"))
        if args.peaks_out:
            peaks.save(args.peaks_out)
        pool.free()
    if args.prototypes:
        pool = scann.build_index(data, level=args.prototypes_level, ids=data.indexes)
        print("Prototypes of the dataset's %d rows (%s level): %d prototypes, %d criticisms" % (
            len(pool), args.prototypes_level, args.prototypes, args.criticisms))
        try:
            res, protos = scann.prototypes(pool, args.prototypes, criticisms=args.criticisms, bandwidth=args.prototypes_bandwidth or "auto")
        except ValueError as e:  # (too many rows for M, a row with a non-finite component under the automatic bandwidth)
            pool.free()
            raise SystemExit("--prototypes: %s" % e) from None
        print("bandwidth %.6g, %d eligible rows" % (res["bandwidth"], res["n_eligible"]))
        for s in range(res["count"]):
            print("prototype %4d: id %d atom %d, mmd2 %.6g%s" % (s, res["id"][s], res["atom"][s], res["mmd2"][s],
                                                                ", stands for %d rows" % res["size"][s] if "size" in res else ""))
        for s in range(len(res["criticism_position"])):
            print("criticism %4d: id %d atom %d, witness %.6g" % (s, res["criticism_id"][s], res["criticism_atom"][s], res["criticism_witness"][s]))
        pickle.dump(res, open(os.path.join(args.trained_model, "prototypes_{}.pickle".format(target)), "wb"))
        if args.prototypes_out and protos is not None:
            protos.save(args.prototypes_out)
        pool.free()
    if args.nearest_prototype:
        from scann.models import LatentPrototypes

        try:
            protos = LatentPrototypes.load(scann.model, args.nearest_prototype)
        except ValueError as e:
            raise SystemExit("--nearest-prototype: %s" % e) from None
        print("Nearest of the %d prototypes of %s (%s level)" % (protos.m, args.nearest_prototype, protos.level))
        pickle.dump(nearest_prototype_records(scann, data, protos),
                    open(os.path.join(args.trained_model, "nearest_prototype_{}.pickle".format(target)), "wb"))
        protos.free()
    if args.density:
        from scann.models import LatentIndex

        try:
            index = LatentIndex.load(scann.model, args.density)
        except ValueError as e:
            raise SystemExit("--density: %s" % e) from None
        print("Kernel density under %s (%s level, %d rows), bandwidth %g" % (args.density, index.level, len(index), args.density_bandwidth))
        pickle.dump(density_records(scann, data, index, args.density_bandwidth),
                    open(os.path.join(args.trained_model, "density_{}.pickle".format(target)), "wb"))
        index.free()
    if args.hierarchy:
        pool = scann.build_index(data, level=args.hierarchy_level, ids=data.indexes)
        print("Hierarchy of the dataset's %d rows (%s level), min_samples %d, min_cluster_size %d" % (
            len(pool), args.hierarchy_level, args.hierarchy_min_samples, args.hierarchy))
        try:
            res, tree = scann.hierarchy(pool, min_samples=args.hierarchy_min_samples, min_cluster_size=args.hierarchy)
        except ValueError as e:  # (too many rows)
            pool.free()
            raise SystemExit("--hierarchy: %s" % e) from None
        print("%d eligible rows, %d edges in %d rounds; %d clusters, %d rows are noise" % (
            res["n_eligible"], len(res["w"]), res["rounds"], len(res["size"]), int((res["label"] < 0).sum())))
        for c in range(len(res["size"])):
            print("cluster %4d: size %8d, persistence %.6g, exemplar id %d atom %d" % (
                c, res["size"][c], res["persistence"][c], tree.ids[res["exemplar"][c]], tree.atoms[res["exemplar"][c]]))
        res["id"], res["atom"] = pool.names()
        pickle.dump(res, open(os.path.join(args.trained_model, "hierarchy_{}.pickle".format(target)), "wb"))
        if args.hierarchy_out:
            tree.save(args.hierarchy_out)
            pool.save(args.hierarchy_out + ".index.npz")
        pool.free()
    if args.attach:
        from scann.models import LatentHierarchy, LatentIndex

        try:
            tree = LatentHierarchy.load(scann.model, args.attach)
            index = LatentIndex.load(scann.model, args.attach + ".index.npz")
        except (ValueError, OSError) as e:
            raise SystemExit("--attach: %s" % e) from None
        print("Labels under %s (%s level, %d rows), min_cluster_size %d" % (args.attach, index.level, len(index), args.attach_min_cluster_size))
        try:
            records = attach_records(scann, data, tree, index, args.attach_min_cluster_size)
        except ValueError as e:
            index.free()
            raise SystemExit("--attach: %s" % e) from None
        pickle.dump(records, open(os.path.join(args.trained_model, "attach_{}.pickle".format(target)), "wb"))
        index.free()


def check_hierarchy_flags(args):
    """--hierarchy / --attach and their companions checked before anything is loaded"""
    if args.hierarchy and args.hierarchy < 2:
        raise SystemExit("--hierarchy: MIN_CLUSTER_SIZE must be >= 2, got %d" % args.hierarchy)
    if args.hierarchy_out and not args.hierarchy:
        raise SystemExit("--hierarchy-out: needs --hierarchy")
    if not 0 <= args.hierarchy_min_samples <= 31:
        raise SystemExit("--hierarchy-min-samples: must lie in 0 .. 31, got %d" % args.hierarchy_min_samples)
    if args.attach_min_cluster_size and not args.attach:
        raise SystemExit("--attach-min-cluster-size: needs --attach")
    if args.attach and args.attach_min_cluster_size < 2:
        raise SystemExit("--attach: needs --attach-min-cluster-size N >= 2")


def check_sweep_flags(args):
    """--cluster-sweep's list of k as integers (None without the flag); SystemExit for a bad list or flags that need it"""
    if not args.cluster_sweep:
        if args.cluster_sample:
            raise SystemExit("--cluster-sample: needs --cluster-sweep")
        return None
    if args.cluster:
        raise SystemExit("--cluster-sweep: chooses k itself, drop --cluster")
    try:
        ks = [int(x) for x in args.cluster_sweep.split(",")]
    except ValueError:
        raise SystemExit("--cluster-sweep: a comma-separated list of integers, got %r" % args.cluster_sweep)
    if not ks or min(ks) < 1 or max(ks) > 1024:
        raise SystemExit("--cluster-sweep: every k must lie in 1 .. 1024, got %r" % args.cluster_sweep)
    if args.cluster_sample < 0:
        raise SystemExit("--cluster-sample: M must be >= 1, got %d" % args.cluster_sample)
    return ks


def attach_records(scann, data, tree, index, min_cluster_size):
    """--attach: one unpadded dict per structure of the dataset, in dataset order"""
    per = []
    atom = index.level == "atom"
    for b in range(len(data)):
        inputs, _ = data[b]
        r = scann.attach(inputs, tree, index, min_cluster_size)
        amask = np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0
        for i in range(len(amask)):
            d = {"predict_property": float(r["predict_property"][i, 0])}
            for key in ("label", "nearest_id", "nearest_atom", "nearest_distance"):
                d[key] = r[key][i][amask[i]] if atom else r[key][i]
            per.append(d)
    return per


def check_peaks_flags(args):
    """--peaks / --density and their companions checked before anything is loaded"""
    if args.peaks < 0:
        raise SystemExit("--peaks: K must be >= 1, got %d" % args.peaks)
    if (args.peaks_out or args.peaks_bandwidth) and not args.peaks:
        raise SystemExit("--peaks-out / --peaks-bandwidth: need --peaks")
    if args.peaks_bandwidth < 0 or args.peaks_bandwidth != args.peaks_bandwidth:
        raise SystemExit("--peaks-bandwidth: H must be > 0, got %g" % args.peaks_bandwidth)
    if args.density_bandwidth and not args.density:
        raise SystemExit("--density-bandwidth: needs --density")
    if args.density and not args.density_bandwidth > 0:
        raise SystemExit("--density: needs --density-bandwidth H > 0 (--peaks prints the one it used)")


def check_prototypes_flags(args):
    """--prototypes and its companions checked before anything is loaded"""
    if args.prototypes < 0:
        raise SystemExit("--prototypes: M must be >= 1, got %d" % args.prototypes)
    if (args.criticisms or args.prototypes_out or args.prototypes_bandwidth) and not args.prototypes:
        raise SystemExit("--criticisms / --prototypes-out / --prototypes-bandwidth: need --prototypes")
    if args.criticisms < 0:
        raise SystemExit("--criticisms: C must be >= 0, got %d" % args.criticisms)
    if args.prototypes_bandwidth < 0 or args.prototypes_bandwidth != args.prototypes_bandwidth:
        raise SystemExit("--prototypes-bandwidth: H must be > 0, got %g" % args.prototypes_bandwidth)


def nearest_prototype_records(scann, data, protos):
    """--nearest-prototype: one unpadded dict per structure of the dataset, in dataset order"""
    per = []
    atom = protos.level == "atom"
    for b in range(len(data)):
        inputs, _ = data[b]
        r = scann.nearest_prototype(inputs, protos)
        amask = np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0
        for i in range(len(amask)):
            d = {"predict_property": float(r["predict_property"][i, 0])}
            for key in ("prototype", "prototype_id", "distance") + (("prototype_atom",) if atom else ()):
                d[key] = r[key][i][amask[i]] if atom else r[key][i]
            per.append(d)
    return per


def density_records(scann, data, index, bandwidth):
    """--density: one unpadded dict per structure of the dataset, in dataset order"""
    per = []
    atom = index.level == "atom"
    for b in range(len(data)):
        inputs, _ = data[b]
        r = scann.density(inputs, index, bandwidth)
        amask = np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0
        for i in range(len(amask)):
            d = {"predict_property": float(r["predict_property"][i, 0])}
            for key in ("density", "sum"):
                d[key] = r[key][i][amask[i]] if atom else r[key][i]
            per.append(d)
    return per


def print_map_quality(scann, pool, coords, k, flag):
    """--map-quality: the scores of a map of ``pool``'s rows, printed; the dict that goes into the pickle"""
    graph = (coords["neighbor_position"], coords["neighbor_dist2"]) if isinstance(coords, dict) else None  # (--embed has searched already)
    try:
        q = scann.map_quality(pool, coords, k=k, graph=graph)
    except ValueError as e:
        pool.free()
        raise SystemExit("--map-quality (%s): %s" % (flag, e)) from None
    print("map quality at k = %d: trustworthiness %.6f, continuity %.6f, neighbour overlap %.6f, LCMC %.6f, R_NX area %.6f" % (
        q["k"], q["trustworthiness"], q["continuity"], q["neighbour_overlap"], q["lcmc"], q["rnx_auc"]))
    return q


def check_embed_flags(args):
    """--embed and its companions checked before anything is loaded; the perplexities of --embed-sweep, or None"""
    if args.embed_out and not (args.embed or args.embed_sweep):
        raise SystemExit("--embed-out: needs --embed")
    if args.embed and not 2 <= args.embed_perplexity <= 15:
        raise SystemExit("--embed-perplexity: P must lie in 2 .. 15, got %g" % args.embed_perplexity)
    if args.map_quality and not 1 <= args.map_quality <= 31:
        raise SystemExit("--map-quality: K must lie in 1 .. 31, got %d" % args.map_quality)
    if args.map_quality and not (args.embed or args.embed_sweep or args.project == 2):
        raise SystemExit("--map-quality: needs --embed, --embed-sweep or --project 2")
    if args.embed and args.embed_sweep:
        raise SystemExit("--embed-sweep: draws its own maps, leave --embed out")
    if not args.embed_sweep:
        return None
    try:
        ps = [float(p) for p in args.embed_sweep.split(",")]
    except ValueError:
        raise SystemExit("--embed-sweep: a comma-separated list of perplexities, got %r" % args.embed_sweep) from None
    if any(not 2 <= p <= 15 for p in ps) or any(b <= a for a, b in zip(ps, ps[1:])):
        raise SystemExit("--embed-sweep: ascending distinct perplexities in 2 .. 15, got %r" % args.embed_sweep)
    return ps


def check_class_head_flags(args):
    """--fit-class-head / --class-head checked before anything is loaded: the labels as int64 [N], or None without --fit-class-head"""
    if args.fit_class_head and args.class_head:
        raise SystemExit("--fit-class-head and --class-head: fit a classification head or evaluate one, not both")
    if args.class_head_out and not args.fit_class_head:
        raise SystemExit("--class-head-out: needs --fit-class-head")
    if args.class_head and not os.path.isfile(args.class_head):
        raise SystemExit("--class-head: no such file: %s" % args.class_head)
    if not args.fit_class_head:
        return None
    try:
        t = np.load(args.fit_class_head, allow_pickle=False)
    except (OSError, ValueError) as e:
        raise SystemExit("--fit-class-head: cannot read %s: %s" % (args.fit_class_head, e)) from None
    if t.dtype.kind not in "iu" or t.ndim != 1 or t.shape[0] < 4:
        raise SystemExit("--fit-class-head: %s must hold integers of shape [N], N >= 4, got %s %s" % (args.fit_class_head, t.dtype, t.shape))
    n_classes = len(np.unique(t[t != -1]))
    if not 2 <= n_classes <= 16:
        raise SystemExit("--fit-class-head: %s must hold 2 .. 16 distinct labels other than -1, got %d" % (args.fit_class_head, n_classes))
    return np.ascontiguousarray(t, dtype=np.int64)


def class_head_records(scann, data, head):
    """--class-head: one unpadded dict per structure of the dataset, in dataset order"""
    per = []
    atom = head.level == "atom"
    for b in range(len(data)):
        inputs, _ = data[b]
        r = scann.predict_class_head(inputs, head)
        amask = np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0
        for i in range(len(amask)):
            d = {"predict_property": float(r["y"][i, 0])}
            for key in ("probability", "label", "confidence", "entropy"):
                d[key] = r[key][i][amask[i]] if atom else r[key][i]
            per.append(d)
    return per


def check_kernel_head_flags(args):
    """--fit-kernel-head / --kernel-head checked before anything is loaded: the targets as fp32 [N, K], or None without --fit-kernel-head"""
    if args.fit_kernel_head and args.kernel_head:
        raise SystemExit("--fit-kernel-head and --kernel-head: fit a kernel head or evaluate one, not both")
    if args.kernel_head_out and not args.fit_kernel_head:
        raise SystemExit("--kernel-head-out: needs --fit-kernel-head")
    if args.kernel_head and not os.path.isfile(args.kernel_head):
        raise SystemExit("--kernel-head: no such file: %s" % args.kernel_head)
    if not args.fit_kernel_head:
        return None
    try:
        t = np.load(args.fit_kernel_head, allow_pickle=False)
    except (OSError, ValueError) as e:
        raise SystemExit("--fit-kernel-head: cannot read %s: %s" % (args.fit_kernel_head, e)) from None
    if t.dtype.kind not in "fiu" or t.ndim not in (1, 2) or (t.ndim == 2 and not 1 <= t.shape[1] <= 16) or t.shape[0] < 3:
        raise SystemExit("--fit-kernel-head: %s must hold numbers of shape [N] or [N, K], N >= 3, 1 <= K <= 16, got %s %s" % (
            args.fit_kernel_head, t.dtype, t.shape))
    if not 1 <= args.landmarks <= 1024 or args.landmarks >= t.shape[0]:
        raise SystemExit("--landmarks: M must lie in 1 .. 1024 and below the %d rows of the targets, got %d" % (t.shape[0], args.landmarks))
    return np.ascontiguousarray(t.reshape(len(t), -1), dtype=np.float32)


def check_head_flags(args):
    """--fit-head / --head checked before anything is loaded: the targets as fp32 [N, K], or None without --fit-head"""
    if args.fit_head and args.head:
        raise SystemExit("--fit-head and --head: fit a head or evaluate one, not both")
    if args.head_out and not args.fit_head:
        raise SystemExit("--head-out: needs --fit-head")
    if args.head and not os.path.isfile(args.head):
        raise SystemExit("--head: no such file: %s" % args.head)
    if not args.fit_head:
        return None
    try:
        t = np.load(args.fit_head, allow_pickle=False)
    except (OSError, ValueError) as e:
        raise SystemExit("--fit-head: cannot read %s: %s" % (args.fit_head, e)) from None
    if t.dtype.kind not in "fiu" or t.ndim not in (1, 2) or (t.ndim == 2 and not 1 <= t.shape[1] <= 16) or t.shape[0] < 3:
        raise SystemExit("--fit-head: %s must hold numbers of shape [N] or [N, K], N >= 3, 1 <= K <= 16, got %s %s" % (args.fit_head, t.dtype, t.shape))
    return np.ascontiguousarray(t.reshape(len(t), -1), dtype=np.float32)


def head_records(scann, data, head, kernel=False):
    """--head / --kernel-head: one unpadded dict per structure of the dataset, in dataset order"""
    per = []
    atom = head.level == "atom"
    for b in range(len(data)):
        inputs, _ = data[b]
        r = scann.predict_kernel_head(inputs, head) if kernel else scann.predict_head(inputs, head)
        amask = np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0
        for i in range(len(amask)):
            d = {"predict_property": float(r["y"][i, 0])}
            for key in ("prediction", "std", "leverage") + (("support",) if kernel else ()):
                d[key] = r[key][i][amask[i]] if atom else r[key][i]
            per.append(d)
    return per


def check_within_flags(args):
    """--duplicates / --within: a radius >= 0 each, and --within needs the index it searches"""
    for flag, value in (("--duplicates", args.duplicates), ("--within", args.within)):
        if value is not None and not value >= 0:
            raise SystemExit("%s: RADIUS must be >= 0, got %r" % (flag, value))
    if args.within is not None and not args.within_index:
        raise SystemExit("--within: needs --within-index FILE, the saved LatentIndex to search")
    if args.within is None and args.within_index:
        raise SystemExit("--within-index: needs --within RADIUS")


def nearest_records(scann, data, index, k, exclude):
    """--nearest: one unpadded dict per structure of the dataset, in dataset order"""
    per = []
    atom = index.level == "atom"
    for b in range(len(data)):
        inputs, _ = data[b]
        sel = data.indexes[b * data.batch_size:(b + 1) * data.batch_size]
        r = scann.nearest(inputs, index, k=k, exclude_ids=sel if exclude else None)
        amask = np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0
        for i in range(len(amask)):
            d = {"predict_property": float(r["predict_property"][i, 0])}
            if atom:  # the structure's own atoms
                d.update(distance=r["distance"][i][amask[i]], neighbor_id=r["neighbor_id"][i][amask[i]],
                         neighbor_atom=r["neighbor_atom"][i][amask[i]], latent_distance=r["latent_distance"][i][amask[i], 0])
            else:
                d.update(distance=r["distance"][i], neighbor_id=r["neighbor_id"][i], latent_distance=float(r["latent_distance"][i, 0]))
            per.append(d)
    return per


def match_records(scann, data, index, k, measure, exclude):
    """--match: one unpadded dict per structure of the dataset, in dataset order"""
    per = []
    for b in range(len(data)):
        inputs, _ = data[b]
        sel = data.indexes[b * data.batch_size:(b + 1) * data.batch_size]
        r = scann.match_structures(inputs, index, k=k, measure=measure, exclude_ids=sel if exclude else None)
        amask = np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0
        for i in range(len(amask)):  # matched_*: the structure's own atoms
            per.append({"predict_property": float(r["predict_property"][i, 0]), "distance": r["distance"][i], "neighbor_id": r["neighbor_id"][i],
                        "neighbor_size": r["neighbor_size"][i], "parts": r["parts"][i], "matched_atom": r["matched_atom"][i][amask[i]],
                        "matched_distance": r["matched_distance"][i][amask[i]]})
    return per


def pair_records(scann, data, index, k, shortlist, measure, exclude):
    """--pair: one unpadded dict per structure of the dataset, in dataset order"""
    per = []
    for b in range(len(data)):
        inputs, _ = data[b]
        sel = data.indexes[b * data.batch_size:(b + 1) * data.batch_size]
        r = scann.pair_structures(inputs, index, k=k, shortlist=shortlist, measure=measure, exclude_ids=sel if exclude else None)
        amask = np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0
        for i in range(len(amask)):  # paired_*: the structure's own atoms
            d = {n: r[n][i] for n in ("distance", "neighbor_id", "neighbor_size", "shortlist_distance", "shortlist_place", "surplus")}
            d.update(predict_property=float(r["predict_property"][i, 0]), paired_atom=r["paired_atom"][i][amask[i]],
                     paired_distance=r["paired_distance"][i][amask[i]])
            per.append(d)
    return per


def parser():
    p = argparse.ArgumentParser()
    p.add_argument("trained_model", type=str, help="Target trained model path for loading")
    p.add_argument("--outputs", type=str, default="",
                   help="comma-separated outputs to pickle as well: local_attention_<k>, after_Lc, bf_property")
    p.add_argument("--mc-samples", type=int, default=0,
                   help="Monte Carlo dropout samples per structure (>= 2; 0: none): pickles mc_<target>.pickle")
    p.add_argument("--mc-seed", type=int, default=0, help="seed of the Monte Carlo dropout masks")
    p.add_argument("--contributions", type=str, default="", choices=["", "leave_one_out", "deletion", "insertion"],
                   help="also pickle per-atom contributions (the prediction with atoms left out of the global pooling) as "
                        "contributions_<target>.pickle: one dict per structure, unpadded, in the units of the target")
    p.add_argument("--shapley", type=int, default=0,
                   help="permutations per structure (0: none) for sampled Shapley values of the atoms for the global pooling: pickles "
                        "shapley_<target>.pickle, one dict per structure, unpadded, in the units of the target")
    p.add_argument("--shapley-seed", type=int, default=0, help="seed of the Shapley permutations")
    p.add_argument("--rollout", action="store_true",
                   help="also pickle the attention rollout (the GA scores traced back to the atoms through the local-attention layers) "
                        "as rollout_<target>.pickle: one dict per structure, unpadded (attribution [n], rollout [n, n])")
    p.add_argument("--rollout-residual", type=float, default=0.5, help="weight of the skip connection in every layer of the rollout, 0 .. 1")
    p.add_argument("--rollout-head", type=int, default=-1, help="one attention head instead of the mean over the heads (-1)")
    p.add_argument("--nearest", type=int, default=0,
                   help="also pickle the K (1 .. 32) nearest structures of the dataset in latent space, leave-one-out, and their mean "
                        "distance as nearest_<target>.pickle: one dict per structure, unpadded, ids = dataset indices")
    p.add_argument("--nearest-level", type=str, default="structure", choices=["structure", "atom"],
                   help="structure: bf_property rows, one per structure; atom: after_Lc rows, one per atom")
    p.add_argument("--nearest-index", type=str, default="",
                   help="a saved LatentIndex (.npz) to search instead of the dataset itself; nothing is left out")
    p.add_argument("--nearest-cells", type=int, default=0,
                   help="partition the searched index into C (1 .. 1024) cells, so that --nearest skips the cells out of reach; the "
                        "answers are the same in every byte (default 0: compare every row)")
    p.add_argument("--match", type=int, default=0,
                   help="also pickle the K (1 .. 32) structures of the dataset made of the most similar local structures (sets of after_Lc "
                        "rows compared on the GPU), leave-one-out, with the atom-to-atom correspondence, as match_<target>.pickle: one dict "
                        "per structure, unpadded, ids = dataset indices")
    p.add_argument("--match-measure", type=str, default="chamfer", choices=["chamfer", "hausdorff", "cover"],
                   help="chamfer: mean nearest-atom distance both ways; hausdorff: the worst one; cover: the query's atoms only")
    p.add_argument("--match-index", type=str, default="",
                   help="a saved atom-level LatentIndex (.npz) to match against instead of the dataset itself; nothing is left out")
    p.add_argument("--pair", type=int, default=0,
                   help="also pickle the K (1 .. 32) structures of the dataset nearest under the one-to-one pairing of their atoms with the "
                        "structure's (the exact assignment over the after_Lc rows, solved on the GPU), leave-one-out, with the atom map, as "
                        "pair_<target>.pickle: one dict per structure, unpadded, ids = dataset indices")
    p.add_argument("--pair-shortlist", type=int, default=32,
                   help="the candidates that are paired: the S (K .. 32) nearest structures under --pair-measure")
    p.add_argument("--pair-measure", type=str, default="chamfer", choices=["chamfer", "hausdorff", "cover"],
                   help="the measure that shortlists the candidates, as --match-measure")
    p.add_argument("--pair-index", type=str, default="",
                   help="a saved atom-level LatentIndex (.npz) to pair against instead of the dataset itself; nothing is left out")
    p.add_argument("--duplicates", type=float, default=None, metavar="RADIUS",
                   help="find the dataset's near-duplicate groups: rows within RADIUS of each other in latent space (the exact radius "
                        "search on the GPU); prints the groups and the redundant rows, pickles duplicates_<target>.pickle")
    p.add_argument("--duplicates-level", type=str, default="structure", choices=["structure", "atom"],
                   help="structure: bf_property rows, one per structure; atom: after_Lc rows, one per atom")
    p.add_argument("--duplicates-out", type=str, default="", help="write the groups to FILE instead")
    p.add_argument("--within", type=float, default=None, metavar="RADIUS",
                   help="the leakage report: how many of the dataset's structures have a row of --within-index within RADIUS; pickles "
                        "within_<target>.pickle, one dict per structure")
    p.add_argument("--within-index", type=str, default="", help="the saved structure-level LatentIndex (.npz) that --within searches")
    p.add_argument("--select", type=int, default=0,
                   help="also pickle the M most diverse structures of the dataset (greedy k-center selection in latent space) as "
                        "selected_<target>.pickle: one dict with ids (dataset indices), atoms and radii in pick order")
    p.add_argument("--select-level", type=str, default="structure", choices=["structure", "atom"],
                   help="structure: bf_property rows, one per structure; atom: after_Lc rows, one per atom")
    p.add_argument("--select-reference", type=str, default="",
                   help="a saved LatentIndex (.npz) of what is labelled already: the picks are the dataset's rows farthest from it")
    p.add_argument("--cluster", type=int, default=0,
                   help="also cluster the dataset's rows in latent space into K clusters (k-means on the GPU, bit-reproducible) and pickle "
                        "labels, distances, centres, sizes and medoids as clusters_<target>.pickle")
    p.add_argument("--cluster-level", type=str, default="atom", choices=["atom", "structure"],
                   help="atom: after_Lc rows, one per atom; structure: bf_property rows, one per structure")
    p.add_argument("--cluster-iter", type=int, default=50, help="at most N updates of the centres")
    p.add_argument("--cluster-out", type=str, default="", help="save the centres as a LatentClustering (.npz) for SCANN.assign")
    p.add_argument("--cluster-sweep", type=str, default="", metavar="K1,K2,...",
                   help="choose the number of clusters: k-means for every k of the list, scored by the silhouette of its labels (exact on "
                        "the GPU, bit-reproducible); prints the table, pickles it as cluster_sweep_<target>.pickle; --cluster-out saves the "
                        "best k's centres")
    p.add_argument("--cluster-sample", type=int, default=0, metavar="M",
                   help="--cluster-sweep scores M sampled rows instead of all (their values are exact: every mean is over all rows)")
    p.add_argument("--project", type=int, default=0,
                   help="also map the dataset's rows onto the M leading principal components of the latent space (moments on the GPU, "
                        "bit-reproducible) and pickle coordinates and distances as projection_<target>.pickle")
    p.add_argument("--project-level", type=str, default="structure", choices=["atom", "structure"],
                   help="rows to map: one per structure (bf_property) or one per atom (after_Lc)")
    p.add_argument("--project-out", type=str, default="", help="save the map as a LatentProjection (.npz) for SCANN.project")
    p.add_argument("--fit-head", type=str, default="",
                   help="TARGETS.npy, [N] or [N, K] values of another property (NaN: unlabelled), one row per structure or atom of the dataset: "
                        "fit a linear readout head on the latent space (ridge, exact leave-one-out on the GPU) and pickle head_<target>.pickle")
    p.add_argument("--head-level", type=str, default="structure", choices=["atom", "structure"],
                   help="rows to regress on: one per structure (bf_property) or one per atom (after_Lc)")
    p.add_argument("--head-out", type=str, default="", help="save the fitted head as a LatentHead (.npz) for SCANN.predict_head")
    p.add_argument("--head", type=str, default="",
                   help="a saved LatentHead (.npz): pickle its prediction, standard deviation and leverage per structure as head_<target>.pickle")
    p.add_argument("--fit-class-head", type=str, default="",
                   help="LABELS.npy, integers [N] (one per structure, or per atom in dataset order with --class-head-level atom; -1: unlabelled): "
                        "fit a classification head on the latent space (softmax regression, cross-validated on the GPU) and pickle "
                        "class_head_<target>.pickle")
    p.add_argument("--class-head-level", type=str, default="structure", choices=["atom", "structure"],
                   help="rows of --fit-class-head: bf_property per structure or after_Lc per atom")
    p.add_argument("--class-head-out", type=str, default="", help="save the fitted head as a LatentClassHead (.npz) for SCANN.predict_class_head")
    p.add_argument("--class-head", type=str, default="",
                   help="a saved LatentClassHead (.npz): pickle its probabilities, label, confidence and entropy per structure as "
                        "class_head_<target>.pickle")
    p.add_argument("--fit-kernel-head", type=str, default="",
                   help="TARGETS.npy as --fit-head takes it: fit a nonlinear readout head on Gaussian features to landmarks of the latent space "
                        "(features, moments and leave-one-out on the GPU) and pickle kernel_head_<target>.pickle")
    p.add_argument("--landmarks", type=int, default=256, metavar="M", help="landmarks of --fit-kernel-head: the M most diverse rows (1 .. 1024)")
    p.add_argument("--kernel-head-level", type=str, default="structure", choices=["atom", "structure"],
                   help="rows to regress on: one per structure (bf_property) or one per atom (after_Lc)")
    p.add_argument("--kernel-head-out", type=str, default="", help="save the fitted head as a LatentKernelHead (.npz) for SCANN.predict_kernel_head")
    p.add_argument("--kernel-head", type=str, default="",
                   help="a saved LatentKernelHead (.npz): pickle its prediction, standard deviation, leverage and support per structure as "
                        "kernel_head_<target>.pickle")
    p.add_argument("--peaks", type=int, default=0, metavar="K",
                   help="also cluster the dataset's rows in latent space into K clusters by density peaks (both passes over all pairs on "
                        "the GPU, bit-reproducible) and pickle labels, densities, parents, centres and the decision values as "
                        "peaks_<target>.pickle")
    p.add_argument("--peaks-level", type=str, default="atom", choices=["atom", "structure"],
                   help="rows --peaks clusters: one per atom (after_Lc) or one per structure (bf_property)")
    p.add_argument("--peaks-bandwidth", type=float, default=0.0, metavar="H",
                   help="kernel width of --peaks (default: automatic, from the 31st-nearest-neighbour distances)")
    p.add_argument("--peaks-out", type=str, default="", help="save the labels as a LatentPeaks (.npz)")
    p.add_argument("--prototypes", type=int, default=0, metavar="M",
                   help="also pick the M rows of the dataset that stand for all of it in latent space (MMD-critic, the greedy loop on the GPU in "
                        "exact integers): prototypes_<target>.pickle")
    p.add_argument("--criticisms", type=int, default=0, metavar="C", help="with --prototypes: also the C rows the prototypes do not stand for")
    p.add_argument("--prototypes-level", type=str, default="atom", choices=["atom", "structure"],
                   help="rows --prototypes picks from: one per atom (after_Lc) or one per structure (bf_property)")
    p.add_argument("--prototypes-bandwidth", type=float, default=0.0, metavar="H",
                   help="kernel width of --prototypes (default: automatic, from the 31st-nearest-neighbour distances)")
    p.add_argument("--prototypes-out", type=str, default="", help="save the picked rows as a LatentPrototypes (.npz)")
    p.add_argument("--nearest-prototype", type=str, default="", metavar="FILE",
                   help="a saved LatentPrototypes: pickle every structure's (or atom's) nearest prototype as nearest_prototype_<target>.pickle")
    p.add_argument("--hierarchy", type=int, default=0, metavar="MIN_CLUSTER_SIZE",
                   help="also cluster the dataset's rows in latent space hierarchically (HDBSCAN on the exact minimum spanning tree, built on "
                        "the GPU, bit-reproducible), keeping clusters of at least MIN_CLUSTER_SIZE rows; the result is pickled as "
                        "hierarchy_<target>.pickle")
    p.add_argument("--hierarchy-level", type=str, default="atom", choices=["atom", "structure"],
                   help="rows --hierarchy clusters: one per atom (after_Lc) or one per structure (bf_property)")
    p.add_argument("--hierarchy-min-samples", type=int, default=5, metavar="S",
                   help="the neighbour whose distance is a row's core distance, 1 .. 31; 0: single linkage")
    p.add_argument("--hierarchy-out", type=str, default="", help="save the tree as a LatentHierarchy (.npz) and its rows as FILE.index.npz")
    p.add_argument("--attach", type=str, default="", metavar="TREE",
                   help="also pickle the label of every structure (or atom) under a saved LatentHierarchy (.npz, with TREE.index.npz beside "
                        "it) as attach_<target>.pickle")
    p.add_argument("--attach-min-cluster-size", type=int, default=0, metavar="N", help="min_cluster_size of --attach")
    p.add_argument("--density", type=str, default="", metavar="INDEX",
                   help="also pickle the Gaussian kernel density of every structure (or atom) under a saved LatentIndex (.npz) as "
                        "density_<target>.pickle")
    p.add_argument("--density-bandwidth", type=float, default=0.0, metavar="H", help="kernel width of --density")
    p.add_argument("--embed", action="store_true",
                   help="draw the neighbour embedding (t-SNE) of the dataset's rows in two dimensions (exact pair repulsion on the GPU, "
                        "bit-reproducible) and pickle embedding_<target>.pickle")
    p.add_argument("--embed-level", type=str, default="structure", choices=["atom", "structure"],
                   help="rows to embed: one per structure (bf_property) or one per atom (after_Lc)")
    p.add_argument("--embed-perplexity", type=float, default=10.0, metavar="P", help="perplexity of --embed (2 .. 15)")
    p.add_argument("--embed-out", type=str, default="", help="save the map as a LatentEmbedding (.npz) for SCANN.place")
    p.add_argument("--map-quality", type=int, default=0, metavar="K",
                   help="score the map of --embed, --embed-sweep or --project 2 at K neighbours (1 .. 31): trustworthiness, continuity and "
                        "neighbourhood overlap from exact neighbour ranks on the GPU")
    p.add_argument("--embed-sweep", type=str, default="", metavar="P1,P2,...",
                   help="choose the perplexity: draw the map at every perplexity of the list, score each (at --map-quality K, default 15) "
                        "and the linear map, pickle embed_sweep_<target>.pickle")
    p.add_argument("--with", dest="with_models", type=str, default="",
                   help="comma-separated trained model folders of the same architecture, run in one model set with this one")
    return p


if __name__ == "__main__":
    main(parser().parse_args())
