#!/usr/bin/env python3
"""CLI with the reference's interface (predict_model.py:95-100): load ``<trained_model>/config.yaml`` and
``<trained_model>/models/model_<target>.h5`` in infer mode, predict the whole dataset, pickle GA scores and
predictions next to the model.  ``--outputs after_Lc,local_attention_2,bf_property`` also pickles each named output as
``<name>_<target>.pickle``: one array per structure, laid out as the padded predict of its batch returns it.
``--mc-samples T [--mc-seed S]`` also pickles Monte Carlo dropout estimates as ``mc_<target>.pickle``: a dict with the de-normalised
mean and standard deviation of the prediction per structure and the mean and standard deviation of its GA scores (one [M, 1] array
per structure, as ga_scores), each structure keyed by its index in the dataset."""
import argparse
import os
import pickle
import sys

import numpy as np
import yaml
from sklearn.metrics import mean_absolute_error, r2_score

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "scann--material_amd"))
from scann.models import SCANN  # noqa: E402


def main(args):
    config = yaml.safe_load(open(os.path.join(args.trained_model, "config.yaml")))
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


def parser():
    p = argparse.ArgumentParser()
    p.add_argument("trained_model", type=str, help="Target trained model path for loading")
    p.add_argument("--outputs", type=str, default="",
                   help="comma-separated outputs to pickle as well: local_attention_<k>, after_Lc, bf_property")
    p.add_argument("--mc-samples", type=int, default=0,
                   help="Monte Carlo dropout samples per structure (>= 2; 0: none): pickles mc_<target>.pickle")
    p.add_argument("--mc-seed", type=int, default=0, help="seed of the Monte Carlo dropout masks")
    return p


if __name__ == "__main__":
    main(parser().parse_args())
