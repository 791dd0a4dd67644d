"""Fine-tuning a pretrained model: which tensors train, at what rate, and which are drawn afresh.

Three keys of ``hyper`` (all absent by default; ``train.py --freeze / --lr-scale / --reset``):

``freeze``    a list of ``fnmatch`` patterns over tensor names (``scann_weight_name``: ``embed_atom/embeddings``,
              ``local_attention_3/query/kernel``, ``bf_property/bias``, ...): the matched tensors get learning-rate scale 0 -- Keras
              ``trainable = False``: the optimiser leaves them and their moments alone, and the training backward stops above the lowest
              stage that still holds a trained tensor (``scann_set_lr_scale``, include/scann_hip.h).
``lr_scale``  a mapping pattern -> factor (finite, >= 0) on the learning rate of the matched tensors.
``reset``     a list of patterns: the matched tensors are drawn again from the model's own initialisers after the pretrained checkpoint
              is loaded -- the head for a new target.

The rules are read in one order -- the ``freeze`` patterns as factor 0, then the ``lr_scale`` entries in the order of the mapping -- and
the LAST rule that matches a tensor wins, so ``freeze: ["*"]`` with ``lr_scale: {"bf_property/*": 1, "predict_property/*": 1}`` trains the
head alone.  A pattern that matches no tensor is a ``ValueError`` that names it; so is a set of rules that leaves nothing to train.
"""
from __future__ import annotations

import fnmatch
import math

import numpy as np


def _as_patterns(value, key):
    if value is None:
        return []
    if isinstance(value, str):
        value = [value]
    out = []
    for p in value:
        if not isinstance(p, str) or not p:
            raise ValueError("hyper.%s: patterns are non-empty strings, got %r" % (key, p))
        out.append(p)
    return out


def _matches(names, pattern, key):
    hit = [i for i, n in enumerate(names) if fnmatch.fnmatchcase(n, pattern)]
    if not hit:
        raise ValueError("hyper.%s: pattern %r matches no tensor of the model" % (key, pattern))
    return hit


def scale_rules(freeze=None, lr_scale=None):
    """-> [(key, pattern, factor)] in the order they are applied"""
    rules = [("freeze", p, 0.0) for p in _as_patterns(freeze, "freeze")]
    if lr_scale is not None:
        if not hasattr(lr_scale, "items"):
            raise ValueError("hyper.lr_scale is a mapping pattern -> factor, got %r" % (lr_scale,))
        for p, s in lr_scale.items():
            _as_patterns([p], "lr_scale")
            try:
                f = float(s)
            except (TypeError, ValueError):
                raise ValueError("hyper.lr_scale[%r]: %r is not a number" % (p, s)) from None
            if not math.isfinite(f) or f < 0.0:
                raise ValueError("hyper.lr_scale[%r]: the factor must be finite and >= 0, got %r" % (p, s))
            rules.append(("lr_scale", p, f))
    return rules


def lr_scale_vector(names, freeze=None, lr_scale=None):
    """Per-tensor factors in the order of ``names`` (float32), or None when neither key is given (the unscaled optimiser)."""
    names = list(names)
    rules = scale_rules(freeze, lr_scale)
    if not rules:
        return None
    vec = np.ones(len(names), dtype=np.float32)
    for key, pattern, f in rules:
        vec[_matches(names, pattern, key)] = f
    if not np.any(vec > 0):
        raise ValueError("hyper.freeze / hyper.lr_scale leave no tensor to train (every factor is 0)")
    return vec


def lr_scale_of_config(config, names):
    hy = config.get("hyper", {})
    return lr_scale_vector(names, hy.get("freeze"), hy.get("lr_scale"))


def trainable_counts(specs, vec):
    """(trainable, total) parameter counts of a model with weight specs [(name, shape)] under the factors ``vec`` (None: all)"""
    sizes = [int(np.prod(shape)) for _, shape in specs]
    total = int(sum(sizes))
    if vec is None:
        return total, total
    return int(sum(n for n, s in zip(sizes, vec) if s > 0)), total


def reset_weights(weights, specs, patterns, seed=None):
    """A copy of ``weights`` with the tensors that ``patterns`` match drawn from the model's own initialisers
    (``keras_default_init``: Glorot-uniform kernels, zero biases, ...).  The draw depends on ``seed`` and the model's tensor list
    only -- not on which tensors are reset -- and ``seed=None`` takes fresh entropy.  -> (weights, names that were reset)"""
    from .scann_model import keras_default_init

    names = [n for n, _ in specs]
    hit = set()
    for p in _as_patterns(patterns, "reset"):
        hit.update(_matches(names, p, "reset"))
    out = dict(weights)
    if not hit:
        return out, []
    fresh = keras_default_init(specs, seed)
    done = [names[i] for i in sorted(hit)]
    for n in done:
        out[n] = fresh[n]
    return out, done


def parse_pattern_list(text):
    """``--freeze`` / ``--reset``: comma-separated patterns -> list (None for an empty argument)"""
    if text is None:
        return None
    items = [t.strip() for t in str(text).split(",") if t.strip()]
    return items or None


def parse_scale_list(text):
    """``--lr-scale PATTERN=S,...`` -> {pattern: factor} in the order given (None for an empty argument)"""
    if text is None:
        return None
    out = {}
    for item in [t.strip() for t in str(text).split(",") if t.strip()]:
        pattern, sep, value = item.rpartition("=")
        if not sep or not pattern.strip():
            raise ValueError("--lr-scale: expected PATTERN=S, got %r" % item)
        try:
            out[pattern.strip()] = float(value)
        except ValueError:
            raise ValueError("--lr-scale: %r is not a number (in %r)" % (value, item)) from None
    return out or None
