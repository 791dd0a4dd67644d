"""Reference for the input gradients (HipModel.input_gradients / scann_input_grads): the graph of create_model (scann_model.py:362-447)
restated in torch on the PACKED layout with the float inputs -- neighbour distance, Voronoi weight, ring features, cgcnn features -- as
autograd leaves.  tests/torch_ref.forward_packed builds those tensors from the batch itself, so it cannot differentiate with respect to
them; tests/test_input_grads_host.py checks this restatement against finite differences of forward_packed.  Inference semantics: no
Dropout.  Test-only."""
import math

import numpy as np
import pytest

pytest.importorskip("torch")

import torch_ref  # noqa: E402


def forward(config, weights, pk, dist, wgt, ring=None, cgcnn=None, dtype="float64"):
    """y [n_struct] for the packed batch `pk` whose edge distances / weights (and ring / cgcnn features) are the given tensors"""
    import torch
    import torch.nn.functional as F

    dt = getattr(torch, dtype)
    cfg = config["model"]
    W = {k: torch.tensor(np.asarray(v), dtype=dt) for k, v in weights.items()}
    d, H = cfg["local_dim"], cfg["num_head"]
    hd = d // H

    def lin(x, p):
        return F.linear(x, W[p + "/kernel"].T, W[p + "/bias"])

    def ln(x, p):
        return F.layer_norm(x, (x.shape[-1],), W[p + "/gamma"], W[p + "/beta"], eps=1e-6)

    def gauss(x, stop):  # GaussianExpansion, width 0.5 (custom_layers.py:51,63-65)
        c = torch.tensor(np.linspace(0, stop, 20, dtype="float32"), dtype=dt)
        return torch.exp(-((x[:, None] - c[None, :]) ** 2) / 0.25)

    col = torch.tensor(pk.edge_col, dtype=torch.long)
    row = torch.tensor(np.repeat(np.arange(pk.n_atom), np.diff(pk.edge_offset)), dtype=torch.long)
    A, E = pk.n_atom, pk.n_edge
    v = lin(cgcnn, "embed_atom") if cfg["feature"] == "cgcnn" else F.embedding(torch.tensor(pk.atomic, dtype=torch.long), W["embed_atom/embeddings"])
    if cfg["use_ring"]:
        v = torch.cat([v, lin(ring, "extra_embed")], -1)
    c = F.silu(lin(v, "dense_embed"))
    gd = gauss(dist, cfg["gaussian_d"])
    if cfg["g_update"]:
        geom = F.silu(lin(gd, "neighbor_d")) * F.silu(lin(gauss(wgt, math.pi * 2), "neighbor_w"))
    for i in range(cfg["n_attention"]):
        p = "local_attention_%d" % i
        cn = c[col]
        if cfg["g_update"]:
            geom = ln(F.silu(lin(torch.cat([c[row], geom, cn], -1), p + "/filter_geo")) + geom, p + "/layer_norm_g")
            g = geom
        else:
            g = F.silu(lin(gd, p + "/filter_geo")) * wgt[:, None]
        q = lin(c, p + "/query")
        k = lin(cn * g, p + "/key")
        e = ((q[row] * hd ** -0.5).view(E, H, hd) * k.view(E, H, hd)).sum(-1)
        attn = torch.zeros_like(e)
        off = pk.edge_offset
        for a in range(A):
            if off[a + 1] > off[a]:
                attn[off[a]:off[a + 1]] = F.softmax(e[off[a]:off[a + 1]], 0)
        ctx = ln(torch.zeros(A, d, dtype=dt).index_add_(0, row, (attn[:, :, None] * k.view(E, H, hd)).reshape(E, d)) + q, p + "/layer_norm")
        if cfg["use_attn_norm"]:
            r = "residual_norm_%d" % i
            c = ln(ctx + lin(F.silu(lin(ctx, r + "/dense_1")), r + "/dense_2"), r + "/layer_norm")
        else:
            c = ctx
    z = F.silu(lin(c, "after_Lc"))
    gq, gk = lin(z, "global_attention/query"), lin(z, "global_attention/key")
    ys = []
    for s in range(pk.n_struct):
        a0, a1 = pk.mol_offset[s], pk.mol_offset[s + 1]
        en = gk[a0:a1] @ gq[a0:a1].T
        agg = (en - torch.diag(torch.diag(en))).sum(-1)
        if cfg["use_ga_norm"]:
            agg = agg / torch.linalg.vector_norm(agg)
        rep = (F.softmax(agg, 0)[:, None] * gk[a0:a1]).sum(0)
        y = lin(F.silu(lin(rep, "bf_property")), "predict_property")
        if config.get("hyper", {}).get("target") == "e_b":
            y = torch_ref._mrelu(y)  # backward: the identity (custom_layers.py:6-15)
        ys.append(y)
    return torch.stack(ys).reshape(-1)


def input_grads(config, weights, pk, dtype="float64"):
    """(y [n_struct], {input name: d y_s / d input}) -- every structure's gradients in one backward of sum(y) (structures are
    independent).  Names as HipModel.input_gradients returns them for a PackedBatch: neighbor_distance / neighbor_weight [n_edge],
    ring_aromatic [n_atom, 2] (use_ring), atomic [n_atom, 92] (feature cgcnn)."""
    import torch

    dt = getattr(torch, dtype)
    cfg = config["model"]
    leaves = {"neighbor_distance": torch.tensor(pk.edge_dist, dtype=dt, requires_grad=True),
              "neighbor_weight": torch.tensor(pk.edge_weight, dtype=dt, requires_grad=True)}
    if cfg["use_ring"]:
        leaves["ring_aromatic"] = torch.tensor(pk.ring, dtype=dt, requires_grad=True)
    if cfg["feature"] == "cgcnn":
        leaves["atomic"] = torch.tensor(pk.cgcnn, dtype=dt, requires_grad=True)
    y = forward(config, weights, pk, leaves["neighbor_distance"], leaves["neighbor_weight"], leaves.get("ring_aromatic"),
                leaves.get("atomic"), dtype)
    y.sum().backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy().astype(np.float64) for k, v in leaves.items()}
    return y.detach().numpy().astype(np.float64), grads
