"""Float64 restatement of oracle.model.resnet_pointnet (models/respointnet.py:33-97) that also returns every intermediate the backward of
egohmr_amd/pointnet_grad.py touches, the closed-form backward of one pass written out by hand, and margin(): how far a forward is from a ReLU kink or
a max-pool tie.  Pure torch on the CPU; shared by tests/test_pointnet_autograd_cpu.py and tests/test_gpu_pointnet_autograd.py."""
from __future__ import annotations

import numpy as np
import torch

PARAM_NAMES = (("fc_pos_0.weight", "fc_pos_0.bias") +
               tuple(f"block_{b}.{n}" for b in range(4) for n in ("fc_0.weight", "fc_0.bias", "fc_1.weight", "fc_1.bias", "shortcut.weight")) +
               ("fc_c.weight", "fc_c.bias"))
PREFIX = "scene_enc."


def manifest(H, out_dim):
    """(name, shape) of the PointNet's parameters at hidden width H: the scene_enc.* rows of egohmr_amd.synthetic.egohmr_manifest."""
    m = [("scene_enc.fc_pos_0.weight", (2 * H, 3)), ("scene_enc.fc_pos_0.bias", (2 * H,))]
    for b in range(4):
        p = f"scene_enc.block_{b}."
        m += [(p + "fc_0.weight", (H, 2 * H)), (p + "fc_0.bias", (H,)), (p + "fc_1.weight", (H, H)), (p + "fc_1.bias", (H,)),
              (p + "shortcut.weight", (H, 2 * H))]
    return m + [("scene_enc.fc_c.weight", (out_dim, H)), ("scene_enc.fc_c.bias", (out_dim,))]


def make_weights(H, out_dim, seed=0, zero_fc1=False):
    """The project's synthetic weights (synthetic.make_state_dict's recipe) at width H as float64 tensors; zero_fc1: fc_1.weight = 0, the reference's
    initialisation (respointnet.py:86)."""
    from egohmr_amd import synthetic as syn
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in syn.make_state_dict(seed, manifest=manifest(H, out_dim)).items()}
    if zero_fc1:
        for b in range(4):
            sd[f"scene_enc.block_{b}.fc_1.weight"].zero_()
    return sd


def make_points(B, N, seed=0):
    g = np.random.Generator(np.random.PCG64(7000 + seed))
    return torch.from_numpy(g.uniform(-1.0, 1.0, size=(B, N, 3)))


def argmax_lowest(net):
    """[B,N,C] -> [B,C] int64: the lowest row that maximises each column; a NaN counts as the maximum."""
    N = net.shape[1]
    nan = torch.isnan(net)
    mx = torch.where(nan, torch.full_like(net, float("-inf")), net).max(dim=1, keepdim=True)[0]
    hit = torch.where(nan.any(dim=1, keepdim=True), nan, net == mx)
    rows = torch.arange(N).view(1, N, 1).expand_as(net)
    return torch.where(hit, rows, torch.full_like(rows, N)).min(dim=1)[0]


def forward(sd, pts, p=PREFIX):
    """-> (out [B,out_dim], dict): net0, and per block the lists x (its input, [B,N,2H]), h, net (its output net'), pooled (max of net'), arg.
    The pool is a gather at `arg`, so autograd through this function follows the tie rule (lowest row)."""
    lin = torch.nn.functional.linear
    net0 = lin(pts, sd[p + "fc_pos_0.weight"], sd[p + "fc_pos_0.bias"])
    it = dict(net0=net0, x=[], h=[], net=[], pooled=[], arg=[])
    x = net0
    for b in range(4):
        q = p + f"block_{b}."
        if b:
            x = torch.cat([it["net"][-1], it["pooled"][-1].unsqueeze(1).expand_as(it["net"][-1])], dim=2)
        h = lin(torch.relu(x), sd[q + "fc_0.weight"], sd[q + "fc_0.bias"])
        net = lin(torch.relu(h), sd[q + "fc_1.weight"], sd[q + "fc_1.bias"]) + lin(x, sd[q + "shortcut.weight"])
        arg = argmax_lowest(net.detach())
        pooled = net.gather(1, arg.unsqueeze(1)).squeeze(1)
        for k, v in (("x", x), ("h", h), ("net", net), ("pooled", pooled), ("arg", arg)):
            it[k].append(v)
    out = lin(torch.relu(it["pooled"][-1]), sd[p + "fc_c.weight"], sd[p + "fc_c.bias"])
    return out, it


def margin(sd, pts):
    """The smallest of: min|v| / max|v| over every tensor a ReLU reads (net0, every block's x including its pooled half, every h, the final pooled
    vector), and - for N >= 2 - over every pooled column the gap between its two largest values divided by max|net'|."""
    with torch.no_grad():
        _, it = forward(sd, pts)
    m = float("inf")
    relu_in = [it["net0"]] + it["x"] + it["h"] + [it["pooled"][-1]]
    for v in relu_in:
        m = min(m, float(v.abs().min()) / float(v.abs().max()))
    if pts.shape[1] >= 2:
        for net in it["net"]:
            top = net.topk(2, dim=1)[0]
            m = min(m, float((top[:, 0] - top[:, 1]).min()) / float(net.abs().max()))
    return m


def backward_by_hand(sd, pts, it, gout, p=PREFIX):
    """The backward of egohmr_amd/pointnet_grad.py in float64 (scatter at arg, gates, per-body sums; no autograd): -> (pbar, dict name -> gradient)."""
    H = sd[p + "fc_c.weight"].shape[1]
    B, N, _ = pts.shape
    g = {}
    pooled = it["pooled"][3]
    g["fc_c.weight"] = gout.T @ torch.relu(pooled)
    g["fc_c.bias"] = gout.sum(0)
    gpool = (gout @ sd[p + "fc_c.weight"]) * (pooled > 0)
    gnet = None
    rows = torch.arange(N).view(1, N, 1)
    for b in (3, 2, 1, 0):
        q = p + f"block_{b}."
        W0, W1, S = sd[q + "fc_0.weight"], sd[q + "fc_1.weight"], sd[q + "shortcut.weight"]
        G = (rows == it["arg"][b].unsqueeze(1)) * gpool.unsqueeze(1)
        if gnet is not None:
            G = G + gnet
        rh = torch.relu(it["h"][b])
        dh = (G @ W1) * (rh > 0)
        sdh, sG = dh.sum(1), G.sum(1)
        g[f"block_{b}.fc_1.weight"] = torch.einsum("bno,bni->oi", G, rh)
        g[f"block_{b}.fc_1.bias"] = G.sum((0, 1))
        g[f"block_{b}.fc_0.bias"] = dh.sum((0, 1))
        if b:
            net, pin = it["net"][b - 1], it["pooled"][b - 1]
            gnet = (dh @ W0[:, :H]) * (net > 0) + G @ S[:, :H]
            gpool = (sdh @ W0[:, H:]) * (pin > 0) + sG @ S[:, H:]
            g[f"block_{b}.fc_0.weight"] = torch.cat([torch.einsum("bno,bni->oi", dh, torch.relu(net)), sdh.T @ torch.relu(pin)], dim=1)
            g[f"block_{b}.shortcut.weight"] = torch.cat([torch.einsum("bno,bni->oi", G, net), sG.T @ pin], dim=1)
        else:
            net0 = it["net0"]
            n0bar = (dh @ W0) * (net0 > 0) + G @ S
            g["block_0.fc_0.weight"] = torch.einsum("bno,bni->oi", dh, torch.relu(net0))
            g["block_0.shortcut.weight"] = torch.einsum("bno,bni->oi", G, net0)
            g["fc_pos_0.weight"] = torch.einsum("bnc,bnk->ck", n0bar, pts)
            g["fc_pos_0.bias"] = n0bar.sum((0, 1))
            pbar = n0bar @ sd[p + "fc_pos_0.weight"]
    return pbar, g


def autograd_reference(sd, pts, gout):
    """torch.autograd.grad through forward(): -> (out, intermediates (detached graph values), pbar, dict name -> gradient)."""
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items()}
    x = pts.clone().requires_grad_()
    out, it = forward(leaves, x)
    gr = torch.autograd.grad(out, [x] + [leaves[PREFIX + n] for n in PARAM_NAMES], gout)
    det = lambda v: [t.detach() for t in v] if isinstance(v, list) else v.detach()
    return out.detach(), {k: det(v) for k, v in it.items()}, gr[0], dict(zip(PARAM_NAMES, gr[1:]))
