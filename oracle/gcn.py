"""Oracle: the Modulated-GCN denoiser's graph convs in float64, cut the way the HIP kernels cut them, on any device.  Test infrastructure only.

Each function restates the reference in its own association order (``oracle.model.modulated_graph_conv`` / ``_bn`` / ``_graph_conv``:
modulated_gcn_conv.py:39-50, modulated_gcn.py:21-28, :38-42, :99-116) without folding BatchNorm into the mix:

* ``hidden_conv``   ehm_gcn_hidden_layer: _GraphConv hid -> hid, optionally + residual
* ``input_conv``    ehm_gcn_input_layer: the input conv with the step-invariant projections hoisted, exactly as include/egohmr_hip.h states it
                    above ehm_gcn_set_uncond_mode (vis-gated h_img, h_oth, tvec, x @ Wx; pass map; uncond mode)
* ``input_rows``    ehm_gcn_input_layer_rows: the same epilogue on ready-made pre-activations [rows, 2, hid]
* ``output_conv``   ehm_gcn_output_layer: gconv_output + the visibility fuse of the two passes (egohmr.py:247-256) with pass-map slots
* ``denoiser``      all of them chained as ModulatedGCN.forward runs them inside the sampler (input conv, residual blocks, output conv)

A layer is a dict of tensors: W [2,K,N], M [24,N], adj2 [24,24], bias [N] and, for a conv with BatchNorm(eval) + ReLU, bn_weight, bn_bias,
bn_mean, bn_var [N].  Everything is promoted to float64 on the device of the activations.
"""
from __future__ import annotations

import torch

BN_EPS = 1e-5        # BatchNorm1d default (modulated_gcn.py:16)


def _f64(t, dev):
    return torch.as_tensor(t).to(device=dev, dtype=torch.float64)


def sym_adjacency(adj, adj2):
    """(a.T + a) / 2 of a = adj + adj2 (modulated_gcn_conv.py:43-44)."""
    a = adj + adj2
    return (a.T + a) / 2


def mix(h0, h1, layer, adj):
    """modulated_gcn_conv.py:45-50 on the two branch responses h0 = x W[0], h1 = x W[1] ([..., 24, N] float64): (a*E) @ (M*h0) +
    (a*(1-E)) @ (M*h1) + bias."""
    dev = h0.device
    a = sym_adjacency(_f64(adj, dev), _f64(layer["adj2"], dev))
    E = torch.eye(a.size(0), dtype=a.dtype, device=dev)
    M = _f64(layer["M"], dev)
    return torch.matmul(a * E, M * h0) + torch.matmul(a * (1 - E), M * h1) + _f64(layer["bias"], dev)


def bn_relu(y, layer):
    """BatchNorm1d(eval) over the channel axis, then ReLU (modulated_gcn.py:21-28, oracle.model._bn); identity without BatchNorm."""
    if layer.get("bn_weight") is None:
        return y
    dev = y.device
    y = (y - _f64(layer["bn_mean"], dev)) / torch.sqrt(_f64(layer["bn_var"], dev) + BN_EPS) * _f64(layer["bn_weight"], dev) \
        + _f64(layer["bn_bias"], dev)
    return torch.relu(y)


def epilogue(h0, h1, layer, adj, residual=None):
    """mix -> BatchNorm -> ReLU [-> + residual (modulated_gcn.py:42: res + out)]."""
    y = bn_relu(mix(h0, h1, layer, adj), layer)
    return y if residual is None else residual + y


def hidden_conv(x, layer, adj, residual=None):
    """_GraphConv (+ residual) on x [bodies, 24, K] -> [bodies, 24, N]."""
    W = _f64(layer["W"], x.device)
    return epilogue(torch.matmul(x, W[0]), torch.matmul(x, W[1]), layer, adj, residual)


def input_pre(h_img, h_oth, vis, x, Wx, tvec, passes=1, mask_items=None, masks_whole_condition=False):
    """The two pre-activations of the hoisted input conv for every virtual body (include/egohmr_hip.h, ehm_gcn_input_layer):
        pre_k = (p==0 ? vis[b,j] * h_img[b,k,:] : 0) + h_oth[b,k,:] + tvec[k,:] + x[b,j,0:6] @ Wx[k]
    (h_oth dropped in the second pass when masks_whole_condition).  Virtual bodies: [0, B) the conditional pass, then the second pass of
    mask_items (every item when None).  Returns (pre0, pre1) [vbodies, 24, N]."""
    dev = x.device
    h_img, h_oth, Wx, tvec = (_f64(t, dev) for t in (h_img, h_oth, Wx, tvec))
    x = _f64(x, dev)
    B = x.shape[0]
    xj = x.view(B, 24, 6)
    v = _f64(vis, dev).view(B, 24, 1)
    out = []
    for k in range(2):
        p0 = v * h_img[:, k].unsqueeze(1) + h_oth[:, k].unsqueeze(1) + tvec[k] + torch.matmul(xj, Wx[k])
        if passes == 2:
            items = torch.arange(B, device=dev) if mask_items is None else torch.as_tensor(mask_items, device=dev).long()
            oth = 0.0 if masks_whole_condition else h_oth[items, k].unsqueeze(1)
            p1 = oth + tvec[k] + torch.matmul(xj[items], Wx[k])
            p0 = torch.cat([p0, p1], 0)
        out.append(p0)
    return out[0], out[1]


def input_conv(h_img, h_oth, vis, x, Wx, tvec, layer, adj, passes=1, mask_items=None, masks_whole_condition=False):
    """ehm_gcn_input_layer: [vbodies, 24, N] float64."""
    p0, p1 = input_pre(h_img, h_oth, vis, x, Wx, tvec, passes, mask_items, masks_whole_condition)
    return epilogue(p0, p1, layer, adj)


def input_rows(pre, layer, adj):
    """ehm_gcn_input_layer_rows: pre [bodies * 24, 2, N] -> [bodies, 24, N]."""
    pre = _f64(pre, pre.device).view(-1, 24, 2, pre.shape[-1])
    return epilogue(pre[:, :, 0], pre[:, :, 1], layer, adj)


def fuse(out, vis, B, passes=1, mask_slot=None):
    """egohmr.py:247-256 on the output conv's [vbodies, 24, 6]: x0[b, j] = vis[b, j] ? out[b, j] : out[B + slot(b), j] (passes == 2; an item
    without a second pass has every joint visible), x0 = out[:B] (passes == 1).  Returns [B, 144]."""
    if passes == 1:
        return out[:B].reshape(B, 144)
    dev = out.device
    own = torch.arange(B, device=dev)
    slot = own if mask_slot is None else torch.as_tensor(mask_slot, device=dev).long()
    second = out[torch.where(slot >= 0, B + slot, own)]      # (an item without a second pass - every joint visible - takes its own rows)
    v = torch.as_tensor(vis, device=dev).bool().view(B, 24, 1)
    return torch.where(v, out[:B], second).reshape(B, 144)


def output_conv(X, layer, adj, vis=None, B=None, passes=1, mask_slot=None):
    """ehm_gcn_output_layer: X [vbodies, 24, K] -> x0 [B, 144]."""
    out = hidden_conv(X, layer, adj)
    return fuse(out, vis, X.shape[0] if B is None else B, passes, mask_slot)


def denoiser(h_img, h_oth, vis, x, Wx, tvec, layers, adj, passes=1, mask_items=None, mask_slot=None, masks_whole_condition=False):
    """The denoiser call of one sampling step: layers = [input conv, hidden convs (pairs: gconv1, gconv2 of a residual block) ..., output conv].
    Returns (x0 [B, 144], the activations in front of every conv)."""
    h = input_conv(h_img, h_oth, vis, x, Wx, tvec, layers[0], adj, passes, mask_items, masks_whole_condition)
    acts = [h]
    hidden = layers[1:-1]
    for b in range(len(hidden) // 2):
        r = h
        h = hidden_conv(h, hidden[2 * b], adj)
        acts.append(h)
        h = hidden_conv(h, hidden[2 * b + 1], adj, residual=r)
        acts.append(h)
    return output_conv(h, layers[-1], adj, vis, x.shape[0], passes, mask_slot), acts
