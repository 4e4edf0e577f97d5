"""CPU: the float64 denoiser-conv references of oracle.gcn (the references of tests/test_gpu_gcn.py), pinned to the oracle's own restatement
(oracle.model._graph_conv / modulated_graph_conv / modulated_gcn) and to the reference's goldens g4_gcn_tiny / g4_gconv_1024."""
import os

import numpy as np
import torch

from egohmr_amd import synthetic as syn
from oracle import gcn as og
from oracle import model as om


def _layer(sd, p, bn=True):
    """oracle.model parameter names -> an oracle.gcn layer"""
    c = p + ".gconv" if bn else p            # (a conv without BatchNorm: gconv_output.W, not gconv_output.gconv.W)
    L = {"W": sd[c + ".W"], "M": sd[c + ".M"], "adj2": sd[c + ".adj2"], "bias": sd[c + ".bias"]}
    if bn:
        L.update(bn_weight=sd[p + ".bn.weight"], bn_bias=sd[p + ".bn.bias"], bn_mean=sd[p + ".bn.running_mean"], bn_var=sd[p + ".bn.running_var"])
    return L


def _sd(seed, cin, hid, blocks):
    man = [(n.replace("diffusion_model.", ""), s) for n, s in syn.egohmr_manifest(hid_dim=hid, num_blocks=blocks, with_backbone=False)
           if n.startswith("diffusion_model.")]
    man = [(n, (2, cin, s[2]) if n == "gconv_input.0.gconv.W" else s) for n, s in man]
    return {k: torch.from_numpy(np.asarray(v)).double() for k, v in syn.make_state_dict(seed=seed, manifest=man).items()}


def test_hidden_and_output_conv_match_the_oracle():
    g = np.random.Generator(np.random.PCG64(3))
    sd = _sd(11, 64, 64, 1)
    adj = om.smpl_adjacency().double()
    x = torch.from_numpy(g.normal(size=(5, 24, 64)))
    p = "gconv_layers.0.gconv1"
    ref = om._graph_conv(sd, p, x, adj)
    torch.testing.assert_close(og.hidden_conv(x, _layer(sd, p), adj), ref, rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(og.hidden_conv(x, _layer(sd, p), adj, residual=x), x + ref, rtol=1e-13, atol=1e-14)
    out = om.modulated_graph_conv(sd, "gconv_output", x, adj)
    torch.testing.assert_close(og.output_conv(x, _layer(sd, "gconv_output", bn=False), adj), out.reshape(5, 144), rtol=1e-13, atol=1e-14)


def test_output_fuse_and_pass_map():
    """ehm_gcn_output_layer's selection: joint j of item b from the conditional pass when visible, else from the item's second-pass slot."""
    g = np.random.Generator(np.random.PCG64(4))
    B = 5
    out = torch.from_numpy(g.normal(size=(B + 2, 24, 6)))
    vis = torch.ones(B, 24, dtype=torch.uint8)
    vis[1, 3] = 0
    vis[4, :7] = 0
    slot = torch.tensor([-1, 0, -1, -1, 1])
    x0 = og.fuse(out, vis, B, 2, slot).view(B, 24, 6)
    want = out[:B].clone()
    want[1, 3] = out[B + 0, 3]
    want[4, :7] = out[B + 1, :7]
    assert torch.equal(x0, want)
    assert torch.equal(og.fuse(out, vis, B, 1), out[:B].reshape(B, 144))
    # an empty map: no second-pass rows at all, every item fully visible
    ones = torch.ones(B, 24, dtype=torch.uint8)
    assert torch.equal(og.fuse(out[:B], ones, B, 2, torch.full((B,), -1)), out[:B].reshape(B, 144))


def test_input_conv_forms_match_the_concatenated_feature():
    """The hoisted input conv (vis-gated image slice, other conditioning, timestep vector, x_t @ Wx) and the rows form equal
    oracle.model._graph_conv on the concatenated per-joint feature it stands for, in both passes and uncond modes."""
    g = np.random.Generator(np.random.PCG64(5))
    B, ci, co, hid = 4, 16, 8, 64
    cin = ci + co + 6 + 1
    sd = _sd(12, cin, hid, 1)
    adj = om.smpl_adjacency().double()
    img = torch.from_numpy(g.normal(size=(B, ci)))
    oth = torch.from_numpy(g.normal(size=(B, co)))
    x = torch.from_numpy(g.normal(size=(B, 144)))
    t = torch.from_numpy(g.normal(size=(1,)))
    vis = torch.from_numpy(g.integers(0, 2, size=(B, 24)).astype(np.uint8))
    W = sd["gconv_input.0.gconv.W"]
    sl = [slice(0, ci), slice(ci, ci + co), slice(ci + co, ci + co + 6), slice(cin - 1, cin)]
    h_img = torch.stack([img @ W[k, sl[0]] for k in range(2)], 1)
    h_oth = torch.stack([oth @ W[k, sl[1]] for k in range(2)], 1)
    Wx = torch.stack([W[k, sl[2]] for k in range(2)])
    tvec = torch.stack([t @ W[k, sl[3]] for k in range(2)])
    layer = _layer(sd, "gconv_input.0")

    def feat(items, p, whole):
        n = len(items)
        f_img = img[items].unsqueeze(1) * vis[items].double().unsqueeze(-1) if p == 0 else torch.zeros(n, 24, ci, dtype=torch.float64)
        f_oth = torch.zeros(n, 24, co, dtype=torch.float64) if (p == 1 and whole) else oth[items].unsqueeze(1).expand(n, 24, co)
        return torch.cat([f_img, f_oth, x[items].view(n, 24, 6), t.expand(n, 24, 1)], -1)

    items = torch.tensor([1, 3])
    for passes, mask_items in ((1, None), (2, None), (2, items), (2, torch.zeros(0, dtype=torch.long))):
        for whole in (False, True):
            got = og.input_conv(h_img, h_oth, vis, x, Wx, tvec, layer, adj, passes, mask_items, whole)
            f = feat(torch.arange(B), 0, whole)
            if passes == 2:
                f = torch.cat([f, feat(torch.arange(B) if mask_items is None else mask_items, 1, whole)], 0)
            ref = om._graph_conv(sd, "gconv_input.0", f, adj)
            torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-13)
            pre = torch.stack([f @ W[0], f @ W[1]], 2).reshape(-1, 2, hid)
            torch.testing.assert_close(og.input_rows(pre, layer, adj), ref, rtol=1e-12, atol=1e-13)


def test_denoiser_matches_modulated_gcn():
    """oracle.gcn.denoiser with the rows form of the input conv = oracle.model.modulated_gcn (two residual blocks)."""
    g = np.random.Generator(np.random.PCG64(6))
    B, cin, hid = 3, 40, 64
    sd = _sd(13, cin, hid, 2)
    adj = om.smpl_adjacency().double()
    f = torch.from_numpy(g.normal(size=(B, 24, cin)))
    ref = om.modulated_gcn(sd, f, adj, p="", num_blocks=2)
    W = sd["gconv_input.0.gconv.W"]
    # the whole feature as the 'image' slice with every joint visible, nothing else: pre_k = f @ W[k] per joint needs a per-joint feature,
    # so go through the rows form and chain the hidden convs / output conv of oracle.gcn by hand
    h = og.input_rows(torch.stack([f @ W[0], f @ W[1]], 2).reshape(-1, 2, hid), _layer(sd, "gconv_input.0"), adj)
    for b in range(2):
        r = h
        h = og.hidden_conv(h, _layer(sd, f"gconv_layers.{b}.gconv1"), adj)
        h = og.hidden_conv(h, _layer(sd, f"gconv_layers.{b}.gconv2"), adj, residual=r)
    torch.testing.assert_close(og.output_conv(h, _layer(sd, "gconv_output", bn=False), adj), ref.reshape(B, 144), rtol=1e-12, atol=1e-13)
    # and the hoisted form through denoiser(): a feature with an image slice only (x = 0, h_oth = tvec = 0)
    ci = 12
    img = torch.from_numpy(g.normal(size=(B, ci)))
    sd2 = _sd(14, ci, hid, 2)
    W2 = sd2["gconv_input.0.gconv.W"]
    layers = [_layer(sd2, "gconv_input.0")] + [_layer(sd2, f"gconv_layers.{b}.gconv{i}") for b in range(2) for i in (1, 2)] + \
        [_layer(sd2, "gconv_output", bn=False)]
    zeros2 = torch.zeros(B, 2, hid, dtype=torch.float64)
    x0, acts = og.denoiser(torch.stack([img @ W2[0], img @ W2[1]], 1), zeros2, torch.ones(B, 24), torch.zeros(B, 144),
                           torch.zeros(2, 6, hid, dtype=torch.float64), torch.zeros(2, hid, dtype=torch.float64), layers, adj)
    ref2 = om.modulated_gcn(sd2, img.unsqueeze(1).expand(B, 24, ci), adj, p="", num_blocks=2)
    torch.testing.assert_close(x0, ref2.reshape(B, 144), rtol=1e-12, atol=1e-13)
    assert len(acts) == 5


def test_reference_goldens(golden_dir):
    """g4_gcn_tiny (ModulatedGCN, one block) and g4_gconv_1024 (one full-width ModulatedGraphConv) of the reference through oracle.gcn."""
    g = np.load(os.path.join(golden_dir, "g4_gcn_tiny.npz"))
    sd = {k[3:]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("w__")}
    adj = torch.from_numpy(g["adj"]).double()
    x = torch.from_numpy(g["x"]).double()
    W = sd["gconv_input.0.gconv.W"]
    h = og.input_rows(torch.stack([x @ W[0], x @ W[1]], 2).reshape(-1, 2, W.shape[2]), _layer(sd, "gconv_input.0"), adj)
    r = h
    h = og.hidden_conv(h, _layer(sd, "gconv_layers.0.gconv1"), adj)
    h = og.hidden_conv(h, _layer(sd, "gconv_layers.0.gconv2"), adj, residual=r)
    y = og.output_conv(h, _layer(sd, "gconv_output", bn=False), adj)
    np.testing.assert_allclose(y.numpy(), g["y"].reshape(-1, 144), atol=1e-5)
    g = np.load(os.path.join(golden_dir, "g4_gconv_1024.npz"))
    man = [("gconv.W", (2, 1024, 1024)), ("gconv.M", (24, 1024)), ("gconv.adj2", (24, 24)), ("gconv.bias", (1024,))]
    sd = {k: torch.from_numpy(v) for k, v in syn.make_state_dict(seed=int(g["weight_seed"]), manifest=man).items()}
    out = og.hidden_conv(torch.from_numpy(g["x"]).double(), _layer(sd, "gconv", bn=False), om.smpl_adjacency())
    np.testing.assert_allclose(out.numpy(), g["y"], atol=2e-5)
