"""Float64 torch restatement of the non-local block of ModulatedGCN (modulated_gcn.py:93-110; nets/non_local_embedded_gaussian.py:62-85) on the joint
axis, and of ModulatedGCN with it, with BatchNorm in eval mode (oracle.model.non_local_block, tests/gcn_train_ref.eval_forward's convs) and in TRAINING
mode (torch.nn.functional.batch_norm(training=True) over all 24 B rows; tests/gcn_train_ref.train_conv).  Autograd goes through everything; the
running statistics are updated in place as torch updates them.  tests/test_nonlocal_grad_cpu.py pins it to the reference's own module
(tests/golden/g22_nonlocal_train.npz, written by tests/make_nonlocal_golden.py); the GPU tests compare the HIP routes against it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import gcn_train_ref as R
from oracle import gcn as og
from oracle import model as om

NL = "non_local."
BLOCK_PARAMS = ("theta.weight", "theta.bias", "phi.weight", "phi.bias", "g.weight", "g.bias", "W.0.weight", "W.0.bias", "W.1.weight", "W.1.bias")
BN_EPS = 1e-5               # nn.BatchNorm2d's default, which NONLocalBlock2D keeps


def block(sd, x, train, p=NL, momentum=0.1, update_running=True):
    """The block on x [B, 24, hid] float64.  train: batch statistics over the 24 B rows (sd[p + 'W.1.running_*'] updated in place when update_running)."""
    if not train:
        return om.non_local_block(sd, p, x)
    lin = lambda n, v: F.linear(v, sd[p + n + ".weight"].flatten(1), sd[p + n + ".bias"])
    g_x, th, ph = lin("g", x), lin("theta", x), lin("phi", x)
    y = torch.matmul(F.softmax(torch.matmul(th, ph.transpose(1, 2)), dim=-1), g_x)
    u = lin("W.0", y)
    C = u.shape[-1]
    rm, rv = (sd[p + "W.1.running_mean"], sd[p + "W.1.running_var"]) if update_running else (None, None)
    v = F.batch_norm(u.reshape(-1, C), rm, rv, sd[p + "W.1.weight"], sd[p + "W.1.bias"], training=True, momentum=momentum, eps=BN_EPS)
    return v.view_as(u) + x


def modulated_gcn(sd, x, adj, blocks=1, train=False, momentum=0.1, update_running=True):
    """ModulatedGCN(nonlocal_layer=True).forward on a state dict of float64 tensors -> (out [B, 24, 6], the BatchNorm outputs in front of every ReLU: what the
    gate margin looks at)."""
    vs = []

    def conv(pfx, t, res=None):
        if train:
            run = (sd[pfx + ".bn.running_mean"], sd[pfx + ".bn.running_var"]) if update_running else None
            out, _, v, _ = R.train_conv(t, R.layer_of(sd, pfx), adj, res, run, momentum)
        else:
            ly = R.layer_of(sd, pfx)
            z = og.mix(t @ ly["W"][0], t @ ly["W"][1], ly, adj)
            v = (z - sd[pfx + ".bn.running_mean"]) / torch.sqrt(sd[pfx + ".bn.running_var"] + og.BN_EPS) * ly["bn_weight"] + ly["bn_bias"]
            out = torch.relu(v) if res is None else res + torch.relu(v)
        vs.append(v)
        return out

    cur = conv("gconv_input.0", x)
    for b in range(blocks):
        cur = conv(f"gconv_layers.{b}.gconv2", conv(f"gconv_layers.{b}.gconv1", cur), cur)
    cur = block(sd, cur, train, momentum=momentum, update_running=update_running)
    ly = R.layer_of(sd, "gconv_output")
    return og.mix(cur @ ly["W"][0], cur @ ly["W"][1], ly, adj), vs


def block_state(seed, hid, logit_std=3.0, x_rms=1.0, p=NL):
    """Synthetic block weights as float64 CPU tensors holding float32 values: theta / phi sized so that the logits of inputs of RMS x_rms have a standard
    deviation of about logit_std (the regime egohmr_amd.synthetic gives the block), a W.1 BatchNorm with gammas of both signs and non-trivial running
    statistics (the reference initialises the affine to zero: an identity block with zero gradients upstream)."""
    g = np.random.Generator(np.random.PCG64(seed))
    ci = hid // 2
    sd = {}
    a = math.sqrt(logit_std / math.sqrt(ci)) / (x_rms * math.sqrt(hid))        # theta, phi entries of std a x_rms sqrt(hid): logits of std a^2 x_rms^2 hid sqrt(ci)
    for n, s in (("theta", a), ("phi", a), ("g", 1.0 / math.sqrt(hid))):
        sd[p + n + ".weight"] = g.normal(scale=s, size=(ci, hid, 1, 1))
        sd[p + n + ".bias"] = g.normal(scale=0.05, size=ci)
    sd[p + "W.0.weight"] = g.normal(scale=1.0 / math.sqrt(ci), size=(hid, ci, 1, 1))
    sd[p + "W.0.bias"] = g.normal(scale=0.05, size=hid)
    sd[p + "W.1.weight"] = g.uniform(0.5, 1.5, size=hid) * g.choice([-1.0, 1.0], size=hid)
    sd[p + "W.1.bias"] = g.normal(scale=0.05, size=hid)
    sd[p + "W.1.running_mean"] = g.normal(scale=0.1, size=hid)
    sd[p + "W.1.running_var"] = g.uniform(0.6, 1.4, size=hid)
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float32)).double() for k, v in sd.items()}


def module_state(seed, in_dim=70, hid=64, blocks=1, bodies=3):
    """gcn_train_ref.module_state + block_state: a ModulatedGCN(nonlocal_layer=True) state dict and an input x [bodies, 24, in_dim]."""
    sd, x = R.module_state(seed, in_dim=in_dim, hid=hid, blocks=blocks, bodies=bodies)
    sd.update(block_state(seed + 1000, hid))
    return sd, x


def grad_names(blocks=1):
    """The state-dict names of ModulatedGCN.grad_parameters() with nonlocal_grad, in its order."""
    out = []
    for pfx in R.conv_prefixes(blocks):
        out += [f"{pfx}.gconv.{k}" for k in ("W", "M", "adj2", "bias")] + [pfx + ".bn.weight", pfx + ".bn.bias"]
    out += [f"gconv_output.{k}" for k in ("W", "M", "adj2", "bias")]
    return out + [NL + k for k in BLOCK_PARAMS]


def run(sd, x, cot, adj, blocks=1, train=False):
    """One forward + backward of the restatement on COPIES of sd's tensors (float64): dict(out, gx, grads {name: gradient}, vs, sd = the copies, with the
    running statistics after the call)."""
    sd = {k: v.clone() for k, v in sd.items()}
    names = grad_names(blocks)
    for n in names:
        sd[n].requires_grad_(True)
    x = x.clone().requires_grad_(True)
    out, vs = modulated_gcn(sd, x, adj, blocks, train)
    gs = torch.autograd.grad(out, [x] + [sd[n] for n in names], cot)
    return dict(out=out.detach(), gx=gs[0], grads=dict(zip(names, gs[1:])), vs=[v.detach() for v in vs], sd={k: v.detach() for k, v in sd.items()})


def gate_margin(res):
    """min over the convs of min|v| / max|v| of a run()'s BatchNorm outputs in front of the ReLUs."""
    return min(float(v.abs().min() / v.abs().max()) for v in res["vs"])
