"""Float64 torch restatement of the Modulated-GCN denoiser with BatchNorm1d in TRAINING mode (modulated_gcn.py:21-28, :38-42, :99-116 under
self.training): oracle.gcn.mix for the pre-activation z, torch.nn.functional.batch_norm(training=True) over all 24 B rows, ReLU, the residual.  Autograd
goes through the batch statistics; the running statistics are updated in place as torch updates them.  Shared by tests/test_gcn_train_cpu.py and
tests/test_gpu_gcn_train.py."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import gcn as og

PARAMS = ("W", "M", "adj2", "bias", "bn_weight", "bn_bias")


def train_conv(x, layer, adj, residual=None, running=None, momentum=0.1, eps=og.BN_EPS):
    """x [b, 24, K] float64, layer: dict of float64 W, M, adj2, bias, bn_weight, bn_bias -> (out, y = the activation before the residual add, the BatchNorm
    output v in front of the ReLU, z).  running: (running_mean, running_var) float64, updated in place, or None."""
    W = layer["W"]
    z = og.mix(x @ W[0], x @ W[1], layer, adj)
    N = z.shape[-1]
    rm, rv = running if running is not None else (None, None)
    v = F.batch_norm(z.reshape(-1, N), rm, rv, layer["bn_weight"], layer["bn_bias"], training=True, momentum=momentum, eps=eps).view_as(z)
    y = torch.relu(v)
    return (y if residual is None else residual + y), y, v, z


def layer_of(sd, p):
    """The layer dict of the conv with prefix p ('gconv_input.0', 'gconv_layers.0.gconv1', 'gconv_output') of a ModulatedGCN state dict."""
    q = p + ".gconv" if (p + ".bn.weight") in sd else p
    ly = {k: sd[f"{q}.{k}"] for k in ("W", "M", "adj2", "bias")}
    if q != p:
        ly.update(bn_weight=sd[p + ".bn.weight"], bn_bias=sd[p + ".bn.bias"])
    return ly


def conv_prefixes(blocks):
    out = ["gconv_input.0"]
    for b in range(blocks):
        out += [f"gconv_layers.{b}.gconv1", f"gconv_layers.{b}.gconv2"]
    return out


def modulated_gcn_train(sd, x, adj, blocks=1, momentum=0.1, eps=og.BN_EPS, update_running=True):
    """ModulatedGCN.forward in training mode on a state dict of float64 tensors (sd[... running_mean / running_var] are updated in place when
    update_running) -> (out [b, 24, 6], the BatchNorm outputs in front of every ReLU and the output conv's result: what the gate margin looks at)."""
    vs = []

    def conv(p, t, res=None):
        run = (sd[p + ".bn.running_mean"], sd[p + ".bn.running_var"]) if update_running else None
        out, _, v, _ = train_conv(t, layer_of(sd, p), adj, res, run, momentum, eps)
        vs.append(v)
        return out

    cur = conv("gconv_input.0", x)
    for b in range(blocks):
        cur = conv(f"gconv_layers.{b}.gconv2", conv(f"gconv_layers.{b}.gconv1", cur), cur)
    ly = layer_of(sd, "gconv_output")
    out = og.mix(cur @ ly["W"][0], cur @ ly["W"][1], ly, adj)
    vs.append(out)
    return out, vs


def eval_forward(sd, x, adj, blocks=1, eps=og.BN_EPS):
    """The same network with BatchNorm in eval mode on sd's running statistics (float64)."""
    def conv(p, t, res=None):
        ly = dict(layer_of(sd, p), bn_mean=sd[p + ".bn.running_mean"], bn_var=sd[p + ".bn.running_var"])
        z = og.mix(t @ ly["W"][0], t @ ly["W"][1], ly, adj)
        y = torch.relu((z - ly["bn_mean"]) / torch.sqrt(ly["bn_var"] + eps) * ly["bn_weight"] + ly["bn_bias"])
        return y if res is None else res + y

    cur = conv("gconv_input.0", x)
    for b in range(blocks):
        cur = conv(f"gconv_layers.{b}.gconv2", conv(f"gconv_layers.{b}.gconv1", cur), cur)
    ly = layer_of(sd, "gconv_output")
    return og.mix(cur @ ly["W"][0], cur @ ly["W"][1], ly, adj)


def module_state(seed, in_dim=70, hid=64, blocks=1, bodies=2):
    """A ModulatedGCN state dict (synthetic weights, gammas of both signs) and an input x [bodies, 24, in_dim]: float64 CPU tensors holding float32 values."""
    g = np.random.Generator(np.random.PCG64(seed))
    sd = {}

    def conv(p, K, N, bn):
        q = p + ".gconv" if bn else p
        sd[q + ".W"] = g.normal(scale=0.55 / math.sqrt(K), size=(2, K, N))
        sd[q + ".M"] = 1 + g.normal(scale=0.15, size=(24, N))
        sd[q + ".adj2"] = g.normal(scale=0.02, size=(24, 24))
        sd[q + ".bias"] = g.normal(scale=0.05, size=N)
        if bn:
            sd[p + ".bn.weight"] = g.uniform(0.8, 1.2, size=N) * g.choice([-1.0, 1.0], size=N)
            sd[p + ".bn.bias"] = g.normal(scale=0.05, size=N)
            sd[p + ".bn.running_mean"] = g.normal(scale=0.1, size=N)
            sd[p + ".bn.running_var"] = g.uniform(0.6, 1.4, size=N)

    for p in conv_prefixes(blocks):
        conv(p, in_dim if p == "gconv_input.0" else hid, hid, True)
    conv("gconv_output", hid, 6, False)
    x = g.normal(scale=0.7, size=(bodies, 24, in_dim))
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).double()
    return {k: f(v) for k, v in sd.items()}, f(x)


def gate_margin(seed, **kw):
    """min over the convs of min|v| / max|v| of the float64 train-mode forward on the CPU: what the seed search of the end-to-end test maximises."""
    from oracle import model as om
    sd, x = module_state(seed, **kw)
    _, vs = modulated_gcn_train(sd, x, om.smpl_adjacency(torch.float64), blocks=kw.get("blocks", 1), update_running=False)
    return min(float(v.abs().min() / v.abs().max()) for v in vs)
