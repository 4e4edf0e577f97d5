"""Torch restatement, on the CPU, of the eval-mode ResNet-50 trunk (models/resnet.py:97-150 as egohmr_amd/encoders.py ResNet50Features runs it) and of its
backward, for tests/test_trunk_autograd_cpu.py and tests/test_gpu_trunk_autograd.py; not collected by pytest.

Two forms: (a) the whole trunk on F.conv2d / F.batch_norm(training=False) / ReLU / max-pool / mean with the UNFOLDED parameters as leaves, under torch
autograd, in the dtype of its inputs (float64: the reference; float32: the seed search's stand-in for a float32 forward); (b) per-conv VJPs written out
by hand as functions of (folded weight, input, gate source, cotangent), chained over the whole trunk with gates and pool indices GIVEN - so that a test can
hand them the device's own - and the fold / unfold formulas.  Tensors are NCHW here."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
LAYERS = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))          # width, blocks, stride of the first block


def unit_names():
    """(conv name, bn name, stride, pad) of every conv of the trunk in forward order: stem, then conv1, conv2, conv3, downsample (None if absent) per block."""
    out = [("conv1", "bn1", 2, 3)]
    for i, (width, n, stride) in enumerate(LAYERS, 1):
        for b in range(n):
            p = f"layer{i}.{b}."
            s = stride if b == 0 else 1
            out += [(p + "conv1", p + "bn1", 1, 0), (p + "conv2", p + "bn2", s, 1), (p + "conv3", p + "bn3", 1, 0),
                    (p + "downsample.0", p + "downsample.1", s, 0) if b == 0 else None]
    return out


def param_names():
    """The trunk's parameters in the order of ResNet50Features.parameters()."""
    out = []
    for u in unit_names():
        if u is None:
            continue
        out += [u[0] + ".weight", u[1] + ".weight", u[1] + ".bias"]
    # module order: conv1, bn1, conv2, bn2, conv3, bn3, downsample - the same as the unit order
    return out


def make_state(seed):
    """Seeded trained-like trunk weights (egohmr_amd.synthetic's rules) as float64 CPU tensors; integer buffers as they are."""
    from egohmr_amd import synthetic as syn
    sd = syn.make_state_dict(seed, manifest=syn._resnet50_manifest(""))
    return {k: (torch.from_numpy(np.asarray(v)).double() if np.asarray(v).dtype.kind == "f" else torch.as_tensor(np.asarray(v)).clone()) for k, v in sd.items()}


def make_image(B, H, W, seed):
    return torch.from_numpy(np.random.default_rng(7000 + seed).normal(size=(B, 3, H, W))).double()


def make_cotangent(B, seed):
    return torch.from_numpy(np.random.default_rng(8000 + seed).normal(size=(B, 2048))).double()


def _cbn(sd, x, conv, bn, stride, pad):
    y = F.conv2d(x, sd[conv + ".weight"], None, stride, pad)
    return F.batch_norm(y, sd[bn + ".running_mean"].to(x.dtype), sd[bn + ".running_var"].to(x.dtype), sd[bn + ".weight"], sd[bn + ".bias"], False, 0.0, EPS)


def trunk(sd, img, acts=None):
    """The eval-mode trunk -> [B,2048], differentiable w.r.t. the tensors of sd; dtype of img.  acts: a list that receives the stem's pre-pool activation
    (before the ReLU), its pooled output and then every conv's (post-ReLU) output, detached, in forward order."""
    keep = (lambda t: None) if acts is None else (lambda t: acts.append(t.detach()))
    z = _cbn(sd, img, "conv1", "bn1", 2, 3)
    keep(z)
    x = F.max_pool2d(F.relu(z), 3, 2, 1)
    keep(x)
    for i, (width, n, stride) in enumerate(LAYERS, 1):
        for b in range(n):
            p = f"layer{i}.{b}."
            s = stride if b == 0 else 1
            y = F.relu(_cbn(sd, x, p + "conv1", p + "bn1", 1, 0))
            keep(y)
            y = F.relu(_cbn(sd, y, p + "conv2", p + "bn2", s, 1))
            keep(y)
            y = _cbn(sd, y, p + "conv3", p + "bn3", 1, 0)
            x = F.relu(y + (_cbn(sd, x, p + "downsample.0", p + "downsample.1", s, 0) if b == 0 else x))
            keep(x)
    return x.mean(dim=(2, 3))


def autograd_grads(sd, img, gout, dtype=torch.float64):
    """{parameter name: gradient} of <trunk(sd, img), gout> by torch autograd in `dtype` (returned as float64)."""
    names = param_names()
    leaves = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    for n in names:
        leaves[n] = leaves[n].clone().requires_grad_()
    out = trunk(leaves, img.to(dtype))
    grads = torch.autograd.grad(out, [leaves[n] for n in names], gout.to(dtype))
    return {n: g.double() for n, g in zip(names, grads)}, out.detach().double()


def float32_error(seed, B=2, H=64, W=64):
    """max over the parameter tensors of max|g32 - g64| / max|g64|: how far a float32 forward + backward (its ReLU-gate and pool flips included) moves
    the gradients at this seed."""
    sd, img, gout = make_state(seed), make_image(B, H, W, seed), make_cotangent(B, seed)
    g64, _ = autograd_grads(sd, img, gout, torch.float64)
    g32, _ = autograd_grads(sd, img, gout, torch.float32)
    return max(float((g32[n] - g64[n]).abs().max() / g64[n].abs().max()) for n in g64)


# ------------------------------------------------------------------------------------------------------------------------ fold / unfold
def fold(w, gamma, beta, mean, var, eps=EPS):
    s = gamma / torch.sqrt(var + eps)
    return w * s.view(-1, 1, 1, 1), beta - mean * s


def fold_state(sd):
    """{unit index: (w', b')} in float64."""
    out = {}
    for i, u in enumerate(unit_names()):
        if u is not None:
            out[i] = fold(sd[u[0] + ".weight"], sd[u[1] + ".weight"], sd[u[1] + ".bias"], sd[u[1] + ".running_mean"], sd[u[1] + ".running_var"])
    return out


def unfold(w, gamma, mean, var, gw, gb, eps=EPS):
    """(wbar, gammabar, betabar) from the folded pair's gradients."""
    inv = 1.0 / torch.sqrt(var + eps)
    return gw * (gamma * inv).view(-1, 1, 1, 1), ((gw * w).sum(dim=(1, 2, 3)) - gb * mean) * inv, gb


# ------------------------------------------------------------------------------------------------------------------------ per-conv VJPs by hand
def conv_vjp(wf, x, gate_src, g, stride, pad, need_x=True):
    """y = relu(conv(x, wf) + b (+ res)), g = dL/dy, gate_src: a tensor whose sign is y's ->  (G, wbar', bbar', xbar).  Written with unfold / einsum and
    conv_transpose, not autograd; the residual's gradient is G itself."""
    G = torch.where(gate_src > 0, g, torch.zeros_like(g))
    Co, Ci, K, _ = wf.shape
    N, _, H, W = x.shape
    cols = F.unfold(x, K, padding=pad, stride=stride)                                  # [N, Ci*K*K, L]
    gw = torch.einsum("ncl,nkl->ck", G.flatten(2), cols).view(Co, Ci, K, K)
    gb = G.sum(dim=(0, 2, 3))
    gx = None
    if need_x:
        Ho, Wo = G.shape[2:]
        oph, opw = H - ((Ho - 1) * stride - 2 * pad + K), W - ((Wo - 1) * stride - 2 * pad + K)
        gx = F.conv_transpose2d(G, wf, None, stride, pad, output_padding=(oph, opw))
    return G, gw, gb, gx


def pool_route(z, gp):
    """z [N,C,Hc,Wc] pre-pool values, gp [N,C,Hq,Wq] cotangent of max_pool2d(z, 3, 2, 1) -> cotangent of z: each window's goes to its arg-max, the lowest
    row-major index among equals, NaN = maximum."""
    N, Cn, Hc, Wc = z.shape
    zp = F.pad(z, (1, 1, 1, 1), value=float("-inf"))
    win = zp.unfold(2, 3, 2).unfold(3, 3, 2).reshape(N, Cn, Hc // 2, Wc // 2, 9)
    key = torch.where(torch.isnan(win), torch.full_like(win, float("inf")), win)
    best = key.max(dim=-1, keepdim=True).values
    first = ((key == best).to(torch.int64) * torch.arange(9, 0, -1)).argmax(dim=-1)    # the first maximiser in row-major order (weights 9..1: unique)
    out = torch.zeros(N, Cn, Hc + 2, Wc + 2, dtype=z.dtype)
    pr = torch.arange(Hc // 2).view(1, 1, -1, 1) * 2 + first // 3
    pc = torch.arange(Wc // 2).view(1, 1, 1, -1) * 2 + first % 3
    n = torch.arange(N).view(-1, 1, 1, 1).expand_as(first)
    c = torch.arange(Cn).view(1, -1, 1, 1).expand_as(first)
    out.index_put_((n, c, pr, pc), gp, accumulate=True)
    return out[:, :, 1:-1, 1:-1]


def stem_vjp(img, gpool_gated, z):
    """Stem: gpool_gated = the pooled output's cotangent already gated by [pooled > 0]; z = the pre-pool activation whose arg-max routes it.
    -> (wbar' [64,3,7,7], bbar' [64], gz)."""
    gz = pool_route(z, gpool_gated)
    cols = F.unfold(img, 7, padding=3, stride=2)
    gw = torch.einsum("ncl,nkl->ck", gz.flatten(2), cols).view(64, 3, 7, 7)
    return gw, gz.sum(dim=(0, 2, 3)), gz


def trunk_vjp_chain(folded, img, acts, z_stem, gout):
    """The whole backward by the hand-written VJPs with GIVEN gates: folded = fold_state(sd); acts = the 1 + 3 * 16 saved activations (NCHW float64:
    the stem's pooled output, then every conv's output) whose signs gate; z_stem the stem's pre-pool activation.  -> {unit index: (w'bar, b'bar)}."""
    U = unit_names()
    res = {}
    nb = (len(U) - 1) // 4
    y = acts[3 * nb]
    g = (gout / (y.shape[2] * y.shape[3])).view(*gout.shape, 1, 1).expand_as(y)
    for b in range(nb - 1, -1, -1):
        i1, i2, i3, id_ = 1 + 4 * b, 2 + 4 * b, 3 + 4 * b, 4 + 4 * b
        xin, a1, a2, y = acts[3 * b], acts[3 * b + 1], acts[3 * b + 2], acts[3 * b + 3]
        G3, gw3, gb3, ga2 = conv_vjp(folded[i3][0], a2, y, g, 1, 0)
        res[i3] = (gw3, gb3)
        if U[id_] is not None:
            _, gwd, gbd, short = conv_vjp(folded[id_][0], xin, y, g, U[id_][2], 0)
            res[id_] = (gwd, gbd)
        else:
            short = G3
        _, gw2, gb2, ga1 = conv_vjp(folded[i2][0], a1, a2, ga2, U[i2][2], 1)
        res[i2] = (gw2, gb2)
        _, gw1, gb1, gx = conv_vjp(folded[i1][0], xin, a1, ga1, 1, 0)
        res[i1] = (gw1, gb1)
        g = gx + short
    G0 = torch.where(acts[0] > 0, g, torch.zeros_like(g))
    gw0, gb0, _ = stem_vjp(img, G0, z_stem)
    res[0] = (gw0, gb0)
    return res


def unfold_all(sd, res):
    """{parameter name: gradient} from trunk_vjp_chain's result."""
    out = {}
    for i, u in enumerate(unit_names()):
        if u is None or i not in res:
            continue
        gw, gg, gb = unfold(sd[u[0] + ".weight"], sd[u[1] + ".weight"], sd[u[1] + ".running_mean"], sd[u[1] + ".running_var"], *res[i])
        out[u[0] + ".weight"], out[u[1] + ".weight"], out[u[1] + ".bias"] = gw, gg, gb
    return out


def x2_decode(buf, pixels, Cn):
    """An X2 activation buffer read back from the device (float32 tensor [rows, C] whose bytes are, per row and 32 channels, 32 f16 hi | 32 f16 lo)
    -> float64 [pixels, C] = hi + lo."""
    h = buf.cpu().contiguous().view(torch.float16).view(buf.shape[0], Cn // 32, 2, 32)
    return (h[:, :, 0, :].double() + h[:, :, 1, :].double()).reshape(buf.shape[0], Cn)[:pixels]


def load_module(sd, dev=None):
    """A ResNet50Features with sd's weights (eval mode), on `dev` when given."""
    from egohmr_amd.encoders import ResNet50Features
    m = ResNet50Features()
    m.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()})
    m.eval()
    return m.to(dev) if dev is not None else m
