"""Torch restatement, on the CPU, of the ResNet-50 trunk with BatchNorm2d in TRAINING mode (models/resnet.py:97-150 under backbone.train(),
egohmr.py:455, as ResNet50Features.train_batchnorm runs it) for tests/test_trunk_train_cpu.py and tests/test_gpu_trunk_train.py; not collected by pytest.

Two forms beside tests/trunk_grad_ref.py's: (a) the whole trunk on F.conv2d / F.batch_norm(training=True) under torch autograd in the dtype of its inputs;
(b) ONE (conv, BatchNorm2d) unit's VJP written out by hand as a function of (w, gamma, x, z, gate source, g) - z the conv's raw output, GIVEN, so that a
test can hand it the device's own tensors and every comparison is a single well-conditioned step.  Tensors are NCHW here."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import trunk_grad_ref as R

EPS, MOMENTUM = R.EPS, 0.1


def batch_stats(z):
    """z [N,C,H,W] -> (mean, biased var, invstd) per channel over N, H, W."""
    mean = z.mean(dim=(0, 2, 3))
    var = ((z - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    return mean, var, 1.0 / torch.sqrt(var + EPS)


def row_stats(z):
    """z [P,C] float64 rows -> (mean, biased var, invstd)."""
    mean = z.mean(dim=0)
    var = ((z - mean) ** 2).mean(dim=0)
    return mean, var, 1.0 / torch.sqrt(var + EPS)


def running_update(rm, rv, mean, var, R_, momentum=MOMENTUM):
    """nn.BatchNorm2d's update of (running_mean, running_var) from a batch's (mean, biased var) over R_ rows."""
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * var * R_ / (R_ - 1)


def _cbn_train(sd, x, conv, bn, stride, pad, stats=None):
    z = F.conv2d(x, sd[conv + ".weight"], None, stride, pad)
    if stats is not None:
        stats.append(batch_stats(z.detach()) + (z.shape[0] * z.shape[2] * z.shape[3],))
    return F.batch_norm(z, None, None, sd[bn + ".weight"], sd[bn + ".bias"], True, 0.0, EPS)


def trunk(sd, img, stats=None):
    """The train-mode trunk -> [B,2048], differentiable w.r.t. the tensors of sd; dtype of img.  stats: a list that receives (mean, var, invstd, rows) per
    BatchNorm2d in the order of R.unit_names() without its Nones."""
    c = lambda x, conv, bn, s, p: _cbn_train(sd, x, conv, bn, s, p, stats)
    x = F.max_pool2d(F.relu(c(img, "conv1", "bn1", 2, 3)), 3, 2, 1)
    for i, (width, n, stride) in enumerate(R.LAYERS, 1):
        for b in range(n):
            p = f"layer{i}.{b}."
            s = stride if b == 0 else 1
            y = F.relu(c(x, p + "conv1", p + "bn1", 1, 0))
            y = F.relu(c(y, p + "conv2", p + "bn2", s, 1))
            y = c(y, p + "conv3", p + "bn3", 1, 0)
            x = F.relu(y + (c(x, p + "downsample.0", p + "downsample.1", s, 0) if b == 0 else x))
    return x.mean(dim=(2, 3))


def autograd_grads(sd, img, gout, dtype=torch.float64):
    """({parameter name: gradient}, output) of <trunk(sd, img), gout> by torch autograd in `dtype` (returned as float64)."""
    names = R.param_names()
    leaves = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    for n in names:
        leaves[n] = leaves[n].clone().requires_grad_()
    out = trunk(leaves, img.to(dtype))
    grads = torch.autograd.grad(out, [leaves[n] for n in names], gout.to(dtype))
    return {n: g.double() for n, g in zip(names, grads)}, out.detach().double()


# ------------------------------------------------------------------------------------------------------------------------ one unit by hand
def bn_vjp(gamma, z, G):
    """y = gamma (z - mu) invstd + beta with mu, var the batch's own; G = dL/dy -> (zbar, gammabar, betabar).  z, G [N,C,H,W]."""
    mean, _, invstd = batch_stats(z)
    Rr = z.shape[0] * z.shape[2] * z.shape[3]
    v = lambda t: t.view(1, -1, 1, 1)
    xhat = (z - v(mean)) * v(invstd)
    gbeta = G.sum(dim=(0, 2, 3))
    ggamma = (G * xhat).sum(dim=(0, 2, 3))
    zbar = v(gamma * invstd) * (G - v(gbeta) / Rr - xhat * v(ggamma) / Rr)
    return zbar, ggamma, gbeta


def unit_vjp(w, gamma, x, z, gate_src, g, stride, pad, need_x=True):
    """One unit y = relu(BN_train(z) (+ res)), z = conv(x, w), g = dL/dy, gate_src: a tensor whose sign is y's
    -> dict(G, zbar, wbar, gammabar, betabar, xbar).  Written with unfold / einsum / conv_transpose, not autograd."""
    G = torch.where(gate_src > 0, g, torch.zeros_like(g))
    zbar, ggamma, gbeta = bn_vjp(gamma, z, G)
    _, gw, _, gx = R.conv_vjp(w, x, torch.ones_like(zbar), zbar, stride, pad, need_x=need_x)
    return dict(G=G, zbar=zbar, wbar=gw, gammabar=ggamma, betabar=gbeta, xbar=gx)


def stem_unit_vjp(w, gamma, img, z, z_route, gpool_gated):
    """The stem: z = conv(img, w) raw; z_route: the pre-pool activation BN_train(z) whose arg-max routes the pooled cotangent (already gated by
    [pooled > 0]) -> dict(gz, zbar, wbar, gammabar, betabar)."""
    gz = R.pool_route(z_route, gpool_gated)
    zbar, ggamma, gbeta = bn_vjp(gamma, z, gz)
    cols = F.unfold(img, 7, padding=3, stride=2)
    gw = torch.einsum("ncl,nkl->ck", zbar.flatten(2), cols).view(64, 3, 7, 7)
    return dict(gz=gz, zbar=zbar, wbar=gw, gammabar=ggamma, betabar=gbeta)


def load_module(sd, dev=None, train_batchnorm=True):
    """R.load_module in .train() with the switch set."""
    m = R.load_module(sd, dev)
    m.train()
    m.train_batchnorm = train_batchnorm
    return m
