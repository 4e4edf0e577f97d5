"""Backward of the ResNet-50 trunk in eval mode on libegohmr_hip (csrc/conv_bwd.hip + the split-f16 conv engine), and the ``torch.autograd.Function``
that ResNet50Features.__call__ runs behind with ``grad_params`` set (encoders.py).

The forward is the X2 route of encoders.FoldedTrunk with every conv's output kept: a conv's saved output is its ReLU gate (sign only) and the next conv's
input.  Per conv with folded weight w', folded bias b', input x, output y = relu(conv(x, w') + b' (+ res)) and g = dL/dy:

    G = s g (.) [y > 0]                         ehm_conv_bwd_gate      (s: a power of two on the device that brings max|g| to about 2^10 - pow2_scale;
                                                                        dense for the weight gradient, zero-dilated for a stride-2 conv's data gradient)
    b'bar = sum_p G,  w'bar = sum_p G x[tap(p)]  ehm_conv_bwd_wgrad     (exact-f32 MFMA over the pixels, taps gathered from the saved X2 activation)
    xbar = conv_transpose(G, w')                ehm_conv_nhwc_split    (w' with its taps flipped and Co <-> Ci transposed, pad = K - 1 - pad; the
                                                                        `residual` input carries the shortcut's gradient into conv1's data gradient)
    stem: w'bar, b'bar                          ehm_resnet_stem_backward (pre-pool activation recomputed, pooled cotangent routed by gather)

The powers of two accumulate along the chain (`cum`: the factor a cotangent tensor carries) and are divided out of the small results - exact.
A fused projection block (y = relu(conv3(a) + downsample(x) + b3 + bd)) sends one G to both convs and the same column sum to both folded biases.
The BatchNorm fold is undone in float64 by `unfold`.  running_mean / running_var / num_batches_tracked are never written.  The backward reads the
parameters again (unfold), so one changed between forward and backward (TensorKey: storage or version counter) is refused, not silently mixed.

One function walks the blocks from the top for both routes (`_walk`): it owns the pruning, the three data gradients per block, the shortcut riding in as
conv1's `residual`, the tensor lifetimes and the powers of two.  What a route does per unit is its step: `_eval_step` is the list above; `_train_step`
(ResNet50Features.train_batchnorm: BatchNorm2d on batch statistics, csrc/bn2d_train.hip) runs a BatchNorm backward per unit on the raw weight, no fold to undo.
`fold`, `units` and `stem_operands` are also what encoders.FoldedTrunk builds its forward from.
"""
from __future__ import annotations

import ctypes as C
from functools import reduce
from operator import mul
from types import SimpleNamespace

import torch

from . import _lib
from .split_gemm import pack_weight, pow2_scale


def fold(conv, bn, stats=None):
    """(w', b') of ResNet50Features.folded() in float64: w' = w g / sqrt(v + eps), b' = beta - mean g / sqrt(v + eps).  stats: (mean, biased variance)
    that stand in for the running ones - the train-mode route's float32 batch statistics."""
    mean, var = (bn.running_mean, bn.running_var) if stats is None else stats
    scale = bn.weight.double() / torch.sqrt(var.double() + bn.eps)
    return conv.weight.double() * scale.view(-1, 1, 1, 1), bn.bias.double() - mean.double() * scale


def unfold(conv, bn, gw, gb):
    """The gradients of (conv.weight, bn.weight, bn.bias) from those of the folded (w' [Co,Ci,KH,KW], b' [Co]); float64 inside, None in -> None out
    where it is needed.  With s = gamma / sqrt(v + eps):  wbar = w'bar s,  gammabar = (sum w'bar w - b'bar mean) / sqrt(v + eps),  betabar = b'bar."""
    inv = 1.0 / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    g_w = g_gamma = g_beta = None
    if gw is not None:
        gw = gw.double()
        g_w = gw * (bn.weight.detach().double() * inv).view(-1, 1, 1, 1)
    if gb is not None:
        g_beta = gb.double()
    if gw is not None and gb is not None:
        g_gamma = ((gw * conv.weight.detach().double()).sum(dim=(1, 2, 3)) - g_beta * bn.running_mean.detach().double()) * inv
    return g_w, g_gamma, g_beta


def units(m):
    """The trunk's (conv, bn) pairs in forward order: the stem, then conv1, conv2, conv3, downsample (or None) of every bottleneck."""
    out = [(m.conv1, m.bn1)]
    for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
        for blk in layer:
            out += [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3),
                    (blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else None]
    return out


def stem_operands(w, b):
    """The stem kernels' operand layout: weight [64,3,7,7] -> [147][64], k = (ci*7 + kh)*7 + kw; the bias contiguous."""
    return w.reshape(64, 147).t().contiguous(), b.contiguous()


def _workspace(query, *dims, dtype=torch.float32, device=None):
    """(scratch of the size `query(*dims, &bytes)` answers, that size in bytes)"""
    nb = C.c_int64(0)
    query(*dims, C.byref(nb))
    return torch.empty(nb.value // dtype.itemsize, dtype=dtype, device=device), nb.value


def dgrad_weight(wf):
    """Folded weight [Co,Ci,KH,KW] float32 -> the packed operand of its data gradient: taps flipped, Co <-> Ci transposed, [Ci][KH*KW*Co] tap-major."""
    Co, Ci, KH, KW = wf.shape
    return pack_weight(wf.flip(2, 3).permute(1, 2, 3, 0).reshape(Ci, KH * KW * Co).contiguous())


def gate(g, y_x2, shape, Cn, scale, out_hw=None, per_image=False):
    """ehm_conv_bwd_gate: g [N,Ho,Wo,C] (or [N,C] with per_image) gated by the saved X2 output of shape (N, Ho, Wo) -> float32 [N,H,W,C], dense or
    (out_hw = the strided conv's input size) zero-dilated."""
    N, Ho, Wo = shape
    H, W = (Ho, Wo) if out_hw is None else out_hw
    out = torch.empty(N, H, W, Cn, device=g.device)
    _lib.api().ehm_conv_bwd_gate(g, 1 if per_image else 0, y_x2, scale, out, N, Ho, Wo, Cn, H, W, _lib.stream_ptr())
    return out


def wgrad(G, x_x2, in_shape, Ci, Co, K, stride, pad, want_w=True, want_b=True):
    """ehm_conv_bwd_wgrad: (w'bar [Co,Ci,K,K] as a view of the tap-major result, b'bar [Co]); G [N,Ho,Wo,Co] dense, x_x2 the conv's saved input."""
    A, dev = _lib.api(), G.device
    N, H, W = in_shape
    ws, nb = _workspace(A.ehm_conv_bwd_wgrad_workspace_bytes, N, H, W, Ci, Co, K, stride, pad, device=dev)
    gw = torch.empty(Co, K * K * Ci, device=dev) if want_w else None
    gb = torch.empty(Co, device=dev) if want_b else None
    A.ehm_conv_bwd_wgrad(G, x_x2 if want_w else None, x_x2.shape[0], gw, gb, N, H, W, Ci, Co, K, stride, pad, ws, nb, _lib.stream_ptr())
    return (gw.view(Co, K, K, Ci).permute(0, 3, 1, 2) if want_w else None), gb


def dgrad(G, packed, Cin, Cout, K, pad, res=None):
    """Data gradient of a stride-1 view of a conv: G [N,H,W,Cin = the conv's Co] (*) flipped / transposed weight -> [N,H,W,Cout = the conv's Ci]."""
    N, H, W, _ = G.shape
    P = _lib.ptr
    y = torch.empty(N, H + 2 * (K - 1 - pad) - K + 1, W + 2 * (K - 1 - pad) - K + 1, Cout, device=G.device)
    d = _lib.ConvDesc(P(G), P(packed.buf), None, P(res), P(y), N, H, W, Cin, Cout, K, K, 1, K - 1 - pad, 0, packed.scale)
    _lib.api().ehm_conv_nhwc_split(C.byref(d), _lib.stream_ptr())
    return y


def stem_backward(img, stem_wt, stem_b, gpool, want_w=True, want_b=True, debug=False):
    """ehm_resnet_stem_backward: (w'bar [64,3,7,7], b'bar [64]) from the gated pooled cotangent [N,H/4,W/4,64]; debug: also (z, gz) [N,H/2,W/2,64]."""
    A, dev = _lib.api(), img.device
    N, _, H, W = img.shape
    ws, nb = _workspace(A.ehm_resnet_stem_backward_workspace_bytes, N, H, W, device=dev)
    gw = torch.empty(64, 147, device=dev) if want_w else None
    gb = torch.empty(64, device=dev) if want_b else None
    z = torch.empty(N, H // 2, W // 2, 64, device=dev) if debug else None
    gz = torch.empty(N, H // 2, W // 2, 64, device=dev) if debug else None
    A.ehm_resnet_stem_backward(img, stem_wt, stem_b, gpool, gw, gb, z, gz, N, H, W, ws, nb, _lib.stream_ptr())
    out = (gw.view(64, 3, 7, 7) if want_w else None), gb
    return out + (z, gz) if debug else out


def _walk(U, acts, gout, need, res, step):
    """The backward of both routes, from the top block down to the stem.  U: units(m); acts: (X2 buffer, (N, H, W)) of the stem's pooled output and of
    every conv's output; gout [N,2048]; need: per unit a tuple of flags or None; res: per unit what the step fills (returned).  No data gradient runs
    below the lowest unit that wants something.  Per conv the route's `step` supplies
        gate(g, y, shape, Cn, per_image) -> (gated, s)      the cotangent g behind the ReLU of the saved output y: a tuple, gated[0] the dense float32 tensor
        head(i, gated, cum, x, x_shape, twin=None) -> state unit i's results into res[i] from its dense conv-output cotangent (which carries cum); x: the conv's
                                                            saved input; twin: the unit that got the same gate before (a projection block's conv3)
        operand(i, gated, state, out_hw, g) -> (T, s)       that cotangent as the data gradient's input, dense or (out_hw) zero-dilated to the conv's input size
        weight(i)                                           unit i's packed flipped weight for dgrad
        stem(g, cum, per_image)                             the stem's results into res[0]
    s: the power of two (device scalar) the call multiplied in, or None.  `cum` collects them along the chain, `below` those a block's shortcut has yet to
    be brought to.  The `del`s bound the peak: a cotangent goes as soon as the next one exists."""
    def wants(i):
        return need[i] is not None and any(need[i])

    wanted = [i for i in range(len(U)) if wants(i)]
    if not wanted:
        return res
    lowest = wanted[0]
    below = []

    def carried(c, s):
        if s is None:
            return c
        below.append(s)
        return c * s

    g, per_image = _lib.f32(gout, gout.device), True
    cum = torch.ones((), device=gout.device)
    for b in range((len(U) - 1) // 4 - 1, -1, -1):
        i1, i2, i3, id_ = 1 + 4 * b, 2 + 4 * b, 3 + 4 * b, 4 + 4 * b
        if lowest > id_:
            break
        (xin, sh_in), (a1, sh1), (a2, sh2), (y, sh3) = acts[3 * b:3 * b + 4]
        c1, c2, c3 = U[i1][0], U[i2][0], U[i3][0]
        Cin, Wd, Cout, stride2 = c1.in_channels, c1.out_channels, c3.out_channels, c2.stride[0]
        dilated = sh_in[1:] if stride2 == 2 else None              # (conv2 and the projection carry the block's stride; conv1 keeps the size: sh1 is sh_in)
        project = U[id_] is not None
        gt3, s = step.gate(g, y, sh3, Cout, per_image)
        c = carried(cum, s)
        del below[:]                                                                 # the shortcut leaves here: it carries c
        st3 = std = None
        if wants(i3) or lowest < i3:
            st3 = step.head(i3, gt3, c, a2, sh2)
        if project and (wants(id_) or lowest < i1):
            std = step.head(id_, gt3, c, xin, sh_in, twin=i3)
        if lowest >= i3:
            break
        T, s = step.operand(i3, gt3, st3, None, g)
        del st3
        c = carried(c, s)
        ga2 = dgrad(T, step.weight(i3), Cout, Wd, 1, 0)
        del T
        gt2, s = step.gate(ga2, a2, sh2, Wd, False)
        c = carried(c, s)
        st2 = step.head(i2, gt2, c, a1, sh1)
        if lowest >= i2:
            break
        T, s = step.operand(i2, gt2, st2, dilated, ga2)
        del gt2, st2, ga2
        c = carried(c, s)
        ga1 = dgrad(T, step.weight(i2), Wd, Wd, 3, 1)
        del T
        gt1, s = step.gate(ga1, a1, sh1, Wd, False)
        del ga1
        c = carried(c, s)
        st1 = step.head(i1, gt1, c, xin, sh_in)
        if lowest >= i1:
            break
        T, s = step.operand(i1, gt1, st1, None, None)
        del gt1, st1
        c = carried(c, s)
        # the shortcut's gradient, brought to the power of two conv1's data gradient carries, rides into it as its `residual`
        if project:
            short, sd = step.operand(id_, gt3, std, dilated, g)
            del gt3, std
            short = dgrad(short, step.weight(id_), Cout, Cin, 1, 0)
        else:
            short, sd = gt3[0], None
            del gt3
        short.mul_(reduce(mul, below) if sd is None else reduce(mul, below) / sd)
        g = dgrad(T, step.weight(i1), Wd, Cin, 1, 0, res=short)
        del T, short
        cum, per_image = c, False
    else:
        if wants(0):
            step.stem(g, cum, per_image)
    return res


def _eval_step(U, fn, img, acts, need, res):
    """The eval-mode unit step of _walk: the gate scaled into the conv engine's range (dense for the weight gradient, gated again zero-dilated for a
    stride-2 data gradient), (w'bar, b'bar) of the FOLDED weight into res[i], the data gradient on the folded weight's pack - kept on the
    FoldedTrunk `fn` the forward ran (fn.dgrad), so rebuilt with it when a weight changes."""
    ops = [fn.stem] + [p for blk in fn.blocks for p in blk]

    def scaled(t, cum):
        return None if t is None else t * (1.0 / cum)

    def gate_(g, y, shape, Cn, per_image):
        s = pow2_scale(g)
        return (gate(g, y, shape, Cn, s, per_image=per_image), s, y, shape, Cn, per_image), s

    def head(i, gated, cum, x, x_shape, twin=None):
        n = need[i]
        if n is None or not any(n):
            return None
        conv = U[i][0]
        shared = res[twin][1] if twin is not None and n[1] else None                  # (the same column sum goes to both folded biases: once)
        gw = gb = None
        if n[0] or (n[1] and shared is None):
            gw, gb = wgrad(gated[0], x, x_shape, conv.in_channels, conv.out_channels, conv.kernel_size[0], conv.stride[0], conv.padding[0],
                           n[0], n[1] and shared is None)
        res[i] = (scaled(gw, cum), scaled(gb, cum) if shared is None else shared)
        return None

    def operand(i, gated, state, out_hw, g):
        G, s, y, shape, Cn, per_image = gated
        return (G if out_hw is None else gate(g, y, shape, Cn, s, out_hw=out_hw, per_image=per_image)), None

    def weight(i):
        if i not in fn.dgrad:
            fn.dgrad[i] = dgrad_weight(ops[i][0])
        return fn.dgrad[i]

    def stem(g, cum, per_image):
        x0, sh0 = acts[0]
        s0 = pow2_scale(g)
        G0 = gate(g, x0, sh0, 64, s0, per_image=per_image)
        gw0, gb0 = stem_backward(img, fn.stem_wt, fn.stem_b, G0, *need[0])
        res[0] = (scaled(gw0, cum * s0), scaled(gb0, cum * s0))

    return SimpleNamespace(gate=gate_, head=head, operand=operand, weight=weight, stem=stem)


def trunk_backward(m, fn, img, acts, gout, need):
    """VJP of the folded trunk.  fn: the FoldedTrunk the forward ran; img [N,3,H,W] float32; acts: what its `saved` list received; gout [N,2048];
    need: per unit of units(m) a pair (w' wanted, b' wanted) or None.  Returns per unit (w'bar [Co,Ci,KH,KW] float32 or None, b'bar or None): what is
    not asked for is neither computed nor written, and no data gradient runs below the lowest unit that wants something."""
    U = units(m)
    res = [(None, None)] * len(U)
    return _walk(U, acts, gout, need, res, _eval_step(U, fn, img, acts, need, res))


# ------------------------------------------------------------------------------------------------------------------ train-mode BatchNorm2d (csrc/bn2d_train.hip)
# With ResNet50Features.train_batchnorm under .train() every BatchNorm2d normalises with the statistics of the batch.  Once (mu, var) are known that IS the
# eval-mode fold with running_mean := mu, running_var := var, so the forward (encoders._BatchUnits) is: raw conv z -> ehm_bn2d_train_stats -> the folded
# launch.  The backward differs per unit: with G = g (.) [y > 0], R = N H W rows, xhat = (z - mu) invstd:
#     betabar = sum_p G,  gammabar = sum_p G xhat                   ehm_bn2d_train_bwd_sums  (float64 partial sums, fixed order)
#     zbar = s gamma invstd (G - betabar / R - xhat gammabar / R)   ehm_bn2d_train_bwd_zbar  (dense for the weight gradient; s: pow2_scale of the dense result,
#                                                                                             applied - dense or zero-dilated - for the data gradient)
#     wbar = wgrad(zbar, x)  (the RAW weight's gradient: no unfold),  xbar = conv_transpose(zbar, w) on the RAW weight's flipped pack
# The gates are not scaled here (G feeds no conv engine); only zbar is, and `cum` collects those powers of two.

# measurement / test hook: a list that receives, per unit the train-mode backward visits, (unit index, g, cum, zbar): the unit's incoming cotangent (for
# the last block [N, 2048] per image, before the average pool's 1 / (H W)), the power of two it carries, and its dense zbar (carrying the same).  None on
# the product path.
_train_debug_hook = None


class TrainRecord:
    """What the train-mode forward leaves for the backward: acts (X2 buffer, (N, H, W)) of the stem's pooled output and of every conv's output; bn: per unit of
    units() (z X2 or None, (N, Ho, Wo), mean, var, invstd) float32, None where an identity block has no downsample; the stem's folded operands."""

    def __init__(self, keep_z=True):
        self.acts, self.bn, self.keep_z = [], [], keep_z
        self.sync = None                 # the dist.StatSync the forward ran with (data parallel): the backward gathers through the same one
        self.stem_wt = self.stem_b = None


def _bn_ws(pixels, Cn, dev):
    """(a rank's share of a data-parallel batch may be one row, and float32 rows any multiple of 8 channels: the query's own granules bound both from above)"""
    return _workspace(_lib.api().ehm_bn2d_train_workspace_bytes, max(pixels, 2), (Cn + 31) // 32 * 32, dtype=torch.float64, device=dev)


def _sync_rows(sync, pixels):
    """(rows per item, all ranks' rows) of a unit whose rank-local z has `pixels` rows"""
    per_item, rem = divmod(pixels, sync.counts[sync.rank])
    if rem:
        raise ValueError(f"the StatSync counts {sync.counts[sync.rank]} items for this rank, which does not divide the unit's {pixels} rows")
    return per_item, per_item * sync.total


def bn_stats(z, pixels, Cn, bn=None, x2=True, eps=1e-5, momentum=0.1, sync=None):
    """ehm_bn2d_train_stats: (mean, biased var, invstd) float32 [C] of the first `pixels` rows of z (an X2 buffer, or x2=False: float32 rows); with bn, its
    eps and momentum, and its running_mean / running_var / num_batches_tracked are updated IN PLACE on the device (the caller bumps their versions).
    sync (a dist.StatSync): the statistics of ALL ranks' rows - ehm_bn2d_train_stats_local, one all-gather, ehm_bn2d_train_stats_merge on every rank."""
    dev = z.device
    total = pixels if sync is None else _sync_rows(sync, pixels)[1]
    if total < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got {total} rows of {Cn} channels")
    mean, var, invstd = (torch.empty(Cn, device=dev) for _ in range(3))
    ws, nb = _bn_ws(pixels, Cn, dev)
    rm = rv = nbt = None
    if bn is not None:
        eps, momentum, rm, rv, nbt = bn.eps, bn.momentum, bn.running_mean, bn.running_var, bn.num_batches_tracked
        if rm.dtype != torch.float32 or rv.dtype != torch.float32 or nbt.dtype != torch.int64:
            raise _lib.EgoHMRHipError("the train-mode BatchNorm2d route updates float32 running statistics and an int64 counter in place")
    z2 = z.view(-1, Cn)
    A, s = _lib.api(), _lib.stream_ptr()
    if sync is None:
        A.ehm_bn2d_train_stats(z2, 1 if x2 else 0, z2.shape[0], pixels, Cn, float(eps), float(momentum), mean, var, invstd, rm, rv, nbt, ws, nb, s)
    else:
        local = torch.empty(2, Cn, device=dev, dtype=torch.float64)
        A.ehm_bn2d_train_stats_local(z2, 1 if x2 else 0, z2.shape[0], pixels, Cn, local, ws, nb, s)
        A.ehm_bn2d_train_stats_merge(sync.gather(local), sync.rows(_sync_rows(sync, pixels)[0]), sync.world, Cn, float(eps), float(momentum), mean, var,
                                     invstd, rm, rv, nbt, s)
    return mean, var, invstd


def bn_sums(G, z, pixels, Cn, mean, invstd, x2=True, sync=None):
    """ehm_bn2d_train_bwd_sums: (betabar, gammabar) float32 [C] from G float32 [pixels, C] and the unit's raw output z.
    sync (a dist.StatSync): (betabar, gammabar, this rank's own betabar, gammabar) - the first two over ALL ranks' rows, for bn_zbar(total_rows=...); the
    own ones are the parameter gradients, which the caller's gradient sum over the ranks completes (ehm_bn2d_train_bwd_local, one all-gather, _bwd_merge)."""
    A, s, dev = _lib.api(), _lib.stream_ptr(), G.device
    gbeta, ggamma = torch.empty(Cn, device=dev), torch.empty(Cn, device=dev)
    ws, nb = _bn_ws(pixels, Cn, dev)
    z2 = z.view(-1, Cn)
    if sync is None:
        A.ehm_bn2d_train_bwd_sums(G, z2, 1 if x2 else 0, z2.shape[0], pixels, Cn, mean, invstd, gbeta, ggamma, ws, nb, s)
        return gbeta, ggamma
    local = torch.empty(2, Cn, device=dev, dtype=torch.float64)
    own_b, own_g = torch.empty(Cn, device=dev), torch.empty(Cn, device=dev)
    A.ehm_bn2d_train_bwd_local(G, z2, 1 if x2 else 0, z2.shape[0], pixels, Cn, mean, invstd, local, ws, nb, s)
    A.ehm_bn2d_train_bwd_merge(sync.gather(local), sync.world, sync.rank, Cn, gbeta, ggamma, own_b, own_g, s)
    return gbeta, ggamma, own_b, own_g


def bn_zbar(G, z, shape, Cn, mean, invstd, gamma, gbeta, ggamma, scale=None, out_hw=None, x2=True, total_rows=None):
    """ehm_bn2d_train_bwd_zbar: float32 [N,H,W,C] = scale gamma invstd (G - betabar / R - xhat gammabar / R); dense, or (out_hw) zero-dilated like gate().
    total_rows (data parallel): R = all ranks' rows, with all ranks' betabar / gammabar (ehm_bn2d_train_bwd_zbar_rows); None: R = N Ho Wo."""
    N, Ho, Wo = shape
    H, W = (Ho, Wo) if out_hw is None else out_hw
    out = torch.empty(N, H, W, Cn, device=G.device)
    z2 = z.view(-1, Cn)
    A, s = _lib.api(), _lib.stream_ptr()
    if total_rows is None:
        A.ehm_bn2d_train_bwd_zbar(G, z2, 1 if x2 else 0, z2.shape[0], mean, invstd, gamma, gbeta, ggamma, scale, out, N, Ho, Wo, Cn, H, W, s)
    else:
        A.ehm_bn2d_train_bwd_zbar_rows(G, z2, 1 if x2 else 0, z2.shape[0], mean, invstd, gamma, gbeta, ggamma, scale, out, N, Ho, Wo, Cn, H, W,
                                       int(total_rows), s)
    return out


def stem_preact(img, wt, b):
    """ehm_resnet_stem_preact: the stem's pre-pool activation [N,H/2,W/2,64] float32 for the operands wt [147][64], b [64]."""
    N, _, H, W = img.shape
    z = torch.empty(N, H // 2, W // 2, 64, device=img.device)
    _lib.api().ehm_resnet_stem_preact(img, wt, b, z, N, H, W, _lib.stream_ptr())
    return z


def train_forward(m, img, keep_z=True):
    """The train-mode forward with its record kept: (out [N,2048], TrainRecord).  Updates m's running statistics."""
    rec = TrainRecord(keep_z)
    return m.folded(train=True)(img, rec=rec), rec


# ehm_resnet_stem_wgrad's scratch in floats (include/egohmr_hip.h: "workspace: 256 * 148 * 64 floats"; it has no size query)
STEM_WGRAD_WS_FLOATS = 256 * 148 * 64


def _train_step(U, img, rec, need, res):
    """The train-mode unit step of _walk: the gate unscaled (it feeds no conv engine), per unit the BatchNorm backward (sums, zbar) and the RAW weight's
    gradient - (wbar, gammabar, betabar) into res[i] -, zbar brought into the engine's range (dense in place, or made again zero-dilated) for the data
    gradient on the raw weight's pack, built per call."""
    hook = _train_debug_hook
    sync = rec.sync

    def sums(G, z, zs, Cn, mean, invstd, x2=True):
        """-> (betabar, gammabar for zbar; betabar, gammabar as parameter gradients; zbar's R or None): one process - the same pair twice; data parallel -
        all ranks' sums over all ranks' rows, and this rank's own sums, which the gradient sum over the ranks completes"""
        pixels = zs[0] * zs[1] * zs[2]
        if sync is None:
            gb, gg = bn_sums(G, z, pixels, Cn, mean, invstd, x2=x2)
            return gb, gg, gb, gg, None
        return (*bn_sums(G, z, pixels, Cn, mean, invstd, x2=x2, sync=sync), _sync_rows(sync, pixels)[1])

    def gate_(g, y, shape, Cn, per_image):
        return (gate(g, y, shape, Cn, None, per_image=per_image), g if hook is not None else None), None

    def head(i, gated, cum, x, x_shape, twin=None):
        """-> (the dense zbar of unit i, carrying cum like the gate; betabar; gammabar)"""
        conv, bn = U[i]
        G, g_in = gated
        z, zs, mean, _, invstd = rec.bn[i]
        Co = conv.out_channels
        gbeta, ggamma, pbeta, pgamma, R = sums(G, z, zs, Co, mean, invstd)
        Z = bn_zbar(G, z, zs, Co, mean, invstd, _lib.f32(bn.weight), gbeta, ggamma, total_rows=R)
        n = need[i] or (False, False, False)
        gw = wgrad(Z, x, x_shape, conv.in_channels, Co, conv.kernel_size[0], conv.stride[0], conv.padding[0], True, False)[0] if n[0] else None
        inv = 1.0 / cum
        res[i] = (gw * inv if n[0] else None, pgamma * inv if n[1] else None, pbeta * inv if n[2] else None)
        if hook is not None:
            hook.append((i, g_in, cum, Z.clone()))
        return Z, gbeta, ggamma, R

    def operand(i, gated, state, out_hw, g):
        """zbar times s = pow2_scale of the dense zbar"""
        Z, gbeta, ggamma, R = state
        s = pow2_scale(Z)
        if out_hw is None:
            return Z.mul_(s), s
        z, zs, mean, _, invstd = rec.bn[i]
        return bn_zbar(gated[0], z, zs, Z.shape[3], mean, invstd, _lib.f32(U[i][1].weight), gbeta, ggamma, scale=s, out_hw=out_hw, total_rows=R), s

    def weight(i):
        return dgrad_weight(U[i][0].weight.detach().float())

    def stem(g, cum, per_image):
        A, dev, n0 = _lib.api(), g.device, need[0]
        x0, sh0 = rec.acts[0]
        N, _, H, W = img.shape
        G0 = gate(g, x0, sh0, 64, None, per_image=per_image)                        # the pooled cotangent, gated by [pooled > 0]
        zf = stem_preact(img, rec.stem_wt, rec.stem_b)                              # the folded pre-pool activation: its arg-max routes
        gz = torch.empty_like(zf)
        A.ehm_resnet_stem_route(zf, G0, gz, N, H, W, _lib.stream_ptr())
        del zf, G0
        conv, bn = U[0]
        _, zs, mean, _, invstd = rec.bn[0]
        wt, zero = stem_operands(conv.weight.detach().float(), torch.zeros(64, device=dev))
        z = stem_preact(img, wt, zero)                                              # the raw one: the BatchNorm's input
        gbeta, ggamma, pbeta, pgamma, R = sums(gz, z, zs, 64, mean, invstd, x2=False)
        inv = 1.0 / cum
        gw = None
        if n0[0] or hook is not None:
            Z0 = bn_zbar(gz, z, zs, 64, mean, invstd, _lib.f32(bn.weight), gbeta, ggamma, x2=False, total_rows=R)
            ws = torch.empty(STEM_WGRAD_WS_FLOATS, device=dev)
            gw = torch.empty(64, 147, device=dev)
            A.ehm_resnet_stem_wgrad(img, Z0, gw, None, N, H, W, ws, ws.numel() * 4, _lib.stream_ptr())
            gw = gw.view(64, 3, 7, 7) * inv
            if hook is not None:
                hook.append((0, g, cum, Z0, gz))
        res[0] = (gw if n0[0] else None, pgamma * inv if n0[1] else None, pbeta * inv if n0[2] else None)

    return SimpleNamespace(gate=gate_, head=head, operand=operand, weight=weight, stem=stem)


def trunk_backward_train(m, img, rec, gout, need):
    """VJP of the train-mode trunk.  rec: the forward's TrainRecord; need: per unit of units(m) (weight wanted, gamma wanted, beta wanted) or None.
    Returns per unit (wbar [Co,Ci,KH,KW], gammabar, betabar) float32, None where not asked for; no data gradient runs below the lowest unit that wants
    something.  The running statistics are not read."""
    U = units(m)
    res = [(None, None, None)] * len(U)
    return _walk(U, rec.acts, gout, need, res, _train_step(U, img, rec, need, res))


def _param_key(m):
    return tuple((p.data_ptr(), p._version) for p in m.parameters())


def _unit_flags(m, needs_input_grad):
    """(per parameter id: does it want a gradient; per unit of units(m): that of (conv.weight, bn.weight, bn.bias), or None) from a backward's
    ctx.needs_input_grad, whose entries behind (module, x) follow m.parameters()."""
    flags = dict(zip((id(p) for p in m.parameters()), needs_input_grad[2:]))
    return flags, [None if u is None else (flags[id(u[0].weight)], flags[id(u[1].weight)], flags[id(u[1].bias)]) for u in units(m)]


def _backward_result(m, flags, grads):
    """What a backward returns - None for (module, x), then one gradient or None per m.parameters() entry - from per unit of units(m) the gradients of
    (conv.weight, bn.weight, bn.bias)."""
    by_id = {}
    for u, r in zip(units(m), grads):
        if u is None:
            continue
        for p, gr in zip((u[0].weight, u[1].weight, u[1].bias), r):
            if flags[id(p)] and gr is not None:
                by_id[id(p)] = gr.to(p.dtype)
    return (None, None, *[by_id.get(id(p)) for p in m.parameters()])


class TrunkTrainFunction(torch.autograd.Function):
    """ResNet50Features.__call__ under .train() with train_batchnorm: forward(module, x, *module.parameters()) -> [B,2048] on batch statistics (the running
    ones updated in place); the backward differentiates through the mean and the variance.  The gradients go to the parameters only."""

    @staticmethod
    def forward(ctx, module, x, *params):
        img = _lib.f32(x)
        out, rec = train_forward(module, img)
        ctx.module, ctx.img, ctx.rec = module, img, rec
        ctx.key = _param_key(module)           # the parameters only: the forward itself moved the running statistics, and the backward does not read them
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        m = ctx.module
        if _param_key(m) != ctx.key:
            raise _lib.EgoHMRHipError("a parameter of ResNet50Features changed (in place, or was replaced) between the forward and the backward "
                                      "of its autograd route; run the backward before the optimizer step")
        flags, need = _unit_flags(m, ctx.needs_input_grad)
        with _lib.on_device(gout.device):
            res = trunk_backward_train(m, ctx.img, ctx.rec, gout, need)
        return _backward_result(m, flags, res)


class TrunkFunction(torch.autograd.Function):
    """ResNet50Features.__call__ with a backward: forward(module, x, *module.parameters()) -> [B,2048].  The gradients go to the parameters only."""

    @staticmethod
    def forward(ctx, module, x, *params):
        fn = module.current()
        img = _lib.f32(x)
        acts = []
        out = fn(img, saved=acts)
        ctx.module, ctx.fn, ctx.img, ctx.acts = module, fn, img, acts
        ctx.key = module._fold_key                     # (data_ptr, _version) of every parameter and buffer the forward folded
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        m = ctx.module
        if m._fold_key_fn() != ctx.key:
            # the folded weights and saved activations are the forward's, `unfold` reads the parameters as they are now: a mix of the two is no gradient
            raise _lib.EgoHMRHipError("a parameter or buffer of ResNet50Features changed (in place, or was replaced) between the forward and the backward "
                                      "of its autograd route; run the backward before the optimizer step")
        flags, unit_flags = _unit_flags(m, ctx.needs_input_grad)
        need = [None if f is None else (f[0] or f[1], f[1] or f[2]) for f in unit_flags]     # the folded (w', b') that unfold needs
        with _lib.on_device(gout.device):
            res = trunk_backward(m, ctx.fn, ctx.img, ctx.acts, gout, need)
            # (a generator: one unit's float64 gradients at a time)
            return _backward_result(m, flags, (None if u is None else unfold(*u, gw, gb) for u, (gw, gb) in zip(units(m), res)))
