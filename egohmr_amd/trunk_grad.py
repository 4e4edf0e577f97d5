"""Backward of the ResNet-50 trunk in eval mode on libegohmr_hip (csrc/conv_bwd.hip + the split-f16 conv engine), and the ``torch.autograd.Function``
that ResNet50Features.__call__ runs behind with ``grad_params`` set (encoders.py).

The forward is ResNet50Features.folded()'s X2 route with every conv's output kept: a conv's saved output is its ReLU gate (sign only) and the next conv's
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

Behind ResNet50Features.train_batchnorm (BatchNorm2d on batch statistics, csrc/bn2d_train.hip) the same walk runs with a BatchNorm backward per unit and
no fold to undo: the second half of this file (TrunkTrainFunction).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .split_gemm import pack_weight, pow2_scale


def fold(conv, bn):
    """(w', b') of ResNet50Features.folded() in float64: w' = w g / sqrt(v + eps), b' = beta - mean g / sqrt(v + eps)."""
    scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return conv.weight.double() * scale.view(-1, 1, 1, 1), bn.bias.double() - bn.running_mean.double() * scale


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
    nb = C.c_int64(0)
    A.ehm_conv_bwd_wgrad_workspace_bytes(N, H, W, Ci, Co, K, stride, pad, C.byref(nb))
    ws = torch.empty(nb.value // 4, device=dev)
    gw = torch.empty(Co, K * K * Ci, device=dev) if want_w else None
    gb = torch.empty(Co, device=dev) if want_b else None
    A.ehm_conv_bwd_wgrad(G, x_x2 if want_w else None, x_x2.shape[0], gw, gb, N, H, W, Ci, Co, K, stride, pad, ws, nb.value, _lib.stream_ptr())
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
    nb = C.c_int64(0)
    A.ehm_resnet_stem_backward_workspace_bytes(N, H, W, C.byref(nb))
    ws = torch.empty(nb.value // 4, device=dev)
    gw = torch.empty(64, 147, device=dev) if want_w else None
    gb = torch.empty(64, device=dev) if want_b else None
    z = torch.empty(N, H // 2, W // 2, 64, device=dev) if debug else None
    gz = torch.empty(N, H // 2, W // 2, 64, device=dev) if debug else None
    A.ehm_resnet_stem_backward(img, stem_wt, stem_b, gpool, gw, gb, z, gz, N, H, W, ws, nb.value, _lib.stream_ptr())
    out = (gw.view(64, 3, 7, 7) if want_w else None), gb
    return out + (z, gz) if debug else out


def _dgrad_weights(fn):
    """The packed data-gradient operands of one folded() closure (rebuilt with it when a weight changes), built on first use."""
    if getattr(fn, "dgrad", None) is None:
        fn.dgrad = {}
    return fn.dgrad


def trunk_backward(m, fn, img, acts, gout, need):
    """VJP of the folded trunk.  fn: the folded() closure the forward ran; img [N,3,H,W] float32; acts: what its `saved` list received; gout [N,2048];
    need: per unit of units(m) a pair (w' wanted, b' wanted) or None.  Returns per unit (w'bar [Co,Ci,KH,KW] float32 or None, b'bar or None): what is
    not asked for is neither computed nor written, and no data gradient runs below the lowest unit that wants something."""
    dev = gout.device
    U = units(m)
    res = [(None, None)] * len(U)
    wanted = [i for i, n in enumerate(need) if n is not None and (n[0] or n[1])]
    if not wanted:
        return res
    lowest = wanted[0]
    packs = _dgrad_weights(fn)

    def packed(i, wf):
        if i not in packs:
            packs[i] = dgrad_weight(wf)
        return packs[i]

    def scaled(t, cum):
        return None if t is None else t * (1.0 / cum)

    g, per_image = _lib.f32(gout, dev), True
    cum = torch.ones((), device=dev)
    nblocks = len(fn.blocks)
    for b in range(nblocks - 1, -1, -1):
        i1, i2, i3, id_ = 1 + 4 * b, 2 + 4 * b, 3 + 4 * b, 4 + 4 * b
        if lowest > id_:
            break
        c1, c2, c3, ds = fn.blocks[b]
        (xin, sh_in), (a1, sh1), (a2, sh2), (y, sh3) = acts[3 * b], acts[3 * b + 1], acts[3 * b + 2], acts[3 * b + 3]
        Cin, Wd, Cout = c1[0].shape[1], c1[0].shape[0], c3[0].shape[0]
        s3 = pow2_scale(g)
        G3 = gate(g, y, sh3, Cout, s3, per_image=per_image)
        cum3 = cum * s3
        n3, nd = need[i3], (need[id_] if ds is not None else None)
        gb3 = None
        if n3 is not None and (n3[0] or n3[1]):
            gw3, gb3 = wgrad(G3, a2, sh2, Wd, Cout, 1, 1, 0, n3[0], n3[1])
            res[i3] = (scaled(gw3, cum3), scaled(gb3, cum3))
        if nd is not None and (nd[0] or nd[1]):
            gwd = gbd = None
            if nd[0] or (nd[1] and gb3 is None):                                         # (the same column sum goes to both folded biases: once)
                gwd, gbd = wgrad(G3, xin, sh_in, Cin, Cout, 1, ds[2][0], 0, nd[0], nd[1] and gb3 is None)
            gbd = res[i3][1] if (nd[1] and gb3 is not None) else scaled(gbd, cum3)
            res[id_] = (scaled(gwd, cum3), gbd)
        if lowest >= i3:
            break
        ga2 = dgrad(G3, packed(i3, c3[0]), Cout, Wd, 1, 0)
        s2 = pow2_scale(ga2)
        cum2 = cum3 * s2
        G2 = gate(ga2, a2, sh2, Wd, s2)
        n2 = need[i2]
        stride2 = c2[2][0]
        if n2 is not None and (n2[0] or n2[1]):
            gw2, gb2 = wgrad(G2, a1, sh1, Wd, Wd, 3, stride2, 1, n2[0], n2[1])
            res[i2] = (scaled(gw2, cum2), scaled(gb2, cum2))
        if lowest >= i2:
            break
        if stride2 == 2:
            G2 = gate(ga2, a2, sh2, Wd, s2, out_hw=sh1[1:])
        del ga2
        ga1 = dgrad(G2, packed(i2, c2[0]), Wd, Wd, 3, 1)
        del G2
        s1 = pow2_scale(ga1)
        cum1 = cum2 * s1
        G1 = gate(ga1, a1, sh1, Wd, s1)
        del ga1
        n1 = need[i1]
        if n1 is not None and (n1[0] or n1[1]):
            gw1, gb1 = wgrad(G1, xin, sh_in, Cin, Wd, 1, 1, 0, n1[0], n1[1])
            res[i1] = (scaled(gw1, cum1), scaled(gb1, cum1))
        if lowest >= i1:
            break
        # the shortcut's gradient, brought to conv1's power of two, rides into conv1's data gradient as its `residual`
        if ds is None:
            short = G3
        else:
            if ds[2][0] == 2:
                G3 = gate(g, y, sh3, Cout, s3, out_hw=sh_in[1:], per_image=per_image)
            short = dgrad(G3, packed(id_, ds[0]), Cout, Cin, 1, 0)
        del G3
        short.mul_(s2 * s1)
        g = dgrad(G1, packed(i1, c1[0]), Wd, Cin, 1, 0, res=short)
        del G1, short
        cum, per_image = cum1, False
    else:
        n0 = need[0]
        if n0 is not None and (n0[0] or n0[1]):
            x0, sh0 = acts[0]
            s0 = pow2_scale(g)
            G0 = gate(g, x0, sh0, 64, s0, per_image=per_image)
            gw0, gb0 = stem_backward(img, fn.stem_wt, fn.stem_b, G0, n0[0], n0[1])
            res[0] = (scaled(gw0, cum * s0), scaled(gb0, cum * s0))
    return res


# ------------------------------------------------------------------------------------------------------------------ train-mode BatchNorm2d (csrc/bn2d_train.hip)
# With ResNet50Features.train_batchnorm under .train() every BatchNorm2d normalises with the statistics of the batch.  Once (mu, var) are known that IS the
# eval-mode fold with running_mean := mu, running_var := var, so the forward (encoders.py run_x2_train) is: raw conv z -> ehm_bn2d_train_stats -> the folded
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
    """What run_x2_train leaves for the backward: acts (X2 buffer, (N, H, W)) of the stem's pooled output and of every conv's output; bn: per unit of
    units() (z X2 or None, (N, Ho, Wo), mean, var, invstd) float32, None where an identity block has no downsample; the stem's folded operands."""

    def __init__(self, keep_z=True):
        self.acts, self.bn, self.keep_z = [], [], keep_z
        self.stem_wt = self.stem_b = None


def _bn_ws(pixels, Cn, dev):
    nb = C.c_int64(0)
    _lib.api().ehm_bn2d_train_workspace_bytes(pixels, Cn, C.byref(nb))
    return torch.empty(nb.value // 8, dtype=torch.float64, device=dev), nb.value


def bn_stats(z, pixels, Cn, bn=None, x2=True, eps=1e-5, momentum=0.1):
    """ehm_bn2d_train_stats: (mean, biased var, invstd) float32 [C] of the first `pixels` rows of z (an X2 buffer, or x2=False: float32 rows); with bn, its
    eps and momentum, and its running_mean / running_var / num_batches_tracked are updated IN PLACE on the device (the caller bumps their versions)."""
    dev = z.device
    if pixels < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got {pixels} rows of {Cn} channels")
    mean, var, invstd = (torch.empty(Cn, device=dev) for _ in range(3))
    ws, nb = _bn_ws(pixels, Cn, dev)
    rm = rv = nbt = None
    if bn is not None:
        eps, momentum, rm, rv, nbt = bn.eps, bn.momentum, bn.running_mean, bn.running_var, bn.num_batches_tracked
        if rm.dtype != torch.float32 or rv.dtype != torch.float32 or nbt.dtype != torch.int64:
            raise _lib.EgoHMRHipError("the train-mode BatchNorm2d route updates float32 running statistics and an int64 counter in place")
    z2 = z.view(-1, Cn)
    _lib.api().ehm_bn2d_train_stats(z2, 1 if x2 else 0, z2.shape[0], pixels, Cn, float(eps), float(momentum), mean, var, invstd, rm, rv, nbt, ws, nb,
                                    _lib.stream_ptr())
    return mean, var, invstd


def bn_sums(G, z, pixels, Cn, mean, invstd, x2=True):
    """ehm_bn2d_train_bwd_sums: (betabar, gammabar) float32 [C] from G float32 [pixels, C] and the unit's raw output z."""
    gbeta, ggamma = torch.empty(Cn, device=G.device), torch.empty(Cn, device=G.device)
    ws, nb = _bn_ws(pixels, Cn, G.device)
    z2 = z.view(-1, Cn)
    _lib.api().ehm_bn2d_train_bwd_sums(G, z2, 1 if x2 else 0, z2.shape[0], pixels, Cn, mean, invstd, gbeta, ggamma, ws, nb, _lib.stream_ptr())
    return gbeta, ggamma


def bn_zbar(G, z, shape, Cn, mean, invstd, gamma, gbeta, ggamma, scale=None, out_hw=None, x2=True):
    """ehm_bn2d_train_bwd_zbar: float32 [N,H,W,C] = scale gamma invstd (G - betabar / R - xhat gammabar / R); dense, or (out_hw) zero-dilated like gate()."""
    N, Ho, Wo = shape
    H, W = (Ho, Wo) if out_hw is None else out_hw
    out = torch.empty(N, H, W, Cn, device=G.device)
    z2 = z.view(-1, Cn)
    _lib.api().ehm_bn2d_train_bwd_zbar(G, z2, 1 if x2 else 0, z2.shape[0], mean, invstd, gamma, gbeta, ggamma, scale, out, N, Ho, Wo, Cn, H, W,
                                       _lib.stream_ptr())
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
    return m.folded(train=True)(img, rec), rec


def trunk_backward_train(m, img, rec, gout, need):
    """VJP of the train-mode trunk.  rec: the forward's TrainRecord; need: per unit of units(m) (weight wanted, gamma wanted, beta wanted) or None.
    Returns per unit (wbar [Co,Ci,KH,KW], gammabar, betabar) float32, None where not asked for; no data gradient runs below the lowest unit that wants
    something.  The running statistics are not read."""
    dev = gout.device
    U = units(m)
    res = [(None, None, None)] * len(U)
    wanted = [i for i, n in enumerate(need) if n is not None and any(n)]
    if not wanted:
        return res
    lowest = wanted[0]
    acts, hook = rec.acts, _train_debug_hook

    def raw_pack(i):
        return dgrad_weight(U[i][0].weight.detach().float())

    def unit_bwd(i, G, cum, x, x_shape, stride, pad, g_in=None):
        """-> (the dense zbar of unit i, carrying cum like G; betabar; gammabar); fills res[i]"""
        conv, bn = U[i]
        z, zs, mean, _, invstd = rec.bn[i]
        Co, Ci, K = conv.out_channels, conv.in_channels, conv.kernel_size[0]
        gbeta, ggamma = bn_sums(G, z, zs[0] * zs[1] * zs[2], Co, mean, invstd)
        Z = bn_zbar(G, z, zs, Co, mean, invstd, _lib.f32(bn.weight), gbeta, ggamma)
        n = need[i] or (False, False, False)
        gw = wgrad(Z, x, x_shape, Ci, Co, K, stride, pad, True, False)[0] if n[0] else None
        inv = 1.0 / cum
        res[i] = (gw * inv if n[0] else None, ggamma * inv if n[1] else None, gbeta * inv if n[2] else None)
        if hook is not None:
            hook.append((i, G if g_in is None else g_in, cum, Z.clone()))
        return Z, gbeta, ggamma

    def scaled_for_dgrad(i, G, zb, out_hw):
        """zbar brought into the conv engine's range by a power of two (pow2_scale of the dense zbar), dense in place or zero-dilated: (tensor, s)"""
        Z, gbeta, ggamma = zb
        s = pow2_scale(Z)
        if out_hw is None:
            return Z.mul_(s), s
        z, zs, mean, _, invstd = rec.bn[i]
        return bn_zbar(G, z, zs, Z.shape[3], mean, invstd, _lib.f32(U[i][1].weight), gbeta, ggamma, scale=s, out_hw=out_hw), s

    def wants(i):
        return need[i] is not None and any(need[i])

    g, per_image = _lib.f32(gout, dev), True
    cum = torch.ones((), device=dev)
    nblocks = (len(U) - 1) // 4
    for b in range(nblocks - 1, -1, -1):
        i1, i2, i3, id_ = 1 + 4 * b, 2 + 4 * b, 3 + 4 * b, 4 + 4 * b
        if lowest > id_:
            break
        (xin, sh_in), (a1, sh1), (a2, sh2), (y, sh3) = acts[3 * b], acts[3 * b + 1], acts[3 * b + 2], acts[3 * b + 3]
        c1, c2, c3 = U[i1][0], U[i2][0], U[i3][0]
        Cin, Wd, Cout = c1.in_channels, c1.out_channels, c3.out_channels
        stride2 = c2.stride[0]
        G3 = gate(g, y, sh3, Cout, None, per_image=per_image)
        Z3 = Zd = None
        if wants(i3) or lowest < i3:
            Z3 = unit_bwd(i3, G3, cum, a2, sh2, 1, 0, g_in=g)
        if U[id_] is not None and (wants(id_) or lowest < i1):
            Zd = unit_bwd(id_, G3, cum, xin, sh_in, stride2, 0, g_in=g)
        if lowest >= i3:
            break
        Z3, s3 = scaled_for_dgrad(i3, G3, Z3, None)
        ga2 = dgrad(Z3, raw_pack(i3), Cout, Wd, 1, 0)
        del Z3
        cum2 = cum * s3
        G2 = gate(ga2, a2, sh2, Wd, None)
        Z2 = unit_bwd(i2, G2, cum2, a1, sh1, stride2, 1, g_in=ga2)
        if lowest >= i2:
            break
        Z2, s2 = scaled_for_dgrad(i2, G2, Z2, sh1[1:] if stride2 == 2 else None)
        del G2, ga2
        ga1 = dgrad(Z2, raw_pack(i2), Wd, Wd, 3, 1)
        del Z2
        cum1 = cum2 * s2
        G1 = gate(ga1, a1, sh1, Wd, None)
        Z1 = unit_bwd(i1, G1, cum1, xin, sh_in, 1, 0, g_in=ga1)
        if lowest >= i1:
            break
        Z1, s1 = scaled_for_dgrad(i1, G1, Z1, None)
        del G1, ga1
        cum_next = cum1 * s1
        # the shortcut's gradient, brought to the power of two conv1's data gradient carries, rides in as its `residual`
        if U[id_] is None:
            short = G3.mul_(s3 * s2 * s1)
        else:
            Zd, sd = scaled_for_dgrad(id_, G3, Zd, sh_in[1:] if stride2 == 2 else None)
            short = dgrad(Zd, raw_pack(id_), Cout, Cin, 1, 0)
            short.mul_(s3 * s2 * s1 / sd)
            del Zd
        del G3
        g = dgrad(Z1, raw_pack(i1), Wd, Cin, 1, 0, res=short)
        del Z1, short
        cum, per_image = cum_next, False
    else:
        n0 = need[0]
        if n0 is not None and any(n0):
            A = _lib.api()
            x0, sh0 = acts[0]
            N, _, H, W = img.shape
            G0 = gate(g, x0, sh0, 64, None, per_image=per_image)                    # the pooled cotangent, gated by [pooled > 0]
            zf = stem_preact(img, rec.stem_wt, rec.stem_b)                          # the folded pre-pool activation: its arg-max routes
            gz = torch.empty_like(zf)
            A.ehm_resnet_stem_route(zf, G0, gz, N, H, W, _lib.stream_ptr())
            del zf, G0
            conv, bn = U[0]
            _, zs, mean, _, invstd = rec.bn[0]
            pixels = zs[0] * zs[1] * zs[2]
            wt = conv.weight.detach().float().reshape(64, 147).t().contiguous()
            z = stem_preact(img, wt, torch.zeros(64, device=dev))                   # the raw one: the BatchNorm's input
            gbeta, ggamma = bn_sums(gz, z, pixels, 64, mean, invstd, x2=False)
            inv = 1.0 / cum
            gw = None
            if n0[0] or hook is not None:
                Z0 = bn_zbar(gz, z, zs, 64, mean, invstd, _lib.f32(bn.weight), gbeta, ggamma, x2=False)
                ws = torch.empty(256 * 148 * 64, device=dev)
                gw = torch.empty(64, 147, device=dev)
                A.ehm_resnet_stem_wgrad(img, Z0, gw, None, N, H, W, ws, ws.numel() * 4, _lib.stream_ptr())
                gw = gw.view(64, 3, 7, 7) * inv
                if hook is not None:
                    hook.append((0, g, cum, Z0, gz))
            res[0] = (gw if n0[0] else None, ggamma * inv if n0[1] else None, gbeta * inv if n0[2] else None)
    return res


def _param_key(m):
    return tuple((p.data_ptr(), p._version) for p in m.parameters())


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
        flags = dict(zip((id(p) for p in m.parameters()), ctx.needs_input_grad[2:]))
        U = units(m)
        need = [None if u is None else (flags[id(u[0].weight)], flags[id(u[1].weight)], flags[id(u[1].bias)]) for u in U]
        with _lib.on_device(gout.device):
            res = trunk_backward_train(m, ctx.img, ctx.rec, gout, need)
        by_id = {}
        for u, r in zip(U, res):
            if u is None:
                continue
            for p, gr in zip((u[0].weight, u[1].weight, u[1].bias), r):
                if flags[id(p)] and gr is not None:
                    by_id[id(p)] = gr.to(p.dtype)
        return (None, None, *[by_id.get(id(p)) for p in m.parameters()])


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
        flags = dict(zip((id(p) for p in m.parameters()), ctx.needs_input_grad[2:]))
        U = units(m)
        need = []
        for u in U:
            if u is None:
                need.append(None)
                continue
            conv, bn = u
            fw, fg, fb = flags[id(conv.weight)], flags[id(bn.weight)], flags[id(bn.bias)]
            need.append((fw or fg, fg or fb))
        with _lib.on_device(gout.device):
            res = trunk_backward(m, ctx.fn, ctx.img, ctx.acts, gout, need)
            by_id = {}
            for u, (gw, gb) in zip(U, res):
                if u is None:
                    continue
                conv, bn = u
                g_w, g_gamma, g_beta = unfold(conv, bn, gw, gb)
                for p, gr in ((conv.weight, g_w), (bn.weight, g_gamma), (bn.bias, g_beta)):
                    if flags[id(p)] and gr is not None:
                        by_id[id(p)] = gr.to(p.dtype)
        return (None, None, *[by_id.get(id(p)) for p in m.parameters()])
