"""Backward of the Modulated-GCN denoiser's graph convs on libegohmr_hip (csrc/gcn_bwd.hip + the split-f16 GEMM engine), and the
``torch.autograd.Function`` that ModulatedGCN.forward runs behind when a gradient is asked for (model.py).

One conv (modulated_gcn_conv.py:39-50 + BatchNorm1d(eval) + ReLU + residual, modulated_gcn.py:21-28, :38-42), X [rows, K] -> out [rows, N]:

    G [rows, 2N] = [h0bar | h1bar]             ehm_gcn_bwd_epilogue          (gate, BatchNorm factor, transposed adjacency mix, modulation)
    Xbar = G [W0; W1]^T                        ehm_conv_nhwc_split, H = W = 1 (float32 rows x ehm_split_pack'ed weights)
    [W0bar | W1bar] = X^T G                    the same engine: X^T as the rows, G^T packed at run time as the weight operand
    pre = X [W0 | W1]                          the same engine (recomputed, not kept by the forward)
    Mbar, adj2bar, biasbar, gammabar, betabar  ehm_gcn_bwd_params            (fixed-order sums)

The engine splits its float32 row operand into f16 hi + lo halves, so a cotangent far below 2^-14 would lose its low bits: G is multiplied by a
power of two that brings its largest entry to 2^10 before it enters a GEMM, and the products are divided by it again (both exact).  The factor is
computed on the device: no host synchronisation.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib

INPUT, OUTPUT = _lib.GCN_CONV_INPUT, _lib.GCN_CONV_OUTPUT


def _up(n, m):
    return (n + m - 1) // m * m


def pack_weight(w2):
    """float32 [Co, K] on a HIP device -> (ehm_split_pack'ed [Co padded to 128, K padded to 32], its power-of-two scale, Co rounded up to 8 = the
    column count ehm_conv_nhwc_split writes for it)."""
    Co, K = w2.shape
    wp = torch.zeros(_up(Co, 128), _up(K, 32), device=w2.device)
    wp[:Co, :K] = w2
    amax = float(wp.abs().max())
    scale = 2.0 ** math.floor(math.log2(2048.0 / amax)) if 0.0 < amax < float("inf") else 1.0
    buf = torch.empty_like(wp)
    _lib.api().ehm_split_pack(wp, buf, wp.shape[0], wp.shape[1], wp.shape[1], scale, _lib.stream_ptr())
    return buf, scale, _up(Co, 8)


def gemm_rows(x, packed, rows=None):
    """x [M, Ci] float32 (Ci a multiple of 32, contiguous) times a pack_weight() operand -> [rows or M, Co8] float32 (ehm_conv_nhwc_split, H = W = 1)."""
    buf, scale, co = packed
    M = x.shape[0] if rows is None else rows
    y = torch.empty(M, co, device=x.device)
    d = _lib.ConvDesc(_lib.ptr(x), _lib.ptr(buf), None, None, _lib.ptr(y), M, 1, 1, x.shape[1], co, 1, 1, 1, 0, 0, scale)
    _lib.api().ehm_conv_nhwc_split(C.byref(d), _lib.stream_ptr())
    return y


def pow2_scale(t, target=1024.0):
    """0-d device tensor: the power of two that brings max|t| into [target/2, target]; 1 for an all-zero or non-finite t.  No host read-back."""
    lo, hi = torch.aminmax(t)                                   # one pass, no |t| temporary
    a = torch.maximum(-lo, hi)
    s = torch.exp2(torch.floor(torch.log2(target / a)))
    return torch.where((a > 0) & torch.isfinite(s) & (s > 0), s, torch.ones_like(s))


class ConvWeights:
    """The two packed GEMM operands of one conv's backward, made on first use from W [2, K, N] (the engine contracts over an operand's columns):
    `bwd` = [W0 | W1] as [K, 2N] for Xbar = G [W0; W1]^T, `fwd` = its transpose [2N, K] for the recompute X [W0 | W1]."""

    def __init__(self, W):
        self.W = W.detach()
        self.K, self.N = W.shape[1], W.shape[2]
        self.ldg = _up(2 * self.N, 32)          # row length of G: the K granule of the engine
        self._fwd = self._bwd = None

    @property
    def fwd(self):
        if self._fwd is None:
            self._fwd = pack_weight(self.W.permute(0, 2, 1).reshape(2 * self.N, self.K).float())
        return self._fwd

    @property
    def bwd(self):
        if self._bwd is None:
            self._bwd = pack_weight(self.W.permute(1, 0, 2).reshape(self.K, 2 * self.N).float())
        return self._bwd


def _new_G(rows, cw, dev):
    return torch.empty(rows, cw.ldg, device=dev) if cw.ldg == 2 * cw.N else torch.zeros(rows, cw.ldg, device=dev)


def _gemm_grads(G, cw, X, rows, need_x, need_w, out, res):
    """The two GEMMs behind a backward epilogue's G = [h0bar | h1bar]: res['x'] = G [W0; W1]^T (need_x), res['W'] = X^T G (need_w)."""
    A, s, N, K, dev = _lib.api(), _lib.stream_ptr(), cw.N, cw.K, G.device
    sc = pow2_scale(G)
    G.mul_(sc)
    inv = 1.0 / sc
    if need_x:
        xb = gemm_rows(G, cw.bwd).mul_(inv)        # [rows, K rounded up to the engine's 8-column granule]
        res["x"] = xb if xb.shape[1] == K else xb[:, :K].contiguous()
    if need_w:
        rp = _up(rows, 32)                         # the contraction runs over the rows: padded to the engine's K granule with zeros
        alloc = lambda r: torch.empty(r, rp, device=dev) if rp == rows else torch.zeros(r, rp, device=dev)
        Xt = alloc(X.shape[1])
        Xt[:, :rows] = X[:rows].t()
        Gt = alloc(2 * N) if 2 * N % 128 == 0 else torch.zeros(_up(2 * N, 128), rp, device=dev)
        Gt[:2 * N, :rows] = G[:, :2 * N].t()
        Gp = torch.empty_like(Gt)
        A.ehm_split_pack(Gt, Gp, Gt.shape[0], rp, rp, 1.0, s)
        Wg = gemm_rows(Xt, (Gp, 1.0, _up(2 * N, 8)))[:K, :2 * N].mul_(inv)          # [K, 2N]
        gW = out.get("W")
        if gW is None:
            gW = torch.empty(2, K, N, device=dev)
        gW.copy_(Wg.reshape(K, 2, N).permute(1, 0, 2))
        res["W"] = gW


def conv_backward(h, conv, cw, X, gate, gout, bodies, need_x=True, need_w=False, need_params=False, has_bn=True, out=None):
    """VJP of the handle's conv `conv` (INPUT, a hidden conv's index, OUTPUT).

    cw: its ConvWeights; X [>= rows, Kp] float32, the conv's input with K padded to a multiple of 32 (zeros); gate [>= rows, N] float32: the
    activation before the residual add (None for the output conv); gout [rows, N] float32.  Returns a dict with 'x' [rows, K] (need_x),
    'W' [2, K, N] (need_w) and 'M', 'adj2', 'bias' (+ 'bn_weight', 'bn_bias' when has_bn) (need_params).  `out` may hold preallocated tensors for
    the parameter gradients under those names; what is not asked for is neither computed nor written.  The residual's gradient is gout itself."""
    A, s = _lib.api(), _lib.stream_ptr()
    rows, N, K, dev = bodies * 24, cw.N, cw.K, gout.device
    out = {} if out is None else out
    res = {}
    if need_x or need_w:
        G = _new_G(rows, cw, dev)
        A.ehm_gcn_bwd_epilogue(h, conv, gout, gate, G, cw.ldg, bodies, s)
        _gemm_grads(G, cw, X, rows, need_x, need_w, out, res)
    if need_params:
        pre = gemm_rows(X, cw.fwd, rows)
        nb = C.c_int64(0)
        A.ehm_gcn_bwd_params_workspace_bytes(h, conv, bodies, C.byref(nb))
        ws = torch.empty(nb.value // 4, device=dev)
        names = ("M", "adj2", "bias") + (("bn_weight", "bn_bias") if has_bn else ())
        shapes = dict(M=(24, N), adj2=(24, 24), bias=(N,), bn_weight=(N,), bn_bias=(N,))
        g = {k: out[k] if out.get(k) is not None else torch.empty(shapes[k], device=dev) for k in names}
        A.ehm_gcn_bwd_params(h, conv, gout, gate, pre, pre.shape[1], bodies, g["M"], g["adj2"], g["bias"], g.get("bn_weight"), g.get("bn_bias"),
                             ws, nb.value, s)
        res.update(g)
    return res


PARAMS_PER_CONV = ("W", "M", "adj2", "bias", "bn_weight", "bn_bias")


class GCNFunction(torch.autograd.Function):
    """ModulatedGCN.forward (modulated_gcn.py:99-116, eval mode) with a backward: forward(module, x, *params) -> [B, 24, 6].  `params` is empty (gradient
    to x only) or ModulatedGCN.grad_parameters(): W, M, adj2, bias, bn.weight, bn.bias of the input conv and every hidden conv, then W, M, adj2, bias
    of the output conv."""

    @staticmethod
    def forward(ctx, module, x, *params):
        out, saved = module._forward_saving(x)
        ctx.module, ctx.saved, ctx.n_params = module, saved, len(params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        m, sv = ctx.module, ctx.saved
        need = ctx.needs_input_grad
        need_x, pneed = need[1], need[2:]
        dev = gout.device
        B, hid, nh = sv["B"], m.hid_dim, 2 * m.num_layers
        grads = [None] * ctx.n_params

        def wants(ci, nparams=6):          # (need_w, need_params) of conv number ci in the parameter list
            if not pneed:
                return False, False
            f = pneed[6 * ci: 6 * ci + nparams]
            return bool(f[0]), any(f[1:])

        def put(ci, r, has_bn):
            for k, name in enumerate(PARAMS_PER_CONV if has_bn else PARAMS_PER_CONV[:4]):
                if name in r and pneed[6 * ci + k]:
                    grads[6 * ci + k] = r[name]

        with _lib.on_device(dev):
            h, cws = sv["h"], m._conv_weights(dev)
            g = _lib.f32(gout, dev).reshape(B * 24, 6)
            # the output conv
            nw, npar = wants(nh + 1, 4)
            r = conv_backward(h, OUTPUT, cws[nh + 1], sv["acts"][nh], None, g, B, True, nw, npar, has_bn=False)
            put(nh + 1, r, False)
            g = r["x"]
            # the residual blocks, last first: out = y2 + block input, y2 = gconv2(y1), y1 = gconv1(block input)
            for blk in reversed(range(m.num_layers)):
                l1, l2 = 2 * blk, 2 * blk + 1
                nw, npar = wants(l2 + 1)
                r2 = conv_backward(h, l2, cws[l2 + 1], sv["ys"][l1 + 1], sv["ys"][l2 + 1], g, B, True, nw, npar)
                put(l2 + 1, r2, True)
                nw, npar = wants(l1 + 1)
                r1 = conv_backward(h, l1, cws[l1 + 1], sv["acts"][l1], sv["ys"][l1 + 1], r2["x"], B, True, nw, npar)
                put(l1 + 1, r1, True)
                g = r1["x"].add_(g)                         # + the residual's gradient
            nw, npar = wants(0)
            gx = None
            if need_x or nw or npar:
                r = conv_backward(h, INPUT, cws[0], sv["xp"], sv["ys"][0], g, B, need_x, nw, npar)
                put(0, r, True)
                if need_x:
                    gx = r["x"].reshape(B, 24, m.in_dim).to(sv["x_dtype"])
        return (None, gx, *grads)


# ---------------------------------------------------------------------------------------------- train-mode BatchNorm (csrc/gcn_train.hip)
def _train_ws(h, conv, bodies, dev):
    nb = C.c_int64(0)
    _lib.api().ehm_gcn_train_workspace_bytes(h, conv, bodies, C.byref(nb))
    return torch.empty(nb.value // 8, device=dev, dtype=torch.float64), nb.value


def train_conv_forward(h, conv, cw, X, bodies, eps, momentum, running=None, res=None, y=None, out=None):
    """One BatchNorm'd conv (INPUT or a hidden conv's index) with batch statistics: X [>= rows, Kp] float32 (K padded to a multiple of 32 with zeros).

    running: (running_mean, running_var) float32 [N] on the device, updated in place, or None; res [rows, N] or None; y / out: float32 buffers of at
    least rows x N for relu(bn(z)) and for y + res (None: not written; with res, out is required).  Returns dict(z, mean, invstd): what the
    backward needs besides X and y (A: the conv's symmetrised adjacency, built once here)."""
    A, s, dev = _lib.api(), _lib.stream_ptr(), X.device
    rows, N = bodies * 24, cw.N
    pre = gemm_rows(X, cw.fwd, rows)
    ws, nb = _train_ws(h, conv, bodies, dev)
    z, mean, invstd = torch.empty(rows, N, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
    adjm = torch.empty(24, 24, device=dev)
    A.ehm_gcn_train_adjacency(h, conv, adjm, s)
    A.ehm_gcn_train_preact(h, conv, pre, pre.shape[1], bodies, adjm, z, ws, nb, s)
    rm, rv = running if running is not None else (None, None)
    A.ehm_gcn_train_stats(h, conv, z, bodies, 1, float(eps), float(momentum), mean, invstd, rm, rv, ws, nb, s)
    A.ehm_gcn_train_normalize(h, conv, z, mean, invstd, res, y, out, bodies, s)
    return dict(z=z, mean=mean, invstd=invstd, A=adjm)


def train_conv_backward(h, conv, cw, X, st, gate, gout, bodies, need_x=True, need_w=False, need_params=False, out=None):
    """VJP of train_conv_forward through the batch statistics.  st: its result; gate [>= rows, N]: its y; gout [rows, N] float32.  Returns what
    conv_backward returns for a BatchNorm'd conv; 'bias' is exact zeros (the batch mean removes the bias)."""
    A, s = _lib.api(), _lib.stream_ptr()
    rows, N, dev = bodies * 24, cw.N, gout.device
    out = {} if out is None else out
    res = {}
    ws, nb = _train_ws(h, conv, bodies, dev)
    zbar = torch.empty(rows, N, device=dev)
    g = {}
    if need_params:
        g = {k: out[k] if out.get(k) is not None else torch.empty(shp, device=dev)
             for k, shp in (("M", (24, N)), ("adj2", (24, 24)), ("bn_weight", (N,)), ("bn_bias", (N,)))}
    A.ehm_gcn_train_bn_backward(h, conv, gout, gate, st["z"], st["mean"], st["invstd"], bodies, zbar, g.get("bn_weight"), g.get("bn_bias"), ws, nb, s)
    if need_x or need_w:
        G = _new_G(rows, cw, dev)
        A.ehm_gcn_train_bwd_epilogue(h, conv, zbar, st["A"], G, cw.ldg, bodies, s)
        _gemm_grads(G, cw, X, rows, need_x, need_w, out, res)
    if need_params:
        pre = gemm_rows(X, cw.fwd, rows)
        pb = C.c_int64(0)
        A.ehm_gcn_train_bwd_params_workspace_bytes(h, conv, bodies, C.byref(pb))
        A.ehm_gcn_train_bwd_params(h, conv, zbar, st["A"], pre, pre.shape[1], bodies, g["M"], g["adj2"], torch.empty(pb.value // 4, device=dev), pb.value, s)
        bias = out["bias"].zero_() if out.get("bias") is not None else torch.zeros(N, device=dev)
        res.update(g, bias=bias)
    return res


class GCNTrainFunction(torch.autograd.Function):
    """ModulatedGCN.forward in training mode (ModulatedGCN.train_batchnorm): batch statistics in every BatchNorm, the running statistics updated in the
    forward, and a backward through the mean and the variance.  Arguments and gradient order as GCNFunction."""

    @staticmethod
    def forward(ctx, module, x, *params):
        out, saved = module._forward_train(x, save=True)
        ctx.module, ctx.saved, ctx.n_params = module, saved, len(params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        m, sv = ctx.module, ctx.saved
        need = ctx.needs_input_grad
        need_x, pneed = need[1], need[2:]
        dev = gout.device
        B, nh = sv["B"], 2 * m.num_layers
        grads = [None] * ctx.n_params

        def wants(ci, nparams=6):
            if not pneed:
                return False, False
            f = pneed[6 * ci: 6 * ci + nparams]
            return bool(f[0]), any(f[1:])

        def put(ci, r, has_bn):
            for k, name in enumerate(PARAMS_PER_CONV if has_bn else PARAMS_PER_CONV[:4]):
                if name in r and pneed[6 * ci + k]:
                    grads[6 * ci + k] = r[name]

        def bn_conv(ci, conv, g, need_x=True):            # conv number ci of the parameter list = the handle's conv `conv`
            nw, npar = wants(ci)
            if not (need_x or nw or npar):
                return None
            r = train_conv_backward(h, conv, cws[ci], sv["X"][ci], sv["st"][ci], sv["y"][ci], g, B, need_x, nw, npar)
            put(ci, r, True)
            return r.get("x")

        with _lib.on_device(dev):
            h, cws = sv["h"], sv["cws"]
            g = _lib.f32(gout, dev).reshape(B * 24, 6)
            nw, npar = wants(nh + 1, 4)
            r = conv_backward(h, OUTPUT, cws[nh + 1], sv["X"][nh + 1], None, g, B, True, nw, npar, has_bn=False)
            put(nh + 1, r, False)
            g = r["x"]
            for blk in reversed(range(m.num_layers)):
                l1, l2 = 2 * blk, 2 * blk + 1
                g1 = bn_conv(l1 + 1, l1, bn_conv(l2 + 1, l2, g))
                g = g1.add_(g)                              # + the residual's gradient
            gx = bn_conv(0, INPUT, g, need_x)
            if gx is not None:
                gx = gx.reshape(B, 24, m.in_dim).to(sv["x_dtype"])
        return (None, gx, *grads)
