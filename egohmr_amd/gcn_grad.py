"""Backward of the Modulated-GCN denoiser's graph convs on libegohmr_hip (csrc/gcn_bwd.hip + the split-f16 GEMM engine), and the
``torch.autograd.Function``s that ModulatedGCN.forward runs behind when a gradient is asked for (model.py), with their forwards.

One conv (modulated_gcn_conv.py:39-50 + BatchNorm1d(eval) + ReLU + residual, modulated_gcn.py:21-28, :38-42), X [rows, K] -> out [rows, N]:

    G [rows, 2N] = [h0bar | h1bar]             ehm_gcn_bwd_epilogue          (gate, BatchNorm factor, transposed adjacency mix, modulation)
    Xbar = G [W0; W1]^T                        ehm_conv_nhwc_split, H = W = 1 (split_gemm.gemm_rows: float32 rows x ehm_split_pack'ed weights)
    [W0bar | W1bar] = X^T G                    the same engine: X^T as the rows, G^T packed at run time as the weight operand
    pre = X [W0 | W1]                          the same engine (recomputed, not kept by the forward)
    Mbar, adj2bar, biasbar, gammabar, betabar  ehm_gcn_bwd_params            (fixed-order sums)

The engine splits its float32 row operand into f16 hi + lo halves, so a cotangent far below 2^-14 would lose its low bits: G is multiplied by a
power of two that brings its largest entry to 2^10 before it enters a GEMM, and the products are divided by it again (both exact).  The factor is
computed on the device: no host synchronisation.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .fused import PRECISIONS
from .split_gemm import Packed, gemm_rows, pack_weight, pad_cols, pow2_scale, round_up

INPUT, OUTPUT = _lib.GCN_CONV_INPUT, _lib.GCN_CONV_OUTPUT


class ConvWeights:
    """The two packed GEMM operands of one conv, made on first use from W [2, K, N] (the engine contracts over an operand's columns):
    `fwd` = [W0 | W1]^T as [2N, K] for X [W0 | W1] (the input conv's forward, the backward's recompute), `bwd` = its transpose [K, 2N] for
    Xbar = G [W0; W1]^T."""

    def __init__(self, W):
        self.W = W.detach()
        self.K, self.N = W.shape[1], W.shape[2]
        self.ldg = round_up(2 * self.N, 32)          # row length of G: the K granule of the engine
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


def _xt_g(X, G, rows, K, N):
    """X[:rows, :K]^T G[:, :N] -> a view [K, N] of the engine's result: X^T as the rows, G^T packed at run time as the weight operand (G already carries its
    power of two).  The contraction runs over the rows: padded to the engine's K granule with zeros."""
    dev = X.device
    rp = round_up(rows, 32)
    alloc = lambda r: torch.empty(r, rp, device=dev) if rp == rows else torch.zeros(r, rp, device=dev)
    Xt = alloc(X.shape[1])
    Xt[:, :rows] = X[:rows].t()
    Gt = alloc(N) if N % 128 == 0 else torch.zeros(round_up(N, 128), rp, device=dev)
    Gt[:N, :rows] = G[:, :N].t()
    Gp = torch.empty_like(Gt)
    _lib.api().ehm_split_pack(Gt, Gp, Gt.shape[0], rp, rp, 1.0, _lib.stream_ptr())
    return gemm_rows(Xt, Packed(Gp, 1.0, round_up(N, 8), None))[:K, :N]


def _gemm_grads(epilogue, cw, X, rows, need_x, need_w, out, res):
    """epilogue(G) writes a conv's G = [h0bar | h1bar] [rows, cw.ldg]; then the two GEMMs behind it: res['x'] = G [W0; W1]^T (need_x),
    res['W'] = X^T G (need_w)."""
    N, K, dev = cw.N, cw.K, X.device
    G = torch.empty(rows, cw.ldg, device=dev) if cw.ldg == 2 * N else torch.zeros(rows, cw.ldg, device=dev)
    epilogue(G)
    sc = pow2_scale(G)
    G.mul_(sc)
    inv = 1.0 / sc
    if need_x:
        xb = gemm_rows(G, cw.bwd).mul_(inv)        # [rows, K rounded up to the engine's 8-column granule]
        res["x"] = xb if xb.shape[1] == K else xb[:, :K].contiguous()
    if need_w:
        Wg = _xt_g(X, G, rows, K, 2 * N).mul_(inv)          # [K, 2N]
        gW = out.get("W")
        if gW is None:
            gW = torch.empty(2, K, N, device=dev)
        gW.copy_(Wg.reshape(K, 2, N).permute(1, 0, 2))
        res["W"] = gW


def _param_bufs(names, N, out, dev):
    """The named parameter gradients' tensors: those preallocated in `out`, else new ones."""
    shapes = dict(M=(24, N), adj2=(24, 24), bias=(N,), bn_weight=(N,), bn_bias=(N,))
    return {k: out[k] if out.get(k) is not None else torch.empty(shapes[k], device=dev) for k in names}


def _recompute(query, h, conv, cw, X, bodies):
    """(pre = X [W0 | W1], float32 workspace of a parameter-gradient kernel, its byte size as `query` gives it)"""
    pre = gemm_rows(X, cw.fwd, bodies * 24)
    nb = C.c_int64(0)
    query(h, conv, bodies, C.byref(nb))
    return pre, torch.empty(nb.value // 4, device=X.device), nb.value


def conv_backward(h, conv, cw, X, gate, gout, bodies, need_x=True, need_w=False, need_params=False, has_bn=True, out=None):
    """VJP of the handle's conv `conv` (INPUT, a hidden conv's index, OUTPUT).

    cw: its ConvWeights; X [>= rows, Kp] float32, the conv's input with K padded to a multiple of 32 (zeros); gate [>= rows, N] float32: the
    activation before the residual add (None for the output conv); gout [rows, N] float32.  Returns a dict with 'x' [rows, K] (need_x),
    'W' [2, K, N] (need_w) and 'M', 'adj2', 'bias' (+ 'bn_weight', 'bn_bias' when has_bn) (need_params).  `out` may hold preallocated tensors for
    the parameter gradients under those names; what is not asked for is neither computed nor written.  The residual's gradient is gout itself."""
    A, s = _lib.api(), _lib.stream_ptr()
    out = {} if out is None else out
    res = {}
    if need_x or need_w:
        _gemm_grads(lambda G: A.ehm_gcn_bwd_epilogue(h, conv, gout, gate, G, cw.ldg, bodies, s), cw, X, bodies * 24, need_x, need_w, out, res)
    if need_params:
        pre, ws, nb = _recompute(A.ehm_gcn_bwd_params_workspace_bytes, h, conv, cw, X, bodies)
        g = _param_bufs(("M", "adj2", "bias") + (("bn_weight", "bn_bias") if has_bn else ()), cw.N, out, gout.device)
        A.ehm_gcn_bwd_params(h, conv, gout, gate, pre, pre.shape[1], bodies, g["M"], g["adj2"], g["bias"], g.get("bn_weight"), g.get("bn_bias"), ws, nb, s)
        res.update(g)
    return res


PARAMS_PER_CONV = ("W", "M", "adj2", "bias", "bn_weight", "bn_bias")


# ---------------------------------------------------------------------------------------------- train-mode BatchNorm (csrc/gcn_train.hip)
def _train_ws(h, conv, bodies, dev):
    nb = C.c_int64(0)
    _lib.api().ehm_gcn_train_workspace_bytes(h, conv, bodies, C.byref(nb))
    return torch.empty(nb.value // 8, device=dev, dtype=torch.float64), nb.value


def train_conv_forward(h, conv, cw, X, bodies, eps, momentum, running=None, res=None, y=None, out=None, sync=None):
    """One BatchNorm'd conv (INPUT or a hidden conv's index) with batch statistics: X [>= rows, Kp] float32 (K padded to a multiple of 32 with zeros).
    sync (a dist.StatSync, data parallel): the statistics are those of ALL ranks' rows - this rank's (mean, M2) in float64, one all-gather, the same merge
    on every rank (ehm_gcn_train_stats_local / _merge); it rides in the result for the backward.

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
    if sync is None:
        A.ehm_gcn_train_stats(h, conv, z, bodies, 1, float(eps), float(momentum), mean, invstd, rm, rv, ws, nb, s)
    else:
        local = torch.empty(2, N, device=dev, dtype=torch.float64)
        A.ehm_gcn_train_stats_local(h, conv, z, bodies, 1, local, ws, nb, s)
        A.ehm_gcn_train_stats_merge(h, conv, sync.gather(local), sync.rows(24), sync.world, float(eps), float(momentum), mean, invstd, rm, rv, s)
    A.ehm_gcn_train_normalize(h, conv, z, mean, invstd, res, y, out, bodies, s)
    return dict(z=z, mean=mean, invstd=invstd, A=adjm, sync=sync)


def train_conv_backward(h, conv, cw, X, st, gate, gout, bodies, need_x=True, need_w=False, need_params=False, out=None):
    """VJP of train_conv_forward through the batch statistics.  st: its result; gate [>= rows, N]: its y; gout [rows, N] float32.  Returns what
    conv_backward returns for a BatchNorm'd conv; 'bias' is exact zeros (the batch mean removes the bias)."""
    A, s = _lib.api(), _lib.stream_ptr()
    rows, N, dev = bodies * 24, cw.N, gout.device
    out = {} if out is None else out
    res = {}
    ws, nb = _train_ws(h, conv, bodies, dev)
    zbar = torch.empty(rows, N, device=dev)
    g = _param_bufs(("M", "adj2", "bn_weight", "bn_bias"), N, out, dev) if need_params else {}
    sync = st.get("sync")
    if sync is None:
        A.ehm_gcn_train_bn_backward(h, conv, gout, gate, st["z"], st["mean"], st["invstd"], bodies, zbar, g.get("bn_weight"), g.get("bn_bias"), ws, nb, s)
    else:                       # zbar on all ranks' sums; bn_weight / bn_bias receive this rank's own, which the caller's gradient sum completes
        local = torch.empty(2, N, device=dev, dtype=torch.float64)
        A.ehm_gcn_train_bwd_local(h, conv, gout, gate, st["z"], st["mean"], st["invstd"], bodies, local, ws, nb, s)
        A.ehm_gcn_train_bwd_merge(h, conv, sync.gather(local), sync.rows(24), sync.world, sync.rank, gout, gate, st["z"], st["mean"], st["invstd"], bodies,
                                  zbar, g.get("bn_weight"), g.get("bn_bias"), ws, nb, s)
    if need_x or need_w:
        _gemm_grads(lambda G: A.ehm_gcn_train_bwd_epilogue(h, conv, zbar, st["A"], G, cw.ldg, bodies, s), cw, X, rows, need_x, need_w, out, res)
    if need_params:
        pre, pws, pb = _recompute(A.ehm_gcn_train_bwd_params_workspace_bytes, h, conv, cw, X, bodies)
        A.ehm_gcn_train_bwd_params(h, conv, zbar, st["A"], pre, pre.shape[1], bodies, g["M"], g["adj2"], pws, pb, s)
        bias = out["bias"].zero_() if out.get("bias") is not None else torch.zeros(N, device=dev)
        res.update(g, bias=bias)
    return res


# ---------------------------------------------------------------------------------------------- the non-local block (csrc/nonlocal_bwd.hip)
# NONLocalBlock2D on the joint axis (modulated_gcn.py:104-110, nets/non_local_embedded_gaussian.py:62-85) on float32 rows X [rows, hid]:
#     qkv = X [theta | phi | g]^T + b,  y = softmax(theta phi^T) g per body,  u = y W0^T + b0,  out = BatchNorm2d(u) + X
# behind ModulatedGCN.nonlocal_grad.  The gradients come back under these names, the order in which ModulatedGCN.grad_parameters appends them:
NONLOCAL_PARAMS = ("theta.weight", "theta.bias", "phi.weight", "phi.bias", "g.weight", "g.bias", "W.0.weight", "W.0.bias", "W.1.weight", "W.1.bias")


class NonLocalWeights:
    """The block's four packed GEMM operands, made on first use from its 1x1 convs (the engine contracts over an operand's columns): `qkv_fwd` =
    [theta; phi; g] [3 Ci, hid] with its bias and `w0_fwd` = W.0 [hid, Ci] with its bias for the forward, `qkv_bwd`, `w0_bwd` = their transposes for the
    two data gradients."""

    def __init__(self, nl, dev):
        f = lambda t: _lib.f32(t, dev)
        self.Ci, self.hid = nl.g.weight.shape[0], nl.g.weight.shape[1]
        self.wqkv = torch.cat([f(nl.theta.weight), f(nl.phi.weight), f(nl.g.weight)], 0).flatten(1)       # [3 Ci, hid]
        self.bqkv = torch.cat([f(nl.theta.bias), f(nl.phi.bias), f(nl.g.bias)], 0)
        self.w0, self.b0 = f(nl.W[0].weight).flatten(1), f(nl.W[0].bias)                                    # [hid, Ci]
        if self.hid % 64 or self.w0.shape != (self.hid, self.Ci) or 2 * self.Ci != self.hid:
            raise _lib.EgoHMRHipError(f"the non-local block's backward is built for hid_dim % 64 == 0 and inter_channels = hid_dim / 2 (got {self.hid}, {self.Ci})")
        self._packed = {}

    def _get(self, name, make):
        if name not in self._packed:
            self._packed[name] = make()
        return self._packed[name]

    qkv_fwd = property(lambda self: self._get("qkv_fwd", lambda: pack_weight(self.wqkv, self.bqkv)))
    w0_fwd = property(lambda self: self._get("w0_fwd", lambda: pack_weight(self.w0, self.b0)))
    qkv_bwd = property(lambda self: self._get("qkv_bwd", lambda: pack_weight(self.wqkv.t().contiguous())))
    w0_bwd = property(lambda self: self._get("w0_bwd", lambda: pack_weight(self.w0.t().contiguous())))


def _column_sums(G, rows, Cn):
    """sum over the rows of G float32 [rows, Cn] -> [Cn], in the fixed order of ehm_bn2d_train_bwd_sums (its gbeta; its ggamma is not used)."""
    from . import trunk_grad
    zero = torch.zeros(Cn, device=G.device)
    return trunk_grad.bn_sums(G, G, rows, Cn, zero, zero, x2=False)[0]


def nonlocal_forward(nw, bn, X, bodies, train, sync=None, out=None, save=True):
    """The block on X [>= rows, hid] float32 rows (rows = 24 bodies).  bn: its BatchNorm2d (W.1).  train False: frozen running statistics; True: the batch's
    (ehm_bn2d_train_stats on float32 rows, pixels = rows), with running_mean / running_var / num_batches_tracked updated as nn.BatchNorm2d updates them;
    sync (a dist.StatSync): the statistics of ALL ranks' rows (ehm_bn2d_train_stats_local, one all-gather, _stats_merge).  out: a float32 buffer of at
    least rows x hid for the result (None: a new one).  Returns (out, st): st what nonlocal_backward needs besides X, or None without `save`."""
    from . import trunk_grad
    A, s, dev = _lib.api(), _lib.stream_ptr(), X.device
    rows, hid, Ci = bodies * 24, nw.hid, nw.Ci
    qkv = gemm_rows(X, nw.qkv_fwd, rows)
    y = torch.empty(rows, Ci, device=dev)
    A.ehm_nonlocal_attention(qkv, y, bodies, Ci, s)
    u = gemm_rows(y, nw.w0_fwd, rows)
    gamma, beta = _lib.f32(bn.weight, dev), _lib.f32(bn.bias, dev)
    if train:
        mean, _, invstd = trunk_grad.bn_stats(u, rows, hid, bn, x2=False, sync=sync)
        for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked):      # the kernel wrote them through their pointers: tell torch (nonlocal_packed's key)
            torch.autograd.graph.increment_version(t)
    else:
        mean = _lib.f32(bn.running_mean, dev)
        invstd = torch.rsqrt(bn.running_var.detach().to(dev).double() + bn.eps).float()
    out = torch.empty(rows, hid, device=dev) if out is None else out
    A.ehm_nonlocal_bn_residual(u, mean, invstd, gamma, beta, X, out, rows, hid, s)
    return out, (dict(qkv=qkv, y=y, u=u, mean=mean, invstd=invstd, gamma=gamma, train=bool(train), sync=sync if train else None) if save else None)


def nonlocal_backward(nw, X, st, gout, bodies, need_x=True, need=(True,) * 10):
    """VJP of nonlocal_forward.  X: its input; st: its record; gout [rows, hid] float32; need: which of NONLOCAL_PARAMS are wanted.  Returns a dict with 'x'
    [rows, hid] (need_x; the residual's share included) and the wanted parameter gradients under their NONLOCAL_PARAMS names, shaped like the parameters.
    The bias gradients are fixed-order column sums (under train-mode statistics that of 'W.0.bias' is zero to rounding: the batch mean removes that bias);
    under sync the BatchNorm's data gradient runs on all ranks' sums (ehm_bn2d_train_bwd_local / _merge / _zbar_rows) and every parameter gradient is
    this rank's own, which the caller's sum completes."""
    from . import trunk_grad
    A, s, dev = _lib.api(), _lib.stream_ptr(), gout.device
    rows, hid, Ci = bodies * 24, nw.hid, nw.Ci
    need = dict(zip(NONLOCAL_PARAMS, need))
    res = {}
    sync = st["sync"]
    # BatchNorm2d
    if st["train"]:
        sums = trunk_grad.bn_sums(gout, st["u"], rows, hid, st["mean"], st["invstd"], x2=False, sync=sync)
        gbeta, ggamma = sums[:2]
        own_b, own_g = sums[2:] if sync is not None else sums
        total = None if sync is None else 24 * sync.total
    else:
        gbeta = ggamma = torch.zeros(hid, device=dev)                      # frozen statistics: ubar = gamma invstd G
        total = None
        if need["W.1.weight"] or need["W.1.bias"]:
            own_b, own_g = trunk_grad.bn_sums(gout, st["u"], rows, hid, st["mean"], st["invstd"], x2=False)
    if need["W.1.weight"]:
        res["W.1.weight"] = own_g
    if need["W.1.bias"]:
        res["W.1.bias"] = own_b
    upstream = need_x or any(need[k] for k in NONLOCAL_PARAMS[:8])
    if not upstream:
        return res
    ubar = trunk_grad.bn_zbar(gout, st["u"], (rows, 1, 1), hid, st["mean"], st["invstd"], st["gamma"], gbeta, ggamma, x2=False,
                              total_rows=total).view(rows, hid)
    # W.0: u = y W0^T + b0
    if need["W.0.bias"]:
        res["W.0.bias"] = _column_sums(ubar, rows, hid)
    sc = pow2_scale(ubar)
    ubar.mul_(sc)
    inv = 1.0 / sc
    if need["W.0.weight"]:
        res["W.0.weight"] = _xt_g(st["y"], ubar, rows, Ci, hid).mul_(inv).t().reshape(hid, Ci, 1, 1).contiguous()
    if not (need_x or any(need[k] for k in NONLOCAL_PARAMS[:6])):
        return res
    ybar = gemm_rows(ubar, nw.w0_bwd).mul_(inv)                            # [rows, Ci]
    # the attention
    gqkv = torch.empty(rows, 3 * Ci, device=dev)
    A.ehm_nonlocal_attention_backward(st["qkv"], ybar, gqkv, bodies, Ci, s)
    # [theta | phi | g]: qkv = X Wqkv^T + b
    if any(need[k] for k in ("theta.bias", "phi.bias", "g.bias")):
        gb = _column_sums(gqkv, rows, 3 * Ci)
        for i, k in enumerate(("theta.bias", "phi.bias", "g.bias")):
            if need[k]:
                res[k] = gb[i * Ci:(i + 1) * Ci].contiguous()
    sc = pow2_scale(gqkv)
    gqkv.mul_(sc)
    inv = 1.0 / sc
    if any(need[k] for k in ("theta.weight", "phi.weight", "g.weight")):
        gw = _xt_g(X, gqkv, rows, hid, 3 * Ci).mul_(inv).t()               # [3 Ci, hid]
        for i, k in enumerate(("theta.weight", "phi.weight", "g.weight")):
            if need[k]:
                res[k] = gw[i * Ci:(i + 1) * Ci].reshape(Ci, hid, 1, 1).contiguous()
    if need_x:
        res["x"] = gemm_rows(gqkv, nw.qkv_bwd).mul_(inv).add_(gout)       # + the residual's gradient
    return res


# ---------------------------------------------------------------------------------------------- ModulatedGCN.forward with a backward
# What a forward below keeps for the backward: dict(h, cws, B, x_dtype, convs): the handle and the ConvWeights it ran on, and one record (X, gate, st) per conv
# in the handle's order (input conv, hidden convs, output conv) - X [>= rows, Kp] the conv's float32 input, gate its activation before the residual add
# (None for the output conv), st what train_conv_forward returned (None: eval-mode BatchNorm)

def _geometry(x):
    """(B, rows, rows rounded up to the hidden convs' row tile)"""
    rows, tile = x.shape[0] * 24, _lib.api().ehm_gcn_row_tile()
    return x.shape[0], rows, (rows + tile - 1) // tile * tile


@torch.no_grad()
def forward_saving(m, x):
    """ModulatedGCN.forward for GCNFunction: the same input conv, then the hidden convs ONE launch each (ehm_gcn_hidden_layer, no residual inside: the add
    happens on the float32 copies, so that every conv's ReLU output - its gate - exists on its own), then gconv_output.  Returns (out [B, 24, 6], saved)."""
    if m.precision == "f16":
        raise _lib.EgoHMRHipError(m.GRAD_F16)
    if m.nonlocal_layer and not m.nonlocal_grad:
        raise NotImplementedError("ModulatedGCN.forward: the non-local block has no backward; the autograd route needs nonlocal_layer=False"
                                  " (or ModulatedGCN.nonlocal_grad = True, which turns the block's backward on)")
    A = _lib.api()
    dev = x.device
    hid, nh = m.hid_dim, 2 * m.num_layers
    with _lib.on_device(dev):
        h, cws = m._native(dev)
        xp, pre = m._input_gemm(x, cws[0])
        s = _lib.stream_ptr()
        B, rows, rows_pad = _geometry(x)
        split = m.precision == "f16x3"                       # activations between the convs in the X2 split format (the last hidden conv writes float32)

        def to_f32(buf, is_f32):
            if is_f32:
                return buf
            out = torch.empty(rows_pad, hid, device=dev)
            A.ehm_gcn_unpack_activations(buf, out, rows_pad, hid, 32, s)
            return out

        def to_mode(f):
            if not split:
                return f
            out = torch.zeros(rows_pad, hid, device=dev)
            A.ehm_gcn_pack_activations_checked(h, f, out, rows, s)
            return out

        cur = torch.zeros(rows_pad, hid, device=dev)
        A.ehm_gcn_input_layer_rows(h, pre, cur, B, s)
        cur_f = to_f32(cur, not split or nh == 0)
        convs = [(xp, cur_f, None)]
        for l in range(0, nh, 2):
            y1 = torch.zeros(rows_pad, hid, device=dev)
            A.ehm_gcn_hidden_layer(h, l, cur, None, y1, rows_pad, s)
            y1_f = to_f32(y1, not split)
            y2 = torch.zeros(rows_pad, hid, device=dev)
            A.ehm_gcn_hidden_layer(h, l + 1, y1, None, y2, rows_pad, s)
            y2_f = to_f32(y2, not split or l + 2 == nh)
            convs += [(cur_f, y1_f, None), (y1_f, y2_f, None)]
            cur_f = y2_f + cur_f                              # modulated_gcn.py:42
            cur = to_mode(cur_f) if l + 2 < nh else cur_f
        nl = None
        if m.nonlocal_layer:                                   # modulated_gcn.py:104-110 (the output conv reads whole row tiles: zeros behind the rows)
            nw = m.nonlocal_weights(dev)
            feat, st = nonlocal_forward(nw, m.non_local.W[1], cur_f, B, False, out=torch.zeros(rows_pad, hid, device=dev))
            nl, cur_f = (nw, cur_f, st), feat
        convs.append((cur_f, None, None))
        x0 = torch.empty(B, 144, device=dev)
        A.ehm_gcn_output_layer(h, cur_f, None, x0, B, 1, s)
        A.ehm_gcn_stack_status(h, s)
    return x0.view(B, 24, 6), dict(h=h, cws=cws, B=B, x_dtype=x.dtype, convs=convs, nl=nl)


@torch.no_grad()
def forward_train(m, x, save):
    """ModulatedGCN.forward under .train() with `train_batchnorm`: per BatchNorm'd conv the split-f16 GEMM X [W0 | W1], then ehm_gcn_train_preact (modulation,
    adjacency mix, bias), ehm_gcn_train_stats (batch mean / biased variance, running statistics) and ehm_gcn_train_normalize (BatchNorm, ReLU,
    residual) on float32 activations; gconv_output as in eval mode.  The handle is this call's own: the running statistics change here, so the
    eval-mode one (ModulatedGCN._native) is rebuilt by the next eval() call through its TensorKey.  Returns (out [B, 24, 6], saved or None).
    With ModulatedGCN.stat_sync set (data parallel) every BatchNorm runs on all ranks' rows - also under no_grad, which still updates the running
    statistics."""
    A = _lib.api()
    dev = x.device
    sync = m.stat_sync
    if sync is not None and sync.counts[sync.rank] != x.shape[0]:
        raise ValueError(f"ModulatedGCN.stat_sync counts {sync.counts[sync.rank]} items for this rank, the input has {x.shape[0]}")
    hid, nh = m.hid_dim, 2 * m.num_layers
    mods = m._convs()
    with _lib.on_device(dev):
        h, keep = m.create_native_handle(dev)
        h = _lib.Handle(h, A.ehm_gcn_destroy, keep)
        A.ehm_gcn_set_precision(h, PRECISIONS[m.precision])
        cws = [ConvWeights(_lib.f32(gc.W, dev)) for gc, _ in mods]
        s = _lib.stream_ptr()
        B, rows, rows_pad = _geometry(x)
        convs = []

        def conv(idx, X, res, last):
            """the handle's conv idx on X; the result (the output conv reads whole row tiles: zeros behind the last one's rows)"""
            ci = len(convs)
            bn = mods[ci][1]
            running = (_lib.f32(bn.running_mean, dev).clone(), _lib.f32(bn.running_var, dev).clone())
            if res is None:                               # the result is y itself
                y, out = (None, torch.zeros(rows_pad, hid, device=dev)) if last else (torch.empty(rows, hid, device=dev), None)
            else:                                         # y is kept for the backward only: its gate
                y = torch.empty(rows, hid, device=dev) if save else None
                out = torch.zeros(rows_pad, hid, device=dev) if last else torch.empty(rows, hid, device=dev)
            st = train_conv_forward(h, idx, cws[ci], X, B, bn.eps, bn.momentum, running, res, y, out, sync)
            bn.running_mean.copy_(running[0])             # (copy_: the buffers' _version moves, which the eval-mode handle's key sees)
            bn.running_var.copy_(running[1])
            bn.num_batches_tracked.add_(1)
            result = out if out is not None else y
            convs.append((X, y if y is not None else result, st))
            return result

        # (the input GEMM runs inside train_conv_forward, like every conv's: only the padding of ModulatedGCN._input_gemm is needed here)
        cur = conv(INPUT, pad_cols(_lib.f32(x).reshape(rows, m.in_dim), round_up(m.in_dim, 32)), None, nh == 0)
        for l in range(0, nh, 2):
            y1 = conv(l, cur, None, False)
            cur = conv(l + 1, y1, cur, l + 2 == nh)
        nl = None
        if m.nonlocal_layer:                                   # (behind nonlocal_grad: ModulatedGCN._check_train); its BatchNorm2d joins the ranks' statistics
            nw = NonLocalWeights(m.non_local, dev)
            feat, st = nonlocal_forward(nw, m.non_local.W[1], cur, B, True, sync=sync, out=torch.zeros(rows_pad, hid, device=dev), save=save)
            nl, cur = (nw, cur, st), feat
        convs.append((cur, None, None))
        x0 = torch.empty(B, 144, device=dev)
        A.ehm_gcn_output_layer(h, cur, None, x0, B, 1, s)
        A.ehm_gcn_stack_status(h, s)
    return x0.view(B, 24, 6), dict(h=h, cws=cws, B=B, x_dtype=x.dtype, convs=convs, nl=nl) if save else None


class GCNFunction(torch.autograd.Function):
    """ModulatedGCN.forward (modulated_gcn.py:99-116, eval mode) with a backward: forward(module, x, *params) -> [B, 24, 6].  `params` is empty (gradient
    to x only) or ModulatedGCN.grad_parameters(): W, M, adj2, bias, bn.weight, bn.bias of the input conv and every hidden conv, then W, M, adj2, bias
    of the output conv, then - a module with the non-local block, behind ModulatedGCN.nonlocal_grad - the block's ten (NONLOCAL_PARAMS)."""

    @staticmethod
    def forward(ctx, module, x, *params):
        out, ctx.saved = forward_saving(module, x)
        ctx.n_params = len(params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        sv = ctx.saved
        need_x, pneed = ctx.needs_input_grad[1], ctx.needs_input_grad[2:]
        h, cws, B, convs = sv["h"], sv["cws"], sv["B"], sv["convs"]
        last = len(convs) - 1                       # the output conv's number in the parameter list
        grads = [None] * ctx.n_params

        def wants(ci, nparams):                     # (need_w, need_params) of conv number ci in the parameter list
            if not pneed:
                return False, False
            f = pneed[6 * ci: 6 * ci + nparams]
            return bool(f[0]), any(f[1:])

        def conv(ci, g, need_x=True):               # conv number ci: its input's gradient from g, its parameters' gradients into grads
            names = PARAMS_PER_CONV if ci < last else PARAMS_PER_CONV[:4]
            nw, npar = wants(ci, len(names))
            if not (need_x or nw or npar):
                return None
            X, gate, st = convs[ci]
            idx = INPUT if ci == 0 else OUTPUT if ci == last else ci - 1
            if st is not None:
                r = train_conv_backward(h, idx, cws[ci], X, st, gate, g, B, need_x, nw, npar)
            else:
                r = conv_backward(h, idx, cws[ci], X, gate, g, B, need_x, nw, npar, has_bn=ci < last)
            for k, name in enumerate(names):
                if name in r and pneed[6 * ci + k]:
                    grads[6 * ci + k] = r[name]
            return r.get("x")

        with _lib.on_device(gout.device):
            g = conv(last, _lib.f32(gout, gout.device).reshape(B * 24, 6))
            if sv.get("nl") is not None:                # the non-local block between the last residual add and gconv_output: its ten parameters are appended
                nw, X, st = sv["nl"]
                base = 6 * last + 4
                flags = tuple(bool(f) for f in pneed[base:base + 10]) if pneed else (False,) * 10
                r = nonlocal_backward(nw, X, st, g, B, True, flags)
                for k, name in enumerate(NONLOCAL_PARAMS):
                    if flags[k]:
                        grads[base + k] = r[name]
                g = r["x"]
            # the residual blocks, last first: out = y2 + block input, y2 = gconv2(y1), y1 = gconv1(block input)
            for c2 in range(last - 1, 1, -2):
                g = conv(c2 - 1, conv(c2, g)).add_(g)           # + the residual's gradient
            gx = conv(0, g, need_x)
            if gx is not None:
                gx = gx.reshape(B, 24, cws[0].K).to(sv["x_dtype"])
        return (None, gx, *grads)


class GCNTrainFunction(GCNFunction):
    """ModulatedGCN.forward in training mode (ModulatedGCN.train_batchnorm): batch statistics in every BatchNorm, the running statistics updated in the
    forward, and a backward through the mean and the variance.  Arguments, gradient order and the backward's walk as GCNFunction."""

    @staticmethod
    def forward(ctx, module, x, *params):
        out, ctx.saved = forward_train(module, x, save=True)
        ctx.n_params = len(params)
        return out
