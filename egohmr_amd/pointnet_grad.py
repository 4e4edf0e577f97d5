"""Backward of the scene PointNet on libegohmr_hip (csrc/pointnet_bwd.hip + the split-f16 GEMM engine), and the ``torch.autograd.Function`` that
ResnetPointnet.forward runs behind when a gradient is asked for (encoders.py).

One block (respointnet.py:62-97 inside :33-59), x = cat[net, pooled] (block 0: x = net0 = fc_pos_0(p)), h = fc_0(relu(x)), net' = fc_1(relu(h)) + shortcut(x),
pooled' = max over the N points of a body; gnet' / gpool' = the gradients arriving at net' / pooled':

    arg [B,H]                                  ehm_pointnet_pool_argmax      (lowest maximising row of the SAVED net', NaN = maximum)
    G = gnet' + one-hot(arg) gpool'            ehm_pointnet_bwd_scatter      (+ its column sums: fc_1.bias grad, per-body sG)
    dh = (G W1) (.) [relu(h) > 0]              ehm_conv_nhwc_split, H = W = 1 (split_gemm.gemm_rows) + ehm_pointnet_bwd_gate (+ sums: fc_0.bias grad, sdh)
    dxa = (dh W0[:, :H]) (.) [net > 0] + G S[:, :H]          two GEMMs + ehm_pointnet_bwd_gate with `add`    -> gnet of the block before
    gpool = (sdh W0[:, H:]) (.) [pooled > 0] + sG S[:, H:]   ehm_skinny_gemm_f32: the pooled half is constant over a body, [B,H] products only
    fc_1.weight grad = G^T relu(h),  fc_0.weight grad = [dh^T relu(net) | sdh^T relu(pooled)],  shortcut.weight grad = [G^T net | sG^T pooled]
                                               ehm_pointnet_bwd_wgrad: the contraction over the rows on the exact-f32 MFMA, straight from the row-major operands
                                               (no transpose, no packing), split over runs of rows whose partial tiles are added in index order

Block 0 has no pooled half and its input is never stored: relu(net0) is recomputed from the points (ehm_pointnet_bwd_net0), shortcut.weight grad =
(G^T p) fc_pos_0.weight^T + (sum G) fc_pos_0.bias^T is a K = 3 product, and ehm_pointnet_bwd_lift turns net0bar into the gradients of fc_pos_0 and p.

As in gcn_grad, a cotangent is brought to 2^10 by a power of two computed on the device before it enters a GEMM of the split-f16 engine, and the product divided
by it again.  The weight gradients do not go through that engine: as [H, M] x [M, H] products they fill (H / 128)^2 of its tiles however long M is (measured at
B = 256, N = 4096: 38 ms each against 1 ms, docs/EXPERIMENTS.md R14.1), and both operands would have to be transposed first.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .split_gemm import gemm_rows, pack_weight, pow2_scale

# the order of the parameter gradients (ResnetPointnet.grad_parameters)
PARAM_NAMES = (("fc_pos_0.weight", "fc_pos_0.bias") +
               tuple(f"block_{b}.{n}" for b in range(4) for n in ("fc_0.weight", "fc_0.bias", "fc_1.weight", "fc_1.bias", "shortcut.weight")) +
               ("fc_c.weight", "fc_c.bias"))


def _f(t, dev):
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _weights(m, dev):
    """The module's parameters as the backward reads them (float32 on the device, data-gradient operands packed), rebuilt when one changes."""
    if m._tkey is None:
        m._tkey = _lib.TensorKey(m)
    key = m._tkey() + (str(dev),)
    if m._grad_packed is not None and m._grad_packed_key == key:
        return m._grad_packed
    H = m.hidden_dim
    Wt = {"pos_w": _f(m.fc_pos_0.weight, dev), "pos_b": _f(m.fc_pos_0.bias, dev), "fc_c": _f(m.fc_c.weight, dev)}
    for i in range(4):
        bl = getattr(m, f"block_{i}")
        W0, W1, S = _f(bl.fc_0.weight, dev), _f(bl.fc_1.weight, dev), _f(bl.shortcut.weight, dev)
        Wt[f"W1T_{i}"] = pack_weight(W1.t().contiguous())                        # T1 = G W1: the engine contracts over a packed operand's columns
        wide = 2 * H if i == 0 else H                                             # block 0: the whole input is per-point
        Wt[f"W0T_{i}"] = pack_weight(W0[:, :wide].t().contiguous())
        Wt[f"ST_{i}"] = pack_weight(S[:, :wide].t().contiguous())
        if i:
            Wt[f"W0b_{i}"], Wt[f"Sb_{i}"] = W0[:, H:].contiguous(), S[:, H:].contiguous()   # [K = out, N = in] of ehm_skinny_gemm_f32
    m._grad_packed, m._grad_packed_key = Wt, key
    return Wt


def _small(x, W):
    """[B,K] x [K,N] in exact float32 (ehm_skinny_gemm_f32)."""
    y = torch.empty(x.shape[0], W.shape[1], device=x.device)
    _lib.api().ehm_skinny_gemm_f32(x.contiguous(), W, None, y, x.shape[0], W.shape[0], W.shape[1], 0, _lib.stream_ptr())
    return y


def _small_tn(a, b):
    """a [B,m]^T b [B,n] -> [m,n] on the same kernel: the contraction over the bodies, padded to its 32 granule with zeros."""
    B = a.shape[0]
    Bp = (B + 31) // 32 * 32
    at = torch.zeros(a.shape[1], Bp, device=a.device)
    at[:, :B] = a.t()
    bp = torch.zeros(Bp, b.shape[1], device=a.device)
    bp[:B] = b
    return _small(at, bp)


def pointnet_backward(m, saved, gout, need_p=True, need=None):
    """VJP of ResnetPointnet.forward.  saved: what ResnetPointnet._forward_on_device(p, save=True) kept - p [B,N,3] float32, B, N, Np, `rh` / `net`: the four
    blocks' relu(h) and net' as X2 [B*Np, H], `pooled` [4,B,H] float32 and optionally `arg`: four int32 [B,H] (else taken from `net`); gout [B,out_dim].
    need: 24 flags in the order of PARAM_NAMES (None / empty: no parameter gradient).  Returns (pbar [B,N,3] float32 or None, list of 24 gradients, None
    where not asked for); what is not asked for is neither computed nor written."""
    A, st = _lib.api(), _lib.stream_ptr()
    dev = gout.device
    need = [False] * 24 if not need else [bool(f) for f in need]
    H, B, N, Np = m.hidden_dim, saved["B"], saved["N"], saved["Np"]
    M = B * Np
    Wt = _weights(m, dev)
    p, pooled_all = saved["p"], saved["pooled"]
    grads = [None] * 24
    geo = (B, N, Np)

    nb = C.c_int64(0)
    A.ehm_pointnet_bwd_workspace_bytes(B, Np, 2 * H, C.byref(nb))
    ws = torch.empty(nb.value // 4, device=dev)
    new = lambda *s: torch.empty(*s, device=dev)
    wb = C.c_int64(0)
    A.ehm_pointnet_bwd_wgrad_workspace_bytes(B, Np, H, 2 * H, C.byref(wb))
    wws = torch.empty(wb.value // 4, device=dev) if any(need[2:22]) else None

    def wgrad(P, Q, x2, relu, Cg, Ca, out=None):
        """out[:, :Ca] = P^T act(Q) over the valid rows (ehm_pointnet_bwd_wgrad); out: a wider [Cg, ld] matrix whose left part is written, or None"""
        out = new(Cg, Ca) if out is None else out
        A.ehm_pointnet_bwd_wgrad(P, Q, x2, relu, out, out.shape[1], *geo, Cg, Ca, wws, wb.value, st)
        return out

    def blk(i):                                                                    # flags of block i: fc_0.w, fc_0.b, fc_1.w, fc_1.b, shortcut.w
        return need[2 + 5 * i: 7 + 5 * i]

    def below(i):                                                                  # is anything in front of block i's input asked for?
        return need_p or any(need[:2 + 5 * i])

    gout = _lib.f32(gout, dev)
    # fc_c(relu(pooled_3))
    pooled = pooled_all[3]
    if need[22]:
        grads[22] = _small_tn(gout, torch.relu(pooled))
    if need[23]:
        grads[23] = gout.sum(0)
    if not (need_p or any(need[:22])):
        return None, grads
    gpool = _small(gout, Wt["fc_c"]).mul_(pooled > 0)
    gnet, gp = None, None

    for i in (3, 2, 1, 0):
        n_w0, n_b0, n_w1, n_b1, n_s = blk(i)
        down = below(i)
        if not (down or n_w0 or n_b0 or n_w1 or n_b1 or n_s):
            break
        arg = saved["arg"][i] if saved.get("arg") is not None else None
        if arg is None:
            arg = torch.empty(B, H, dtype=torch.int32, device=dev)
            A.ehm_pointnet_pool_argmax(saved["net"][i], 1, arg, *geo, H, ws, nb.value, st)
        G, sumG, sG = new(M, H), new(H), new(B, H)
        A.ehm_pointnet_bwd_scatter(gnet, gpool, arg, G, sumG, sG, *geo, H, ws, nb.value, st)
        del gnet
        if n_b1:
            grads[2 + 5 * i + 3] = sumG
        GtP3 = None
        if i == 0 and n_s:                                                         # G^T p [H,3], before G is scaled
            GtP3 = new(H, 3)
            A.ehm_pointnet_bwd_lift(G, p, None, GtP3, None, None, *geo, H, ws, nb.value, st)
        sc = pow2_scale(G)
        G.mul_(sc)
        isc = 1.0 / sc
        need_dh = down or n_w0 or n_b0
        if need_dh:
            dh, sumdh, sdh = gemm_rows(G, Wt[f"W1T_{i}"]), new(H), new(B, H)
            A.ehm_pointnet_bwd_gate(dh, saved["rh"][i], 1, None, isc, None, dh, sumdh, sdh, *geo, H, ws, nb.value, st)
            if n_b0:
                grads[2 + 5 * i + 1] = sumdh
            if down or n_w0:
                sc2 = pow2_scale(dh)
                dh.mul_(sc2)
                isc2 = 1.0 / sc2
        if i == 0:
            rnet0 = None
            if down or n_w0:
                rnet0 = new(M, 2 * H)
                A.ehm_pointnet_bwd_net0(p, Wt["pos_w"], Wt["pos_b"], None, rnet0, *geo, 2 * H, st)
        # ---- data gradients
        nxt_gnet = nxt_gpool = None
        if down:
            T2, T3 = gemm_rows(dh, Wt[f"W0T_{i}"]), gemm_rows(G, Wt[f"ST_{i}"])
            if i:
                A.ehm_pointnet_bwd_gate(T2, saved["net"][i - 1], 1, T3, isc2, isc, T2, None, None, *geo, H, None, 0, st)
                nxt_gnet = T2
                pin = pooled_all[i - 1]
                nxt_gpool = _small(sdh, Wt[f"W0b_{i}"]).mul_(pin > 0).add_(_small(sG, Wt[f"Sb_{i}"]))
            else:
                A.ehm_pointnet_bwd_gate(T2, rnet0, 0, T3, isc2, isc, T2, None, None, *geo, 2 * H, None, 0, st)
                gW = new(2 * H, 3) if need[0] else None
                gb = new(2 * H) if need[1] else None
                gp = new(B, N, 3) if need_p else None
                A.ehm_pointnet_bwd_lift(T2, p, Wt["pos_w"], gW, gb, gp, *geo, 2 * H, ws, nb.value, st)
                grads[0], grads[1] = gW, gb
            del T2, T3
        # ---- weight gradients: the contraction runs over the rows (G / dh still carry their power of two: taken out of the small result)
        if n_w1:
            grads[2 + 5 * i + 2] = wgrad(G, saved["rh"][i], 1, 0, H, H).mul_(isc)
        if i:
            pin = pooled_all[i - 1]
            if n_s:
                gS = new(H, 2 * H)
                wgrad(G, saved["net"][i - 1], 1, 0, H, H, gS)
                gS[:, :H].mul_(isc)
                gS[:, H:] = _small_tn(sG, pin)
                grads[2 + 5 * i + 4] = gS
            if n_w0:
                gW0 = new(H, 2 * H)
                wgrad(dh, saved["net"][i - 1], 1, 1, H, H, gW0)
                gW0[:, :H].mul_(isc2)
                gW0[:, H:] = _small_tn(sdh, torch.relu(pin))
                grads[2 + 5 * i] = gW0
        else:
            if n_s:                                                                # G^T net0 = (G^T p) W^T + (sum G) b^T
                grads[6] = torch.addmm(torch.outer(sumG, Wt["pos_b"]), GtP3, Wt["pos_w"].t())
            if n_w0:
                grads[2] = wgrad(dh, rnet0, 0, 0, H, 2 * H).mul_(isc2)
        gnet, gpool = nxt_gnet, nxt_gpool
    return gp, grads


class PointnetFunction(torch.autograd.Function):
    """ResnetPointnet.forward (respointnet.py:33-59) with a backward: forward(module, p, *params) -> [B,out_dim].  `params` is empty (gradient to p only)
    or ResnetPointnet.grad_parameters(), the 24 parameters in the order of PARAM_NAMES."""

    @staticmethod
    def forward(ctx, module, p, *params):
        with _lib.on_device(p.device):
            out, saved = module._forward_on_device(p, save=True)
        saved["p_dtype"] = p.dtype
        ctx.module, ctx.saved, ctx.n_params = module, saved, len(params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        need = ctx.needs_input_grad
        with _lib.on_device(gout.device):
            gp, grads = pointnet_backward(ctx.module, ctx.saved, gout, need[1], need[2:])
        if gp is not None:
            gp = gp.to(ctx.saved["p_dtype"])
        return (None, gp, *grads[:ctx.n_params])
