"""Backward of the stage-1 Glow flow on libegohmr_hip (csrc/flow.hip), and the ``torch.autograd.Function`` that GlowFlow.log_prob and
GlowFlow.sample_and_log_prob run behind when a gradient is asked for (stage1.py).  The definition is tests/flow_ref.py; tests/flow_grad_ref.py
restates it in torch, and float64 autograd of that is the reference of the tests.

One coupling, s the state after it, ds its cotangent, sg = +1 (x -> z) / -1 (sampling); the walk carries dt' = sg dt and puts the sign where a
result leaves it (a negation is exact), so the data path needs no signed copy of ds[:, trf]:

    dt'_2 = ds[:, trf] Wf^T                                   ehm_flow_gemm, gather = transform_features, W = final_layer.weight ([out, in] = [K, N])
    dWf = sg ds[:, trf]^T t_2,  dbf = sg sum_r ds[:, trf]     ehm_flow_wgrad (gather on G), ehm_flow_reduce COLS
    k = 1, 0:
      dPg_k[i] = sg sum_{r in i} dt' u2 s (1 - s)             ehm_flow_reduce GATE, straight into its 1024 columns of dP [B, 12 * 1024]
      dWb_k = sg (dt' s)^T relu(u1),  dbb_k                   ehm_flow_wgrad / _reduce with the per-item gate on G
      du1' = ((dt' s) Wb_k^T) [u1 > 0]                        ehm_flow_gemm, PRO_GATE, EPI_MASK
      dWa_k = sg du1'^T relu(t_k),  dba_k                     ehm_flow_wgrad (ReLU on X), ehm_flow_reduce COLS
      dt' <- dt' + (du1' Wa_k^T) [t_k > 0]                    ehm_flow_gemm, EPI_MASK_ADD in place
    dP0[i] = sg sum_{r in i} dt'                              ehm_flow_reduce ITEM
    dWx = sg dt'^T s[:, idf]                                  ehm_flow_wgrad (gather on X) into columns 0 .. 71 of initial_layer.weight's gradient
    ds[:, idf] += sg dt' Wx^T                                 ehm_flow_gemm, scatter = identity_features, EPI_SCATTER_ADD / _SUB; W = the first 72
                                                              columns of initial_layer.weight [1024, 72 + ctx], read in place (ldw = 72 + ctx)

and once per call: dWctx (twelve ehm_flow_wgrad over the B rows of dP and the context, each into the context columns of its weight's gradient),
dbctx (one COLS reduction), dctx = dP Wctx^T (twelve ehm_flow_gemm over the context columns of the torch weights, summed in slot order by EPI_ADD).
The affine maps: ds_in = ds_out A, dA = ds_out^T s_in, dc = sum_r ds_out; sampling, x = (s - c) Ainv^T: ds = dx Ainv, dAinv = dx^T (s - c) (x_shift),
dc = -sum_r ds.  (dA, dc, dAinv, dlogdet) reach the six ActNorm / LULinear parameters through torch autograd of `fold`, float64 on the host.

Nothing here uses atomics and every sum has a fixed order: two backward calls on the same inputs give the same bits.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .synthetic import FLOW_DEPTH, FLOW_DIM, FLOW_LAYERS

_HALF, _H = FLOW_DIM // 2, 1024
_AFFINE = ("log_scale", "shift", "lower_entries", "upper_entries", "unconstrained_upper_diag", "bias")


# --------------------------------------------------------------------------------------------- the fold, differentiable
def fold(log_scale, shift, lower_entries, upper_entries, unconstrained_upper_diag, bias):
    """GlowFlow.fold as a torch function of the six parameters (float64, CPU): (A, c, Ainv, logdet), s <- s A^T + c.  A = L U diag(exp(log_scale)),
    c = L U shift + bias, Ainv = diag(exp(-log_scale)) U^-1 L^-1 by two triangular solves, logdet = sum(log_scale) + sum(log diag U)."""
    D = FLOW_DIM
    dt = log_scale.dtype
    il, iu = torch.tril_indices(D, D, -1), torch.triu_indices(D, D, 1)
    diag = torch.log1p(torch.exp(unconstrained_upper_diag)) + 1e-3
    Lm = torch.eye(D, dtype=dt).index_put((il[0], il[1]), lower_entries)
    U = torch.zeros(D, D, dtype=dt).index_put((iu[0], iu[1]), upper_entries) + torch.diag(diag)
    LU = Lm @ U
    A, c = LU * torch.exp(log_scale)[None, :], LU @ shift + bias
    eye = torch.eye(D, dtype=dt)
    Linv = torch.linalg.solve_triangular(Lm, eye, upper=False)
    Ainv = torch.exp(-log_scale)[:, None] * torch.linalg.solve_triangular(U, Linv, upper=True)
    logdet = log_scale.sum() + torch.log(diag).sum()
    # GlowFlow.logdet is numpy's sum, and two float64 sums of 144 terms in different orders may differ in the last bit: the value is moved onto
    # numpy's (the difference of two such neighbours is exact, and so is adding it), the gradient stays this graph's
    d64 = lambda t: t.detach().double().numpy()
    want = float(d64(log_scale).sum() + np.log(np.log1p(np.exp(d64(unconstrained_upper_diag))) + 1e-3).sum())
    return A, c, Ainv, logdet + (want - float(logdet.detach()))


# --------------------------------------------------------------------------------------------- route selection
def wants_grad(module, *tensors) -> bool:
    """The autograd route is taken when grad mode is on and an input requires grad, or `grad_params` is set and a parameter does."""
    if not torch.is_grad_enabled():
        return False
    if any(t is not None and t.requires_grad for t in tensors):
        return True
    return bool(module.grad_params) and any(p.requires_grad for p in module.parameters())


def run_with_grad(m, ctx, rows, num_samples, sampling):
    """GlowFlow.sample_and_log_prob / log_prob behind FlowSampleFunction / FlowFunction.  ctx: [B, ctx_dim], or the padded row [B, ctx_pad]."""
    if m.batch_norm:
        raise _lib.EgoHMRHipError("GlowFlow: the BatchNorm of the flow's ResidualNet is not differentiated (batch_norm=True runs without a graph only; "
                                  "nflows' ConditionalGlow as models/prohmr/smpl_flow.py builds it has none)")
    params = list(m.parameters()) if m.grad_params else []
    if not sampling:
        return FlowFunction.apply(m, rows, ctx, *params)
    if rows is None:
        if num_samples is None or int(num_samples) < 1:
            raise ValueError("sample_and_log_prob needs z or num_samples >= 1")
        rows = torch.randn(ctx.shape[0] * int(num_samples), FLOW_DIM, device=ctx.device).reshape(ctx.shape[0], int(num_samples), FLOW_DIM)
    p6, lp, go, bp = FlowSampleFunction.apply(m, rows, ctx, *params)
    return {"pred_pose_6d": p6, "log_prob": lp, "z": rows, "global_orient": go, "body_pose": bp}


# --------------------------------------------------------------------------------------------- launches
def _wgrad(st, G, X, out, R, Cg, Ca, ldg, ldx, ld_out, S=1, gather_g=None, gather_x=None, item=None, ld_item=0, x_shift=None, relu=False, alpha=1.0):
    P = lambda t: t if isinstance(t, int) else _lib.ptr(t)
    d = _lib.FlowWgradDesc(G=P(G), gather_g=P(gather_g), item=item, X=P(X), gather_x=P(gather_x), x_shift=P(x_shift), out=P(out), R=R, Cg=Cg, Ca=Ca,
                           S=S, ldg=ldg, ldx=ldx, ld_item=ld_item, ld_out=ld_out, act=_lib.FLOW_ACT_RELU if relu else _lib.FLOW_ACT_NONE,
                           alpha=alpha, beta=0.0)
    _lib.api().ehm_flow_wgrad(C.byref(d), st)


def _reduce(st, mode, G, out, R, N, ldg, S=1, gather=None, U2=None, ldu=0, item=None, ld_item=0, ld_out=0, scale=1.0):
    P = lambda t: t if isinstance(t, int) else _lib.ptr(t)
    d = _lib.FlowReduceDesc(G=P(G), gather=P(gather), U2=P(U2), item=item, out=P(out), R=R, N=N, S=S, ldg=ldg, ldu=ldu, ld_item=ld_item,
                            ld_out=ld_out, mode=mode, scale=scale)
    _lib.api().ehm_flow_reduce(C.byref(d), st)


def _fold_backward(m, l, dA, dc, dAinv, dlogdet):
    """The cotangents of block l's (A, c, Ainv, logdet) -> those of its six parameters, by torch autograd of `fold` (float64, host).  A cotangent that
    is None is a zero."""
    tr = m._transform._transforms
    src = [getattr(tr[3 * l], n) for n in _AFFINE[:2]] + [getattr(tr[3 * l + 1], n) for n in _AFFINE[2:]]
    with torch.enable_grad():
        leaves = [p.detach().double().cpu().requires_grad_(True) for p in src]
        outs, cots = [], []
        for o, g in zip(fold(*leaves), (dA, dc, dAinv, dlogdet)):
            if g is not None:
                outs.append(o)
                cots.append(g.detach().double().cpu().reshape(o.shape))
        grads = torch.autograd.grad(outs, leaves, cots, allow_unused=True)
    return [torch.zeros_like(p) if g is None else g.to(device=p.device, dtype=p.dtype) for g, p in zip(grads, src)]


def flow_backward(m, keep, sampling, gout, need_rows, need_ctx, need_w, need_affine):
    """VJP of one direction.  keep: what GlowFlow._run(keep=...) kept; gout: the cotangents of the outputs, each may be None - (log_prob [R], z [R,144])
    or (pred_pose_6d [R,144], log_prob [R], global_orient, body_pose).  need_w: the gradients of the coupling nets' parameters, need_affine: those
    of the ActNorm / LULinear parameters.  Returns (drows [R,144] | None, dctx [B, ctx_dim] | None, {parameter name: gradient}); what is not asked
    for is neither computed nor launched."""
    A, st = _lib.api(), _lib.stream_ptr()
    w, Pm, S, rows, ctxp = keep["w"], keep["P"], keep["S"], keep["rows"], keep["ctxp"]
    dev = rows.device
    R, D, H, B, ctx = rows.shape[0], FLOW_DIM, _H, ctxp.shape[0], m.ctx_dim
    ldp, ld0 = Pm.shape[1], _HALF + m.ctx_dim
    new = lambda *s: torch.empty(*s, device=dev)
    f = lambda t: None if t is None else _lib.f32(t, dev).reshape(R, -1)
    gemm = m._gemm
    item = lambda slot: Pm.data_ptr() + 4 * H * slot
    need_P = need_ctx or need_w
    grads = {}
    pre = "_transform._transforms."
    dP = new(B, ldp) if need_P else None
    dcol = lambda slot: dP.data_ptr() + 4 * H * slot

    # ---- the finish: the cotangent of the chain's output rows, and of its log|det|
    dsum = None
    if sampling:
        g6, glp, ggo, gbp = (f(g) for g in gout)
        ds = new(R, D)
        if g6 is None and ggo is None and gbp is None:
            ds.zero_()
        else:
            A.ehm_flow_finish_backward(None, None, None, None, None, keep["x"], g6, ggo, gbp, ds, R, st)
    else:
        glp, gz = (f(g) for g in gout)
        ds = new(R, D)
        if glp is None and gz is None:
            ds.zero_()
        else:
            A.ehm_flow_finish_backward(glp, keep["z"], gz, ds, None, None, None, None, None, None, R, st)
    if glp is not None and need_affine:
        dsum = new(1)
        A.ehm_flow_finish_backward(glp, None, None, None, dsum, None, None, None, None, None, R, st)

    def coupling(l, ds, down):
        """the coupling of block l, in place on ds (rows of the state after it); down: is ds[:, idf] still read afterwards?"""
        wl, kp = w["blocks"][l], keep["blocks"][l]
        sg = -1.0 if sampling else 1.0
        s_id = keep["states"][l] if sampling else keep["states"][l + 1]           # (a coupling leaves s[:, idf] alone)
        net = f"{pre}{3 * l + 2}.transform_net."
        dT = new(R, H)
        gemm(st, ds, wl["Wf_oi"], dT, R, _HALF, H, D, H, H, gather=wl["trf"])
        if need_w:
            grads[net + "final_layer.weight"], grads[net + "final_layer.bias"] = new(_HALF, H), new(_HALF)
            _wgrad(st, ds, kp["t"][2], grads[net + "final_layer.weight"], R, _HALF, H, D, H, H, gather_g=wl["trf"], alpha=sg)
            _reduce(st, _lib.FLOW_RED_COLS, ds, grads[net + "final_layer.bias"], R, _HALF, D, gather=wl["trf"], scale=sg)
        dU = new(R, H)
        for k in reversed(range(FLOW_DEPTH)):
            e0, e1 = wl["lin"][2 * k], wl["lin"][2 * k + 1]
            gate = item(3 * l + 1 + k)
            blk = f"{net}blocks.{k}."
            if need_P:
                _reduce(st, _lib.FLOW_RED_GATE, dT, dcol(3 * l + 1 + k), R, H, H, S=S, U2=kp["u2"][k], ldu=H, item=gate, ld_item=ldp, ld_out=ldp, scale=sg)
            if need_w:
                gW, gb = new(H, H), new(H)
                _wgrad(st, dT, kp["u1"][k], gW, R, H, H, H, H, H, S=S, item=gate, ld_item=ldp, relu=True, alpha=sg)
                _reduce(st, _lib.FLOW_RED_COLS, dT, gb, R, H, H, S=S, item=gate, ld_item=ldp, scale=sg)
                grads[blk + "linear_layers.1.weight"], grads[blk + "linear_layers.1.bias"] = gW, gb
            gemm(st, dT, e1["W"], dU, R, H, H, H, H, H, S=S, pro=_lib.FLOW_PRO_GATE, item=gate, ld_item=ldp, epi=_lib.FLOW_EPI_MASK,
                 mask=kp["u1"][k], ld_mask=H)
            if need_w:
                gW, gb = new(H, H), new(H)
                _wgrad(st, dU, kp["t"][k], gW, R, H, H, H, H, H, relu=True, alpha=sg)
                _reduce(st, _lib.FLOW_RED_COLS, dU, gb, R, H, H, scale=sg)
                grads[blk + "linear_layers.0.weight"], grads[blk + "linear_layers.0.bias"] = gW, gb
            gemm(st, dU, e0["W"], dT, R, H, H, H, H, H, epi=_lib.FLOW_EPI_MASK_ADD, mask=kp["t"][k], ld_mask=H, add=dT, ld_add=H)
        if need_P:
            _reduce(st, _lib.FLOW_RED_ITEM, dT, dcol(3 * l), R, H, H, S=S, ld_out=ldp, scale=sg)
        if need_w:
            gW0 = new(H, ld0)
            _wgrad(st, dT, s_id, gW0, R, H, _HALF, H, D, ld0, gather_x=wl["idf"], alpha=sg)
            grads[net + "initial_layer.weight"] = gW0
        if down:
            gemm(st, dT, wl["W0"], ds, R, H, _HALF, H, ld0, D, scatter=wl["idf"], w_window=1,
                 epi=_lib.FLOW_EPI_SCATTER_SUB if sampling else _lib.FLOW_EPI_SCATTER_ADD)

    aff = {}
    other = new(R, D)
    if sampling:                                   # forward order: l = 3 .. 0, coupling then (s - c) Ainv^T; backward: l = 0 .. 3, the map first
        for l in range(FLOW_LAYERS):
            wl, s = w["blocks"][l], keep["states"][l]
            last = l == FLOW_LAYERS - 1
            if need_affine:
                aff[l] = dict(dAinv=new(D, D), dc=new(D))
                _wgrad(st, ds, s, aff[l]["dAinv"], R, D, D, D, D, D, x_shift=wl["c"])
            gemm(st, ds, wl["Ainv"], other, R, D, D, D, D, D, w_window=1)
            ds, other = other, ds
            if need_affine:
                _reduce(st, _lib.FLOW_RED_COLS, ds, aff[l]["dc"], R, D, D, scale=-1.0)
            if need_rows or need_P or need_w or not last:
                coupling(l, ds, down=need_rows or not last)
    else:                                          # forward order: l = 0 .. 3, s A^T + c then the coupling; backward: l = 3 .. 0, the coupling first
        for l in reversed(range(FLOW_LAYERS)):
            wl = w["blocks"][l]
            last = l == 0
            coupling(l, ds, down=need_rows or need_affine or not last)
            if need_affine:
                aff[l] = dict(dA=new(D, D), dc=new(D))
                _wgrad(st, ds, keep["states"][l], aff[l]["dA"], R, D, D, D, D, D)
                _reduce(st, _lib.FLOW_RED_COLS, ds, aff[l]["dc"], R, D, D)
            if need_rows or not last:
                gemm(st, ds, wl["A"], other, R, D, D, D, D, D, w_window=1)
                ds, other = other, ds
    drows = None
    if need_rows:
        drows = ds
        if sampling and glp is not None:           # the noise also enters log_prob: -1/2 ||z||^2
            drows = new(R, D)
            A.ehm_flow_finish_backward(glp, rows, ds, drows, None, None, None, None, None, None, R, st)

    # ---- the per-item terms: P = ctx_pad Wctx + bctx, twelve slots of 1024 columns
    dctx = None
    if need_P:
        tr = m._transform._transforms
        slots = []                                 # (name of the weight, its float32 tensor, the column its context part starts at)
        for l in range(FLOW_LAYERS):
            wl = w["blocks"][l]
            net = f"{pre}{3 * l + 2}.transform_net."
            slots.append((net + "initial_layer", wl["W0"], _HALF))
            slots += [(f"{net}blocks.{k}.context_layer", wl["Wc"][k], 0) for k in range(FLOW_DEPTH)]
        if need_w:
            db = new(ldp)
            _reduce(st, _lib.FLOW_RED_COLS, dP, db, B, ldp, ldp)
            for i, (name, W, c0) in enumerate(slots):
                if c0 == 0:
                    grads[name + ".weight"] = new(H, ctx)
                gW = grads[name + ".weight"]
                _wgrad(st, dcol(i), ctxp, gW.data_ptr() + 4 * c0, B, H, ctx, ldp, ctxp.shape[1], gW.shape[1])
                grads[name + ".bias"] = db[i * H:(i + 1) * H]
        if need_ctx:
            dctx = new(B, ctx)
            for i, (name, W, c0) in enumerate(slots):
                gemm(st, dcol(i), W.data_ptr() + 4 * c0, dctx, B, H, ctx, ldp, W.shape[1], ctx, epi=_lib.FLOW_EPI_ADD if i else _lib.FLOW_EPI_BIAS,
                     add=dctx if i else None, ld_add=ctx if i else 0, w_window=1)
    if need_affine:
        for l in range(FLOW_LAYERS):
            g = _fold_backward(m, l, aff[l].get("dA"), aff[l]["dc"], aff[l].get("dAinv"), dsum)
            for n, v in zip(_AFFINE, g):
                grads[f"{pre}{3 * l if n in _AFFINE[:2] else 3 * l + 1}.{n}"] = v
    return drows, dctx, grads


# --------------------------------------------------------------------------------------------- autograd
def _forward(ctx_, sampling, module, rows, c, params):
    keep = {}
    padded = c.dim() == 2 and c.shape[1] == module.ctx_pad != module.ctx_dim
    with _lib.on_device(rows.device):
        if sampling:
            o = module._sample_and_log_prob(None if padded else c, None, rows, c if padded else None, keep=keep)
            out = (o["pred_pose_6d"], o["log_prob"], o["global_orient"], o["body_pose"])
        else:
            lp, z = module._log_prob(rows, None if padded else c, c if padded else None, keep=keep)
            out = (lp, z.clone())                                  # (z's buffer is the last kept state: the caller gets its own)
    ctx_.module, ctx_.keep, ctx_.sampling, ctx_.padded = module, keep, sampling, padded
    ctx_.names = [n for n, _ in module.named_parameters()][:len(params)]
    ctx_.dtypes = (rows.dtype, c.dtype)
    ctx_.weights_key = module._key                                 # (data_ptr, _version) of every parameter and buffer as this forward read them
    ctx_.set_materialize_grads(False)
    return out


def _backward(ctx_, gout):
    m, keep = ctx_.module, ctx_.keep
    # The kept activations belong to the weights of the forward, and the backward reads the live float32 parameters themselves (no copy): a
    # parameter changed in between (an optimizer step before .backward()) would mix two weight versions, and autograd's own version check does
    # not see tensors kept outside save_for_backward.
    if m._key_fn() + (str(keep["rows"].device),) != ctx_.weights_key:
        raise _lib.EgoHMRHipError("GlowFlow: a parameter or buffer of the flow was modified (or moved) between a forward and its backward; the kept "
                                  "activations belong to the weights of the forward - run the backward before the optimizer's step")
    need = ctx_.needs_input_grad                                   # (module, rows, ctx, *params)
    wanted = {n for n, f in zip(ctx_.names, need[3:]) if f}
    need_affine = any(n.rsplit(".", 1)[1] in _AFFINE and ".transform_net." not in n for n in wanted)
    need_w = any(".transform_net." in n for n in wanted)
    with _lib.on_device(keep["rows"].device):
        drows, dctx, grads = flow_backward(m, keep, ctx_.sampling, gout, need[1], need[2], need_w, need_affine)
    if drows is not None:
        drows = drows.reshape(-1, keep["S"], FLOW_DIM).to(ctx_.dtypes[0])
    if dctx is not None:
        if ctx_.padded:
            dctx = torch.cat([dctx, dctx.new_zeros(dctx.shape[0], m.ctx_pad - m.ctx_dim)], 1)
        dctx = dctx.to(ctx_.dtypes[1])
    return (None, drows, dctx, *[grads.get(n) if n in wanted else None for n in ctx_.names])


class FlowFunction(torch.autograd.Function):
    """GlowFlow.log_prob with a backward: apply(module, x [B,S,144], ctx, *params) -> (log_prob [B,S], z [B,S,144]).  `params` is empty (gradients
    to x and ctx only) or list(module.parameters()); one gradient per parameter comes back, in torch layout (buffers get none)."""

    @staticmethod
    def forward(ctx_, module, rows, c, *params):
        return _forward(ctx_, False, module, rows, c, params)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx_, *gout):
        return _backward(ctx_, gout)


class FlowSampleFunction(torch.autograd.Function):
    """GlowFlow.sample_and_log_prob with a backward: apply(module, z [B,S,144], ctx, *params) -> (pred_pose_6d, log_prob, global_orient, body_pose)."""

    @staticmethod
    def forward(ctx_, module, rows, c, *params):
        return _forward(ctx_, True, module, rows, c, params)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx_, *gout):
        return _backward(ctx_, gout)
