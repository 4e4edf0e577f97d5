"""Backward of EgoHMR.compute_loss's total on libegohmr_hip (csrc/loss.hip: ehm_val_losses_backward), and the ``torch.autograd.Function``s that
compute_loss runs behind when a gradient is asked for (model.py).

    ValLossesFunction      ehm_val_losses forward, ehm_val_losses_backward as its VJP w.r.t. the eight prediction arrays and the penetration term
    ProxyPenetration       the build's collision proxy as the penetration term [B] of the bodies' vertices (ehm_scene_cap_points + ehm_collision_query, or
                           ehm_mesh_collision_query under EgoHMR.collision_proxy = 'mesh');
                           the bounding box and the point cap carry no gradient, as the reference detaches them (egohmr.py:406-407)

First derivatives only (``once_differentiable``).  No host synchronisation.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

PREDICTIONS = _lib.ValLossesBwdDesc.PREDICTIONS


def f32_graph(t, dev):
    """_lib.f32 without the detach: contiguous float32 on the device, still in the autograd graph."""
    return t.to(device=dev, dtype=torch.float32).contiguous()


def val_losses_grad_native(t, weights, gloss=None, want=PREDICTIONS + ("penetration",), out=None) -> dict:
    """ehm_val_losses_backward on the dict of contiguous device tensors val_losses_native takes.  gloss: device scalar (None = 1); want: the names whose
    gradient is computed (of PREDICTIONS and 'penetration'); out: preallocated tensors by name.  -> {name: gradient, shaped like t[name]; penetration [B]}."""
    pv = t["pred_vertices"]
    dev, P, A = pv.device, _lib.ptr, _lib.api()
    B, V = pv.shape[0], pv.shape[1]
    out = {} if out is None else out
    g = {k: out[k] if out.get(k) is not None else (torch.empty(B, device=dev) if k == "penetration" else torch.empty_like(t[k])) for k in want}
    with _lib.on_device(dev):
        nb = C.c_int64(0)
        A.ehm_val_losses_backward_workspace_bytes(B, V, C.byref(nb))
        ws = torch.empty(max(nb.value // 4, 1), device=dev, dtype=torch.int32)
        d = _lib.ValLossesBwdDesc(B=B, V=V, pred_joints=t["pred_keypoints_3d"].shape[1], gt_joints=t["gt_joints_male"].shape[1],
                                  kp3d_points=t["keypoints_3d"].shape[1], kp3d_full_points=t["keypoints_3d_full"].shape[1],
                                  kp2d_points=t["keypoints_2d"].shape[1], gloss=P(gloss), weights=(C.c_double * 9)(*[float(w) for w in weights]),
                                  workspace=P(ws), workspace_bytes=nb.value, **{k: P(t[k]) for k in _lib.ValLossesBwdDesc.INPUTS},
                                  **{"g_" + k: P(v) for k, v in g.items()})
        A.ehm_val_losses_backward(C.byref(d), _lib.stream_ptr())
    return g


class ValLossesFunction(torch.autograd.Function):
    """forward(consts, weights, penetration or None, *the eight prediction arrays in PREDICTIONS' order) -> (total, losses [11], joint_vis_num [1],
    per_item [B,11], per_item_vis [B], vis_mask [B,24]); only `total` is differentiable.  `consts`: the ground-truth entries of EgoHMR.loss_inputs."""

    @staticmethod
    def forward(ctx, consts, weights, penetration, *preds):
        from .model import val_losses_native
        t = dict(consts)
        t.update({k: p.detach() for k, p in zip(PREDICTIONS, preds)})
        res = val_losses_native(t, weights, None if penetration is None else penetration.detach())
        ctx.t, ctx.weights = t, list(weights)
        outs = (res["losses"][0].clone(), res["losses"], res["joint_vis_num"], res["per_item"], res["per_item_vis"], res["vis_mask"])
        ctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gloss, *_):
        need = ctx.needs_input_grad                 # (consts, weights, penetration, *preds)
        want = tuple(k for k, n in zip(PREDICTIONS, need[3:]) if n) + (("penetration",) if need[2] else ())
        if not want:
            return (None,) * len(need)
        dev = ctx.t["pred_vertices"].device
        g = val_losses_grad_native(ctx.t, ctx.weights, _lib.f32(gloss, dev).reshape(1), want)
        return (None, None, g.get("penetration"), *[g.get(k) for k in PREDICTIONS])


class ProxyPenetration(torch.autograd.Function):
    """forward(model, vertices [B,V,3]) -> the proxy's penetration term [B] (EgoHMR._penetration_term_proxy); backward: g[:, None, None] * d term / d vertices."""

    @staticmethod
    def forward(ctx, model, verts):
        term, gverts = model._penetration_term_proxy(verts.detach(), want_grad=True)
        ctx.save_for_backward(gverts)
        return term

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (gverts,) = ctx.saved_tensors
        return None, g[:, None, None] * gverts
