"""The denoiser's input feature on the training route of EgoHMR.forward (csrc/train.hip) and the ``torch.autograd.Function`` around it.

The reference assembles X [B, 24, in_dim] = [ img (visibility-masked) | scene + transl + cam | x_t embedding | timestep embedding ] from about ten
repeat / cat / mask ops (models/egohmr/egohmr.py:190-191, :220-236, mask_cond :150-169) and its autograd reduces the [B, 24, in_dim] cotangent back over
the joints; here either direction is one launch (ehm_cond_assemble / ehm_cond_assemble_backward).
"""
from __future__ import annotations

import torch

from . import _lib


def cond_assemble_native(img_feats, vis, drop, other, n_other, x_feat, temb, only_mask_img) -> torch.Tensor:
    """ehm_cond_assemble on contiguous device tensors: img_feats [B,img] float32, vis [B,24] uint8, drop [B] uint8 or None, other [B,ld >= n_other]
    float32, x_feat [24 B,E], temb [B,E] -> X [B,24,img + n_other + 2 E].  No host synchronisation."""
    B, img, E = img_feats.shape[0], img_feats.shape[1], temb.shape[1]
    if (vis.shape != (B, 24) or vis.dtype != torch.uint8 or other.dim() != 2 or other.shape[0] != B or other.shape[1] < n_other
            or x_feat.shape != (B * 24, E) or temb.shape[0] != B or (drop is not None and (drop.shape != (B,) or drop.dtype != torch.uint8))):
        raise ValueError("cond_assemble: the operands do not describe the same B items")
    X = torch.empty(B, 24, img + n_other + 2 * E, device=img_feats.device)
    _lib.api().ehm_cond_assemble(img_feats, vis, drop, other, other.shape[1], n_other, x_feat, temb, int(bool(only_mask_img)), X, B, img, E,
                                 _lib.stream_ptr())
    return X


def cond_assemble_backward_native(gX, vis, drop, n_other, only_mask_img, img, E, want=(True, True, True, True), out=None) -> list:
    """ehm_cond_assemble_backward: gX [B,24,D] -> [g_img [B,img], g_other [B,n_other], g_x_feat [24 B,E], g_temb [B,E]], None where `want` is False
    (neither computed nor read).  out: the four tensors to write into (tests), else fresh ones."""
    B, dev = gX.shape[0], gX.device
    if gX.shape != (B, 24, img + n_other + 2 * E):
        raise ValueError(f"cond_assemble_backward: expected a cotangent [B, 24, {img + n_other + 2 * E}], got {tuple(gX.shape)}")
    shapes = ((B, img), (B, n_other), (B * 24, E), (B, E))
    g = [None if not w else (out[i] if out is not None else torch.empty(*s, device=dev)) for i, (w, s) in enumerate(zip(want, shapes))]
    _lib.api().ehm_cond_assemble_backward(gX, vis, drop, n_other, int(bool(only_mask_img)), *g, B, img, E, _lib.stream_ptr())
    return g


class CondAssemble(torch.autograd.Function):
    """forward(img_feats [B,img], vis [B,24] uint8, drop [B] uint8 or None, other [B,n_other], x_feat [24 B,E], temb [B,E], only_mask_img) -> X [B,24,D].
    Gradients to img_feats, other, x_feat and temb, each only where asked for: with the image trunk frozen the img columns of the cotangent are never
    read.  First derivatives only; launches on the current device's stream."""

    @staticmethod
    def forward(ctx, img_feats, vis, drop, other, x_feat, temb, only_mask_img):
        dev = img_feats.device
        f = lambda t: _lib.f32(t, dev)
        other = f(other)
        with _lib.on_device(dev):
            X = cond_assemble_native(f(img_feats), vis, drop, other, other.shape[1], f(x_feat), f(temb), only_mask_img)
        ctx.vis, ctx.drop, ctx.only_mask_img = vis, drop, bool(only_mask_img)
        ctx.dims = (img_feats.shape[1], other.shape[1], temb.shape[1])
        ctx.dtypes = (img_feats.dtype, other.dtype, x_feat.dtype, temb.dtype)
        return X

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gX):
        need = ctx.needs_input_grad
        img, n_other, E = ctx.dims
        with _lib.on_device(gX.device):
            g = cond_assemble_backward_native(_lib.f32(gX, gX.device), ctx.vis, ctx.drop, n_other, ctx.only_mask_img, img, E,
                                              want=(need[0], need[3], need[4], need[5]))
        g = [t if t is None else t.to(d) for t, d in zip(g, ctx.dtypes)]
        return g[0], None, None, g[1], g[2], g[3], None
