"""Float64 torch restatement of the reference's evaluation-branch EgoHMR.compute_loss (models/egohmr/egohmr.py:307-449, models/egohmr/losses.py) as whole-tensor
expressions on the CPU, written from the reference text - nothing of csrc/loss.hip's block / slab / wave structure - so that torch.autograd gives the
gradient reference of ehm_val_losses_backward.  The L1 arguments are formed in the reference's (= the forward kernel's) expression order:
(pred - pred pelvis) - (gt - gt pelvis).  Not collected by pytest."""
from __future__ import annotations

import numpy as np
import torch

from val_losses_ref import LOSS_KEYS, SMPL_TO_OPENPOSE

PREDICTIONS = ("pred_vertices", "pred_keypoints_3d", "pred_keypoints_3d_full", "pred_keypoints_2d_full", "pred_global_orient", "pred_body_pose",
               "pred_betas", "pred_pose_6d")


def as_f64(inp: dict, requires_grad=()) -> dict:
    """numpy / torch arrays -> float64 CPU tensors ('gender' stays int64); the names in `requires_grad` become leaves."""
    out = {}
    for k, v in inp.items():
        t = torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v))
        out[k] = t.long() if k == "gender" else t.double().clone().requires_grad_(k in requires_grad)
    return out


def val_losses_torch64(inp: dict, weights, penetration=None) -> dict:
    """inp: float64 CPU tensors named like the fields of ehm_val_losses_desc (as_f64); weights: the nine of egohmr.py:422-430; penetration: [B] tensor or
    None.  -> {key: 0-d float64 tensor} for the eleven keys of the reference's `losses` dict, `loss` with the graph of every input that requires grad."""
    f = inp
    B = f["pred_vertices"].shape[0]
    fem = f["gender"] == 1
    # ---- :314-331, losses.py:20-25
    pred2d = f["pred_keypoints_2d_full"][:, SMPL_TO_OPENPOSE, :]
    gt2d = f["keypoints_2d"][:, :25]
    conf = gt2d[:, :, -1].unsqueeze(-1).clone()
    conf[:, [1, 9, 12], :] = 0
    kp2d = (conf * (pred2d - gt2d[:, :, :-1]).abs()).sum(dim=(1, 2)).mean()
    # ---- :334-341, losses.py:44-50
    p3, g3 = f["pred_keypoints_3d"][:, 0:24], f["keypoints_3d"][:, 0:24]
    p3a, g3a = p3 - p3[:, [0], :], g3 - g3[:, [0], :]
    kp3d = (p3a - g3a).abs().sum(dim=(1, 2)).mean()
    kp3d_full = (f["pred_keypoints_3d_full"][:, 0:24] - f["keypoints_3d_full"][:, 0:24]).abs().sum(dim=(1, 2)).mean()
    # ---- :344-355
    gt_v = torch.where(fem[:, None, None], f["gt_vertices_female"], f["gt_vertices_male"])
    gt_j = torch.where(fem[:, None, None], f["gt_joints_female"], f["gt_joints_male"])
    v2v = ((f["pred_vertices"] - p3[:, [0], :]) - (gt_v - gt_j[:, [0], :])).abs().mean()
    # ---- :358-372 (evaluation branch; not part of the total)
    with torch.no_grad():
        q = gt_j[:, :24] / gt_j[:, :24, 2:3]
        u = f["focal"][:, None, 0] * q[..., 0] + f["center"][:, None, 0] * q[..., 2]
        v = f["focal"][:, None, 1] * q[..., 1] + f["center"][:, None, 1] * q[..., 2]
        mask = (u >= 0) & (u < 1920) & (v >= 0) & (v < 1080)
        vis = (torch.sqrt(((p3a - g3a) ** 2).sum(dim=-1)) * mask).sum()
    # ---- :376-383
    betas = ((f["pred_betas"] - f["gt_betas"]) ** 2).sum() / B
    body_pose = ((f["pred_body_pose"].reshape(B, -1) - f["gt_body_pose"].reshape(B, -1)) ** 2).sum() / B
    global_orient = ((f["pred_global_orient"].reshape(B, -1) - f["gt_global_orient"].reshape(B, -1)) ** 2).sum() / B
    # ---- :386-388
    x = f["pred_pose_6d"].reshape(-1, 3, 2)
    ortho = ((torch.matmul(x.permute(0, 2, 1), x) - torch.eye(2, dtype=x.dtype).unsqueeze(0)) ** 2).mean()
    # ---- :390-419 (handed in)
    pen = torch.zeros((), dtype=torch.float64) if penetration is None else penetration.double().mean()
    terms = [v2v, kp3d, kp3d_full, kp2d, betas, body_pose, global_orient, ortho, pen]
    loss = sum(float(w) * t for w, t in zip(weights, terms))                                           # :422-430
    return dict(zip(LOSS_KEYS, [loss] + terms + [vis]))


def val_losses_grads64(inp: dict, weights, gloss=1.0, penetration=None) -> dict:
    """d (gloss * loss) / d each prediction array (and 'penetration' when given) as float64 numpy arrays, by torch.autograd.grad on val_losses_torch64."""
    t = as_f64(inp, PREDICTIONS)
    pen = None if penetration is None else torch.as_tensor(np.asarray(penetration)).double().requires_grad_()
    loss = val_losses_torch64(t, weights, pen)["loss"]
    names = list(PREDICTIONS) + (["penetration"] if pen is not None else [])
    grads = torch.autograd.grad([loss * float(gloss)], [t[k] for k in PREDICTIONS] + ([pen] if pen is not None else []), allow_unused=True)
    return {k: (np.zeros(tuple((pen if k == "penetration" else t[k]).shape)) if g is None else g.numpy()) for k, g in zip(names, grads)}
