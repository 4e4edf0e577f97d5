"""Float64 torch restatement, on the CPU, of the training route of EgoHMR.forward with the image trunk frozen (models/egohmr/egohmr.py:173-303 under
self.training, :453-472) and of its loss: the conditioning assembly written as the reference's repeat / cat / mask_cond ops, the scene PointNet, the
timestep embedding and the graph convs from oracle.model, batch-statistics BatchNorm from gcn_train_ref, SMPL / geometry from the oracle, the loss from
val_losses_grad_ref.  `img_feats` is an input: the frozen trunk is not under test.  Shared by tests/test_train_step_cpu.py and tests/test_gpu_train_step.py;
not collected by pytest."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import gcn_train_ref as T
import val_losses_grad_ref as G
from oracle import geometry as ogeo
from oracle import model as om
from oracle.smpl import SMPLOracle

IMG = 2048
FX_NORM_COEFF = 1500.0                   # configs/prohmr.yaml:56
# the modules of init_optimizers (egohmr.py:140-147) in its order, without `backbone`
OPT_MODULES = ("scene_enc", "transl_enc", "beta_layer", "diffusion_model", "embed_timestep", "input_process")


def assemble_ref(img_feats, vis, drop, other, x_feat, temb, only_mask_img):
    """egohmr.py:190-191, :220-236 with mask_cond (:159-167) in the reference's ops.  img_feats [B,2048], vis [B,24] bool, drop [B] (1 = dropped) or None,
    other [B,n_other] = [scene | transl | cam], x_feat [B,24,E], temb [B,E] -> [B,24,2048 + n_other + 2 E], in the dtype of img_feats.
    (:167 multiplies [bs,24,d] by a [bs,1] mask, which broadcasts only for bs = 24 - and then over the joints; its comment says per item, and that is
    what is written here and what ehm_cond_assemble does.)"""
    B, dt = img_feats.shape[0], img_feats.dtype
    img24 = img_feats.unsqueeze(1).repeat(1, 24, 1)                                                      # :190
    img24 = img24 * vis.unsqueeze(-1).repeat(1, 1, img_feats.shape[-1]).to(dt)                           # :191
    cond = other.unsqueeze(1).repeat(1, 24, 1)                                                           # :222
    cond = torch.cat([img24, cond], dim=-1)                                                              # :223
    if drop is not None:                                                                                 # :159-167
        mask = drop.to(dt).view(B, 1)
        if only_mask_img:
            mask_final = torch.zeros([B, 24, cond.shape[-1]], dtype=dt)
            mask_final[torch.where(mask == 1)[0], :, 0:IMG] = 1
            cond = cond * (1. - mask_final)
        else:
            cond = cond * (1. - mask).unsqueeze(-1)
    temb24 = temb.unsqueeze(1).repeat(1, 24, 1)                                                          # :179
    return torch.cat([cond, x_feat, temb24], dim=-1)                                                     # :236


def state64(sd_np) -> dict:
    """A numpy state dict -> float64 CPU tensors (integer entries as they are)."""
    return {k: (torch.as_tensor(np.asarray(v)).double() if np.asarray(v).dtype.kind == "f" else torch.as_tensor(np.asarray(v)).clone()) for k, v in sd_np.items()}


def opt_names(model) -> list:
    """The names of model.opt_params in their order (an EgoHMR after init_optimizers())."""
    by_id = {id(p): n for n, p in model.named_parameters()}
    return [by_id[id(p)] for p in model.opt_params]


def visibility(kp2d, op2smpl):
    vis = torch.as_tensor(np.asarray(kp2d))[:, :, -1] > 0                                                # :186
    vis = vis.clone()
    vis[:, 8] = True                                                                                     # :187
    return vis[:, op2smpl]                                                                               # :188


def gt_inputs(batch, assets) -> dict:
    """The ground-truth arrays of compute_loss (egohmr.py:344-349, :380-381) in float64: `assets` = (male, female) SMPL assets."""
    d = lambda v: torch.as_tensor(np.asarray(v)).double()
    sp = batch["smpl_params"]
    B = d(sp["transl"]).shape[0]
    rot = {k: ogeo.aa_to_rotmat(d(sp[k]).reshape(-1, 3)).view(B, -1, 3, 3) for k in ("global_orient", "body_pose")}
    gt = {s: SMPLOracle(a, torch.float64)(betas=d(sp["betas"]), body_pose=rot["body_pose"], global_orient=rot["global_orient"], transl=d(sp["transl"]))
          for s, a in zip(("male", "female"), assets)}
    return dict(keypoints_2d=d(batch["orig_keypoints_2d"]), keypoints_3d=d(batch["keypoints_3d"]), keypoints_3d_full=d(batch["keypoints_3d_full"]),
                gt_vertices_male=gt["male"].vertices, gt_vertices_female=gt["female"].vertices, gt_joints_male=gt["male"].joints,
                gt_joints_female=gt["female"].joints, gender=torch.as_tensor(np.asarray(batch["gender"])).long().reshape(-1),
                gt_global_orient=rot["global_orient"].reshape(B, 9), gt_body_pose=rot["body_pose"].reshape(B, 207), gt_betas=d(sp["betas"]))


def x_start_of(batch, mean, std):
    """gaussian_diffusion.py:731-737 in float64."""
    d = lambda v: torch.as_tensor(np.asarray(v)).double()
    sp = batch["smpl_params"]
    B = d(sp["transl"]).shape[0]
    aa = torch.cat([d(sp["global_orient"]).reshape(B, -1), d(sp["body_pose"]).reshape(B, -1)], dim=1).reshape(-1, 3)
    rot6d = ogeo.rotmat_to_rot6d(ogeo.aa_to_rotmat(aa).reshape(-1, 3, 3), "diffusion").reshape(B, -1)
    return (rot6d - d(mean)) / d(std)


def train_forward(sd, batch, img_feats, x_t, t, *, weights, smpl_asset, gt, mean, std, op2smpl=om.OPENPOSE_TO_SMPL_LOOSE, drop=None,
                  only_mask_img=True, train_bn=True, update_running=True, blocks=4) -> dict:
    """The training forward + loss.  sd: float64 state dict (the leaves among its tensors receive the gradient; with train_bn the denoiser's running
    statistics are updated in place when update_running); batch: the annotated CPU batch; img_feats [B,2048], x_t [B,144], t [B] long; gt = gt_inputs(...).
    The model switches are the synthetic model's: with_bbox_info, with_cam_center, scene_cano.
    -> x0, betas, loss, losses, X, margin (min over the BatchNorm outputs / the output conv of min|v| / max|v|: the gates' distance from zero; train_bn only)."""
    d = lambda v: torch.as_tensor(np.asarray(v)).double()
    img_feats, x_t = d(img_feats), d(x_t)
    B = img_feats.shape[0]
    transl = d(batch["smpl_params"]["transl"])
    scene = d(batch["scene_pcd_verts_full"]) - transl.unsqueeze(1)                                       # :211 (scene_cano)
    scene_feats = om.resnet_pointnet(sd, scene)                                                          # :214
    h = F.relu(F.linear(transl, sd["transl_enc.layers.0.weight"], sd["transl_enc.layers.0.bias"]))
    transl_feat = F.linear(h, sd["transl_enc.layers.2.weight"], sd["transl_enc.layers.2.bias"])        # :217
    fx = d(batch["fx"])
    ofx = fx * FX_NORM_COEFF
    bc, bs = d(batch["box_center"]), d(batch["box_size"])
    cam = torch.cat([torch.stack([d(batch["cam_cx"]) / ofx, d(batch["cam_cy"]) / ofx], -1), torch.stack([bc[:, 0] / ofx, bc[:, 1] / ofx, bs / ofx], -1),
                     fx.unsqueeze(1)], dim=1)                                                            # :195-205: each part is PREpended
    other = torch.cat([scene_feats, transl_feat, cam], dim=1)                                            # :220-221
    vis = visibility(batch["orig_keypoints_2d"], op2smpl)
    temb = om.timestep_embedding(sd, torch.as_tensor(np.asarray(t)).long())                              # :178
    x_feat = F.linear(x_t.reshape(B, 24, 6), sd["input_process.poseEmbedding.weight"], sd["input_process.poseEmbedding.bias"])   # :234
    X = assemble_ref(img_feats, vis, None if drop is None else torch.as_tensor(np.asarray(drop)), other, x_feat, temb, only_mask_img)
    p = "diffusion_model."
    gsd = {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
    adj = om.smpl_adjacency(torch.float64)
    margin = None
    if train_bn:
        out, vs = T.modulated_gcn_train(gsd, X, adj, blocks=blocks, update_running=update_running)
        margin = min(float(v.detach().abs().min() / v.detach().abs().max()) for v in vs)
    else:
        out = T.eval_forward(gsd, X, adj, blocks=blocks)
    x0 = out.reshape(B, 144)                                                                             # :256
    pose6d = x0 * d(std) + d(mean)                                                                       # :258
    Rm = ogeo.rot6d_to_rotmat(pose6d, "diffusion").view(B, 24, 3, 3)
    hb = F.relu(F.linear(torch.cat([img_feats, other], dim=1), sd["beta_layer.layers.0.weight"], sd["beta_layer.layers.0.bias"]))   # :263-265
    betas = F.linear(hb, sd["beta_layer.layers.2.weight"], sd["beta_layer.layers.2.bias"]) + sd["beta_layer.init_betas"]
    so = SMPLOracle(smpl_asset, torch.float64)(betas=betas, body_pose=Rm[:, 1:], global_orient=Rm[:, [0]])
    focal = fx.unsqueeze(-1).repeat(1, 2) * FX_NORM_COEFF                                                # :283-285
    center = torch.stack([d(batch["cam_cx"]), d(batch["cam_cy"])], dim=-1)
    kp2d = ogeo.perspective_projection(so.joints, transl, focal, center)                                 # :295-298
    kp2d = torch.stack([kp2d[..., 0] / 1920 - 0.5, kp2d[..., 1] / 1080 - 0.5], dim=-1)
    inp = dict(gt, pred_vertices=so.vertices, pred_keypoints_3d=so.joints, pred_keypoints_3d_full=so.joints + transl[:, None], pred_keypoints_2d_full=kp2d,
               pred_global_orient=Rm[:, :1].reshape(B, 9), pred_body_pose=Rm[:, 1:].reshape(B, 207), pred_betas=betas, pred_pose_6d=pose6d,
               focal=focal, center=center)
    losses = G.val_losses_torch64(inp, weights)
    return dict(x0=x0, betas=betas, loss=losses["loss"], losses=losses, X=X, margin=margin)


def leaves(sd, names):
    """sd with the tensors in `names` replaced by leaves that require grad -> (sd, [leaves in the order of names])."""
    out = dict(sd)
    for n in names:
        out[n] = sd[n].detach().clone().requires_grad_()
    return out, [out[n] for n in names]


def adamw_steps(sd, names, step_fn, K, lr, weight_decay):
    """K steps of torch.optim.AdamW on the leaves `names` of sd (float64): step_fn(sd) -> loss.  -> (the K losses, sd after the last step)."""
    sd, ps = leaves(sd, names)
    opt = torch.optim.AdamW(params=ps, lr=lr, weight_decay=weight_decay)
    losses = []
    for _ in range(K):
        loss = step_fn(sd)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return losses, sd
