"""The sample / decode / evaluate block of the reference's stage-2 driver as a reusable harness.

What it stands in for (test_egohmr.py; argparse, the EgoBody dataloader, open3d rendering and logging are out of scope):
    :241-266   S sampling loops per batch through ``diffusion.val_losses`` (optionally collision-guided), ``model.eval_coll`` per
               sample, ``pred_smpl_params`` stacked to [B, S, ...]
    :268-318   ground-truth bodies (male / female SMPL by ``gender``), pelvis alignment
    :291-301   second SMPL decode of all B*S predicted bodies, camera-frame vertices / joints
    :374-505   G-MPJPE / MPJPE / PA-MPJPE / V2V with their visible / invisible splits, std / APD diversity, contact score
    :507-560   the running means the script prints (`error_dict`, `diversity_dict`)
    :672-695   ``results_seed_{seed}.pkl``
``Stage1Driver`` is the counterpart for the stage-1 script (test_prohmr_scene.py:160-217, 293-321, 417-426): the body translation of every image
into ``output_prohmr_scene_{model_id}/results.pkl``, which ``--two_stage`` stage-2 runs read, and the six error figures of the mode.
Everything stays on the device until ``summary()`` / ``results()``; the reference moves every metric to numpy per batch and runs
the Procrustes alignment as a CPU loop of numpy SVDs (utils/pose_utils.py).  The S samples of a batch share one conditioning pass
(``FusedSampler.prepare`` caches it per batch), the reference re-runs ResNet-50 and the PointNet in every denoising step.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import io as eio
from . import metrics as M
from .geometry import perspective_projection


@torch.no_grad()
def ground_truth_bodies(smpl_male, smpl_female, batch, transl) -> dict:
    """The ground-truth bodies of test_egohmr.py:306-318 / test_prohmr_scene.py:219-232: the male and the female model on the batch's annotations
    at the translation ``transl``, the female one where ``gender == 1``; the first 24 joints, the vertices, the pelvis and both pelvis-aligned."""
    sp = batch["smpl_params"]
    kw = dict(global_orient=sp["global_orient"], transl=transl, body_pose=sp["body_pose"], betas=sp["betas"])
    male, female = smpl_male(**kw), smpl_female(**kw)
    fem = (batch["gender"] == 1).view(-1, 1, 1)
    joints = torch.where(fem, female.joints, male.joints)
    verts = torch.where(fem, female.vertices, male.vertices)
    j24 = joints[:, :24, :]
    pelvis = j24[:, [0], :].clone()
    return dict(joints=j24, vertices=verts, pelvis=pelvis, joints_align=j24 - pelvis, vertices_align=verts - pelvis)


class Stage2Driver:
    def __init__(self, model, diffusion, smpl_neutral, smpl_male, smpl_female, num_samples: int = 5, timestep_respacing: str = "",
                 with_coap_grad: bool = False, cond_grad_weight: float = 2.0, eval_coll_loss: bool = False,
                 eval_contact_score: bool = True, eval_with_vis_mask_pa: bool = False, fx_norm_coeff: float = 1500.0,
                 batch_samples: bool = True, two_stage: bool = False):
        self.model, self.diffusion = model, diffusion
        self.smpl_neutral, self.smpl_male, self.smpl_female = smpl_neutral, smpl_male, smpl_female
        self.S, self.respacing = int(num_samples), timestep_respacing
        self.guided, self.w = bool(with_coap_grad), float(cond_grad_weight)
        self.eval_coll_loss, self.eval_contact = bool(eval_coll_loss), bool(eval_contact_score)
        self.fx_norm_coeff = fx_norm_coeff
        self.batch_samples = bool(batch_samples)   # the S samples of a batch as one fused loop over S*B bodies (FusedSampler.run_samples)
        # --two_stage (test_egohmr.py:24, default True there): the batch carries `stage1_transl_full` [B,3] - the stage-1 (ProHMR-scene)
        # camera-frame translation, results.pkl['pred_cam_full_list'] read by egohmr_amd.io.load_stage1_cam - and the sampler is
        # conditioned on it instead of the ground-truth translation (:243-245)
        self.two_stage = bool(two_stage)
        # --eval_with_vis_mask_pa (test_egohmr.py:73, default True in the reference's script; False here so that existing results do not change):
        # PA-MPJPE aligns on the visible joints only (reconstruction_error_with_vis_mask, utils/pose_utils.py:75-126; ehm_eval_procrustes_vis)
        self.eval_with_vis_mask_pa = bool(eval_with_vis_mask_pa)
        self._acc = {}
        self._lists = {k: [] for k in ("pred_betas", "pred_global_orient", "pred_body_pose", "gt_cam_full", "pred_cam_full", "coll", "contact")}
        self._vis_counts = dict(joint_vis=0, joint_invis=0, vertex_vis=0, vertex_invis=0)

    # ------------------------------------------------------------------ :241-266
    @torch.no_grad()
    def sample(self, batch, noise_stacks=None):
        """-> ({'betas' [B,S,10], 'global_orient' [B,S,1,3,3], 'body_pose' [B,S,23,3,3]}, coll_ratio [B,S] float64 numpy)."""
        B = batch["img"].shape[0]
        out = {"betas": [], "global_orient": [], "body_pose": []}
        coll = np.zeros((B, self.S))
        batched = None
        ddim = self.respacing[0:4] == "ddim"
        if self.S > 1 and self.batch_samples and self.diffusion._fused_ok(self.model, 0, None, None, False, 0.0, guided=self.guided) and not (ddim and self.guided):
            # the S loops of the reference (test_egohmr.py:251-266) as ONE loop over S*B bodies (FusedSampler.run_samples): same noise
            # draws in the same order, same per-body arithmetic
            self.model.validation_setup()
            dev = self.model.device
            stacks = noise_stacks if noise_stacks is not None else [self.diffusion._draw_stack([B, 144], dev, None) for _ in range(self.S)]
            batched = self.model.fused_sampler.run_samples(self.diffusion, batch, list(stacks[: self.S]), ddim=ddim, guided=self.guided,
                                                           cond_grad_weight=self.w)
        for n in range(self.S):
            if batched is not None:
                o = batched[n]["other_outputs"]
            else:
                o = self.diffusion.val_losses(model=self.model, batch=batch, shape=[B, 144], progress=False, clip_denoised=False, cur_epoch=0,
                                              timestep_respacing=self.respacing, cond_fn_with_grad=self.guided, cond_grad_weight=self.w,
                                              noise_stack=None if noise_stacks is None else noise_stacks[n])
            if self.eval_coll_loss:
                coll[:, n] = np.array(self.model.eval_coll(o))
            for k in out:
                out[k].append(o["pred_smpl_params"][k].unsqueeze(1))
        return {k: torch.cat(v, dim=1) for k, v in out.items()}, coll

    # ------------------------------------------------------------------ :291-301
    @torch.no_grad()
    def decode(self, pred, transl):
        B, S = pred["betas"].shape[:2]
        o = self.smpl_neutral(betas=pred["betas"].reshape(-1, 10), body_pose=pred["body_pose"].reshape(-1, 23, 3, 3),
                              global_orient=pred["global_orient"].reshape(-1, 1, 3, 3), pose2rot=False)
        verts = o.vertices.reshape(B, S, -1, 3)
        j24 = o.joints.reshape(B, S, -1, 3)[:, :, 0:24, :]
        pelvis = j24[:, :, [0], :].clone()
        t = transl.unsqueeze(1).unsqueeze(1)
        return dict(vertices=verts, joints=j24, pelvis=pelvis, joints_align=j24 - pelvis, vertices_align=verts - pelvis,
                    vertices_full=verts + t, joints_full=j24 + t)

    # ------------------------------------------------------------------ :306-318
    @torch.no_grad()
    def ground_truth(self, batch, gt_cam_full):
        return ground_truth_bodies(self.smpl_male, self.smpl_female, batch, gt_cam_full)

    # ------------------------------------------------------------------ one batch: :230-505
    @torch.no_grad()
    def step(self, batch, noise_stacks=None):
        dev = batch["img"].device
        B = batch["img"].shape[0]
        gt_cam_full = batch["smpl_params"]["transl"].clone()                       # :238
        if self.two_stage:                                                         # :243-245: replace the gt camera translation by stage 1's
            if "stage1_transl_full" not in batch:
                raise KeyError("two_stage=True needs batch['stage1_transl_full'] [B,3] (egohmr_amd.io.load_stage1_cam reads it from the stage-1 results.pkl)")
            batch["smpl_params"]["transl"] = batch["stage1_transl_full"].to(dev).float()
            self._lists["pred_cam_full"].append(batch["smpl_params"]["transl"])    # :302-303
        pred, coll = self.sample(batch, noise_stacks)
        p = self.decode(pred, batch["smpl_params"]["transl"])
        g = self.ground_truth(batch, gt_cam_full)
        # visibility of the ground truth in the full image (:374-389)
        focal = (batch["fx"] * self.fx_norm_coeff).unsqueeze(-1).repeat(1, 2)
        center = torch.stack([batch["cam_cx"], batch["cam_cy"]], dim=-1)
        zero = torch.zeros(B, 3, device=dev)
        inside = lambda uv: (uv[..., 0] >= 0) & (uv[..., 0] < 1920) & (uv[..., 1] >= 0) & (uv[..., 1] < 1080)
        jvis = inside(perspective_projection(g["joints"], zero, focal, center))                  # [B,24]
        vvis = inside(perspective_projection(g["vertices"], zero, focal, center))                # [B,V]
        S = self.S
        # :399-449 as four launches (csrc/eval.hip): per-point error, its mean and its sums over the visible / invisible points; PA-MPJPE's similarity
        # transform (utils/pose_utils.py:10-66) in float64 inside the kernel - the reference copies to the host and loops numpy SVDs per sample
        res = {}
        for k, r in (("g_mpjpe", M.point_errors(p["joints_full"], g["joints"], points=24, mask=jvis)),                       # :399
                     ("mpjpe", M.point_errors(p["joints_align"], g["joints_align"], points=24, mask=jvis)),                  # :409
                     ("v2v", M.point_errors(p["vertices_align"], g["vertices_align"], mask=vvis)),                           # :441
                     ("pa_mpjpe", M.procrustes(p["joints_align"][:, :, :24].contiguous(), g["joints_align"][:, :24].contiguous(), mask=jvis,       # :418-437
                                               align_mask=jvis if self.eval_with_vis_mask_pa else None))):
            res[k], res[k + "_vis_sum"], res[k + "_invis_sum"] = r["mean"], r["vis_sum"], r["invis_sum"]                     # [B,S] each
        if S > 1:                                                                               # :453-494: (std, apd) per joint selection, one launch each
            ja = p["joints_align"][:, :, :24].contiguous()
            res["std_joints"], res["apd_joints"] = M.diversity(ja)
            res["std_joints_vis"], res["apd_joints_vis"] = M.diversity(ja, jvis)
            res["std_joints_invis"], res["apd_joints_invis"] = M.diversity(ja, jvis, invert=True)
        else:
            res["std_joints"] = res["std_joints_vis"] = res["std_joints_invis"] = torch.full((B,), float("nan"), device=dev)
        if self.eval_contact:                                                                   # :496-505
            scene = batch["scene_pcd_verts_full"].unsqueeze(1).expand(-1, S, -1, -1).reshape(B * S, -1, 3)
            res["contact"] = M.contact_score(p["vertices_full"].reshape(B * S, -1, 3), scene).reshape(B, S).float()
        res["coll"] = torch.from_numpy(coll).to(dev)
        for k, v in res.items():
            self._acc.setdefault(k, []).append(v)
        self._vis_counts["joint_vis"] += int(jvis.sum())
        self._vis_counts["joint_invis"] += B * 24 - int(jvis.sum())
        self._vis_counts["vertex_vis"] += int(vvis.sum())
        self._vis_counts["vertex_invis"] += B * vvis.shape[1] - int(vvis.sum())
        self._lists["pred_betas"].append(pred["betas"])
        self._lists["pred_global_orient"].append(pred["global_orient"])
        self._lists["pred_body_pose"].append(pred["body_pose"])
        self._lists["gt_cam_full"].append(gt_cam_full)
        return dict(pred=pred, decoded=p, gt=g, joint_vis_mask=jvis, vertex_vis_mask=vvis, **res)

    # ------------------------------------------------------------------ :555-589
    @torch.no_grad()
    def render(self, step_result, batch, frames, frame_index, items=(0,), samples=None, renderer=None):
        """The overlay of test_egohmr.py:576-589 for the batch items ``items`` and the samples ``samples`` (None: all S) of one ``step`` result:
        ``decoded['vertices_full']`` over frame ``frame_index[item]`` of ``frames`` uint8 [Fr,H,W,3] (BGR as decoded, on the device), with
        fx = fy = ``batch['fx'] * fx_norm_coeff`` and the principal point ``int(cam_cx), int(cam_cy)`` as there.  -> uint8 [len(items), S', H, W, 3].
        The bbox rectangle and the image grid of the script are not drawn.  ``renderer``: a ``MeshRenderer`` over ``smpl_neutral.faces`` to reuse
        (one is built and kept otherwise).  The pixels are egohmr_amd.render's rule, not pyrender's."""
        from .render import MeshRenderer
        verts = step_result["decoded"]["vertices_full"]
        dev = verts.device
        if renderer is None:
            if getattr(self, "_renderer", None) is None or self._renderer.device != dev:
                self._renderer = MeshRenderer(self.smpl_neutral.faces, dev, num_vertices=verts.shape[2])
            renderer = self._renderer
        it = torch.as_tensor(list(items), dtype=torch.long, device=dev)
        sm = torch.arange(verts.shape[1], device=dev) if samples is None else torch.as_tensor(list(samples), dtype=torch.long, device=dev)
        n_i, n_s = it.numel(), sm.numel()
        v = verts[it][:, sm].reshape(n_i * n_s, verts.shape[2], 3)
        per = lambda x: x.to(dev).float()[it].repeat_interleave(n_s)
        focal = per(batch["fx"]) * self.fx_norm_coeff
        fidx = torch.as_tensor(frame_index).to(dev)[it].repeat_interleave(n_s).to(torch.int32)
        img = renderer.render(v, focal, focal, per(batch["cam_cx"]).trunc(), per(batch["cam_cy"]).trunc(), frames=frames, frame_index=fidx, bgr=True)["color"]
        return img.reshape(n_i, n_s, *img.shape[1:])

    # ------------------------------------------------------------------ :619-626
    @torch.no_grad()
    def save_overlays(self, images, names, folder, in_scene=None, frames=None, frame_index=None, quality=95, encoder=None):
        """The files of test_egohmr.py:619-626: one contact sheet per item of ``images`` (what ``render`` returns, uint8 [items, S, H, W, 3] BGR)
        written as ``<folder>/<names[i]>`` - the naming '{recording}_{frame}' stays the caller's.  Each sheet row is [input | overlay | in-scene]:
        the input is frame ``frame_index[i]`` of ``frames`` uint8 [Fr,H,W,3] (left out when ``frames`` is None), ``in_scene`` uint8
        [items, S, H, W, 3] is optional.  The sheet is halved (egohmr_amd.render.contact_sheet) and encoded on the device by a ``JpegEncoder``
        (``encoder``: one to reuse; one is built and kept otherwise) at ``quality`` and 4:2:0, cv2.imwrite's documented defaults.  -> the paths."""
        from .jpeg import JpegEncoder
        from .render import contact_sheet
        names = list(names)
        if images.dim() != 5 or len(names) != images.shape[0]:
            raise ValueError(f"save_overlays: {len(names)} names for images of shape {tuple(images.shape)}")
        dev = images.device
        if encoder is None:
            if getattr(self, "_encoder", None) is None or self._encoder.device != dev:
                self._encoder = JpegEncoder(dev)
            encoder = self._encoder
        inputs = None
        if frames is not None:
            fidx = torch.arange(len(names)) if frame_index is None else torch.as_tensor(frame_index)
            inputs = frames.to(dev)[fidx.to(dev).long()]
        sheets = [contact_sheet(None if inputs is None else inputs[i], images[i], None if in_scene is None else in_scene[i]) for i in range(len(names))]
        os.makedirs(folder, exist_ok=True)
        return encoder.write(torch.stack(sheets), [os.path.join(folder, n) for n in names], bgr=True, quality=quality)

    # ------------------------------------------------------------------ :507-560, :660-670
    def summary(self) -> dict:
        a = {k: torch.cat(v, 0).double().cpu().numpy() for k, v in self._acc.items()}
        S, c = self.S, self._vis_counts
        out = {}
        for name, key, vis_n, invis_n in (("G-MPJPE", "g_mpjpe", c["joint_vis"], c["joint_invis"]), ("MPJPE", "mpjpe", c["joint_vis"], c["joint_invis"]),
                                          ("PA-MPJPE", "pa_mpjpe", c["joint_vis"], c["joint_invis"]), ("V2V", "v2v", c["vertex_vis"], c["vertex_invis"])):
            out[name] = 1000 * a[key].mean()
            out[name + "-vis"] = 1000 * a[key + "_vis_sum"].sum() / max(vis_n, 1) / S
            out[name + "-invis"] = 1000 * a[key + "_invis_sum"].sum() / max(invis_n, 1) / S
        for name, key in (("std-joints", "std_joints"), ("std-joints-vis", "std_joints_vis"), ("std-joints-invis", "std_joints_invis"),
                          ("apd-joints", "apd_joints"), ("apd-joints-vis", "apd_joints_vis"), ("apd-joints-invis", "apd_joints_invis")):
            if key in a:
                v = a[key]
                out[name] = 1000 * v[~np.isnan(v)].mean() if (~np.isnan(v)).any() else float("nan")
        if "contact" in a:
            out["contact"] = a["contact"].mean()
        out["coll"] = a["coll"].mean()
        return out

    def results(self) -> dict:
        cat = lambda k: torch.cat(self._lists[k], 0)
        contact = torch.cat(self._acc["contact"], 0) if "contact" in self._acc else torch.zeros_like(torch.cat(self._acc["coll"], 0))
        return eio.results_dict(cat("pred_betas"), cat("pred_global_orient"), cat("pred_body_pose"), torch.cat(self._acc["coll"], 0), contact,
                                cat("gt_cam_full"), pred_cam_full=cat("pred_cam_full") if self.two_stage else None)      # :685-693

    def save(self, save_root: str, model_id: str, seed: int) -> str:
        return eio.save_results(save_root, model_id, seed, self.results())


class Stage1Driver:
    """test_prohmr_scene.py as a harness.  ``Stage1Driver(model)`` with an egohmr_amd.stage1.ProHMRSceneTransl is the translation half: run it over
    the stage-1 batches (whole-scene clouds), collect pred_cam_full (:209-217) and write results.pkl (:417-426).  With the three body models and an
    egohmr_amd.stage1.ProHMRScene, ``step`` also draws ``num_samples`` bodies per image and computes the six error figures of the mode (z = 0,
    :293-321): G-MPJPE, MPJPE, PA-MPJPE, G-V2V, V2V, PA-V2V, on the kernels of egohmr_amd.metrics; ``summary()`` returns their means in
    millimetres.  Stage-1 rendering is egohmr_amd.render's (it draws any vertices)."""

    METRICS = (("G-MPJPE", "g_mpjpe"), ("MPJPE", "mpjpe"), ("PA-MPJPE", "pa_mpjpe"), ("G-V2V", "g_v2v"), ("V2V", "v2v"), ("PA-V2V", "pa_v2v"))

    def __init__(self, model, smpl_neutral=None, smpl_male=None, smpl_female=None, num_samples: int = 4):
        self.model = model
        self.smpl_neutral, self.smpl_male, self.smpl_female = smpl_neutral, smpl_male, smpl_female
        self.S = int(num_samples)
        self.with_metrics = smpl_neutral is not None or smpl_male is not None or smpl_female is not None
        if self.with_metrics and (smpl_neutral is None or smpl_male is None or smpl_female is None):
            raise ValueError("Stage1Driver: the stage-1 metrics need all three body models (smpl_neutral, smpl_male, smpl_female)")
        if self.with_metrics:
            from .stage1 import ProHMRScene
            if not isinstance(model, ProHMRScene):
                raise TypeError(f"Stage1Driver: the stage-1 metrics need an egohmr_amd.stage1.ProHMRScene (pose samples), not {type(model).__name__}")
        self._cams = []
        self._acc = {}

    @torch.no_grad()
    def step(self, batch, z=None) -> dict:
        if not self.with_metrics:
            out = self.model(batch)
            self._cams.append(out["pred_cam_full"])
            return out
        out = self.model(batch, num_samples=self.S, z=z)
        self._cams.append(out["pred_cam_full"])
        sp, cam = out["pred_smpl_params"], out["pred_cam_full"]
        o = self.smpl_neutral(betas=sp["betas"][:, 0].contiguous(), body_pose=sp["body_pose"][:, 0].contiguous(),
                              global_orient=sp["global_orient"][:, 0].contiguous(), pose2rot=False)          # :195-200: the script's own decode
        # (with ITS neutral model, which need not be the one the network carries; the mode only)
        j24, verts = o.joints[:, :24, :], o.vertices
        pelvis = j24[:, [0], :].clone()                                                                       # :203-205
        p = dict(joints_align=(j24 - pelvis).unsqueeze(1), vertices_align=(verts - pelvis).unsqueeze(1),
                 joints_full=(j24 + cam.unsqueeze(1)).unsqueeze(1), vertices_full=(verts + cam.unsqueeze(1)).unsqueeze(1))   # :214-216
        g = ground_truth_bodies(self.smpl_male, self.smpl_female, batch, batch["smpl_params"]["transl"])      # :219-232
        res = {"g_mpjpe": M.point_errors(p["joints_full"], g["joints"], points=24)["mean"],                   # :293-295
               "mpjpe": M.point_errors(p["joints_align"], g["joints_align"], points=24)["mean"],              # :298-300
               "pa_mpjpe": M.procrustes(p["joints_align"].contiguous(), g["joints_align"].contiguous())["mean"],              # :303-306
               "g_v2v": M.point_errors(p["vertices_full"], g["vertices"])["mean"],                            # :309-311
               "v2v": M.point_errors(p["vertices_align"], g["vertices_align"])["mean"],                       # :314-316
               "pa_v2v": M.procrustes(p["vertices_align"].contiguous(), g["vertices_align"].contiguous())["mean"]}            # :319-321
        res = {k: v[:, 0] for k, v in res.items()}                                                            # [B] each
        for k, v in res.items():
            self._acc.setdefault(k, []).append(v)
        return dict(out, decoded=p, gt=g, **res)

    def summary(self) -> dict:
        """The means test_prohmr_scene.py:324-329 prints, in millimetres, over the images stepped so far (empty without the body models)."""
        return {name: 1000 * float(torch.cat(self._acc[key], 0).double().mean()) for name, key in self.METRICS if key in self._acc}

    def results(self) -> dict:
        """{'pred_cam_full_list': float32 numpy [n, 3]}, n = the images stepped so far, in order."""
        cam = torch.cat(self._cams, 0) if self._cams else torch.zeros(0, 3)
        return {"pred_cam_full_list": cam.detach().float().cpu().numpy()}

    def save(self, save_root: str, model_id: str) -> str:
        return eio.save_stage1_results(save_root, model_id, self.results()["pred_cam_full_list"])


def aggregate_val_losses(per_batch) -> dict:
    """The aggregation of train_egohmr.py:176-207 over an iterable of (losses dict, joint_vis_num_batch): every key summed over the batches (on the
    tensors' device) and divided by the number of batches, except 'loss_keypoints_3d_vis_batch_sum' (the plain sum), plus
    'loss_keypoints_3d_vis' = batch_sum / joint_vis_num * 1000 (mm per visible joint; the figure that picks best_model_vis.pt) and 'joint_vis_num'.
    (The reference's loop goes on to divide 'loss_keypoints_3d_vis' by the number of batches as well, :203-205 - an accident of iterating the dict it is
    adding to; not reproduced.)  Values are tensors / numbers as given: no host read-back here."""
    sums, vis_num, n = {}, 0, 0
    for losses, num in per_batch:
        for k, v in losses.items():
            sums[k] = sums[k] + v if k in sums else v + 0
        vis_num = vis_num + num
        n += 1
    if n == 0:
        raise ValueError("validate: no batches")
    out = {k: (v if k == "loss_keypoints_3d_vis_batch_sum" else v / n) for k, v in sums.items()}
    out["loss_keypoints_3d_vis"] = out["loss_keypoints_3d_vis_batch_sum"] / vis_num * 1000
    out["joint_vis_num"] = vis_num
    return out


@torch.no_grad()
def validate(model, diffusion, batches, timestep_respacing="", cur_epoch=0, noise_stacks=None) -> dict:
    """The validation loop of train_egohmr.py:176-213 without logging: one sampling loop + EgoHMR.compute_loss per batch
    (`diffusion.val_losses(..., compute_loss=True)`), the loss tensors summed on the device, ONE host read-back at the end.
    batches: an iterable of annotated batches on the model's device (EgoHMR.compute_loss lists the keys); noise_stacks: optional, one
    [T+1, B, 144] stack per batch.  -> {key: float} for the reference's eleven keys, 'loss_keypoints_3d_vis' and 'joint_vis_num' (int)."""
    def run():
        for i, batch in enumerate(batches):
            B = batch["img"].shape[0]
            o = diffusion.val_losses(model=model, batch=batch, shape=[B, 144], progress=False, clip_denoised=False, cur_epoch=cur_epoch,
                                     timestep_respacing=timestep_respacing, noise_stack=None if noise_stacks is None else noise_stacks[i])
            if not o["losses"]:
                raise KeyError("validate: batch %d carries no 'keypoints_3d' (a sampling-only batch has no validation loss)" % i)
            yield o["losses"], o["joint_vis_num_batch"]
    agg = aggregate_val_losses(run())
    keys = list(agg)
    host = torch.stack([agg[k].double() for k in keys]).cpu().tolist()
    return {k: (int(round(v)) if k == "joint_vis_num" else v) for k, v in zip(keys, host)}
