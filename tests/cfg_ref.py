"""Reference for the classifier-free guidance scales on the visibility fuse: `CFGOracle`, the CPU oracle's EgoHMR whose forward combines the
conditional output c and the masked output u per joint as

    x0[b, j, :] = u + s(b, j) * (c - u),        s(b, j) = vis[b, j] ? s_vis : s_inv,

with plain torch ops in the oracle's dtype (one rounding per op, the reference's egohmr.py:249); s == 1 takes c and s == 0 takes u unchanged.
It plugs into oracle.sampler's loops like EgoHMROracle does.  At (s_vis, s_inv) = (1, 0) it is EgoHMROracle, bit for bit.

Also here: the batch of the B = 3 cases (item 0 all joints visible, item 1 mixed, item 2 nothing but the forced joint), shared by
tests/make_cfg_golden.py and the tests, and the error bar of an affine combination of two outputs.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from egohmr_amd import synthetic as syn
from oracle import geometry as geo
from oracle.model import EgoHMROracle, modulated_gcn, timestep_embedding

B3, SEED, TIMESTEP, NUM_SCENE_POINTS = 3, 21, 37, 512            # weights and batch seeded as G10 (oracle/make_golden.py: g10_forward)
SCALE_PAIRS = [(1.0, 0.5), (2.5, 0.0), (2.5, 1.25), (0.5, 0.5), (1.0, -0.5)]


def make_batch3():
    """(batch dict of numpy arrays, x_t [3,144]) of the B = 3 forward cases."""
    b = syn.make_batch(B3, num_scene_points=NUM_SCENE_POINTS, seed=SEED)
    b["orig_keypoints_2d"][0, :, 2] = 1.0          # all visible
    b["orig_keypoints_2d"][2, :, 2] = 0.0          # none visible but the forced joint (egohmr.py:187); item 1 keeps its random mix
    return b, syn.make_noise_stack(0, B3, seed=SEED)[0]


def to_torch(b):
    return {k: (to_torch(v) if isinstance(v, dict) else torch.from_numpy(np.asarray(v))) for k, v in b.items()}


def bar(s, unit=5e-5):
    """|s c + (1 - s) u - exact| <= (|s| + |1 - s|) * unit when c and u are each within `unit` of theirs."""
    return (abs(s) + abs(1.0 - s)) * unit


class CFGOracle(EgoHMROracle):
    def __init__(self, *args, s_vis=1.0, s_inv=0.0, **kwargs):
        super().__init__(*args, **kwargs)
        self.s_vis, self.s_inv = float(s_vis), float(s_inv)

    def denoise(self, batch, timesteps):
        """(c, u, vis): the two denoiser outputs [B,24,6] and the joint visibility [B,24] (u is None when both scales are 1: one pass)."""
        sd, dt = self.sd, self.dtype
        B = batch["img"].shape[0]
        temb = timestep_embedding(sd, timesteps).unsqueeze(1).repeat(1, 24, 1)
        enc = self._encode(batch)
        vis = self.visibility(batch)
        batch["vis_mask_smpl"] = vis
        img24 = enc["img_feats"].unsqueeze(1).repeat(1, 24, 1) * vis.unsqueeze(-1).to(dt)
        other = torch.cat([enc["scene_feats"], enc["transl_feat"], enc["cam"]], dim=1)
        cond = torch.cat([img24, other.unsqueeze(1).repeat(1, 24, 1)], dim=-1)
        x_t = batch["x_t"].to(dt).reshape(B, 24, -1)
        x_feat = F.linear(x_t, sd["input_process.poseEmbedding.weight"], sd["input_process.poseEmbedding.bias"])
        run = lambda cnd: modulated_gcn(sd, torch.cat([cnd, x_feat, temb], dim=-1), self.adj, num_blocks=self.num_blocks, nonlocal_layer=self.nonlocal_layer)
        c, u = run(cond), None
        if not (self.s_vis == 1.0 and self.s_inv == 1.0):
            cond_u = cond.clone()
            if self.only_mask_img_cond:
                cond_u[:, :, 0:2048] = 0
            else:
                cond_u = torch.zeros_like(cond)
            u = run(cond_u)
        return c, u, vis, enc, other

    @staticmethod
    def combine(c, u, s):
        if s == 1.0:
            return c
        if s == 0.0:
            return u
        return u + s * (c - u)

    def forward(self, batch, timesteps):
        dt = self.dtype
        B = batch["img"].shape[0]
        c, u, vis, enc, other = self.denoise(batch, timesteps)
        if u is None:
            out = c
        else:
            out = torch.where(vis.unsqueeze(-1), self.combine(c, u, self.s_vis), self.combine(c, u, self.s_inv))
        x0 = out.reshape(B, -1)
        # the decode of EgoHMROracle.forward (egohmr.py:258-301)
        sd = self.sd
        pose6d = x0 * self.std + self.mean
        R = geo.rot6d_to_rotmat(pose6d, "diffusion").view(B, 24, 3, 3)
        feats_beta = torch.cat([enc["img_feats"], other], dim=1)
        h = F.relu(F.linear(feats_beta, sd["beta_layer.layers.0.weight"], sd["beta_layer.layers.0.bias"]))
        betas = F.linear(h, sd["beta_layer.layers.2.weight"], sd["beta_layer.layers.2.bias"]) + sd["beta_layer.init_betas"]
        so = self.smpl(betas=betas, body_pose=R[:, 1:], global_orient=R[:, [0]], return_full_pose=True)
        self.scene_pcd_verts = enc["scene"]
        focal = (batch["fx"].to(dt).unsqueeze(-1).repeat(1, 2)) * self.FX_NORM_COEFF
        center = torch.stack([batch["cam_cx"].to(dt), batch["cam_cy"].to(dt)], dim=-1)
        kp2d = geo.perspective_projection(so.joints, enc["transl"], focal, center)
        kp2d = torch.stack([kp2d[:, :, 0] / 1920 - 0.5, kp2d[:, :, 1] / 1080 - 0.5], dim=-1)
        return {
            "pred_x_start": x0,
            "pred_smpl_params": {"global_orient": R[:, [0]].clone(), "body_pose": R[:, 1:].clone(), "betas": betas.clone()},
            "pred_pose_6d": pose6d,
            "pred_keypoints_3d": so.joints,
            "pred_vertices": so.vertices,
            "pred_keypoints_3d_full": so.joints + enc["transl"].unsqueeze(1),
            "pred_keypoints_2d_full": kp2d,
        }


def make_oracle(dtype=torch.float32, s_vis=1.0, s_inv=0.0, cls=CFGOracle, **kw):
    """CFGOracle (or EgoHMROracle) on the seed-0 synthetic weights and asset."""
    mean, std = syn.make_body_rep_stats(0)
    extra = dict(s_vis=s_vis, s_inv=s_inv) if cls is CFGOracle else {}
    return cls(syn.make_state_dict(0), syn.make_smpl_asset(0), mean, std, dtype=dtype, faithful=False, **extra, **kw)
