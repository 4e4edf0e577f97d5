#!/usr/bin/env python3
"""Write tests/golden/g21_val_losses_{a,b,c}.npz by running the REFERENCE's own EgoHMR.compute_loss / EgoHMRVolsmpl.compute_loss on the CPU
(models/egohmr/egohmr.py:307-449).  Test infrastructure, run by hand where the reference tree is present; not collected by pytest.

    python tests/make_loss_golden.py            # from the repository root

It reuses the shims of oracle/make_golden.py and replaces `smplx.create` with a gender-aware one: the synthetic asset of the gender
(neutral 0, male 1, female 2), axis-angle input through smplx's batch_rodrigues (pose2rot=True), `transl` added to vertices and joints.
The files hold data only: seeds and sizes, the annotations, the nine weights, x_t and the timestep, what the reference's forward returned that
compute_loss reads (no vertices: the tests decode them again from pred_x_start), and the reference's results.  Cases:
  a  EgoHMR, B = 6, N = 512, mixed genders, cur_epoch 0 (below start_coap_epoch: no penetration term)
  b  the same at N = 8000 on val_losses_ref.case_b_scene, at cur_epoch = start_coap_epoch and start_coap_epoch - 1
  c  EgoHMRVolsmpl on case a's inputs
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import val_losses_ref as R  # noqa: E402
from egohmr_amd import synthetic as syn  # noqa: E402
from oracle import make_golden as mg  # noqa: E402
from oracle.smpl import SMPLOracle  # noqa: E402

B, SEED, TIMESTEP = 6, 21, 3
ASSET_SEED = {"neutral": 0, "male": 1, "female": 2}


def batch_rodrigues(rot_vecs):
    """smplx/lbs.py batch_rodrigues: [n,3] axis-angle -> [n,3,3]."""
    angle = torch.norm(rot_vecs + 1e-8, dim=1, keepdim=True)
    d = rot_vecs / angle
    cos, sin = torch.cos(angle)[:, None], torch.sin(angle)[:, None]
    rx, ry, rz = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    z = torch.zeros_like(rx)
    K = torch.cat([z, -rz, ry, rz, z, -rx, -ry, rx, z], dim=1).view(-1, 3, 3)
    return torch.eye(3, dtype=rot_vecs.dtype)[None] + sin * K + (1 - cos) * torch.bmm(K, K)


class GenderSMPL(nn.Module):
    def __init__(self, gender):
        super().__init__()
        self.gender = gender
        asset = syn.make_smpl_asset(ASSET_SEED[gender])
        self._oracle = SMPLOracle(asset)
        for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"):
            self.register_buffer(k, torch.as_tensor(asset[k]))
        self.faces = asset["faces"]

    def forward(self, betas=None, body_pose=None, global_orient=None, transl=None, return_full_pose=False, pose2rot=True, **kw):
        n = betas.shape[0]
        if pose2rot:
            global_orient = batch_rodrigues(global_orient.reshape(-1, 3)).view(n, 1, 3, 3)
            body_pose = batch_rodrigues(body_pose.reshape(-1, 3)).view(n, 23, 3, 3)
        o = self._oracle(betas=betas, body_pose=body_pose, global_orient=global_orient, transl=transl, return_full_pose=return_full_pose)
        return SimpleNamespace(vertices=o.vertices, joints=o.joints, full_pose=o.full_pose, betas=betas, body_pose=body_pose, global_orient=global_orient)


def annotated_batch(N):
    """syn.make_batch + the ground-truth annotations of the EgoBody loader: axis-angle parameters, gender, the flags, keypoints_3d (the gendered body's 24
    joints in the body frame, 5 mm of annotation noise) and keypoints_3d_full (the same in the camera frame)."""
    b = syn.make_batch(B, N, seed=SEED)
    a = syn.make_gt_annotations(B, seed=SEED)
    b["smpl_params"].update(global_orient=a["global_orient"], body_pose=a["body_pose"], betas=a["betas"])
    b["gender"] = a["gender"]
    sp = {k: torch.from_numpy(v) for k, v in b["smpl_params"].items()}
    jm, jf = GenderSMPL("male")(**sp).joints.numpy(), GenderSMPL("female")(**sp).joints.numpy()
    j = np.where((a["gender"] == 1)[:, None, None], jf, jm)[:, :24]
    g = np.random.default_rng(9000 + SEED)
    b["keypoints_3d_full"] = (j + g.normal(scale=0.005, size=j.shape)).astype(np.float32)
    b["keypoints_3d"] = (j - b["smpl_params"]["transl"][:, None] + g.normal(scale=0.005, size=j.shape)).astype(np.float32)
    flags = {"global_orient": np.ones(B, bool), "body_pose": np.ones(B, bool), "betas": np.zeros(B, bool), "transl": np.zeros(B, bool)}
    return b, flags


def run_case(name, volsmpl, N, epochs, scene_fn=None):
    sd, mean_std = syn.make_state_dict(0), syn.make_body_rep_stats(0)
    model = mg.build_reference_model(sd, syn.make_smpl_asset(0), *mean_std, diffuse_fuse=True, volsmpl=volsmpl, start_coap_epoch=R.START_COAP_EPOCH,
                                     **R.CASE_WEIGHTS)
    assert model.smpl_male.gender == "male" and model.smpl_female.gender == "female" and model.smpl.gender == "neutral"
    b_np, flags = annotated_batch(N)
    if scene_fn is not None:
        b_np["scene_pcd_verts_full"] = scene_fn(b_np["scene_pcd_verts_full"], b_np["smpl_params"]["transl"], SEED)
    x_t = syn.make_noise_stack(1, B, seed=SEED)[0]
    batch = mg.to_torch_batch(b_np)
    batch["smpl_params_is_axis_angle"] = {k: torch.from_numpy(v) for k, v in flags.items()}
    batch["x_t"] = torch.from_numpy(x_t)
    model.validation_setup()
    with torch.no_grad():
        out = model(batch, torch.full((B,), TIMESTEP, dtype=torch.long))
        res = {}
        for e in epochs:
            o = dict(out)
            model.compute_loss(batch, o, cur_epoch=e)
            res[e] = ({k: float(v) for k, v in o["losses"].items()}, int(o["joint_vis_num_batch"]))
        # the mask the reference formed (:363-369), with the same float32 expressions, and the margin of its decisions
        sp = {k: v.float() for k, v in batch["smpl_params"].items()}
        jm, jf = model.smpl_male(**sp).joints, model.smpl_female(**sp).joints
        gj = torch.where((batch["gender"] == 1)[:, None, None], jf, jm)
        from utils.geometry import perspective_projection
        uv = perspective_projection(gj, translation=torch.zeros(B, 3), camera_center=model.camera_center_full, focal_length=model.focal_length)[:, :24]
    mask = ((uv[:, :, 0] >= 0) * (uv[:, :, 0] < 1920) * (uv[:, :, 1] >= 0) * (uv[:, :, 1] < 1080)).numpy()
    uvn = uv.numpy().astype(np.float64)
    margin = float(np.minimum(np.minimum(np.abs(uvn[..., 0]), np.abs(uvn[..., 0] - 1920)), np.minimum(np.abs(uvn[..., 1]), np.abs(uvn[..., 1] - 1080))).min())
    assert list(res[epochs[0]][0]) == list(R.LOSS_KEYS), list(res[epochs[0]][0])
    assert all(int(mask.sum()) == r[1] for r in res.values()) and 0 < mask.sum() < B * 24 and margin >= 0.5, (mask.sum(), res, margin)
    assert 0 < b_np["gender"].sum() < B
    extra = {}
    if scene_fn is not None:
        verts = model.smpl_output.vertices.numpy()
        term, n_sel, n_hi = R.penetration_f64(verts, model.scene_pcd_verts.numpy())
        print("   selected", n_sel.tolist(), "at index >= cap", n_hi.tolist(), "float64 term", term.mean())
        assert n_sel[0] > R.POINT_CAP and n_hi[0] > 0 and n_sel[1] == 0, (n_sel, n_hi)
        assert all(0 < n_sel[i] < R.POINT_CAP and n_hi[i] > 0 for i in range(2, B)), (n_sel, n_hi)
        pen_on, pen_off = res[R.START_COAP_EPOCH][0]["loss_coap_penetration"], res[R.START_COAP_EPOCH - 1][0]["loss_coap_penetration"]
        assert pen_on > 0 and pen_off == 0, (pen_on, pen_off)
        extra = dict(n_selected=n_sel, n_selected_high=n_hi, scene_sum=np.float64(b_np["scene_pcd_verts_full"].astype(np.float64).sum()))
    print(f"   {name}: margin {margin:.2f} px, {int(mask.sum())} of {B * 24} joints visible, genders {b_np['gender'].tolist()}")
    for e in epochs:
        print(f"   epoch {e}:", {k: f"{v:.6g}" for k, v in res[e][0].items()})
    mg.save(name, B=B, N=N, seed=SEED, timestep=TIMESTEP, volsmpl=int(volsmpl), epochs=np.array(epochs), start_coap_epoch=R.START_COAP_EPOCH,
            weight_names=np.array(R.WEIGHT_NAMES), weights=np.array([R.CASE_WEIGHTS[k] for k in R.WEIGHT_NAMES], np.float64),
            loss_keys=np.array(R.LOSS_KEYS), losses=np.array([[res[e][0][k] for k in R.LOSS_KEYS] for e in epochs], np.float32),
            joint_vis_num_batch=np.array([res[e][1] for e in epochs]), mask=mask, margin_px=margin,
            x_t=x_t, keypoints_3d=b_np["keypoints_3d"], keypoints_3d_full=b_np["keypoints_3d_full"], gender=b_np["gender"],
            gt_global_orient=b_np["smpl_params"]["global_orient"], gt_body_pose=b_np["smpl_params"]["body_pose"], gt_betas=b_np["smpl_params"]["betas"],
            **{"flag_" + k: v for k, v in flags.items()},
            pred_x_start=out["pred_x_start"].numpy(), pred_betas=out["pred_smpl_params"]["betas"].numpy(),
            pred_keypoints_2d_full=out["pred_keypoints_2d_full"].numpy(), pred_keypoints_3d_full=out["pred_keypoints_3d_full"].numpy(),
            focal=model.focal_length.numpy(), center=model.camera_center_full.numpy(),
            img_sum=np.float64(b_np["img"].astype(np.float64).sum()), **extra)


def main():
    mg.install_shims(syn.make_smpl_asset(0))
    sys.modules["smplx"].create = lambda *a, gender="neutral", **k: GenderSMPL(gender)
    torch.manual_seed(0)
    run_case("g21_val_losses_a", False, 512, [0])
    run_case("g21_val_losses_b", False, 8000, [R.START_COAP_EPOCH, R.START_COAP_EPOCH - 1], scene_fn=R.case_b_scene)
    run_case("g21_val_losses_c", True, 512, [0])


if __name__ == "__main__":
    main()
