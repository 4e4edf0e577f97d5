#!/usr/bin/env python3
"""Timing of the validation losses (csrc/loss.hip): ehm_val_losses alone against its bytes from shapes and against the same formulas as eager float32
torch ops (tools/_eager.py: val_losses_eager - there is no earlier native version to compare with), and the whole EgoHMR.compute_loss (two
ground-truth SMPL decodes + the rotations + the kernel).  HIP events, warm-up, back-to-back calls.
    python tools/bench_losses.py [--batches 256 1280] [--reps 30] [--once]      -> one JSON line per batch size
--once: one call of each after the warm-up, for a `rocprofv3 --kernel-trace --stats` run of its own."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _eager import val_losses_eager  # noqa: E402
from egohmr_amd import synthetic as syn  # noqa: E402
from egohmr_amd.factory import batch_to_device, build_synthetic_model  # noqa: E402
from egohmr_amd.model import val_losses_native  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, MI355X


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def annotated(B, dev, seed=21):
    b, a = syn.make_batch(B, 512, seed=seed), syn.make_gt_annotations(B, seed=seed)
    b["smpl_params"].update(global_orient=a["global_orient"], body_pose=a["body_pose"], betas=a["betas"])
    g = np.random.default_rng(seed)
    b.update(gender=a["gender"], keypoints_3d=g.normal(size=(B, 24, 3)).astype(np.float32),
             keypoints_3d_full=(g.normal(size=(B, 24, 3)) + [0, 0, 3]).astype(np.float32))
    batch = batch_to_device(b, dev)
    batch["smpl_params_is_axis_angle"] = {"global_orient": np.ones(B, bool), "body_pose": np.ones(B, bool)}
    return batch


def measure(model, B, reps, once, dev):
    batch = annotated(B, dev)
    V, J = model.smpl.num_verts, model.smpl.num_joints_out
    # a model output of the right shapes (the losses do not care where it came from): the neutral body of the ground-truth parameters
    so = model.smpl(betas=batch["smpl_params"]["betas"], body_pose=batch["smpl_params"]["body_pose"], global_orient=batch["smpl_params"]["global_orient"])
    rot = torch.randn(B, 24, 3, 3, device=dev)
    out = {"pred_smpl_params": {"global_orient": rot[:, :1].contiguous(), "body_pose": rot[:, 1:].contiguous(), "betas": torch.randn(B, 10, device=dev)},
           "pred_pose_6d": torch.randn(B, 144, device=dev), "pred_keypoints_3d": so.joints, "pred_vertices": so.vertices,
           "pred_keypoints_3d_full": so.joints + batch["smpl_params"]["transl"][:, None], "pred_keypoints_2d_full": torch.rand(B, J, 2, device=dev) - 0.5}
    model.focal_length = (batch["fx"] * 1500.0).unsqueeze(-1).repeat(1, 2)
    model.camera_center_full = torch.stack([batch["cam_cx"], batch["cam_cy"]], -1)
    t = model.loss_inputs(batch, out)
    w = model.loss_weights()
    nbytes = 2 * B * V * 3 * 4 + sum(v.numel() * v.element_size() for k, v in t.items() if "vertices" not in k) - B * J * 3 * 4   # one ground truth per item
    n = 1 if once else reps
    t_native = timed(lambda: val_losses_native(t, w), n)
    t_eager = timed(lambda: val_losses_eager(t, w), n)
    t_whole = timed(lambda: model.compute_loss(batch, dict(out)), n)
    a, (b, cnt) = val_losses_native(t, w), val_losses_eager(t, w)
    rel = ((a["losses"] - b).abs() / b.abs().clamp_min(1e-30)).max().item()
    return {"B": B, "V": V, "reps": n, "ehm_val_losses_ms": t_native, "bytes": nbytes, "frac_of_hbm_peak": nbytes / (t_native * 1e-3) / HBM_PEAK,
            "eager_f32_ms": t_eager, "eager_over_native": t_eager / t_native, "compute_loss_ms": t_whole,
            "max_rel_dev_native_vs_eager_f32": rel, "visible_joints_equal": bool(int(a["joint_vis_num"][0]) == int(cnt))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1280])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = build_synthetic_model(dev, 0, smpl_asset_male=syn.make_smpl_asset(1), smpl_asset_female=syn.make_smpl_asset(2), weight_loss_v2v=0.5,
                                  weight_loss_keypoints_3d=0.05, weight_loss_keypoints_3d_full=0.02, weight_loss_keypoints_2d_full=0.01,
                                  weight_loss_betas=0.0005, weight_loss_body_pose=0.001, weight_loss_global_orient=0.002, weight_loss_pose_6d_ortho=0.1)
    for B in args.batches:
        print(json.dumps(measure(model, B, args.reps, args.once, dev)), flush=True)


if __name__ == "__main__":
    main()
