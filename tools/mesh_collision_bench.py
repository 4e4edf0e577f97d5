#!/usr/bin/env python3
"""What the mesh collision term (EgoHMR.collision_proxy = 'mesh', csrc/mesh_collision.hip) costs beside the vertex proxy, on one GPU:
  entry    ehm_mesh_collision_query / ehm_collision_query at 1280 bodies x 20 000 scene points, bbox selection, with and without gverts (the
           difference is the scatter); posed bodies of the synthetic asset (13 776 faces), scene as synthetic.make_batch draws it
  guided   one BASELINE config 3 sampling call (B128 x S10 through run_samples, DDPM-100, N = 4096, 11 guided steps, weight 2) under 'vertex' and
           under 'mesh', every step in f16x3 (f16x3_last_steps = None: no calibration run, the same arithmetic in both)
HIP events, 1 warm-up, 3 timed calls, medians.  The synthetic asset's faces are random (not a closed surface): the pair loop's work is the real one,
the number of inside points (the scatter's work) is whatever the fractional winding number gives, and is reported.
    python tools/mesh_collision_bench.py [entry|guided|both]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egohmr_amd import _lib, synthetic as syn  # noqa: E402
from egohmr_amd.diffusion import create_gaussian_diffusion  # noqa: E402
from egohmr_amd.factory import batch_to_device, build_synthetic_model  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "both"
dev = torch.device("cuda:0")


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms)), 3)


out = {}
model = build_synthetic_model(dev, 0, diffuse_fuse=True)
model.f16x3_last_steps = None
fs = model.fused_sampler
if what in ("entry", "both"):
    B, N = 1280, 20000
    g = np.random.Generator(np.random.PCG64(1))
    x = torch.from_numpy(g.normal(size=(B, 144)).astype(np.float32)).to(dev) * 0.5
    betas = torch.from_numpy(g.normal(size=(B, 10)).astype(np.float32)).to(dev)
    mean, std = model._std_mean()
    verts = torch.empty(B, model.smpl.num_verts, 3, device=dev)
    joints = torch.empty(B, model.smpl.num_joints_out, 3, device=dev)
    _lib.api().ehm_smpl_forward_rot6d(model.smpl.handle(), betas, x, mean, std, verts, joints, None, None, None, B, _lib.stream_ptr())
    scene = torch.from_numpy(g.uniform(-1.0, 1.0, size=(B, N, 3)).astype(np.float32)).to(dev)
    row = {"bodies": B, "points": N, "faces": int(model.smpl.faces_tensor.shape[0])}
    for mode in ("vertex", "mesh"):
        model.collision_proxy = mode
        row[mode + "_ms"] = timed(lambda: fs.collision(verts, scene, want_grad=True, want_hits=True, all_points=False))
        row[mode + "_no_gverts_ms"] = timed(lambda: fs.collision(verts, scene, want_grad=False, want_hits=True, all_points=False))
        _, _, hits = fs.collision(verts, scene, want_grad=False, want_hits=True, all_points=False)
        row[mode + "_hits_per_body"] = round(float(hits.float().mean()), 1)
    lo, hi = verts.min(1, keepdim=True).values, verts.max(1, keepdim=True).values
    sel = ((scene >= lo) & (scene <= hi)).all(-1).sum(1).float()
    row["selected_per_body"] = round(float(sel.mean()), 1)
    row["mesh_pairs"] = int(sel.sum().item()) * row["faces"]
    row["mesh_gpairs_per_s"] = round(row["mesh_pairs"] / row["mesh_no_gverts_ms"] / 1e6, 1)
    out["entry"] = row
if what in ("guided", "both"):
    B, S, N = 128, 10, 4096
    d = create_gaussian_diffusion(num_diffusion_timesteps=100, timestep_respacing="")
    batch = batch_to_device(syn.make_batch(B, N, seed=100), dev)
    batch["scene_pcd_verts_full"][:, : N // 3, 1] = batch["smpl_params"]["transl"][:, None, 1] - 0.6
    noises = [torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B, seed=100 + 1000 * k)).to(dev) for k in range(S)]
    row = {"workload": "B128 x S10 DDPM-100, N=4096, 11 guided steps, weight 2, f16x3 every step"}

    def call(guided=True):
        fs.invalidate()
        fs.run_samples(d, batch, noises, ddim=False, guided=guided, cond_grad_weight=2.0 if guided else 1.0)
    row["unguided_ms"] = timed(lambda: call(False))
    for mode in ("vertex", "mesh"):
        model.collision_proxy = mode
        row[mode + "_ms"] = timed(call)
    out["guided"] = row
print(json.dumps(out))
