#!/usr/bin/env python3
"""Time of one GaussianDiffusion.training_losses call (EgoHMR.frozen_trunk_training: forward, loss, backward, one AdamW step) on the default synthetic
model, B = 64 items with N = 4096 scene points, batch-statistics BatchNorm: the median of the timed calls after warm-up, whole and split by phase with
device events recorded on the launch stream around each phase (everything runs on one stream, so a phase's events bracket its kernels):
  trunk | PointNet fwd + bwd | assembly fwd + bwd | denoiser fwd + bwd | decode + loss fwd + bwd | optimiser | rest (the small torch modules, host gaps)
A record, not a bar: the parent commit has no training step.  Prints one JSON line.
--trunk-grad: with EgoHMR.trunk_grad (the trunk's weights train: its autograd forward is the "trunk" phase, its backward "trunk_bwd").
--train-bn (with --trunk-grad): ResNet50Features.train_batchnorm too - the backbone in .train() on batch statistics, as the reference trains it.
--gpus N: the data-parallel step (EgoHMR.data_parallel): this process starts N rank processes of itself (one device each over RCCL; --backend gloo: all
    on device 0, a functional run), each under its own time limit, --batch is the GLOBAL batch, dealt out by dist.shard_range; rank 0 prints the line, with
    the slowest rank's median beside its own.
    python tools/train_step_bench.py [--batch 64] [--points 4096] [--warmup 3] [--calls 12] [--trunk-grad] [--train-bn] [--gpus N]"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egohmr_amd import gcn_grad, pointnet_grad, train_grad, trunk_grad  # noqa: E402
from egohmr_amd import dist as edist  # noqa: E402
from egohmr_amd import synthetic as syn  # noqa: E402
from egohmr_amd.diffusion import create_gaussian_diffusion  # noqa: E402
from egohmr_amd.factory import batch_to_device, build_synthetic_model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--points", type=int, default=4096)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=12)
ap.add_argument("--trunk-grad", action="store_true")
ap.add_argument("--train-bn", action="store_true")
ap.add_argument("--gpus", type=int, default=1)
ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"])
ap.add_argument("--rank-timeout", type=float, default=600.0, help="seconds each rank process may take")
args = ap.parse_args()
assert args.trunk_grad or not args.train_bn, "--train-bn is consulted with --trunk-grad only"
assert args.calls >= 10, "the median is taken over at least 10 calls"
assert torch.cuda.is_available(), "this measurement needs the GPU; there is no CPU fallback"
assert 1 <= args.gpus <= args.batch, "every rank needs at least one item"
if args.gpus > 1 and "RANK" not in os.environ:
    # the launcher: one fresh process per rank, each under its own time limit; rank 0's line is the result
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    procs = [subprocess.Popen([sys.executable] + sys.argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), LOCAL_RANK=str(r),
                                       WORLD_SIZE=str(args.gpus), EGOHMR_DIST_BACKEND=args.backend)) for r in range(args.gpus)]
    rc = 0
    for r, p in enumerate(procs):
        try:
            out, err = p.communicate(timeout=args.rank_timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            sys.exit(f"rank {r} did not finish within {args.rank_timeout:g} s")
        if p.returncode != 0:
            rc = p.returncode
            print(f"rank {r} failed ({p.returncode}):\n{err[-2000:]}", file=sys.stderr)
        elif r == 0:
            print(out.strip().splitlines()[-1])
    sys.exit(rc)
rank, world, local = edist.init_from_env(args.backend) if args.gpus > 1 else (0, 1, 0)
dev = torch.device("cuda", local if world > 1 and args.backend == "nccl" else 0)
torch.cuda.set_device(dev)
B = len(edist.shard_range(args.batch, rank, world))          # this rank's items

# the loss weights of tests/val_losses_ref.CASE_WEIGHTS (every term on except the penetration term, which starts at a later epoch)
weights = dict(weight_loss_v2v=0.5, weight_loss_keypoints_3d=0.05, weight_loss_keypoints_3d_full=0.02, weight_loss_keypoints_2d_full=0.01,
               weight_loss_betas=0.0005, weight_loss_body_pose=0.001, weight_loss_global_orient=0.002, weight_loss_pose_6d_ortho=0.1)
model = build_synthetic_model(dev, 0, smpl_asset_male=syn.make_smpl_asset(1), smpl_asset_female=syn.make_smpl_asset(2), **weights)
model.frozen_trunk_training = True
model.diffusion_model.train_batchnorm = True
model.trunk_grad = bool(args.trunk_grad)
model.backbone.train_batchnorm = bool(args.train_bn)
model.data_parallel = world > 1
model.init_optimizers()
g = np.random.default_rng(1 + rank)
b = syn.make_batch(B, args.points, seed=1 + rank)
b["smpl_params"].update(global_orient=g.normal(scale=0.3, size=(B, 3)).astype(np.float32), body_pose=g.normal(scale=0.2, size=(B, 69)).astype(np.float32),
                        betas=g.normal(scale=0.5, size=(B, 10)).astype(np.float32))
kp3d = g.normal(scale=0.3, size=(B, 24, 3)).astype(np.float32)
b.update(keypoints_3d=kp3d, keypoints_3d_full=kp3d + b["smpl_params"]["transl"][:, None], gender=g.integers(0, 2, size=B))
batch = batch_to_device(b, dev)
batch["smpl_params_is_axis_angle"] = {k: np.ones(B, bool) for k in ("global_orient", "body_pose", "betas", "transl")}
mean, std = syn.make_body_rep_stats(0)
d = create_gaussian_diffusion(num_diffusion_timesteps=1000, timestep_respacing="", body_rep_mean=mean, body_rep_std=std)
t = torch.from_numpy(g.integers(0, 1000, size=B)).to(dev)
noise = torch.from_numpy(g.normal(size=(B, 144)).astype(np.float32)).to(dev)

# ---- phase events
spans = {}          # phase -> [(start, end)] of the current call
marks = {}


def timed(fn, phase):
    def call(*a, **k):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        try:
            return fn(*a, **k)
        finally:
            e.record()
            spans.setdefault(phase, []).append((s, e))
    return call


def mark(fn, name, before):
    def call(*a, **k):
        if before:
            marks[name] = torch.cuda.Event(enable_timing=True)
            marks[name].record()
        out = fn(*a, **k)
        if not before:
            marks[name] = torch.cuda.Event(enable_timing=True)
            marks[name].record()
        return out
    return call


fs = model.fused_sampler
backbone_fn = fs._backbone_fn
fs._backbone_fn = lambda: timed(backbone_fn(), "trunk")
if args.trunk_grad:
    model.backbone.forward = timed(model.backbone.forward, "trunk")
    trunk_grad.TrunkFunction.backward = staticmethod(timed(trunk_grad.TrunkFunction.backward, "trunk_bwd"))
    trunk_grad.TrunkTrainFunction.backward = staticmethod(timed(trunk_grad.TrunkTrainFunction.backward, "trunk_bwd"))
model.scene_enc.forward = timed(model.scene_enc.forward, "pointnet_fwd")
pointnet_grad.PointnetFunction.backward = staticmethod(timed(pointnet_grad.PointnetFunction.backward, "pointnet_bwd"))
train_grad.cond_assemble_native = timed(train_grad.cond_assemble_native, "assembly_fwd")
train_grad.cond_assemble_backward_native = timed(train_grad.cond_assemble_backward_native, "assembly_bwd")
model.diffusion_model.forward = timed(model.diffusion_model.forward, "denoiser_fwd")
gcn_grad.GCNTrainFunction.backward = staticmethod(mark(timed(gcn_grad.GCNTrainFunction.backward, "denoiser_bwd"), "denoiser_bwd_start", True))
model.decode_output = timed(model.decode_output, "decode_loss_fwd")
model.compute_loss = timed(model.compute_loss, "decode_loss_fwd")
opt = model.optimizer
opt.zero_grad = mark(opt.zero_grad, "backward_start", False)             # training_step: zero_grad, loss.backward(), step
opt.step = timed(opt.step, "optimiser")


def one_call():
    spans.clear()
    marks.clear()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = d.training_losses(model, batch, t, noise=noise)
    e.record()
    torch.cuda.synchronize()
    ms = {k: sum(a.elapsed_time(z) for a, z in v) for k, v in spans.items()}
    ms["decode_loss_bwd"] = marks["backward_start"].elapsed_time(marks["denoiser_bwd_start"])    # loss -> SMPL -> rot6d, up to the denoiser's output
    ms["total"] = s.elapsed_time(e)
    ms["rest"] = ms["total"] - sum(v for k, v in ms.items() if k != "total")
    return ms, float(out["losses"]["loss"])


for _ in range(args.warmup):
    one_call()
runs, losses = [], []
torch.cuda.reset_peak_memory_stats()
for _ in range(args.calls):
    ms, loss = one_call()
    runs.append(ms)
    losses.append(loss)
med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
pair = lambda a, b_: round(med[a] + med[b_], 3)
med.setdefault("trunk_bwd", 0.0)
slowest = edist.max_over_ranks(med["total"], dev)
if rank != 0:
    sys.exit(0)
print(json.dumps({"gpus": world, "backend": args.backend if world > 1 else None, "global_batch": args.batch, "slowest_rank_median_ms": round(slowest, 3),
                  "what": "one training_losses call, " + (("trunk_grad + train_batchnorm" if args.train_bn else "trunk_grad") if args.trunk_grad else "frozen trunk"), "batch": B, "scene_points": args.points, "warmup": args.warmup, "calls": args.calls,
                  "median_ms": round(med["total"], 3), "min_ms": round(min(r["total"] for r in runs), 3), "max_ms": round(max(r["total"] for r in runs), 3),
                  "phases_median_ms": {"trunk": round(med["trunk"], 3), "trunk_bwd": round(med["trunk_bwd"], 3), "pointnet_fwd_bwd": pair("pointnet_fwd", "pointnet_bwd"),
                                       "assembly_fwd_bwd": pair("assembly_fwd", "assembly_bwd"), "denoiser_fwd_bwd": pair("denoiser_fwd", "denoiser_bwd"),
                                       "decode_loss_fwd_bwd": pair("decode_loss_fwd", "decode_loss_bwd"), "optimiser": round(med["optimiser"], 3),
                                       "rest": round(med["rest"], 3)},
                  "assembly_fwd_ms": round(med["assembly_fwd"], 4), "assembly_bwd_ms": round(med["assembly_bwd"], 4),
                  "assembly_bytes": 4 * B * 24 * model.diffusion_model.in_dim, "loss_first": losses[0], "loss_last": losses[-1],
                  "peak_allocated_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))
