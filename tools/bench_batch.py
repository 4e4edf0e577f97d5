"""Time the batch builder (egohmr_amd.batch) at the loader's shape: B = 256 patches of 224 x 224 from 1080 x 1920 uint8 frames (8 resident
frames, 32 items each), boxes of 150 - 600 px (the range synthetic.make_batch draws), full augmentation; the scene cloud at N = 20 000 float32
points per item.  Prints one JSON line per measurement:
  * ehm_image_patch and ehm_scene_augment alone: device events around `iters` back-to-back calls, `repeats` times (median, min, max), with the
    algorithmic bytes from the shapes (3 P^2 4 written plus the touched source footprint, box^2 3 bytes clipped to the frame, read; 12 N read and
    12 N / stride written per item) and their share of the 8 TB/s HBM bound;
  * for comparison, alternating with the kernel in the same process: the same patches as torch ops on the same GPU - uint8 BGR -> float RGB
    planes per frame, torch.nn.functional.grid_sample (bilinear, zeros, align_corners=True) for the frame's items, colour scale, clamp,
    normalise (no uint8 rounding step: it has no quantize);
  * BatchBuilder.build as a whole (host arithmetic, two uploads, both kernels, the batched SMPL call), wall clock with a final synchronize."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egohmr_amd import batch as eb, synthetic as syn  # noqa: E402
from egohmr_amd.smpl import SMPL  # noqa: E402

HBM_BPS = 8e12


def events_ms(fn, iters, repeats):
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def torch_patches(frames, frame_index, Minv, flip, color, mean, std, P):
    """The comparison path: grid_sample per frame on an expanded (stride-0) batch of that frame, then the colour / normalise chain."""
    F, H, W, _ = frames.shape
    B = Minv.shape[0]
    ys, xs = torch.meshgrid(torch.arange(P, device=frames.device, dtype=torch.float32), torch.arange(P, device=frames.device, dtype=torch.float32), indexing="ij")
    m = Minv.float()
    sx = m[:, 0, 0, None, None] * xs + m[:, 0, 1, None, None] * ys + m[:, 0, 2, None, None]
    sy = m[:, 1, 0, None, None] * xs + m[:, 1, 1, None, None] * ys + m[:, 1, 2, None, None]
    sx = torch.where(flip[:, None, None], (W - 1) - sx, sx)
    grid = torch.stack([2 * sx / (W - 1) - 1, 2 * sy / (H - 1) - 1], -1)
    out = torch.empty(B, 3, P, P, device=frames.device)
    for f in range(F):
        sel = (frame_index == f).nonzero().flatten()
        if len(sel):
            plane = frames[f].permute(2, 0, 1).flip(0).float()[None]
            out[sel] = torch.nn.functional.grid_sample(plane.expand(len(sel), -1, -1, -1), grid[sel], mode="bilinear", padding_mode="zeros", align_corners=True)
    out = (out * color.float()[:, :, None, None]).clamp(0, 255)
    return (out - mean[None, :, None, None]) / std[None, :, None, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = np.random.default_rng(0)
    B, P, F, H, W, N = args.batch, 224, 8, 1080, 1920, 20000
    frames = torch.from_numpy(g.integers(0, 256, (F, H, W, 3), dtype=np.uint8)).to(dev)
    fidx = np.arange(B) % F
    box = g.uniform(150, 600, B).astype(np.float32)
    center = np.stack([g.uniform(400, 1500, B), g.uniform(200, 900, B)], -1).astype(np.float32)
    np.random.seed(0)
    import random
    random.seed(0)
    aug = eb.draw_augmentation(eb.AugmentConfig(), B)
    a = syn.make_gt_annotations(B, seed=0)
    transl = (np.array([0.0, 0.0, 3.0]) + g.uniform(-0.5, 0.5, (B, 3))).astype(np.float32)
    kp2 = np.concatenate([g.uniform(0, W, (B, 25, 1)), g.uniform(0, H, (B, 25, 1)), g.uniform(0, 1, (B, 25, 1))], -1)
    scene = torch.from_numpy((transl[:, None] + g.uniform(-1, 1, (B, N, 3))).astype(np.float32)).to(dev)
    inputs = dict(center=center, bbox_size=box, keypoints_2d=kp2, keypoints_3d=transl[:, None].astype(np.float64) + g.normal(scale=0.3, size=(B, 24, 3)),
                  smpl_params=dict(global_orient=a["global_orient"], body_pose=a["body_pose"], betas=a["betas"], transl=transl),
                  fx=np.full(B, 1500.0), cx=np.full(B, 960.0), cy=np.full(B, 540.0))
    h = eb.host_item(aug, img_hw=(H, W), patch=P, **inputs)
    pp, apar = torch.from_numpy(h["patch_params"]).to(dev), torch.from_numpy(h["aug_params"]).to(dev)
    fidx_d = torch.from_numpy(fidx.astype(np.int32)).to(dev)
    img = torch.empty(B, 3, P, P, device=dev)

    # the touched source footprint from the shapes: the (scaled) box clipped to the frame
    half = h["box_size"].astype(np.float64) / 2
    bx, by = h["box_center"][:, 0].astype(np.float64), h["box_center"][:, 1].astype(np.float64)
    wx = np.clip(np.minimum(bx + half, W) - np.maximum(bx - half, 0), 0, None)
    wy = np.clip(np.minimum(by + half, H) - np.maximum(by - half, 0), 0, None)
    patch_bytes = B * 3 * P * P * 4 + float((wx * wy).sum()) * 3
    scene_bytes = B * N * 12 * 2

    Minv = pp[:, :6].reshape(B, 2, 3)
    flip, color = pp[:, 6] != 0, pp[:, 7:10]
    mean, std = torch.from_numpy(eb.IMAGE_MEAN).float().to(dev), torch.from_numpy(eb.IMAGE_STD).float().to(dev)
    k_fn = lambda: eb.image_patch(frames, fidx_d, pp, P, out=img)
    t_fn = lambda: torch_patches(frames, fidx_d, Minv, flip, color, mean, std, P)
    ref = t_fn()
    got = eb.image_patch(frames, fidx_d, pp, P, quantize=False)
    torch.cuda.synchronize()
    print(json.dumps({"check": "kernel (quantize off) against the float32 grid_sample path", "max_abs_diff": float((ref - got).abs().max()),
                      "mean_abs_diff": float((ref - got).abs().mean())}), flush=True)
    for _ in range(3):
        k_fn(), t_fn()
    torch.cuda.synchronize()
    k_ms, t_ms = [], []
    for _ in range(args.repeats):                                             # alternating, in the same process
        k_ms += events_ms(k_fn, args.iters, 1)
        t_ms += events_ms(t_fn, max(args.iters // 4, 1), 1)
    km = statistics.median(k_ms)
    print(json.dumps({"case": f"ehm_image_patch B={B} P={P} from {F} x {H}x{W} frames, boxes 150-600 px", **stats(k_ms), "algorithmic_bytes": int(patch_bytes),
                      "achieved_GBps": round(patch_bytes / km / 1e6, 1), "share_of_8TBps": round(patch_bytes / (km * 1e-3) / HBM_BPS, 4),
                      "patches_per_s": round(B / (km * 1e-3))}), flush=True)
    print(json.dumps({"case": "the same patches: torch grid_sample + normalise", **stats(t_ms), "ratio_to_kernel_median": round(statistics.median(t_ms) / km, 2)}), flush=True)
    s_ms = events_ms(lambda: eb.scene_augment(scene, apar, 1), args.iters, args.repeats)
    sm = statistics.median(s_ms)
    print(json.dumps({"case": f"ehm_scene_augment B={B} N={N} float32 stride 1", **stats(s_ms), "algorithmic_bytes": scene_bytes,
                      "achieved_GBps": round(scene_bytes / sm / 1e6, 1), "share_of_8TBps": round(scene_bytes / (sm * 1e-3) / HBM_BPS, 4)}), flush=True)

    bld = eb.BatchBuilder(dev, smpl_male=SMPL(syn.make_smpl_asset(1), gender="male").to(dev), smpl_female=SMPL(syn.make_smpl_asset(2), gender="female").to(dev))
    build = lambda augment: bld.build(frames, fidx, gender=a["gender"], fy=np.full(B, 1500.0), scene=scene, augment=augment, **inputs)
    for name, augment in (("augment=None", None), ("explicit augmentation", aug)):
        build(augment)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            build(augment)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"case": f"BatchBuilder.build B={B}, {name} (wall clock)", **stats(ms), "items_per_s": round(B / (statistics.median(ms) * 1e-3))}), flush=True)


if __name__ == "__main__":
    main()
