#!/usr/bin/env python3
"""ehm_val_losses_backward (csrc/loss.hip) at V = 6890, B = 256 and B = 1280: HIP-event time over back-to-back calls of the C entry point on preallocated
arrays, and in the same run (a) ehm_val_losses on the same inputs and (b) the backward of the same formulas written as eager float32 torch ops.
    python tools/bench_val_losses_grad.py [--reps 200] [--batches 256 1280]
Prints one JSON line per batch size: microseconds per call, the bytes the kernel must move from shapes (2 reads + 1 write of 4 B V 3 bytes: 63.5 MB at
B = 256) and the achieved bytes/s with its share of 8 TB/s.  `enqueue_us` is the host time to issue one call: where it exceeds the device time per call,
the event time measures the host, not the kernels (a `rocprofv3 --kernel-trace --stats` run of its own gives the kernel times then)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from egohmr_amd import _lib  # noqa: E402

V, HBM_BYTES_PER_S = 6890, 8.0e12
WEIGHTS = [0.5, 0.05, 0.02, 0.01, 0.0005, 0.001, 0.002, 0.1, 0.3]
SMPL_TO_OPENPOSE = [24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34]


def make_inputs(B, dev):
    g = torch.Generator(device=dev).manual_seed(B)
    f = lambda *s: torch.randn(*s, device=dev, generator=g)
    kp2d = torch.rand(B, 25, 3, device=dev, generator=g)
    gj = f(B, 45, 3) * 0.6
    gj[..., 2] += 3.0
    return dict(pred_vertices=f(B, V, 3), pred_keypoints_3d=f(B, 45, 3), pred_keypoints_3d_full=f(B, 45, 3), pred_keypoints_2d_full=f(B, 45, 2) * 0.3,
                pred_global_orient=f(B, 9), pred_body_pose=f(B, 207), pred_betas=f(B, 10), pred_pose_6d=f(B, 144), keypoints_2d=kp2d,
                keypoints_3d=f(B, 24, 3), keypoints_3d_full=f(B, 24, 3), gt_vertices_male=f(B, V, 3), gt_vertices_female=f(B, V, 3),
                gt_joints_male=gj, gt_joints_female=gj.clone(), gender=(torch.rand(B, device=dev, generator=g) < 0.5).long(),
                gt_global_orient=f(B, 9), gt_body_pose=f(B, 207), gt_betas=f(B, 10), focal=torch.full((B, 2), 1500.0, device=dev),
                center=torch.tensor([960.0, 540.0], device=dev).repeat(B, 1))


def sizes(t):
    return dict(B=t["pred_vertices"].shape[0], V=V, pred_joints=45, gt_joints=45, kp3d_points=24, kp3d_full_points=24, kp2d_points=25)


def native_backward(t, gloss):
    """-> (call, keep): `call()` issues one ehm_val_losses_backward with every output asked for."""
    B, P, A = t["pred_vertices"].shape[0], _lib.ptr, _lib.api()
    nb = C.c_int64(0)
    A.ehm_val_losses_backward_workspace_bytes(B, V, C.byref(nb))
    ws = torch.empty(nb.value // 4, device=gloss.device, dtype=torch.int32)
    g = {k: torch.empty_like(t[k]) for k in _lib.ValLossesBwdDesc.PREDICTIONS}
    g["penetration"] = torch.empty(B, device=gloss.device)
    d = _lib.ValLossesBwdDesc(**sizes(t), gloss=P(gloss), weights=(C.c_double * 9)(*WEIGHTS), workspace=P(ws), workspace_bytes=nb.value,
                              **{k: P(t[k]) for k in _lib.ValLossesBwdDesc.INPUTS}, **{"g_" + k: P(v) for k, v in g.items()})
    ref, s = C.byref(d), _lib.stream_ptr()
    return (lambda: A.ehm_val_losses_backward(ref, s)), (d, ws, g)


def native_forward(t):
    B, P, A = t["pred_vertices"].shape[0], _lib.ptr, _lib.api()
    dev = t["pred_vertices"].device
    nb = C.c_int64(0)
    A.ehm_val_losses_workspace_bytes(B, V, C.byref(nb))
    ws = torch.empty(nb.value // 8, device=dev, dtype=torch.float64)
    out = dict(losses=torch.empty(11, device=dev), joint_vis_num=torch.empty(1, device=dev, dtype=torch.int64), per_item=torch.empty(B, 11, device=dev),
               per_item_vis=torch.empty(B, device=dev, dtype=torch.int64), vis_mask=torch.empty(B, 24, device=dev, dtype=torch.uint8))
    d = _lib.ValLossesDesc(**sizes(t), penetration=None, weights=(C.c_double * 9)(*WEIGHTS), workspace=P(ws), workspace_bytes=nb.value,
                           **{k: P(v) for k, v in t.items()}, **{k: P(v) for k, v in out.items()})
    ref, s = C.byref(d), _lib.stream_ptr()
    return (lambda: A.ehm_val_losses(ref, s)), (d, ws, out)


def eager_backward(t, gloss):
    """The same gradients as whole-tensor float32 torch ops (ehm_val_losses_backward's formulas, include/egohmr_hip.h)."""
    B = t["pred_vertices"].shape[0]
    fem = (t["gender"] == 1)[:, None, None]
    idx = torch.tensor(SMPL_TO_OPENPOSE, device=gloss.device)

    def call():
        s = [gloss * (w / B) for w in WEIGHTS]
        gv, gj = torch.where(fem, t["gt_vertices_female"], t["gt_vertices_male"]), torch.where(fem, t["gt_joints_female"], t["gt_joints_male"])
        p3, g3 = t["pred_keypoints_3d"], t["keypoints_3d"]
        sv = torch.sign((t["pred_vertices"] - p3[:, [0]]) - (gv - gj[:, [0]]))
        g_pv = sv * (s[0] / (3 * V))
        sj = torch.sign((p3[:, :24] - p3[:, [0]]) - (g3[:, :24] - g3[:, [0]]))
        g_pj = torch.zeros_like(p3)
        g_pj[:, :24] = sj * s[1]
        g_pj[:, 0] -= sj.sum(1) * s[1] + sv.sum(1) * (s[0] / (3 * V))
        g_pf = torch.zeros_like(p3)
        g_pf[:, :24] = torch.sign(t["pred_keypoints_3d_full"][:, :24] - t["keypoints_3d_full"][:, :24]) * s[2]
        conf = t["keypoints_2d"][:, :25, 2:].clone()
        conf[:, [1, 9, 12]] = 0
        g_p2 = torch.zeros_like(t["pred_keypoints_2d_full"])
        g_p2[:, idx] = conf * torch.sign(t["pred_keypoints_2d_full"][:, idx] - t["keypoints_2d"][:, :25, :2]) * s[3]
        g_b = (t["pred_betas"] - t["gt_betas"]) * (2 * s[4])
        g_bp = (t["pred_body_pose"] - t["gt_body_pose"]) * (2 * s[5])
        g_go = (t["pred_global_orient"] - t["gt_global_orient"]) * (2 * s[6])
        x = t["pred_pose_6d"].reshape(-1, 3, 2)
        g_6d = (torch.matmul(x, torch.matmul(x.transpose(1, 2), x) - torch.eye(2, device=x.device)) * (4 * s[7] / 96)).reshape(B, 144)
        return g_pv, g_pj, g_pf, g_p2, g_go, g_bp, g_b, g_6d, s[8].expand(B)
    return call


def timed(call, reps):
    """(HIP-event microseconds per call over `reps` back-to-back calls, host microseconds to issue one call)."""
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    h0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    h1 = time.perf_counter()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, (h1 - h0) * 1e6 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1280])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    for B in a.batches:
        t = make_inputs(B, dev)
        gloss = torch.tensor([0.37], device=dev)
        bwd, keep_b = native_backward(t, gloss)
        fwd, keep_f = native_forward(t)
        eager = eager_backward(t, gloss)
        res = {}
        for _ in range(2):                                     # alternating: each of the three is measured twice, the second figures are reported
            for name, call in (("backward", bwd), ("forward", fwd), ("eager_backward", eager)):
                res[name] = timed(call, a.reps if name != "eager_backward" else max(a.reps // 10, 5))
        ref = eager()
        err = max(float((g - r).abs().max()) for g, r in zip([keep_b[2][k] for k in _lib.ValLossesBwdDesc.PREDICTIONS], ref))
        moved = 3 * 4 * B * V * 3
        us = res["backward"][0]
        print(json.dumps(dict(B=B, V=V, reps=a.reps, backward_us=us, backward_enqueue_us=res["backward"][1], forward_us=res["forward"][0],
                              forward_enqueue_us=res["forward"][1], eager_backward_us=res["eager_backward"][0], bytes_moved=moved,
                              backward_bytes_per_s=moved / (us * 1e-6), share_of_8TBps=moved / (us * 1e-6) / HBM_BYTES_PER_S,
                              forward_bytes_per_s=2 * 4 * B * V * 3 / (res["forward"][0] * 1e-6), max_abs_diff_to_eager=err)))


if __name__ == "__main__":
    main()
