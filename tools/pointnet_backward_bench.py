#!/usr/bin/env python3
"""The autograd route of ResnetPointnet.forward (egohmr_amd/pointnet_grad.py, csrc/pointnet_bwd.hip) at the headline shape B = 256, N = 4096, H = 256,
next to the eager float32 torch autograd of the same graph (tools/_eager.py) on the same device:
    python tools/pointnet_backward_bench.py [--reps 5] [--warmup 2] [--batch 256] [--points 4096] [--hidden 256] [--profile]
fwd       = the chained no-grad forward (what sampling runs)
fwd_save  = the forward of the autograd route (keeps every block's relu(h) and net)
fwd_bwd   = fwd_save + the backward with all 24 parameter gradients and the gradient to the points
The modes alternate, every iteration is timed with HIP events of its own, the medians are reported.  --profile adds the backward's HIP-event time per
stage of one iteration (a synchronise per stage: a breakdown, not a total).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from _eager import resnet_pointnet_eager  # noqa: E402
from egohmr_amd import pointnet_grad, synthetic as syn  # noqa: E402
from egohmr_amd.encoders import ResnetPointnet  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--out-dim", type=int, default=512)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    B, N, H = a.batch, a.points, a.hidden
    man = [("scene_enc.fc_pos_0.weight", (2 * H, 3)), ("scene_enc.fc_pos_0.bias", (2 * H,))]           # synthetic.egohmr_manifest's scene_enc.* rows at width H
    for b in range(4):
        q = f"scene_enc.block_{b}."
        man += [(q + "fc_0.weight", (H, 2 * H)), (q + "fc_0.bias", (H,)), (q + "fc_1.weight", (H, H)), (q + "fc_1.bias", (H,)), (q + "shortcut.weight", (H, 2 * H))]
    man += [("scene_enc.fc_c.weight", (a.out_dim, H)), ("scene_enc.fc_c.bias", (a.out_dim,))]
    m = ResnetPointnet(out_dim=a.out_dim, hidden_dim=H)
    m.load_state_dict({k[len("scene_enc."):]: torch.from_numpy(v) for k, v in syn.make_state_dict(0, manifest=man).items()})
    m = m.to(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    p = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(dev)
    cot = torch.randn(B, a.out_dim, generator=g).to(dev)

    def clear():
        m.zero_grad(set_to_none=True)

    def fwd():
        m.grad_params = False
        with torch.no_grad():
            m(p)

    def fwd_save():
        m.grad_params = True
        m(p.detach().requires_grad_())

    def fwd_bwd():
        m.grad_params = True
        q = p.detach().requires_grad_()
        m(q).backward(cot)
        clear()

    def eager_fwd():
        with torch.no_grad():
            resnet_pointnet_eager(m, p)

    def eager_fwd_bwd():
        q = p.detach().requires_grad_()
        resnet_pointnet_eager(m, q).backward(cot)
        clear()

    modes = dict(fwd=fwd, fwd_save=fwd_save, fwd_bwd=fwd_bwd)
    if not a.no_eager:
        modes.update(eager_fwd=eager_fwd, eager_fwd_bwd=eager_fwd_bwd)
    for _ in range(a.warmup):
        for fn in modes.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in modes}
    for _ in range(a.reps):
        for k, fn in modes.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = dict(batch=B, points=N, hidden=H, out_dim=a.out_dim, reps=a.reps, warmup=a.warmup,
               ms={k: round(v, 3) for k, v in med.items()}, ms_min={k: round(min(v), 3) for k, v in ms.items()},
               backward_ms=round(med["fwd_bwd"] - med["fwd_save"], 3),
               backward_over_forward=round((med["fwd_bwd"] - med["fwd_save"]) / med["fwd"], 3),
               saved_bytes_per_point=8 * H * 4, peak_allocated_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    if not a.no_eager:
        res["eager_backward_ms"] = round(med["eager_fwd_bwd"] - med["eager_fwd"], 3)
        res["fwd_bwd_speedup_over_eager"] = round(med["eager_fwd_bwd"] / med["fwd_bwd"], 3)
    if a.profile:
        res["backward_stage_ms"] = profile_backward(m, p, cot)
    print(json.dumps(res))


def profile_backward(m, p, cot):
    """HIP-event time of every native entry and torch op family inside one backward: the entries of _lib.api() and the helpers of pointnet_grad are
    wrapped for this one call (a synchronise after each, so the sum exceeds the asynchronous backward)."""
    from egohmr_amd import _lib
    acc = {}

    def wrap(name, fn):
        def call(*args, **kw):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*args, **kw)
            e1.record()
            torch.cuda.synchronize()
            acc[name] = acc.get(name, 0.0) + e0.elapsed_time(e1)
            return r
        return call

    m.grad_params = True
    q = p.detach().requires_grad_()
    out = m(q)
    api = _lib.api()
    names = [n for n in vars(api) if n.startswith("ehm_pointnet_") or n in ("ehm_split_pack", "ehm_skinny_gemm_f32")]
    keep = {n: getattr(api, n) for n in names}
    keep_rows, keep_scale = pointnet_grad.gemm_rows, pointnet_grad.pow2_scale
    try:
        for n in names:
            setattr(api, n, wrap(n, keep[n]))
        pointnet_grad.gemm_rows = wrap("gemm_rows (ehm_conv_nhwc_split)", keep_rows)
        pointnet_grad.pow2_scale = wrap("pow2_scale", keep_scale)
        total = timed(lambda: out.backward(cot))
    finally:
        for n in names:
            setattr(api, n, keep[n])
        pointnet_grad.gemm_rows, pointnet_grad.pow2_scale = keep_rows, keep_scale
    m.zero_grad(set_to_none=True)
    acc["whole backward, synchronised per stage"] = total
    return {k: round(v, 3) for k, v in sorted(acc.items(), key=lambda kv: -kv[1])}


if __name__ == "__main__":
    main()
