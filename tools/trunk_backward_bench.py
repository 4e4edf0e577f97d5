#!/usr/bin/env python3
"""The autograd route of ResNet50Features.__call__ (egohmr_amd/trunk_grad.py, csrc/conv_bwd.hip; BatchNorm in eval mode) at B = 64, 224 x 224, trained-like
synthetic weights, next to this repository's own no-graph forward and to the eager float32 torch autograd of the same graph (tools/_eager.py) on the same device:
    python tools/trunk_backward_bench.py [--reps 5] [--warmup 2] [--batch 64] [--size 224] [--no-eager] [--profile] [--train-bn]
fwd       = the folded no-graph forward (what sampling runs)
fwd_save  = the forward of the autograd route (keeps every conv's X2 output)
fwd_bwd   = fwd_save + the backward with all 159 parameter gradients
The modes alternate, every iteration is timed with HIP events of its own, the medians are reported.  --profile adds the backward's HIP-event time per
kernel family of one iteration (a synchronise per call: a breakdown, not a total) and the weight-gradient time per conv shape.  Prints one JSON line.
--train-bn adds the batch-statistics route (ResNet50Features.train_batchnorm under .train(), csrc/bn2d_train.hip) beside the others:
train_fwd = its no-graph forward, train_fwd_save = the forward of its autograd route (keeps every unit's raw conv output too), train_fwd_bwd = that +
the backward through the mean and the variance; the eval-mode modes run with the module in eval mode as before."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from _eager import resnet50_eager  # noqa: E402
from egohmr_amd import synthetic as syn, trunk_grad  # noqa: E402
from egohmr_amd.encoders import ResNet50Features  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--train-bn", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    B = a.batch
    m = ResNet50Features()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_state_dict(0, manifest=syn._resnet50_manifest("")).items()})
    m = m.to(dev).eval()
    g = torch.Generator(device="cpu").manual_seed(0)
    img = torch.randn(B, 3, a.size, a.size, generator=g).to(dev)
    cot = torch.randn(B, 2048, generator=g).to(dev)

    def clear():
        m.zero_grad(set_to_none=True)

    def fwd():
        m.grad_params = False
        m(img)

    def fwd_save():
        m.grad_params = True
        m(img)

    def fwd_bwd():
        m.grad_params = True
        m(img).backward(cot)
        clear()

    def eager_fwd():
        with torch.no_grad():
            resnet50_eager(m, img)

    def eager_fwd_bwd():
        resnet50_eager(m, img).backward(cot)
        clear()

    def in_train(fn):
        def call():
            m.train()
            m.train_batchnorm = True
            try:
                fn()
            finally:
                m.train_batchnorm = False
                m.eval()
        return call

    def train_fwd():
        m.grad_params = False
        with torch.no_grad():
            m(img)

    modes = dict(fwd=fwd, fwd_save=fwd_save, fwd_bwd=fwd_bwd)
    if not a.no_eager:
        modes.update(eager_fwd=eager_fwd, eager_fwd_bwd=eager_fwd_bwd)
    # the train-mode calls move the running statistics, after which an eval-mode call folds again: they alternate among themselves, behind the others
    groups = [modes] + ([dict(train_fwd=in_train(train_fwd), train_fwd_save=in_train(fwd_save), train_fwd_bwd=in_train(fwd_bwd))] if a.train_bn else [])
    ms, peak = {}, {}
    for group in groups:
        for _ in range(a.warmup):
            for fn in group.values():
                fn()
        torch.cuda.synchronize()
        m.check_status()
        ms.update({k: [] for k in group})
        for _ in range(a.reps):
            for k, fn in group.items():
                torch.cuda.reset_peak_memory_stats()
                ms[k].append(timed(fn))
                peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated())
    med = {k: statistics.median(v) for k, v in ms.items()}
    acts = []
    m.grad_params = False
    m.current()(img, saved=acts)
    torch.cuda.synchronize()
    saved = sum(buf.numel() for buf, _ in acts)
    res = dict(batch=B, size=a.size, reps=a.reps, warmup=a.warmup, ms={k: round(v, 3) for k, v in med.items()}, ms_min={k: round(min(v), 3) for k, v in ms.items()},
               backward_ms=round(med["fwd_bwd"] - med["fwd_save"], 3), backward_over_forward=round((med["fwd_bwd"] - med["fwd_save"]) / med["fwd"], 3),
               saved_values_per_image=saved // B, saved_gib=round(saved * 4 / 2 ** 30, 3), peak_allocated_gib={k: round(v / 2 ** 30, 2) for k, v in peak.items()})
    if a.train_bn:
        rec = trunk_grad.train_forward(m, img)[1]
        torch.cuda.synchronize()
        kept = sum(buf.numel() for buf, _ in rec.acts) + sum(e[0].numel() for e in rec.bn if e is not None and e[0] is not None)
        res.update(train_backward_ms=round(med["train_fwd_bwd"] - med["train_fwd_save"], 3), train_saved_values_per_image=kept // B,
                   train_saved_gib=round(kept * 4 / 2 ** 30, 3))
    if not a.no_eager:
        res["eager_backward_ms"] = round(med["eager_fwd_bwd"] - med["eager_fwd"], 3)
        res["fwd_bwd_speedup_over_eager"] = round(med["eager_fwd_bwd"] / med["fwd_bwd"], 3)
    if a.profile:
        res["backward_stage_ms"], res["wgrad_ms_by_shape"] = profile_backward(m, img, cot)
    print(json.dumps(res))


def profile_backward(m, img, cot):
    """HIP-event time of the helpers of trunk_grad inside one backward, wrapped for this one call (a synchronise after each, so the sum exceeds the
    asynchronous backward), and the weight-gradient calls grouped by (pixels, Ci, Co, K, stride)."""
    acc, shapes = {}, {}

    def wrap(name, fn, shape_of=None):
        def call(*args, **kw):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*args, **kw)
            e1.record()
            torch.cuda.synchronize()
            dt = e0.elapsed_time(e1)
            acc[name] = acc.get(name, 0.0) + dt
            if shape_of is not None:
                k = shape_of(*args, **kw)
                shapes[k] = shapes.get(k, 0.0) + dt
            return r
        return call

    m.grad_params = True
    out = m(img)
    names = ("gate", "wgrad", "dgrad", "stem_backward", "pow2_scale", "unfold")
    keep = {n: getattr(trunk_grad, n) for n in names}
    wg_shape = lambda G, x, in_shape, Ci, Co, K, stride, pad, *r, **k: f"{G.shape[0] * G.shape[1] * G.shape[2]}px {Ci}->{Co} k{K} s{stride}"
    try:
        for n in names:
            setattr(trunk_grad, n, wrap(n, keep[n], wg_shape if n == "wgrad" else None))
        total = timed(lambda: out.backward(cot))
    finally:
        for n in names:
            setattr(trunk_grad, n, keep[n])
    m.zero_grad(set_to_none=True)
    acc["whole backward, synchronised per call"] = total
    rnd = lambda d: {k: round(v, 3) for k, v in sorted(d.items(), key=lambda kv: -kv[1])}
    return rnd(acc), rnd(shapes)


if __name__ == "__main__":
    main()
