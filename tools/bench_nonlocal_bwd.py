#!/usr/bin/env python3
"""Time ehm_nonlocal_attention_backward (csrc/nonlocal_bwd.hip) and, beside it, the forward kernel on the same inputs: HIP events around `--calls` back-to-back
launches after `--warmup` ones, `--rounds` times; the median round, per call, and the GB/s it implies for the bytes each call must move at least once
(backward: qkv + gy read, gqkv written; forward: qkv read, y written).  One JSON line.

    python tools/bench_nonlocal_bwd.py [--bodies 256] [--ci 512]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egohmr_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=256)
    ap.add_argument("--ci", type=int, default=512)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    A = _lib.api()
    rows, Ci = a.bodies * 24, a.ci
    g = torch.Generator(device=dev).manual_seed(0)
    s = (3.0 / Ci ** 0.5) ** 0.5
    qkv = torch.cat([torch.randn(rows, Ci, generator=g, device=dev) * s, torch.randn(rows, Ci, generator=g, device=dev) * s,
                     torch.randn(rows, Ci, generator=g, device=dev)], 1).contiguous()
    gy = torch.randn(rows, Ci, generator=g, device=dev)
    gqkv, y = torch.empty(rows, 3 * Ci, device=dev), torch.empty(rows, Ci, device=dev)
    st = _lib.stream_ptr()
    entries = {"backward": (lambda: A.ehm_nonlocal_attention_backward(qkv, gy, gqkv, a.bodies, Ci, st), 4 * rows * Ci * 7),
               "forward": (lambda: A.ehm_nonlocal_attention(qkv, y, a.bodies, Ci, st), 4 * rows * Ci * 4)}
    out = dict(bodies=a.bodies, Ci=Ci, calls=a.calls, rounds=a.rounds)
    with _lib.on_device(dev):
        for name, (call, nbytes) in entries.items():
            for _ in range(a.warmup):
                call()
            torch.cuda.synchronize()
            us = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    call()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / a.calls)
            med = statistics.median(us)
            out[name] = dict(us_per_call=round(med, 2), us_min=round(min(us), 2), us_max=round(max(us), 2), min_bytes=nbytes, GBps=round(nbytes / med * 1e-3, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
