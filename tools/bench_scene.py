"""Time ehm_scene_select (egohmr_amd.scene.SceneClouds.cube) at B = 256 items, target 20 000, on synthetic 2^21-vertex meshes: one mesh (50 MB
of float64 vertices, inside the Infinity Cache) and eight meshes (32 items each).  Prints one JSON line per case: the native call alone
(device events around back-to-back calls: its 5 launches, no host work) and the whole Python call (parameters on the host, upload, status
read-back), with the bytes the three vertex-reading passes (ymin, count, scatter) read at the group reuse of 8 items per vertex load."""
import argparse
import json
import os
import sys
import time

import ctypes as C
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egohmr_amd import _lib, scene as es  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--verts", type=int, default=2**21)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = np.random.default_rng(0)
    B, target = 256, 20000
    for M in (1, 8):
        meshes = [np.stack([g.uniform(-3, 3, args.verts), g.uniform(0, 3, args.verts), g.uniform(-3, 3, args.verts)], -1) for _ in range(M)]
        sc = es.SceneClouds(meshes, dev)
        mi = np.arange(B) % M
        crop = np.tile(np.eye(4), (B, 1, 1))
        tp = g.uniform(-1.5, 1.5, (B, 3)).astype(np.float32)
        ang = g.uniform(0, 2 * np.pi, B)
        sc.cube(mi, tp, crop, crop, angle=ang, target=target)                  # warm-up (and a check that every item succeeds)
        params = es.cube_params(tp, crop, crop, ang, 2, B)
        with _lib.on_device(dev):
            st = _lib.stream_ptr()
            d, out = sc._prepare(es.CUBE, mi, params, 0, target, 1, False)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                _lib.api().ehm_scene_select(C.byref(d), st)
            e1.record()
            torch.cuda.synchronize()
        native_ms = e0.elapsed_time(e1) / args.iters
        t0 = time.perf_counter()
        for _ in range(args.iters):
            sc.cube(mi, tp, crop, crop, angle=ang, target=target)
        torch.cuda.synchronize()
        call_ms = (time.perf_counter() - t0) * 1e3 / args.iters
        groups = len(es.group_items(mi))
        pass_bytes = groups * args.verts * 24                                   # each group block reads its tile's vertices once per pass
        print(json.dumps({"case": f"cube B={B} target={target} meshes={M} x {args.verts} verts", "native_ms": round(native_ms, 4),
                          "python_call_ms": round(call_ms, 3), "groups": groups, "bytes_per_pass": pass_bytes, "passes": 3,
                          "achieved_GBps_3_passes": round(3 * pass_bytes / native_ms / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
