"""Time the mesh rasteriser (egohmr_amd.render, csrc/render.hip) at the reference's overlay shape: B = 32 bodies over 1920 x 1080 uint8 frames (8
resident frames shared by 4 items each), fx = 1500, bodies about 3 m away.  The synthetic SMPL asset's `faces` are random index triples, not a
surface, so the bodies are a real closed mesh of the SMPL counts - an ellipsoid of 83 stacks x 84 slices: 6890 vertices, 13 776 faces, a body's
1.7 m x 0.5 m x 0.3 m - each with its own rotation and translation.  Prints one JSON line:
  * ehm_render alone (colour only, smooth normals): device events around `iters` back-to-back calls of the entry on one prepared descriptor,
    `repeats` times; per body, with the HBM floor from the shapes (one frame read plus one image write per body, 2 x 3 H W bytes, at 8 TB/s)
    and the share of it the call reaches; the list capacity the items needed;
  * MeshRenderer.render as a whole (workspace allocation, the call, the one read-back of the needed capacities), wall clock.
`--clip-near 1` times the same case with the near-plane clipping on (no face crosses the plane there); `--scene` times one picture of a body inside
a room mesh around the camera instead, with the clipping off and on, and reports the list capacity needed and the share of pixels that change.
The per-kernel split comes from running this tool under `rocprofv3 --kernel-trace --stats` with a small --iters."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egohmr_amd import _lib  # noqa: E402
from egohmr_amd.render import MeshRenderer  # noqa: E402

HBM_BPS = 8e12


def ellipsoid(stacks=83, slices=84, axes=(0.25, 0.85, 0.15)):
    """A closed UV ellipsoid, its poles single vertices: 2 + (stacks - 1) slices vertices, 2 slices (stacks - 1) faces, wound outwards."""
    th = np.pi * np.arange(1, stacks) / stacks
    ph = 2 * np.pi * np.arange(slices) / slices
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones(slices)), np.outer(np.sin(th), np.sin(ph))], -1).reshape(-1, 3)
    v = np.concatenate([[[0.0, 1.0, 0.0]], ring, [[0.0, -1.0, 0.0]]], 0) * np.asarray(axes)
    at = lambda i, j: 1 + (i - 1) * slices + j % slices
    f = []
    for j in range(slices):
        f += [(0, at(1, j), at(1, j + 1)), (len(v) - 1, at(stacks - 1, j + 1), at(stacks - 1, j))]
    for i in range(1, stacks - 1):
        for j in range(slices):
            f += [(at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1))]
    f = np.asarray(f, np.int32)
    if np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() < 0:
        f = f[:, ::-1].copy()
    return v.astype(np.float32), f


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


def room(n=20, lo=(-3.0, -1.6, -2.5), hi=(3.5, 1.3, 5.0)):
    """A closed box around the camera, every wall an n x n grid of quads: 6 (n + 1)^2 vertices, 12 n^2 faces, slightly turned.  The walls beside,
    above and below the camera pass behind it, so a band of their faces straddles the near plane."""
    lo, hi = np.asarray(lo), np.asarray(hi)
    s = np.linspace(0.0, 1.0, n + 1)
    a, b = np.meshgrid(s, s, indexing="ij")
    verts, faces = [], []
    for axis in range(3):
        for side in (0.0, 1.0):
            p = np.empty((n + 1, n + 1, 3))
            p[..., axis] = side
            p[..., (axis + 1) % 3], p[..., (axis + 2) % 3] = a, b
            base = len(verts) * (n + 1) ** 2
            at = lambda i, j: base + i * (n + 1) + j
            verts.append((lo + p * (hi - lo)).reshape(-1, 3))
            faces += [t for i in range(n) for j in range(n) for t in ((at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1)))]
    c, sn = math.cos(0.1), math.sin(0.1)
    v = np.concatenate(verts, 0) @ np.array([[c, 0, sn], [0, 1, 0], [-sn, 0, c]]).T
    return v.astype(np.float32), np.asarray(faces, np.int32)


def scene_case(args, dev):
    """render_in_scene's shape: one 1920 x 1080 picture of a body inside a room mesh, with clip_near off and on.  Prints one JSON line."""
    from egohmr_amd.render import scene_renderer
    g = np.random.default_rng(1)
    H, W = 1080, 1920
    bv, bf = ellipsoid()
    sv, sf = room(args.room_grid)
    sc = g.uniform(0.2, 1.0, (len(sv), 3)).astype(np.float32)
    verts = torch.from_numpy(np.concatenate([bv + np.float32([0.2, 0.3, 2.8]), sv], 0)[None]).to(dev)
    cams = [torch.full((1,), x, device=dev) for x in (1500.0, 1500.0, 960.0, 540.0)]
    A, stream = _lib.api(), _lib.stream_ptr()
    res, pics = {}, {}
    for flag in (False, True):
        r = scene_renderer(bf, len(bv), sf, sc, dev, two_sided=True, clip_near=flag)
        out = r.render(verts, 1500.0, 1500.0, 960.0, 540.0, size=(H, W), bg_color=(255, 255, 255), want=("color", "face_index"), bgr=True)      # (settles the capacity)
        color, needed = torch.empty(1, H, W, 3, dtype=torch.uint8, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        d = r._desc(verts, *cams, None, None, H, W, (255, 255, 255), True, {"color": color}, needed, r.bin_capacity)
        n = C.c_int64(0)
        A.ehm_render_workspace_bytes(C.byref(d), C.byref(n))
        ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
        d.workspace, d.workspace_bytes = ws.data_ptr(), n.value
        entry = lambda: A.ehm_render(C.byref(d), stream)
        for _ in range(3):
            entry()
        torch.cuda.synchronize()
        assert torch.equal(color, out["color"])
        ms = events_ms(entry, args.iters, args.repeats)
        pics[flag] = out
        res["clip_near" if flag else "dropped"] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                                                   "needed_capacity": int(needed.max()), "reruns_of_first_call": r.reruns,
                                                   "background_share_of_pixels": round(float((out["face_index"] < 0).float().mean()), 4)}
    changed = float((pics[False]["color"] != pics[True]["color"]).any(-1).float().mean())
    print(json.dumps({"case": f"render_in_scene shape: a body of {len(bf)} faces in a room of {len(sf)} faces around the camera, {W}x{H}, per-vertex colours",
                      **res, "share_of_pixels_that_change": round(changed, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--clip-near", type=int, default=0, help="the body case with MeshRenderer(clip_near=...): no face crosses, the time should not move")
    ap.add_argument("--scene", action="store_true", help="time a body inside a room mesh around the camera, clip_near off and on, instead")
    ap.add_argument("--room-grid", type=int, default=20, help="quads per wall edge of the room: 12 n^2 faces")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.scene:
        return scene_case(args, dev)
    g = np.random.default_rng(0)
    B, Fr, H, W = args.batch, 8, 1080, 1920
    v, f = ellipsoid()
    assert v.shape == (6890, 3) and f.shape == (13776, 3)
    verts = np.empty((B, len(v), 3), np.float32)
    for b in range(B):
        a, c = g.uniform(-0.4, 0.4), g.uniform(-math.pi, math.pi)
        rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
        ry = np.array([[math.cos(c), 0, math.sin(c)], [0, 1, 0], [-math.sin(c), 0, math.cos(c)]])
        verts[b] = v @ (rz @ ry).T + (np.array([0.0, 0.0, 3.0]) + g.uniform(-0.5, 0.5, 3))
    verts = torch.from_numpy(verts).to(dev)
    frames = torch.from_numpy(g.integers(0, 256, (Fr, H, W, 3), dtype=np.uint8)).to(dev)
    fidx = torch.from_numpy((np.arange(B) % Fr).astype(np.int32)).to(dev)
    r = MeshRenderer(f, dev, num_vertices=len(v), **({"clip_near": True} if args.clip_near else {}))
    call = lambda: r.render(verts, 1500.0, 1500.0, 960.0, 540.0, frames=frames, frame_index=fidx, bgr=True, want=("color", "face_index"))
    out = call()                                              # (settles the list capacity)
    covered = float((out["face_index"] >= 0).float().mean())
    # the entry alone, on one prepared descriptor
    cams = [torch.full((B,), x, device=dev) for x in (1500.0, 1500.0, 960.0, 540.0)]
    color, needed = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    d = r._desc(verts, *cams, frames, fidx, H, W, (0, 0, 0), True, {"color": color}, needed, r.bin_capacity)
    n = C.c_int64(0)
    A = _lib.api()
    A.ehm_render_workspace_bytes(C.byref(d), C.byref(n))
    ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n.value
    stream = _lib.stream_ptr()
    entry = lambda: A.ehm_render(C.byref(d), stream)
    for _ in range(3):
        entry()
    torch.cuda.synchronize()
    assert torch.equal(color, out["color"]) and int(needed.max()) <= r.bin_capacity
    ms = events_ms(entry, args.iters, args.repeats)
    med = statistics.median(ms)
    floor_bytes = 2 * 3 * H * W
    wall = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"clip_near": int(bool(args.clip_near)), "case": f"ehm_render B={B} bodies of {len(v)} vertices / {len(f)} faces over {Fr} shared {W}x{H} frames, colour, smooth normals",
                      "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                      "us_per_body": round(med * 1e3 / B, 2), "hbm_floor_us_per_body_at_8TBps": round(floor_bytes / HBM_BPS * 1e6, 3),
                      "share_of_hbm_floor": round(floor_bytes * B / (med * 1e-3) / HBM_BPS, 4), "covered_share_of_pixels": round(covered, 4),
                      "needed_capacity_max": int(needed.max()), "bin_capacity": r.bin_capacity, "reruns_of_first_call": r.reruns,
                      "workspace_MiB": round(n.value / 2 ** 20, 1),
                      "MeshRenderer_render_wall_ms_median": round(statistics.median(wall), 3)}), flush=True)


if __name__ == "__main__":
    main()
