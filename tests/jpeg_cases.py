"""Seeded synthetic inputs for the three JPEG device kernels (csrc/jpeg.hip: jpeg_idct_kernel, jpeg_colour_kernel; csrc/jpeg_enc.hip:
jpeg_forward_kernel), away from what PIL's encoder emits: a separate quantisation row for every frame and component, sizes off the 8-pixel
grid, every chroma width around the replicate threshold and the fast / clamped switch of chroma_row6, one and two chroma rows, samples and
colours far outside 0...255, padding blocks with content of their own, several frames per call.  tests/test_jpeg_cases_cpu.py proves what the
set claims (every case inside the exact int32 domain, every planted mistake of the two references caught); tests/test_gpu_jpeg_kernels.py
runs the kernels on it.  Everything is numpy and deterministic: a case's seed is the CRC of its id.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

import jpeg_enc_ref as enc_ref
import jpeg_ref

SAMPLINGS = {"gray": (1, 1, 1), "444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2)}     # name -> (components, hmax, vmax)
SQUARE = [(1, 1), (3, 5), (8, 8), (8, 16), (9, 17), (16, 23)]                             # gray and 4:4:4
# chroma widths 1, 1, 2, 2, 3, 3, 4, 5, 8, 9, 9, 12, 13, 13: both sides of the replicate threshold (cw <= 2); cw 9 and 13, where the last
# octet's chroma_row6 reads index cw - 1 on the fast path; cw 8 and 12, where it takes the clamped path; both parities of the MCU count
WIDTHS = [1, 2, 3, 4, 5, 6, 8, 10, 16, 17, 18, 24, 25, 26]
HEIGHTS = {"422": [1, 8, 9], "420": [1, 2, 3, 4, 15, 16, 17]}                             # 4:2:0: ch 1, 1, 2, 2, 8, 8, 9
CONTENTS = ("dense", "sparse_extreme", "encoded")
# (sampling, H, W): blocks per frame 6, 18, 16, 12 - no multiple of the 32 blocks of a workgroup, so a workgroup spans frames
MULTI = [("gray", 9, 17), ("444", 9, 17), ("422", 9, 25), ("420", 17, 9)]
FORWARD_CONTENTS = ("noise", "saturated", "constant")


def geometries():
    """[(sampling, H, W)]"""
    out = [(s, H, W) for s in ("gray", "444") for H, W in SQUARE]
    return out + [(s, H, W) for s in ("422", "420") for H in HEIGHTS[s] for W in WIDTHS]


def _rng(case_id):
    return np.random.default_rng(zlib.crc32(case_id.encode()))


def _tables(rng, F, top=255):
    """uint16 [F, 3, 64], entries 1...top: another row for every frame and component"""
    while True:
        q = rng.integers(1, top + 1, (F, 3, 64)).astype(np.uint16)
        if len({r.tobytes() for r in q.reshape(-1, 64)}) == 3 * F:
            return q


def _quantised(target, q):
    """The int16 coefficient whose product with q is nearest target, never 0 where target is not"""
    c = np.rint(target / q).astype(np.int64)
    return np.where((c == 0) & (target != 0), np.sign(target), c).astype(np.int16)


def _dense(rng, grids, quant):
    """All 64 coefficients non-zero, |coef q| <= 512"""
    planes = []
    for c, (by, bx) in enumerate(grids):
        top = 512 // quant[c].astype(np.int64)                                            # >= 2 for q <= 255
        mag = rng.integers(1, top + 1, (by, bx, 64))
        planes.append((mag * rng.choice([-1, 1], mag.shape)).astype(np.int16))
    return planes


def _sample00(block, q):
    return int(jpeg_ref.idct_samples(block[None, None], q)[0, 0])


def _sparse_extreme(rng, grids, quant):
    """A DC and two or three AC per block with dequantised magnitudes of 2000 ... 8000: samples of several hundred on both sides of 0...255.
    The three blocks that cover pixel (0, 0) are built, not drawn, so that even a 1 x 1 frame drives the colour conversion out of range on
    both sides: every DCT basis function is positive at (0, 0), so all-positive coefficients put the block's maximum there and all-negative
    ones its minimum.  Cb is all-positive (B = Y + 226 at the clamp), Cr all-negative (R = Y - 179), and the luma block carries (0, 1) and
    (1, 0) with opposite signs and the DC that brings its sample (0, 0) nearest 128 (within q / 16 <= 16)."""
    planes = []
    for c, (by, bx) in enumerate(grids):
        p = np.zeros((by, bx, 64), np.int16)
        for y in range(by):
            for x in range(bx):
                at = np.concatenate([[0], rng.choice(np.arange(1, 64), rng.integers(2, 4), replace=False)])
                target = rng.integers(2000, 8001, at.size) * rng.choice([-1, 1], at.size)
                p[y, x, at] = _quantised(target, quant[c, at].astype(np.int64))
        q = quant[c].astype(np.int64)
        first = np.zeros(64, np.int16)
        if c == 0:
            first[[1, 8]] = _quantised(np.array([6000, -6000]), q[[1, 8]])
            if len(grids) == 3:
                first[0] = np.rint((128 - _sample00(first, quant[c])) * 8 / q[0])
            else:
                first[0] = _quantised(np.array(3000), q[0])
        else:
            sign = 1 if c == 1 else -1
            first[[0, 1, 8, 9]] = _quantised(sign * np.array([2000, 7000, 5000, 3000]), q[[0, 1, 8, 9]])
        p[0, 0] = first
        planes.append(p)
    return planes


def _encoded(rng, H, W, components, hmax, vmax, quant):
    """jpeg_enc_ref's coefficients of a noise image: an encoder's statistics, dummy blocks with a replicated DC"""
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    planes = enc_ref.coefficient_planes(rgb, quant, hmax, vmax)
    return planes[:components]


@functools.lru_cache(maxsize=None)
def decode_cases():
    """[(id, case)]: case has sampling, content, H, W, components, hmax, vmax, F, coef int16 [F, coef_count], quant uint16 [F, 3, 64]."""
    todo = [(s, H, W, 1, content) for s, H, W in geometries() for content in CONTENTS]
    todo += [(s, H, W, F, content) for s, H, W in MULTI for F in (2, 5) for content in CONTENTS]
    out = []
    for s, H, W, F, content in todo:
        case_id = f"{s}-{H}x{W}-{content}" + (f"-F{F}" if F > 1 else "")
        rng = _rng(case_id)
        components, hmax, vmax = SAMPLINGS[s]
        grids = jpeg_ref.block_grids(H, W, components, hmax, vmax)
        quant = _tables(rng, F)
        frames = []
        for f in range(F):
            if content == "dense":
                planes = _dense(rng, grids, quant[f])
            elif content == "sparse_extreme":
                planes = _sparse_extreme(rng, grids, quant[f])
            else:
                planes = _encoded(rng, H, W, components, hmax, vmax, quant[f])
            frames.append(np.concatenate([p.reshape(-1) for p in planes]))
        out.append((case_id, dict(sampling=s, content=content, H=H, W=W, components=components, hmax=hmax, vmax=vmax, F=F,
                                  coef=np.stack(frames), quant=quant, blocks=sum(a * b for a, b in grids))))
    return out


def decode_want(case, wrong=None, dtype=np.int64, detail=None):
    """-> (planes uint8 [F, coef_count]: the workspace, pixels uint8 [F, H, W, 3]) of jpeg_ref.planes_and_pixels; detail: a list that
    receives one dict per frame."""
    planes, pixels = [], []
    for f in range(case["F"]):
        d = None if detail is None else {}
        p, px = jpeg_ref.planes_and_pixels(case["coef"][f], case["quant"][f], case["H"], case["W"], case["components"], case["hmax"],
                                           case["vmax"], wrong=wrong, quant0=case["quant"][0], dtype=dtype, detail=d)
        planes.append(np.concatenate([a.reshape(-1) for a in p]))
        pixels.append(px)
        if detail is not None:
            detail.append(d)
    return np.stack(planes), np.stack(pixels)


def _frame(rng, content, H, W):
    if content == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if content == "saturated":
        return (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    return np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (H, W, 3)).copy()


@functools.lru_cache(maxsize=None)
def forward_cases():
    """[(id, case)]: case has sampling, content, H, W, hmax, vmax, F, rgb (the flag of ehm_jpeg_forward), frames uint8 [F, H, W, 3], quant
    uint16 [F, 3, 64].  Every geometry but the gray ones takes all three contents; (F, rgb) rotates through its four combinations along the
    geometries, so every (sampling, content) meets all four."""
    out, combos = [], [(1, 0), (3, 1), (1, 1), (3, 0)]
    for g, (s, H, W) in enumerate(x for x in geometries() if x[0] != "gray"):
        for ci, content in enumerate(FORWARD_CONTENTS):
            F, rgb = combos[(g + ci) % 4]
            case_id = f"{s}-{H}x{W}-{content}-F{F}-{'rgb' if rgb else 'bgr'}"
            rng = _rng(case_id)
            _, hmax, vmax = SAMPLINGS[s]
            quant = _tables(rng, F, 16 if content == "saturated" else 255)     # saturated content over small entries: the largest coefficients
            frames = np.stack([_frame(rng, content, H, W) for _ in range(F)])
            out.append((case_id, dict(sampling=s, content=content, H=H, W=W, hmax=hmax, vmax=vmax, F=F, rgb=rgb, frames=frames, quant=quant)))
    return out


def forward_want(case, wrong=None):
    """-> int16 [F, coef_count] of jpeg_enc_ref.coefficients with the [3, 64] rows"""
    out = []
    for f in range(case["F"]):
        rgb = case["frames"][f] if case["rgb"] else case["frames"][f][..., ::-1]
        out.append(enc_ref.coefficients(rgb, case["quant"][f], case["hmax"], case["vmax"], wrong=wrong, quant0=case["quant"][0]))
    return np.stack(out)
