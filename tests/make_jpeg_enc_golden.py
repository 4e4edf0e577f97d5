"""Generates tests/golden/jpeg_enc.npz with PIL (libjpeg-turbo) from seeded synthetic images (run by hand: python
tests/make_jpeg_enc_golden.py; the tests read only the committed file, so a machine without PIL runs them).  Per fixture it holds
<name>_rgb (the uint8 [H, W, 3] RGB input), <name>_meta (quality, hmax, vmax) and <name>_jpg (the bytes PIL wrote with optimize=False, i.e.
with the fixed Annex K Huffman tables).  cv2.imwrite uses the same libjpeg defaults; cv2 itself was never run.
"""
import io
import os

import numpy as np

from make_jpeg_golden import synthetic

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden", "jpeg_enc.npz")

# name: (H, W, sampling, quality, kind)
FIXTURES = {
    "p5x3_420_q75": (5, 3, "4:2:0", 75, "RGB"),
    "p8x8_420_q95": (8, 8, "4:2:0", 95, "RGB"),               # one MCU: a dummy luma column, a dummy luma row and the block that is both
    "p24x40_420_q10": (24, 40, "4:2:0", 10, "RGB"),           # a dummy luma row and a dummy luma column
    "p41x67_420_q75": (41, 67, "4:2:0", 75, "RGB"),           # a dummy luma column only
    "p9x4_422_q95": (9, 4, "4:2:2", 95, "RGB"),
    "p33x50_422_q75": (33, 50, "4:2:2", 75, "RGB"),
    "p24x40_444_q100": (24, 40, "4:4:4", 100, "RGB"),
    "noise24x40_420_q100": (24, 40, "4:2:0", 100, "noise"),   # many FF bytes in the packed stream
    "flat16x24_420_q75": (16, 24, "4:2:0", 75, "flat"),       # EOB-only blocks, DC differences of zero
}
SAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
PIL_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def image(seed, H, W, kind):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(np.uint8([200, 90, 30]), (H, W, 3)).copy()
    return synthetic(seed, H, W, kind)


def pil_encode(rgb, quality, sampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling=PIL_SUBSAMPLING[sampling], optimize=False)
    return buf.getvalue()


def load(path=OUT):
    """-> {name: (rgb, quality, (hmax, vmax), jpg bytes)}"""
    z = np.load(path)
    return {n: (z[n + "_rgb"], int(z[n + "_meta"][0]), (int(z[n + "_meta"][1]), int(z[n + "_meta"][2])), z[n + "_jpg"].tobytes()) for n in FIXTURES}


def main():
    arrays = {}
    for seed, (name, (H, W, sampling, quality, kind)) in enumerate(FIXTURES.items()):
        rgb = image(2000 + seed, H, W, kind)
        arrays[name + "_rgb"] = rgb
        arrays[name + "_meta"] = np.int32([quality, *SAMPLINGS[sampling]])
        arrays[name + "_jpg"] = np.frombuffer(pil_encode(rgb, quality, sampling), np.uint8)
    np.savez_compressed(OUT, **arrays)
    print(f"{len(FIXTURES)} fixtures, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
