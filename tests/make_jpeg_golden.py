"""Generates tests/golden/jpeg/*.jpg and tests/golden/jpeg_pixels.npz with PIL from seeded synthetic images (run by hand: python
tests/make_jpeg_golden.py; the tests read only the committed files, so a machine without PIL runs them).  jpeg_pixels.npz holds, per
fixture, PIL's decoded pixels as uint8 [H, W, 3] BGR: libjpeg's defaults (ISLOW IDCT, fancy upsampling), which is also what
cv2.imread(IMREAD_COLOR | IMREAD_IGNORE_ORIENTATION) gives - cv2 itself was never run against these files.
"""
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden", "jpeg")

# name: (H, W, mode, save options)                 subsampling 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0
FIXTURES = {
    "p17x9_420": (17, 9, "RGB", dict(quality=85, subsampling=2)),
    "p41x67_420": (41, 67, "RGB", dict(quality=85, subsampling=2)),
    "p56x72_420": (56, 72, "RGB", dict(quality=85, subsampling=2)),
    "p24x520_420": (24, 520, "RGB", dict(quality=85, subsampling=2)),
    "p33x50_422": (33, 50, "RGB", dict(quality=85, subsampling=1)),
    "p24x40_444": (24, 40, "RGB", dict(quality=85, subsampling=0)),
    "p40x40_gray": (40, 40, "L", dict(quality=85)),
    "p37x53_420_rst3": (37, 53, "RGB", dict(quality=85, subsampling=2, restart_marker_blocks=3)),
    "p56x72_420_opt": (56, 72, "RGB", dict(quality=85, subsampling=2, optimize=True)),
    "checker40x56_q30": (40, 56, "checker", dict(quality=30, subsampling=2)),
    "checker40x56_q10": (40, 56, "checker", dict(quality=10, subsampling=2)),
    "batch48x64_q50": (48, 64, "RGB", dict(quality=50, subsampling=2)),
    "batch48x64_q90": (48, 64, "RGB", dict(quality=90, subsampling=2)),
    "batch48x64_q98": (48, 64, "RGB", dict(quality=98, subsampling=2)),
    "p5x3_420": (5, 3, "RGB", dict(quality=85, subsampling=2)),          # chroma planes two samples wide: libjpeg replicates instead of filtering
    "p9x4_422": (9, 4, "RGB", dict(quality=85, subsampling=1)),
}
PROGRESSIVE = "progressive32x32"
BATCH = ("batch48x64_q50", "batch48x64_q90", "batch48x64_q98")


def synthetic(seed, H, W, mode):
    rng = np.random.default_rng(seed)
    if mode == "checker":
        c = ((np.arange(H)[:, None] + np.arange(W)[None, :]) & 1) * 255
        return np.repeat(c[:, :, None], 3, 2).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([128 + 100 * np.sin(x / (3.0 + k) + rng.uniform(0, 6)) * np.cos(y / (4.0 + 2 * k) + rng.uniform(0, 6)) for k in range(3)], -1)
    img += rng.normal(0, 12, img.shape)
    y0, x0 = H // 3, W // 3
    img[y0:y0 + max(H // 4, 1), x0:x0 + max(W // 4, 1)] = rng.uniform(0, 255, 3)      # a hard-edged patch: strong chroma steps
    img = np.clip(img, 0, 255).astype(np.uint8)
    return img[:, :, 0] if mode == "L" else img


def pil_decode_bgr(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def main():
    from PIL import Image
    os.makedirs(OUT, exist_ok=True)
    pixels = {}
    for seed, (name, (H, W, mode, opts)) in enumerate(FIXTURES.items()):
        img = synthetic(1000 + seed, H, W, mode)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", **opts)
        data = buf.getvalue()
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
        pixels[name] = pil_decode_bgr(data)
        assert pixels[name].shape == (H, W, 3)
    buf = io.BytesIO()
    Image.fromarray(synthetic(999, 32, 32, "RGB")).save(buf, "JPEG", quality=85, progressive=True)
    with open(os.path.join(OUT, PROGRESSIVE + ".jpg"), "wb") as f:
        f.write(buf.getvalue())
    np.savez_compressed(os.path.join(HERE, "golden", "jpeg_pixels.npz"), **pixels)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT)) + os.path.getsize(os.path.join(HERE, "golden", "jpeg_pixels.npz"))
    print(f"{len(pixels) + 1} files, {total} bytes")


if __name__ == "__main__":
    main()
