"""JPEG encoding, measured: python tools/jpeg_encode_bench.py [--frames 32] [--repeats 5] [--calls 10] [--kernels-only]

Inputs, synthesised from a seed on the device's host: F rendered-like 1920 x 1080 B G R frames (a smooth field, hard-edged boxes, noise of
sigma 5) and the 2880 x 1080 contact sheets egohmr_amd.render.contact_sheet makes of them (two samples, three columns, halved).  Quality 95,
4:2:0.  Legs, per input:
  (i)   ehm_jpeg_forward and ehm_jpeg_entropy_encode each between device events (`calls` calls per timing), and the bytes of the stage's
        traffic floor - pixels in, coefficients out and back in, packed words and stream out - over the sum of the two
  (ii)  JpegEncoder.encode end to end by the host clock (the call ends in its device-to-host copy): frames/s, and the bytes that cross PCIe
  (iii) the route a user has without the encoder: frames.cpu(), then PIL save (quality 95, 4:2:0, optimize=False: the same tables) on 8 and
        16 host threads: frames/s
Per-kernel times come from a run of their own: rocprofv3 --kernel-trace --stats -d DIR -- python tools/jpeg_encode_bench.py --kernels-only
(no timing of its own then, just `calls` encodes of each input).  Without a HIP device it fails rather than falls back.  Prints one JSON line."""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egohmr_amd import _lib  # noqa: E402
from egohmr_amd.jpeg import JpegEncoder  # noqa: E402
from egohmr_amd.render import contact_sheet  # noqa: E402


def synthesise(n, H=1080, W=1920):
    out = np.empty((n, H, W, 3), np.uint8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    for k in range(n):
        rng = np.random.default_rng(6000 + k)
        img = np.stack([128 + 90 * np.sin(x / rng.uniform(20, 90) + rng.uniform(0, 6)) * np.cos(y / rng.uniform(20, 90) + rng.uniform(0, 6)) for _ in range(3)], -1)
        for _ in range(40):
            y0, x0 = int(rng.integers(0, H - 64)), int(rng.integers(0, W - 64))
            img[y0:y0 + int(rng.integers(8, 200)), x0:x0 + int(rng.integers(8, 300))] = rng.uniform(0, 255, 3)
        img += rng.normal(0, 5, img.shape).astype(np.float32)
        out[k] = np.clip(img, 0, 255).astype(np.uint8)
    return out


def wall(fn, repeats):
    """(best, median) wall seconds of fn() over `repeats` runs after one warm-up"""
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


def events(fn, calls, repeats):
    """(best, median) device milliseconds of one fn() call"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / calls)
    return min(ts), float(np.median(ts))


def pil_save(bgr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(bgr[:, :, ::-1]).save(buf, "JPEG", quality=95, subsampling=2, optimize=False)
    return buf.getvalue()


def measure(frames, a, have_pil):
    dev = frames.device
    F, H, W, _ = frames.shape
    enc = JpegEncoder(dev, quality=95, subsampling="4:2:0")
    files = enc.encode(frames)                                          # sizes the buffers; every later call reuses them
    if enc.reruns:
        files = enc.encode(frames)
    res = dict(F=F, H=H, W=W, mean_file_bytes=int(np.mean([len(f) for f in files])), reruns_first_call=enc.reruns)
    if a.kernels_only:
        for _ in range(a.calls):
            enc.encode(frames)
        torch.cuda.synchronize()
        return res
    # (i) the two entries alone
    coef, quant = enc.coefficients(frames)
    stream = _lib.stream_ptr()
    fd = _lib.JpegForwardDesc(frames=_lib.ptr(frames), quant=_lib.ptr(quant), H=H, W=W, hmax=2, vmax=2, F=F, rgb=0, coef=_lib.ptr(coef))
    capacity = enc._streams.numel() // F
    info = torch.empty(2, F, dtype=torch.int64, device=dev)
    ed = _lib.JpegEntropyEncodeDesc(coef=_lib.ptr(coef), H=H, W=W, hmax=2, vmax=2, F=F, streams=enc._streams.data_ptr(), capacity=capacity,
                                    lengths=info[0].data_ptr(), needed=info[1].data_ptr(), workspace=_lib.ptr(enc._workspace),
                                    workspace_bytes=enc._workspace.numel())
    fb, fm = events(lambda: _lib.api().ehm_jpeg_forward(C.byref(fd), stream), a.calls, a.repeats)
    eb, em = events(lambda: _lib.api().ehm_jpeg_entropy_encode(C.byref(ed), stream), a.calls, a.repeats)
    lengths = info[0].cpu().numpy()
    stuffed = float(lengths.mean())
    packed = stuffed - float(np.mean([f[_lib.JPEG_ENC_HEADER_BYTES:-2].count(b"\xff\x00") for f in files]))
    count = coef.shape[1]
    floor = H * W * 3 + 2 * count + 2 * count + packed + stuffed       # pixels in | coefficients out | and back in | packed words out | stream out
    res.update(forward_ms=round(fb, 4), forward_ms_median=round(fm, 4), entropy_ms=round(eb, 4), entropy_ms_median=round(em, 4),
               device_us_per_frame=round((fb + eb) * 1e3 / F, 2), floor_bytes_per_frame=int(floor),
               floor_tb_per_s=round(F * floor / ((fb + eb) * 1e-3) / 1e12, 3), workspace_mb=round(enc._workspace.numel() / 2 ** 20, 1),
               stream_equals_encode=bool(all(enc._streams[f * capacity:f * capacity + lengths[f]].cpu().numpy().tobytes() == files[f][_lib.JPEG_ENC_HEADER_BYTES:-2]
                                             for f in range(F))))
    # (ii) end to end
    b, m = wall(lambda: enc.encode(frames), a.repeats)
    res.update(encode_fps=round(F / b, 1), encode_fps_median=round(F / m, 1), encode_ms_per_call=round(b * 1e3, 2),
               pcie_bytes_per_frame=int(lengths.max()) + 16, pixels_bytes_per_frame=H * W * 3)
    # (iii) the yardstick
    if have_pil:
        ref = pil_save(frames[0].cpu().numpy())
        res["file_equals_pil_first_frame"] = bool(ref == files[0])
        for t in (8, 16):
            with ThreadPoolExecutor(max_workers=t) as ex:
                b, m = wall(lambda: list(ex.map(pil_save, frames.cpu().numpy())), a.repeats)
            res[f"pil_t{t}_fps"] = round(F / b, 1)
            res[f"pil_t{t}_fps_median"] = round(F / m, 1)
    else:
        res["pil_note"] = "PIL not installed: leg (iii) not measured"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: the encoder is not measured on a CPU")
    try:
        import PIL
        have_pil = PIL.__version__
    except ImportError:
        have_pil = None
    dev = torch.device("cuda:0")
    frames = torch.from_numpy(synthesise(a.frames)).to(dev)
    res = dict(pil=have_pil, repeats=a.repeats, calls=a.calls, frames_1080p=measure(frames, a, have_pil))
    pairs = frames.reshape(a.frames // 2, 2, *frames.shape[1:])
    sheets = torch.stack([contact_sheet(p, p.flip(0), p.flip(2)) for p in pairs[:max(a.frames // 4, 1)]])
    res["contact_sheets"] = measure(sheets, a, have_pil)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
