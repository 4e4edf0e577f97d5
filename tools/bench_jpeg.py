"""JPEG decoding, measured: python tools/bench_jpeg.py [--dir DIR] [--frames 32] [--repeats 5] [--host-only]

Frames are 1920 x 1080 4:2:0 quality-95 JPEGs synthesised with PIL from a seed (or every *.jpg of --dir, which must share one geometry).  Legs:
  (i)   host entropy stage (ehm_jpeg_entropy_decode through JpegDecoder.entropy): ms per frame on one thread, frames/s with 8 and 16 threads
  (ii)  device stage (ehm_jpeg_decode, the two kernels) for F frames: device-event time per call, and the bytes the algorithm moves
        (coefficients in, planes out and in, pixels out, tables) over that time
  (iii) JpegDecoder.decode end to end, host clock around calls that end in a device synchronise: frames/s with 8 and 16 threads
  (iv)  the yardstick: PIL decodes of the same bytes on the same number of threads, stacked and uploaded: frames/s
Without a HIP device legs (ii) - (iv) fail rather than fall back; --host-only runs (i) and the PIL decode of (iv) without its upload.
Prints one JSON line."""
import argparse
import glob
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
from egohmr_amd.jpeg import JpegDecoder  # noqa: E402


def synthesise(n, H=1080, W=1920, quality=95):
    from PIL import Image
    out = []
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    for k in range(n):
        rng = np.random.default_rng(4000 + k)
        img = np.stack([128 + 90 * np.sin(x / rng.uniform(20, 90) + rng.uniform(0, 6)) * np.cos(y / rng.uniform(20, 90) + rng.uniform(0, 6)) for _ in range(3)], -1)
        for _ in range(40):                                   # hard-edged boxes: detail for the Huffman stage beyond a smooth field
            y0, x0 = int(rng.integers(0, H - 64)), int(rng.integers(0, W - 64))
            img[y0:y0 + int(rng.integers(8, 200)), x0:x0 + int(rng.integers(8, 300))] = rng.uniform(0, 255, 3)
        img += rng.normal(0, 5, img.shape).astype(np.float32)
        buf = io.BytesIO()
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=quality, subsampling=2)
        out.append(buf.getvalue())
    return out


def best(fn, repeats):
    """(best, median) wall seconds of fn() over `repeats` runs after one warm-up"""
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


def pil_decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im.convert("RGB"))[:, :, ::-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    try:
        import PIL
        have_pil = PIL.__version__
    except ImportError:
        have_pil = None
    if a.dir:
        datas = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(a.dir, "*.jpg")))[:a.frames]]
    elif have_pil:
        datas = synthesise(a.frames)
    else:
        raise SystemExit("PIL is not installed: give --dir with JPEG files")
    F = len(datas)
    res = dict(frames=F, mean_file_bytes=int(np.mean([len(d) for d in datas])), pil=have_pil, repeats=a.repeats)
    gpu = torch.cuda.is_available()
    if not gpu and not a.host_only:
        raise SystemExit("no HIP device: legs (ii) - (iv) are not measured on a CPU (use --host-only for the host legs)")
    dev = torch.device("cuda:0" if gpu else "cpu")

    # (i) host entropy
    decs = {t: JpegDecoder(dev, threads=t) for t in (1, 8, 16)}
    headers, _ = decs[1].entropy(datas)
    h = headers[0]
    res.update(H=h.H, W=h.W, components=h.components, sampling=[h.hmax, h.vmax], coef_count=int(h.coef_count))
    for t, d in decs.items():
        b, m = best(lambda: d.entropy(datas), a.repeats)
        res[f"entropy_t{t}_fps"] = round(F / b, 1)
        res[f"entropy_t{t}_fps_median"] = round(F / m, 1)
    res["entropy_ms_per_frame_one_thread"] = round(1e3 / res["entropy_t1_fps"], 3)

    # (iv) the yardstick's decode
    for t in (8, 16):
        with ThreadPoolExecutor(max_workers=t) as ex:
            if have_pil:
                def yard():
                    frames = np.stack(list(ex.map(pil_decode, datas)))
                    if gpu:
                        torch.from_numpy(frames).to(dev)
                        torch.cuda.synchronize()
                b, m = best(yard, a.repeats)
                res[f"pil_t{t}_{'upload_' if gpu else ''}fps"] = round(F / b, 1)
                res[f"pil_t{t}_{'upload_' if gpu else ''}fps_median"] = round(F / m, 1)
    if not have_pil:
        res["pil_note"] = "PIL not installed: leg (iv) not measured"

    if gpu:
        # (iii) end to end
        for t in (8, 16):
            def e2e():
                decs[t].decode(datas)
                torch.cuda.synchronize()
            b, m = best(e2e, a.repeats)
            res[f"decode_t{t}_fps"] = round(F / b, 1)
            res[f"decode_t{t}_fps_median"] = round(F / m, 1)
        # (ii) the device stage alone, on coefficients already uploaded
        import ctypes as C
        headers, coef = decs[8].entropy(datas)
        coef_d = coef.to(dev)
        quant_d = torch.from_numpy(JpegDecoder.quant_rows(headers)).to(dev)
        frames = torch.empty(F, h.H, h.W, 3, dtype=torch.uint8, device=dev)
        d = _lib.JpegDecodeDesc(coef=_lib.ptr(coef_d), quant=_lib.ptr(quant_d), H=h.H, W=h.W, components=h.components, hmax=h.hmax, vmax=h.vmax, F=F,
                                frames=_lib.ptr(frames))
        need = C.c_int64(0)
        _lib.api().ehm_jpeg_workspace_bytes(C.byref(d), C.byref(need))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        d.workspace, d.workspace_bytes = _lib.ptr(ws), need.value
        stream = _lib.stream_ptr()
        calls = 50
        for _ in range(5):
            _lib.api().ehm_jpeg_decode(C.byref(d), stream)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                _lib.api().ehm_jpeg_decode(C.byref(d), stream)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / calls)
        count = int(h.coef_count)
        bytes_per_frame = 2 * count + count + count + h.H * h.W * 3 + 3 * 64 * 2        # coefficients | planes out | planes in | pixels | tables
        res.update(device_ms_per_call=round(min(times), 4), device_ms_per_call_median=round(float(np.median(times)), 4),
                   device_bytes_per_frame=bytes_per_frame, device_tb_per_s=round(F * bytes_per_frame / (min(times) * 1e-3) / 1e12, 3),
                   device_us_per_frame=round(min(times) * 1e3 / F, 2))
        same = torch.equal(decs[8].decode(datas), frames)
        res["device_equals_decode"] = bool(same)
        if have_pil:
            ref = np.stack([pil_decode(x) for x in datas[:2]])
            res["max_diff_vs_pil_first_two"] = int(np.abs(frames[:2].cpu().numpy().astype(np.int32) - ref.astype(np.int32)).max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
