"""Baseline-JPEG frames decoded onto the device: the reference's cv2.imread(path, IMREAD_COLOR | IMREAD_IGNORE_ORIENTATION)
(dataloaders/augmentation.py:346), split where the format is serial.

    host     csrc/jpeg_entropy.h  ehm_jpeg_entropy_decode   marker parser + Huffman stage, plain C++, one frame per thread (ctypes releases the GIL)
    device   csrc/jpeg.hip        ehm_jpeg_decode           dequantisation + 8x8 IDCT, then chroma upsampling + YCbCr -> BGR: uint8 [F,H,W,3]

The pixels are libjpeg's defaults (ISLOW integer IDCT, fancy upsampling, its fixed-point colour tables; include/egohmr_hip.h states the rule),
checked bit for bit against PIL's decode of the fixtures under tests/golden/jpeg - not against cv2, which was never run.  EXIF orientation is
ignored, as the reference's flag asks.  Progressive, arithmetic, 12-bit and 4-component files are refused (EgoHMRHipError).
"""
from __future__ import annotations

import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib

_GEOMETRY = ("H", "W", "components", "hmax", "vmax")


def _read(item) -> bytes:
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    with open(os.fspath(item), "rb") as f:
        return f.read()


def _refused(function, rc, msg, index):
    return _lib.EgoHMRHipError(f"{function} failed on item {index} (rc={rc}): {msg}", rc=rc, function=function)


def _geometry_text(h):
    return f"{h.H}x{h.W} with {h.components} component(s), sampling {h.hmax}x{h.vmax}"


class JpegDecoder:
    """``decode(items)``: a list of encoded frames (``bytes`` or paths) of one geometry -> uint8 [F,H,W,3] BGR on ``device``.
    ``entropy(items)``: the host stage alone (runs without a GPU).  ``threads`` host threads (clamped to 1...16) each decode whole frames."""

    def __init__(self, device, threads=8):
        self.device = torch.device(device)
        self.threads = min(max(int(threads), 1), 16)
        self._pool = None
        self._staging = None            # one reusable int16 host buffer, pinned where a HIP device is available
        self._uploaded = None           # event behind the last upload out of it
        self._workspace = None

    def _executor(self):
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="ehm-jpeg")
        return self._pool

    def close(self):
        if self._pool is not None:
            self._pool.shutdown()
            self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stage(self, count):
        if self._uploaded is not None:                   # the previous call's copy out of the buffer must have left it
            self._uploaded.synchronize()
            self._uploaded = None
        if self._staging is None or self._staging.numel() < count:
            buf = torch.empty(count, dtype=torch.int16)
            self._staging = buf.pin_memory() if torch.cuda.is_available() else buf
        return self._staging

    def entropy(self, items):
        """-> (headers, coef): one ehm_jpeg_header mirror per item and the quantised coefficients, int16 [F, coef_count] on the host - a view
        of the decoder's staging buffer, valid until its next call.  All items must share one geometry (ValueError names both otherwise); a
        file the library refuses raises EgoHMRHipError with its message and the item's index."""
        L = _lib.lib()
        datas = [_read(it) for it in items]
        if not datas:
            raise ValueError("no frames to decode")
        headers = []
        for i, d in enumerate(datas):
            h = _lib.JpegHeader()
            rc = L.ehm_jpeg_read_header(d, len(d), C.byref(h))
            if rc != 0:
                raise _refused("ehm_jpeg_read_header", rc, L.ehm_last_error().decode(), i)
            if i and any(getattr(h, k) != getattr(headers[0], k) for k in _GEOMETRY):
                raise ValueError(f"frames of different geometry in one call: item 0 is {_geometry_text(headers[0])}, item {i} is {_geometry_text(h)}")
            headers.append(h)
        count = int(headers[0].coef_count)
        coef = self._stage(count * len(datas))[:count * len(datas)].view(len(datas), count)
        base = coef.data_ptr()

        def one(i):
            rc = L.ehm_jpeg_entropy_decode(datas[i], len(datas[i]), None, base + 2 * count * i, count)
            return rc, (L.ehm_last_error().decode() if rc else "")          # the text is per thread: read it on the thread that failed

        results = [one(0)] if len(datas) == 1 else list(self._executor().map(one, range(len(datas))))
        for i, (rc, msg) in enumerate(results):
            if rc != 0:
                raise _refused("ehm_jpeg_entropy_decode", rc, msg, i)
        return headers, coef

    @staticmethod
    def quant_rows(headers) -> np.ndarray:
        """uint16 [F, 3, 64]: per frame and component the table its quant_id names (natural order)."""
        q = np.zeros((len(headers), 3, 64), np.uint16)
        for f, h in enumerate(headers):
            tables = np.ctypeslib.as_array(h.quant)
            for c in range(h.components):
                q[f, c] = tables[h.quant_id[c]]
        return q

    def decode(self, items) -> torch.Tensor:
        dev = self.device
        if dev.type != "cuda":
            raise _lib.EgoHMRHipError("JpegDecoder.decode runs on the HIP kernels only (got a CPU device); there is no CPU path")
        headers, coef = self.entropy(items)
        h0, F = headers[0], len(headers)
        with _lib.on_device(dev):
            stream = _lib.stream_ptr()
            coef_d = coef.to(dev, non_blocking=True)
            if coef.is_pinned():
                self._uploaded = torch.cuda.Event()
                self._uploaded.record()
            quant_d = torch.from_numpy(self.quant_rows(headers)).to(dev)
            frames = torch.empty(F, h0.H, h0.W, 3, dtype=torch.uint8, device=dev)
            d = _lib.JpegDecodeDesc(coef=_lib.ptr(coef_d), quant=_lib.ptr(quant_d), H=h0.H, W=h0.W, components=h0.components, hmax=h0.hmax,
                                    vmax=h0.vmax, F=F, frames=_lib.ptr(frames))
            need = C.c_int64(0)
            _lib.api().ehm_jpeg_workspace_bytes(C.byref(d), C.byref(need))
            if self._workspace is None or self._workspace.numel() < need.value or self._workspace.device != dev:
                self._workspace = torch.empty(need.value, dtype=torch.uint8, device=dev)
            d.workspace, d.workspace_bytes = _lib.ptr(self._workspace), self._workspace.numel()
            _lib.api().ehm_jpeg_decode(C.byref(d), stream)
        return frames
