"""Baseline-JPEG frames decoded onto the device: the reference's cv2.imread(path, IMREAD_COLOR | IMREAD_IGNORE_ORIENTATION)
(dataloaders/augmentation.py:346), split where the format is serial.

    host     csrc/jpeg_entropy.h  ehm_jpeg_entropy_decode   marker parser + Huffman stage, plain C++, one frame per thread (ctypes releases the GIL)
    device   csrc/jpeg.hip        ehm_jpeg_decode           dequantisation + 8x8 IDCT, then chroma upsampling + YCbCr -> BGR: uint8 [F,H,W,3]

The pixels are libjpeg's defaults (ISLOW integer IDCT, fancy upsampling, its fixed-point colour tables; include/egohmr_hip.h states the rule),
checked bit for bit against PIL's decode of the fixtures under tests/golden/jpeg - not against cv2, which was never run.  EXIF orientation is
ignored, as the reference's flag asks.  Progressive, arithmetic, 12-bit and 4-component files are refused (EgoHMRHipError).

The way back, ``JpegEncoder`` (the reference's cv2.imwrite of its overlay sheets, test_egohmr.py:626), has no serial stage and runs on the device
as a whole:

    device   csrc/jpeg_enc.hip    ehm_jpeg_forward          colour conversion, chroma downsampling, forward DCT, quantisation, dummy blocks
    device   csrc/jpeg_enc.hip    ehm_jpeg_entropy_encode   Huffman coding at prefix-summed bit offsets, byte stuffing
    host     csrc/jpeg_enc.h      ehm_jpeg_write_header     the 623 bytes of markers around the stream
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


SAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}


def quality_tables(quality) -> np.ndarray:
    """uint16 [2, 64] (natural order): libjpeg's scaling of the Annex K tables for ``quality`` in 1...100 (ehm_jpeg_quality_tables; no GPU needed)."""
    q = np.zeros((2, 64), np.uint16)
    rc = _lib.lib().ehm_jpeg_quality_tables(int(quality), q.ctypes.data)
    if rc != 0:
        raise _lib.EgoHMRHipError(f"ehm_jpeg_quality_tables failed (rc={rc}): {_lib.lib().ehm_last_error().decode()}", rc=rc, function="ehm_jpeg_quality_tables")
    return q


def file_header(H, W, hmax, vmax, tables) -> bytes:
    """SOI ... SOS for one frame (ehm_jpeg_write_header; no GPU needed)."""
    q = np.ascontiguousarray(tables, dtype=np.uint16).reshape(2, 64)
    out = np.zeros(_lib.JPEG_ENC_HEADER_BYTES, np.uint8)
    n = C.c_int64(0)
    rc = _lib.lib().ehm_jpeg_write_header(int(H), int(W), int(hmax), int(vmax), q.ctypes.data, out.ctypes.data, out.size, C.byref(n))
    if rc != 0:
        raise _lib.EgoHMRHipError(f"ehm_jpeg_write_header failed (rc={rc}): {_lib.lib().ehm_last_error().decode()}", rc=rc, function="ehm_jpeg_write_header")
    return out[:n.value].tobytes()


class JpegEncoder:
    """uint8 [F,H,W,3] frames on ``device`` -> baseline-JPEG files, every stage on the device (csrc/jpeg_enc.hip): colour conversion, chroma
    downsampling, forward DCT, quantisation, Huffman coding and byte stuffing.  Only the compressed stream crosses to the host, which adds the
    623 bytes of markers.  The rule is libjpeg's default encoder with the fixed Annex K Huffman tables (no ``optimize``), no restart markers, no
    progressive mode (include/egohmr_hip.h, "JPEG encoding"); the bytes were compared with PIL's, not with cv2's.  ``quality`` 95 and
    ``subsampling`` '4:2:0' are what cv2.imwrite's documentation gives as its defaults.  ``tables``: explicit uint16 [2, 64] quantisation tables
    (natural order, entries 1...255) instead of ``quality``."""

    def __init__(self, device, quality=95, subsampling="4:2:0", tables=None):
        if subsampling not in SAMPLINGS:
            raise ValueError(f"subsampling must be one of {sorted(SAMPLINGS)}, got {subsampling!r}")
        self.device = torch.device(device)
        self.quality, self.subsampling = quality, subsampling
        self.hmax, self.vmax = SAMPLINGS[subsampling]
        self.tables = None if tables is None else np.ascontiguousarray(tables, dtype=np.uint16).reshape(2, 64)
        self.bytes_per_pixel = 0.5          # first guess of a stream's size; a flagged frame corrects the capacity in one rerun
        self.reruns = 0                     # calls that needed the second pass
        self._workspace = self._streams = None

    def _tables(self, F, quality):
        """[(2,64)] * F: the explicit tables, or one per quality"""
        if self.tables is not None and quality is None:
            return [self.tables] * F
        q = self.quality if quality is None else quality
        qs = [int(v) for v in q] if isinstance(q, (list, tuple, np.ndarray)) else [int(q)] * F
        if len(qs) != F:
            raise ValueError(f"{len(qs)} qualities for {F} frames")
        cache = {v: quality_tables(v) for v in set(qs)}
        return [cache[v] for v in qs]

    def _check(self, frames):
        if self.device.type != "cuda":
            raise _lib.EgoHMRHipError("JpegEncoder runs on the HIP kernels only (got a CPU device); there is no CPU path")
        if frames.dim() == 3:
            frames = frames[None]
        if frames.dim() != 4 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
            raise ValueError(f"frames must be uint8 [F, H, W, 3], got {frames.dtype} {tuple(frames.shape)}")
        return frames.to(self.device).contiguous()

    def _forward(self, frames, tables, bgr, stream):
        F, H, W, _ = frames.shape
        rows = np.stack([np.stack([t[0], t[1], t[1]]) for t in tables])                    # [F, 3, 64]: luma, chroma, chroma
        if (rows == 0).any() or (rows > 255).any():
            raise ValueError("quantisation table entries must be 1...255")
        quant = torch.from_numpy(rows).to(self.device)
        mx, my = -(-W // (8 * self.hmax)), -(-H // (8 * self.vmax))
        count = 64 * mx * my * (self.hmax * self.vmax + 2)
        coef = torch.empty(F, count, dtype=torch.int16, device=self.device)
        d = _lib.JpegForwardDesc(frames=_lib.ptr(frames), quant=_lib.ptr(quant), H=H, W=W, hmax=self.hmax, vmax=self.vmax, F=F, rgb=0 if bgr else 1,
                                 coef=_lib.ptr(coef))
        _lib.api().ehm_jpeg_forward(C.byref(d), stream)
        return coef, quant

    def coefficients(self, frames, bgr=True, quality=None):
        """The forward stage alone -> (int16 [F, coef_count] in the decoder's layout, uint16 [F, 3, 64] quant rows), both on the device."""
        frames = self._check(frames)
        with _lib.on_device(self.device):
            return self._forward(frames, self._tables(frames.shape[0], quality), bgr, _lib.stream_ptr())

    def entropy(self, coef, H, W, capacity):
        """The entropy stage alone on int16 [F, coef_count] device coefficients -> (streams uint8 [F, capacity], lengths, needed int64 [F]), all
        on the device: ehm_jpeg_entropy_encode's contract (lengths -1: needed > capacity; -2: a coefficient without a code)."""
        F, dev = coef.shape[0], self.device
        with _lib.on_device(dev):
            stream = _lib.stream_ptr()
            if self._streams is None or self._streams.numel() < F * capacity or self._streams.device != dev:
                self._streams = torch.empty(F * capacity, dtype=torch.uint8, device=dev)
            streams = self._streams[:F * capacity].view(F, capacity)
            info = torch.empty(2, F, dtype=torch.int64, device=dev)
            d = _lib.JpegEntropyEncodeDesc(coef=_lib.ptr(coef), H=H, W=W, hmax=self.hmax, vmax=self.vmax, F=F, streams=streams.data_ptr(),
                                           capacity=capacity, lengths=info[0].data_ptr(), needed=info[1].data_ptr())
            need = C.c_int64(0)
            _lib.api().ehm_jpeg_entropy_encode_workspace_bytes(C.byref(d), C.byref(need))
            if self._workspace is None or self._workspace.numel() < need.value or self._workspace.device != dev:
                self._workspace = torch.empty(need.value, dtype=torch.uint8, device=dev)
            d.workspace, d.workspace_bytes = _lib.ptr(self._workspace), self._workspace.numel()
            _lib.api().ehm_jpeg_entropy_encode(C.byref(d), stream)
        return streams, info[0], info[1]

    def encode(self, frames, bgr=True, quality=None):
        """-> a list of F ``bytes``, each a whole file.  One geometry per call; ``quality`` (default: the encoder's) may be one value per frame.
        One host read-back of the lengths per call, then one copy of the used bytes; a frame whose stream did not fit the buffer triggers ONE
        rerun of the entropy stage with the reported size."""
        frames = self._check(frames)
        F, H, W, _ = frames.shape
        tables = self._tables(F, quality)
        with _lib.on_device(self.device):
            coef, _ = self._forward(frames, tables, bgr, _lib.stream_ptr())
            capacity = max(int(H * W * self.bytes_per_pixel), 1024)
            if self._streams is not None and self._streams.device == self.device:
                capacity = max(capacity, self._streams.numel() // F)
            streams, lengths, needed = self.entropy(coef, H, W, capacity)
            host = torch.stack([lengths, needed]).cpu().numpy()
            if (host[0] == -2).any():
                raise _lib.EgoHMRHipError("ehm_jpeg_entropy_encode: a coefficient has no Huffman code (frame %d)" % int(np.argmax(host[0] == -2)))
            if (host[0] < 0).any():
                self.reruns += 1
                capacity = int(host[1].max()) + int(host[1].max()) // 8
                streams, lengths, needed = self.entropy(coef, H, W, capacity)
                host = torch.stack([lengths, needed]).cpu().numpy()
                if (host[0] < 0).any():
                    raise _lib.EgoHMRHipError("ehm_jpeg_entropy_encode flagged a frame again after the rerun with the size it reported")
            used = int(host[0].max())
            data = streams[:, :used].cpu().numpy()
        out = []
        for f in range(F):
            out.append(file_header(H, W, self.hmax, self.vmax, tables[f]) + data[f, :int(host[0][f])].tobytes() + b"\xff\xd9")
        return out

    def write(self, frames, paths, bgr=True, quality=None):
        """Encodes and writes one file per frame."""
        paths = [os.fspath(p) for p in paths]
        frames = self._check(frames)
        if len(paths) != frames.shape[0]:
            raise ValueError(f"{len(paths)} paths for {frames.shape[0]} frames")
        for path, data in zip(paths, self.encode(frames, bgr=bgr, quality=quality)):
            with open(path, "wb") as f:
                f.write(data)
        return paths
