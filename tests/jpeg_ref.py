"""A numpy restatement of the baseline-JPEG rule of include/egohmr_hip.h (section "JPEG decoding"): the marker parser and the Huffman stage
bit by bit, then libjpeg's defaults - the ISLOW integer IDCT, "fancy" chroma upsampling, its fixed-point colour tables.  It is the
reference of tests/test_jpeg_cpu.py (header fields, quantisation tables, quantised coefficients) and, through the committed pixels it
reproduces with difference 0, of tests/test_gpu_jpeg.py.  Slow and plain on purpose: test fixtures are a few thousand pixels.
planes_and_pixels is the device stage alone, on coefficients and one table row per component - the reference of
tests/test_gpu_jpeg_kernels.py on the synthetic cases of tests/jpeg_cases.py - with the IDCT in int64 under a range check and a set of
planted mistakes (``wrong=``) that tests/test_jpeg_cases_cpu.py shows the cases to catch.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class JpegError(ValueError):
    pass


def _huffman_table(counts, symbols):
    """{(length, code): symbol} of the canonical code."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return table


class _Bits:
    """The entropy-coded segment as a bit stream: FF 00 is the byte FF, any other FF xx ends the data (a marker)."""

    def __init__(self, data, pos):
        self.data, self.pos, self.acc, self.cnt = data, pos, 0, 0

    def bit(self):
        if self.cnt == 0:
            if self.pos >= len(self.data):
                raise JpegError("truncated entropy data")
            b = self.data[self.pos]
            if b == 0xFF:
                if self.pos + 1 >= len(self.data):
                    raise JpegError("truncated entropy data")
                if self.data[self.pos + 1] != 0:
                    raise JpegError("marker inside entropy data")
                self.pos += 2
            else:
                self.pos += 1
            self.acc, self.cnt = b, 8
        self.cnt -= 1
        return (self.acc >> self.cnt) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in table:
                return table[(length, code)]
        raise JpegError("Huffman code with no entry")

    def restart(self, expected):
        self.cnt = 0
        d, p = self.data, self.pos
        if p >= len(d) or d[p] != 0xFF:
            raise JpegError("restart marker missing")
        while p < len(d) and d[p] == 0xFF:
            p += 1
        if p >= len(d) or d[p] != 0xD0 + expected:
            raise JpegError("restart marker out of order")
        self.pos = p + 1


def _extend(v, s):
    return v if s == 0 or v >= (1 << (s - 1)) else v - (1 << s) + 1


def parse(data: bytes, decode: bool = True) -> SimpleNamespace:
    """-> H, W, components, hmax, vmax, mcus_x, mcus_y, restart_interval, h, v, blocks_x, blocks_y, quant_id (per component), quant uint16 [4,64]
    (natural order), coef_count and - with ``decode`` - coef: the quantised int16 coefficients, component planes one after the other, each
    [blocks_y, blocks_x, 64] in natural order over the MCU-padded grid."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise JpegError("no SOI")
    pos = 2
    quant, qdef = np.zeros((4, 64), np.uint16), [False] * 4
    huff = {}
    frame, ri = None, 0
    while True:
        if pos + 2 > len(data) or data[pos] != 0xFF:
            raise JpegError("marker expected")
        while pos < len(data) and data[pos] == 0xFF:
            pos += 1
        if pos >= len(data):
            raise JpegError("truncated")
        m = data[pos]
        pos += 1
        if m == 0xD9 or m == 0x01 or 0xD0 <= m <= 0xD8:
            raise JpegError("unexpected marker")
        if pos + 2 > len(data):
            raise JpegError("truncated")
        n = (data[pos] << 8) | data[pos + 1]
        if n < 2 or pos + n > len(data):
            raise JpegError("truncated segment")
        seg = data[pos + 2:pos + n]
        pos += n
        if m == 0xDB:
            p = 0
            while p < len(seg):
                if seg[p] >> 4:
                    raise JpegError("16-bit quantisation table")
                t = seg[p] & 15
                if t > 3 or p + 65 > len(seg):
                    raise JpegError("bad DQT")
                quant[t, ZIGZAG] = np.frombuffer(seg[p + 1:p + 65], np.uint8)
                qdef[t] = True
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                tc, th = seg[p] >> 4, seg[p] & 15
                if tc > 1 or th > 3 or p + 17 > len(seg):
                    raise JpegError("bad DHT")
                counts = list(seg[p + 1:p + 17])
                total = sum(counts)
                if total > 256 or p + 17 + total > len(seg):
                    raise JpegError("bad DHT")
                huff[(tc, th)] = _huffman_table(counts, list(seg[p + 17:p + 17 + total]))
                p += 17 + total
        elif m in (0xC0, 0xC1):
            if frame is not None:
                raise JpegError("two frames")
            if len(seg) < 6 or seg[0] != 8:
                raise JpegError("precision")
            H, W, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if nc not in (1, 3) or len(seg) != 6 + 3 * nc or H == 0 or W == 0:
                raise JpegError("unsupported frame")
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)]
            frame = (H, W, comps)
        elif m == 0xC2 or (0xC3 <= m <= 0xCF and m not in (0xC4, 0xC8)):
            raise JpegError("progressive" if m == 0xC2 else "unsupported process")
        elif m == 0xDD:
            if len(seg) != 2:
                raise JpegError("bad DRI")
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            break
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            pass
        else:
            raise JpegError("unsupported marker")
    if frame is None:
        raise JpegError("SOS before SOF")
    H, W, comps = frame
    nc = len(comps)
    if seg[0] != nc or len(seg) != 4 + 2 * nc:
        raise JpegError("one interleaved scan only")
    tables = []
    for i in range(nc):
        if seg[1 + 2 * i] != comps[i][0]:
            raise JpegError("scan component order")
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if (0, td) not in huff or (1, ta) not in huff:
            raise JpegError("Huffman table not defined")
        tables.append((huff[(0, td)], huff[(1, ta)]))
    if tuple(seg[1 + 2 * nc:]) != (0, 63, 0):
        raise JpegError("spectral selection")
    h = [1] if nc == 1 else [c[1] for c in comps]
    v = [1] if nc == 1 else [c[2] for c in comps]
    if nc == 3 and ((h[0], v[0]) not in ((1, 1), (2, 1), (2, 2)) or (h[1], v[1], h[2], v[2]) != (1, 1, 1, 1)):
        raise JpegError("unsupported sampling")
    hmax, vmax = h[0], v[0]
    qid = [c[3] for c in comps]
    if any(q > 3 or not qdef[q] for q in qid):
        raise JpegError("quantisation table not defined")
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    bx, by = [mx * hi for hi in h], [my * vi for vi in v]
    out = SimpleNamespace(H=H, W=W, components=nc, hmax=hmax, vmax=vmax, mcus_x=mx, mcus_y=my, restart_interval=ri, h=h, v=v, blocks_x=bx,
                          blocks_y=by, quant_id=qid, quant=quant, coef_count=64 * sum(a * b for a, b in zip(bx, by)))
    if not decode:
        return out
    planes = [np.zeros((by[c], bx[c], 64), np.int16) for c in range(nc)]
    br = _Bits(data, pos)
    pred, nrst = [0] * nc, 0
    for mcu in range(mx * my):
        if ri and mcu and mcu % ri == 0:
            br.restart(nrst & 7)
            nrst += 1
            pred = [0] * nc
        my_, mx_ = divmod(mcu, mx)
        for c in range(nc):
            dc_t, ac_t = tables[c]
            for vy in range(v[c]):
                for hx in range(h[c]):
                    blk = planes[c][my_ * v[c] + vy, mx_ * h[c] + hx]
                    s = br.symbol(dc_t)
                    if s > 11:
                        raise JpegError("DC size")
                    pred[c] += _extend(br.bits(s), s)
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = br.symbol(ac_t)
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        if k > 63:
                            raise JpegError("k > 63")
                        blk[ZIGZAG[k]] = _extend(br.bits(s), s)
                        k += 1
    p = br.pos                                                     # the scan ends in EOI (fill bytes FF may precede it)
    if p >= len(data) or data[p] != 0xFF:
        raise JpegError("EOI missing")
    while p < len(data) and data[p] == 0xFF:
        p += 1
    if p >= len(data) or data[p] != 0xD9:
        raise JpegError("EOI missing")
    out.coef = np.concatenate([p.reshape(-1) for p in planes])
    return out


DECODE_WRONG = ("cr_uses_cb_table", "quant_of_frame0", "replicate_le1", "replicate_le3", "below_from_padding", "right_from_padding",
                "h2v2_bias_swapped", "h2v1_bias_swapped", "idct_wraps", "colour_wraps", "rows_before_columns", "luma_stride_unpadded")
_I32 = (-(1 << 31), (1 << 31) - 1)


class _Tracked:
    """An integer array whose +, -, *, << return a _Tracked again and widen the shared ``span`` [lowest, highest] by every result: whatever the
    pass below computes is range-checked, named or not, without the pass having to list it."""

    def __init__(self, v, span):
        self.v, self.span = v, span
        if span is not None and v.size:
            span[0], span[1] = min(span[0], int(v.min())), max(span[1], int(v.max()))

    def _op(self, other, f):
        return _Tracked(f(self.v, other.v if isinstance(other, _Tracked) else other), self.span)

    def __add__(self, o):
        return self._op(o, lambda a, b: a + b)

    def __sub__(self, o):
        return self._op(o, lambda a, b: a - b)

    def __mul__(self, o):
        return self._op(o, lambda a, b: a * b)

    def __lshift__(self, o):
        return self._op(o, lambda a, b: a << b)


def _idct_pass(x, shift, round_, dtype=np.int64):
    """One 1-D pass of jidctint over the LAST axis of x[..., 8], every operation in the kernel's order.  dtype int64 (the default): exact, and
    JpegError if the input or the result of ANY operation of the pass before the final shift - every named value, every operand, the eight
    sums - leaves int32: the domain on which the header's "all int32" rule says anything.  dtype int32: what an int32 machine computes
    (numpy wraps silently); inside the domain the two agree."""
    span = [0, 0] if dtype == np.int64 else None                       # (nothing to track where wrapping is the point)
    x0, x1, x2, x3, x4, x5, x6, x7 = (_Tracked(x[..., i].astype(dtype), span) for i in range(8))
    z1 = (x2 + x6) * 4433
    t2 = z1 - x6 * 15137
    t3 = z1 + x2 * 6270
    t0 = ((x0 + x4) << 13) + round_
    t1 = ((x0 - x4) << 13) + round_
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = x7, x5, x3, x1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + (z1 + z3), a1 + (z2 + z4), a2 + (z2 + z3), a3 + (z1 + z4)
    sums = (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)
    if span is not None and (span[0] < _I32[0] or span[1] > _I32[1]):
        raise JpegError(f"IDCT intermediate outside int32 ({span[0]} ... {span[1]}): beyond the domain of the integer rule")
    return np.stack([s.v for s in sums], -1) >> shift


def idct_samples(coef, quant, dtype=np.int64, wrong=None):
    """coef int16 [by, bx, 64], quant uint16 [64] -> the IDCT's results + 128 BEFORE the clamp, [by * 8, bx * 8] (dtype)."""
    by, bx, _ = coef.shape
    x = (coef.astype(dtype) * quant.astype(dtype)).reshape(by, bx, 8, 8)
    if wrong == "rows_before_columns":
        out = _idct_pass(_idct_pass(x, 11, 1 << 10, dtype).swapaxes(-1, -2), 18, 1 << 17, dtype).swapaxes(-1, -2)
    else:
        ws = _idct_pass(x.swapaxes(-1, -2), 11, 1 << 10, dtype).swapaxes(-1, -2)    # columns first
        out = _idct_pass(ws, 18, 1 << 17, dtype)                                    # then rows
    return (out + 128).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def _to_u8(v, wraps):
    return (v & 255).astype(np.uint8) if wraps else np.clip(v, 0, 255).astype(np.uint8)


def idct_plane(coef, quant, dtype=np.int64, wrong=None):
    """coef int16 [by, bx, 64], quant uint16 [64] -> uint8 samples [by * 8, bx * 8]."""
    return _to_u8(idct_samples(coef, quant, dtype, wrong), wrong == "idct_wraps")


def upsample(plane, ch, cw, hf, vf, H, W, wrong=None):
    """A chroma plane on the MCU grid, its real size ch x cw -> [H, W] int32.  Edges replicate the last REAL row and column; libjpeg takes the
    triangle filter only for planes more than two samples wide (jdsample.c), a narrower one is replicated."""
    plane = plane.astype(np.int32)
    if hf == 1 and vf == 1:
        return plane[:H, :W]
    limit = {"replicate_le1": 1, "replicate_le3": 3}.get(wrong, 2)
    if cw <= limit:
        return np.repeat(np.repeat(plane[:ch, :cw], vf, 0), hf, 1)[:H, :W]
    below = ch if wrong == "below_from_padding" and ch < plane.shape[0] else ch - 1
    right = cw if wrong == "right_from_padding" and cw < plane.shape[1] else cw - 1
    e = plane[np.ix_([0] + list(range(ch)) + [below], [0] + list(range(cw)) + [right])]     # the real samples with one neighbour on each side
    if vf == 1:
        rows, (even, odd), shift = [e[1:-1]], ((2, 1) if wrong == "h2v1_bias_swapped" else (1, 2)), 2
    else:
        rows, (even, odd), shift = [3 * e[1:-1] + e[:-2], 3 * e[1:-1] + e[2:]], ((7, 8) if wrong == "h2v2_bias_swapped" else (8, 7)), 4
    out = np.empty((vf * ch, 2 * cw), np.int32)
    for k, u in enumerate(rows):
        out[k::vf, 0::2] = (3 * u[:, 1:-1] + u[:, :-2] + even) >> shift
        out[k::vf, 1::2] = (3 * u[:, 1:-1] + u[:, 2:] + odd) >> shift
    return out[:H, :W]


def _fix(x):
    return int(x * 65536 + 0.5)


def block_grids(H, W, components, hmax, vmax):
    """-> [(blocks_y, blocks_x)] per component over the MCU grid"""
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    return [(my * vmax, mx * hmax)] + [(my, mx)] * (components - 1)


def planes_and_pixels(coef, quant, H, W, components, hmax, vmax, wrong=None, quant0=None, dtype=np.int64, detail=None):
    """One frame through the device stage's rule.  coef int16 [coef_count] in the decoder's layout, quant uint16 [3, 64]: one row per component
    (a one-component frame uses row 0) -> (planes, pixels): the uint8 component planes on the MCU grid, padding blocks included - one after the
    other they are what ehm_jpeg_decode leaves in its workspace for the frame - and the uint8 [H, W, 3] BGR pixels.
    wrong: one of DECODE_WRONG, a planted mistake (quant_of_frame0 takes the rows from ``quant0``, frame 0's).  dtype: see _idct_pass.
    detail: a dict that receives "samples" (per plane, before the clamp) and "bgr" (int32 [H, W, 3] before the clamp)."""
    assert wrong is None or wrong in DECODE_WRONG
    coef, quant = np.asarray(coef), np.asarray(quant if wrong != "quant_of_frame0" else quant0)
    rows = [0, 1, 1] if wrong == "cr_uses_cb_table" else [0, 1, 2]
    samples, o = [], 0
    for c, (by, bx) in enumerate(block_grids(H, W, components, hmax, vmax)):
        samples.append(idct_samples(coef[o:o + by * bx * 64].reshape(by, bx, 64), quant[rows[c]], dtype, wrong))
        o += by * bx * 64
    assert o == coef.size
    planes = [_to_u8(s, wrong == "idct_wraps") for s in samples]
    if wrong == "luma_stride_unpadded":
        y = planes[0].reshape(-1)[:H * W].reshape(H, W).astype(np.int32)
    else:
        y = planes[0][:H, :W].astype(np.int32)
    if components == 1:
        bgr = np.repeat(y[:, :, None], 3, 2)
    else:
        ch, cw = -(-H // vmax), -(-W // hmax)
        cb = upsample(planes[1], ch, cw, hmax, vmax, H, W, wrong) - 128
        cr = upsample(planes[2], ch, cw, hmax, vmax, H, W, wrong) - 128
        r = y + ((_fix(1.40200) * cr + 32768) >> 16)
        b = y + ((_fix(1.77200) * cb + 32768) >> 16)
        g = y + ((-_fix(0.34414) * cb + (-_fix(0.71414) * cr + 32768)) >> 16)
        bgr = np.stack([b, g, r], -1)
    if detail is not None:
        detail["samples"], detail["bgr"] = samples, bgr
    return planes, _to_u8(bgr, wrong == "colour_wraps")


def pixels(p, wrong=None) -> np.ndarray:
    """parse()'s result -> uint8 [H, W, 3] BGR."""
    quant = p.quant[[p.quant_id[min(c, p.components - 1)] for c in range(3)]]
    return planes_and_pixels(p.coef, quant, p.H, p.W, p.components, p.hmax, p.vmax, wrong=wrong)[1]


def decode(data: bytes) -> np.ndarray:
    return pixels(parse(data))
