"""A numpy restatement of the baseline-JPEG rule of include/egohmr_hip.h (section "JPEG decoding"): the marker parser and the Huffman stage
bit by bit, then libjpeg's defaults - the ISLOW integer IDCT, "fancy" chroma upsampling, its fixed-point colour tables.  It is the
reference of tests/test_jpeg_cpu.py (header fields, quantisation tables, quantised coefficients) and, through the committed pixels it
reproduces with difference 0, of tests/test_gpu_jpeg.py.  Slow and plain on purpose: test fixtures are a few thousand pixels.
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


def _idct_pass(x, shift, round_):
    """One 1-D pass of jidctint over the LAST axis of int32 x[..., 8]."""
    x = x.astype(np.int32)
    x0, x1, x2, x3, x4, x5, x6, x7 = (x[..., i] for i in range(8))
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
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], -1) >> shift


def idct_plane(coef, quant):
    """coef int16 [by, bx, 64], quant uint16 [64] -> uint8 samples [by * 8, bx * 8]."""
    by, bx, _ = coef.shape
    x = (coef.astype(np.int32) * quant.astype(np.int32)).reshape(by, bx, 8, 8)
    ws = _idct_pass(x.swapaxes(-1, -2), 11, 1 << 10).swapaxes(-1, -2)          # columns first
    out = _idct_pass(ws, 18, 1 << 17)                                           # then rows
    return np.clip(out + 128, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def _upsample_h(u, bias_even, bias_odd, shift):
    """out[2i] = (3 u[i] + u[i-1] + bias_even) >> shift, out[2i+1] = (3 u[i] + u[i+1] + bias_odd) >> shift, edges replicated."""
    left = np.concatenate([u[:, :1], u[:, :-1]], 1)
    right = np.concatenate([u[:, 1:], u[:, -1:]], 1)
    out = np.empty((u.shape[0], 2 * u.shape[1]), np.int32)
    out[:, 0::2] = (3 * u + left + bias_even) >> shift
    out[:, 1::2] = (3 * u + right + bias_odd) >> shift
    return out


def upsample(s, hf, vf, H, W):
    """A chroma plane cropped to its real size -> [H, W] int32.  libjpeg takes the triangle filter only for planes more than two samples
    wide (jdsample.c); a narrower one is replicated."""
    s = s.astype(np.int32)
    if hf == 1 and vf == 1:
        return s[:H, :W]
    if s.shape[1] <= 2:
        return np.repeat(np.repeat(s, vf, 0), hf, 1)[:H, :W]
    if vf == 1:
        return _upsample_h(s, 1, 2, 2)[:H, :W]
    above = np.concatenate([s[:1], s[:-1]], 0)
    below = np.concatenate([s[1:], s[-1:]], 0)
    u = np.empty((2 * s.shape[0], s.shape[1]), np.int32)
    u[0::2] = 3 * s + above
    u[1::2] = 3 * s + below
    return _upsample_h(u, 8, 7, 4)[:H, :W]


def _fix(x):
    return int(x * 65536 + 0.5)


def pixels(p) -> np.ndarray:
    """parse()'s result -> uint8 [H, W, 3] BGR."""
    H, W = p.H, p.W
    planes, o = [], 0
    for c in range(p.components):
        n = p.blocks_y[c] * p.blocks_x[c] * 64
        planes.append(idct_plane(p.coef[o:o + n].reshape(p.blocks_y[c], p.blocks_x[c], 64), p.quant[p.quant_id[c]]))
        o += n
    y = planes[0][:H, :W].astype(np.int32)
    if p.components == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    ch, cw = -(-H // p.vmax), -(-W // p.hmax)
    cb = upsample(planes[1][:ch, :cw], p.hmax, p.vmax, H, W) - 128
    cr = upsample(planes[2][:ch, :cw], p.hmax, p.vmax, H, W) - 128
    r = y + ((_fix(1.40200) * cr + 32768) >> 16)
    b = y + ((_fix(1.77200) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + (-_fix(0.71414) * cr + 32768)) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def decode(data: bytes) -> np.ndarray:
    return pixels(parse(data))
