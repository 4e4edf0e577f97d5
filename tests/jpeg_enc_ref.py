"""A numpy restatement of the baseline-JPEG ENCODING rule of include/egohmr_hip.h (section "JPEG encoding"): libjpeg's default encoder -
its fixed-point colour conversion, chroma downsampling with its padding order, the ISLOW integer forward DCT, its quantiser, the dummy
blocks of the MCU padding, the fixed Annex K Huffman tables, byte stuffing and the marker segments in the order PIL writes them.  It is the
reference of tests/test_jpeg_enc_cpu.py (where it is compared with PIL's bytes), tests/test_gpu_jpeg_enc.py and, with one table row per
component and its planted mistakes (``wrong=``), of tests/test_gpu_jpeg_kernels.py.  Slow and plain on purpose.
"""
from __future__ import annotations

import numpy as np

from jpeg_ref import ZIGZAG

SAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}

BASE_QUANT = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32])

# Annex K.3 - K.6: (counts per code length 1..16, symbols), in the order of the DHT segments: DC0, AC0, DC1, AC1
_AC_LUMA = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546474849"
    "4a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
    "c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN = (
    (0x00, [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0x10, [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], list(_AC_LUMA)),
    (0x01, [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (0x11, [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], list(_AC_CHROMA)),
)


def quality_tables(quality: int) -> np.ndarray:
    """uint16 [2, 64], natural order: libjpeg's scaling of the Annex K tables (jpeg_set_quality, force_baseline)."""
    if not 1 <= quality <= 100:
        raise ValueError("quality outside 1..100")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((BASE_QUANT * s + 50) // 100, 1, 255).astype(np.uint16)


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc(rgb):
    """uint8 [H, W, 3] RGB -> three int32 [H, W] planes (jccolor.c)."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_fix(.29900) * r + _fix(.58700) * g + _fix(.11400) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.50000) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.50000) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return [p.astype(np.int32) for p in (y, cb, cr)]


def _extend(p, rows, cols):
    """Repeats the last row / column up to the given size."""
    p = np.concatenate([p, np.repeat(p[-1:], rows - p.shape[0], 0)], 0) if rows > p.shape[0] else p
    return np.concatenate([p, np.repeat(p[:, -1:], cols - p.shape[1], 1)], 1) if cols > p.shape[1] else p


def component_planes(rgb, hmax, vmax, wrong=None):
    """-> [(samples int32 [rh * 8, rw * 8], rw, rh)] per component: the REAL block grid's samples (jcprepct.c / jcsample.c)."""
    H, W = rgb.shape[:2]
    out = []
    if wrong == "odd_height_reads_padding" and vmax == 2 and H % 2:    # the row under the frame read as it is (black here), not as row H - 1
        rgb = np.concatenate([rgb, np.zeros_like(rgb[:1])], 0)
    for c, full in enumerate(ycc(rgb)):
        h, v = (hmax, vmax) if c == 0 else (1, 1)
        fh, fv = hmax // h, vmax // v
        rw, rh = -(-W * h // (8 * hmax)), -(-H * v // (8 * vmax))
        full = full[:-(-H // fv) * fv]
        p = _extend(full, -(-H // fv) * fv, rw * 8 * fh)           # columns to the block grid, rows only to a multiple of the factor
        if (fh, fv) == (2, 1):
            bias = np.arange(p.shape[1] // 2) & 1
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        elif (fh, fv) == (2, 2):
            bias = 1 + (np.arange(p.shape[1] // 2) & 1)
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        out.append((_extend(p, rh * 8, rw * 8), rw, rh))           # rows to the block grid AFTER downsampling
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One 1-D pass of jfdctint over the LAST axis of int32 d[..., 8]."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i].astype(np.int32) for i in range(8))
    t0, t1, t2, t3 = d0 + d7, d1 + d6, d2 + d5, d3 + d4
    t7, t6, t5, t4 = d0 - d7, d1 - d6, d2 - d5, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o0 = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o4 = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o2 = _descale(z1 + t13 * 6270, n)
    o6 = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    o7, o5, o3, o1 = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], -1)


def fdct_quant(samples, quant):
    """samples int32 [rh * 8, rw * 8], quant [64] -> quantised int32 [rh, rw, 64] (natural order)."""
    rh, rw = samples.shape[0] // 8, samples.shape[1] // 8
    x = samples.reshape(rh, 8, rw, 8).transpose(0, 2, 1, 3) - 128
    x = _fdct_pass(x, True)                                         # rows
    x = _fdct_pass(x.swapaxes(-1, -2), False).swapaxes(-1, -2)      # columns
    x = x.reshape(rh, rw, 64)
    d = 8 * quant.astype(np.int32)
    a = np.abs(x) + (d >> 1)
    r = np.where(a >= d, a // d, 0)
    return np.where(x < 0, -r, r)


FORWARD_WRONG = ("cr_uses_cb_table", "quant_of_frame0", "bgr_as_rgb", "dummy_keeps_ac", "dummy_row_from_left", "odd_height_reads_padding")


def coefficient_planes(rgb, quant, hmax, vmax, wrong=None, quant0=None):
    """rgb uint8 [H, W, 3], quant [2, 64] (luma, both chroma planes) or [3, 64] (one row per component, ehm_jpeg_forward's) -> three int16
    planes [blocks_y, blocks_x, 64] over the MCU grid, dummy blocks included.
    wrong: one of FORWARD_WRONG, a planted mistake (quant_of_frame0 takes the rows from ``quant0``, frame 0's)."""
    assert wrong is None or wrong in FORWARD_WRONG
    quant = np.asarray(quant0 if wrong == "quant_of_frame0" else quant)
    assert quant.shape in ((2, 64), (3, 64))
    rows = [0, 1, 1] if len(quant) == 2 or wrong == "cr_uses_cb_table" else [0, 1, 2]
    if wrong == "bgr_as_rgb":
        rgb = rgb[..., ::-1]
    H, W = rgb.shape[:2]
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    planes = []
    for c, (samples, rw, rh) in enumerate(component_planes(rgb, hmax, vmax, wrong)):
        h, v = (hmax, vmax) if c == 0 else (1, 1)
        real = fdct_quant(samples, quant[rows[c]])
        out = np.zeros((my * v, mx * h, 64), np.int32)
        out[:rh, :rw] = real
        keep = 64 if wrong == "dummy_keeps_ac" else 1               # all AC of a dummy block are zero
        for by in range(rh):                                        # dummy columns of real rows: the DC of the block to the left
            for bx in range(rw, mx * h):
                out[by, bx, :keep] = out[by, bx - 1, :keep]
        for by in range(rh, my * v):                                # dummy rows: the DC of the MCU's last block of the row above
            for m in range(mx):
                out[by, m * h:(m + 1) * h, :keep] = out[by - 1, m * h + h - 1, :keep]
            if wrong == "dummy_row_from_left":
                for bx in range(1, mx * h):
                    out[by, bx, 0] = out[by, bx - 1, 0]
        planes.append(out.astype(np.int16))
    return planes


def coefficients(rgb, quant, hmax, vmax, wrong=None, quant0=None):
    """The decoder's layout: the planes one after the other, int16 [coef_count]."""
    return np.concatenate([p.reshape(-1) for p in coefficient_planes(rgb, quant, hmax, vmax, wrong, quant0)])


def split_planes(coef, H, W, hmax, vmax):
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    shapes = [(my * vmax, mx * hmax), (my, mx), (my, mx)]
    out, o = [], 0
    for by, bx in shapes:
        out.append(np.asarray(coef[o:o + by * bx * 64]).reshape(by, bx, 64))
        o += by * bx * 64
    assert o == len(coef)
    return out


def _codes(counts, symbols):
    """{symbol: (code, length)} of the canonical code."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


_DC = [_codes(HUFFMAN[0][1], HUFFMAN[0][2]), _codes(HUFFMAN[2][1], HUFFMAN[2][2])]
_AC = [_codes(HUFFMAN[1][1], HUFFMAN[1][2]), _codes(HUFFMAN[3][1], HUFFMAN[3][2])]


def _value_bits(v):
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v - 1) & ((1 << s) - 1)


def block_bits(blk, pred, t, out):
    """Appends (value, length) pairs of one block to out."""
    s, bits = _value_bits(int(blk[0]) - pred)
    out.append(_DC[t][s])
    if s:
        out.append((bits, s))
    run = 0
    for k in range(1, 64):
        v = int(blk[ZIGZAG[k]])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(_AC[t][0xF0])
            run -= 16
        s, bits = _value_bits(v)
        out.append(_AC[t][(run << 4) | s])
        out.append((bits, s))
        run = 0
    if run:
        out.append(_AC[t][0x00])


def packed_stream(planes, hmax, vmax):
    """The scan's bits before stuffing: bytes, the last one padded with 1 bits."""
    my, mx = planes[1].shape[:2]
    pairs, pred = [], [0, 0, 0]
    for m in range(mx * my):
        y, x = divmod(m, mx)
        for c in range(3):
            h, v = (hmax, vmax) if c == 0 else (1, 1)
            for vy in range(v):
                for hx in range(h):
                    blk = planes[c][y * v + vy, x * h + hx]
                    block_bits(blk, pred[c], min(c, 1), pairs)
                    pred[c] = int(blk[0])
    out, acc, n = bytearray(), 0, 0
    for value, length in pairs:
        acc = (acc << length) | value
        n += length
        while n >= 8:
            n -= 8
            out.append(acc >> n)
            acc &= (1 << n) - 1
    if n:
        out.append((acc << (8 - n)) | ((1 << (8 - n)) - 1))
    return bytes(out)


def stuff(data: bytes) -> bytes:
    return data.replace(b"\xff", b"\xff\x00")


def scan_bytes(planes, hmax, vmax) -> bytes:
    return stuff(packed_stream(planes, hmax, vmax))


def header(H, W, hmax, vmax, quant) -> bytes:
    """SOI, APP0 JFIF 1.01, DQT 0, DQT 1, SOF0, DHT DC0 AC0 DC1 AC1, SOS."""
    seg = lambda marker, body: bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2):
        out += seg(0xDB, bytes([t]) + bytes(int(quant[t][z]) for z in ZIGZAG))
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, (hmax << 4) | vmax, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tid, counts, symbols in HUFFMAN:
        out += seg(0xC4, bytes([tid]) + bytes(counts) + bytes(symbols))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode(rgb, quant, hmax, vmax) -> bytes:
    """rgb uint8 [H, W, 3], quant uint16 [2, 64] -> the whole file."""
    H, W = rgb.shape[:2]
    return header(H, W, hmax, vmax, quant) + scan_bytes(coefficient_planes(rgb, quant, hmax, vmax), hmax, vmax) + b"\xff\xd9"


def scan_of(data: bytes) -> bytes:
    """The bytes of a file from the end of SOS to (not including) EOI."""
    pos = 2
    while data[pos + 1] != 0xDA:
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    assert data[-2:] == b"\xff\xd9"
    return data[pos:-2]


def segment(data: bytes, marker: int, which: int = 0) -> bytes:
    """The which-th segment with this marker byte, FF xx and length included."""
    pos = 2
    while True:
        n = (data[pos + 2] << 8) | data[pos + 3]
        if data[pos + 1] == marker:
            if which == 0:
                return data[pos:pos + 2 + n]
            which -= 1
        if data[pos + 1] == 0xDA:
            raise KeyError(marker)
        pos += 2 + n
