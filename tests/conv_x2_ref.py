"""Plain restatements of the X2 conv engine (ehm_conv_x2, csrc/conv.hip: conv_x2_tile_kernel), for tests/test_conv_x2_cpu.py and
tests/test_gpu_conv_x2.py (no GPU, no package import):

  split_x2 / pack_x2 / unpack_x2 / pack_weight   the ehm_split_pack layout on the host: per 32 columns 32 hi halves, then 32 lo halves
  operands      the implicit GEMM's operands as exact halves: A = [im2col(x) | x2 sampled] and W' = [W | W2] s, each as (hi, lo)
  conv_ref64    the convolution in float64 of the values the engine READS (hi + lo decoded exactly; the hi halves alone in the hi-only tier)
  tol           the per-output error bound of the engine
  emulate       a numpy restatement of the engine in the kernel's product order, with the output re-split and the hi-only tier
  selector_weights / selector_expected   weights that copy one tap's channels to the output, and the bits y must then hold

The engine computes, for X2 activations x [N, H, W, Ci] (and x2 [N, H2, W2, Ci2]), w [Co, Ci, KH, KW] (w2 [Co, Ci2]), s = w_scale (a power of two),

    y[m, co] = X2( relu?( (1 / s) sum_k A[m, k] W'[co, k] + bias[co] (+ res[m, co]) ) )

with m = (n, ho, wo), k = (kh KW + kw) Ci + ci (tap-major) and behind them the Ci2 channels of x2's pixel (stride2 ho, stride2 wo).

Error model.  The reference is taken from the DECODED operands a = ah + al, w' = wh + wl, r = rh + rl, so no representation error of an input enters.
Split tier (x2_mm16 in csrc/x2_tile_dev.h: per 32-k tile al.wh, ah.wl, ah.wh on the 16 x 16 x 32 matrix-core instruction):
  * dropped product: the engine leaves al.wl out.  Both factors are known here, so the bound takes the sum itself in the worst case,
    D = (|Al| . |Wl|^T) / s - no random-walk argument.  (Per product it is at most 2^-22 |a||w|: a lo half is at most half an ulp of its hi half.)
  * f32 accumulation: the three products of a k-step are exact in f32 (11 x 11 bits); the matrix cores add them into the f32 accumulator with
    at most one rounding per 16 k and product - n = 3 K / 16 roundings, each <= 2^-24 of a partial sum.  The partial sums have the scale R + |P| with
    P = A . W'^T / s and R = sqrt((A^2) . (W'^2)^T) / s, the random-walk scale of conv_split_ref (random-signed weights drawn independently of the
    activations in every case of both test files).  The roundings add like a walk of n steps: sqrt(n) . 2^-24 (R + |P|), taken 4 times for the
    tail over all outputs (for n <= 16 that also covers the worst case n . 2^-24).  Stream-K adds the partial sums of up to two more blocks to the
    owner's: two more roundings of sums of the same scale, taken in the worst case with the same factor: 4 . 2 . 2^-24 (R + |P|).
  * epilogue: t1 = fma(acc, 1 / s, bias) - the product with a power of two is exact, one rounding <= 2^-24 |t1|; then t = t1 + (rh + rl) - rh + rl is
    exact in f32 for halves that came from a float32, one rounding <= 2^-24 |t| (two if a compiler adds the halves one by one).  With |t1| <= |t| + |r|:
    3 . 2^-24 (|t| + |r|) <= 2^-22 (|t| + |r|).  ReLU is 1-Lipschitz: the same bound holds behind it.
  * re-split of y (|y| <= |t|): hi = f16(y), y - hi exact in f32, lo = f16(y - hi): |y - hi - lo| <= 2^-11 |y - hi| <= 2^-22 |y|, or 2^-25 when lo falls
    below the f16 normal range.  (Valid for |y| <= 65504; past it the FP16_OVFL mode clamps hi: tests/test_gpu_conv_x2.py pins that separately.)

    split:    tol = D + 4 . 2^-24 (sqrt(3 K / 16) + 2 [stream-K]) (R + |P|) + 2^-22 (|t| + |r|) + 2^-22 |t| + 2^-25

Hi-only tier (x2_mfmas with SPLIT = false: one ah.wh product per 16 k on the 32 x 32 x 16 instruction; reference = the hi halves alone, r = rh):
  * accumulation: n = K / 16 roundings, as above with R, P of the hi halves;
  * epilogue: as above, 2^-22 (|t| + |r|);
  * y is ONE f16: |y - f16(y)| <= 2^-11 |y|, or 2^-25 below the normal range.

    hi-only:  tol = 4 . 2^-24 (sqrt(K / 16) + 2 [stream-K]) (R + |P|) + 2^-22 (|t| + |r|) + 2^-11 |t| + 2^-25

What the bound can tell apart (tests/test_conv_x2_cpu.py): an engine without al.wh or ah.wl is off by about 2^-12 R, the accumulation term is about
2^-22 sqrt(K) R - at activations of order 1 and above such an engine misses the bound by one to two orders of magnitude.  Below that the lo halves
reach the f16 subnormal range and a correction product shrinks to the 2^-25 floor: conv_split_ref's docstring."""
import math

import numpy as np
import torch

from tests.conv_split_ref import F16_MAX, im2col, out_hw, weight_rows  # noqa: F401  (out_hw: re-exported for the two test files)

G = 32                               # values per hi / lo group of the X2 layout
XBM = 192                            # rows of the engine's output tile (ehm_conv_x2_rows pads to it)
NAN_HALF = 0x7E00                    # a quiet NaN as f16 bits


def round_up(a, b):
    return -(-a // b) * b


def x2_rows(pixels):
    """ehm_conv_x2_rows: the tile padding and the zero row"""
    return round_up(pixels, XBM) + 1


# ------------------------------------------------------------------------------------------------ the layout
def split_x2(v):
    """float32 tensor -> (hi, lo) float16 tensors as ehm_split_pack stores a FINITE or infinite value: hi = f16(clamp(v, +-65504)),
    lo = f16(clamp(v - hi, +-65504)), round to nearest even, subnormals kept.  (A NaN is not a value of the format: the device packer's fmin / fmax
    clamps turn it into -131008; the tests that need a NaN half write the halves themselves, pack_halves.)"""
    v = v.float()
    hi = v.clamp(-F16_MAX, F16_MAX).half()
    lo = (v - hi.float()).clamp(-F16_MAX, F16_MAX).half()
    return hi, lo


def pack_halves(hi, lo):
    """(hi, lo) float16 [rows, C] -> the X2 row image, float16 [rows, 2 C]: per 32 columns 32 hi halves, then 32 lo halves"""
    rows, c = hi.shape
    assert c % G == 0 and lo.shape == hi.shape
    return torch.stack([hi.reshape(rows, c // G, G), lo.reshape(rows, c // G, G)], 2).reshape(rows, 2 * c).contiguous()


def unpack_halves(buf):
    """the inverse of pack_halves: float16 [rows, 2 C] -> (hi, lo) float16 [rows, C]"""
    rows, c2 = buf.shape
    assert c2 % (2 * G) == 0
    b = buf.reshape(rows, c2 // (2 * G), 2, G)
    return b[:, :, 0].reshape(rows, c2 // 2), b[:, :, 1].reshape(rows, c2 // 2)


def pack_x2(v):
    """float32 [rows, C] -> float16 [rows, 2 C], what ehm_split_pack(v, scale = 1) writes"""
    return pack_halves(*split_x2(v))


def unpack_x2(buf):
    """float16 [rows, 2 C] -> the decoded values hi + lo, float64 [rows, C] (exact)"""
    hi, lo = unpack_halves(buf)
    return hi.double() + lo.double()


def x2_buffer(v, rows=None, fill=NAN_HALF):
    """float32 [pixels, C] -> an activation buffer of `rows` rows (default: x2_rows(pixels)): the pixels, then padding rows whose every half has the
    bits `fill`, then the all-zero row as the LAST row."""
    pixels, c = v.shape
    rows = x2_rows(pixels) if rows is None else rows
    assert rows >= x2_rows(pixels)
    buf = torch.full((rows, 2 * c), fill, dtype=torch.int16).view(torch.float16)
    buf[:pixels] = pack_x2(v)
    buf[rows - 1] = 0
    return buf


def weight_operand(w, s, w2=None):
    """w [Co, Ci, KH, KW] (w2 [Co, Ci2]) -> W' float32 [Co padded to 128, K]: tap-major rows, [W | W2] along K, times s, zero rows behind Co"""
    rows = weight_rows(w.float())
    if w2 is not None:
        rows = torch.cat([rows, w2.float()], 1)
    Co, K = rows.shape
    assert K % G == 0
    out = torch.zeros(round_up(Co, 128), K)
    out[:Co] = rows * float(s)
    return out


def pack_weight(w, s, w2=None):
    """the engine's weight operand, float16 [Co padded to 128, 2 K]"""
    return pack_x2(weight_operand(w, s, w2))


# ------------------------------------------------------------------------------------------------ the operands the engine reads
def gather(x, geom, x2=None, stride2=1):
    """x [N, H, W, Ci] (x2 [N, H2, W2, Ci2]) of any dtype -> the GEMM's A [M, K]: im2col(x), zeros at out-of-image taps, then x2's pixels
    (stride2 ho, stride2 wo)"""
    KH, KW, stride, pad = geom
    A = im2col(x, KH, KW, stride, pad)
    if x2 is not None:
        s2 = x2[:, ::stride2, ::stride2]
        assert s2.shape[0] * s2.shape[1] * s2.shape[2] == A.shape[0]
        A = torch.cat([A, s2.reshape(A.shape[0], -1)], 1)
    return A


class Operands:
    """Ah, Al [M, K] and Wh, Wl [Co, K] as float64 tensors holding f16 values; s"""

    def __init__(self, x, w, s, geom, x2=None, w2=None, stride2=1):
        xh, xl = split_x2(x)
        if x2 is not None:
            x2h, x2l = split_x2(x2)
            self.Ah, self.Al = gather(xh.double(), geom, x2h.double(), stride2), gather(xl.double(), geom, x2l.double(), stride2)
        else:
            self.Ah, self.Al = gather(xh.double(), geom), gather(xl.double(), geom)
        wh, wl = split_x2(weight_operand(w, s, w2)[:w.shape[0]])
        self.Wh, self.Wl, self.s = wh.double(), wl.double(), float(s)
        self.M, self.K, self.Co = self.Ah.shape[0], self.Ah.shape[1], w.shape[0]
        assert self.Wh.shape == (self.Co, self.K) and self.K % G == 0


def _res_halves(res, M, Co):
    if res is None:
        return None, None
    rh, rl = split_x2(res.reshape(M, Co))
    return rh.double(), rl.double()


def conv_ref64(ops, bias, res, relu, hi_only=False):
    """(out, pre) float64 [M, Co] from the decoded operands: A . W'^T / s + bias (+ res); pre is the value in front of the ReLU.  hi_only: the hi
    halves of A, W' and res alone.  bias float32 [Co] or None, res float32 [M, Co] (any shape of M Co values) or None."""
    A, W = (ops.Ah, ops.Wh) if hi_only else (ops.Ah + ops.Al, ops.Wh + ops.Wl)
    pre = A @ W.t() / ops.s
    if bias is not None:
        pre = pre + bias.double()[None, :]
    rh, rl = _res_halves(res, ops.M, ops.Co)
    if res is not None:
        pre = pre + (rh if hi_only else rh + rl)
    return (torch.relu(pre) if relu else pre), pre


def tol(ops, res, pre, hi_only=False, stream_k=False):
    """The bound of the module docstring, float64 [M, Co]; pre = conv_ref64's pre-ReLU output of the same tier."""
    A, W = (ops.Ah, ops.Wh) if hi_only else (ops.Ah + ops.Al, ops.Wh + ops.Wl)
    P = (A @ W.t()).abs() / ops.s
    R = torch.sqrt((A * A) @ (W * W).t()) / ops.s
    n = ops.K / 16 if hi_only else 3 * ops.K / 16
    acc = 4 * 2.0 ** -24 * (math.sqrt(n) + (2 if stream_k else 0)) * (R + P)
    t = pre.abs()
    rh, rl = _res_halves(res, ops.M, ops.Co)
    r = torch.zeros_like(t) if res is None else (rh if hi_only else rh + rl).abs()
    epi = 2.0 ** -22 * (t + r)
    if hi_only:
        return acc + epi + 2.0 ** -11 * t + 2.0 ** -25
    D = ops.Al.abs() @ ops.Wl.abs().t() / ops.s
    return D + acc + epi + 2.0 ** -22 * t + 2.0 ** -25


# ------------------------------------------------------------------------------------------------ the engine in numpy
def emulate(ops, bias, res, relu, hi_only=False, drop=None, cuts=None):
    """The engine in numpy -> (hi, lo) float16 tensors [M, Co] (lo = None in the hi-only tier).
    Split tier: per 32-k tile three products of f16 halves - exact, here in float64 - are added into the f32 accumulator in the order of x2_mm16
    (al.wh, ah.wl, ah.wh), one rounding each.  Hi-only tier: per 16-k step the one product ah.wh (x2_mfmas, SPLIT = false).  Then fma(acc, 1 / s, bias),
    + (rh + rl) (hi-only: + rh), ReLU, and the re-split under FP16_OVFL: hi = f16(clamp(v)), lo = f16(clamp(v - hi)).
    drop in {"xlwh", "xhwl"} leaves one correction product out - the wrong engine the bound has to tell from the right one.
    cuts: K-tile indices at which stream-K cuts the K loop, e.g. (12, 24): every run has its own accumulator and the later runs' sums are added to
    the first one's in k order."""
    assert drop in (None, "xlwh", "xhwl") and not (hi_only and drop)
    M, K, Co = ops.M, ops.K, ops.Co
    step = 16 if hi_only else G
    ah, al = (h.numpy().reshape(M, K // step, step) for h in (ops.Ah, ops.Al))
    wh, wl = (h.numpy().reshape(Co, K // step, step) for h in (ops.Wh, ops.Wl))
    terms = (("xhwh", ah, wh),) if hi_only else (("xlwh", al, wh), ("xhwl", ah, wl), ("xhwh", ah, wh))
    bounds = [0] + [c * (G // step) for c in (cuts or ())] + [K // step]
    parts = []
    for g0, g1 in zip(bounds[:-1], bounds[1:]):
        assert g0 < g1
        acc = np.zeros((M, Co), np.float32)
        for g in range(g0, g1):
            for name, a, b in terms:
                if name != drop:
                    acc = (acc.astype(np.float64) + a[:, g] @ b[:, g].T).astype(np.float32)
        parts.append(acc)
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p                                                                  # (float32 + float32: one rounding)
    v = acc.astype(np.float64) / ops.s
    if bias is not None:
        v = v + bias.double().numpy()[None, :]
    v = v.astype(np.float32)
    rh, rl = _res_halves(res, M, Co)
    if res is not None:
        v = v + (rh if hi_only else rh + rl).numpy().astype(np.float32)
    if relu:
        v = np.maximum(v, np.float32(0))
    v = torch.from_numpy(v)
    inf = torch.isinf(v)                                                               # (FP16_OVFL clamps an overflow, not an infinity)
    hi = torch.where(inf, v, v.clamp(-F16_MAX, F16_MAX)).half()
    if hi_only:
        return hi, None
    return hi, torch.where(inf, torch.full_like(v, float("nan")), (v - hi.float()).clamp(-F16_MAX, F16_MAX)).half()


def decoded(hi, lo=None):
    """float64 value of an output (hi-only tier: lo = None)"""
    return hi.double() if lo is None else hi.double() + lo.double()


def ratio(got, ref, bound):
    """Largest |got - ref| / bound (got, ref float64); a non-finite `got` gives inf."""
    e = (got - ref).abs() / bound
    e = torch.where(torch.isfinite(got), e, torch.full_like(e, float("inf")))
    return float(e.max())


# ------------------------------------------------------------------------------------------------ exact gather
def selector_weights(KH, KW, Ci, Co, tap):
    """w [Co, Ci, KH, KW] of zeros and ones: output channel co copies channel co % Ci of tap `tap` (= kh KW + kw).  Packed with a power-of-two s every
    weight is 0 or s (lo half 0), so the engine's sum is s (xh + xl) - exact in f32 - and y is the re-split of the gathered value."""
    w = torch.zeros(Co, Ci, KH, KW)
    co = torch.arange(Co)
    w[co, co % Ci, tap // KW, tap % KW] = 1.0
    return w


def selector_expected(x, geom, Co, tap):
    """The halves y must hold BIT FOR BIT under selector_weights: (hi, lo) float16 [M, Co] = the X2 split of the decoded value xh + xl of tap `tap`'s
    pixel, channel co % Ci; zeros at an out-of-image tap.  Splitting hi + lo again returns the same halves except where lo is exactly half an ulp of hi
    and hi is odd (the sum is a tie and rounds to the even neighbour: hi + 2 lo, -lo) - about one value in 2^13, more where lo is an f16 subnormal of a
    few bits - which is why the expectation is the re-split and not the input halves.  The hi-only tier: selector_expected_hi_only."""
    Ci = x.shape[3]
    xh, xl = split_x2(x)
    A = gather(xh.float() + xl.float(), geom)                        # (exact: both halves came from one float32)
    cols = tap * Ci + torch.arange(Co) % Ci
    return split_x2(A[:, cols])


def selector_expected_hi_only(x, geom, Co, tap):
    """float16 [M, Co]: the gathered hi halves themselves"""
    Ci = x.shape[3]
    A = gather(split_x2(x)[0], geom)
    return A[:, tap * Ci + torch.arange(Co) % Ci]
