"""The host side of the split-f16 row GEMM: float32 rows times an ``ehm_split_pack``'ed weight on ehm_conv_nhwc_split with H = W = 1.

The engine splits its float32 row operand into f16 hi + lo halves, so a weight is multiplied by a power of two that brings its largest entry to about
2^11 before it is packed (weight_scale), and a cotangent by one that brings it to 2^10 before it enters a GEMM (pow2_scale: computed on the device);
the products are divided by it again (both exact).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from . import _lib


def round_up(n, m):
    return (n + m - 1) // m * m


def weight_scale(amax):
    """The power of two a weight matrix of largest magnitude `amax` is packed with; 1 for an all-zero or non-finite one.  It brings amax into
    (1024, 2048] and stops at 2^126: the engine takes it and its reciprocal as float32, and past 2^127 the one is inf and the other flushes (a
    matrix whose largest entry is below 2^-115 is packed below 2048 instead)."""
    if not 0.0 < amax < float("inf"):
        return 1.0
    r = 2048.0 / amax
    return 2.0 ** min(math.floor(math.log2(r)), 126) if r < float("inf") else 2.0 ** 126


class Packed(NamedTuple):
    buf: torch.Tensor               # X2 [Co padded to 128, K padded to 32]
    scale: float
    cols: int                       # Co rounded up to 8: the column count ehm_conv_nhwc_split writes
    bias: Optional[torch.Tensor]    # float32 [cols] (zeros behind Co) or None


def pack_weight(w2, bias=None):
    """float32 [Co, K] on a HIP device -> Packed (ehm_split_pack, scaled by weight_scale).  The engine reads bias[0 .. cols): a bias [Co] with
    Co % 8 != 0 is zero-padded to cols here (the padding columns then come out as the residual alone, or zero).  A contiguous float32 matrix that has the
    padded shape already (Co % 128 == 0, K % 32 == 0) is packed as it is: no zero-filled copy."""
    Co, K = w2.shape
    wp = w2
    if Co % 128 or K % 32 or not w2.is_contiguous() or w2.dtype != torch.float32:
        wp = torch.zeros(round_up(Co, 128), round_up(K, 32), device=w2.device)
        wp[:Co, :K] = w2
    scale = weight_scale(float(wp.abs().max()))
    buf = torch.empty_like(wp)
    _lib.api().ehm_split_pack(wp, buf, wp.shape[0], wp.shape[1], wp.shape[1], scale, _lib.stream_ptr())
    cols = round_up(Co, 8)
    if bias is not None and bias.shape[0] != cols:
        bias = torch.cat([bias, bias.new_zeros(cols - bias.shape[0])])
    return Packed(buf, scale, cols, bias)


def gemm_rows(x, packed, rows=None, res=None, out=None):
    """x [M, Ci] float32 (Ci a multiple of 32, contiguous) times a Packed operand (+ its bias, + res [rows, cols]) -> [rows or M, cols] float32,
    written to `out` when given."""
    M = x.shape[0] if rows is None else rows
    y = torch.empty(M, packed.cols, device=x.device) if out is None else out
    P = _lib.ptr
    d = _lib.ConvDesc(P(x), P(packed.buf), P(packed.bias), P(res), P(y), M, 1, 1, x.shape[1], packed.cols, 1, 1, 1, 0, 0, packed.scale)
    _lib.api().ehm_conv_nhwc_split(C.byref(d), _lib.stream_ptr())
    return y


def pow2_scale(t, target=1024.0):
    """0-d device tensor: the power of two that brings max|t| into [target/2, target]; 1 for an all-zero or non-finite t.  No host read-back."""
    lo, hi = torch.aminmax(t)                                   # one pass, no |t| temporary
    a = torch.maximum(-lo, hi)
    s = torch.exp2(torch.floor(torch.log2(target / a)))
    return torch.where((a > 0) & torch.isfinite(s) & (s > 0), s, torch.ones_like(s))


def pad_cols(x2d, Kp):
    """float32 [rows, K] -> [rows, Kp] with zeros behind column K (the engine's K granule is 32)."""
    xp = torch.zeros(x2d.shape[0], Kp, device=x2d.device)
    xp[:, :x2d.shape[1]] = x2d
    return xp
