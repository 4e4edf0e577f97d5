"""Plain restatements of the float32-activation conv engine (ehm_conv_nhwc_split, csrc/conv.hip: conv_nhwc_split_kernel), for
tests/test_conv_split_cpu.py and tests/test_gpu_conv_split.py (no GPU, no package import):

  conv_ref64   the convolution in float64 from the exact float32 inputs (torch.nn.functional.conv2d)
  tol          the per-output error bound of the engine
  emulate      a numpy restatement of the engine: f16 halves, one f32 rounding per matrix-core product, the f32 epilogue
  im2col       the gathered operand of the implicit GEMM, zeros at out-of-image taps

The engine computes, for x [N, H, W, Ci] float32, w [Co, Ci, KH, KW], s = w_scale (a power of two),

    y[n, ho, wo, co] = relu?( (1 / s) sum_k A[m, k] W'[co, k] + bias[co] (+ res[m, co]) )

with A the im2col operand (m = (n, ho, wo), k = (kh KW + kw) Ci + ci: tap-major) and W' = f32(w s).

Error model (the one of tests/test_gpu_linear.py's docstring, restated for this engine; a = an entry of A, w unscaled):
  * A is float32, split in the kernel: hi = f16(clamp(a, +-65504)), lo = f16(a - hi); W' is packed by ehm_split_pack the same way.  Either way
    |v - hi - lo| <= 2^-22 |v| + 2^-25 (the last term: lo below the f16 normal range).
  * a product is al.wh + ah.wl + ah.wh, exact in f32; the dropped al.wl and the two representation errors are at most 3 . 2^-22 |a||w| per product,
    plus 2^-25 (|w| + |a| / s) from the floor above.
  * the weights are random-signed and independent of the activations in every case of both test files, so the K per-product errors add like a
    random walk of scale R = sqrt((A^2) . (W^2)^T), taken over the gathered operand (an out-of-image tap is a zero of A).  The bound takes 8 R.
  * f32 accumulation: at most 3K roundings, each <= 2^-24 of a partial sum of scale R + |P|, P = A . W^T: 4 sqrt(3K) . 2^-24 (R + |P|).
  * epilogue: Y is NOT re-split (the linear engine's 2^-21 |Y| term goes).  There are two f32 roundings - the fma with the bias (the product with
    1 / s is exact) and the residual add - each <= 2^-24 of its result, |t - res| and |t| with t the pre-ReLU output; doubled for margin:
    2^-22 (|t| + |res|) covers both.  ReLU is 1-Lipschitz: the same bound holds behind it.
So, with K = KH KW Ci,

    tol = 8 . 2^-20 R + 2^-22 sqrt(3K) (R + |P|) + 2^-25 (sum|w| + sum|a| / s) + 2^-22 (|t| + |res|) + 2^-25

The floor term is what limits the bound's power at small activations: with |a| ~ 1e-3 the lo halves sit in the f16 subnormal range, the floor term
is as large as the product terms, and an engine that drops a whole correction product is off by only 1.4 - 1.6 times the bound (at |a| ~ 1 and above:
20 - 70 times).  That is a property of the split format, not of the bound - the reason the callers bring a cotangent to about 2^10 with
split_gemm.pow2_scale before it enters a GEMM."""
import math

import numpy as np
import torch
import torch.nn.functional as F

F16_MAX = 65504.0


def out_hw(H, W, KH, KW, stride, pad):
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


def im2col(x, KH, KW, stride, pad):
    """x [N, H, W, Ci] (any dtype) -> [N Ho Wo, KH KW Ci], tap-major, zeros at out-of-image taps."""
    N, H, W, Ci = x.shape
    Ho, Wo = out_hw(H, W, KH, KW, stride, pad)
    xp = torch.zeros(N, H + 2 * pad, W + 2 * pad, Ci, dtype=x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    taps = [xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride] for kh in range(KH) for kw in range(KW)]
    return torch.cat(taps, 3).reshape(N * Ho * Wo, KH * KW * Ci)


def weight_rows(w):
    """w [Co, Ci, KH, KW] -> [Co, KH KW Ci], tap-major: the rows the engine's weight operand is packed from."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def conv_ref64(x, w, bias, res, stride, pad, relu):
    """(out, pre) as float64 [N, Ho, Wo, Co]: conv2d + bias (+ res) from the exact float32 x [N, H, W, Ci], w [Co, Ci, KH, KW], bias [Co] or None,
    res [N, Ho, Wo, Co] or None; pre is the value in front of the ReLU."""
    pre = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None if bias is None else bias.double(), stride=stride, padding=pad)
    pre = pre.permute(0, 2, 3, 1).contiguous()
    if res is not None:
        pre = pre + res.double()
    return (torch.relu(pre) if relu else pre), pre


def tol(x, w, res, pre, stride, pad, w_scale):
    """The bound of the module docstring, float64 [N, Ho, Wo, Co]; pre = conv_ref64's pre-ReLU output."""
    Co, _, KH, KW = w.shape
    A = im2col(x.double(), KH, KW, stride, pad)
    W2 = weight_rows(w.double())
    K = W2.shape[1]
    P = A @ W2.t()
    R = torch.sqrt((A * A) @ (W2 * W2).t())
    floor = 2.0 ** -25 * (W2.abs().sum(1)[None, :] + A.abs().sum(1, keepdim=True) / w_scale)
    t = pre.reshape(-1, Co).abs()
    r = torch.zeros_like(t) if res is None else res.double().reshape(-1, Co).abs()
    b = 8 * 2.0 ** -20 * R + 2.0 ** -22 * math.sqrt(3 * K) * (R + P.abs()) + floor + 2.0 ** -22 * (t + r) + 2.0 ** -25
    return b.reshape(pre.shape)


def split_f16(v):
    """float32 array -> (hi, lo) as float64 arrays holding f16 values: hi = f16(clamp(v)), lo = f16(v - hi) (round to nearest even, subnormals kept)."""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = np.clip(v, -F16_MAX, F16_MAX).astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def emulate(x, w, bias, res, stride, pad, relu, w_scale, drop=None):
    """The engine in numpy, float32 [N, Ho, Wo, Co].  Per 16-k group three products of f16 halves - exact, here in float64 - are added into the f32
    accumulator in the kernel's order (al.wh, ah.wl, ah.wh), one rounding each; then . 1/s + bias in one rounding (the fma), + res, ReLU.
    drop in {"alwh", "ahwl"} leaves one correction product out: the wrong engine the bound has to tell from the right one."""
    assert drop in (None, "alwh", "ahwl")
    Co, Ci, KH, KW = w.shape
    N, H, W, _ = x.shape
    Ho, Wo = out_hw(H, W, KH, KW, stride, pad)
    A = im2col(x.float(), KH, KW, stride, pad).numpy()
    Wp = (weight_rows(w.float()).numpy() * np.float32(w_scale)).astype(np.float32)
    M, K = A.shape
    assert K % 16 == 0
    ah, al = (h.reshape(M, K // 16, 16) for h in split_f16(A))
    wh, wl = (h.reshape(Co, K // 16, 16) for h in split_f16(Wp))
    acc = np.zeros((M, Co), np.float32)
    for g in range(K // 16):
        for name, a, b in (("alwh", al, wh), ("ahwl", ah, wl), ("ahwh", ah, wh)):
            if name != drop:
                acc = (acc.astype(np.float64) + a[:, g] @ b[:, g].T).astype(np.float32)
    y = acc.astype(np.float64) / float(w_scale)
    if bias is not None:
        y = y + bias.double().numpy()[None, :]
    y = y.astype(np.float32)
    if res is not None:
        y = y + res.float().reshape(M, Co).numpy()
    if relu:
        y = np.maximum(y, np.float32(0))
    return torch.from_numpy(y.reshape(N, Ho, Wo, Co))


def ratio(got, ref, bound):
    """Largest |got - ref| / bound."""
    return float(((got.double() - ref).abs() / bound).max())
