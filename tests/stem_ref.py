"""Plain restatements of the ResNet stem (ehm_resnet_stem, csrc/stem.hip: stem_pad_kernel / stem_pack_w_kernel / stem_mfma_kernel), for
tests/test_stem_cpu.py and tests/test_gpu_stem.py (no GPU, no package import):

  stem_ref64      conv 7x7 / stride 2 / pad 3 + bias + ReLU + max-pool 3x3 / stride 2 / pad 1 in float64 from the exact float32 inputs
  stem_tol        the per-output error bound of the kernel
  emulate         a numpy restatement of the kernel's arithmetic: f16 halves, one f32 rounding per matrix-core product, bias, ReLU, pool
  split_x2        the X2 row law of the kernel's write-out (float32 rows -> rows of 128 halves)
  decode_x2       an X2 buffer read back -> (hi, lo)
  patches         the host's patch count (ehm_resnet_stem), backward_chunk the image chunk of the backward (csrc/conv_bwd.hip: stem_plan)

The stem is the split-f16 scheme of the float32-activation conv engine with w_scale = 1 and no residual: image and weights are split hi + lo in the
kernel (stem_pack_w_kernel, and in registers in stem_mfma_kernel), a product is al.wh + ah.wl + ah.wh accumulated in f32, the bias is added in f32 and
the output is not re-split before the ReLU.  So every conv pixel carries the bound of tests/conv_split_ref.py (tol; its docstring has the error model) at
stride 2, pad 3, w_scale 1, and - max-pooling being 1-Lipschitz in the max norm: |max_i a_i - max_i b_i| <= max_i |a_i - b_i| - a pooled output carries
the largest bound of its window: the 3x3 / stride 2 / pad 1 max-pool of the tolerance map.  The pool itself adds nothing (a maximum of float32 values is
one of them) and the pool padding is neutral (every window holds a real ReLU output >= 0).

X2 row law (stem.hip's write-out): a pooled pixel is a row of 128 halves; channel c has hi = f16(min(v, 65504)) at half (c >> 5) * 64 + (c & 31) and
lo = f16(v - f32(hi)) 32 halves further on.  v >= 0 behind the ReLU, so only the upper clamp exists."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import conv_split_ref as CR

MP_R, MP_C = 7, 14                   # pooled pixels of a patch (rows, columns)
ROW_HALVES = 128                     # an X2 row of 64 channels


def stem_ref64(img, w, b):
    """(out, pre) float64 NHWC: out [N, H/4, W/4, 64] the pooled output, pre [N, H/2, W/2, 64] the activation in front of the ReLU, from the exact
    float32 img [N, 3, H, W], w [64, 3, 7, 7], b [64]."""
    pre = F.conv2d(img.double(), w.double(), b.double(), stride=2, padding=3)
    out = F.max_pool2d(torch.relu(pre), 3, stride=2, padding=1)
    return out.permute(0, 2, 3, 1).contiguous(), pre.permute(0, 2, 3, 1).contiguous()


def _pool_nhwc(t):
    return F.max_pool2d(t.permute(0, 3, 1, 2), 3, stride=2, padding=1).permute(0, 2, 3, 1).contiguous()


def stem_tol(img, w, b):
    """The bound of the module docstring, float64 [N, H/4, W/4, 64]: conv_split_ref.tol of the conv pixels, max-pooled."""
    out = []
    for n0 in range(0, img.shape[0], 16):                                   # (images are independent: 16 at a time keeps the gathered operand small)
        part = img[n0:n0 + 16]
        _, pre = stem_ref64(part, w, b)
        out.append(_pool_nhwc(CR.tol(part.permute(0, 2, 3, 1).contiguous(), w, None, pre, 2, 3, 1.0)))
    return torch.cat(out)


def emulate(img, w, b, drop=None):
    """The kernel in numpy, float32 [N, H/4, W/4, 64].  K = 21 rows (ci, kh) of eight taps (kw 0..6 and a zero), padded to 22 rows = 11 k-steps of 16;
    per k-step three products of f16 halves - exact, here in float64 - are added into the f32 accumulator in the kernel's order (al.wh, ah.wl, ah.wh),
    one rounding each; then + bias in f32, ReLU, max-pool.  drop in {"alwh", "ahwl"} leaves one correction product out: the wrong stem the bound has to
    tell from the right one."""
    assert drop in (None, "alwh", "ahwl")
    N, _, H, W = img.shape
    Hc, Wc = H // 2, W // 2
    A = CR.im2col(img.float().permute(0, 2, 3, 1).contiguous(), 7, 7, 2, 3).numpy()          # [M, (kh, kw, ci)]
    M = A.shape[0]

    def rows16(t, n):
        """[n, kh, kw, ci] -> [n, 11, 16]: rows (ci, kh), kw 0..6 + one zero, a 22nd row of zeros"""
        t = np.ascontiguousarray(t.transpose(0, 3, 1, 2)).reshape(n, 21, 7)
        out = np.zeros((n, 22, 8), np.float32)
        out[:, :21, :7] = t
        return out.reshape(n, 11, 16)
    ah, al = CR.split_f16(rows16(A.reshape(M, 7, 7, 3), M))
    wh, wl = CR.split_f16(rows16(w.float().permute(0, 2, 3, 1).numpy(), 64))
    acc = np.zeros((M, 64), np.float32)
    for s in range(11):
        for name, a, bb in (("alwh", al, wh), ("ahwl", ah, wl), ("ahwh", ah, wh)):
            if name != drop:
                acc = (acc.astype(np.float64) + a[:, s] @ bb[:, s].T).astype(np.float32)
    y = np.maximum(acc + b.float().numpy()[None, :], np.float32(0))
    return _pool_nhwc(torch.from_numpy(y.reshape(N, Hc, Wc, 64)))


def split_x2(v):
    """float32 [pixels, 64] (tensor or array, >= 0) -> int16 array [pixels, 128]: the bit patterns of the X2 rows the kernel writes for them."""
    v = np.asarray(v, np.float32)
    assert v.ndim == 2 and v.shape[1] == 64
    with np.errstate(over="ignore", invalid="ignore"):
        hi = np.fmin(v, np.float32(CR.F16_MAX)).astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    rows = np.stack([hi.reshape(-1, 2, 32), lo.reshape(-1, 2, 32)], axis=2)                   # [pixels, 32-channel group, hi / lo, 32]
    return np.ascontiguousarray(rows.reshape(-1, ROW_HALVES)).view(np.int16)


def decode_x2(buf, pixels):
    """An X2 buffer - a tensor (any 2- or 4-byte dtype, read back from the device) or an array of halves / their bit patterns, rows of 128 halves -
    -> (hi, lo) float16 arrays [pixels, 64]."""
    if isinstance(buf, torch.Tensor):
        buf = buf.detach().cpu().contiguous().view(torch.int16).numpy()
    h = np.ascontiguousarray(buf).view(np.float16).reshape(-1, 2, 2, 32)[:pixels]
    return h[:, :, 0, :].reshape(pixels, 64), h[:, :, 1, :].reshape(pixels, 64)


def patches(N, H, W):
    """The patches ehm_resnet_stem deals out: 7 x 14 pooled pixels each, per image."""
    Hq, Wq = H // 4, W // 4
    return N * ((Hq + MP_R - 1) // MP_R) * ((Wq + MP_C - 1) // MP_C)


def backward_chunk(H, W):
    """The images ehm_resnet_stem_backward takes at a time: 8 Mi floats of pre-pool activations (before the cap at N)."""
    return max(1, (8 << 20) // ((H // 2) * (W // 2) * 64))
