"""CPU: the error bound of tests/conv_split_ref.py tells the float32-activation conv engine (ehm_conv_nhwc_split) from an engine that drops one of
its two correction products, the host helpers of egohmr_amd/split_gemm.py on their edges, and the refusals of ehm_conv_nhwc_split (before any device
call).  The GPU side is tests/test_gpu_conv_split.py.

The bound discriminates at activations of order 1 and above (the emulated engine at 0.03 - 0.11 of it, either mutant above it); at |a| ~ 1e-3 the lo
halves of the activations sit in the f16 subnormal range, the floor term of the bound is as large as a whole correction product, and a mutant is only
about 1.5 times over.  Every case that has to discriminate therefore uses activations of order 1 or larger - a condition on the inputs, the bound is
the same - and the callers of the engine bring their cotangents to about 2^10 with split_gemm.pow2_scale for the same reason."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import conv_split_ref as CR

MUTANTS = ("alwh", "ahwl")
# (N, H, W, Ci, Co, KH, KW, stride, pad): three GEMM-shaped cases (M, K, Co) = (128, 32, 128), (256, 576, 128), (128, 2304, 64) and a 3 x 3 stride-2 conv
CASES = [(128, 1, 1, 32, 128, 1, 1, 1, 0), (256, 1, 1, 576, 128, 1, 1, 1, 0), (128, 1, 1, 2304, 64, 1, 1, 1, 0), (2, 8, 8, 64, 64, 3, 3, 2, 1)]


def _inputs(case, seed, act=1.0, epilogue=False):
    """standard-normal activations (times act), He-scaled weights, the scale weight_scale gives them; with epilogue: bias, residual and ReLU"""
    from egohmr_amd.split_gemm import weight_scale
    N, H, W, Ci, Co, KH, KW, stride, pad = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Ci, generator=g) * act
    w = torch.randn(Co, Ci, KH, KW, generator=g) * math.sqrt(2.0 / (Ci * KH * KW))
    Ho, Wo = CR.out_hw(H, W, KH, KW, stride, pad)
    bias = torch.randn(Co, generator=g) * act if epilogue else None
    res = torch.randn(N, Ho, Wo, Co, generator=g) * act if epilogue else None
    return dict(x=x, w=w, bias=bias, res=res, stride=stride, pad=pad, relu=int(epilogue)), weight_scale(float(w.abs().max()))


def _ratios(kw, s):
    """error / bound of the emulated engine and of its two mutants"""
    ref, pre = CR.conv_ref64(**kw)
    bound = CR.tol(kw["x"], kw["w"], kw["res"], pre, kw["stride"], kw["pad"], s)
    return [CR.ratio(CR.emulate(**kw, w_scale=s, drop=d), ref, bound) for d in (None,) + MUTANTS]


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_bound_tells_the_engine_from_one_without_a_correction_product(case, epilogue):
    r = _ratios(*_inputs(case, seed=sum(case), epilogue=epilogue))
    print(f"[{case} epilogue={epilogue}] err/bound: engine {r[0]:.3f}, without al.wh {r[1]:.1f}, without ah.wl {r[2]:.1f}")
    assert r[0] <= 1.0 and r[1] > 1.0 and r[2] > 1.0, r


@pytest.mark.parametrize("case", CASES[1::2], ids=lambda c: "x".join(map(str, c)))
def test_bound_discriminates_at_large_activations(case):
    r = _ratios(*_inputs(case, seed=5, act=300.0))
    print(f"[{case} act=300] err/bound: engine {r[0]:.3f}, without al.wh {r[1]:.1f}, without ah.wl {r[2]:.1f}")
    assert r[0] <= 1.0 and r[1] > 1.0 and r[2] > 1.0, r


def test_bound_holds_at_small_activations():
    """|a| ~ 1e-3: the engine stays under the bound; the mutants are NOT asserted here (module docstring: the f16 subnormal floor of the lo halves -
    the reason for pow2_scale in front of every cotangent GEMM)."""
    r = _ratios(*_inputs(CASES[1], seed=6, act=1e-3))
    print(f"[act=1e-3] err/bound: engine {r[0]:.3f} (mutants {r[1]:.2f}, {r[2]:.2f}: not asserted)")
    assert r[0] <= 1.0, r


def test_emulation_of_exactly_representable_operands_is_exact():
    """Small integers are their own hi halves (lo = 0) and every partial sum is an integer below 2^24: the emulation must return the float64 result
    exactly, with the stride, the padding zeros and the tap order of the reference."""
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-8, 9, (2, 5, 4, 32), generator=g).float()
    w = torch.randint(-4, 5, (16, 32, 3, 2), generator=g).float()
    for stride, pad in ((1, 0), (2, 1), (1, 2)):
        ref, _ = CR.conv_ref64(x, w, None, None, stride, pad, 0)
        assert torch.equal(CR.emulate(x, w, None, None, stride, pad, 0, 4.0).double(), ref), (stride, pad)


# ------------------------------------------------------------------------------------------------ host helpers
def test_weight_scale_edges():
    from egohmr_amd.split_gemm import weight_scale
    for amax in (0.0, float("inf"), float("nan"), -1.0):
        assert weight_scale(amax) == 1.0, amax
    assert weight_scale(1.0) == 2048.0 and weight_scale(0.25) == 8192.0        # an exact power of two lands ON 2048
    assert weight_scale(2048.0) == 1.0
    assert weight_scale(math.nextafter(2048.0, math.inf)) == 0.5               # just above: the next power down
    assert weight_scale(math.nextafter(2048.0, 0.0)) == 1.0
    assert weight_scale(3e38) == 2.0 ** -117
    for amax in (1e-3, 0.7, 1.0, 3.0, 2047.9, 2048.0, 2048.1, 1e30, 3e38, 1e-30, 2.0 ** -114):
        s = weight_scale(amax)
        assert math.frexp(s)[0] == 0.5 and 1024.0 < amax * s <= 2048.0, (amax, s)
    # below 2^-115 the scale stops at 2^126: it and its reciprocal stay normal float32 numbers (the engine takes both as float32)
    for amax in (2.0 ** -116, 1e-38, 1e-45, 5e-324):                            # float32 subnormals, and the smallest double
        s = weight_scale(amax)
        assert s == 2.0 ** 126 and amax * s <= 2048.0, (amax, s)
        assert np.isfinite(np.float32(s)) and float(np.float32(1.0) / np.float32(s)) == 2.0 ** -126


def test_pad_cols():
    from egohmr_amd.split_gemm import pad_cols, round_up
    x = torch.arange(15.0).view(3, 5) + 1
    p = pad_cols(x, 32)
    assert p.shape == (3, 32) and p.dtype == torch.float32 and torch.equal(p[:, :5], x) and bool((p[:, 5:] == 0).all())
    assert torch.equal(pad_cols(x, 5), x) and pad_cols(x, 5).data_ptr() != x.data_ptr()
    assert [round_up(n, 8) for n in (1, 6, 8, 9)] == [8, 8, 8, 16] and round_up(129, 128) == 256


@pytest.mark.parametrize("target", [1024.0, 256.0])
def test_pow2_scale_on_cpu_tensors(target):
    """0-d result; 1 for an all-zero or a non-finite tensor; otherwise a power of two s with target/2 < s max|t| <= target.  (The exponent comes from
    a float32 log2: a maximum within an ulp or two ABOVE a power of two may round onto it and land an ulp over the target - harmless at a target of
    2^10 against the f16 range, and not asserted here.)"""
    from egohmr_amd.split_gemm import pow2_scale
    one = lambda t: float(pow2_scale(t, target))
    assert pow2_scale(torch.zeros(4, 3), target).shape == ()
    assert one(torch.zeros(4, 3)) == 1.0
    for bad in (float("inf"), float("-inf"), float("nan")):
        t = torch.ones(5)
        t[2] = bad
        assert one(t) == 1.0, bad
    g = torch.Generator().manual_seed(0)
    cases = [torch.tensor([-3.0, 1.0]), torch.tensor([1.0, -1e-3]), torch.tensor([-5e-7]), torch.tensor([0.0, 1e-30]), torch.tensor([3e38, -1.0])]
    cases += [torch.randn(7, 9, generator=g) * a for a in (1e-6, 1e-3, 1.0, 37.0, 1e5)]
    cases += [torch.tensor([p, -p / 2]) for p in (2.0 ** -20, 0.5, 1.0, 4.0, 1024.0, 2.0 ** 20)]           # exact powers of two
    cases += [-c for c in cases]                                                                          # negative-dominant twins
    for t in cases:
        s, a = one(t), float(t.abs().max())
        assert math.frexp(s)[0] == 0.5, (t, s)
        assert target / 2 < s * a <= target, (a, s)
    for p in (2.0 ** -20, 1.0, 4.0, 2.0 ** 20):
        assert one(torch.tensor([p])) * p == target                                                       # a power of two lands ON the target


# ------------------------------------------------------------------------------------------------ refusals
def _dummy_conv_desc(**kw):
    """An ehm_conv_desc that every check of ehm_conv_nhwc_split accepts, on dummy (never dereferenced) addresses.  Each use breaks one rule, so no
    call reaches a launch."""
    from egohmr_amd import _lib
    f = dict(x=0x10000, W=0x20000, bias=None, residual=None, y=0x30000, N=2, H=8, Wd=8, Ci=64, Co=64, KH=3, KW=3, stride=1, pad=1, relu=0, w_scale=1.0)
    f.update(kw)
    return _lib.ConvDesc(**f)


def test_conv_nhwc_split_rejects_bad_arguments_without_a_gpu():
    from egohmr_amd import _lib
    L = _lib.lib()
    assert L.ehm_conv_nhwc_split(None, None) == -22
    assert b"bad argument" in L.ehm_last_error()
    for bad in (dict(x=None), dict(W=None), dict(y=None),
                dict(Ci=48), dict(Ci=16), dict(Ci=0),                     # Ci % 32
                dict(Co=60), dict(Co=6), dict(Co=0),                      # Co % 8
                dict(stride=0), dict(stride=3), dict(stride=-1),
                dict(KH=6, KW=6, pad=3), dict(KH=33, KW=1, H=40),         # KH KW > 32
                dict(KH=0), dict(KW=0),
                dict(pad=-1),
                dict(w_scale=0.0), dict(w_scale=-1.0), dict(w_scale=float("nan")),
                dict(N=0), dict(H=0), dict(Wd=0),
                dict(H=2, pad=0), dict(Wd=2, pad=0),                      # a kernel larger than the padded image: Ho, Wo <= 0
                dict(KH=5, KW=5, H=1, Wd=1, pad=1), dict(KH=7, KW=1, H=1, pad=2, stride=2),
                dict(H=2, pad=0, stride=2), dict(Wd=2, pad=0, stride=2)):  # ... by one at stride 2: -1 / 2 is 0 in C, Ho must not come out as 1
        assert L.ehm_conv_nhwc_split(C.byref(_dummy_conv_desc(**bad)), None) == -22, bad
        assert b"bad argument" in L.ehm_last_error(), bad
