"""CPU: the error bound of tests/conv_x2_ref.py tells the X2 conv engine (ehm_conv_x2) from an engine that drops one of its two correction
products, and its hi-only tier from one that reads lo halves; the host restatement of the ehm_split_pack layout round-trips; selector weights through
the emulated engine are bit-exact; and the refusals ehm_conv_x2 decides before any device call.  The GPU side is tests/test_gpu_conv_x2.py.

Every discriminating case uses activations of order 1 or above (conv_split_ref's docstring: at 1e-3 the lo halves are f16 subnormals and a correction
product is as small as the format's floor).  Ratios seen (error / bound; docs/EXPERIMENTS.md, round 32, has the table): the emulated engine 0.09 -
0.17, without xl.wh 101 - 667, without xh.wl 90 - 599; the hi-only emulation 0.97 - 0.99 of its bound (the half ulp of one f16: sharp by construction),
the split emulation against the hi-only reference 131 - 671 times over it."""
import ctypes as C
import itertools
import math

import pytest
import torch

from tests import conv_x2_ref as XR

MUTANTS = ("xlwh", "xhwl")
# (N, H, W, Ci, Co, (KH, KW, stride, pad), Ci2, stride2): K-tile counts 2 (the minimum), 3, 18, 72; the last two have the second K segment (3 and 4 K tiles)
CASES = [(2, 7, 9, 64, 64, (1, 1, 1, 0), 0, 1), (3, 5, 5, 96, 32, (1, 1, 2, 0), 0, 1), (2, 8, 8, 64, 96, (3, 3, 2, 1), 0, 1),
         (128, 1, 1, 2304, 64, (1, 1, 1, 0), 0, 1), (2, 4, 5, 64, 128, (1, 1, 1, 0), 32, 2), (2, 4, 5, 64, 128, (1, 1, 1, 0), 64, 1)]
_id = lambda c: "x".join(map(str, c[:5])) + "-k%dx%ds%dp%d" % c[5] + ("-seg%ds%d" % c[6:] if c[6] else "")


def _inputs(case, seed, act=1.0, epilogue=False):
    """standard-normal activations (times act), He-scaled weights, the scale weight_scale gives them; with epilogue: bias, residual and ReLU"""
    from egohmr_amd.split_gemm import weight_scale
    N, H, W, Ci, Co, geom, Ci2, stride2 = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Ci, generator=g) * act
    K = geom[0] * geom[1] * Ci + Ci2
    w = torch.randn(Co, Ci, geom[0], geom[1], generator=g) * math.sqrt(2.0 / K)
    Ho, Wo = XR.out_hw(H, W, *geom)
    x2 = w2 = None
    if Ci2:
        x2 = torch.randn(N, (Ho - 1) * stride2 + 1, (Wo - 1) * stride2 + 1, Ci2, generator=g) * act
        w2 = torch.randn(Co, Ci2, generator=g) * math.sqrt(2.0 / K)
    s = weight_scale(max(float(w.abs().max()), float(w2.abs().max()) if Ci2 else 0.0))
    bias = torch.randn(Co, generator=g) * act if epilogue else None
    res = torch.randn(N * Ho * Wo, Co, generator=g) * act if epilogue else None
    return XR.Operands(x, w, s, geom, x2, w2, stride2), bias, res, int(epilogue)


def _ratios(ops, bias, res, relu, **kw):
    """error / bound of the emulated engine and of its two mutants"""
    ref, pre = XR.conv_ref64(ops, bias, res, relu)
    bound = XR.tol(ops, res, pre, stream_k="cuts" in kw)
    return [XR.ratio(XR.decoded(*XR.emulate(ops, bias, res, relu, drop=d, **kw)), ref, bound) for d in (None,) + MUTANTS]


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bound_tells_the_engine_from_one_without_a_correction_product(case, epilogue):
    r = _ratios(*_inputs(case, seed=sum(case[:5]), epilogue=epilogue))
    print(f"[{_id(case)} epilogue={epilogue}] err/bound: engine {r[0]:.3f}, without xl.wh {r[1]:.1f}, without xh.wl {r[2]:.1f}")
    assert r[0] <= 1.0 and r[1] > 1.0 and r[2] > 1.0, r


@pytest.mark.parametrize("case", CASES[2:5:2], ids=_id)
def test_bound_discriminates_at_large_activations(case):
    r = _ratios(*_inputs(case, seed=5, act=300.0))
    print(f"[{_id(case)} act=300] err/bound: engine {r[0]:.3f}, without xl.wh {r[1]:.1f}, without xh.wl {r[2]:.1f}")
    assert r[0] <= 1.0 and r[1] > 1.0 and r[2] > 1.0, r


def test_bound_holds_at_small_activations():
    """|a| ~ 1e-3: the engine stays under the bound; the mutants are NOT asserted (module docstring)."""
    r = _ratios(*_inputs(CASES[2], seed=6, act=1e-3))
    print(f"[act=1e-3] err/bound: engine {r[0]:.3f} (mutants {r[1]:.2f}, {r[2]:.2f}: not asserted)")
    assert r[0] <= 1.0, r


@pytest.mark.parametrize("cuts", [(24,), (24, 48), (2, 70)])
def test_stream_k_partial_sums_stay_under_the_bound(cuts):
    """the K loop of 72 K tiles cut into two or three runs whose sums are added in k order: under the stream-K bound, the mutants over it"""
    r = _ratios(*_inputs(CASES[3], seed=7, epilogue=True), cuts=cuts)
    print(f"[stream-K cuts {cuts}] err/bound: engine {r[0]:.3f}, without xl.wh {r[1]:.1f}, without xh.wl {r[2]:.1f}")
    assert r[0] <= 1.0 and r[1] > 1.0 and r[2] > 1.0, r


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("case", CASES[::2] + CASES[3:4], ids=_id)
def test_hi_only_bound_sees_lo_halves_read_by_mistake(case, epilogue):
    """The hi-only emulation stays under the hi-only bound; the split emulation - an engine that reads the lo halves it must not - does not stay under
    it against the same (hi halves only) reference."""
    ops, bias, res, relu = _inputs(case, seed=11 + sum(case[:5]), epilogue=epilogue)
    ref, pre = XR.conv_ref64(ops, bias, res, relu, hi_only=True)
    bound = XR.tol(ops, res, pre, hi_only=True)
    r_hi = XR.ratio(XR.decoded(*XR.emulate(ops, bias, res, relu, hi_only=True)), ref, bound)
    r_split = XR.ratio(XR.decoded(*XR.emulate(ops, bias, res, relu)), ref, bound)
    print(f"[{_id(case)} epilogue={epilogue}] hi-only err/bound: hi-only engine {r_hi:.3f}, split engine {r_split:.1f}")
    assert r_hi <= 1.0 and r_split > 1.0, (r_hi, r_split)


def test_emulation_of_exactly_representable_operands_is_exact():
    """Small integers are their own hi halves and every partial sum is an integer below 2^11: both tiers return the float64 result exactly, with the
    stride, the padding zeros, the tap order and the second segment of the reference."""
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-4, 5, (2, 5, 4, 32), generator=g).float()
    w = torch.randint(-2, 3, (32, 32, 3, 2), generator=g).float()
    for stride, pad in ((1, 0), (2, 1), (1, 2)):
        Ho, Wo = XR.out_hw(5, 4, 3, 2, stride, pad)
        x2 = torch.randint(-4, 5, (2, 2 * Ho - 1, 2 * Wo - 1, 32), generator=g).float()
        w2 = torch.randint(-2, 3, (32, 32), generator=g).float()
        ops = XR.Operands(x, w, 4.0, (3, 2, stride, pad), x2, w2, 2)
        ref, _ = XR.conv_ref64(ops, None, None, 0)
        assert float(ref.abs().max()) < 2048
        for hi_only in (False, True):
            assert torch.equal(XR.decoded(*XR.emulate(ops, None, None, 0, hi_only=hi_only)), ref), (stride, pad, hi_only)


# ------------------------------------------------------------------------------------------------ the layout helpers
def test_split_and_pack_round_trip():
    g = torch.Generator().manual_seed(1)
    v = torch.randn(7, 96, generator=g) * torch.tensor([1e-6, 1e-3, 1.0, 37.0, 3e3, 6e4, 1.0])[:, None]
    v[6, :8] = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 65519.9, 131008.0, 2e5, -float("inf")])
    hi, lo = XR.split_x2(v)
    assert hi.dtype == lo.dtype == torch.float16 and bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all())      # saturates, never inf
    dec = hi.double() + lo.double()
    inside = v.abs() <= 65504
    assert bool(((dec - v.double()).abs() <= 2.0 ** -22 * v.double().abs() + 2.0 ** -25)[inside].all())
    assert dec[6, 5:8].tolist() == [131008.0, 131008.0, -131008.0]
    buf = XR.pack_x2(v)
    assert buf.shape == (7, 192)
    assert torch.equal(buf[:, 0:32], hi[:, 0:32]) and torch.equal(buf[:, 32:64], lo[:, 0:32]) and torch.equal(buf[:, 128:160], hi[:, 64:96])
    h2, l2 = XR.unpack_halves(buf)
    assert torch.equal(h2.view(torch.int16), hi.view(torch.int16)) and torch.equal(l2.view(torch.int16), lo.view(torch.int16))
    assert torch.equal(XR.unpack_x2(buf), dec)
    # splitting the decoded value again returns the same halves, except at a tie (selector_expected's docstring)
    h3, l3 = XR.split_x2(dec[:6].float())
    same = (h3 == hi[:6]) & (l3 == lo[:6])
    tie = (h3.double() == hi[:6].double() + 2 * lo[:6].double()) & (l3 == -lo[:6])                # lo = half an ulp of an odd hi: the even neighbour takes it
    assert bool((same | tie).all()) and int(same.sum()) > 500 and torch.equal(h3.double() + l3.double(), dec[:6])


def test_x2_buffer_and_weight_operand_layout():
    v = torch.arange(5 * 32, dtype=torch.float32).view(5, 32)
    buf = XR.x2_buffer(v, rows=XR.x2_rows(5) + 3)
    assert buf.shape == (196, 64) and XR.x2_rows(5) == 193 and XR.x2_rows(192) == 193 and XR.x2_rows(193) == 385
    assert torch.equal(XR.unpack_x2(buf[:5]), v.double())
    assert bool((buf[5:195].view(torch.int16) == XR.NAN_HALF).all()) and bool(torch.isnan(buf[5:195]).all()) and bool((buf[195] == 0).all())
    w = torch.randn(40, 32, 2, 3, generator=torch.Generator().manual_seed(2))
    w2 = torch.randn(40, 64, generator=torch.Generator().manual_seed(3))
    op = XR.weight_operand(w, 8.0, w2)
    assert op.shape == (128, 2 * 3 * 32 + 64) and bool((op[40:] == 0).all())
    assert torch.equal(op[:40, :192].view(40, 2, 3, 32), w.permute(0, 2, 3, 1) * 8.0) and torch.equal(op[:40, 192:], w2 * 8.0)      # tap-major, [W | W2]
    dec = XR.unpack_x2(XR.pack_weight(w, 8.0, w2))
    assert dec.shape == op.shape and bool(((dec - op.double()).abs() <= 2.0 ** -22 * op.double().abs() + 2.0 ** -25).all())


@pytest.mark.parametrize("geom,image", [((3, 3, 1, 1), (2, 4, 5)), ((3, 3, 2, 1), (2, 5, 4)), ((1, 1, 2, 0), (3, 5, 5))], ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("Co", [32, 64, 128])
def test_selector_weights_through_the_emulated_engine_are_bit_exact(geom, image, Co):
    """every tap: y's halves are the re-split of the gathered pixel (hi-only: its hi half), zeros at out-of-image taps"""
    g = torch.Generator().manual_seed(Co + geom[2])
    x = torch.randn(*image, 32, generator=g) * 3.0
    x.view(-1)[::7] *= 1e-4                                                     # some lo halves in the subnormal range
    for tap in range(geom[0] * geom[1]):
        w = XR.selector_weights(geom[0], geom[1], 32, Co, tap)
        ops = XR.Operands(x.repeat(1, 1, 1, 2), torch.cat([w, torch.zeros_like(w)], 1), 2048.0, geom)        # (Ci = 64: two K tiles for a 1 x 1)
        hi, lo = XR.emulate(ops, None, None, 0)
        eh, el = XR.selector_expected(x, geom, Co, tap)
        assert torch.equal(hi.view(torch.int16), eh.view(torch.int16)) and torch.equal(lo.view(torch.int16), el.view(torch.int16)), tap
        hi1, _ = XR.emulate(ops, None, None, 0, hi_only=True)
        assert torch.equal(hi1.view(torch.int16), XR.selector_expected_hi_only(x, geom, Co, tap).view(torch.int16)), tap
    if geom[3]:                                                                  # the first tap of the first output pixel lies outside the image
        e0, _ = XR.selector_expected(x, geom, Co, 0)
        assert bool((e0[0] == 0).all()) and not bool((e0 == 0).all())


# ------------------------------------------------------------------------------------------------ the case lists of the GPU file
def test_descriptor_matrix_is_a_pairwise_cover():
    """Every pair of levels of two factors occurs in some row of tests/test_gpu_conv_x2.py's MATRIX - except a 1 x 1 kernel on 32 channels (one K tile:
    refused), which no row has."""
    from tests import test_gpu_conv_x2 as T
    assert len(T.MATRIX) == 63 and all(T._legal(r[4], r[5]) for r in T.MATRIX) and len(set(T.MATRIX)) == 63
    assert {g[0] * g[1] * (Ci // 32) for _, _, _, _, g, Ci, _, _ in T.MATRIX} >= {2, 3, 9, 27, 18, 32}
    for a, b in itertools.combinations(range(8), 2):
        want = set(itertools.product(T.LEVELS[a], T.LEVELS[b]))
        if (a, b) == (4, 5):
            want = {(g, Ci) for g, Ci in want if T._legal(g, Ci)}
            assert len(want) == 24
        assert {(r[a], r[b]) for r in T.MATRIX} == want, (a, b)


def test_tile_loop_cases_take_both_block_orders():
    """the condition of x2_xcd_order (csrc/x2_tile_dev.h) for the tile-loop cases of tests/test_gpu_conv_x2.py on a 256-CU device: both answers occur"""
    from tests import test_gpu_conv_x2 as T
    slots, seen = 512, set()
    for target, n_tiles, _ in T._tile_loop_cases():
        G = min(-(-(target[0] * slots + target[1]) // n_tiles) * n_tiles, slots)
        seen.add((n_tiles, G % 8 == 0 and (G // 8) % n_tiles == 0))
    assert seen == {(1, True), (1, False), (2, True), (3, False)}


# ------------------------------------------------------------------------------------------------ refusals
def _dummy_x2_desc(**kw):
    """An ehm_conv_x2_desc that every check of ehm_conv_x2 accepts, on dummy (never dereferenced) addresses.  Each use breaks one rule that is
    decided before any device call, so no call reaches a launch."""
    from egohmr_amd import _lib
    f = dict(x=0x10000, x_rows=193, W=0x20000, bias=None, residual=None, y=0x30000, N=2, H=8, Wd=8, Ci=64, Co=128, KH=1, KW=1, stride=1, pad=0, relu=0,
             w_scale=1.0)
    f.update(kw)
    return _lib.ConvX2Desc(**f)


def test_conv_x2_rejects_bad_arguments_without_a_gpu():
    from egohmr_amd import _lib
    L = _lib.lib()
    assert L.ehm_conv_x2(None, None) == -22
    seg = dict(x2=0x40000, x2_rows=193, H2=8, W2=8, Ci2=32, stride2=1)
    for bad in (dict(x=None), dict(W=None), dict(y=None),
                dict(Co=48), dict(Co=16), dict(Co=0),                        # Co % 32
                dict(Ci=48), dict(Ci=16), dict(Ci=0),                        # Ci % 32
                dict(Ci=32),                                                 # one K tile: the K loop needs two
                dict(x_rows=192), dict(x_rows=128),                          # no zero row
                dict(KH=6, KW=6, pad=3), dict(stride=3), dict(pad=-1), dict(w_scale=0.0),
                dict(H=2, KH=3, KW=3),                                       # a kernel larger than the padded image
                dict(seg, H2=10), dict(seg, W2=7), dict(seg, stride2=2),     # a shortcut grid that does not map onto the output grid
                dict(seg, Co=64), dict(seg, Co=192),                         # Co % 128 with a second segment
                dict(seg, Ci2=48), dict(seg, x2_rows=192), dict(seg, stride2=3)):
        assert L.ehm_conv_x2(C.byref(_dummy_x2_desc(**bad)), None) == -22, bad
        assert L.ehm_last_error(), bad
    assert XR.x2_rows(2 * 8 * 8) == 193 == L.ehm_conv_x2_rows(128) and L.ehm_conv_x2_rows(193) == XR.x2_rows(193)
