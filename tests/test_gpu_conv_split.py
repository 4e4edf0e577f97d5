"""GPU (MI355X): the float32-activation conv engine (ehm_conv_nhwc_split, csrc/conv.hip: conv_nhwc_split_kernel) called through _lib.ConvDesc,
every output element against float64 (tests/conv_split_ref.py: conv_ref64) under the derived bound of that module (tol; its docstring has the error
model, tests/test_conv_split_cpu.py shows that the bound tells the engine from one that drops a correction product).

In every case the output sits between canary guards, the activations sit in a buffer whose surrounding floats are NaN (an out-of-image tap or a row
past M read as data would show in the output, the padding rows of the weight operand being zero), and the largest error / bound ratio is printed.

Measured on an MI355X, the engine stays under an eighth of its bound: descriptor matrix <= 0.113 (0.005 - 0.060 wherever a row gathers at least one
in-image tap; 0.089 - 0.113 in the three cases that have output pixels with NO tap inside the image - 1 x 3 and 7 x 1 kernels padded on both axes -
where the bound is its epilogue term alone), tile schedule <= 0.054, gemm_rows <= 0.033, activations up to 65504 0.040, beyond 2 GiB 0.041.  The same
library with the al.wh product taken out of the kernel failed 61 of the 65 tests this file then had, the float64 comparisons by 4.2 to 74 times their bound - the
figures tests/conv_split_ref.py: emulate predicts for each case to three digits (docs/EXPERIMENTS.md, round 23)."""
import ctypes as C
import itertools
import math

import pytest
import torch

from tests import conv_split_ref as CR
from tests.test_gpu_trunk_autograd import CANARY, guarded, guards_intact

pytestmark = pytest.mark.gpu

NAN = float("nan")
CBM = CBN = 128                      # output tile of conv_nhwc_split_kernel


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def nan_framed(x, dev, frame):
    """x on the device inside a buffer with `frame` NaN floats in front of and behind it (frame % 4 == 0: the engine's 16-byte loads stay aligned)"""
    assert frame % 4 == 0
    n = x.numel()
    full = torch.full((n + 2 * frame,), NAN, device=dev)
    v = full[frame:frame + n].view(x.shape)
    v.copy_(x)
    return full, v


def pack(w, dev):
    """w [Co, Ci, KH, KW] -> (the engine's weight operand: tap-major rows, Co padded to 128 with zero rows, times s, ehm_split_pack; s = weight_scale)"""
    from egohmr_amd import _lib
    from egohmr_amd.split_gemm import round_up, weight_scale
    rows = CR.weight_rows(w)
    Co, K = rows.shape
    w2 = torch.zeros(round_up(Co, CBN), K, device=dev)
    w2[:Co] = rows.to(dev)
    s = weight_scale(float(w.abs().max()))
    buf = torch.empty_like(w2)
    _lib.api().ehm_split_pack(w2, buf, w2.shape[0], K, K, s, _lib.stream_ptr())
    return buf, s


class Conv:
    """One ehm_conv_nhwc_split launch: seeded float32 inputs (standard-normal activations, bias and residual, He-scaled weights), their device
    forms, and the float64 reference with its bound (computed once, on the CPU)."""

    def __init__(self, dev, image, Ci, Co, geom, bias=True, res=True, relu=1, seed=0):
        self.dev, self.geom, self.relu = dev, geom, relu
        (N, H, W), (KH, KW, stride, pad) = image, geom
        self.shape = (N, H, W, Ci, Co)
        self.Ho, self.Wo = CR.out_hw(H, W, KH, KW, stride, pad)
        assert self.Ho > 0 and self.Wo > 0
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn(N, H, W, Ci, generator=g)
        self.w = torch.randn(Co, Ci, KH, KW, generator=g) * math.sqrt(2.0 / (Ci * KH * KW))
        self.bias = torch.randn(Co, generator=g) if bias else None
        self.res = torch.randn(N, self.Ho, self.Wo, Co, generator=g) if res else None
        self._ref = None

    def upload(self):
        (N, H, W, Ci, Co), (KH, KW, stride, pad) = self.shape, self.geom
        self.xfull, self.xd = nan_framed(self.x, self.dev, 64 + 4 * ((pad * (W + 1) + KW) * Ci))     # the frame covers every out-of-image tap's address
        self.wbuf, self.s = pack(self.w, self.dev)
        self.bd = None if self.bias is None else self.bias.to(self.dev)
        self.rd = None if self.res is None else self.res.to(self.dev).contiguous()
        return self

    def run(self):
        """launch once -> (guarded buffer, its y view [N, Ho, Wo, Co])"""
        from egohmr_amd import _lib
        (N, H, W, Ci, Co), (KH, KW, stride, pad) = self.shape, self.geom
        full, y = guarded(self.dev, N, self.Ho, self.Wo, Co)
        P = _lib.ptr
        d = _lib.ConvDesc(P(self.xd), P(self.wbuf), P(self.bd), P(self.rd), P(y), N, H, W, Ci, Co, KH, KW, stride, pad, self.relu, self.s)
        _lib.api().ehm_conv_nhwc_split(C.byref(d), _lib.stream_ptr())
        torch.cuda.synchronize()
        return full, y

    def reference(self):
        if self._ref is None:
            _, _, stride, pad = self.geom
            ref, pre = CR.conv_ref64(self.x, self.w, self.bias, self.res, stride, pad, self.relu)
            self._ref = ref, CR.tol(self.x, self.w, self.res, pre, stride, pad, self.s)
        return self._ref

    def check(self, full, y, tag):
        """every output element against float64; returns the largest error / bound ratio"""
        assert guards_intact(full), f"{tag}: wrote outside y"
        got = y.cpu()
        ref, bound = self.reference()
        assert got.shape == ref.shape and bool(torch.isfinite(got).all()), tag
        r = CR.ratio(got, ref, bound)
        print(f"[{tag}] max err/bound = {r:.3f}")
        assert r <= 1.0, f"{tag}: off by {r:.2f} x the bound (max|err| = {float((got.double() - ref).abs().max()):.3e})"
        return r


# --------------------------------------------------------------------------------------------- descriptor matrix
BIASES, RESIDUALS, RELUS = (False, True), (False, True), (0, 1)
# (KH, KW, stride, pad); (3, 3, 1, 2) is the full correlation the data gradient uses, (5, 5, 1, 2) has 25 taps
GEOMS = ((1, 1, 1, 0), (1, 1, 2, 0), (3, 3, 1, 1), (3, 3, 2, 1), (3, 3, 1, 0), (3, 3, 1, 2), (1, 3, 1, 1), (5, 5, 1, 2), (7, 1, 2, 3))
CIS = (32, 64, 96)                   # 32: one K tile per tap
COS = (8, 64, 128, 136, 264)         # 136, 264: the last n-tile holds 8 valid columns
IMAGES = ((1, 1, 1), (3, 5, 3), (2, 7, 7), (2, 8, 8))
LEVELS = (BIASES, RESIDUALS, RELUS, GEOMS, CIS, COS, IMAGES)
# row = geometry, column = Co, entry = the indices of (bias, residual, relu, Ci, image): a pairwise cover found by search, verified below
_TABLE = ("10011 11112 10003 11020 00103", "00011 01023 10102 11110 11102", "10111 11022 11103 11021 00010",
          "11101 01003 10021 00112 01010", "01022 01123 10112 00101 00123", "10113 01011 00120 00011 01002",
          "10003 11112 01111 01002 01020", "11110 00002 11021 01003 11121", "00102 11100 11001 00013 00121")
MATRIX = [(BIASES[int(e[0])], RESIDUALS[int(e[1])], RELUS[int(e[2])], GEOMS[i], CIS[int(e[3])], COS[j], IMAGES[int(e[4])])
          for i, row in enumerate(_TABLE) for j, e in enumerate(row.split())]


def _fits(geom, image):
    KH, KW, stride, pad = geom
    return min(CR.out_hw(image[1], image[2], KH, KW, stride, pad)) > 0


def _matrix_id(r):
    b, rs, relu, g, Ci, Co, im = r
    return f"k{g[0]}x{g[1]}s{g[2]}p{g[3]}-{'x'.join(map(str, im))}-Ci{Ci}-Co{Co}-{'bias' if b else 'nobias'}-{'res' if rs else 'nores'}-relu{relu}"


def test_descriptor_matrix_is_a_pairwise_cover():
    """Every pair of levels of two factors occurs in some row - except a geometry on an image it does not fit (3 x 3 unpadded on 1 x 1), which no row has."""
    assert len(MATRIX) == 45 and all(_fits(r[3], r[6]) for r in MATRIX)
    for a, b in itertools.combinations(range(7), 2):
        want = set(itertools.product(LEVELS[a], LEVELS[b]))
        if (a, b) == (3, 6):
            want = {(g, im) for g, im in want if _fits(g, im)}
            assert len(want) == 35
        assert {(r[a], r[b]) for r in MATRIX} == want, (a, b)


@pytest.mark.parametrize("row", MATRIX, ids=_matrix_id)
def test_conv_split_descriptor_matrix_vs_fp64(dev, row):
    bias, res, relu, geom, Ci, Co, image = row
    c = Conv(dev, image, Ci, Co, geom, bias, res, relu, seed=MATRIX.index(row)).upload()
    c.check(*c.run(), tag=f"matrix {_matrix_id(row)}")


# --------------------------------------------------------------------------------------------- tile schedule
# (M, Co, tiles, remapped): the kernel takes the XCD remap when its tile count is a multiple of 8
SCHEDULE = [(1024, 128, 8, True), (512, 256, 8, True), (1024, 384, 24, True), (1025, 128, 9, False), (1, 128, 1, False), (127, 8, 1, False),
            (129, 136, 4, False)]


@pytest.mark.parametrize("M,Co,tiles,remap", SCHEDULE)
def test_conv_split_tile_schedule_vs_fp64(dev, M, Co, tiles, remap):
    """H = W = 1, Ci = 64, with bias, residual and ReLU: one, two and three column tiles under the XCD remap (a block's tile is no longer its index),
    a tile count that is no multiple of 8, a single row, a ragged single tile, and ragged last tiles both ways."""
    assert -(-M // CBM) * -(-Co // CBN) == tiles and (tiles % 8 == 0) == remap
    c = Conv(dev, (M, 1, 1), 64, Co, (1, 1, 1, 0), seed=M + Co).upload()
    c.check(*c.run(), tag=f"schedule M={M} Co={Co} tiles={tiles} remap={remap}")


# --------------------------------------------------------------------------------------------- split_gemm.gemm_rows
@pytest.mark.parametrize("with_res", [False, True])
def test_gemm_rows_with_six_true_columns(dev, with_res):
    """rows < x.shape[0] (the rows of x behind them are NaN), out= given, a Packed of Co = 6 with a bias: cols = 8 and pack_weight pads the bias to
    it.  Columns 0..5 against float64; columns 6 and 7 are exactly the residual (0 without one: gemm_rows sets no ReLU); rows of `out` behind `rows`
    keep their bits."""
    from egohmr_amd.split_gemm import gemm_rows, pack_weight
    M0, rows, Ci, Co = 300, 270, 64, 6
    g = torch.Generator().manual_seed(11 + with_res)
    x = torch.randn(M0, Ci, generator=g)
    w2 = torch.randn(Co, Ci, generator=g) * math.sqrt(2.0 / Ci)
    bias = torch.randn(Co, generator=g)
    res = torch.randn(rows, 8, generator=g) if with_res else None
    xd = x.to(dev)
    xd[rows:] = NAN
    packed = pack_weight(w2.to(dev), bias.to(dev))
    assert packed.cols == 8 and packed.bias.shape == (8,) and torch.equal(packed.bias.cpu(), torch.cat([bias, torch.zeros(2)]))
    full, out = guarded(dev, M0, 8)
    y = gemm_rows(xd, packed, rows=rows, res=None if res is None else res.to(dev), out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr() and guards_intact(full)
    got = out.cpu()
    assert bool((got[rows:] == CANARY).all()), "rows behind `rows` were written"
    assert torch.equal(got[:rows, 6:], res[:, 6:] if with_res else torch.zeros(rows, 2))
    r6 = None if res is None else res[:, :6].reshape(rows, 1, 1, 6)
    ref, pre = CR.conv_ref64(x[:rows].view(rows, 1, 1, Ci), w2.view(Co, Ci, 1, 1), bias, r6, 1, 0, 0)
    bound = CR.tol(x[:rows].view(rows, 1, 1, Ci), w2.view(Co, Ci, 1, 1), r6, pre, 1, 0, packed.scale)
    assert bool(torch.isfinite(got[:rows]).all())
    r = CR.ratio(got[:rows, :6].reshape(rows, 1, 1, 6), ref, bound)
    print(f"[gemm_rows Co=6 res={with_res}] max err/bound = {r:.3f}")
    assert r <= 1.0, r


# --------------------------------------------------------------------------------------------- range and non-finite behaviour
def test_conv_split_activations_up_to_the_f16_limit(dev):
    """|x| up to 65504 (the clamp in front of the hi half is the identity there): within the bound, nothing non-finite."""
    c = Conv(dev, (2, 7, 7), 64, 72, (3, 3, 1, 1), seed=21)
    for (n, h, w_, ch), v in {(0, 0, 0, 0): 65504.0, (1, 6, 6, 63): -65504.0, (0, 3, 3, 17): 6e4, (1, 2, 5, 40): -33333.3, (0, 6, 0, 5): 65503.99}.items():
        c.x[n, h, w_, ch] = v
    c.upload()
    c.check(*c.run(), tag="range |x| <= 65504")


POISON_AT = (1, 3, 4, 37)            # (n, h, w, channel) of the non-finite activation


@pytest.mark.parametrize("geom", [(1, 1, 1, 0), (3, 3, 2, 1), (3, 3, 1, 2)], ids=lambda g: "k%dx%ds%dp%d" % g)
@pytest.mark.parametrize("bad", [NAN, float("inf"), 2e5], ids=["nan", "inf", "2e5"])
def test_one_non_finite_activation_poisons_its_receptive_field_only(dev, bad, geom):
    """relu = 0: the outputs whose receptive field holds the pixel come out non-finite in every channel (the NaN / inf lands in the lo half; 0 . inf of a
    padding column included), as in the float64 reference; every other output keeps the bits of the clean run.  relu = 1: the epilogue's max(v, 0)
    returns 0 for a NaN or -inf - an in-field output is non-finite or exactly 0, the others again keep their bits (the callers carry a flag beside the
    data: tests/test_gpu_nonfinite.py).  A finite activation past the format's 131008 (2e5: hi = 65504, lo = f16(134496) = inf) does the same: the
    engine has no range flag."""
    for relu in (0, 1):
        c = Conv(dev, (2, 8, 8), 64, 72, geom, relu=relu, seed=31).upload()
        _, clean = c.run()
        clean = clean.cpu()
        x_bad = c.x.clone()
        x_bad[POISON_AT] = bad
        c.xd.copy_(x_bad)
        full, y = c.run()
        got = y.cpu()
        ind = torch.zeros_like(c.x)
        ind[POISON_AT] = 1.0
        field = CR.im2col(ind, geom[0], geom[1], geom[2], geom[3]).sum(1) > 0                    # the rows of the GEMM that gather the pixel
        assert 0 < int(field.sum()) < field.numel()
        hit = field.view(2, c.Ho, c.Wo, 1).expand(2, c.Ho, c.Wo, c.shape[4]).contiguous()
        if not math.isfinite(bad):                                                               # ... are the reference's non-finite outputs
            ref, _ = CR.conv_ref64(x_bad, c.w, c.bias, c.res, geom[2], geom[3], 0)
            assert torch.equal(~torch.isfinite(ref), hit)
        assert guards_intact(full)
        assert torch.equal(got[~hit].view(torch.int32), clean[~hit].view(torch.int32)), "an output outside the receptive field changed"
        if relu:
            assert bool((~torch.isfinite(got[hit]) | (got[hit] == 0)).all())
        else:
            assert torch.equal(~torch.isfinite(got), hit)


def test_all_zero_weight_gives_the_epilogue_alone(dev):
    """w = 0: exactly relu(bias + res) in float32, whatever the activations (weight_scale is 1 then)."""
    c = Conv(dev, (2, 7, 7), 32, 136, (3, 3, 2, 1), seed=41)
    c.w.zero_()
    c.upload()
    assert c.s == 1.0
    full, y = c.run()
    assert guards_intact(full)
    assert torch.equal(y.cpu().view(torch.int32), torch.relu(c.bias[None, None, None, :] + c.res).view(torch.int32))


def test_conv_split_is_deterministic(dev):
    """Two launches of one matrix case (3 x 3, stride 2, two column tiles): equal bits."""
    bias, res, relu, geom, Ci, Co, image = MATRIX[18]
    assert geom == (3, 3, 2, 1) and Co == 136
    c = Conv(dev, image, Ci, Co, geom, bias, res, relu, seed=18).upload()
    (_, y1), (_, y2) = c.run(), c.run()
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))


# --------------------------------------------------------------------------------------------- offsets beyond 2 GiB
def test_conv_split_offsets_beyond_2_gib(dev):
    """H = W = 1, M = 2^22 + 133 rows, Ci = 32, Co = 128: y and the residual are 2 GiB + 66.5 KiB each (row 2^22 starts at byte 2^31), x is 512 MiB.  The
    first 256 and the last 261 rows against float64; the rows around row 2^22 against a second launch on the last 4096 rows alone (another tile
    alignment, the same sums: equal bits)."""
    from egohmr_amd import _lib
    M, Ci, Co, tail = 2 ** 22 + 133, 32, 128, 4096
    assert M * Co * 4 > 2 ** 31 and (M - tail) * Co * 4 < 2 ** 31
    g = torch.Generator().manual_seed(51)
    w = torch.randn(Co, Ci, 1, 1, generator=g) * math.sqrt(2.0 / Ci)
    bias = torch.randn(Co, generator=g)
    try:
        gd = torch.Generator(device=dev).manual_seed(52)
        xfull = torch.full((M * Ci + 128,), NAN, device=dev)
        xd = xfull[64:64 + M * Ci].view(M, Ci)
        xd.normal_(generator=gd)
        rd = torch.randn(M, Co, generator=gd, device=dev)
        full, y = guarded(dev, M, Co)
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip(f"no room for the 2 GiB operands: {e}")
    wbuf, s = pack(w, dev)
    bd, P = bias.to(dev), _lib.ptr

    def launch(x_, r_, y_, rows):
        d = _lib.ConvDesc(P(x_), P(wbuf), P(bd), P(r_), P(y_), rows, 1, 1, Ci, Co, 1, 1, 1, 0, 1, s)
        _lib.api().ehm_conv_nhwc_split(C.byref(d), _lib.stream_ptr())
        torch.cuda.synchronize()

    launch(xd, rd, y, M)
    assert guards_intact(full)
    worst = 0.0
    for name, sl in (("first 256", slice(0, 256)), ("last 261", slice(M - 261, M))):
        xs, rs = xd[sl].cpu().view(-1, 1, 1, Ci), rd[sl].cpu().view(-1, 1, 1, Co)
        ref, pre = CR.conv_ref64(xs, w, bias, rs, 1, 0, 1)
        got = y[sl].cpu().view(-1, 1, 1, Co)
        assert bool(torch.isfinite(got).all()), name
        r = CR.ratio(got, ref, CR.tol(xs, w, rs, pre, 1, 0, s))
        assert r <= 1.0, (name, r)
        worst = max(worst, r)
    full2, y2 = guarded(dev, tail, Co)
    launch(xd[M - tail:], rd[M - tail:], y2, tail)
    assert guards_intact(full2)
    assert torch.equal(y[M - tail:].view(torch.int32), y2.view(torch.int32)), "rows around byte 2^31 differ from the launch on those rows alone"
    print(f"[beyond 2 GiB] max err/bound = {worst:.3f}")
    del xfull, xd, rd, full, y
    torch.cuda.empty_cache()
