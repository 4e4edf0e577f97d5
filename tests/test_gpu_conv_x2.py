"""GPU (MI355X): the X2 conv engine (ehm_conv_x2, csrc/conv.hip: conv_x2_tile_kernel) called through _lib.ConvX2Desc, every valid output element
against float64 of the operands the engine reads (tests/conv_x2_ref.py: conv_ref64) under the derived bound of that module (tol; its docstring has the
error model, tests/test_conv_x2_cpu.py shows that the bound tells the engine from one that drops a correction product or reads the wrong halves).

In every case y sits between canary guards and is pre-filled with a sentinel bit pattern (its zero row included), every padding row of x, x2 and the
residual - between the last pixel and the zero row - holds NaN halves, the X2 operands are packed on the host (conv_x2_ref.pack_x2, checked against
ehm_split_pack below), the float64 reference is computed once per case on the CPU, and the largest error / bound ratio is printed.  Large cases
repeat a base of PERIOD images (reference and bound are computed for the base, the comparison of every element runs on the device).

Measured on an MI355X (largest error / bound per group; docs/EXPERIMENTS.md, round 32): split tier - descriptor matrix 0.785 (an output with NO tap
inside the image, where the bound is the re-split of y alone; 0.16 - 0.45 elsewhere), rows 0.285, x_rows 0.257, tile loop 0.383, second K segment 0.406
(one launch against two: 0.121 of the summed bounds), stream-K 0.323 (against whole tiles: 0.178), half-live tiles 0.236, +-65504 0.262, a saturated
activation 0.984 (its dropped xl.wl product IS the error: the bound's first term is exact there).  Hi-only tier: 0.96 - 0.996 everywhere - its bound
is the half ulp of the one f16 that y is rounded to, which some output always comes close to.  The same library with the xl.wh product taken out of the
K loop failed 102 of the 170 tests that pass here, the float64 comparisons by 87 to 728 times their bound - the figures conv_x2_ref.emulate predicts
per case to three digits.

FOUND AND FIXED (test_one_poisoned_activation_reaches_its_receptive_field_only, its docstring has the figures): the engine did not carry a NaN or an
infinity of an activation into its outputs while conv_x2_tile_kernel ran with MODE.FP16_OVFL = 1 for the life of the wave; the bit is now set around
the epilogue's conversions only."""
import ctypes as C
import math

import pytest
import torch

from tests import conv_x2_ref as XR
from tests.test_gpu_linear import SENTINEL
from tests.test_gpu_trunk_autograd import guarded, guards_intact

pytestmark = pytest.mark.gpu

PERIOD = 1031                        # images of the base of a large case (a prime: the base never lines up with the 192-row tiles)
SENTINEL32 = SENTINEL * 0x10001      # two sentinel halves
WIDE, NARROW = 128, 64               # column-tile widths: NU = 2 when Co % 128 == 0, else NU = 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def slots(dev):
    """block slots of the persistent grid: two blocks per CU"""
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def _bits(t):
    return t.contiguous().view(torch.int16)


class Conv:
    """One ehm_conv_x2 problem: seeded inputs (standard-normal activations, bias and residual times `act`, He-scaled weights), their device forms and
    the float64 reference with its bound.  seg = (Ci2, stride2) adds the second K segment.  N > PERIOD repeats the first PERIOD images."""

    def __init__(self, dev, image, Ci, Co, geom, bias=True, res=True, relu=1, hi_only=False, seg=None, act=1.0, extra_rows=0, seed=0, w=None):
        from egohmr_amd.split_gemm import weight_scale
        self.dev, self.geom, self.relu, self.hi_only, self.seg, self.extra_rows = dev, geom, int(relu), bool(hi_only), seg, extra_rows
        N, H, W = image
        KH, KW, stride, pad = geom
        self.N, self.H, self.W, self.Ci, self.Co = N, H, W, Ci, Co
        self.Nb = min(N, PERIOD)
        self.Ho, self.Wo = XR.out_hw(H, W, KH, KW, stride, pad)
        assert self.Ho > 0 and self.Wo > 0
        self.M, self.Mb = N * self.Ho * self.Wo, self.Nb * self.Ho * self.Wo
        K = KH * KW * Ci + (seg[0] if seg else 0)
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn(self.Nb, H, W, Ci, generator=g) * act
        self.w = torch.randn(Co, Ci, KH, KW, generator=g) * math.sqrt(2.0 / K) if w is None else w
        self.x2 = self.w2 = None
        if seg:
            Ci2, s2 = seg
            self.H2, self.W2 = (self.Ho - 1) * s2 + 1, (self.Wo - 1) * s2 + 1
            self.x2 = torch.randn(self.Nb, self.H2, self.W2, Ci2, generator=g) * act
            self.w2 = torch.randn(Co, Ci2, generator=g) * math.sqrt(2.0 / K)
        self.bias = torch.randn(Co, generator=g) * act if bias else None
        self.res = torch.randn(self.Mb, Co, generator=g) * act if res else None
        self.s = weight_scale(max(float(self.w.abs().max()), float(self.w2.abs().max()) if seg else 0.0))
        self._ref = {}
        self.ws = None

    # ---- device forms
    def _rows(self, base, n_items, rows_per_item, extra=0):
        """base float32 [Nb rows_per_item, C] -> the X2 buffer of n_items rows_per_item pixels (the base repeated), NaN padding rows, the zero row last"""
        pixels = n_items * rows_per_item
        rows = XR.x2_rows(pixels) + extra
        b = XR.pack_x2(base).to(self.dev)
        buf = torch.full((rows, b.shape[1]), XR.NAN_HALF, dtype=torch.int16, device=self.dev).view(torch.float16)
        reps = -(-pixels // b.shape[0])
        buf[:pixels] = b if reps == 1 else b.repeat(reps, 1)[:pixels]
        buf[rows - 1] = 0
        return buf

    def upload(self):
        self.xd = self._rows(self.x.reshape(-1, self.Ci), self.N, self.H * self.W, self.extra_rows)
        self.x2d = None if self.x2 is None else self._rows(self.x2.reshape(-1, self.seg[0]), self.N, self.H2 * self.W2)
        self.rd = None if self.res is None else self._rows(self.res, self.N, self.Ho * self.Wo)
        self.wd = XR.pack_weight(self.w, self.s, self.w2).to(self.dev)
        self.bd = None if self.bias is None else self.bias.to(self.dev)
        return self

    def desc(self, y):
        from egohmr_amd import _lib
        KH, KW, stride, pad = self.geom
        p = lambda t: None if t is None else t.data_ptr()
        d = _lib.ConvX2Desc(p(self.xd), self.xd.shape[0], p(self.wd), p(self.bd), p(self.rd), p(y), self.N, self.H, self.W, self.Ci, self.Co, KH, KW, stride, pad,
                            self.relu, self.s, None, 0)
        if self.seg:
            d.x2, d.x2_rows, d.H2, d.W2, d.Ci2, d.stride2 = p(self.x2d), self.x2d.shape[0], self.H2, self.W2, self.seg[0], self.seg[1]
        d.hi_only = int(self.hi_only)
        return d

    def workspace_bytes(self):
        from egohmr_amd import _lib
        return int(_lib.lib().ehm_conv_x2_workspace_bytes(C.byref(self.desc(None))))

    def run(self, workspace=True):
        """launch once -> (guarded buffer, y as float32 [rows_out, Co]); y is pre-filled with sentinel halves.  workspace = False: whole tiles"""
        from egohmr_amd import _lib
        rows_out = XR.x2_rows(self.M)
        full, y = guarded(self.dev, rows_out, self.Co)
        y.view(torch.int32).fill_(SENTINEL32)
        d = self.desc(y)
        need = self.workspace_bytes()
        if need and workspace:
            if self.ws is None:
                self.ws = torch.zeros(need, dtype=torch.uint8, device=self.dev)
            d.workspace, d.workspace_bytes = self.ws.data_ptr(), need
        _lib.check(_lib.lib().ehm_conv_x2(C.byref(d), None), "ehm_conv_x2")
        torch.cuda.synchronize()
        return full, y

    # ---- reference
    def reference(self, stream_k=False):
        """(ref, bound) float64 [Mb, Co] on the device"""
        if stream_k not in self._ref:
            ops = XR.Operands(self.x, self.w, self.s, self.geom, self.x2, self.w2, self.seg[1] if self.seg else 1)
            ref, pre = XR.conv_ref64(ops, self.bias, self.res, self.relu, self.hi_only)
            self._ref[stream_k] = ref.to(self.dev), XR.tol(ops, self.res, pre, self.hi_only, stream_k).to(self.dev)
        return self._ref[stream_k]

    def halves(self, y):
        """y float32 [rows_out, Co] -> (hi, lo) float16 [rows_out, Co] on the device"""
        return XR.unpack_halves(y.view(torch.float16))

    def value(self, y):
        """the decoded valid outputs, float64 [M, Co] on the device"""
        hi, lo = self.halves(y)
        return hi[:self.M].double() if self.hi_only else hi[:self.M].double() + lo[:self.M].double()

    def expand(self, t):
        """[Mb, ...] -> [M, ...]: the base repeated"""
        return t if self.M == self.Mb else t[torch.arange(self.M, device=t.device) % self.Mb]

    def check_writes(self, full, y, tag):
        assert guards_intact(full), f"{tag}: wrote outside y"
        hi, lo = self.halves(y)
        assert bool((y[-1].view(torch.int32) == 0).all()), f"{tag}: y's zero row is not cleared"
        if self.hi_only:
            assert bool((_bits(lo[:-1]) == SENTINEL).all()), f"{tag}: the hi-only tier wrote {int((_bits(lo[:-1]) != SENTINEL).sum())} lo halves"

    def check(self, full, y, tag, stream_k=False):
        """guards, zero row, sentinel; every valid output element against float64; returns the largest error / bound ratio"""
        self.check_writes(full, y, tag)
        got = self.value(y)
        ref, bound = self.reference(stream_k)
        assert bool(torch.isfinite(got).all()), f"{tag}: {int((~torch.isfinite(got)).sum())} non-finite outputs (a padding row read?)"
        e = (got - self.expand(ref)).abs() / self.expand(bound)
        r = float(e.max())
        print(f"[{tag}] max err/bound = {r:.3f}")
        if r > 1.0:
            i = int(e.argmax())
            row, col = i // self.Co, i % self.Co
            raise AssertionError(f"{tag}: off by {r:.2f} x the bound at row {row} (row tile {row // XR.XBM}, row {row % XR.XBM} in it), column {col}: "
                                 f"got {float(got[row, col])!r}, float64 {float(self.expand(ref)[row, col])!r}; {int((e > 1).sum())} elements over")
        return r


# --------------------------------------------------------------------------------------------- the host packer against the device's
def test_host_pack_equals_ehm_split_pack(dev):
    from egohmr_amd import _lib
    g = torch.Generator().manual_seed(1)
    v = torch.randn(40, 96, generator=g) * torch.logspace(-7, 5, 40)[:, None]
    v[0, :6] = torch.tensor([0.0, 65504.0, -65519.9, 131008.0, 2e5, -float("inf")])
    for scale in (1.0, 256.0):
        src, dst = v.to(dev), torch.empty(40, 96, device=dev)
        _lib.check(_lib.lib().ehm_split_pack(src.data_ptr(), dst.data_ptr(), 40, 96, 96, scale, None))
        torch.cuda.synchronize()
        assert torch.equal(_bits(dst.cpu().view(torch.float16)), _bits(XR.pack_x2(v * scale))), scale


# --------------------------------------------------------------------------------------------- descriptor matrix
BIASES, RESIDUALS, RELUS, TIERS = (False, True), (False, True), (0, 1), (False, True)          # tier: hi_only
# (KH, KW, stride, pad): (1, 1, 1, 1) has output pixels with NO tap inside the image, so have (1, 7, 1, 3) and (7, 1, 1, 3); (4, 8, 1, 2) has 32 taps
GEOMS = ((1, 1, 1, 0), (1, 1, 2, 0), (1, 1, 1, 1), (3, 3, 1, 1), (3, 3, 2, 1), (1, 7, 1, 3), (7, 1, 1, 3), (5, 5, 1, 2), (4, 8, 1, 2))
CIS = (32, 64, 96)                   # K tiles: 1 x 1: 2 (the minimum), 3;  3 x 3: 9, 18, 27;  4 x 8: 32, 64, 96
COS = (32, 64, 96, 128, 160, 192, 256)
IMAGES = ((2, 7, 9), (3, 8, 8), (4, 6, 7))
LEVELS = (BIASES, RESIDUALS, RELUS, TIERS, GEOMS, CIS, COS, IMAGES)
# row = geometry, column = Co, entry = the indices of (bias, residual, relu, tier, Ci, image): a pairwise cover found by search, verified below
_TABLE = ("110112 101011 111011 000111 001011 101020 100012", "100022 110120 101021 000120 001110 011111 110020",
          "100012 011121 001122 111020 000111 010011 010122", "001000 010012 101121 000102 011021 000010 010012",
          "101011 010020 000011 010112 011110 010102 001011", "110110 001002 000001 110002 101112 001011 110120",
          "111111 101122 010001 001002 100110 110110 010100", "010100 000021 100012 100121 101002 101022 000000",
          "101012 101102 101110 011002 011021 010112 001101")
MATRIX = [(BIASES[int(e[0])], RESIDUALS[int(e[1])], RELUS[int(e[2])], TIERS[int(e[3])], GEOMS[i], CIS[int(e[4])], COS[j], IMAGES[int(e[5])])
          for i, row in enumerate(_TABLE) for j, e in enumerate(row.split())]


def _legal(geom, Ci):
    """the K loop needs two K tiles: a 1 x 1 conv of 32 channels is refused"""
    return geom[0] * geom[1] * (Ci // 32) >= 2


def _matrix_id(r):
    b, rs, relu, ho, g, Ci, Co, im = r
    return (f"k{g[0]}x{g[1]}s{g[2]}p{g[3]}-{'x'.join(map(str, im))}-Ci{Ci}-Co{Co}-{'bias' if b else 'nobias'}-{'res' if rs else 'nores'}-relu{relu}-"
            f"{'hi' if ho else 'split'}")


@pytest.mark.parametrize("row", MATRIX, ids=_matrix_id)
def test_conv_x2_descriptor_matrix_vs_fp64(dev, row):
    bias, res, relu, hi_only, geom, Ci, Co, image = row
    c = Conv(dev, image, Ci, Co, geom, bias, res, relu, hi_only, seed=MATRIX.index(row)).upload()
    assert c.workspace_bytes() == 0
    c.check(*c.run(), tag=f"matrix {_matrix_id(row)}")


# --------------------------------------------------------------------------------------------- exact gather
@pytest.mark.parametrize("hi_only", [False, True], ids=["split", "hi"])
@pytest.mark.parametrize("Co", [NARROW, WIDE])
@pytest.mark.parametrize("geom,image,Ci", [((3, 3, 1, 1), (2, 7, 9), 32), ((3, 3, 2, 1), (3, 8, 7), 32), ((1, 1, 2, 0), (3, 7, 8), 64)], ids=["3x3s1", "3x3s2", "1x1s2"])
def test_selector_weights_copy_every_tap_bit_for_bit(dev, geom, image, Ci, Co, hi_only):
    """conv_x2_ref.selector_weights for every tap: y's halves equal the re-split of the gathered pixel (hi-only: its hi half) BIT FOR BIT, zeros at
    out-of-image taps - the gather, the borders, the stride, the tile's row order and its column order with no tolerance at all."""
    for tap in range(geom[0] * geom[1]):
        c = Conv(dev, image, Ci, Co, geom, bias=False, res=False, relu=0, hi_only=hi_only, seed=7, act=3.0, w=XR.selector_weights(geom[0], geom[1], Ci, Co, tap))
        assert c.s == 2048.0
        c.x.view(-1)[::7] *= 1e-4                                                # some lo halves in the f16 subnormal range
        c.upload()
        full, y = c.run()
        c.check_writes(full, y, f"selector tap {tap}")
        hi, lo = c.halves(y)
        if hi_only:
            assert torch.equal(_bits(hi[:c.M].cpu()), _bits(XR.selector_expected_hi_only(c.x, geom, Co, tap))), tap
        else:
            eh, el = XR.selector_expected(c.x, geom, Co, tap)
            bad = (_bits(hi[:c.M].cpu()) != _bits(eh)) | (_bits(lo[:c.M].cpu()) != _bits(el))
            assert not bool(bad.any()), f"tap {tap}: {int(bad.sum())} elements differ, the first at (row, column) {bad.nonzero()[0].tolist()}"


# --------------------------------------------------------------------------------------------- rows
@pytest.mark.parametrize("Co", [NARROW, WIDE])
@pytest.mark.parametrize("M", [1, 191, 192, 193, 385])
def test_conv_x2_row_counts_around_the_tile(dev, M, Co):
    """H = W = 1, 1 x 1: one row, one row short of a tile, a full tile (no padding row at all), one row over, two tiles and one row"""
    c = Conv(dev, (M, 1, 1), 64, Co, (1, 1, 1, 0), seed=M + Co).upload()
    c.check(*c.run(), tag=f"rows M={M} Co={Co}")


@pytest.mark.parametrize("extra", [1, 200])
def test_x_buffer_with_more_rows_than_needed(dev, extra):
    """x_rows > ehm_conv_x2_rows(pixels): the zero row is the buffer's LAST row, every row between the pixels and it holds NaN (3 x 3, pad 1: the
    border taps read the zero row)"""
    c = Conv(dev, (3, 7, 9), 64, 96, (3, 3, 1, 1), extra_rows=extra, seed=extra).upload()
    assert c.xd.shape[0] == XR.x2_rows(3 * 7 * 9) + extra and bool(torch.isnan(c.xd[3 * 7 * 9:-1]).all())
    c.check(*c.run(), tag=f"x_rows + {extra}")


# --------------------------------------------------------------------------------------------- the tile loop without stream-K
def _tile_loop_cases():
    # (tile-count target as (a, b): a slots + b, column tiles, Co): 1, 2, 3 column tiles of both widths (Co = 96: the second narrow tile is half live)
    return [(t, n, Co) for t in ((1, -1), (1, 0), (1, 1), (2, 3)) for n, Co in ((1, 128), (2, 256), (3, 384), (1, 64), (2, 96), (3, 192))]


@pytest.mark.parametrize("target,n_tiles,Co", _tile_loop_cases(), ids=lambda v: "%dslots%+d" % v if isinstance(v, tuple) else str(v))
def test_conv_x2_persistent_tile_loop_vs_fp64(dev, slots, target, n_tiles, Co):
    """Ci = 64 (two K tiles: no stream-K plan), 1 x 1, H = W = 1, N such that the tile count is slots - 1, slots, slots + 1, 2 slots + 3 (rounded up to a
    multiple of the column tiles): blocks with one tile, with two, with three, the prefetch of the next tile across the epilogue, and both answers of
    x2_xcd_order (grid of `slots` blocks: remapped with 1 and 2 column tiles, not with 3; a grid of slots - 1 blocks: never)."""
    assert -(-Co // (WIDE if Co % 128 == 0 else NARROW)) == n_tiles
    m_tiles = -(-(target[0] * slots + target[1]) // n_tiles)
    tiles = m_tiles * n_tiles
    G = min(tiles, slots)
    remap = G % 8 == 0 and (G // 8) % n_tiles == 0
    M = m_tiles * XR.XBM - 5
    c = Conv(dev, (M, 1, 1), 64, Co, (1, 1, 1, 0), seed=tiles + Co).upload()
    assert c.workspace_bytes() == 0
    c.check(*c.run(), tag=f"tile loop {tiles} tiles on {slots} slots, {n_tiles} column tiles of {WIDE if Co % 128 == 0 else NARROW}, remap={remap}")


# --------------------------------------------------------------------------------------------- second K segment
@pytest.mark.parametrize("hi_only", [False, True], ids=["split", "hi"])
@pytest.mark.parametrize("stride2", [1, 2])
@pytest.mark.parametrize("Ci2", [32, 64])
@pytest.mark.parametrize("Ci", [64, 96])
@pytest.mark.parametrize("Co", [128, 256])
def test_conv_x2_second_k_segment_vs_fp64_and_two_launches(dev, Co, Ci, Ci2, stride2, hi_only):
    """relu(conv1x1(x) + conv1x1_stride2(x2) + bias) in one launch: 3, 4 and 5 K tiles in all.  Against float64; and, where the shortcut conv can run on
    its own (Ci2 = 64: two K tiles), against the two-launch route - the shortcut conv, then the main conv with it as residual - under the sum of the
    bounds of the three launches."""
    c = Conv(dev, (3, 5, 6), Ci, Co, (1, 1, 1, 0), bias=True, res=False, relu=1, hi_only=hi_only, seg=(Ci2, stride2), seed=Co + Ci + Ci2 + stride2).upload()
    assert c.workspace_bytes() == 0
    full, y = c.run()
    tag = f"second segment Co={Co} Ci={Ci} Ci2={Ci2} stride2={stride2} {'hi' if hi_only else 'split'}"
    c.check(full, y, tag)
    if Ci2 < 64:
        return
    one = c.value(y)
    # the shortcut on its own: a 1 x 1 conv of x2 with stride2, no bias, no ReLU, the SAME scale (its weights are a column block of the one operand)
    sc = Conv(dev, (3, c.H2, c.W2), Ci2, Co, (1, 1, stride2, 0), bias=False, res=False, relu=0, hi_only=hi_only, w=c.w2[:, :, None, None])
    sc.x, sc.s = c.x2, c.s
    sc.upload()
    fsc, ysc = sc.run()
    r1 = sc.check(fsc, ysc, tag + ": shortcut alone")
    _, bound_sc = sc.reference()
    # the main conv with the shortcut's output as its residual
    main = Conv(dev, (3, 5, 6), Ci, Co, (1, 1, 1, 0), bias=True, res=True, relu=1, hi_only=hi_only, w=c.w)
    main.x, main.s, main.bias, main.res = c.x, c.s, c.bias, sc.value(ysc).float().cpu()         # (hi + lo of an X2 output is a float32)
    main.upload()
    fm, ym = main.run()
    main.check(fm, ym, tag + ": main conv on the shortcut")
    _, bound_one = c.reference()
    _, bound_main = main.reference()
    r = float(((one - main.value(ym)).abs() / (bound_one + bound_sc + bound_main)).max())
    print(f"[{tag}] one launch against two: max diff / sum of bounds = {r:.3f} (shortcut alone {r1:.3f})")
    assert r <= 1.0, r


# --------------------------------------------------------------------------------------------- stream-K
def _stream_k_case(dev, slots, plan, Co, hi_only, seg):
    """the smallest shape that turns a plan of sk_plan (csrc/conv.hip) on, from the block slots of this device:
      every tile: K loop >= 64 K tiles (Ci = 2048, 1 x 1), slots / 2 tiles (the least it takes; under 7 / 8 of a round) -> runs of 16 pairs, each tile cut in two;
      tail only:  one whole round and 2 tiles behind it, K loop of 32 (with the second segment 34) K tiles -> the 2 tiles cut into three runs each"""
    n_tiles = -(-Co // (WIDE if Co % 128 == 0 else NARROW))
    tiles = slots // 2 if plan == "every" else slots + 2
    assert tiles % n_tiles == 0
    M = tiles // n_tiles * XR.XBM - 5
    return Conv(dev, (M, 1, 1), 2048 if plan == "every" else 1024, Co, (1, 1, 1, 0), bias=True, res=not seg, relu=1, hi_only=hi_only, seg=(64, 2) if seg else None,
                seed=tiles + Co)


@pytest.mark.parametrize("plan,Co,hi_only,seg", [("every", 128, False, False), ("every", 64, False, False), ("every", 128, True, False),
                                                 ("tail", 256, False, False), ("tail", 256, False, True), ("tail", 256, True, False)],
                         ids=["every-Co128", "every-Co64", "every-Co128-hi", "tail-Co256", "tail-Co256-seg", "tail-Co256-hi"])
def test_conv_x2_stream_k_vs_fp64(dev, slots, plan, Co, hi_only, seg):
    """Under the stream-K bound; bit-equal across two launches; within the sum of the bounds of the same conv with workspace = NULL (whole tiles);
    ehm_conv_x2_workspace_status is 0 afterwards and every arrival counter is back at zero."""
    from egohmr_amd import _lib
    c = _stream_k_case(dev, slots, plan, Co, hi_only, seg).upload()
    need = c.workspace_bytes()
    assert need > 4096, f"the {plan} plan is off for {c.M} rows, Co = {Co} on {slots} slots"
    tag = f"stream-K {plan} Co={Co}{' hi' if hi_only else ''}{' seg' if seg else ''} ({need >> 10} KiB)"
    full, y = c.run()
    c.check(full, y, tag, stream_k=True)
    full2, y2 = c.run()
    assert guards_intact(full2) and torch.equal(y.view(torch.int32)[:c.M], y2.view(torch.int32)[:c.M]), f"{tag}: two launches differ"
    assert _lib.lib().ehm_conv_x2_workspace_status(c.ws.data_ptr(), None, None) == 0
    assert int(c.ws[:4096].view(torch.int32).abs().sum()) == 0, f"{tag}: arrival counters left behind"
    full0, y0 = c.run(workspace=False)
    c.check(full0, y0, tag + ", workspace = NULL")
    _, b_sk = c.reference(True)
    _, b_whole = c.reference(False)
    r = float(((c.value(y) - c.value(y0)).abs() / c.expand(b_sk + b_whole)).max())
    print(f"[{tag}] stream-K against whole tiles: max diff / sum of bounds = {r:.3f}")
    assert r <= 1.0, r


# --------------------------------------------------------------------------------------------- writes
@pytest.mark.parametrize("hi_only", [False, True], ids=["split", "hi"])
@pytest.mark.parametrize("Co", [32, 96, 160])
def test_half_live_column_tiles_write_nothing_past_co(dev, Co, hi_only):
    """The last 64-wide column tile holds 32 valid columns: the 32 behind them are never written - a write past Co of a row lands in the next row (seen
    by the comparison), of the last tile row in y's zero row (cleared by the call although it was pre-filled: checked), of that row in the guard.  M = 192
    k: the last tile row is a valid one."""
    c = Conv(dev, (192, 1, 1), 64, Co, (1, 1, 1, 0), hi_only=hi_only, seed=Co).upload()
    c.check(*c.run(), tag=f"half-live tile Co={Co} {'hi' if hi_only else 'split'}")


# --------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("Co", [96, 128])
def test_all_zero_weight_gives_the_split_of_the_epilogue_alone(dev, Co, relu):
    """w = 0: exactly the X2 split of act(bias + (rh + rl)) in float32, whatever the activations (weight_scale is 1 then)"""
    c = Conv(dev, (2, 7, 9), 64, Co, (3, 3, 2, 1), relu=relu, seed=41, w=torch.zeros(Co, 64, 3, 3)).upload()
    assert c.s == 1.0
    full, y = c.run()
    c.check_writes(full, y, "zero weight")
    rh, rl = XR.split_x2(c.res)
    v = c.bias[None, :] + (rh.float() + rl.float())
    eh, el = XR.split_x2(torch.relu(v) if relu else v)
    hi, lo = c.halves(y)
    assert torch.equal(_bits(hi[:c.M].cpu()), _bits(eh)) and torch.equal(_bits(lo[:c.M].cpu()), _bits(el))


def test_conv_x2_activations_and_outputs_up_to_the_f16_limit(dev):
    """|x| up to 65504 (hi = +-65504 exactly, lo = 0), and outputs up to +-65504 through the bias and the residual: within the bound, nothing non-finite"""
    c = Conv(dev, (2, 7, 7), 64, 96, (3, 3, 1, 1), seed=21)
    for (n, h, w_, ch), v in {(0, 0, 0, 0): 65504.0, (1, 6, 6, 63): -65504.0, (0, 3, 3, 17): 6e4, (1, 2, 5, 40): -33333.3, (0, 6, 0, 5): 65503.99}.items():
        c.x[n, h, w_, ch] = v
    c.upload()
    r1 = c.check(*c.run(), tag="range |x| <= 65504")
    c = Conv(dev, (2, 7, 7), 64, 96, (3, 3, 1, 1), relu=0, seed=22)
    c.w[5] = 0.0
    c.w[6] = 0.0
    c.bias[3], c.bias[4], c.bias[5], c.bias[6] = 65400.0, -65400.0, 65504.0, -30000.0
    c.res[:, 5] = 0.0
    c.res[:, 6] = -35504.0
    c.upload()
    ref, _ = c.reference()
    assert 65504.0 == float(ref.abs().max()) and float(ref[:, 3].min()) > 65300
    full, y = c.run()
    r2 = c.check(full, y, tag="range |y| <= 65504")
    hi, lo = c.halves(y)
    assert bool((hi[:c.M, 5] == 65504).all()) and bool((lo[:c.M, 5] == 0).all())
    assert max(r1, r2) <= 1.0


OVFL = [7e4, -1e5, 131008.0, 131009.0, 2e5, -1e6, 3e38, 65504.0, 65519.9, 65520.0, -65536.0, 98304.0]


@pytest.mark.parametrize("hi_only", [False, True], ids=["split", "hi"])
def test_outputs_past_the_f16_range_saturate(dev, hi_only):
    """MODE.FP16_OVFL in the epilogue's conversions: a FINITE output v past 65504 is stored as hi = +-65504, lo = f16(clamp(v -+ 65504)) - the value
    itself (at the precision of ONE f16 for the part past 65504) up to +-131008, +-131008 beyond; never inf.  The hi-only tier stores +-65504.  That
    is what ehm_split_pack writes for such a value (conv_x2_ref.split_x2)."""
    Co = 96
    c = Conv(dev, (1, 3, 4), 64, Co, (1, 1, 1, 0), res=False, relu=0, hi_only=hi_only, seed=3, w=torch.zeros(Co, 64, 1, 1))
    c.bias[:len(OVFL)] = torch.tensor(OVFL)
    c.upload()
    full, y = c.run()
    c.check_writes(full, y, "overflow")
    hi, lo = (h[:c.M].cpu() for h in c.halves(y))
    eh, el = XR.split_x2(c.bias[None, :].expand(c.M, Co))
    print(f"[overflow {'hi' if hi_only else 'split'}] bias {OVFL} -> hi {hi[0, :len(OVFL)].tolist()} lo {lo[0, :len(OVFL)].tolist()}")
    assert bool(torch.isfinite(hi).all()) and torch.equal(_bits(hi), _bits(eh))
    if not hi_only:
        assert bool(torch.isfinite(lo).all()) and torch.equal(_bits(lo), _bits(el))
        assert (hi[0, :7].double() + lo[0, :7].double()).tolist() == [7e4, -1e5, 131008.0, 131008.0, 131008.0, -131008.0, 131008.0]


POISON_AT = (1, 3, 4, 37)            # (n, h, w, channel) of the poisoned activation
POISONS = {"nan-hi": (float("nan"), 0.0), "nan-lo": (None, float("nan")), "inf": (float("inf"), 0.0), "saturated": (65504.0, 65504.0)}


@pytest.mark.parametrize("hi_only", [False, True], ids=["split", "hi"])
@pytest.mark.parametrize("geom,Ci", [((1, 1, 1, 0), 256), ((3, 3, 2, 1), 64)], ids=["k1x1", "k3x3s2p1"])
@pytest.mark.parametrize("bad", list(POISONS))
def test_one_poisoned_activation_reaches_its_receptive_field_only(dev, bad, geom, Ci, hi_only):
    """One activation whose halves are (NaN, 0), (its hi half, NaN), (inf, 0) or (65504, 65504) - the saturated form ehm_split_pack and the epilogue give any
    finite value past +-131008 - in one input pixel:
      NaN / inf: with relu = 0 exactly the outputs whose receptive field holds the pixel are non-finite, in every channel; with relu = 1 the epilogue's
        max(v, 0) returns 0 for a NaN or -inf: non-finite or exactly 0.  In the hi-only tier a NaN in the LO half is not read: no output changes.
      saturated: the value IS 131008 - the format has no range flag - and every output is finite and within the bound of the float64 reference.
    Every output outside the receptive field keeps the bits of the clean launch.

    This test found a defect (docs/EXPERIMENTS.md, R32.3).  While conv_x2_tile_kernel kept MODE.FP16_OVFL = 1 for the life of the wave, 10 of the 16
    cases failed on an MI355X: nan-hi and inf in both tiers, nan-lo in the split tier, both geometries ("outside the receptive field" held in all 16).
    Measured then, 1 x 1, Ci = 256, relu = 0, the poisoned pixel's row, first channels, clean outputs 1.7911 / -2.9092 / 1.8502 / -2.1178:
      NaN in the hi half:  1.7301 / -3.0313 / 1.1376 / -1.2848 - finite and plausible, neither the clean value nor the value with the activation at
                           zero (1.7179 / -2.9107 / 1.8629 / -2.0946); 96 of 96 field outputs finite (3 x 3 stride 2: 192 of 192);
      NaN in the lo half:  1.7681 / -3.2361 / 1.4206 / -1.9431, again all finite;
      inf:                 +-131008 (hi = lo = +-65504) with the sign of the weight: the saturated form, finite.
    With that bit set the matrix cores do not propagate a non-finite f16 operand.  The kernel now sets the bit around each epilogue's f32 -> f16
    conversions only (x2_fp16_ovfl_on / x2_fp16_ovfl_off, csrc/x2_tile_dev.h) and its K loop runs with the bit clear: all 16 cases pass, and the
    saturation of FINITE overflows (test_outputs_past_the_f16_range_saturate) is as it was - the conversions themselves pass a NaN and an infinity on."""
    h_bad, l_bad = POISONS[bad]
    for relu in (0, 1):
        c = Conv(dev, (2, 8, 8), Ci, 96, geom, relu=relu, hi_only=hi_only, seed=31).upload()
        _, clean = c.run()
        n, h, w_, ch = POISON_AT
        row, col = (n * 8 + h) * 8 + w_, (ch // 32) * 64 + ch % 32
        if h_bad is not None:
            c.xd[row, col] = h_bad
        c.xd[row, col + 32] = l_bad
        full, y = c.run()
        c.check_writes(full, y, f"poison {bad}")
        ind = torch.zeros(2, 8, 8, Ci)
        ind[POISON_AT] = 1.0
        field = XR.gather(ind, geom).sum(1) > 0                                                   # the rows of the GEMM that gather the pixel
        assert 0 < int(field.sum()) < field.numel()
        hit = field[:, None].expand(c.M, 96).contiguous().to(dev)
        same = y.view(torch.int32)[:c.M] == clean.view(torch.int32)[:c.M]
        assert bool(same[~hit].all()), "an output outside the receptive field changed"
        got = c.value(y)
        if bad == "saturated":
            c.x[POISON_AT] = 131008.0
            c._ref = {}
            ref, bound = c.reference()
            assert float(ref.abs().max()) <= 65504 and bool(torch.isfinite(got).all())
            r = float(((got - ref).abs() / bound).max())
            print(f"[saturated activation {geom} relu={relu} {'hi' if hi_only else 'split'}] max err/bound = {r:.3f}")
            assert r <= 1.0 and not bool(same[hit].all())
        elif hi_only and bad == "nan-lo":
            assert bool(same.all()), "the hi-only tier read a lo half"
        elif relu:
            assert bool((~torch.isfinite(got[hit]) | (got[hit] == 0)).all()) and bool(torch.isfinite(got[~hit]).all())
        else:
            nf = ~torch.isfinite(got)
            assert bool(nf[hit].all()) and not bool(nf[~hit].any()), f"{int((~nf[hit]).sum())} finite outputs inside the receptive field, {int(nf[~hit].sum())} non-finite outside"


# --------------------------------------------------------------------------------------------- refusals
def test_conv_x2_refusals_leave_y_alone(dev):
    """What ehm_conv_x2 decides before any device call, on real buffers: Co % 32, Ci % 32, fewer than two K tiles, a missing zero row (x and x2), a
    shortcut grid that does not map onto the output grid, Co % 128 with a second segment.  Every call returns an error and y keeps its pre-fill."""
    from egohmr_amd import _lib
    L = _lib.lib()
    c = Conv(dev, (2, 5, 6), 64, 128, (1, 1, 1, 0), seg=(64, 2), res=False).upload()
    full, y = guarded(dev, XR.x2_rows(c.M), 128)
    y.view(torch.int32).fill_(SENTINEL32)
    assert L.ehm_conv_x2(C.byref(c.desc(y)), None) == 0                          # (the descriptor itself is fine)
    y.view(torch.int32).fill_(SENTINEL32)
    torch.cuda.synchronize()
    for field, value in (("Co", 112), ("Co", 16), ("Ci", 48), ("Ci", 16), ("Ci", 32), ("x_rows", c.xd.shape[0] - 1), ("x2_rows", c.x2d.shape[0] - 1),
                         ("H2", c.H2 + 2), ("W2", c.W2 - 1), ("stride2", 1), ("Co", 64), ("Co", 96)):
        d = c.desc(y)
        setattr(d, field, value)
        assert L.ehm_conv_x2(C.byref(d), None) != 0, (field, value)
    d = c.desc(y)                                                                # one K tile without the second segment
    d.x2, d.Ci = None, 32
    assert L.ehm_conv_x2(C.byref(d), None) != 0
    torch.cuda.synchronize()
    assert guards_intact(full) and bool((y.view(torch.int32) == SENTINEL32).all())
