"""GPU (MI355X): the ResNet stem (ehm_resnet_stem, csrc/stem.hip) called through _lib, on the paths production takes: float32 rows against float64
(tests/stem_ref.py: stem_ref64) under the derived bound of that module (stem_tol; tests/test_stem_cpu.py shows that the bound tells the stem from one
that drops a correction product), the X2 rows (out_x2 = 1, what ResNet50Features.folded() uses) bit for bit against the row law applied to the float32
output of the same inputs, and the persistent patch loop on more patches than resident blocks.

In every call the scratch buffer is NaN before the call (a padded float the conv reads and stem_pad_kernel does not write would show; afterwards the
padded image must be the zero-padded image exactly), the output sits between canary guards, and the output is NaN (float32) or a canary half (X2, 0x7E00,
a NaN too) before the call, so that a pixel nobody writes shows.  Every float64 reference is computed once per module.

Measured on an MI355X (256 CUs: 512 resident blocks), largest error / bound per case: standard-normal image 0.054 at (1, 32, 32) and 0.053 at (3, 64, 96);
the image plus 8 0.048 / 0.050; the image times 1e-3 0.180 / 0.199 (the floor term of the bound: the CPU restatement gives 0.163 at (2, 32, 64)); zero
image 0 (exactly relu(b)); a bias of -100 on every second channel 0.057; pooled outputs up to 1.2e5 (1577 of 73728 above 65504) 0.068; 257 images of
32 x 32 (514 patches) 0.067; 87 images of 64 x 96 (522 patches) 0.071.  Every X2 comparison and every bit comparison held.  The same library without the
pooled tile's clear from a block's second patch on fails both persistent tests and no other; with the clamp of the X2 hi half taken out it fails the
beyond-f16 test alone; with the al.wh MFMA taken out it fails every float64 comparison but the zero image, by 1.8 - 2.4 times the bound at the image
times 1e-3 and 30 - 58 times elsewhere (docs/EXPERIMENTS.md, round 26)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import conv_split_ref as CR
from tests import stem_ref as SR
from tests.test_gpu_trunk_autograd import guarded, guards_intact
from tests.test_stem_cpu import FAMILIES, family_inputs

pytestmark = pytest.mark.gpu

NAN = float("nan")
X2_CANARY = 0x7E00                   # a half NaN
SHAPES = [(1, 32, 32), (3, 64, 96)]  # the smallest legal image (7 + 1 pooled rows); partial patches on both axes (7 + 7 + 2 rows, 14 + 10 columns)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


class Case:
    """float32 inputs of one stem call with their float64 reference and bound (computed on first use, kept, left unchanged)."""

    def __init__(self, img, w, b):
        self.img, self.w, self.b = img.contiguous(), w, b
        self.N, _, self.H, self.W = img.shape
        self.pixels = self.N * (self.H // 4) * (self.W // 4)

    @functools.cached_property
    def ref(self):
        return SR.stem_ref64(self.img, self.w, self.b)[0]

    @functools.cached_property
    def bound(self):
        return SR.stem_tol(self.img, self.w, self.b)

    def head(self, n0, n1):
        """the case of images n0 .. n1 - 1 alone (no reference of its own)"""
        return Case(self.img[n0:n1], self.w, self.b)


@functools.lru_cache(maxsize=None)
def family_case(family, shape):
    return Case(*family_inputs(family, *shape))


@functools.lru_cache(maxsize=None)
def special_case(kind):
    img, w, b = family_inputs("normal", 3, 64, 96, seed=11)
    if kind == "zero_image":
        return Case(torch.zeros_like(img), w, b)
    if kind == "closed_channels":                                          # a bias of -100 on every second channel: conv values are a few units
        b = b.clone()
        b[::2] = -100.0
        return Case(img, w, b)
    assert kind == "beyond_f16"                                            # everything times a power of two: pooled outputs around 1e5
    return Case(img * 128.0, w * 128.0, b * 16384.0)


def run(dev, case, x2):
    """One ehm_resnet_stem call under the three rules of the module docstring -> float32 [N, H/4, W/4, 64], or the whole X2 buffer as int16 [rows, 128]."""
    from egohmr_amd import _lib
    A = _lib.api()
    N, H, W = case.N, case.H, case.W
    img = case.img.to(dev)
    wt, b = case.w.reshape(64, 147).t().contiguous().to(dev), case.b.to(dev)
    scratch = torch.full((A.ehm_resnet_stem_scratch_bytes(N, H, W) // 4,), NAN, device=dev)
    if x2:
        rows = int(A.ehm_conv_x2_rows(case.pixels))
        assert rows > case.pixels                                          # (tile padding and the zero row: not the stem's to write)
        full, y = guarded(dev, rows, 64)
        y.view(torch.int16).fill_(X2_CANARY)
    else:
        full, y = guarded(dev, N, H // 4, W // 4, 64)
        y.fill_(NAN)
    A.ehm_resnet_stem(img, wt, b, scratch, y, N, H, W, 1 if x2 else 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert guards_intact(full)
    # the padded image: 5 zeros left / on top, 3 right / below, every float written
    padded = scratch[:N * 3 * (H + 8) * (W + 8)].view(N, 3, H + 8, W + 8)
    assert torch.equal(padded, torch.nn.functional.pad(img, (5, 3, 5, 3)))
    return y.view(torch.int16).cpu() if x2 else y.cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


def check_f32(tag, case, y):
    """float32 rows against float64 under the bound; prints and returns the largest error / bound ratio"""
    assert y.shape == case.ref.shape and bool(torch.isfinite(y).all()), tag
    assert not bool((bits(y) < 0).any()), f"{tag}: a negative or -0.0 output behind the ReLU"
    r = CR.ratio(y, case.ref, case.bound)
    print(f"[stem {tag}] largest err/bound = {r:.3f} (max|y| = {float(case.ref.abs().max()):.4g})")
    assert r <= 1.0, f"{tag}: over the bound ({r:.3f})"
    return r


def check_x2(tag, case, rows, y):
    """X2 rows against the row law applied to the float32 output y of the same inputs, hi and lo bit for bit; every row past the pixels keeps the canary"""
    want = SR.split_x2(y.reshape(case.pixels, 64).numpy())
    got = rows.numpy()
    assert got.shape[1] == SR.ROW_HALVES and np.array_equal(got[:case.pixels], want), \
        f"{tag}: {int((got[:case.pixels] != want).sum())} X2 halves differ from the row law"
    assert bool((got[case.pixels:] == X2_CANARY).all()), f"{tag}: a row past the pixels was written"


# ------------------------------------------------------------------------------------------------ float32 rows, X2 rows
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", FAMILIES)
def test_rows_against_float64_and_x2_rows_against_the_row_law(dev, family, shape):
    case = family_case(family, shape)
    tag = f"{family} {shape}"
    y = run(dev, case, x2=False)
    check_f32(tag, case, y)
    assert torch.equal(bits(run(dev, case, x2=False)), bits(y))            # integer maxima: the float32 output is deterministic
    check_x2(tag, case, run(dev, case, x2=True), y)


def test_zero_image_gives_relu_of_the_bias(dev):
    case = special_case("zero_image")
    y = run(dev, case, x2=False)
    want = torch.relu(case.b).view(1, 1, 1, 64).expand_as(y)
    assert bool((case.b < 0).any()) and bool((case.b > 0).any())
    assert torch.equal(bits(y), bits(want))                                # exactly relu(b); +0.0 where b < 0
    check_f32("zero image", case, y)
    check_x2("zero image", case, run(dev, case, x2=True), y)


def test_closed_channels_are_positive_zero(dev):
    case = special_case("closed_channels")
    assert float(SR.stem_ref64(case.img, case.w, case.b)[1][..., ::2].max()) < 0      # every pre-pool value of those channels is negative
    y = run(dev, case, x2=False)
    assert bool((bits(y)[..., ::2] == 0).all())                            # +0.0 bit for bit, not -0.0
    assert bool((y[..., 1::2] > 0).any())
    check_f32("bias -100 on every second channel", case, y)
    rows = run(dev, case, x2=True)
    check_x2("bias -100 on every second channel", case, rows, y)
    hi, lo = SR.decode_x2(rows, case.pixels)
    assert not hi.view(np.uint16)[:, ::2].any() and not lo.view(np.uint16)[:, ::2].any()


def test_outputs_beyond_the_f16_range(dev):
    case = special_case("beyond_f16")
    over = case.ref > CR.F16_MAX
    print(f"[stem beyond f16] {int(over.sum())} of {over.numel()} pooled outputs above 65504, the largest {float(case.ref.max()):.6g}")
    assert int(over.sum()) > 0 and 7e4 < float(case.ref.max()) < 2e5       # around 1e5
    assert float(case.img.abs().max()) < CR.F16_MAX and float(case.w.abs().max()) < CR.F16_MAX      # the operands themselves stay inside
    y = run(dev, case, x2=False)
    check_f32("beyond f16", case, y)
    rows = run(dev, case, x2=True)
    check_x2("beyond f16", case, rows, y)
    hi, lo = SR.decode_x2(rows, case.pixels)
    big = (y.reshape(-1, 64) > CR.F16_MAX).numpy()
    assert big.any() and bool((hi[big] == np.float16(CR.F16_MAX)).all()) and bool(np.isfinite(lo[big]).all()) and bool((lo[big] > 0).all())


# ------------------------------------------------------------------------------------------------ more patches than resident blocks
def persistent_images(cus, H, W):
    return {(32, 32): cus + 1, (64, 96): math.ceil(2 * cus / 6) + 1}[(H, W)]


@functools.lru_cache(maxsize=None)
def persistent_case(N, H, W):
    """N distinct standard-normal images"""
    return Case(*family_inputs("normal", N, H, W, seed=100 + H))


@pytest.mark.parametrize("H,W", [(32, 32), (64, 96)])
def test_more_patches_than_resident_blocks(dev, cus, H, W):
    """The grid is min(patches, 2 CUs) blocks: here at least one block takes a second patch, after clearing the pooled tile it has just written out.  A
    patch's result depends on its image alone, so the images of the big run have the bits of runs that take one turn."""
    N = persistent_images(cus, H, W)
    slots = 2 * cus
    assert SR.patches(N, H, W) > slots
    case = persistent_case(N, H, W)
    tag = f"{N} x {H}x{W}, {SR.patches(N, H, W)} patches on {slots} blocks"
    y = run(dev, case, x2=False)
    check_f32(tag, case, y)
    check_x2(tag, case, run(dev, case, x2=True), y)
    # the first CUs // 2 images alone - with six patches an image that is more images than the run has and more patches than blocks: there, the most
    # images that still take one turn
    n = min(cus // 2, slots // SR.patches(1, H, W))
    assert 0 < n < N and SR.patches(n, H, W) <= slots
    assert torch.equal(bits(run(dev, case.head(0, n), x2=False)), bits(y[:n])), f"{tag}: the first {n} images differ from a run of them alone"
    assert torch.equal(bits(run(dev, case.head(N - 1, N), x2=False)), bits(y[N - 1:])), f"{tag}: the last image differs from a run of it alone"
