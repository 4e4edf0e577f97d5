"""CPU: the error bound of tests/stem_ref.py (conv_split_ref.tol of the conv pixels, max-pooled) tells the ResNet stem (csrc/stem.hip) from a stem
that drops one of its two correction products; the X2 row law and the host arithmetic tests/test_gpu_stem.py relies on are pinned against
hand-computed values.  The GPU side is tests/test_gpu_stem.py.

At images of order 1 (and the same plus 8: large cancelling sums) the emulated stem sits well under a fifth of the pooled bound and either mutant tens of
times over it.  At images of order 1e-3 the lo halves of the image sit in the f16 subnormal range and a mutant is only a few times over: the property
of the split format that tests/conv_split_ref.py's docstring describes.  Asserted are only < 1 and > 1; the ratios are printed."""
import numpy as np
import pytest
import torch

from tests import conv_split_ref as CR
from tests import stem_ref as SR

MUTANTS = ("alwh", "ahwl")
FAMILIES = ("normal", "plus8", "times1e-3")


def family_inputs(family, N, H, W, seed=0):
    """(img [N,3,H,W], w [64,3,7,7], b [64]) float32: a standard-normal image, 0.1 randn weights, a randn bias; "plus8": the image plus 8 (large
    cancelling sums: the lo halves matter); "times1e-3": the image times 1e-3 (its lo halves in the f16 subnormal range)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(N, 3, H, W, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    b = torch.randn(64, generator=g)
    if family == "plus8":
        img = img + 8.0
    elif family == "times1e-3":
        img = img * 1e-3
    else:
        assert family == "normal"
    return img, w, b


@pytest.mark.parametrize("family", FAMILIES)
def test_pooled_bound_tells_the_stem_from_one_without_a_correction_product(family):
    img, w, b = family_inputs(family, 2, 32, 64)
    ref, _ = SR.stem_ref64(img, w, b)
    bound = SR.stem_tol(img, w, b)
    assert ref.shape == bound.shape == (2, 8, 16, 64) and bool((bound > 0).all())
    r = [CR.ratio(SR.emulate(img, w, b, drop=d), ref, bound) for d in (None,) + MUTANTS]
    print(f"[{family}] err/bound: stem {r[0]:.3f}, without al.wh {r[1]:.2f}, without ah.wl {r[2]:.2f}")
    assert r[0] < 1.0 and r[1] > 1.0 and r[2] > 1.0, r


def test_emulation_of_exactly_representable_operands_is_exact():
    """Small integers are their own hi halves and every partial sum is an integer below 2^24: the emulation returns the float64 result exactly - its
    gather (stride, padding zeros, the (ci, kh) x 8 tap rows) is the reference's."""
    g = torch.Generator().manual_seed(1)
    img = torch.randint(-8, 9, (2, 3, 32, 64), generator=g).float()
    w = torch.randint(-4, 5, (64, 3, 7, 7), generator=g).float()
    b = torch.randint(-50, 51, (64,), generator=g).float()
    ref, _ = SR.stem_ref64(img, w, b)
    assert bool((ref > 0).any()) and torch.equal(SR.emulate(img, w, b).double(), ref)


def test_x2_rows_round_trip_and_layout():
    g = np.random.default_rng(2)
    v = np.abs(g.normal(size=(5, 64))).astype(np.float32)
    v[0, :4] = [0.0, 65504.0, 65520.0, 1e5]                                # +0, the largest half, the rounding edge to inf, beyond the range
    v[1, 7] = 2.0 ** -26                                                    # below the smallest f16 subnormal: hi = lo = 0
    v[2, 40] = 1.0 + 2.0 ** -12                                             # a lo half in the subnormal range (2^-12 is normal; 2^-20 below)
    v[2, 41] = 1.0 + 2.0 ** -20
    rows = SR.split_x2(v)
    assert rows.shape == (5, 128) and rows.dtype == np.int16
    hi, lo = SR.decode_x2(rows, 5)
    assert hi.dtype == lo.dtype == np.float16 and hi.shape == lo.shape == (5, 64)
    # the row law, element by element, at the addresses the kernel uses
    halves = rows.view(np.float16)
    for p in range(5):
        for c in range(64):
            at = (c >> 5) * 64 + (c & 31)
            h = np.float16(min(v[p, c], np.float32(65504.0)))
            assert halves[p, at] == h == hi[p, c] and halves[p, at + 32] == np.float16(v[p, c] - np.float32(h)) == lo[p, c], (p, c)
    # hi + lo keeps 22 bits of a value in the f16 range
    inside = v <= 65504.0
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - v.astype(np.float64))
    assert bool((err[inside] <= 2.0 ** -22 * v[inside] + 2.0 ** -25).all())
    # beyond the range: hi is the largest half, lo the finite rest
    assert hi[0, 1] == hi[0, 2] == hi[0, 3] == np.float16(65504.0) and lo[0, 1] == 0 and lo[0, 2] == np.float16(16.0)
    assert np.isfinite(lo[0, 3]) and lo[0, 3] == np.float16(1e5 - 65504.0)
    assert rows.view(np.uint16)[0, 0] == 0 and rows.view(np.uint16)[0, 32] == 0                 # +0.0, not -0.0
    assert hi[1, 7] == 0 and lo[1, 7] == 0 and lo[2, 40] == np.float16(2.0 ** -12) and lo[2, 41] == np.float16(2.0 ** -20)
    # a tensor read back as float32 rows of 64 decodes like the array
    t = torch.from_numpy(rows.copy()).view(torch.float32)
    assert t.shape == (5, 64)
    h2, l2 = SR.decode_x2(t, 4)
    assert np.array_equal(h2.view(np.uint16), hi[:4].view(np.uint16)) and np.array_equal(l2.view(np.uint16), lo[:4].view(np.uint16))


def test_patch_and_chunk_arithmetic():
    assert SR.patches(1, 32, 32) == 2                                      # 8 pooled rows = 7 + 1, 8 columns
    assert SR.patches(2, 224, 224) == 64                                   # 56 = 8 x 7 rows, 56 = 4 x 14 columns
    assert SR.patches(1, 64, 96) == 6                                      # 16 = 7 + 7 + 2 rows, 24 = 14 + 10 columns
    assert SR.patches(3, 64, 96) == 18 and SR.patches(256, 224, 224) == 8192
    assert SR.backward_chunk(224, 224) == 10 and SR.backward_chunk(64, 64) == 128 and SR.backward_chunk(32, 32) == 512
    assert SR.backward_chunk(2048, 2048) == 1                              # an image above 8 Mi floats: one at a time
