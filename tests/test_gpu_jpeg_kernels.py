"""GPU: the three JPEG device kernels called directly through the C ABI (ehm_jpeg_decode: jpeg_idct_kernel + jpeg_colour_kernel;
ehm_jpeg_forward: jpeg_forward_kernel) on the synthetic cases of tests/jpeg_cases.py, against the numpy restatements tests/jpeg_ref.py and
tests/jpeg_enc_ref.py.  tests/test_jpeg_cases_cpu.py shows what the cases reach and that each planted mistake of the restatements changes
some case: a separate table for Cr, several frames per call, sizes off the 8-pixel grid, every chroma width and height at an edge, both
clamps far out of range, padding blocks with content of their own.  The planes in the workspace are compared too, so a difference is placed
in the IDCT or in the colour kernel, and every buffer sits between guard bytes.  The rule is integer: every bar is equality."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases as cases  # noqa: E402
import jpeg_enc_ref as enc_ref  # noqa: E402
import jpeg_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
DECODE_GROUPS = [(s, c) for s in cases.SAMPLINGS for c in cases.CONTENTS]
FORWARD_GROUPS = [(s, c) for s in ("444", "422", "420") for c in cases.FORWARD_CONTENTS]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


class Guarded:
    """``nbytes`` bytes at byte ``offset`` behind a 64-byte guard inside a larger buffer, another 64 guard bytes behind them, all pre-filled
    with ``fill``.  The buffer's base is at least 256-byte aligned (asserted), so offset 0 keeps a 16-byte alignment."""

    def __init__(self, dev, nbytes, offset=0, fill=0xA5):
        self.buf = torch.full((GUARD + offset + nbytes + GUARD,), fill, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 256 == 0
        self.lo, self.hi, self.fill = GUARD + offset, GUARD + offset + nbytes, fill
        self.ptr = self.buf.data_ptr() + self.lo

    def host(self):
        """-> the payload as numpy uint8, after asserting that every byte outside it still holds the fill"""
        h = self.buf.cpu().numpy()
        assert (h[:self.lo] == self.fill).all() and (h[self.hi:] == self.fill).all(), "a guard byte was written"
        return h[self.lo:self.hi]


def _same(got, want, case_id, stage):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        pytest.fail(f"{case_id}: {stage} differ in {bad.size} of {want.size} bytes, first at index {int(bad[0])} "
                    f"(got {int(got.reshape(-1)[bad[0]])}, want {int(want.reshape(-1)[bad[0]])})")


def decode_desc(case, coef, quant, frames_ptr, ws_ptr, ws_bytes):
    from egohmr_amd import _lib
    return _lib.JpegDecodeDesc(coef=coef.data_ptr(), quant=quant.data_ptr(), H=case["H"], W=case["W"], components=case["components"],
                               hmax=case["hmax"], vmax=case["vmax"], F=case["F"], frames=frames_ptr, workspace=ws_ptr, workspace_bytes=ws_bytes)


def run_decode(dev, case, coef=None, frames_offset=0, fill=0xA5):
    """One ehm_jpeg_decode on guarded buffers -> (planes uint8 [F, coef_count], pixels uint8 [F, H, W, 3]); the workspace is exactly as large
    as ehm_jpeg_workspace_bytes asks."""
    from egohmr_amd import _lib
    F, H, W = case["F"], case["H"], case["W"]
    coef = torch.from_numpy(case["coef"]).to(dev) if coef is None else coef
    quant = torch.from_numpy(case["quant"]).to(dev)
    assert coef.data_ptr() % 16 == 0 and quant.data_ptr() % 16 == 0
    d = decode_desc(case, coef, quant, 0, 0, 0)
    need = C.c_int64(0)
    _lib.api().ehm_jpeg_workspace_bytes(C.byref(d), C.byref(need))
    assert need.value == coef.numel()                                   # one plane byte per coefficient
    ws, frames = Guarded(dev, need.value, fill=fill), Guarded(dev, F * H * W * 3, offset=frames_offset, fill=fill)
    d.frames, d.workspace, d.workspace_bytes = frames.ptr, ws.ptr, need.value
    _lib.api().ehm_jpeg_decode(C.byref(d), _lib.stream_ptr())
    torch.cuda.synchronize()
    return ws.host().reshape(F, -1), frames.host().reshape(F, H, W, 3)


def run_forward(dev, case, frames_offset=0, fill=0xA5):
    """One ehm_jpeg_forward on guarded buffers -> int16 [F, coef_count]"""
    from egohmr_amd import _lib
    F, H, W = case["F"], case["H"], case["W"]
    count = 64 * sum(a * b for a, b in jpeg_ref.block_grids(H, W, 3, case["hmax"], case["vmax"]))
    src = Guarded(dev, F * H * W * 3, offset=frames_offset)
    src.buf[src.lo:src.hi] = torch.from_numpy(case["frames"].reshape(-1)).to(dev)
    quant = torch.from_numpy(case["quant"]).to(dev)
    coef = Guarded(dev, F * count * 2, fill=fill)
    assert coef.ptr % 16 == 0
    d = _lib.JpegForwardDesc(frames=src.ptr, quant=quant.data_ptr(), H=H, W=W, hmax=case["hmax"], vmax=case["vmax"], F=F, rgb=case["rgb"], coef=coef.ptr)
    _lib.api().ehm_jpeg_forward(C.byref(d), _lib.stream_ptr())
    torch.cuda.synchronize()
    src.host()                                                          # (the input's guards too)
    return coef.host().view(np.int16).reshape(F, count)


# ---------------------------------------------------------------------------------------------------- ehm_jpeg_decode

@pytest.mark.parametrize("sampling,content", DECODE_GROUPS, ids=[f"{s}-{c}" for s, c in DECODE_GROUPS])
def test_decode_equals_the_restatement_on_every_case(dev, sampling, content):
    group = [(cid, c) for cid, c in cases.decode_cases() if c["sampling"] == sampling and c["content"] == content]
    assert group
    for cid, case in group:
        want_planes, want_pixels = cases.decode_want(case)
        planes, pixels = run_decode(dev, case)
        _same(planes, want_planes, cid, "planes")
        _same(pixels, want_pixels, cid, "pixels")
        again_planes, again_pixels = run_decode(dev, case, fill=0x3C)    # a second call, over another fill: every byte is written, the same
        _same(again_planes, planes, cid, "planes of the second call")
        _same(again_pixels, pixels, cid, "pixels of the second call")
    print(f"{sampling} {content}: {len(group)} cases equal")


@pytest.mark.parametrize("case_id", ["420-16x16-dense", "gray-8x16-sparse_extreme"])
def test_decode_into_unaligned_frames(dev, case_id):
    """W % 8 == 0 with frames off the 8-byte grid: the colour kernel's byte-wise stores instead of its 8-byte ones"""
    case = dict(cases.decode_cases())[case_id]
    assert case["W"] % 8 == 0
    _, aligned = run_decode(dev, case)
    _same(aligned, cases.decode_want(case)[1], case_id, "pixels")
    for offset in (1, 4):
        _same(run_decode(dev, case, frames_offset=offset)[1], aligned, case_id, f"pixels at byte offset {offset}")


# ---------------------------------------------------------------------------------------------------- ehm_jpeg_forward

@pytest.mark.parametrize("sampling,content", FORWARD_GROUPS, ids=[f"{s}-{c}" for s, c in FORWARD_GROUPS])
def test_forward_equals_the_restatement_on_every_case(dev, sampling, content):
    group = [(cid, c) for cid, c in cases.forward_cases() if c["sampling"] == sampling and c["content"] == content]
    assert group
    for cid, case in group:
        want = cases.forward_want(case)
        got = run_forward(dev, case)
        _same(got.view(np.uint8), want.view(np.uint8), cid, "coefficients")
        _same(run_forward(dev, case, fill=0x3C).view(np.uint8), got.view(np.uint8), cid, "coefficients of the second call")
        _same(run_forward(dev, case, frames_offset=1).view(np.uint8), got.view(np.uint8), cid, "coefficients from frames at byte offset 1")
    print(f"{sampling} {content}: {len(group)} cases equal")


# ---------------------------------------------------------------------------------------------------- the two together

@pytest.mark.parametrize("sampling,H,W", [("444", 9, 17), ("422", 9, 17), ("420", 17, 9), ("420", 3, 21)])
def test_forward_feeds_decode_on_the_device(dev, sampling, H, W):
    """Odd sizes; all but the 4:4:4 one have dummy blocks (a dummy luma column, a dummy luma row, both)"""
    from egohmr_amd import _lib
    _, hmax, vmax = cases.SAMPLINGS[sampling]
    rng = np.random.default_rng([H, W, hmax, vmax])
    F = 2
    bgr = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    quant = rng.integers(1, 256, (F, 3, 64)).astype(np.uint16)
    case = dict(H=H, W=W, components=3, hmax=hmax, vmax=vmax, F=F, quant=quant)
    grids = jpeg_ref.block_grids(H, W, 3, hmax, vmax)
    real = [(-(-H // 8), -(-W // 8))] + [(-(-H // (8 * vmax)), -(-W // (8 * hmax)))] * 2
    assert (grids != real) == (sampling != "444")
    frames_d, quant_d = torch.from_numpy(bgr).to(dev), torch.from_numpy(quant).to(dev)
    coef_d = torch.full((F, 64 * sum(a * b for a, b in grids)), 0x5A5A, dtype=torch.int16, device=dev)
    d = _lib.JpegForwardDesc(frames=frames_d.data_ptr(), quant=quant_d.data_ptr(), H=H, W=W, hmax=hmax, vmax=vmax, F=F, rgb=0, coef=coef_d.data_ptr())
    _lib.api().ehm_jpeg_forward(C.byref(d), _lib.stream_ptr())
    planes, pixels = run_decode(dev, case, coef=coef_d)
    for f in range(F):
        coef = enc_ref.coefficients(bgr[f][..., ::-1], quant[f], hmax, vmax)
        _same(coef_d[f].cpu().numpy().view(np.uint8), coef.view(np.uint8), f"{sampling}-{H}x{W} frame {f}", "coefficients")
        want_planes, want_pixels = jpeg_ref.planes_and_pixels(coef, quant[f], H, W, 3, hmax, vmax)
        _same(planes[f], np.concatenate([p.reshape(-1) for p in want_planes]), f"{sampling}-{H}x{W} frame {f}", "planes")
        _same(pixels[f], want_pixels, f"{sampling}-{H}x{W} frame {f}", "pixels")


# ---------------------------------------------------------------------------------------------------- refusals

def _refused(call, d):
    from egohmr_amd import _lib
    rc = call(C.byref(d), _lib.stream_ptr())
    msg = _lib.lib().ehm_last_error().decode()
    assert rc == -22 and "bad argument" in msg, (rc, msg)


DECODE_REFUSALS = {
    "coef_off_16": lambda d: setattr(d, "coef", d.coef + 2),
    "quant_off_16": lambda d: setattr(d, "quant", d.quant + 2),
    "workspace_off_16": lambda d: setattr(d, "workspace", d.workspace + 8),
    "workspace_one_short": lambda d: setattr(d, "workspace_bytes", d.workspace_bytes - 1),
    "F_0": lambda d: setattr(d, "F", 0),
    "F_65536": lambda d: setattr(d, "F", 65536),
    "H_0": lambda d: setattr(d, "H", 0),
    "components_2": lambda d: setattr(d, "components", 2),
    "sampling_1x2": lambda d: (setattr(d, "hmax", 1), setattr(d, "vmax", 2)),
    "gray_hmax_2": lambda d: (setattr(d, "components", 1), setattr(d, "hmax", 2), setattr(d, "vmax", 1)),
}


@pytest.mark.parametrize("what", list(DECODE_REFUSALS))
def test_decode_refuses_bad_arguments_before_any_launch(dev, what):
    """Argument checks only: the host side answers -22 and nothing is launched, so no pointer given here is ever followed."""
    from egohmr_amd import _lib
    case = dict(cases.decode_cases())["420-17x17-dense"]
    coef, quant = torch.from_numpy(case["coef"]).to(dev), torch.from_numpy(case["quant"]).to(dev)
    ws, frames = Guarded(dev, coef.numel()), Guarded(dev, case["H"] * case["W"] * 3)
    d = decode_desc(case, coef, quant, frames.ptr, ws.ptr, coef.numel())
    DECODE_REFUSALS[what](d)
    _refused(_lib.lib().ehm_jpeg_decode, d)
    torch.cuda.synchronize()
    assert (ws.host() == 0xA5).all() and (frames.host() == 0xA5).all()


FORWARD_REFUSALS = {
    "coef_off_16": lambda d: setattr(d, "coef", d.coef + 2),
    "quant_odd": lambda d: setattr(d, "quant", d.quant + 1),
    "sampling_1x2": lambda d: (setattr(d, "hmax", 1), setattr(d, "vmax", 2)),
    "W_0": lambda d: setattr(d, "W", 0),
    "F_0": lambda d: setattr(d, "F", 0),
}


@pytest.mark.parametrize("what", list(FORWARD_REFUSALS))
def test_forward_refuses_bad_arguments_before_any_launch(dev, what):
    from egohmr_amd import _lib
    H, W, F = 17, 17, 1
    frames = torch.zeros(F, H, W, 3, dtype=torch.uint8, device=dev)
    quant = torch.ones(F, 3, 64, dtype=torch.int16, device=dev)
    coef = Guarded(dev, F * 2 * 64 * (4 * 4 + 2 * 2 * 2))
    d = _lib.JpegForwardDesc(frames=frames.data_ptr(), quant=quant.data_ptr(), H=H, W=W, hmax=2, vmax=2, F=F, rgb=0, coef=coef.ptr)
    FORWARD_REFUSALS[what](d)
    _refused(_lib.lib().ehm_jpeg_forward, d)
    torch.cuda.synchronize()
    assert (coef.host() == 0xA5).all()
