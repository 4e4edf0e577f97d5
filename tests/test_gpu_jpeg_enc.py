"""GPU: the baseline-JPEG encoder (csrc/jpeg_enc.hip behind ehm_jpeg_forward / ehm_jpeg_entropy_encode, egohmr_amd.jpeg.JpegEncoder,
Stage2Driver.save_overlays) against the numpy restatement tests/jpeg_enc_ref.py and the bytes PIL wrote (tests/golden/jpeg_enc.npz).  The rule
is integer, so every bar is equality.  PIL is not needed here.  Every test fails without the feature: the entries do not exist on the parent."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_ref as enc_ref  # noqa: E402
import jpeg_ref  # noqa: E402
import make_jpeg_enc_golden as golden  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(golden.FIXTURES)
SAMPLING_NAME = {v: k for k, v in golden.SAMPLINGS.items()}
GUARD = 256


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return golden.load(os.path.join(golden_dir, "jpeg_enc.npz"))


@pytest.fixture(scope="module")
def parsed(fixtures):
    return {n: jpeg_ref.parse(fixtures[n][3]) for n in NAMES}


@pytest.fixture(scope="module")
def noise():
    """{name: (rgb, tables, file bytes of the restatement)} of the two scan-boundary frames, encoded once"""
    out = {}
    for name, (H, W) in (("136x264", (136, 264)), ("24x520", (24, 520))):
        rgb = np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        tables = enc_ref.quality_tables(95)
        out[name] = (rgb, tables, enc_ref.encode(rgb, tables, 2, 2))
    return out


def encoder(dev, hv, quality=95):
    from egohmr_amd import JpegEncoder
    return JpegEncoder(dev, quality=quality, subsampling=SAMPLING_NAME[hv])


def entropy_direct(dev, coef, H, W, hv, capacity):
    """ehm_jpeg_entropy_encode on its own buffers: -> (streams uint8 [F, capacity] numpy, lengths, needed, the guard bytes behind the streams)"""
    from egohmr_amd import _lib
    F = coef.shape[0]
    buf = torch.full((F * capacity + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    info = torch.full((2, F), -7, dtype=torch.int64, device=dev)
    d = _lib.JpegEntropyEncodeDesc(coef=_lib.ptr(coef), H=H, W=W, hmax=hv[0], vmax=hv[1], F=F, streams=buf.data_ptr(), capacity=capacity,
                                   lengths=info[0].data_ptr(), needed=info[1].data_ptr())
    need = C.c_int64(0)
    _lib.api().ehm_jpeg_entropy_encode_workspace_bytes(C.byref(d), C.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    d.workspace, d.workspace_bytes = _lib.ptr(ws), need.value
    _lib.api().ehm_jpeg_entropy_encode(C.byref(d), _lib.stream_ptr())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return host[:F * capacity].reshape(F, capacity), info[0].cpu().numpy(), info[1].cpu().numpy(), host[F * capacity:]


# ---------------------------------------------------------------------------------------------------- the forward stage

@pytest.mark.parametrize("name", NAMES)
def test_forward_equals_pils_coefficients(dev, fixtures, parsed, name):
    rgb, q, hv, _ = fixtures[name]
    enc = encoder(dev, hv, q)
    coef, quant = enc.coefficients(torch.from_numpy(rgb).to(dev), bgr=False)
    torch.cuda.synchronize()
    assert coef.dtype == torch.int16 and tuple(coef.shape) == (1, parsed[name].coef_count) and tuple(quant.shape) == (1, 3, 64)
    assert np.array_equal(quant[0].cpu().numpy(), parsed[name].quant[[0, 1, 1]])
    got = coef[0].cpu().numpy()
    assert np.array_equal(got, parsed[name].coef), f"{int((got != parsed[name].coef).sum())} coefficients differ"
    bgr, _ = enc.coefficients(torch.from_numpy(rgb[..., ::-1].copy()).to(dev), bgr=True)
    assert torch.equal(bgr, coef)


def test_forward_mixes_qualities_in_one_call(dev, fixtures):
    rgbs = [fixtures[n][0] for n in ("p24x40_420_q10", "noise24x40_420_q100")]
    frames = torch.from_numpy(np.stack([rgbs[0], rgbs[1], rgbs[0]])).to(dev)
    enc = encoder(dev, (2, 2))
    qualities = [10, 75, 100]
    together, quant = enc.coefficients(frames, bgr=False, quality=qualities)
    assert not torch.equal(quant[0], quant[1]) and not torch.equal(quant[1], quant[2])
    for f, q in enumerate(qualities):
        one, _ = enc.coefficients(frames[f:f + 1], bgr=False, quality=q)
        assert torch.equal(one[0], together[f])
        assert np.array_equal(together[f].cpu().numpy(), enc_ref.coefficients(frames[f].cpu().numpy(), enc_ref.quality_tables(q), 2, 2))


# ---------------------------------------------------------------------------------------------------- the entropy stage on hand-made coefficients

def _handmade():
    """{case: int16 [3, 3, 5, 64]}: one 4:4:4 frame of 3 x 5 blocks per plane (24 x 40 pixels)"""
    from egohmr_amd import _lib
    Z = jpeg_ref.ZIGZAG
    cases = {"zeros": np.zeros((3, 3, 5, 64), np.int16)}
    for k in (63, 17, 33):                                             # three, one and two ZRL codes in front of the coefficient
        c = np.zeros((3, 3, 5, 64), np.int16)
        c[..., Z[k]] = (np.arange(45).reshape(3, 3, 5) % 7) - 3        # zero in some blocks, so EOB-only blocks sit between them
        c[0, 1, 2, Z[k]] = 1
        cases[f"lone{k}"] = c
    c = np.zeros((3, 3, 5, 64), np.int16)
    c[..., 0] = np.where(np.arange(15).reshape(3, 5) % 2 == 0, 1023, -1023)       # every DC difference but the first is +-2046: size 11
    cases["dc1023"] = c
    c = np.zeros((3, 3, 5, 64), np.int16)
    c[..., 1:] = np.where(np.arange(63) % 2 == 0, 1023, -1023)
    c[1, :, :, 1:] *= -1
    cases["ac1023"] = c
    # FF bytes at the stuffing kernel's chunk boundaries: every AC +1023 packs into runs of nine and twelve 1 bits; the first block's DC size
    # shifts the whole stream bit by bit until the last byte of chunk 0 (then the first byte of chunk 1) is FF
    chunk = _lib.JPEG_ENC_STUFF_CHUNK
    for at in (chunk - 1, chunk):
        for dc in range(0, 1024):
            c = np.zeros((3, 3, 5, 64), np.int16)
            c[..., 1:] = 1023
            c[0, ..., 0] = dc                                            # (only the first luma difference is dc, the later ones stay zero)
            packed = enc_ref.packed_stream(list(c), 1, 1)
            if len(packed) > 2 * chunk and packed[at] == 0xFF:
                break
        else:
            raise AssertionError("no pattern puts FF at byte %d" % at)
        cases[f"ff_at_{at}"] = c
    return cases


@pytest.fixture(scope="module")
def handmade():
    return _handmade()


@pytest.mark.parametrize("case", ["zeros", "lone63", "lone17", "lone33", "dc1023", "ac1023", "ff_at_4095", "ff_at_4096"])
def test_entropy_stage_on_handmade_coefficients(dev, handmade, case):
    from egohmr_amd import _lib, jpeg
    assert _lib.JPEG_ENC_STUFF_CHUNK == 4096
    planes = handmade[case]
    want = enc_ref.scan_bytes(list(planes), 1, 1)
    flat = planes.reshape(1, -1)
    coef = torch.from_numpy(flat).to(dev)
    streams, lengths, needed, guard = entropy_direct(dev, coef, 24, 40, (1, 1), len(want) + 64)
    assert lengths[0] == len(want) and needed[0] == len(want)
    got = streams[0, :len(want)].tobytes()
    assert got == want, "first difference at byte %d of %d" % (next(i for i in range(len(want)) if got[i] != want[i]), len(want))
    assert (streams[0, len(want):] == 0xA5).all() and (guard == 0xA5).all()
    if case.startswith("ff_at"):
        packed = enc_ref.packed_stream(list(planes), 1, 1)
        assert packed[int(case[6:])] == 0xFF and len(packed) > 2 * _lib.JPEG_ENC_STUFF_CHUNK
    # and back through the decoder's host stage
    tables = jpeg.quality_tables(50)
    data = jpeg.file_header(24, 40, 1, 1, tables) + got + b"\xff\xd9"
    back = np.full(flat.size, 0x5A5A, np.int16)
    assert _lib.lib().ehm_jpeg_entropy_decode(data, len(data), None, back.ctypes.data, back.size) == 0, _lib.lib().ehm_last_error()
    assert np.array_equal(back, flat[0])


def test_entropy_stage_flags_a_coefficient_without_a_code(dev):
    c = np.zeros((2, 3, 3, 5, 64), np.int16)
    c[1, 0, 1, 1, 5] = 1024                                             # an AC of size 11: no code in a baseline table
    streams, lengths, needed, guard = entropy_direct(dev, torch.from_numpy(c.reshape(2, -1)).to(dev), 24, 40, (1, 1), 512)
    want = enc_ref.scan_bytes(list(c[0]), 1, 1)
    assert lengths.tolist() == [len(want), -2] and needed.tolist() == [len(want), 0]
    assert streams[0, :len(want)].tobytes() == want and (streams[1] == 0xA5).all() and (guard == 0xA5).all()


# ---------------------------------------------------------------------------------------------------- scan boundaries, the whole path

@pytest.mark.parametrize("name", ["136x264", "24x520"])
def test_noise_frames_across_the_scan_chunks(dev, noise, name):
    from egohmr_amd import _lib
    rgb, tables, want = noise[name]
    H, W = rgb.shape[:2]
    blocks = -(-H // 16) * -(-W // 16) * 6
    if name == "136x264":                                              # more than twice every per-launch chunk the scans walk
        assert blocks > 2 * _lib.JPEG_ENC_SCAN_CHUNK and len(enc_ref.scan_of(want)) > 2 * _lib.JPEG_ENC_STUFF_CHUNK
    else:
        assert -(-H // 16) == 2 and -(-W // 16) == 33                  # long MCU rows, a dummy luma row, a dummy luma column
    enc = encoder(dev, (2, 2), 95)
    got = enc.encode(torch.from_numpy(rgb).to(dev), bgr=False)
    assert len(got) == 1 and len(got[0]) == len(want)
    assert got[0] == want, "first difference at byte %d" % next(i for i in range(len(want)) if got[0][i] != want[i])


@pytest.mark.parametrize("name", NAMES)
def test_encode_equals_pil_and_decodes_to_the_same_pixels(dev, fixtures, name):
    from egohmr_amd import JpegDecoder
    rgb, q, hv, jpg = fixtures[name]
    enc = encoder(dev, hv, q)
    frames = torch.from_numpy(rgb).to(dev)
    a = enc.encode(frames, bgr=False)
    b = enc.encode(frames[None], bgr=False)
    assert a == b and len(a) == 1
    assert enc_ref.scan_of(a[0]) == enc_ref.scan_of(jpg)
    for marker, which in ((0xDB, 0), (0xDB, 1), (0xC0, 0)):
        assert enc_ref.segment(a[0], marker, which) == enc_ref.segment(jpg, marker, which)
    assert a[0] == jpg                                                  # the whole file, as it happens
    decoded = JpegDecoder(dev, threads=1).decode(a)
    assert np.array_equal(decoded[0].cpu().numpy(), jpeg_ref.decode(jpg))


def test_encode_batches_frames_and_writes_files(dev, fixtures, tmp_path):
    names = ("p24x40_420_q10", "noise24x40_420_q100")
    frames = torch.from_numpy(np.stack([fixtures[n][0] for n in names] + [fixtures[names[0]][0]])).to(dev)
    enc = encoder(dev, (2, 2))
    out = enc.encode(frames, bgr=False, quality=[10, 100, 10])
    assert out[0] == fixtures[names[0]][3] and out[1] == fixtures[names[1]][3] and out[2] == out[0]
    paths = enc.write(frames[:2], [tmp_path / "a.jpg", tmp_path / "b.jpg"], bgr=False, quality=[10, 100])
    assert [open(p, "rb").read() for p in paths] == out[:2]


# ---------------------------------------------------------------------------------------------------- capacity

def test_a_stream_buffer_one_byte_short_flags_only_that_frame(dev, fixtures, parsed):
    names = ("p24x40_420_q10", "noise24x40_420_q100", "p24x40_420_q10")
    coef = torch.from_numpy(np.stack([parsed[n].coef for n in names])).to(dev)
    want = [enc_ref.scan_of(fixtures[n][3]) for n in names]
    assert len(want[1]) > len(want[0])
    capacity = len(want[1]) - 1
    streams, lengths, needed, guard = entropy_direct(dev, coef, 24, 40, (2, 2), capacity)
    assert needed.tolist() == [len(w) for w in want] and lengths.tolist() == [len(want[0]), -1, len(want[2])]
    assert (guard == 0xA5).all() and (streams[1] == 0xA5).all()
    for f in (0, 2):
        assert streams[f, :len(want[f])].tobytes() == want[f] and (streams[f, len(want[f]):] == 0xA5).all()
    # exactly enough is enough
    streams, lengths, needed, guard = entropy_direct(dev, coef, 24, 40, (2, 2), capacity + 1)
    assert lengths.tolist() == [len(w) for w in want] and streams[1].tobytes() == want[1] and (guard == 0xA5).all()
    # capacity 0: every frame flagged, every size still exact, nothing written
    streams, lengths, needed, guard = entropy_direct(dev, coef, 24, 40, (2, 2), 0)
    assert lengths.tolist() == [-1, -1, -1] and needed.tolist() == [len(w) for w in want] and (guard == 0xA5).all()


def test_encode_recovers_by_one_rerun(dev, noise):
    rgb, _, want = noise["136x264"]
    enc = encoder(dev, (2, 2), 95)
    enc.bytes_per_pixel = 0.05                                          # a first buffer far too small for noise
    frames = torch.from_numpy(np.stack([rgb, rgb])).to(dev)
    assert enc.encode(frames, bgr=False) == [want, want] and enc.reruns == 1
    assert enc.encode(frames, bgr=False) == [want, want] and enc.reruns == 1     # the grown buffer is kept


# ---------------------------------------------------------------------------------------------------- the driver

def test_save_overlays_writes_the_contact_sheets(dev, tmp_path):
    from egohmr_amd import JpegDecoder
    from egohmr_amd.driver import Stage2Driver
    from egohmr_amd.render import contact_sheet
    rng = np.random.default_rng(626)
    smooth = lambda *shape: torch.from_numpy(np.clip(np.cumsum(rng.normal(0, 6, shape + (64, 96, 3)), -2) + 128, 0, 255).astype(np.uint8)).to(dev)
    images, in_scene, frames = smooth(2, 2), smooth(2, 2), smooth(3)
    drv = Stage2Driver(None, None, None, None, None)
    names = ["rec_a_frame_01.jpg", "rec_b_frame_02.jpg"]
    paths = drv.save_overlays(images, names, tmp_path / "vis", in_scene=in_scene, frames=frames, frame_index=[2, 0], quality=90)
    assert paths == [str(tmp_path / "vis" / n) for n in names] and all(os.path.getsize(p) > 700 for p in paths)
    got = JpegDecoder(dev, threads=1).decode(paths)
    assert tuple(got.shape) == (2, 64, 144, 3)
    tables = enc_ref.quality_tables(90)
    for i, fi in enumerate((2, 0)):
        sheet = contact_sheet(frames[fi], images[i], in_scene[i])
        assert tuple(sheet.shape) == (64, 144, 3)
        want = enc_ref.encode(sheet.cpu().numpy()[..., ::-1], tables, 2, 2)                    # the sheet is B G R
        assert open(paths[i], "rb").read() == want
        assert np.array_equal(got[i].cpu().numpy(), jpeg_ref.decode(want))
    # without the input frames and the in-scene views: one column
    only = drv.save_overlays(images[:1], ["only.jpg"], tmp_path / "vis")
    assert tuple(JpegDecoder(dev, threads=1).decode(only).shape) == (1, 64, 48, 3)
