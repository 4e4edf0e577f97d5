"""CPU: the host stage of the JPEG decoder (csrc/jpeg_entropy.h behind ehm_jpeg_read_header / ehm_jpeg_entropy_decode) against the numpy
restatement tests/jpeg_ref.py, and that restatement against the committed pixels (PIL's decode, tests/make_jpeg_golden.py) with difference 0.
Every bar here is equality: the rule is integer.  These tests fail on the parent commit, where the module and the symbols do not exist."""
import ctypes as C
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref  # noqa: E402
from make_jpeg_golden import BATCH, FIXTURES, PROGRESSIVE  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(FIXTURES)
CANARY = 64


def load(golden_dir, name):
    with open(os.path.join(golden_dir, "jpeg", name + ".jpg"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def pixels(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "jpeg_pixels.npz")))


@pytest.fixture(scope="module")
def parsed(golden_dir):
    """jpeg_ref.parse of every fixture, computed once"""
    return {n: jpeg_ref.parse(load(golden_dir, n)) for n in NAMES}


@pytest.fixture(scope="module")
def L():
    from egohmr_amd import _lib
    _lib.build()
    return _lib.lib()


def test_fixture_set_is_complete_and_small(golden_dir, pixels):
    files = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(golden_dir, "jpeg", "*.jpg")))
    assert files == sorted(NAMES + [PROGRESSIVE]) and sorted(pixels) == sorted(NAMES)
    size = sum(os.path.getsize(p) for p in glob.glob(os.path.join(golden_dir, "jpeg", "*.jpg"))) + os.path.getsize(os.path.join(golden_dir, "jpeg_pixels.npz"))
    assert size < 256 * 1024
    for n, (H, W, _, _) in FIXTURES.items():
        assert pixels[n].shape == (H, W, 3) and pixels[n].dtype == np.uint8


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_the_committed_pixels_and_pil(golden_dir, pixels, parsed, name):
    got = jpeg_ref.pixels(parsed[name])
    assert got.shape == pixels[name].shape
    assert int(np.abs(got.astype(np.int32) - pixels[name].astype(np.int32)).max()) == 0
    try:
        import PIL  # noqa: F401
    except ImportError:
        return
    from make_jpeg_golden import pil_decode_bgr
    assert np.array_equal(got, pil_decode_bgr(load(golden_dir, name)))


def test_fixtures_cover_what_they_are_named_for(parsed):
    geo = {n: (p.components, p.hmax, p.vmax, p.restart_interval) for n, p in parsed.items()}
    assert geo["p33x50_422"] == (3, 2, 1, 0) and geo["p24x40_444"] == (3, 1, 1, 0) and geo["p40x40_gray"] == (1, 1, 1, 0)
    assert geo["p37x53_420_rst3"] == (3, 2, 2, 3) and geo["p17x9_420"] == (3, 2, 2, 0)
    assert parsed["p24x520_420"].mcus_x == 33 and parsed["p56x72_420"].mcus_y == 4 and 56 % 16 == 8
    assert not np.array_equal(parsed["batch48x64_q50"].quant, parsed["batch48x64_q98"].quant)


def _header_fields(h):
    nc = h.components
    return dict(H=h.H, W=h.W, components=nc, hmax=h.hmax, vmax=h.vmax, mcus_x=h.mcus_x, mcus_y=h.mcus_y, restart_interval=h.restart_interval,
                h=list(h.h)[:nc], v=list(h.v)[:nc], blocks_x=list(h.blocks_x)[:nc], blocks_y=list(h.blocks_y)[:nc], quant_id=list(h.quant_id)[:nc],
                coef_count=h.coef_count)


@pytest.mark.parametrize("name", NAMES)
def test_header_and_coefficients_equal_the_reference(L, golden_dir, parsed, name):
    from egohmr_amd import _lib
    data, ref = load(golden_dir, name), parsed[name]
    want = {k: getattr(ref, k) for k in _header_fields(ref)}
    h = _lib.JpegHeader()
    assert L.ehm_jpeg_read_header(data, len(data), C.byref(h)) == 0
    assert _header_fields(h) == want
    assert np.array_equal(np.ctypeslib.as_array(h.quant), ref.quant)
    coef = np.full(ref.coef_count + CANARY, 0x5A5A, np.int16)
    h2 = _lib.JpegHeader()
    assert L.ehm_jpeg_entropy_decode(data, len(data), C.byref(h2), coef.ctypes.data, ref.coef_count) == 0
    assert _header_fields(h2) == want and np.array_equal(np.ctypeslib.as_array(h2.quant), ref.quant)
    assert np.array_equal(coef[:ref.coef_count], ref.coef)
    assert (coef[ref.coef_count:] == 0x5A5A).all()
    # a capacity one element too small is refused, and nothing is written past it
    coef[:] = 0x5A5A
    assert L.ehm_jpeg_entropy_decode(data, len(data), None, coef.ctypes.data, ref.coef_count - 1) == -22
    assert b"capacity" in L.ehm_last_error() and (coef == 0x5A5A).all()


def _refused(L, data, capacity=1 << 16):
    from egohmr_amd import _lib
    coef = np.full(capacity + CANARY, 0x5A5A, np.int16)
    h = _lib.JpegHeader()
    rc = L.ehm_jpeg_entropy_decode(data, len(data), C.byref(h), coef.ctypes.data, capacity)
    msg = L.ehm_last_error()
    assert (coef[capacity:] == 0x5A5A).all(), "the canary behind the coefficient buffer was written"
    return rc, msg


def _segment(data, marker):
    """(start, end) of the first segment with this marker byte, the FF xx included"""
    pos = 2
    while data[pos + 1] != marker:
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    return pos, pos + 2 + ((data[pos + 2] << 8) | data[pos + 3])


def test_progressive_and_random_bytes_are_refused(L, golden_dir):
    from egohmr_amd import _lib
    data = load(golden_dir, PROGRESSIVE)
    rc, msg = _refused(L, data)
    assert rc == -22 and b"progressive" in msg
    h = _lib.JpegHeader()
    assert L.ehm_jpeg_read_header(data, len(data), C.byref(h)) == -22 and b"progressive" in L.ehm_last_error()
    rng = np.random.default_rng(7)
    for n in (0, 1, 2, 3, 64, 4096):
        junk = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        rc, msg = _refused(L, junk)
        assert rc == -22 and len(msg) > 0, n
        rc, msg = _refused(L, b"\xff\xd8" + junk)
        assert rc == -22 and len(msg) > 0, n
    assert L.ehm_jpeg_read_header(None, 0, C.byref(h)) == -22 and L.ehm_jpeg_entropy_decode(b"", 0, None, None, 0) == -22


@pytest.mark.parametrize("name", NAMES)
def test_every_cut_of_a_fixture_is_refused(L, golden_dir, name):
    data = load(golden_dir, name)
    dqt, dht, sos = _segment(data, 0xDB), _segment(data, 0xC4), _segment(data, 0xDA)
    scan = len(data) - sos[1]
    cuts = sorted({2, 3, dqt[0] + 3, dqt[0] + 20, dqt[1] - 1, dht[0] + 5, dht[1] - 2, sos[0] + 1, sos[1], sos[1] + 1, sos[1] + scan // 3,
                   sos[1] + scan // 2, len(data) - 3, len(data) - 2, len(data) - 1})
    assert len(cuts) >= 12 and all(0 < c < len(data) for c in cuts)
    for c in cuts:
        rc, msg = _refused(L, data[:c])
        assert rc == -22 and len(msg) > 0, (name, c)
    # the first Huffman-table segment removed: the scan names a table that was never defined (or, with several tables in one segment, none is)
    rc, msg = _refused(L, data[:dht[0]] + data[dht[1]:])
    assert rc == -22 and len(msg) > 0


def test_unsupported_variants_are_refused(L, golden_dir):
    data = bytearray(load(golden_dir, "p24x40_444"))
    sof = _segment(data, 0xC0)[0]
    for off, value, text in ((4, 12, b"8-bit"),              # precision
                             (9, 4, b"component"),           # component count
                             (11, 0x12, b"sampling"),        # luma 1x2
                             (1, 0xC9, b"arithmetic")):      # the marker itself
        bad = bytearray(data)
        bad[sof + off] = value
        rc, msg = _refused(L, bytes(bad))
        assert rc == -22 and text in msg, (off, msg)


def test_decoder_entropy_threads_equal_one_by_one(golden_dir, parsed):
    from egohmr_amd import EgoHMRHipError, JpegDecoder
    datas = [load(golden_dir, n) for n in BATCH]
    dec = JpegDecoder("cpu", threads=4)
    assert JpegDecoder("cpu", threads=0).threads == 1 and JpegDecoder("cpu", threads=99).threads == 16
    headers, coef = dec.entropy(datas)
    assert tuple(coef.shape) == (3, parsed[BATCH[0]].coef_count) and coef.dtype.is_floating_point is False
    together = coef.numpy().copy()
    for i, d in enumerate(datas):
        h1, c1 = dec.entropy([d])
        assert np.array_equal(c1.numpy()[0], together[i]) and np.array_equal(together[i], parsed[BATCH[i]].coef)
        assert _header_fields(h1[0]) == _header_fields(headers[i])
    q = JpegDecoder.quant_rows(headers)
    for i, n in enumerate(BATCH):
        assert np.array_equal(q[i], parsed[n].quant[parsed[n].quant_id])
    # paths work like bytes; mixed geometries and refused files raise with the item's index
    paths = [os.path.join(golden_dir, "jpeg", n + ".jpg") for n in BATCH]
    assert np.array_equal(dec.entropy(paths)[1].numpy(), together)
    with pytest.raises(ValueError, match=r"48x64.*item 1 is 56x72"):
        dec.entropy([datas[0], load(golden_dir, "p56x72_420")])
    with pytest.raises(EgoHMRHipError, match=r"item 2 .*progressive"):
        dec.entropy([datas[0], datas[1], load(golden_dir, PROGRESSIVE)])
    with pytest.raises(EgoHMRHipError, match=r"item 1 "):
        dec.entropy([datas[0], datas[1][:-1]])
    with pytest.raises(EgoHMRHipError, match="HIP"):
        dec.decode(datas)
    dec.close()


def test_cabi_mirrors_and_source_list(L):
    from egohmr_amd import _lib
    header = open(os.path.join(REPO, "include", "egohmr_hip.h")).read()
    for name, nargs in (("ehm_jpeg_read_header", 3), ("ehm_jpeg_entropy_decode", 5), ("ehm_jpeg_workspace_bytes", 2), ("ehm_jpeg_decode", 2)):
        assert name + "(" in header and hasattr(L, name) and name not in _lib.VALUE_FUNCTIONS
        assert _lib.PROTOTYPES[name][0] is C.c_int and len(_lib.PROTOTYPES[name][1]) == nargs
    assert "jpeg.hip" in _lib.SOURCES
    # argument checks of the device entries run before any device call
    d = _lib.JpegDecodeDesc(H=56, W=72, components=3, hmax=2, vmax=2, F=2)
    need = C.c_int64(0)
    assert L.ehm_jpeg_workspace_bytes(C.byref(d), C.byref(need)) == 0 and need.value == 2 * 64 * (10 * 8 + 2 * 5 * 4)
    assert L.ehm_jpeg_decode(C.byref(d), None) == -22 and b"bad argument" in L.ehm_last_error()
    d.hmax, d.vmax = 1, 2
    assert L.ehm_jpeg_workspace_bytes(C.byref(d), C.byref(need)) == -22


def test_header_struct_matches_its_mirror(tmp_path):
    """sizeof / offsetof of ehm_jpeg_header and ehm_jpeg_decode_desc as a C99 compiler lays them out"""
    from egohmr_amd import _lib
    src = tmp_path / "sizes.c"
    src.write_text('#include "egohmr_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                   '  printf("%d %d %d %d %d\\n", (int)sizeof(ehm_jpeg_header), (int)offsetof(ehm_jpeg_header, quant), (int)offsetof(ehm_jpeg_header, coef_count),\n'
                   '         (int)sizeof(ehm_jpeg_decode_desc), (int)offsetof(ehm_jpeg_decode_desc, workspace_bytes));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    H, D = _lib.JpegHeader, _lib.JpegDecodeDesc
    assert got == [C.sizeof(H), H.quant.offset, H.coef_count.offset, C.sizeof(D), D.workspace_bytes.offset]


def test_sanitized_stand_alone_check(golden_dir, tmp_path):
    """tools/jpeg_entropy_check.cpp under AddressSanitizer + UBSan: a plain host binary (nothing loaded into Python), every fixture, every prefix,
    20 000 seeded single-byte mutations; exit 0 and no sanitizer report."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tools/jpeg_entropy_check.cpp"
    exe = tmp_path / "jpeg_entropy_check"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(REPO, "egohmr_amd", "csrc"), os.path.join(REPO, "tools", "jpeg_entropy_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)] + sorted(glob.glob(os.path.join(golden_dir, "jpeg", "*.jpg"))), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "20000 mutations" in run.stdout
