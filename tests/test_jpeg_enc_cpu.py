"""CPU: the baseline-JPEG encoding rule.  The numpy restatement tests/jpeg_enc_ref.py against the bytes PIL wrote (tests/golden/jpeg_enc.npz,
tests/make_jpeg_enc_golden.py): quantised coefficients, the entropy-coded segment, the tables.  Then the encoder's host entries
(csrc/jpeg_enc.h behind ehm_jpeg_quality_tables / ehm_jpeg_write_header), its refusals with no GPU present, the ctypes mirrors, contact_sheet,
and a sanitizer-built stand-alone program.  Every bar is equality: the rule is integer.  All but the first three tests fail on the parent
commit, where the entries, JpegEncoder and contact_sheet do not exist."""
import ctypes as C
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_ref as enc_ref  # noqa: E402
import jpeg_ref  # noqa: E402
import make_jpeg_enc_golden as golden  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(golden.FIXTURES)
CANARY = 64


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return golden.load(os.path.join(golden_dir, "jpeg_enc.npz"))


@pytest.fixture(scope="module")
def parsed(fixtures):
    """jpeg_ref.parse of PIL's bytes, computed once"""
    return {n: jpeg_ref.parse(fixtures[n][3]) for n in NAMES}


@pytest.fixture(scope="module")
def L():
    from egohmr_amd import _lib
    _lib.build()
    return _lib.lib()


def test_fixture_set_is_the_issues_and_small(golden_dir, fixtures, parsed):
    assert os.path.getsize(os.path.join(golden_dir, "jpeg_enc.npz")) < 256 * 1024
    want = {(5, 3, 2, 2), (8, 8, 2, 2), (24, 40, 2, 2), (41, 67, 2, 2), (9, 4, 2, 1), (33, 50, 2, 1), (24, 40, 1, 1)}
    have = {(rgb.shape[0], rgb.shape[1], h, v) for rgb, _, (h, v), _ in fixtures.values()}
    assert want <= have and {10, 75, 95, 100} <= {q for _, q, _, _ in fixtures.values()}
    for n, (rgb, q, (h, v), _) in fixtures.items():
        H, W, sampling, quality, _ = golden.FIXTURES[n]
        assert rgb.shape == (H, W, 3) and rgb.dtype == np.uint8 and q == quality and (h, v) == golden.SAMPLINGS[sampling]
        assert (parsed[n].H, parsed[n].W, parsed[n].hmax, parsed[n].vmax) == (H, W, h, v)
    # what the fixtures are named for: dummy luma rows / columns, FF bytes, EOB-only blocks
    rows_cols = lambda n: (parsed[n].blocks_y[0] - -(-parsed[n].H // 8), parsed[n].blocks_x[0] - -(-parsed[n].W // 8))
    assert rows_cols("p8x8_420_q95") == (1, 1) and parsed["p8x8_420_q95"].mcus_x * parsed["p8x8_420_q95"].mcus_y == 1
    assert rows_cols("p24x40_420_q10") == (1, 1) and rows_cols("p41x67_420_q75") == (0, 1)
    assert enc_ref.scan_of(fixtures["noise24x40_420_q100"][3]).count(b"\xff\x00") >= 5
    flat = parsed["flat16x24_420_q75"].coef.reshape(-1, 64)
    assert not flat[:, 1:].any()


@pytest.mark.parametrize("name", NAMES)
def test_reference_coefficients_and_stream_equal_pil(fixtures, parsed, name):
    rgb, q, (h, v), jpg = fixtures[name]
    tables = enc_ref.quality_tables(q)
    assert np.array_equal(tables, parsed[name].quant[:2])
    coef = enc_ref.coefficients(rgb, tables, h, v)
    assert coef.dtype == np.int16 and np.array_equal(coef, parsed[name].coef)
    planes = enc_ref.split_planes(parsed[name].coef, rgb.shape[0], rgb.shape[1], h, v)
    assert enc_ref.scan_bytes(planes, h, v) == enc_ref.scan_of(jpg)
    assert enc_ref.encode(rgb, tables, h, v) == jpg                       # welcome, not required: the whole file is PIL's


def test_reference_equals_pil_on_a_seeded_grid():
    try:
        import PIL  # noqa: F401
    except ImportError:                                                # the committed fixtures above carry the comparison without PIL
        return
    rng = np.random.default_rng(28)
    for H, W in ((5, 3), (8, 8), (9, 4), (16, 16), (17, 9), (24, 40), (33, 50), (41, 67), (56, 72), (23, 130)):
        for si, sampling in enumerate(golden.SAMPLINGS):
            for qi, q in enumerate((10, 50, 75, 95, 100)):
                kind = (H + W + si + qi) % 3
                if kind == 0:
                    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
                elif kind == 1:
                    rgb = np.broadcast_to(((np.arange(W) * 255) // max(W - 1, 1)).astype(np.uint8)[None, :, None], (H, W, 3)).copy()
                    rgb[..., 1] = ((np.arange(H) * 255) // max(H - 1, 1)).astype(np.uint8)[:, None]
                else:
                    rgb = golden.image(int(rng.integers(1 << 30)), H, W, "RGB")
                h, v = golden.SAMPLINGS[sampling]
                pil = golden.pil_encode(rgb, q, sampling)
                tables = enc_ref.quality_tables(q)
                assert np.array_equal(enc_ref.coefficients(rgb, tables, h, v), jpeg_ref.parse(pil).coef), (H, W, sampling, q)
                if (si + qi) % 3 == 0:
                    assert enc_ref.encode(rgb, tables, h, v) == pil, (H, W, sampling, q)


def test_quality_tables_equal_pils_dqt(L):
    from egohmr_amd import jpeg
    pil_tables = {}
    try:
        from PIL import Image
        for q in (1, 10, 49, 50, 75, 95, 100):
            buf = io.BytesIO()
            Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(buf, "JPEG", quality=q)
            pil_tables[q] = jpeg_ref.parse(buf.getvalue()).quant[:2]
    except ImportError:
        pass
    for q in (1, 10, 49, 50, 75, 95, 100):
        got = jpeg.quality_tables(q)
        assert got.shape == (2, 64) and got.dtype == np.uint16 and np.array_equal(got, enc_ref.quality_tables(q))
        if q in pil_tables:
            assert np.array_equal(got, pil_tables[q]), q


@pytest.mark.parametrize("name", NAMES)
def test_written_header_with_the_stream_is_a_file_every_reader_accepts(L, fixtures, parsed, name):
    from egohmr_amd import _lib, jpeg
    rgb, q, (h, v), jpg = fixtures[name]
    H, W = rgb.shape[:2]
    tables = jpeg.quality_tables(q)
    head = jpeg.file_header(H, W, h, v, tables)
    assert len(head) == _lib.JPEG_ENC_HEADER_BYTES and head == enc_ref.header(H, W, h, v, tables)
    for marker in (0xE0, 0xC0, 0xDA):
        assert enc_ref.segment(head, marker) == enc_ref.segment(jpg, marker)
    for k in range(2):
        assert enc_ref.segment(head, 0xDB, k) == enc_ref.segment(jpg, 0xDB, k)
    for k in range(4):                                                 # the typed-in Annex K tables are the ones PIL carries
        assert enc_ref.segment(head, 0xC4, k) == enc_ref.segment(jpg, 0xC4, k)
    data = head + enc_ref.scan_bytes(enc_ref.coefficient_planes(rgb, tables, h, v), h, v) + b"\xff\xd9"
    p = jpeg_ref.parse(data)
    assert np.array_equal(p.coef, parsed[name].coef)
    hdr = _lib.JpegHeader()
    assert L.ehm_jpeg_read_header(data, len(data), C.byref(hdr)) == 0
    assert (hdr.H, hdr.W, hdr.components, hdr.hmax, hdr.vmax, hdr.restart_interval) == (H, W, 3, h, v, 0)
    assert list(hdr.quant_id) == [0, 1, 1] and np.array_equal(np.ctypeslib.as_array(hdr.quant)[:2], tables)
    try:
        from make_jpeg_golden import pil_decode_bgr
        import PIL  # noqa: F401
    except ImportError:
        return
    assert np.array_equal(pil_decode_bgr(data), jpeg_ref.decode(data))


def test_mirrors_match_a_c99_compile(tmp_path):
    from egohmr_amd import _lib
    src = tmp_path / "sizes.c"
    src.write_text('#include "egohmr_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                   '  printf("%d %d %d %d %d %d %d\\n", (int)sizeof(ehm_jpeg_forward_desc), (int)offsetof(ehm_jpeg_forward_desc, rgb),\n'
                   '         (int)offsetof(ehm_jpeg_forward_desc, coef), (int)sizeof(ehm_jpeg_entropy_encode_desc),\n'
                   '         (int)offsetof(ehm_jpeg_entropy_encode_desc, streams), (int)offsetof(ehm_jpeg_entropy_encode_desc, needed),\n'
                   '         (int)offsetof(ehm_jpeg_entropy_encode_desc, workspace_bytes));\n'
                   '  printf("%d %d %d %d\\n", EHM_JPEG_ENC_HEADER_BYTES, EHM_JPEG_ENC_SCAN_CHUNK, EHM_JPEG_ENC_STUFF_CHUNK, EHM_JPEG_ENC_MAX_BLOCK_BYTES);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    Fd, Ed = _lib.JpegForwardDesc, _lib.JpegEntropyEncodeDesc
    assert got[:7] == [C.sizeof(Fd), Fd.rgb.offset, Fd.coef.offset, C.sizeof(Ed), Ed.streams.offset, Ed.needed.offset, Ed.workspace_bytes.offset]
    assert got[7:] == [_lib.JPEG_ENC_HEADER_BYTES, _lib.JPEG_ENC_SCAN_CHUNK, _lib.JPEG_ENC_STUFF_CHUNK, _lib.JPEG_ENC_MAX_BLOCK_BYTES]


def test_cabi_prototypes_and_source_list(L):
    from egohmr_amd import JpegEncoder, _lib  # noqa: F401
    header = open(os.path.join(REPO, "include", "egohmr_hip.h")).read()
    for name, nargs in (("ehm_jpeg_quality_tables", 2), ("ehm_jpeg_write_header", 8), ("ehm_jpeg_forward", 2),
                        ("ehm_jpeg_entropy_encode_workspace_bytes", 2), ("ehm_jpeg_entropy_encode", 2)):
        assert name + "(" in header and hasattr(L, name) and name not in _lib.VALUE_FUNCTIONS
        assert _lib.PROTOTYPES[name][0] is C.c_int and len(_lib.PROTOTYPES[name][1]) == nargs
    assert "jpeg_enc.hip" in _lib.SOURCES


def test_every_refusal_is_minus_22_without_a_gpu(L):
    from egohmr_amd import _lib
    q = np.ascontiguousarray(enc_ref.quality_tables(75))
    out = np.full(_lib.JPEG_ENC_HEADER_BYTES + CANARY, 0xA5, np.uint8)
    n = C.c_int64(-1)
    header = lambda H=16, W=16, h=2, v=2, quant=q.ctypes.data, o=out.ctypes.data, cap=_lib.JPEG_ENC_HEADER_BYTES, np_=C.byref(n): \
        L.ehm_jpeg_write_header(H, W, h, v, quant, o, cap, np_)
    assert header() == 0 and n.value == _lib.JPEG_ENC_HEADER_BYTES and (out[_lib.JPEG_ENC_HEADER_BYTES:] == 0xA5).all()
    out[:] = 0xA5
    for kw, text in ((dict(h=1, v=2), b"sampling"), (dict(h=4, v=1), b"sampling"), (dict(h=0, v=0), b"sampling"), (dict(H=0), b"height"),
                     (dict(W=65536), b"height"), (dict(quant=None), b"null"), (dict(o=None), b"null"), (dict(np_=None), b"null"),
                     (dict(cap=_lib.JPEG_ENC_HEADER_BYTES - 1), b"capacity"), (dict(cap=0), b"capacity")):
        assert header(**kw) == -22 and text in L.ehm_last_error(), kw
        assert (out == 0xA5).all(), kw
    zero = q.copy()
    zero[1, 17] = 0
    assert header(quant=zero.ctypes.data) == -22 and b"quantisation" in L.ehm_last_error() and n.value == 0
    big = q.copy()
    big[0, 3] = 256
    assert header(quant=big.ctypes.data) == -22 and b"quantisation" in L.ehm_last_error()
    for quality in (0, -5, 101):
        assert L.ehm_jpeg_quality_tables(quality, q.ctypes.data) == -22 and b"quality" in L.ehm_last_error()
    assert L.ehm_jpeg_quality_tables(75, None) == -22
    # the device entries: every check comes before the first device call, so it runs (and refuses) with no GPU
    fake = 0x10000                                                     # an aligned address that is never dereferenced
    fwd = lambda **kw: _lib.JpegForwardDesc(**{**dict(frames=fake, quant=fake, coef=fake, H=16, W=16, hmax=2, vmax=2, F=1, rgb=0), **kw})
    for kw in (dict(hmax=1, vmax=2), dict(hmax=3, vmax=1), dict(F=65536), dict(F=0), dict(frames=None), dict(quant=None), dict(coef=None),
               dict(coef=fake + 8), dict(H=0), dict(W=70000)):
        assert L.ehm_jpeg_forward(C.byref(fwd(**kw)), None) == -22 and b"bad argument" in L.ehm_last_error(), kw
    assert L.ehm_jpeg_forward(None, None) == -22
    base = dict(coef=fake, H=16, W=16, hmax=2, vmax=2, F=2, streams=fake, capacity=100, lengths=fake, needed=fake, workspace=fake)
    need = C.c_int64(0)
    assert L.ehm_jpeg_entropy_encode_workspace_bytes(C.byref(_lib.JpegEntropyEncodeDesc(**base)), C.byref(need)) == 0
    assert need.value >= 2 * 6 * _lib.JPEG_ENC_MAX_BLOCK_BYTES and need.value % 16 == 0
    ent = lambda **kw: _lib.JpegEntropyEncodeDesc(**{**base, "workspace_bytes": need.value, **kw})
    for kw in (dict(hmax=1, vmax=2), dict(F=65536), dict(coef=None), dict(streams=None), dict(lengths=None), dict(needed=None), dict(workspace=None),
               dict(coef=fake + 2), dict(workspace=fake + 4), dict(lengths=fake + 4), dict(needed=fake + 1), dict(workspace_bytes=need.value - 1),
               dict(capacity=-1)):
        assert L.ehm_jpeg_entropy_encode(C.byref(ent(**kw)), None) == -22 and b"bad argument" in L.ehm_last_error(), kw
    assert L.ehm_jpeg_entropy_encode_workspace_bytes(C.byref(ent(hmax=2, vmax=4)), C.byref(need)) == -22
    assert L.ehm_jpeg_entropy_encode_workspace_bytes(C.byref(ent(F=65536)), C.byref(need)) == -22


def test_encoder_without_a_device_raises_and_checks_its_arguments():
    from egohmr_amd import EgoHMRHipError, JpegEncoder
    enc = JpegEncoder("cpu", quality=75)
    with pytest.raises(EgoHMRHipError, match="HIP"):
        enc.encode(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="subsampling"):
        JpegEncoder("cpu", subsampling="4:1:1")
    with pytest.raises(EgoHMRHipError, match="quality"):
        enc._tables(1, 101)
    with pytest.raises(ValueError, match="2 qualities for 3"):
        enc._tables(3, [50, 60])
    assert [t[0][0] for t in enc._tables(2, [50, 100])] == [16, 1]


@pytest.mark.parametrize("S,H,W", [(2, 6, 10), (1, 7, 9), (3, 7, 9)])
def test_contact_sheet_equals_a_numpy_loop(S, H, W):
    from egohmr_amd.render import contact_sheet
    rng = np.random.default_rng(S * 100 + H)
    a, b, c = (rng.integers(0, 256, (S, H, W, 3), dtype=np.uint8) for _ in range(3))
    for parts in ((a, b, c), (a, b), (None, b, c)):
        cols = [p for p in parts if p is not None]
        full = np.concatenate(cols, 2).reshape(S * H, len(cols) * W, 3).astype(np.int64)
        want = np.zeros((S * H // 2, len(cols) * W // 2, 3), np.uint8)
        for y in range(want.shape[0]):
            for x in range(want.shape[1]):
                want[y, x] = (full[2 * y, 2 * x] + full[2 * y, 2 * x + 1] + full[2 * y + 1, 2 * x] + full[2 * y + 1, 2 * x + 1] + 2) >> 2
        t = [None if p is None else torch.from_numpy(p) for p in parts]
        got = contact_sheet(t[0], t[1], t[2] if len(t) > 2 else None)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and np.array_equal(got.numpy(), want)
        assert np.array_equal(contact_sheet(t[0], t[1], t[2] if len(t) > 2 else None, halve=False).numpy(), full.astype(np.uint8))
    assert np.array_equal(contact_sheet(torch.from_numpy(a[0]), torch.from_numpy(b)).numpy(),
                          contact_sheet(torch.from_numpy(np.repeat(a[:1], S, 0)), torch.from_numpy(b)).numpy())
    with pytest.raises(ValueError, match="uint8"):
        contact_sheet(torch.from_numpy(a).float(), torch.from_numpy(b))


def test_sanitized_stand_alone_header_check(tmp_path):
    """tools/jpeg_header_check.cpp under AddressSanitizer + UBSan: a plain host binary (nothing loaded into Python).  Every size 1..40 x 1..40,
    the three samplings, every capacity from 0 to the needed size, every quality; exit 0 and no sanitizer report."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tools/jpeg_header_check.cpp"
    exe = tmp_path / "jpeg_header_check"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(REPO, "egohmr_amd", "csrc"), os.path.join(REPO, "tools", "jpeg_header_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "4800 geometries" in run.stdout
