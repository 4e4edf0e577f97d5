"""CPU: what the synthetic JPEG case set (tests/jpeg_cases.py) claims, proved before tests/test_gpu_jpeg_kernels.py relies on it - every decode
case inside the domain where the header's int32 IDCT is exact, the geometries that reach each edge of the kernels present, both clamp sites
driven far out of range, every planted mistake of tests/jpeg_ref.py and tests/jpeg_enc_ref.py caught by at least one case - and the two
restatements once more against PIL, away from the fixture files.  The rule is integer: every bar is equality."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases as cases  # noqa: E402
import jpeg_enc_ref as enc_ref  # noqa: E402
import jpeg_ref  # noqa: E402
from make_jpeg_golden import FIXTURES  # noqa: E402


@pytest.fixture(scope="module")
def decode_wants():
    """{id: (planes, pixels, detail)} of the int64 evaluation - which raises for a case outside the exact domain"""
    out, excluded = {}, []
    for cid, case in cases.decode_cases():
        detail = []
        try:
            out[cid] = cases.decode_want(case, detail=detail) + (detail,)
        except jpeg_ref.JpegError as e:
            excluded.append(f"{cid}: {e}")
    print(f"{len(out)} decode cases inside the exact int32 domain, {len(excluded)} excluded")
    assert not excluded, excluded
    return out


@pytest.fixture(scope="module")
def forward_wants():
    return {cid: cases.forward_want(case) for cid, case in cases.forward_cases()}


def test_every_decode_case_is_inside_the_exact_domain(decode_wants):
    all_cases = cases.decode_cases()
    assert len(decode_wants) == len(all_cases) == len({cid for cid, _ in all_cases})
    for cid, case in all_cases:                                         # what an int32 machine computes is the same there
        planes, pixels = cases.decode_want(case, dtype=np.int32)
        assert np.array_equal(planes, decode_wants[cid][0]) and np.array_equal(pixels, decode_wants[cid][1]), cid


def test_the_range_check_refuses_what_leaves_int32():
    """The finding behind it: all 64 dequantised values at 2048 leave int32 in the second pass (every basis function is positive at sample
    (0, 0), so equal signs add up there), at 1024 they do not."""
    rng = np.random.default_rng(2048)
    ones = np.ones(64, np.uint16)
    same = np.ones((1, 1, 64), np.int16)
    for sign in [same, -same] + [rng.choice([-1, 1], (1, 1, 64)).astype(np.int16) for _ in range(200)]:
        jpeg_ref.idct_samples(1024 * sign, ones)                        # raises outside the domain
    for block, q in ((2048 * same, ones), (-2048 * same, ones), (1023 * same, np.full(64, 255, np.uint16))):   # (the last: legal in a baseline stream)
        with pytest.raises(jpeg_ref.JpegError, match="outside int32"):
            jpeg_ref.idct_samples(block, q)
        wrapped = jpeg_ref.idct_samples(block, q, dtype=np.int32)       # what silently happens without the check
        assert wrapped.dtype == np.int32 and wrapped.shape == (8, 8)


def test_case_ids_cover_what_they_claim():
    seen = {"422": set(), "420": set()}
    ch = set()
    for _, c in cases.decode_cases():
        if c["sampling"] in seen:
            seen[c["sampling"]].add(-(-c["W"] // c["hmax"]))
            if c["vmax"] == 2:                                          # (only 4:2:0 filters vertically: the above / below clamp)
                ch.add(-(-c["H"] // c["vmax"]))
    for s in seen:
        assert {1, 2, 3, 8, 9, 12, 13} <= seen[s], (s, sorted(seen[s]))
    assert {1, 2, 8, 9} <= ch
    for s in ("444", "gray"):
        assert any(c["sampling"] == s and c["W"] % 8 for _, c in cases.decode_cases()), s
    multi = [c for _, c in cases.decode_cases() if c["F"] > 1]
    assert {c["F"] for c in multi} == {2, 5} and len({(c["sampling"], c["H"], c["W"]) for c in multi}) == 4
    assert all(c["blocks"] % 32 for c in multi)                         # a workgroup of 32 blocks spans two frames
    assert any(c["blocks"] == 12 and c["sampling"] == "420" for c in multi)
    for cid, c in cases.decode_cases():
        grids = jpeg_ref.block_grids(c["H"], c["W"], c["components"], c["hmax"], c["vmax"])
        assert c["coef"].shape == (c["F"], 64 * sum(a * b for a, b in grids)) and c["coef"].dtype == np.int16, cid
        q = c["quant"].reshape(-1, 64)
        assert q.min() >= 1 and q.max() <= 255 and len({r.tobytes() for r in q}) == len(q), cid
        if c["content"] == "dense":
            rows = np.repeat(np.arange(c["components"]), [a * b for a, b in grids])        # the component of every block of a frame
            for f in range(c["F"]):
                deq = c["coef"][f].reshape(-1, 64).astype(np.int64) * c["quant"][f][rows]
                assert (deq != 0).all() and np.abs(deq).max() <= 512, cid
    fw = cases.forward_cases()
    assert {c["sampling"] for _, c in fw} == {"444", "422", "420"} and {c["F"] for _, c in fw} == {1, 3} and {c["rgb"] for _, c in fw} == {0, 1}
    assert {(c["sampling"], c["H"], c["W"]) for _, c in fw} == {g for g in cases.geometries() if g[0] != "gray"}
    for cid, c in fw:
        q = c["quant"].reshape(-1, 64)
        assert q.min() >= 1 and q.max() <= 255 and len({r.tobytes() for r in q}) == len(q), cid
    print(f"{len(cases.decode_cases())} decode cases, {len(fw)} forward cases")


def test_sparse_extreme_cases_reach_both_clamp_sites(decode_wants):
    """A kernel that wrapped instead of clamping beyond +-512 must not pass: the unclamped values go that far."""
    n = 0
    for cid, case in cases.decode_cases():
        if case["content"] != "sparse_extreme":
            continue
        n += 1
        for d in decode_wants[cid][2]:
            assert any(s.min() < 0 and s.max() > 255 for s in d["samples"]), cid
            assert min(s.min() for s in d["samples"]) < -512 and max(s.max() for s in d["samples"]) > 512 + 255, cid
            if case["components"] == 3:                                 # (a one-component frame's B G R are its clamped Y: no second clamp)
                assert all(s.min() < 0 and s.max() > 255 for s in d["samples"]), cid
                assert d["bgr"].min() < 0 and d["bgr"].max() > 255, cid
    assert n == len(cases.geometries()) + 2 * len(cases.MULTI)


@pytest.mark.parametrize("wrong", jpeg_ref.DECODE_WRONG)
def test_planted_decode_mistake_is_caught(decode_wants, wrong):
    hits = 0
    for cid, case in cases.decode_cases():
        # (int32, as a mistaken kernel would compute: another frame's table can take a sparse_extreme block out of the exact domain)
        planes, pixels = cases.decode_want(case, wrong=wrong, dtype=np.int32)
        hits += not (np.array_equal(planes, decode_wants[cid][0]) and np.array_equal(pixels, decode_wants[cid][1]))
    print(f"decode {wrong}: caught by {hits} of {len(decode_wants)} cases")
    assert hits > 0


@pytest.mark.parametrize("wrong", enc_ref.FORWARD_WRONG)
def test_planted_forward_mistake_is_caught(forward_wants, wrong):
    hits = sum(not np.array_equal(cases.forward_want(case, wrong=wrong), forward_wants[cid]) for cid, case in cases.forward_cases())
    print(f"forward {wrong}: caught by {hits} of {len(forward_wants)} cases")
    assert hits > 0


def test_the_table_mix_up_is_invisible_on_the_committed_files(golden_dir):
    """The hole of the suite as it was: on the committed files Cb and Cr share a table, and the mix-up changes nothing."""
    for name in FIXTURES:
        with open(os.path.join(golden_dir, "jpeg", name + ".jpg"), "rb") as f:
            p = jpeg_ref.parse(f.read())
        assert np.array_equal(jpeg_ref.pixels(p, wrong="cr_uses_cb_table"), jpeg_ref.pixels(p)), name


def test_forward_cases_round_trip_through_a_file():
    """A file carries two tables, and no forward case's rows repeat the chroma row (every row of a case is distinct).  So the tables are
    REBUILT here, not taken as they are: rows 0, 1, 1 of frame 0 of every fourth case, with entries of at least 2, which keep every
    coefficient of saturated content inside the Huffman tables' 10 bits."""
    n = 0
    for cid, case in cases.forward_cases()[::4]:
        q = np.maximum(case["quant"][0][[0, 1, 1]], 2)
        rgb = case["frames"][0]
        want = enc_ref.coefficients(rgb, q, case["hmax"], case["vmax"])
        assert np.array_equal(want, enc_ref.coefficients(rgb, q[:2], case["hmax"], case["vmax"])), cid
        p = jpeg_ref.parse(enc_ref.encode(rgb, q[:2], case["hmax"], case["vmax"]))
        assert (p.H, p.W, p.hmax, p.vmax) == (case["H"], case["W"], case["hmax"], case["vmax"]) and np.array_equal(p.coef, want), cid
        n += 1
    assert n > 100


def test_restatement_equals_pil_on_noise_and_saturated_frames():
    Image = pytest.importorskip("PIL.Image")
    from make_jpeg_golden import pil_decode_bgr
    sizes = [(1, 1), (3, 5), (8, 8), (9, 17), (15, 6), (17, 26), (32, 40)]
    files = 0
    for si, (mode, sub) in enumerate((("L", None), ("RGB", 0), ("RGB", 1), ("RGB", 2))):
        for zi, (H, W) in enumerate(sizes):
            for qi, quality in enumerate((1, 3, 10, 50, 95, 100)):
                if (si + zi + qi) % 3 == 0:                             # a third of the grid is left out: 112 files
                    continue
                rng = np.random.default_rng([H, W, quality, si])
                shape = (H, W) if mode == "L" else (H, W, 3)
                a = rng.integers(0, 256, shape, dtype=np.uint8) if (zi + qi) % 2 else (rng.integers(0, 2, shape) * 255).astype(np.uint8)
                buf = io.BytesIO()
                Image.fromarray(a).save(buf, "JPEG", quality=quality, **({} if sub is None else {"subsampling": sub}))
                data = buf.getvalue()
                assert np.array_equal(jpeg_ref.decode(data), pil_decode_bgr(data)), (mode, sub, H, W, quality)
                if mode == "RGB":                                       # and the encoder's restatement gives PIL's coefficients
                    hv = ((1, 1), (2, 1), (2, 2))[sub]
                    p = jpeg_ref.parse(data)
                    assert np.array_equal(enc_ref.coefficients(a, p.quant[:2], *hv), p.coef), (sub, H, W, quality)
                files += 1
    print(f"{files} files, difference 0")
    assert files >= 100
