"""CPU: the host half of egohmr_amd.batch against the reference loader's own results (tests/golden/g23_batch_*.npz, written by
tests/make_batch_golden.py from dataloaders/augmentation.py:get_example), the numpy restatements of the two kernels' rules (imported by
tests/test_gpu_batch.py and by the golden generator's cv2 stand-in), and the argument validation of the two C entries.

Bars.  Flags, permutations, box_center, box_size, cam_cx, the visibility mask and every value that does not pass through the affine solve, the
rotation matrix M or Rodrigues: bit equality.  What does: at most 1 float32 ulp - two float64 solves of the same 3-point system differ in their
last bits and the float32 cast can then fall either side.  The golden `img` was evaluated by numpy >= 2, whose `(p - mean) / std` runs in
float64 where the reference's numpy 1.22 stays in float32 (mean, std are float64 scalars: value-based casting); with p <= 306 the two differ
by at most (ulp32(123) + ulp32(255)) / 57 plus one final rounding, about 2.6e-7: the bar is 2^-21."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from egohmr_amd import batch as eb

CASES = ("noaug", "flip_rot", "rotmiss_noflip", "border")
IMG_BAR = 2.0 ** -21
TIE_MARGIN = 1e-9


# ------------------------------------------------------------------------------------------------ restatements (also used by test_gpu_batch)
def invert_affine_ref(trans):
    """The map warpAffine applies (patch pixel -> source pixel) for a 2x3 `trans`: cv2's closed-form inverse, float64."""
    M = np.array(trans, np.float64)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1. / D if D != 0 else 0.
    A11, A22 = M[1, 1] * D, M[0, 0] * D
    M[0, 0] = A11
    M[0, 1] *= -D
    M[1, 0] *= -D
    M[1, 1] = A22
    b1 = -M[0, 0] * M[0, 2] - M[0, 1] * M[1, 2]
    b2 = -M[1, 0] * M[0, 2] - M[1, 1] * M[1, 2]
    M[0, 2], M[1, 2] = b1, b2
    return M


def bilinear_f64(img, Minv, P, flip=False):
    """The real-valued bilinear rule of include/egohmr_hip.h for one frame: img uint8 [H,W,3]; output pixel (x, y) samples
    (sx, sy) = Minv (x, y, 1) of the (mirrored, with `flip`) frame; a neighbour outside the frame is 0.  -> float64 [P,P,3]."""
    H, W = img.shape[:2]
    Minv = np.asarray(Minv, np.float64)
    ys, xs = np.meshgrid(np.arange(P, dtype=np.float64), np.arange(P, dtype=np.float64), indexing="ij")
    sx = (Minv[0, 0] * xs + Minv[0, 1] * ys) + Minv[0, 2]
    sy = (Minv[1, 0] * xs + Minv[1, 1] * ys) + Minv[1, 2]
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    src = img[:, ::-1, :] if flip else img

    def at(xi, yi):
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        xc, yc = np.clip(xi, 0, W - 1).astype(np.int64), np.clip(yi, 0, H - 1).astype(np.int64)
        return np.where(ok[..., None], src[yc, xc, :].astype(np.float64), 0.0)

    a, b, c, d = at(x0, y0), at(x0 + 1, y0), at(x0, y0 + 1), at(x0 + 1, y0 + 1)
    gx, gy, fx, fy = (1.0 - fx)[..., None], (1.0 - fy)[..., None], fx[..., None], fy[..., None]
    return (a * gx + b * fx) * gy + (c * gx + d * fx) * fy


def tie_distance(v):
    """Smallest distance of a float64 pixel value from a half-integer (where floor(v + 0.5) would depend on the last bits)."""
    return float(np.abs((v - np.floor(v)) - 0.5).min())


def quantize_u8(v):
    return np.floor(v + 0.5)


def patch_ref(frame, Minv, flip, color, mean, std, P, quantize=True):
    """ehm_image_patch's rule for one item -> float32 [3,P,P]: the float64 bilinear value, floor(v + 0.5) with `quantize`, then the float32
    chain of the reference under numpy 1.22: p = float32(v); p = clip(p * float32(color[c]), 0, 255); (p - float32(mean[c])) / float32(std[c])."""
    v = bilinear_f64(frame, Minv, P, flip)
    if quantize:
        v = quantize_u8(v)
    out = np.empty((3, P, P), np.float32)
    for c in range(3):
        p = v[:, :, 2 - c].astype(np.float32)
        p = np.clip(p * np.float32(color[c]), np.float32(0), np.float32(255))
        out[c] = (p - np.float32(mean[c])) / np.float32(std[c])
    assert out.dtype == np.float32
    return out


def scene_ref(scene, t_full, t_crop, flip, cs, sn, stride=1, spelling="sums"):
    """ehm_scene_augment's rule for one item, float64 with the float32 rounding in the middle -> (out float32 [ceil(N/stride),3], the float32
    intermediate).  `spelling`: 'sums' (explicit, in order) or 'einsum' (the reference's call)."""
    p = np.asarray(scene, np.float64)[::stride]
    t_full, t_crop = np.asarray(t_full, np.float64), np.asarray(t_crop, np.float64)
    q = (p - t_full) + t_crop
    if flip:
        q = q * np.array([-1.0, 1.0, 1.0])
    if spelling == "einsum":
        r = np.einsum("ij,kj->ki", np.array([[cs, -sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, 1.0]]), q)
    else:
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        r = np.stack([(cs * x + (-sn) * y) + 0.0 * z, (sn * x + cs * y) + 0.0 * z, (0.0 * x + 0.0 * y) + 1.0 * z], -1)
    mid = r.astype(np.float32)
    sg = np.array([-1.0 if flip else 1.0, 1.0, 1.0])
    return ((mid.astype(np.float64) - sg * t_crop) + sg * t_full).astype(np.float32), mid


def ulps32(a, b):
    """|a - b| in units of the float32 spacing at the larger magnitude."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def load_case(golden_dir, case):
    return np.load(os.path.join(golden_dir, f"g23_batch_{case}.npz"))


def golden_aug(g):
    """The golden's drawn parameters as egohmr_amd.batch's dict, B = 1."""
    return dict(scale=g["aug_scale"].reshape(1), rot=g["aug_rot"].reshape(1), flip=g["aug_flip"].reshape(1), color=g["aug_color"].reshape(1, 3),
                tx=g["aug_tx"].reshape(1), ty=g["aug_ty"].reshape(1))


def golden_inputs(g):
    """The keyword arguments of host_item / BatchBuilder.build a golden holds, B = 1."""
    return dict(center=g["center"][None], bbox_size=g["bbox_size"].reshape(1), keypoints_2d=g["keypoints_2d"][None], keypoints_3d=g["keypoints_3d"][None],
                smpl_params={k: g["in_" + k][None] for k in ("global_orient", "body_pose", "betas", "transl")},
                fx=g["fx"].reshape(1), cx=g["cx"].reshape(1), cy=g["cy"].reshape(1))


EXACT = ("keypoints_2d_vis_mask", "box_center", "box_size", "cam_cx", "cam_cy", "body_pose", "betas")
ONE_ULP = ("keypoints_2d", "orig_keypoints_2d", "keypoints_3d", "keypoints_3d_full", "global_orient")


def check_small_outputs(got, g, what=""):
    """The bars of the module docstring, key by key: `got` maps the names above to arrays of one item."""
    for k in EXACT:
        assert np.array_equal(np.asarray(got[k]), g["out_" + k]), (what, k, got[k], g["out_" + k])
    for k in ONE_ULP:
        u = ulps32(got[k], g["out_" + k])
        print(f"{what} {k}: largest deviation {u.max():.2f} float32 ulp")
        assert u.max() <= 1.0, (what, k, float(u.max()))


# ------------------------------------------------------------------------------------------------ the host half against the reference
@pytest.mark.parametrize("case", CASES[1:])
def test_draw_augmentation_is_the_references_draw(golden_dir, case):
    g = load_case(golden_dir, case)
    np.random.seed(int(g["seed"]))
    random.seed(int(g["seed"]))
    a = eb.draw_augmentation(eb.AugmentConfig(), 1)
    for k, want in golden_aug(g).items():
        assert a[k].dtype == want.dtype and np.array_equal(a[k].view(np.uint8), want.view(np.uint8)), (k, a[k], want)
    # the generators stand where the reference left them: the next draws agree too
    assert np.random.randn() == float(g["next_randn"]) and random.random() == float(g["next_random"])


def test_drawn_cases_are_what_their_names_say(golden_dir):
    g = {c: load_case(golden_dir, c) for c in CASES}
    assert float(g["noaug"]["aug_scale"]) == 1.0 and float(g["noaug"]["aug_rot"]) == 0 and not bool(g["noaug"]["aug_flip"])
    assert float(g["flip_rot"]["aug_rot"]) != 0 and bool(g["flip_rot"]["aug_flip"])
    assert float(g["rotmiss_noflip"]["aug_rot"]) == 0 and not bool(g["rotmiss_noflip"]["aug_flip"])
    b = g["border"]
    half = float(b["out_box_size"]) / 2
    assert float(b["out_box_center"][0]) + half > b["frame"].shape[1] and float(b["out_box_center"][1]) - half < 0


@pytest.mark.parametrize("case", CASES)
def test_host_outputs_against_the_reference(golden_dir, case):
    g = load_case(golden_dir, case)
    h = eb.host_item(golden_aug(g), img_hw=g["frame"].shape[:2], patch=int(g["patch"]), **golden_inputs(g))
    got = {k: h[k][0] for k in EXACT + ONE_ULP}
    check_small_outputs(got, g, case)
    assert np.array_equal(h["transl"][0], g["in_transl"])
    if case == "noaug":
        assert np.array_equal(h["transl"][0], g["out_transl"])              # the test loader leaves transl alone
    assert np.abs(h["trans"][0] - g["trans_crop"]).max() <= 1e-12 * np.abs(g["trans_crop"]).max()
    fx = (g["fx"] / 1500.0).astype(np.float32)
    assert np.array_equal(fx, g["out_fx"])


@pytest.mark.parametrize("case", CASES)
def test_restated_rules_equal_the_reference(golden_dir, case):
    g = load_case(golden_dir, case)
    h = eb.host_item(golden_aug(g), img_hw=g["frame"].shape[:2], patch=int(g["patch"]), **golden_inputs(g))
    P = int(g["patch"])
    pp, ap = h["patch_params"][0], h["aug_params"][0]
    Minv, flip = pp[0:6].reshape(2, 3), bool(pp[6])
    v = bilinear_f64(g["frame"], Minv, P, flip)
    d = tie_distance(v)
    print(f"{case}: nearest pixel value to a half-integer: {d:.3e}")
    assert d > TIE_MARGIN                                                   # the precondition of every quantised comparison
    img = patch_ref(g["frame"], Minv, flip, pp[7:10], eb.IMAGE_MEAN, eb.IMAGE_STD, P)
    err = np.abs(img.astype(np.float64) - g["out_img"].astype(np.float64)).max()
    print(f"{case}: img against the reference: {err:.3e} (bar {IMG_BAR:.3e})")
    assert err <= IMG_BAR
    for stride in (1, 3):
        sums, _ = scene_ref(g["scene"], ap[0:3], ap[3:6], bool(ap[6]), ap[7], ap[8], stride)
        ein, _ = scene_ref(g["scene"], ap[0:3], ap[3:6], bool(ap[6]), ap[7], ap[8], stride, "einsum")
        assert np.array_equal(sums, ein)                                   # the two float64 spellings differ on no coordinate of this fixture
        assert np.array_equal(sums, g["out_scene_pcd_verts_full"][::stride])


def test_rational_steps_put_pixels_on_exact_ties():
    """Why boxes such as 112 or 336 at rot = 0 are compared with quantize = False only: a rational step lands many values on k + 1/2."""
    frame = np.random.default_rng(5).integers(0, 256, (135, 240, 3), dtype=np.uint8)
    for box in (112.0, 336.0):
        a = eb.no_augmentation(1)
        trans = eb.gen_trans_from_patch(np.array([120.0]), np.array([67.0]), np.float32([box]), np.float32([box]), 224, 224, a["scale"], a["rot"])
        v = bilinear_f64(frame, eb.invert_affine(trans)[0], 224)
        on_tie = np.mean(np.abs((v - np.floor(v)) - 0.5) < TIE_MARGIN)
        print(f"box {box}: {100 * on_tie:.1f} % of the values within {TIE_MARGIN} of a half-integer")
        assert on_tie > 0.01


def test_invert_affine_and_solve_agree_with_the_scalar_forms():
    g = np.random.default_rng(7)
    src = g.uniform(0, 200, (5, 3, 2)).astype(np.float32)
    dst = np.float32([[112, 112], [112, 224], [224, 112]])[None].repeat(5, 0)
    T = eb.affine_from_3_points(src, dst)
    for b in range(5):
        pts = np.concatenate([src[b].astype(np.float64), np.ones((3, 1))], 1)
        assert np.abs(pts @ T[b].T - dst[b]).max() < 1e-9
        assert np.array_equal(eb.invert_affine(T)[b], invert_affine_ref(T[b]))


def test_config_defaults_and_argument_errors():
    c = eb.AugmentConfig()
    assert (c.SCALE_FACTOR, c.ROT_FACTOR, c.TRANS_FACTOR, c.COLOR_SCALE, c.ROT_AUG_RATE, c.DO_FLIP, c.FLIP_AUG_RATE) == (0.3, 30, 0.02, 0.2, 0.6, True, 0.5)
    from egohmr_amd._lib import EgoHMRHipError
    import egohmr_amd
    assert egohmr_amd.BatchBuilder is eb.BatchBuilder
    with pytest.raises(EgoHMRHipError, match="no CPU path"):
        eb.BatchBuilder("cpu")
    a = eb.no_augmentation(2)
    assert a["scale"].tolist() == [1, 1] and not a["flip"].any() and a["color"].tolist() == [[1, 1, 1]] * 2
    with pytest.raises(ValueError, match="color"):
        eb._check_augmentation(dict(a, color=np.ones((2, 2))), 2)
    with pytest.raises(ValueError, match="lacks"):
        eb._check_augmentation({k: v for k, v in a.items() if k != "tx"}, 2)


def test_batch_entries_reject_bad_arguments_without_a_gpu():
    from egohmr_amd import _lib
    L = _lib.lib()

    def desc(**kw):
        f = dict(frames=0x10000, F=2, H=135, W=240, frame_index=0x20000, params=0x30000, B=3, P=32, quantize=1, img=0x40000)
        f.update(kw)
        return C.byref(_lib.ImagePatchDesc(**f))

    assert L.ehm_image_patch(None, None) == -22 and b"bad argument" in L.ehm_last_error()
    for bad in (dict(frames=None), dict(frame_index=None), dict(params=None), dict(img=None), dict(B=0), dict(B=-1), dict(B=65536), dict(P=30), dict(P=0),
                dict(P=-4), dict(F=0), dict(H=0), dict(W=0), dict(img=0x40004)):
        assert L.ehm_image_patch(desc(**bad), None) == -22, bad
        assert b"bad argument" in L.ehm_last_error(), bad
    good = (0x10000, 0, 0x20000, 0x30000, 3, 257, 1)
    for i, v in ((0, None), (2, None), (3, None), (4, 0), (4, -2), (4, 65536), (5, 0), (6, 0), (6, -1)):
        args = list(good)
        args[i] = v
        assert L.ehm_scene_augment(*args, None) == -22, args
        assert b"bad argument" in L.ehm_last_error(), args
    with pytest.raises(_lib.EgoHMRHipError, match="ehm_scene_augment"):
        _lib.api().ehm_scene_augment(None, 0, None, None, 1, 1, 1, None)
