"""GPU: csrc/batch.hip (ehm_image_patch, ehm_scene_augment) against the numpy restatements of tests/test_batch_cpu.py on identical parameters,
BatchBuilder.build against the reference loader's own results (tests/golden/g23_batch_*.npz), and a built batch through the sampling call and
compute_loss.  Every test here fails without the feature (egohmr_amd.batch and the two entry points do not exist on the parent).

Bars (derived, not measured).
  image patch, quantised, generic geometry: at most 1 float32 ulp.  The float64 bilinear value is formed from the same separately rounded
      operations on both sides, no value lies within 1e-9 of a half-integer (asserted per item), so the uint8 level is the same and the three
      float32 operations that follow are correctly rounded on both sides; a one-level miss would be 1 / 57 = 0.02.
  image patch, rational steps (quantize = False only: 9 - 31 % of the values sit on exact ties): 2^-21, the bar of the CPU file.
  scene: at most 2 float32 ulps at the larger of the intermediate's and the result's magnitude (the float32 rounding in the middle can fall either
      side when the float64 value before it differs in its last bit), and at most 1e-3 of the coordinates may differ at all.
  builder against the reference: the bars of tests/test_batch_cpu.py key by key; the augmented transl within the SMPL joint bar of
      tests/test_gpu_parity.py (atol 5e-6: the float32 LBS against the oracle)."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_batch_cpu as T  # noqa: E402
from egohmr_amd import batch as eb  # noqa: E402
from egohmr_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, F = 135, 240, 2
FRAME_INDEX = np.array([1, 0, 1], np.int32)
SMPL_JOINT_ATOL = 5e-6


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def frames():
    return np.random.default_rng(2301).integers(0, 256, (F, H, W, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def smpl_models(dev):
    from egohmr_amd.smpl import SMPL
    return SMPL(syn.make_smpl_asset(1), gender="male").to(dev), SMPL(syn.make_smpl_asset(2), gender="female").to(dev)


def _rows(items, P):
    """The kernel's parameter rows for items (cx, cy, box, scale, rot, flip, color) - or a ready (Minv, flip, color)."""
    rows = np.zeros((len(items), eb.PATCH_PARAMS))
    for b, it in enumerate(items):
        if len(it) == 3:
            Minv, flip, color = it
        else:
            cx, cy, box, scale, rot, flip, color = it
            c_x = W - cx - 1 if flip else cx
            trans = eb.gen_trans_from_patch(np.array([c_x]), np.array([cy]), np.float32([box]), np.float32([box]), P, P, np.array([scale]), np.array([rot]))
            Minv = eb.invert_affine(trans)[0]
        rows[b, 0:6], rows[b, 6], rows[b, 7:10] = np.asarray(Minv).reshape(6), flip, color
    return rows


def _run_patch(frames, rows, P, dev, quantize=True, frame_index=FRAME_INDEX):
    img = eb.image_patch(torch.from_numpy(frames).to(dev), torch.from_numpy(frame_index).to(dev), torch.from_numpy(rows).to(dev), P, quantize=quantize)
    torch.cuda.synchronize()
    return img.cpu().numpy()


def _ref_patch(frames, rows, P, quantize=True, frame_index=FRAME_INDEX):
    return np.stack([T.patch_ref(frames[frame_index[b]], r[0:6].reshape(2, 3), bool(r[6]), r[7:10], eb.IMAGE_MEAN, eb.IMAGE_STD, P, quantize)
                     for b, r in enumerate(rows)])


C1, C2, C3 = (1.13, 0.87, 1.02), (0.81, 1.19, 0.95), (1.0, 1.0, 1.0)
GENERIC = {
    "flip_off_on_rot_pm": [(117.3, 66.9, 150, 1.13, 17.0, False, C1), (117.3, 66.9, 150, 1.13, -23.0, True, C2), (101.7, 71.2, 150, 1.13, 0.0, True, C3)],
    "up8_down_outside": [(101.2, 70.3, 28, 1.0, 5.0, False, C1), (121.9, 64.2, 600, 1.0, -11.0, True, C2), (700.5, -400.2, 100, 1.0, 3.0, False, C3)],
    "left_right_top": [(5.3, 60.1, 60, 1.07, 9.0, False, C2), (236.2, 70.4, 60, 0.93, -6.0, True, C1), (120.6, 3.2, 60, 1.0, 0.0, False, C3)],
    "bottom_and_mixed": [(118.4, 133.1, 60, 1.11, 14.0, True, C1), (3.1, 2.2, 90, 1.0, -31.0, False, C2), (238.3, 133.6, 90, 1.0, 44.0, True, C3)],
}


@pytest.mark.parametrize("P", [32, 224])
@pytest.mark.parametrize("name", list(GENERIC))
def test_image_patch_quantised_generic(dev, frames, name, P):
    rows = _rows(GENERIC[name], P)
    for b, r in enumerate(rows):
        d = T.tie_distance(T.bilinear_f64(frames[FRAME_INDEX[b]], r[0:6].reshape(2, 3), P, bool(r[6])))
        assert d > T.TIE_MARGIN, (name, b, d)
    got, ref = _run_patch(frames, rows, P, dev), _ref_patch(frames, rows, P)
    u = T.ulps32(got, ref)
    print(f"{name} P={P}: largest deviation {u.max():.2f} float32 ulp, {int((got != ref).sum())} of {got.size} values differ")
    assert got.shape == (3, 3, P, P) and got.dtype == np.float32
    assert u.max() <= 1.0
    if name == "up8_down_outside":                                          # wholly outside: every pixel is the normalised border value
        for c in range(3):
            want = (np.float32(0) - np.float32(eb.IMAGE_MEAN[c])) / np.float32(eb.IMAGE_STD[c])
            assert np.all(got[2, c] == want)
        assert len(np.unique(got[0])) > 100 and len(np.unique(got[1])) > 100


@pytest.mark.parametrize("P", [32, 224])
def test_image_patch_map_onto_the_last_row_and_column(dev, frames, P):
    """sx = x + (W - P), sy = y + (H - P): the last patch pixel samples (W-1, H-1) with fx = fy = 0 - the neighbours at column W and row H carry
    weight 0 and lie outside the frame (of the LAST frame: past the allocation); the patch is the frame's corner, exactly."""
    Minv = np.array([[1.0, 0.0, W - P], [0.0, 1.0, H - P]])
    rows = _rows([(Minv, False, C3), (Minv, True, C3), (Minv, False, C1)], P)
    got, ref = _run_patch(frames, rows, P, dev), _ref_patch(frames, rows, P)
    assert np.array_equal(got, ref)
    for b, flip in ((0, False), (1, True)):
        fr = frames[FRAME_INDEX[b]][:, ::-1] if flip else frames[FRAME_INDEX[b]]
        corner = np.zeros((P, P, 3))
        h = min(P, H)
        corner[P - h:, :, :] = fr[H - h:, W - P:, :]
        want = np.stack([(corner[:, :, 2 - c].astype(np.float32) - np.float32(eb.IMAGE_MEAN[c])) / np.float32(eb.IMAGE_STD[c]) for c in range(3)])
        assert np.array_equal(got[b], want)


@pytest.mark.parametrize("P", [32, 224])
def test_image_patch_rational_steps_unquantised(dev, frames, P):
    items = [(120.0, 67.0, 112, 1.0, 0.0, False, C1), (120.0, 67.0, 336, 1.0, 0.0, True, C2), (64.0, 32.0, 56, 1.0, 0.0, False, C3)]
    rows = _rows(items, P)
    got, ref = _run_patch(frames, rows, P, dev, quantize=False), _ref_patch(frames, rows, P, quantize=False)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()
    print(f"rational steps P={P}: largest deviation {err:.3e} (bar {T.IMG_BAR:.3e})")
    assert err <= T.IMG_BAR


def test_image_patch_refusals_and_repeatability(dev, frames):
    from egohmr_amd._lib import EgoHMRHipError
    rows = _rows(GENERIC["flip_off_on_rot_pm"], 32)
    with pytest.raises(EgoHMRHipError, match="ehm_image_patch"):
        _run_patch(frames, _rows(GENERIC["flip_off_on_rot_pm"], 30), 30, dev)
    a, b = _run_patch(frames, rows, 32, dev), _run_patch(frames, rows, 32, dev)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    a, b = _run_patch(frames, _rows(GENERIC["left_right_top"], 224), 224, dev), _run_patch(frames, _rows(GENERIC["left_right_top"], 224), 224, dev)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # a frame index outside [0, F) is marked, not read
    bad = _run_patch(frames, rows, 32, dev, frame_index=np.array([1, 2, -1], np.int32))
    assert np.isfinite(bad[0]).all() and np.isnan(bad[1]).all() and np.isnan(bad[2]).all()


# ------------------------------------------------------------------------------------------------ scene augmentation
def _scene_case(seed=2302, B=4, N=257):
    g = np.random.default_rng(seed)
    t_full = g.uniform(-0.7, 0.7, (B, 3)).astype(np.float32).astype(np.float64)
    t_full[:, 2] += 3.0
    t_full = t_full.astype(np.float32).astype(np.float64)
    t_crop = t_full + g.uniform(-0.5, 0.5, (B, 3)) * [1, 1, 3]
    scene = t_full[:, None, :] + g.uniform(-1.5, 1.5, (B, N, 3))
    flip = np.array([0, 1, 0, 1], bool)[:B]
    rot = np.array([0.0, 0.0, 21.7, -38.2])[:B]
    rot_rad = -rot * np.pi / 180
    cs, sn = np.where(rot != 0, np.cos(rot_rad), 1.0), np.where(rot != 0, np.sin(rot_rad), 0.0)
    params = np.zeros((B, eb.AUG_PARAMS))
    params[:, 0:3], params[:, 3:6], params[:, 6], params[:, 7], params[:, 8] = t_full, t_crop, flip, cs, sn
    return scene, params


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("stride", [1, 3])
def test_scene_augment_against_float64(dev, stride, dtype):
    scene, params = _scene_case()
    scene = scene.astype(dtype)
    B, N = scene.shape[:2]
    refs = [T.scene_ref(scene[b], params[b, 0:3], params[b, 3:6], bool(params[b, 6]), params[b, 7], params[b, 8], stride) for b in range(B)]
    for b in range(B):                                                       # the fixture's precondition: the two float64 spellings differ on none
        ein, _ = T.scene_ref(scene[b], params[b, 0:3], params[b, 3:6], bool(params[b, 6]), params[b, 7], params[b, 8], stride, "einsum")
        assert np.array_equal(ein, refs[b][0])
    ref, mid = np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
    got = eb.scene_augment(torch.from_numpy(scene).to(dev), torch.from_numpy(params).to(dev), stride)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == (B, -(-N // stride), 3) and got.dtype == np.float32
    scale = np.spacing(np.maximum(np.abs(mid), np.abs(ref))).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / scale
    differ = float(np.mean(got != ref))
    print(f"scene stride {stride} {np.dtype(dtype).name}: largest deviation {err.max():.2f} float32 ulp, {differ:.2e} of the coordinates differ")
    assert err.max() <= 2.0 and differ <= 1e-3
    again = eb.scene_augment(torch.from_numpy(scene).to(dev), torch.from_numpy(params).to(dev), stride).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


def test_scene_augment_refusals(dev):
    from egohmr_amd._lib import EgoHMRHipError
    scene, params = _scene_case()
    with pytest.raises(EgoHMRHipError, match="ehm_scene_augment"):
        eb.scene_augment(torch.from_numpy(scene).to(dev), torch.from_numpy(params).to(dev), 0)
    with pytest.raises(ValueError):
        eb.scene_augment(torch.from_numpy(scene).to(dev).half(), torch.from_numpy(params).to(dev), 1)


# ------------------------------------------------------------------------------------------------ the builder against the reference
def _build_from_golden(g, dev, smpl_models, augment, stride=1, scene_on_device=False):
    bld = eb.BatchBuilder(dev, img_size=int(g["patch"]), smpl_male=smpl_models[0], smpl_female=smpl_models[1], scene_stride=stride)
    kw = T.golden_inputs(g)
    frames = np.stack([np.zeros_like(g["frame"]), g["frame"]])                # the item's frame is the second of two
    scene = g["scene"][None]
    if scene_on_device:
        frames, scene = torch.from_numpy(frames).to(dev), torch.from_numpy(scene).to(dev)
    return bld.build(frames, np.array([1]), kw["center"], kw["bbox_size"], kw["keypoints_2d"], kw["keypoints_3d"], kw["smpl_params"], g["gender"].reshape(1),
                     kw["fx"], g["fy"].reshape(1), kw["cx"], kw["cy"], scene, augment=augment)


LOADER_KEYS = ["img", "keypoints_2d", "orig_keypoints_2d", "keypoints_2d_vis_mask", "keypoints_3d", "keypoints_3d_full", "smpl_params", "has_smpl_params",
               "smpl_params_is_axis_angle", "gender", "fx", "fy", "cam_cx", "cam_cy", "box_center", "box_size", "scene_pcd_verts_full"]


@pytest.mark.parametrize("case", T.CASES)
def test_builder_against_the_reference(dev, golden_dir, smpl_models, case):
    g = T.load_case(golden_dir, case)
    aug = None if case == "noaug" else T.golden_aug(g)
    out = _build_from_golden(g, dev, smpl_models, aug, scene_on_device=(case == "border"))
    torch.cuda.synchronize()
    assert list(out) == LOADER_KEYS
    P = int(g["patch"])
    shapes = dict(img=(1, 3, P, P), keypoints_2d=(1, 25, 3), orig_keypoints_2d=(1, 25, 3), keypoints_2d_vis_mask=(1, 25), keypoints_3d=(1, 24, 3),
                  keypoints_3d_full=(1, 24, 3), gender=(1,), fx=(1,), fy=(1,), cam_cx=(1,), cam_cy=(1,), box_center=(1, 2), box_size=(1,),
                  scene_pcd_verts_full=(1, 257, 3))
    for k, s in shapes.items():
        assert tuple(out[k].shape) == s and out[k].is_cuda, k
        if k not in ("keypoints_2d_vis_mask", "gender"):
            assert out[k].dtype == torch.float32, k
    assert {k: tuple(v.shape) for k, v in out["smpl_params"].items()} == dict(global_orient=(1, 3), transl=(1, 3), body_pose=(1, 69), betas=(1, 10))
    for d in (out["has_smpl_params"], out["smpl_params_is_axis_angle"]):
        assert list(d) == ["global_orient", "transl", "body_pose", "betas"] and all(not v.is_cuda and v.dtype == torch.bool for v in d.values())
    assert [bool(v[0]) for v in out["smpl_params_is_axis_angle"].values()] == [True, False, True, False]
    c = lambda t: t[0].cpu().numpy()
    got = {k: c(out[k]) for k in ("keypoints_2d", "orig_keypoints_2d", "keypoints_2d_vis_mask", "keypoints_3d", "keypoints_3d_full", "box_center", "box_size",
                                  "cam_cx", "cam_cy")}
    got.update({k: c(out["smpl_params"][k]) for k in ("global_orient", "body_pose", "betas")})
    T.check_small_outputs(got, g, case)
    assert np.array_equal(c(out["fx"]), g["out_fx"]) and np.array_equal(c(out["fy"]), g["out_fy"]) and int(out["gender"][0]) == int(g["gender"])
    err = np.abs(c(out["img"]).astype(np.float64) - g["out_img"].astype(np.float64)).max()
    print(f"{case}: img against the reference {err:.3e} (bar {T.IMG_BAR:.3e})")
    assert err <= T.IMG_BAR
    sc, ref = c(out["scene_pcd_verts_full"]), g["out_scene_pcd_verts_full"]
    ap = eb.host_item(aug if aug is not None else eb.no_augmentation(1), img_hw=g["frame"].shape[:2], patch=P, **T.golden_inputs(g))["aug_params"][0]
    _, mid = T.scene_ref(g["scene"], ap[0:3], ap[3:6], bool(ap[6]), ap[7], ap[8])
    scale = np.spacing(np.maximum(np.abs(mid), np.abs(ref))).astype(np.float64)
    assert (np.abs(sc.astype(np.float64) - ref.astype(np.float64)) / scale).max() <= 2.0 and np.mean(sc != ref) <= 1e-3
    transl = c(out["smpl_params"]["transl"])
    if case == "noaug":
        assert np.array_equal(transl, g["out_transl"])
    else:
        print(f"{case}: augmented transl against the reference {np.abs(transl - g['out_transl']).max():.3e} (bar {SMPL_JOINT_ATOL:.1e})")
        np.testing.assert_allclose(transl, g["out_transl"], atol=SMPL_JOINT_ATOL)


def test_builder_draw_stride_and_errors(dev, golden_dir, smpl_models):
    g = T.load_case(golden_dir, "flip_rot")
    np.random.seed(int(g["seed"]))
    random.seed(int(g["seed"]))
    drawn = _build_from_golden(g, dev, smpl_models, "draw", stride=3)
    explicit = _build_from_golden(g, dev, smpl_models, T.golden_aug(g), stride=1)
    assert np.array_equal(drawn["img"].cpu().numpy(), explicit["img"].cpu().numpy())
    assert np.array_equal(drawn["scene_pcd_verts_full"].cpu().numpy(), explicit["scene_pcd_verts_full"].cpu().numpy()[:, ::3])
    assert np.array_equal(drawn["smpl_params"]["transl"].cpu().numpy(), explicit["smpl_params"]["transl"].cpu().numpy())
    with pytest.raises(ValueError, match="smpl_male"):
        _build_from_golden(g, dev, (None, None), T.golden_aug(g))
    _build_from_golden(g, dev, (None, None), None)                            # the test loader needs no SMPL model
    with pytest.raises(ValueError, match="frame_index"):
        eb.BatchBuilder(dev).build(np.zeros((1, 8, 8, 3), np.uint8), np.array([1]), *[None] * 10, np.zeros((1, 4, 3)))
    with pytest.raises(ValueError, match="img_size"):
        eb.BatchBuilder(dev, img_size=30)


# ------------------------------------------------------------------------------------------------ end to end
def test_built_batch_through_sampling_and_compute_loss(dev, frames, smpl_models, synth_weights, smpl_asset):
    import val_losses_ref as R
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import build_synthetic_model
    B, N = 4, 512
    model = build_synthetic_model(dev, 0, diffuse_fuse=True, state_dict=synth_weights, smpl_asset=smpl_asset, smpl_asset_male=syn.make_smpl_asset(1),
                                  smpl_asset_female=syn.make_smpl_asset(2), start_coap_epoch=R.START_COAP_EPOCH, **R.CASE_WEIGHTS)
    g = np.random.default_rng(2303)
    a = syn.make_gt_annotations(B, seed=23)
    transl = (np.array([0.0, 0.0, 3.0]) + g.uniform(-0.5, 0.5, (B, 3))).astype(np.float32)
    kp2 = np.concatenate([g.uniform(0, W, (B, 25, 1)), g.uniform(0, H, (B, 25, 1)), (g.random((B, 25, 1)) < 0.7) * g.uniform(0.3, 1, (B, 25, 1))], -1)
    args = dict(frames=frames, frame_index=np.array([1, 0, 0, 1]), center=np.float32([[117.3, 66.9], [60.2, 40.8], [200.4, 100.1], [120.0, 67.0]]),
                bbox_size=np.float32([150, 90, 120, 60]), keypoints_2d=kp2, keypoints_3d=transl[:, None].astype(np.float64) + g.normal(scale=0.3, size=(B, 24, 3)),
                smpl_params=dict(global_orient=a["global_orient"], body_pose=a["body_pose"], betas=a["betas"], transl=transl), gender=a["gender"],
                fx=np.full(B, 187.3), fy=np.full(B, 187.3), cx=np.full(B, 120.0), cy=np.full(B, 67.5),
                scene=(transl[:, None] + g.uniform(-1, 1, (B, N, 3))).astype(np.float32),
                augment=dict(scale=[1.1, 0.9, 1.0, 1.2], rot=[12.0, 0.0, -20.0, 0.0], flip=[True, False, False, True], color=np.full((B, 3), 1.05), tx=[0.01] * B, ty=[-0.01] * B))
    bld = eb.BatchBuilder(dev, smpl_male=smpl_models[0], smpl_female=smpl_models[1])
    d = create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="ddim5")
    noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B, seed=4)).to(dev)
    runs = []
    for _ in range(2):
        batch = bld.build(**args)
        assert batch["img"].shape == (B, 3, 224, 224) and torch.isfinite(batch["img"]).all()
        o = d.val_losses(model, batch, shape=[B, 144], clip_denoised=False, timestep_respacing="ddim5", cur_epoch=0, noise_stack=noise)
        assert list(o["losses"]) == list(R.LOSS_KEYS) and all(torch.isfinite(v).item() for v in o["losses"].values())
        assert torch.isfinite(o["pred_keypoints_3d_full"]).all() and o["losses_per_item"]["loss"].shape == (B,)
        runs.append({k: v.cpu().numpy() for k, v in o["losses"].items()} | {"kp": o["pred_keypoints_3d_full"].cpu().numpy()})
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
