#!/usr/bin/env python3
"""Write tests/golden/g23_batch_<case>.npz by running the REFERENCE's own loader item on the CPU: dataloaders/augmentation.py:get_example (and
its do_augmentation), followed by the casts of dataloaders/egobody_dataset.py:241-274.  Test infrastructure, run by hand where the reference
tree is present; not collected by pytest.

    python tests/make_batch_golden.py            # from the repository root

augmentation.py imports cv2 and yacs, which are not installed: both are stand-ins placed in sys.modules here.
  * yacs.config gets a dummy CfgNode: a dict with attribute access, enough for configs/__init__.py:16-32 to state its defaults.
  * cv2 gets FLOAT64 RESTATEMENTS of the five functions the loader calls: imread (returns the case's seeded frame), getAffineTransform (the
    3-point system, solved per output row), warpAffine (the real-valued bilinear rule of include/egohmr_hip.h with floor(v + 0.5): NOT cv2's
    1/32-pixel grid with 15-bit weights), Rodrigues and getRotationMatrix2D (cv2's published formulas).  The `img` of these files is therefore
    the build's pixel rule driven through the reference's flow (flip, crop map, BGR -> RGB, colour scale, normalisation), not cv2's pixels; every
    other value is the reference's arithmetic on these restated matrices.
  * The SMPL models are the oracle's CPU SMPL on the synthetic assets (male 1, female 2), as tests/make_loss_golden.py sets them up.
np.random.seed / random.seed are fixed per case.  Each file holds data only: the inputs, the drawn parameters, every returned value.  Cases:
  noaug           the test loader (do_augment = False).  Box 168 and transl z = 2.5: `auge_scale * width / 224 * z` is then exact in float32,
                  so numpy >= 2 (which keeps this all-scalar product in float32 when auge_scale is the Python float 1.0) and the reference's
                  numpy 1.22 (float64) give the same bits
  flip_rot        augmentation with the rotation drawn and the flip hit
  rotmiss_noflip  augmentation with rot = 0 (the ROT_AUG_RATE miss) and no flip
  border          augmentation with the box across the frame's top and right borders
"""
from __future__ import annotations

import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import test_batch_cpu as T  # noqa: E402
from make_loss_golden import GenderSMPL  # noqa: E402
from oracle import make_golden as mg  # noqa: E402

H, W, N, PATCH = 135, 240, 257, 224
MEAN = 255. * np.array([0.485, 0.456, 0.406])          # egobody_dataset.py:46-47 on configs/prohmr.yaml
STD = 255. * np.array([0.229, 0.224, 0.225])
FX_NORM = 1500
PERM_2D = [0, 1, 5, 6, 7, 2, 3, 4, 8, 12, 13, 14, 9, 10, 11, 16, 15, 18, 17, 22, 23, 24, 19, 20, 21]     # egobody_dataset.py:65-66
PERM_3D = [0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22]

#        name              do_augment  seed  centre           box    transl
CASES = [("noaug",          False,      0,    (117.3, 66.9),  168.0, (0.1, -0.2, 2.5)),
         ("flip_rot",       True,       28,   (117.3, 66.9),  150.0, (0.13, -0.21, 2.83)),
         ("rotmiss_noflip", True,       6,    (101.7, 71.2),  100.0, (-0.27, 0.09, 3.41)),
         ("border",         True,       13,   (228.6, 12.4),  120.0, (0.52, -0.66, 2.97))]


# ------------------------------------------------------------------------------------------------ the cv2 stand-in
class _Cv2:
    IMREAD_COLOR, IMREAD_IGNORE_ORIENTATION, INTER_LINEAR = 1, 128, 1
    frames: dict = {}
    tie_distance = np.inf

    @staticmethod
    def imread(path, flags=None):
        return _Cv2.frames[path].copy()

    @staticmethod
    def getAffineTransform(src, dst):
        src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
        A = np.array([[src[k, 0], src[k, 1], 1.0] for k in range(3)])
        return np.stack([np.linalg.solve(A, dst[:, i]) for i in range(2)])

    @staticmethod
    def warpAffine(img, trans, size, flags=None):
        assert size[0] == size[1] and img.dtype == np.uint8
        v = T.bilinear_f64(np.ascontiguousarray(img), T.invert_affine_ref(trans), size[0])
        _Cv2.tie_distance = min(_Cv2.tie_distance, T.tie_distance(v))
        return T.quantize_u8(v).astype(np.uint8)

    @staticmethod
    def getRotationMatrix2D(center, angle, scale):
        a = angle * np.pi / 180
        alpha, beta = np.cos(a) * scale, np.sin(a) * scale
        return np.array([[alpha, beta, (1 - alpha) * center[0] - beta * center[1]], [-beta, alpha, beta * center[0] + (1 - alpha) * center[1]]])

    @staticmethod
    def Rodrigues(src):
        src = np.asarray(src, np.float64)
        if src.size == 3:
            r = src.reshape(3)
            theta = np.sqrt(r @ r)
            if theta < np.finfo(np.float64).eps:
                return np.eye(3), None
            c, s = np.cos(theta), np.sin(theta)
            u = r / theta
            K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
            return c * np.eye(3) + (1 - c) * np.outer(u, u) + s * K, None
        U, _, Vt = np.linalg.svd(src)
        R = U @ Vt
        r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        s = np.sqrt((r @ r) * 0.25)
        c = min(max((R[0, 0] + R[1, 1] + R[2, 2] - 1) * 0.5, -1.0), 1.0)
        theta = np.arccos(c)
        assert s >= 1e-5, "the fixtures stay away from cv2's branches at 0 and pi"
        return (r * (theta / (2 * s))).reshape(3, 1), None


def install():
    mg.install_shims(None)                                   # puts the reference tree on sys.path
    yacs, cfg = types.ModuleType("yacs"), types.ModuleType("yacs.config")
    cfg.CfgNode = _Cfg
    yacs.config = cfg
    sys.modules.update({"yacs": yacs, "yacs.config": cfg, "cv2": _Cv2})


def aug_config():
    from configs import _C                                   # configs/__init__.py:25-32, through the dummy CfgNode
    return _C.DATASETS.CONFIG


class _Cfg(dict):
    """yacs.config.CfgNode as configs/__init__.py uses it: attribute access, new_allowed."""
    def __init__(self, new_allowed=False):
        super().__init__()

    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def fixture(name, centre, box, transl):
    g = np.random.default_rng([23, sum(map(ord, name))])
    kp2 = np.zeros((25, 3))
    kp2[:, 0], kp2[:, 1] = g.uniform(-10, W + 10, 25), g.uniform(-10, H + 10, 25)
    kp2[:, 2] = (g.random(25) < 0.7) * g.uniform(0.3, 1.0, 25)
    t = np.float32(transl)
    return dict(frame=g.integers(0, 256, (H, W, 3), dtype=np.uint8), center=np.float32(centre), bbox_size=np.float32(box),
                keypoints_2d=kp2, keypoints_3d=t.astype(np.float64) + g.normal(scale=0.3, size=(24, 3)),
                in_global_orient=g.normal(scale=0.4, size=3).astype(np.float32), in_body_pose=g.normal(scale=0.25, size=69).astype(np.float32),
                in_betas=g.normal(scale=0.8, size=10).astype(np.float32), in_transl=t, gender=np.int32(g.integers(0, 2)),
                fx=np.float64(187.31), fy=np.float64(186.94), cx=np.float64(121.7), cy=np.float64(66.2),
                scene=t.astype(np.float64) + g.uniform(-1.5, 1.5, (N, 3)))


def run_case(name, do_augment, seed, centre, box, transl, get_example, do_augmentation, models):
    f = fixture(name, centre, box, transl)
    _Cv2.frames, _Cv2.tie_distance = {name: f["frame"]}, np.inf
    cfg = aug_config()
    # what the reference will draw, drawn once before: the same seeds give the same stream
    np.random.seed(seed)
    random.seed(seed)
    drawn = do_augmentation(cfg) if do_augment else (1.0, 0, False, [1.0, 1.0, 1.0], 0., 0.)
    np.random.seed(seed)
    random.seed(seed)
    sp = {k: f["in_" + k].copy() for k in ("global_orient", "transl", "body_pose", "betas")}
    has = {k: True for k in sp}
    center, bbox_size = f["center"].copy(), f["bbox_size"]
    # egobody_dataset.py:229-239
    (img_patch, kp2_crop, vis_mask, kp2_full, scene_full, kp3_crop, kp3_full, sp_out, has_out, center_x_auge, center_y, cam_cx_auge, auge_scale,
     _) = get_example(name, center[0], center[1], bbox_size, bbox_size, f["keypoints_2d"], f["keypoints_3d"][0:24].copy(), sp, has, PERM_2D, PERM_3D,
                      PATCH, PATCH, MEAN, STD, do_augment, cfg, f["fx"], cam_cx=f["cx"], cam_cy=f["cy"], scene_pcd_verts=f["scene"],
                      smpl_male=models[0], smpl_female=models[1], gender=f["gender"])
    nxt = (np.random.randn(), random.random())
    scale, rot, flip, color, tx, ty = drawn
    assert float(auge_scale) == float(scale)
    assert _Cv2.tie_distance > T.TIE_MARGIN, _Cv2.tie_distance
    # egobody_dataset.py:241-274
    out = dict(out_img=img_patch, out_keypoints_2d=kp2_crop.astype(np.float32), out_orig_keypoints_2d=kp2_full.astype(np.float32),
               out_keypoints_2d_vis_mask=vis_mask, out_keypoints_3d=kp3_crop.astype(np.float32), out_keypoints_3d_full=kp3_full.astype(np.float32),
               out_fx=(f["fx"] / FX_NORM).astype(np.float32), out_fy=(f["fy"] / FX_NORM).astype(np.float32), out_cam_cx=cam_cx_auge.astype(np.float32),
               out_cam_cy=f["cy"].astype(np.float32), out_box_center=np.array([center_x_auge, center_y]).astype(np.float32),
               out_box_size=(bbox_size * auge_scale).astype(np.float32), out_scene_pcd_verts_full=scene_full.astype(np.float32))
    for k in sp_out:
        out["out_" + k] = np.asarray(sp_out[k]).astype(np.float32)
    assert img_patch.dtype == np.float32 and img_patch.shape == (3, PATCH, PATCH) and all(bool(v) for v in has_out.values())
    # the crop's map as the reference made it (for the solve's own error bar), from the same stand-in
    from dataloaders.augmentation import gen_trans_from_patch_cv
    trans = gen_trans_from_patch_cv(center_x_auge, center_y, bbox_size, bbox_size, PATCH, PATCH, scale, rot)      # (center_x_auge: already mirrored)
    print(f"   {name}: seed {seed} scale {float(scale):.4f} rot {float(rot):.3f} flip {bool(flip)} tx {float(tx):.4f} ty {float(ty):.4f}; "
          f"nearest tie {_Cv2.tie_distance:.2e}; visible {int(vis_mask.sum())} of 25")
    mg.save(f"g23_batch_{name}", seed=seed, do_augment=do_augment, patch=PATCH, aug_scale=np.float64(scale), aug_rot=np.float64(rot), aug_flip=bool(flip),
            aug_color=np.array(color, np.float64), aug_tx=np.float64(tx), aug_ty=np.float64(ty), next_randn=nxt[0], next_random=nxt[1],
            tie_distance=_Cv2.tie_distance, trans_crop=trans, **f, **out)


def main():
    install()
    from dataloaders.augmentation import do_augmentation, get_example
    models = (GenderSMPL("male"), GenderSMPL("female"))
    for name, do_augment, seed, centre, box, transl in CASES:
        run_case(name, do_augment, seed, centre, box, transl, get_example, do_augmentation, models)


if __name__ == "__main__":
    main()
