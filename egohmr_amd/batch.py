"""The EgoBody loader's batch, built on the device from decoded frames and per-item annotations.

The reference builds one item at a time on the CPU (dataloaders/egobody_dataset.py:167-279 -> dataloaders/augmentation.py:get_example): a
cv2.warpAffine, a Python loop over channels, a per-item SMPL call for the augmented translation and a 600 KB upload per item.  Here:

    img                     csrc/batch.hip ehm_image_patch     generate_image_patch + BGR->RGB + the colour / normalise loop (:121-150, :373-383)
    scene_pcd_verts_full    csrc/batch.hip ehm_scene_augment   augmentation.py:429-438 + scene_verts_3d_processing + egobody_dataset.py:272-273
    smpl_params['transl']   SMPL.forward, batched, by gender   augmentation.py:446-460 (under augmentation only)
    everything else         numpy on the host, below           the 25-rows-per-item arithmetic, expression by expression as the reference writes it

Every scalar the host can derive is computed here in numpy and the kernels get parameter rows in one upload, as egohmr_amd.scene does.  The
dtypes follow the reference's operands: centre and box are float32 (egobody_dataset.py:173-176), the camera intrinsics float64 (:80-83), the
drawn parameters float64; a float32 value meeting a float64 one is promoted to float64, which is how numpy 1.22 (the reference's) evaluates
these scalar expressions.

The frames themselves may arrive decoded (uint8 [F,H,W,3] BGR) or still encoded: a sequence of baseline-JPEG ``bytes`` or paths is decoded
onto the device by egohmr_amd.jpeg.JpegDecoder (host Huffman stage, HIP IDCT / upsampling / colour: libjpeg's pixels, which are cv2.imread's
with IMREAD_COLOR | IMREAD_IGNORE_ORIENTATION, augmentation.py:346; checked against PIL, not against cv2).

Not built: the dataset index, a prefetching loader, `orig_img` / `imgname`, the commented-out extreme
crop, and cv2's fixed-point interpolation grid - the patch is the real-valued bilinear rule of include/egohmr_hip.h.
"""
from __future__ import annotations

import ctypes as C
import os
import random as _random
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

PATCH_PARAMS, AUG_PARAMS = 16, 16                 # EHM_PATCH_PARAMS, EHM_AUG_PARAMS
IMAGE_MEAN = 255. * np.array([0.485, 0.456, 0.406])          # egobody_dataset.py:46-47 on configs/prohmr.yaml:39-40
IMAGE_STD = 255. * np.array([0.229, 0.224, 0.225])
FLIP_CAM_WIDTH = 1920                             # augmentation.py:441: the literal, not the frame's width
CROP_CAM_RES = 224                                # augmentation.py:424: the literal, not patch_width
# openpose 25 / smpl 24 topologies (egobody_dataset.py:65-66)
FLIP_2D = [0, 1, 5, 6, 7, 2, 3, 4, 8, 12, 13, 14, 9, 10, 11, 16, 15, 18, 17, 22, 23, 24, 19, 20, 21]
FLIP_3D = [0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22]
# augmentation.py:189-195 (fliplr_params), already shifted by the global orientation's three entries
BODY_POSE_FLIP = [i - 3 for i in [6, 7, 8, 3, 4, 5, 9, 10, 11, 15, 16, 17, 12, 13, 14, 18, 19, 20, 24, 25, 26, 21, 22, 23, 27, 28, 29, 33,
                                  34, 35, 30, 31, 32, 36, 37, 38, 42, 43, 44, 39, 40, 41, 45, 46, 47, 51, 52, 53, 48, 49, 50, 57, 58, 59, 54, 55,
                                  56, 63, 64, 65, 60, 61, 62, 69, 70, 71, 66, 67, 68]]


@dataclass
class AugmentConfig:
    """The seven DATASETS.CONFIG values do_augmentation reads, with the defaults of configs/__init__.py:25-32 (the eighth, TRANS_AUG_RATE, is
    read nowhere in the reference)."""
    SCALE_FACTOR: float = 0.3
    ROT_FACTOR: float = 30
    TRANS_FACTOR: float = 0.02
    COLOR_SCALE: float = 0.2
    ROT_AUG_RATE: float = 0.6
    DO_FLIP: bool = True
    FLIP_AUG_RATE: float = 0.5


def no_augmentation(B: int) -> dict:
    """The test loader's parameters (augmentation.py:356): 1.0, 0, False, [1, 1, 1], 0, 0."""
    return dict(scale=np.ones(B), rot=np.zeros(B), flip=np.zeros(B, bool), color=np.ones((B, 3)), tx=np.zeros(B), ty=np.zeros(B))


def draw_augmentation(cfg: AugmentConfig, B: int) -> dict:
    """do_augmentation (augmentation.py:14-38) per item, in item order, on the global ``np.random`` and ``random`` generators in the
    reference's order: three randn, then ``random.random()`` and - only on a hit - the rotation's randn (:31-32), the flip's
    ``random.random()`` (only with DO_FLIP), three ``random.uniform``."""
    out = no_augmentation(B)
    for b in range(B):
        tx = np.clip(np.random.randn(), -1.0, 1.0) * cfg.TRANS_FACTOR
        ty = np.clip(np.random.randn(), -1.0, 1.0) * cfg.TRANS_FACTOR
        scale = np.clip(np.random.randn(), -1.0, 1.0) * cfg.SCALE_FACTOR + 1.0
        rot = np.clip(np.random.randn(), -2.0,
                      2.0) * cfg.ROT_FACTOR if _random.random() <= cfg.ROT_AUG_RATE else 0
        do_flip = cfg.DO_FLIP and _random.random() <= cfg.FLIP_AUG_RATE
        c_up = 1.0 + cfg.COLOR_SCALE
        c_low = 1.0 - cfg.COLOR_SCALE
        color_scale = [_random.uniform(c_low, c_up), _random.uniform(c_low, c_up), _random.uniform(c_low, c_up)]
        out["scale"][b], out["rot"][b], out["flip"][b], out["color"][b], out["tx"][b], out["ty"][b] = scale, rot, bool(do_flip), color_scale, tx, ty
    return out


def _check_augmentation(aug: dict, B: int) -> dict:
    shapes = dict(scale=(B,), rot=(B,), flip=(B,), color=(B, 3), tx=(B,), ty=(B,))
    out = {}
    for k, shp in shapes.items():
        if k not in aug:
            raise ValueError(f"augment lacks {k!r} (expected the keys {sorted(shapes)})")
        a = np.asarray(aug[k], bool if k == "flip" else np.float64)
        if a.shape != shp:
            raise ValueError(f"augment[{k!r}] has shape {a.shape}, expected {shp}")
        out[k] = a
    return out


# ---------------------------------------------------------------------------------------------------------------- geometry, vectorised over B
def rotate_2d(x, y, rot_rad):
    """augmentation.py:40-54 on float32 x, y [B] and float64 angles: float64 products, the result rounded to float32."""
    sn, cs = np.sin(rot_rad), np.cos(rot_rad)
    xx = x * cs - y * sn
    yy = x * sn + y * cs
    return np.stack([xx, yy], -1).astype(np.float32)


def affine_from_3_points(src, dst):
    """cv2.getAffineTransform's system for float32 point triples [B,3,2], solved in float64: the 2x3 `trans` with trans @ [x, y, 1] = dst."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    A = np.concatenate([src, np.ones(src.shape[:-1] + (1,))], -1)            # [B,3,3]: rows [x_k, y_k, 1]
    return np.swapaxes(np.linalg.solve(A, dst), -1, -2)                       # [B,2,3]


def gen_trans_from_patch(c_x, c_y, src_width, src_height, dst_width, dst_height, scale, rot):
    """gen_trans_from_patch_cv (augmentation.py:57-104) over B, with its float32 roundings of the direction vectors and of src / dst."""
    B = len(c_x)
    src_w = src_width * scale
    src_h = src_height * scale
    src_center = np.stack([c_x, c_y], -1).astype(np.float64)                  # np.zeros(2): float64
    rot_rad = np.pi * rot / 180
    zero = np.zeros(B, np.float32)
    src_downdir = rotate_2d(zero, (src_h * 0.5).astype(np.float32), rot_rad)
    src_rightdir = rotate_2d((src_w * 0.5).astype(np.float32), zero, rot_rad)
    dst_w, dst_h = dst_width, dst_height
    dst_center = np.array([dst_w * 0.5, dst_h * 0.5], dtype=np.float32)
    dst_downdir = np.array([0, dst_h * 0.5], dtype=np.float32)
    dst_rightdir = np.array([dst_w * 0.5, 0], dtype=np.float32)
    src = np.zeros((B, 3, 2), dtype=np.float32)
    src[:, 0, :] = src_center
    src[:, 1, :] = src_center + src_downdir
    src[:, 2, :] = src_center + src_rightdir
    dst = np.zeros((B, 3, 2), dtype=np.float32)
    dst[:, 0, :] = dst_center
    dst[:, 1, :] = dst_center + dst_downdir
    dst[:, 2, :] = dst_center + dst_rightdir
    return affine_from_3_points(src, dst)


def invert_affine(trans):
    """The patch-pixel -> source-pixel map cv2.warpAffine makes of `trans` (no WARP_INVERSE_MAP): the closed form, float64, [B,2,3]."""
    M = np.array(trans, np.float64)
    D = M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]
    with np.errstate(divide="ignore"):
        D = np.where(D != 0, 1. / D, 0.)
    A11, A22 = M[:, 1, 1] * D, M[:, 0, 0] * D
    out = np.empty_like(M)
    out[:, 0, 0], out[:, 0, 1] = A11, M[:, 0, 1] * -D
    out[:, 1, 0], out[:, 1, 1] = M[:, 1, 0] * -D, A22
    out[:, 0, 2] = -out[:, 0, 0] * M[:, 0, 2] - out[:, 0, 1] * M[:, 1, 2]
    out[:, 1, 2] = -out[:, 1, 0] * M[:, 0, 2] - out[:, 1, 1] * M[:, 1, 2]
    return out


def rotation_matrix_2d(cx, cy, angle_deg, scale=1.0):
    """cv2.getRotationMatrix2D's formula, [B,2,3] float64."""
    a = np.asarray(angle_deg, np.float64) * (np.pi / 180)
    alpha, beta = np.cos(a) * scale, np.sin(a) * scale
    M = np.empty((len(a), 2, 3))
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = alpha, beta, (1 - alpha) * cx - beta * cy
    M[:, 1, 0], M[:, 1, 1], M[:, 1, 2] = -beta, alpha, beta * cx + (1 - alpha) * cy
    return M


def rodrigues_to_matrix(r):
    """cv2.Rodrigues, vector [B,3] -> matrix [B,3,3], float64: R = c I + (1 - c) r r^T + s [r]x with r normalised; I below DBL_EPSILON."""
    r = np.asarray(r, np.float64)
    theta = np.sqrt((r * r).sum(-1))
    small = theta < np.finfo(np.float64).eps
    t = np.where(small, 1.0, theta)
    c, s = np.cos(t), np.sin(t)
    c1 = 1. - c
    u = r / t[:, None]
    rrt = u[:, :, None] * u[:, None, :]
    z = np.zeros(len(r))
    rx = np.stack([z, -u[:, 2], u[:, 1], u[:, 2], z, -u[:, 0], -u[:, 1], u[:, 0], z], -1).reshape(-1, 3, 3)
    R = c[:, None, None] * np.eye(3) + c1[:, None, None] * rrt + s[:, None, None] * rx
    R[small] = np.eye(3)
    return R


def rodrigues_to_vector(R):
    """cv2.Rodrigues, matrix [B,3,3] -> vector [B,3], float64: R is first replaced by the nearest rotation (U V^T of its SVD), then the
    axis comes from the skew part and the angle from acos((trace - 1) / 2); near 0 and near pi by cv2's own branches."""
    R = np.asarray(R, np.float64)
    U, _, Vt = np.linalg.svd(R)
    R = U @ Vt
    r = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], -1)
    s = np.sqrt((r * r).sum(-1) * 0.25)
    c = np.clip((R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1) * 0.5, -1., 1.)
    theta = np.arccos(c)
    out = np.empty_like(r)
    for b in range(len(r)):                                   # (the branches are data dependent; B rows of scalars)
        if s[b] < 1e-5:
            if c[b] > 0:
                out[b] = 0.
            else:
                rx = np.sqrt(max((R[b, 0, 0] + 1) * 0.5, 0.))
                ry = np.sqrt(max((R[b, 1, 1] + 1) * 0.5, 0.)) * (-1. if R[b, 0, 1] < 0 else 1.)
                rz = np.sqrt(max((R[b, 2, 2] + 1) * 0.5, 0.)) * (-1. if R[b, 0, 2] < 0 else 1.)
                if abs(rx) < abs(ry) and abs(rx) < abs(rz) and (R[b, 1, 2] > 0) != (ry * rz > 0):
                    rz = -rz
                v = np.array([rx, ry, rz])
                out[b] = v * (theta[b] / np.sqrt((v * v).sum()))
        else:
            out[b] = r[b] * ((1. / (2 * s[b])) * theta[b])
    return out


def rot_aa(aa, rot):
    """augmentation.py:292-310 over B: the global orientation [B,3] turned by -rot degrees about z, through Rodrigues both ways -> float32."""
    a = np.deg2rad(-np.asarray(rot, np.float64))
    R = np.zeros((len(a), 3, 3))
    R[:, 0, 0], R[:, 0, 1] = np.cos(a), -np.sin(a)
    R[:, 1, 0], R[:, 1, 1] = np.sin(a), np.cos(a)
    R[:, 2, 2] = 1
    per_rdg = rodrigues_to_matrix(aa)
    return rodrigues_to_vector(R @ per_rdg).astype(np.float32)


def _apply_2x3(T, kp):
    """trans_point2d (augmentation.py:107-118) of kp[..., :2] for all joints: np.dot(trans, [x, y, 1.]) in float64, summed in order."""
    x, y = kp[:, :, 0].astype(np.float64), kp[:, :, 1].astype(np.float64)
    return np.stack([T[:, i, None, 0] * x + T[:, i, None, 1] * y + T[:, i, None, 2] * 1. for i in range(2)], -1)


def _z_rotation(v, rot):
    """keypoint_3d_processing / scene_verts_3d_processing's einsum('ij,kj->ki', rot_mat, v) (augmentation.py:251-258), v [B,n,3] float64,
    summed over j in order; rot == 0 keeps the identity matrix.  -> (rotated, cos, sin) with cos, sin of -rot."""
    rot_rad = -rot * np.pi / 180
    hit = rot != 0
    cs, sn = np.where(hit, np.cos(rot_rad), 1.0), np.where(hit, np.sin(rot_rad), 0.0)
    c, s = cs[:, None], sn[:, None]
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([(c * x + (-s) * y) + 0. * z, (s * x + c * y) + 0. * z, (0. * x + 0. * y) + 1. * z], -1), cs, sn


def host_item(aug, center, bbox_size, keypoints_2d, keypoints_3d, smpl_params, fx, cx, cy, img_hw, patch, flip_cam_width=FLIP_CAM_WIDTH):
    """get_example's small per-item arithmetic over B, on the host (augmentation.py:358-362, :386-443, :499-517).  ``aug``: the
    parameter dict of draw_augmentation / no_augmentation.  Returns a dict of numpy arrays: the loader's small outputs (float32 unless
    noted), the kernels' parameter rows ``patch_params`` / ``aug_params`` (float64) and ``keypoints_3d_full_f64`` (for the augmented transl)."""
    H, W = img_hw
    B = len(aug["scale"])
    scale, rot, flip, color, tx, ty = (aug[k] for k in ("scale", "rot", "flip", "color", "tx", "ty"))
    center = np.asarray(center, np.float32).reshape(B, 2)
    width = np.asarray(bbox_size, np.float32).reshape(B)
    fx, cam_cx, cam_cy = (np.asarray(v, np.float64).reshape(B) for v in (fx, cx, cy))
    center_x = center[:, 0] + width * tx                                    # :361-362 (float32 + float32 * float64 -> float64)
    center_y = center[:, 1] + width * ty

    # ---- the crop's map (:143-149) and the full image's rotation about the (flipped) centre (:406-412)
    center_x_auge = np.where(flip, W - center_x - 1, center_x)
    trans = gen_trans_from_patch(center_x_auge, center_y, width, width, patch, patch, scale, rot)
    M = rotation_matrix_2d(center_x_auge, center_y, rot, 1.0)

    # ---- smpl params: flip, then the global orientation turned (:312-326)
    go = np.asarray(smpl_params["global_orient"]).reshape(B, 3).copy()
    bp = np.asarray(smpl_params["body_pose"]).reshape(B, -1).copy()
    if bp.shape[1] != 69:
        raise ValueError(f"smpl_params['body_pose'] has {bp.shape[1]} values per item, expected 69 (axis-angle)")
    go_f, bp_f = go.copy(), bp[:, BODY_POSE_FLIP]
    go_f[:, 1::3] *= -1
    go_f[:, 2::3] *= -1
    bp_f[:, 1::3] *= -1
    bp_f[:, 2::3] *= -1
    go = np.where(flip[:, None], go_f, go).astype(np.float32)
    bp = np.where(flip[:, None], bp_f, bp).astype(np.float32)
    betas = np.asarray(smpl_params["betas"]).reshape(B, -1).astype(np.float32)
    transl = np.asarray(smpl_params["transl"]).reshape(B, 3).astype(np.float32)
    go = rot_aa(go, rot)

    # ---- 2-D keypoints in the crop (:390-401) and in the rotated full image (:500-517)
    kp = np.array(keypoints_2d)
    if not np.issubdtype(kp.dtype, np.floating):
        kp = kp.astype(np.float64)
    if kp.shape != (B, len(FLIP_2D), 3):
        raise ValueError(f"keypoints_2d has shape {kp.shape}, expected ({B}, {len(FLIP_2D)}, 3)")
    kp_f = kp.copy()
    kp_f[:, :, 0] = W - kp_f[:, :, 0] - 1
    kp_f = kp_f[:, FLIP_2D, :]
    kp = np.where(flip[:, None, None], kp_f, kp)
    kp_crop, kp_orig = kp.copy(), kp.copy()
    vis = kp_crop[:, :, -1] > 0
    kp_crop[:, :, 0:2] = _apply_2x3(trans, kp_crop)
    temp = (kp_crop[:, :, 0] >= 0) * (kp_crop[:, :, 0] <= patch) * (kp_crop[:, :, 1] >= 0) * (kp_crop[:, :, 1] <= patch)
    vis = vis * temp
    kp_crop[:, :, :-1] = kp_crop[:, :, :-1] / patch - 0.5
    kp_orig[:, :, 0:2] = _apply_2x3(M, kp_orig)
    kp_orig[:, :, 0] = kp_orig[:, :, 0] / W - 0.5
    kp_orig[:, :, 1] = kp_orig[:, :, 1] / H - 0.5

    # ---- the crop camera (:418-426)
    cam_t_full = transl                                                     # float32 [B,3]
    tz = cam_t_full[:, 2]
    s = 2 * fx / (scale * width) / tz
    delta_x = 2 * (center_x - cam_cx) / (scale * width * s)
    delta_y = 2 * (center_y - cam_cy) / (scale * width * s)
    cam_t_crop = np.stack([cam_t_full[:, 0] - delta_x, cam_t_full[:, 1] - delta_y, scale * width / CROP_CAM_RES * tz], -1)     # float64

    # ---- 3-D keypoints (:427, :433-437; keypoint_3d_processing)
    k3 = np.asarray(keypoints_3d, np.float64)                               # egobody_dataset.py:88: float64
    if k3.shape != (B, len(FLIP_3D), 3):
        raise ValueError(f"keypoints_3d has shape {k3.shape}, expected ({B}, {len(FLIP_3D)}, 3)")
    k3 = k3 - cam_t_full[:, None, :] + cam_t_crop[:, None, :]
    k3_f = k3.copy()
    k3_f[:, :, 0] = 1 - k3_f[:, :, 0] - 1                                   # fliplr_keypoints(..., width = 1, ...)
    k3_f = k3_f[:, FLIP_3D, :]
    k3 = np.where(flip[:, None, None], k3_f, k3)
    k3_crop, cs, sn = _z_rotation(k3, rot)
    k3_crop = k3_crop.astype("float32")                                     # :260
    sign = np.where(flip, -1.0, 1.0)
    t_full2 = cam_t_full.copy()
    t_crop2 = cam_t_crop.copy()
    t_full2[:, 0] = (sign * t_full2[:, 0]).astype(np.float32)               # :434-436
    t_crop2[:, 0] = sign * t_crop2[:, 0]
    k3_full = k3_crop - t_crop2[:, None, :] + t_full2[:, None, :]           # float64

    cam_cx_auge = np.where(flip, flip_cam_width - cam_cx, cam_cx)           # :440-443

    patch_params = np.zeros((B, PATCH_PARAMS))
    patch_params[:, 0:6] = invert_affine(trans).reshape(B, 6)
    patch_params[:, 6] = flip
    patch_params[:, 7:10] = color
    aug_params = np.zeros((B, AUG_PARAMS))
    aug_params[:, 0:3], aug_params[:, 3:6], aug_params[:, 6], aug_params[:, 7], aug_params[:, 8] = cam_t_full, cam_t_crop, flip, cs, sn
    return dict(keypoints_2d=kp_crop.astype(np.float32), orig_keypoints_2d=kp_orig.astype(np.float32), keypoints_2d_vis_mask=vis,
                keypoints_3d=k3_crop.astype(np.float32), keypoints_3d_full=k3_full.astype(np.float32), keypoints_3d_full_f64=k3_full,
                global_orient=go, body_pose=bp, betas=betas, transl=transl,
                box_center=np.stack([center_x_auge, center_y], -1).astype(np.float32), box_size=(width * scale).astype(np.float32),
                cam_cx=cam_cx_auge.astype(np.float32), cam_cy=cam_cy.astype(np.float32),
                trans=trans, M=M, patch_params=patch_params, aug_params=aug_params)


# ---------------------------------------------------------------------------------------------------------------- the two native calls
def image_patch(frames, frame_index, params, patch, mean=IMAGE_MEAN, std=IMAGE_STD, quantize=True, out=None):
    """ehm_image_patch: frames uint8 [F,H,W,3] (BGR), frame_index int32 [B], params float64 [B, PATCH_PARAMS], all on one HIP device
    -> img float32 [B,3,patch,patch]."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames must be uint8 [F,H,W,3], not {frames.dtype} {tuple(frames.shape)}")
    B = int(frame_index.shape[0])
    if frame_index.dtype != torch.int32 or params.dtype != torch.float64 or tuple(params.shape) != (B, PATCH_PARAMS):
        raise ValueError("frame_index must be int32 [B] and params float64 [B, PATCH_PARAMS]")
    dev = frames.device
    img = out if out is not None else torch.empty(B, 3, int(patch), int(patch), dtype=torch.float32, device=dev)
    P = _lib.ptr
    d = _lib.ImagePatchDesc(frames=P(frames), F=frames.shape[0], H=frames.shape[1], W=frames.shape[2], frame_index=P(frame_index), params=P(params),
                            B=B, P=int(patch), quantize=int(bool(quantize)), mean=(C.c_double * 3)(*[float(m) for m in mean]),
                            std=(C.c_double * 3)(*[float(s) for s in std]), img=P(img))
    with _lib.on_device(dev):
        _lib.api().ehm_image_patch(C.byref(d), _lib.stream_ptr())
    return img


def scene_augment(scene, params, stride=1):
    """ehm_scene_augment: scene float32 / float64 [B,N,3], params float64 [B, AUG_PARAMS] on one HIP device -> float32 [B, ceil(N/stride), 3]."""
    if scene.dtype not in (torch.float32, torch.float64) or scene.dim() != 3 or scene.shape[2] != 3:
        raise ValueError(f"scene must be float32 or float64 [B,N,3], not {scene.dtype} {tuple(scene.shape)}")
    B, N = int(scene.shape[0]), int(scene.shape[1])
    if params.dtype != torch.float64 or tuple(params.shape) != (B, AUG_PARAMS):
        raise ValueError("params must be float64 [B, AUG_PARAMS]")
    stride = int(stride)
    out = torch.empty(B, -(-N // max(stride, 1)), 3, dtype=torch.float32, device=scene.device)
    with _lib.on_device(scene.device):
        _lib.api().ehm_scene_augment(scene, int(scene.dtype == torch.float64), params, out, B, N, stride, _lib.stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------------------------- the public builder
class BatchBuilder:
    """The reference loader's batch dict (dataloaders/egobody_dataset.py:241-274) for B items at once, on one HIP device.

    ``smpl_male`` / ``smpl_female``: egohmr_amd.smpl.SMPL modules on the device, needed under augmentation only (the augmented translation is
    the annotated pelvis position minus the gendered model's own pelvis, augmentation.py:446-460).  ``scene_stride``: the loader's
    scene_downsample_rate."""

    def __init__(self, device, img_size=224, mean=IMAGE_MEAN, std=IMAGE_STD, fx_norm_coeff=1500.0, smpl_male=None, smpl_female=None,
                 scene_stride=1, fy_norm_coeff=None, flip_cam_width=FLIP_CAM_WIDTH, augment_config=None, jpeg_threads=8):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.EgoHMRHipError("BatchBuilder runs on the HIP kernels only (got a CPU device); there is no CPU path")
        if int(img_size) < 4 or int(img_size) % 4:
            raise ValueError(f"img_size must be a positive multiple of 4, not {img_size}")
        if int(scene_stride) < 1:
            raise ValueError(f"scene_stride must be >= 1, not {scene_stride}")
        self.device, self.img_size, self.scene_stride = device, int(img_size), int(scene_stride)
        self.mean, self.std = np.asarray(mean, np.float64).reshape(3), np.asarray(std, np.float64).reshape(3)
        self.fx_norm_coeff = fx_norm_coeff
        self.fy_norm_coeff = fx_norm_coeff if fy_norm_coeff is None else fy_norm_coeff
        self.smpl_male, self.smpl_female = smpl_male, smpl_female
        self.flip_cam_width = flip_cam_width
        self.augment_config = augment_config if augment_config is not None else AugmentConfig()
        self.quantize = True
        self.jpeg_threads, self._jpeg = jpeg_threads, None          # the decoder of encoded frames, made at their first use

    def _decoded(self, frames):
        """Encoded frames (a sequence of JPEG bytes / paths) -> uint8 [F,H,W,3] on the device; anything else passes through."""
        if isinstance(frames, (list, tuple)) and len(frames) and all(isinstance(f, (bytes, bytearray, memoryview, str, os.PathLike)) for f in frames):
            if self._jpeg is None:
                from .jpeg import JpegDecoder
                self._jpeg = JpegDecoder(self.device, threads=self.jpeg_threads)
            return self._jpeg.decode(frames)
        return frames

    def _device_tensor(self, x, dtypes, name):
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        if t.dtype not in dtypes:
            raise ValueError(f"{name} has dtype {t.dtype}, expected one of {[str(d) for d in dtypes]}")
        return t.to(self.device).contiguous()

    def build(self, frames, frame_index, center, bbox_size, keypoints_2d, keypoints_3d, smpl_params, gender, fx, fy, cx, cy, scene, augment=None):
        """``frames`` uint8 [F,H,W,3] BGR as decoded - or a sequence of F encoded baseline-JPEG frames, ``bytes`` or paths, decoded here - and ``scene`` [B,N,3] float32 / float64 in the PV camera (numpy, or tensors already on the
        device: SceneClouds output); ``frame_index`` [B]; ``center`` [B,2], ``bbox_size`` [B] (scale * 200); ``keypoints_2d`` [B,25,3];
        ``keypoints_3d`` [B,24,3]; ``smpl_params`` with global_orient [B,3], body_pose [B,69], betas [B,10], transl [B,3]; ``gender`` [B]
        (0 male, 1 female); ``fx, fy, cx, cy`` [B].  ``augment``: None (the test loader), 'draw' (draw_augmentation on the global generators) or
        a dict of per-item parameters (scale, rot, flip, color [B,3], tx, ty)."""
        fidx = np.asarray(frame_index.detach().cpu().numpy() if isinstance(frame_index, torch.Tensor) else frame_index).reshape(-1)
        B = len(fidx)
        if B == 0:
            raise ValueError("empty batch")
        frames_d = self._device_tensor(self._decoded(frames), (torch.uint8,), "frames")
        if frames_d.dim() != 4 or frames_d.shape[3] != 3:
            raise ValueError(f"frames has shape {tuple(frames_d.shape)}, expected [F,H,W,3]")
        F, H, W = (int(v) for v in frames_d.shape[:3])
        if not np.issubdtype(fidx.dtype, np.integer) or fidx.min() < 0 or fidx.max() >= F:
            raise ValueError(f"frame_index must hold integers in [0, {F})")
        scene_d = self._device_tensor(scene, (torch.float32, torch.float64), "scene")
        if scene_d.dim() != 3 or scene_d.shape[0] != B or scene_d.shape[2] != 3:
            raise ValueError(f"scene has shape {tuple(scene_d.shape)}, expected [{B},N,3]")
        augmented = augment is not None
        if augment is None:
            aug = no_augmentation(B)
        elif isinstance(augment, str):
            if augment != "draw":
                raise ValueError(f"augment must be None, 'draw' or a dict of per-item parameters, not {augment!r}")
            aug = draw_augmentation(self.augment_config, B)
        else:
            aug = _check_augmentation(augment, B)
        gender = np.asarray(gender.detach().cpu().numpy() if isinstance(gender, torch.Tensor) else gender).reshape(-1)
        if gender.shape != (B,):
            raise ValueError(f"gender has {gender.size} values, expected {B}")
        if augmented:
            if self.smpl_male is None or self.smpl_female is None:
                raise ValueError("augmentation needs smpl_male and smpl_female (the augmented transl is the pelvis of the gendered SMPL model)")
            if not np.isin(gender, (0, 1)).all():
                raise ValueError("gender must be 0 (male) or 1 (female) under augmentation")
        h = host_item(aug, center, bbox_size, keypoints_2d, keypoints_3d, smpl_params, fx, cx, cy, (H, W), self.img_size, self.flip_cam_width)
        self.last_augmentation = aug

        # one upload: the kernels' parameter rows and the float64 pelvis annotation | one upload: every small float32 output
        dev = self.device
        rows = torch.from_numpy(np.concatenate([h["patch_params"], h["aug_params"], h["keypoints_3d_full_f64"][:, 0, :]], 1)).to(dev)
        patch_params, aug_params = rows[:, :PATCH_PARAMS].contiguous(), rows[:, PATCH_PARAMS:PATCH_PARAMS + AUG_PARAMS].contiguous()
        small = dict(keypoints_2d=h["keypoints_2d"], orig_keypoints_2d=h["orig_keypoints_2d"], keypoints_3d=h["keypoints_3d"],
                     keypoints_3d_full=h["keypoints_3d_full"], global_orient=h["global_orient"], body_pose=h["body_pose"], betas=h["betas"],
                     transl=h["transl"], box_center=h["box_center"], box_size=h["box_size"], cam_cx=h["cam_cx"], cam_cy=h["cam_cy"],
                     fx=(np.asarray(fx, np.float64).reshape(B) / self.fx_norm_coeff).astype(np.float32),
                     fy=(np.asarray(fy, np.float64).reshape(B) / self.fy_norm_coeff).astype(np.float32))
        flat = torch.from_numpy(np.concatenate([v.reshape(B, -1) for v in small.values()], 1)).to(dev)
        t, col = {}, 0
        for k, v in small.items():
            n = v.reshape(B, -1).shape[1]
            t[k] = flat[:, col:col + n].reshape(v.shape).contiguous()
            col += n
        img = image_patch(frames_d, torch.from_numpy(fidx.astype(np.int32)).to(dev), patch_params, self.img_size, self.mean, self.std, self.quantize)
        scene_out = scene_augment(scene_d, aug_params, self.scene_stride)

        if augmented:                                                       # :446-460
            pelvis = torch.empty(B, 3, dtype=torch.float32, device=dev)
            with torch.no_grad():
                for g, model in ((0, self.smpl_male), (1, self.smpl_female)):
                    sel = np.nonzero(gender == g)[0]
                    if len(sel):
                        i = torch.from_numpy(sel).to(dev)
                        o = model(global_orient=t["global_orient"][i], body_pose=t["body_pose"][i], betas=t["betas"][i], return_verts=False)
                        pelvis[i] = o.joints[:, 0]
            t["transl"] = (rows[:, PATCH_PARAMS + AUG_PARAMS:] - pelvis.double()).float()

        ones = lambda: torch.ones(B, dtype=torch.bool)                      # the flag dicts stay on the host, as the loader's do
        return {
            "img": img,
            "keypoints_2d": t["keypoints_2d"], "orig_keypoints_2d": t["orig_keypoints_2d"],
            "keypoints_2d_vis_mask": torch.from_numpy(h["keypoints_2d_vis_mask"]).to(dev),
            "keypoints_3d": t["keypoints_3d"], "keypoints_3d_full": t["keypoints_3d_full"],
            "smpl_params": {k: t[k] for k in ("global_orient", "transl", "body_pose", "betas")},
            "has_smpl_params": {k: ones() for k in ("global_orient", "transl", "body_pose", "betas")},
            "smpl_params_is_axis_angle": {"global_orient": ones(), "transl": ~ones(), "body_pose": ones(), "betas": ~ones()},
            "gender": torch.from_numpy(gender.astype(np.int32)).to(dev),
            "fx": t["fx"], "fy": t["fy"], "cam_cx": t["cam_cx"], "cam_cy": t["cam_cy"],
            "box_center": t["box_center"], "box_size": t["box_size"],
            "scene_pcd_verts_full": scene_out,
        }
