"""Plain numpy restatements of the small per-item kernels, for tests/test_prep_pack_cpu.py and tests/test_gpu_prep_pack.py (no GPU, no package import):

  item_prep_ref / pass_map_ref   csrc/prep.hip ehm_item_prep    (models/egohmr/egohmr.py:186-188, :195-205, :217, :249-254)
  pack_ref                       csrc/prep.hip ehm_pack_outputs (egohmr.py:283-301, utils/geometry.py:78-116)
  ddpm_step_ref / ddim_step_ref  csrc/sampler.hip               (diffusion/gaussian_diffusion.py:217-220, :286-290, :333-336, :539-555)
  grad_finish_ref                csrc/guidance.hip              (egohmr.py:561-570)

Where the device chain is made of correctly rounded IEEE float32 operations only (+ - * /), the restatement performs the same operations on
numpy float32 arrays, one rounding per operation, and the comparison is bit for bit (`same_bits`: NaN equals NaN).  Where the device uses
fused multiply-adds (TranslEnc) or expf (the DDPM step), the restatement is float64 and comes with a derived per-element bound."""
import numpy as np

F32 = np.float32
POSE_DIM, NJ = 144, 24
OPENPOSE_TO_SMPL = [8, 12, 9, 8, 13, 10, 8, 14, 11, 8, 14, 11, 0, 5, 2, 0, 5, 2, 6, 3, 7, 4, 7, 4]    # egohmr.py:111
OPENPOSE_TO_SMPL_LOOSE = [8, 13, 10, 8, 13, 10, 8, 14, 11, 8, 14, 11, 1, 5, 2, 0, 5, 2, 6, 3, 7, 4, 7, 4]  # egohmr.py:114 (pelvis_vis_loosen)
GRAD_X1, GRAD_X2 = (1, 2), (4, 5, 7, 8, 10, 11)                                                       # egohmr.py:562-567: every other joint is zeroed


def same_bits(a, b):
    """Elementwise: equal bit patterns, or both NaN (a NaN's payload is not part of any contract here)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _f32(a):
    return None if a is None else np.asarray(a, F32)


# ------------------------------------------------------------------------------------------------ ehm_item_prep
def item_prep_ref(kp, joint_map, force_visible, transl, fx, fx_norm, tW1, tb1, tW2, tb2, other_ld, other_col0, cx=None, cy=None, box_center=None,
                  box_size=None, with_cam_center=False, with_bbox=False, img_rowsum=None, scene_rowsum=None, hidden_units=None):
    """kp [B,NK,3], joint_map [24], transl [B,3], fx (cx, cy, box_size) [B], box_center [B,2]; torch [out,in] TranslEnc weights.
    Returns a dict:
      vis [B,24] u8, need [B] bool, finite [B] u8
      transl_enc [B,t_out] float64 and transl_bound [B,t_out]: |device - transl_enc| <= transl_bound (see below)
      cam [B, other_ld - other_col0 - t_out] float32: the camera columns, then the zero fill up to other_ld
    hidden_units: use only the first that many hidden units (the tests drop one to show that the bound can tell a wrong kernel)."""
    kp, transl, fx = _f32(kp), _f32(transl), _f32(fx)
    jm = np.asarray(joint_map, np.int64)
    B = kp.shape[0]
    vis = (jm[None, :] == force_visible) | (kp[:, jm, 2] > 0)                                        # :186-188
    # TranslEnc (:217): Linear(3, t_hidden) -> ReLU -> Linear(t_hidden, t_out) in float64
    W1, b1, W2, b2 = (np.asarray(w, np.float64) for w in (tW1, tb1, tW2, tb2))
    t_hidden, t_out = W1.shape[0], W2.shape[0]
    H = t_hidden if hidden_units is None else hidden_units
    with np.errstate(all="ignore"):
        t64 = transl.astype(np.float64)
        hid = np.maximum(t64 @ W1[:H].T + b1[:H], 0.0)
        enc = hid @ W2[:, :H].T + b2
        # The device evaluates each unit as a chain of float32 FMAs (3 for a hidden unit, t_hidden for an output).  A chain of n FMAs onto a bias
        # is within n 2^-24 (1 + O(2^-24)) of the exact sum, relative to the sum of the magnitudes of its terms; the hidden values carry their own
        # 3 2^-24 into the second layer (ReLU is 1-Lipschitz).  (t_hidden + 3) 2^-24 (|b2| + sum |W2| (|b1| + |W1| |t|)) in all, to first order;
        # 2^-23 (t_hidden + 8) leaves more than a factor of two for the higher-order terms.
        mag = np.abs(b2) + (np.abs(b1) + np.abs(t64) @ np.abs(W1).T) @ np.abs(W2).T
    bound = 2.0 ** -23 * (t_hidden + 8) * mag
    # camera columns (:195-205), float32 operation by operation in the kernel's order
    with np.errstate(all="ignore"):
        ofx = fx * F32(fx_norm)
        cols = []
        if with_cam_center:
            cols += [_f32(cx) / ofx, _f32(cy) / ofx]
        if with_bbox:
            bc = _f32(box_center)
            cols += [bc[:, 0] / ofx, bc[:, 1] / ofx, _f32(box_size) / ofx]
        cols.append(fx)
    cam = np.zeros((B, other_ld - other_col0 - t_out), F32)
    assert cam.shape[1] >= len(cols)
    for i, c in enumerate(cols):
        cam[:, i] = c
    # finite: every COMPONENT that is read, and the given row sums
    ok = np.isfinite(transl).all(axis=1) & np.isfinite(fx)
    if with_cam_center:
        ok &= np.isfinite(_f32(cx)) & np.isfinite(_f32(cy))
    if with_bbox:
        ok &= np.isfinite(_f32(box_center)).all(axis=1) & np.isfinite(_f32(box_size))
    for s in (img_rowsum, scene_rowsum):
        if s is not None:
            ok &= np.isfinite(_f32(s))
    return {"vis": vis.astype(np.uint8), "need": ~vis.all(axis=1), "finite": ok.astype(np.uint8), "transl_enc": enc, "transl_bound": bound, "cam": cam}


def pass_map_ref(need, group=1):
    """-> mask_slot [B] int32 (slot among the items that need the second pass, ascending; -1: none), mask_items [count] int32, count."""
    need = np.asarray(need, bool)
    B = need.shape[0]
    n = np.array([need[b // group * group: min(b // group * group + group, B)].any() for b in range(B)], bool)
    items = np.flatnonzero(n).astype(np.int32)
    slot = np.full(B, -1, np.int32)
    slot[items] = np.arange(items.size, dtype=np.int32)
    return slot, items, int(items.size)


# ------------------------------------------------------------------------------------------------ ehm_pack_outputs
def pack_ref(x0, pose6d, R, verts, joints, betas_in, transl, fx, cx, cy, fx_norm, finite=None, chk=None, last_noise=None, x_final=None):
    """The inputs as the kernel finds them (x0, pose6d [B,144]; R [B,24,9]; verts [B,V,3]; joints [B,J,3]; betas_in [B,10]; transl [B,3]; fx, cx, cy [B];
    finite [B] or None; chk [rows,B,144] or None; last_noise, x_final [B,144] or None).  Returns every buffer the kernel writes, as it leaves it."""
    x0, pose6d, R, verts, joints = (_f32(a).copy() for a in (x0, pose6d, R, verts, joints))
    transl, fx, cx, cy = _f32(transl), _f32(fx), _f32(cx), _f32(cy)
    B = x0.shape[0]
    R = R.reshape(B, NJ, 9)
    bad = np.zeros(B, bool)                                                                          # header of ehm_pack_desc
    if finite is not None:
        bad |= np.asarray(finite).astype(np.uint8) == 0
    if chk is not None:
        bad |= ~np.isfinite(_f32(chk)).all(axis=(0, 2))
    out = {"finite_out": (~bad).astype(np.uint8)}
    if x_final is not None:
        xf = _f32(x_final).copy()
        poison = np.repeat(bad[:, None], POSE_DIM, axis=1)
        if last_noise is not None:
            poison |= ~np.isfinite(_f32(last_noise))                                                 # gaussian_diffusion.py:357-359: 0 * draw
        xf[poison] = np.nan
        out["x_final"] = xf
    for a in (x0, pose6d, R, verts, joints):
        a[bad] = np.nan
    betas = _f32(betas_in).copy()
    betas[bad] = np.nan
    out.update(x0=x0, pose6d=pose6d, R=R, verts=verts, joints=joints, betas_out=betas, global_orient=R[:, :1].copy(), body_pose=R[:, 1:].copy())
    with np.errstate(all="ignore"):
        f = fx * F32(fx_norm)                                                                        # :283-285
        out["focal"] = np.stack([f, f], axis=1)
        out["center"] = np.stack([cx, cy], axis=1)                                                   # :286
        p = joints + transl[:, None, :]                                                              # :294, geometry.py:108
        q = p / p[:, :, 2:3]                                                                         # geometry.py:111 (p.z / p.z included)
        u = f[:, None] * q[:, :, 0] + cx[:, None] * q[:, :, 2]                                       # geometry.py:114, K = [[f, 0, cx], [0, f, cy], [0, 0, 1]]
        v = f[:, None] * q[:, :, 1] + cy[:, None] * q[:, :, 2]
        out["kp3d_full"] = p
        out["kp2d_full"] = np.stack([u / F32(1920.0) - F32(0.5), v / F32(1080.0) - F32(0.5)], axis=2)   # :299-300
    assert all(a.dtype == F32 for k, a in out.items() if k != "finite_out")
    return out


# ------------------------------------------------------------------------------------------------ sampler steps
def ddpm_step_ref(x, x0, noise, grad, coef1, coef2, log_variance, nonzero, grad_scale):
    """float64 on the float32 coefficients the entry point is handed -> (x_next, bound): |device - x_next| <= bound per element.
    The device rounds four products and up to three sums (each within 2^-24 of a value no larger than the sum of the terms' magnitudes) and takes
    expf of an exactly halved log variance (a few ulp): 8 2^-24 (|c1 x0| + |c2 x| + |g grad| + |nz sd noise|) covers them."""
    c1, c2, lv, nz, gs = (float(F32(v)) for v in (coef1, coef2, log_variance, nonzero, grad_scale))
    x, x0, noise = (np.asarray(a, F32).astype(np.float64) for a in (x, x0, noise))
    sd = np.exp(0.5 * lv)
    with np.errstate(all="ignore"):
        terms = [c1 * x0, c2 * x] + ([gs * np.asarray(grad, F32).astype(np.float64)] if grad is not None else []) + [nz * sd * noise]
        out = sum(terms[1:], terms[0])
        bound = 8 * 2.0 ** -24 * sum((np.abs(t) for t in terms[1:]), np.abs(terms[0]))
    return out, bound


def ddim_step_ref(x, x0, noise, sqrt_recip_ac, sqrt_recipm1_ac, sqrt_ac_prev, dir_coef, sigma, nonzero):
    """float32, one rounding per operation, in the kernel's order (bit for bit)."""
    sr, srm1, sap, dr, sg, nz = (F32(v) for v in (sqrt_recip_ac, sqrt_recipm1_ac, sqrt_ac_prev, dir_coef, sigma, nonzero))
    x, x0, noise = (np.asarray(a, F32) for a in (x, x0, noise))
    with np.errstate(all="ignore"):
        eps = (sr * x - x0) / srm1                                                                   # :286-290
        mean = x0 * sap + dr * eps                                                                   # :548-551
        return mean + (nz * sg) * noise                                                              # :555


# ------------------------------------------------------------------------------------------------ ehm_guidance_grad_finish
def grad_finish_ref(gpose6d, denom):
    """[B,144] float32: -g / denom * scale on joints {1, 2} (x 1) and {4, 5, 7, 8, 10, 11} (x 2), +0 on every other joint (bit for bit)."""
    g = np.asarray(gpose6d, F32).reshape(-1, NJ, 6)
    out = np.zeros_like(g)
    with np.errstate(all="ignore"):
        for joints, scale in ((GRAD_X1, 1.0), (GRAD_X2, 2.0)):
            for j in joints:
                out[:, j] = -g[:, j] / F32(denom) * F32(scale)
    return out.reshape(-1, POSE_DIM)
