"""ctypes binding of libegohmr_hip.so (C ABI: include/egohmr_hip.h).

The library is the product: there is no eager / CPU fallback.  If it is missing or cannot be
loaded this module raises - loudly - at first use.

``lib()`` is the raw C contract: every entry point returns its rc / size / string and never throws.  ``api()`` is the package's
convention: a ``torch.Tensor`` in any argument position is validated by ``ptr()`` (HIP device, contiguous) and passed as its address;
a status function raises on a nonzero rc, one of ``VALUE_FUNCTIONS`` on a negative one and otherwise returns it (``EgoHMRRangeError``
for rc -34, ``EgoHMRHipError`` else).  Opaque native objects (the denoiser, the SMPL model) are owned by a ``Handle``.

``import torch`` happens before the dlopen on purpose: PyTorch-ROCm ships its own
``libamdhip64.so`` (SONAME libamdhip64.so.7, same as /opt/rocm's) and the dynamic loader then
binds our library to that already-loaded runtime, so device pointers / streams handed over
from torch tensors are valid inside the kernels' launches.
"""
from __future__ import annotations

import ctypes as C
import glob
import itertools
import os
import subprocess
import sys
from types import SimpleNamespace

import torch  # noqa: F401  (must precede the dlopen, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EHM_LIB_PATH") or os.path.join(_HERE, "libegohmr_hip.so")   # EHM_LIB_PATH: A/B a second build (experiments)
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
SOURCES = ["gcn.hip", "gcn_tile.hip", "linear.hip", "conv.hip", "stem.hip", "metrics.hip", "smpl.hip", "sampler.hip", "guidance.hip", "prep.hip", "step.hip", "eval.hip", "stage1.hip", "scene.hip", "loss.hip", "gcn_bwd.hip", "gcn_train.hip", "pointnet_bwd.hip", "train.hip", "conv_bwd.hip", "bn2d_train.hip", "nonlocal_bwd.hip", "batch.hip", "render.hip", "mesh_collision.hip", "jpeg.hip", "jpeg_enc.hip", "flow.hip"]


class EgoHMRHipError(RuntimeError):
    def __init__(self, msg="", rc=None, function=None):        # rc, function: the failed entry point's (None: not a native call's error)
        super().__init__(msg)
        self.rc, self.function = rc, function


class EgoHMRRangeError(EgoHMRHipError):
    """rc = -34: an activation of the denoiser reached the f16 range and was clamped in its X2 / f16 store (ehm_gcn_stack_status).  The results are finite
    but not parity grade; the remedy is float32 activations for that checkpoint: EgoHMR.gcn_precision = 'f32' (EgoHMR.on_saturation = 'f32' does it
    and re-runs the call)."""


def build(verbose: bool = False, force: bool = False) -> str:
    """Compile the gfx950 library in-tree with hipcc (cross-compiles without a GPU): one object per source, the sources in parallel, objects
    kept under egohmr_amd/build/ and reused while neither their source, a header nor the flags changed."""
    import hashlib
    from concurrent.futures import ThreadPoolExecutor
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = os.environ.get("EHM_HIPCC_FLAGS", "").split()   # e.g. -DEHM_STAMPS (tools/stamp_*.py)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{INCLUDE}", f"-I{CSRC}", *extra]
    hdrs = glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(INCLUDE, "egohmr_hip.h")]   # every header: an edit of any of them rebuilds every object
    hdr_time = max(os.path.getmtime(h) for h in hdrs)
    tag = hashlib.sha1(" ".join([hipcc] + flags).encode()).hexdigest()[:10]
    objdir = os.path.join(_HERE, "build", os.path.basename(LIB_PATH) + "." + tag)
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    sources = SOURCES
    for s in sources:
        src, obj = os.path.join(CSRC, s), os.path.join(objdir, s.replace(".hip", ".o"))
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), hdr_time):
            jobs.append((src, obj))
    objs = [os.path.join(objdir, s.replace(".hip", ".o")) for s in sources]
    # every flag set links into the same LIB_PATH: the tag of the object directory the library was linked from is kept beside it, and a library
    # linked from ANOTHER flag set (say -DEHM_STAMPS, then a default build whose objects were already up to date) is relinked, never reused
    tag_path = LIB_PATH + ".tag"
    linked_tag = open(tag_path).read().strip() if os.path.exists(tag_path) else None
    if not jobs and os.path.exists(LIB_PATH) and linked_tag == tag and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(o) for o in objs):
        return LIB_PATH

    def compile_one(job):
        cmd = [hipcc, *flags, "-c", job[0], "-o", job[1]]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        return subprocess.run(cmd, capture_output=True, text=True)

    with ThreadPoolExecutor(max_workers=int(os.environ.get("EHM_BUILD_JOBS", min(len(jobs) or 1, os.cpu_count() or 1)))) as ex:
        for (src, _), r in zip(jobs, ex.map(compile_one, jobs)):
            if r.returncode != 0:
                raise EgoHMRHipError(f"hipcc failed on {src}:\n{r.stdout}\n{r.stderr}")
            if "failed to meet occupancy target" in r.stderr:
                # __launch_bounds__(256, 2) is a wish, not a limit: a kernel that lost its second block per CU still compiles (with this warning) and
                # every test stays green at half the speed - the host-side plans count on the occupancy, so treat it as a build error
                os.remove(os.path.join(objdir, os.path.basename(src).replace(".hip", ".o")))
                raise EgoHMRHipError(f"hipcc: a kernel of {src} missed its occupancy target:\n{r.stderr}")
    cmd = [hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", *objs, "-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise EgoHMRHipError(f"hipcc (link) failed:\n{r.stdout}\n{r.stderr}")
    with open(tag_path, "w") as f:
        f.write(tag + "\n")
    return LIB_PATH


def build_features() -> set:
    """Optional parts the loaded library was built with (ehm_build_features): 'stamps'."""
    return set(lib().ehm_build_features().decode().split())


class GConvParams(C.Structure):
    """ehm_gconv_params"""
    _fields_ = [("W", C.c_void_p), ("M", C.c_void_p), ("adj2", C.c_void_p), ("bias", C.c_void_p),
                ("bn_weight", C.c_void_p), ("bn_bias", C.c_void_p), ("bn_mean", C.c_void_p), ("bn_var", C.c_void_p),
                ("in_dim", C.c_int), ("out_dim", C.c_int)]


class LinearDesc(C.Structure):
    """ehm_linear_desc"""
    _fields_ = [("A0", C.c_void_p), ("A1", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("group_bias", C.c_void_p),
                ("Y", C.c_void_p), ("colmax", C.c_void_p), ("M", C.c_int64), ("N", C.c_int), ("K0", C.c_int), ("K1", C.c_int),
                ("rows_per_group", C.c_int), ("valid_rows_per_group", C.c_int), ("relu_in0", C.c_int), ("relu_out", C.c_int),
                ("w_scale", C.c_float), ("lift_points", C.c_void_p), ("lift_W4", C.c_void_p), ("hi_only", C.c_int), ("group_bias_stride", C.c_int)]


class ConvDesc(C.Structure):
    """ehm_conv_desc"""
    _fields_ = [("x", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("residual", C.c_void_p), ("y", C.c_void_p),
                ("N", C.c_int), ("H", C.c_int), ("Wd", C.c_int), ("Ci", C.c_int), ("Co", C.c_int),
                ("KH", C.c_int), ("KW", C.c_int), ("stride", C.c_int), ("pad", C.c_int), ("relu", C.c_int),
                ("w_scale", C.c_float)]


class ConvX2Desc(C.Structure):
    """ehm_conv_x2_desc"""
    _fields_ = [("x", C.c_void_p), ("x_rows", C.c_int64), ("W", C.c_void_p), ("bias", C.c_void_p), ("residual", C.c_void_p), ("y", C.c_void_p),
                ("N", C.c_int), ("H", C.c_int), ("Wd", C.c_int), ("Ci", C.c_int), ("Co", C.c_int),
                ("KH", C.c_int), ("KW", C.c_int), ("stride", C.c_int), ("pad", C.c_int), ("relu", C.c_int),
                ("w_scale", C.c_float), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("x2", C.c_void_p), ("x2_rows", C.c_int64), ("H2", C.c_int), ("W2", C.c_int), ("Ci2", C.c_int), ("stride2", C.c_int), ("hi_only", C.c_int),
                ("workspace_clean", C.c_int)]


class EvalPointsDesc(C.Structure):
    """ehm_eval_points_desc"""
    _fields_ = [("pred", C.c_void_p), ("gt", C.c_void_p), ("pred_origin", C.c_void_p), ("gt_origin", C.c_void_p), ("mask", C.c_void_p),
                ("per_point", C.c_void_p), ("mean", C.c_void_p), ("vis_sum", C.c_void_p), ("invis_sum", C.c_void_p),
                ("B", C.c_int), ("S", C.c_int), ("P", C.c_int), ("pred_points", C.c_int), ("gt_points", C.c_int), ("origin_point", C.c_int)]


class ItemPrepDesc(C.Structure):
    """ehm_item_prep_desc"""
    _fields_ = [("keypoints_2d", C.c_void_p), ("joint_map", C.c_void_p), ("NK", C.c_int), ("force_visible", C.c_int),
                ("fx", C.c_void_p), ("cx", C.c_void_p), ("cy", C.c_void_p), ("box_center", C.c_void_p), ("box_size", C.c_void_p), ("transl", C.c_void_p),
                ("fx_norm", C.c_float), ("with_bbox", C.c_int), ("with_cam_center", C.c_int),
                ("tW1", C.c_void_p), ("tb1", C.c_void_p), ("tW2", C.c_void_p), ("tb2", C.c_void_p), ("t_hidden", C.c_int), ("t_out", C.c_int),
                ("img_rowsum", C.c_void_p), ("scene_rowsum", C.c_void_p), ("other", C.c_void_p), ("other_ld", C.c_int), ("other_col0", C.c_int),
                ("vis", C.c_void_p), ("mask_slot", C.c_void_p), ("mask_items", C.c_void_p), ("count", C.c_void_p), ("finite", C.c_void_p),
                ("need_scratch", C.c_void_p), ("pass_group", C.c_int), ("B", C.c_int), ("need_all", C.c_int)]


class PackDesc(C.Structure):
    """ehm_pack_desc"""
    _fields_ = [("B", C.c_int), ("J", C.c_int), ("V", C.c_int), ("finite", C.c_void_p), ("chk", C.c_void_p), ("chk_rows", C.c_int),
                ("last_noise", C.c_void_p), ("x_final", C.c_void_p), ("x0", C.c_void_p), ("pose6d", C.c_void_p), ("R", C.c_void_p),
                ("verts", C.c_void_p), ("joints", C.c_void_p), ("betas_in", C.c_void_p), ("betas_out", C.c_void_p),
                ("transl", C.c_void_p), ("fx", C.c_void_p), ("cx", C.c_void_p), ("cy", C.c_void_p), ("fx_norm", C.c_float),
                ("global_orient", C.c_void_p), ("body_pose", C.c_void_p), ("kp3d_full", C.c_void_p), ("kp2d_full", C.c_void_p),
                ("focal", C.c_void_p), ("center", C.c_void_p), ("finite_out", C.c_void_p)]


class ValLossesDesc(C.Structure):
    """ehm_val_losses_desc"""
    _fields_ = ([(n, C.c_int) for n in ("B", "V", "pred_joints", "gt_joints", "kp3d_points", "kp3d_full_points", "kp2d_points")] +
                [(n, C.c_void_p) for n in ("pred_vertices", "pred_keypoints_3d", "pred_keypoints_3d_full", "pred_keypoints_2d_full",
                                           "pred_global_orient", "pred_body_pose", "pred_betas", "pred_pose_6d",
                                           "keypoints_2d", "keypoints_3d", "keypoints_3d_full",
                                           "gt_vertices_male", "gt_vertices_female", "gt_joints_male", "gt_joints_female", "gender",
                                           "gt_global_orient", "gt_body_pose", "gt_betas", "focal", "center", "penetration")] +
                [("weights", C.c_double * 9), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)] +
                [(n, C.c_void_p) for n in ("losses", "joint_vis_num", "per_item", "per_item_vis", "vis_mask")])


class ValLossesBwdDesc(C.Structure):
    """ehm_val_losses_bwd_desc"""
    INPUTS = ("pred_vertices", "pred_keypoints_3d", "pred_keypoints_3d_full", "pred_keypoints_2d_full", "pred_global_orient", "pred_body_pose",
              "pred_betas", "pred_pose_6d", "keypoints_2d", "keypoints_3d", "keypoints_3d_full", "gt_vertices_male", "gt_vertices_female",
              "gt_joints_male", "gt_joints_female", "gender", "gt_global_orient", "gt_body_pose", "gt_betas", "focal", "center")
    PREDICTIONS = INPUTS[:8]          # the arrays with a gradient, in the order of the g_* outputs
    _fields_ = ([(n, C.c_int) for n in ("B", "V", "pred_joints", "gt_joints", "kp3d_points", "kp3d_full_points", "kp2d_points")] +
                [(n, C.c_void_p) for n in INPUTS + ("gloss",)] +
                [("weights", C.c_double * 9), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)] +
                [("g_" + n, C.c_void_p) for n in PREDICTIONS + ("penetration",)])


# columns of ehm_val_losses' per_item / losses = the keys of the reference's `losses` dict in its order (egohmr.py:432-443; EHM_LOSS_* of the header)
LOSS_KEYS = ("loss", "loss_v2v", "loss_keypoints_3d", "loss_keypoints_3d_full", "loss_keypoints_2d_full", "loss_betas", "loss_body_pose",
             "loss_global_orient", "loss_pose_6d_ortho", "loss_coap_penetration", "loss_keypoints_3d_vis_batch_sum")


GCN_CONV_INPUT, GCN_CONV_OUTPUT = -1, -2        # EHM_GCN_CONV_* of the header: how the backward entries address a conv (hidden convs: their index)


class StepCoefs(C.Structure):
    """ehm_step_coefs"""
    _fields_ = [(n, C.c_float) for n in ("coef1", "coef2", "log_variance", "variance", "sqrt_recip_ac", "sqrt_recipm1_ac",
                                         "sqrt_ac_prev", "dir_coef", "sigma", "nonzero", "grad_scale")]


class NonlocalParams(C.Structure):
    """ehm_nonlocal_params"""
    _fields_ = [("Wqkv", C.c_void_p), ("bqkv", C.c_void_p), ("qkv_scale", C.c_float), ("Wo", C.c_void_p), ("bo", C.c_void_p), ("o_scale", C.c_float),
                ("Ci", C.c_int)]


class SampleDesc(C.Structure):
    """ehm_sample_desc"""
    _fields_ = [("B", C.c_int), ("passes", C.c_int), ("num_steps", C.c_int), ("ddim", C.c_int), ("lbs_every_step", C.c_int),
                ("num_scene_points", C.c_int), ("guide_denom", C.c_float), ("tau", C.c_float), ("num_masked", C.c_int), ("guide_all_points", C.c_int), ("lowprec_steps", C.c_int), ("nonlocal_ci", C.c_int), ("per_step_launches", C.c_int), ("twoterm_steps", C.c_int)]


class Stage1Desc(C.Structure):
    """ehm_stage1_desc"""
    _fields_ = [("img_feats", C.c_void_p), ("scene_feats", C.c_void_p), ("fx", C.c_void_p), ("cam_cx", C.c_void_p), ("cam_cy", C.c_void_p),
                ("box_center", C.c_void_p), ("box_size", C.c_void_p), ("W1t", C.c_void_p), ("b1", C.c_void_p), ("W2", C.c_void_p), ("b2", C.c_void_p),
                ("init_cam", C.c_void_p), ("init_betas", C.c_void_p), ("pred_cam", C.c_void_p), ("pred_cam_full", C.c_void_p), ("pred_betas", C.c_void_p),
                ("fx_norm", C.c_float), ("crop_res", C.c_float), ("with_cam_center", C.c_int), ("with_bbox_info", C.c_int), ("with_focal_length", C.c_int),
                ("img_dim", C.c_int), ("scene_dim", C.c_int), ("hidden", C.c_int), ("B", C.c_int)]


class FlowContextDesc(C.Structure):
    """ehm_flow_context_desc"""
    _fields_ = [("img_feats", C.c_void_p), ("scene_feats", C.c_void_p), ("fx", C.c_void_p), ("cam_cx", C.c_void_p), ("cam_cy", C.c_void_p),
                ("box_center", C.c_void_p), ("box_size", C.c_void_p), ("out", C.c_void_p), ("fx_norm", C.c_float), ("with_cam_center", C.c_int),
                ("with_bbox_info", C.c_int), ("with_focal_length", C.c_int), ("img_dim", C.c_int), ("scene_dim", C.c_int), ("ctx_pad", C.c_int), ("B", C.c_int)]


class FlowGemmDesc(C.Structure):
    """ehm_flow_gemm_desc"""
    _fields_ = [("X", C.c_void_p), ("gather", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("pro_scale", C.c_void_p), ("pro_shift", C.c_void_p),
                ("item", C.c_void_p), ("scatter", C.c_void_p), ("Y", C.c_void_p), ("R", C.c_int), ("K", C.c_int), ("N", C.c_int), ("S", C.c_int),
                ("ldx", C.c_int), ("ldw", C.c_int), ("ldy", C.c_int), ("ld_item", C.c_int), ("prologue", C.c_int), ("epilogue", C.c_int),
                ("mask", C.c_void_p), ("add", C.c_void_p), ("aux", C.c_void_p), ("ld_mask", C.c_int), ("ld_add", C.c_int),
                ("w_window", C.c_int)]


class FlowWgradDesc(C.Structure):
    """ehm_flow_wgrad_desc"""
    _fields_ = [("G", C.c_void_p), ("gather_g", C.c_void_p), ("item", C.c_void_p), ("X", C.c_void_p), ("gather_x", C.c_void_p), ("x_shift", C.c_void_p),
                ("out", C.c_void_p), ("R", C.c_int), ("Cg", C.c_int), ("Ca", C.c_int), ("S", C.c_int), ("ldg", C.c_int), ("ldx", C.c_int),
                ("ld_item", C.c_int), ("ld_out", C.c_int), ("act", C.c_int), ("alpha", C.c_float), ("beta", C.c_float)]


class FlowReduceDesc(C.Structure):
    """ehm_flow_reduce_desc"""
    _fields_ = [("G", C.c_void_p), ("gather", C.c_void_p), ("U2", C.c_void_p), ("item", C.c_void_p), ("out", C.c_void_p), ("R", C.c_int), ("N", C.c_int),
                ("S", C.c_int), ("ldg", C.c_int), ("ldu", C.c_int), ("ld_item", C.c_int), ("ld_out", C.c_int), ("mode", C.c_int), ("scale", C.c_float)]


FLOW_PRO_NONE, FLOW_PRO_RELU, FLOW_PRO_BN_RELU, FLOW_PRO_SHIFT, FLOW_PRO_GATE = 0, 1, 2, 3, 4                 # EHM_FLOW_PRO_* of the header
FLOW_EPI_BIAS, FLOW_EPI_ITEM_ADD, FLOW_EPI_GLU_RES, FLOW_EPI_SCATTER_ADD, FLOW_EPI_SCATTER_SUB = 0, 1, 2, 3, 4   # EHM_FLOW_EPI_*
FLOW_EPI_MASK, FLOW_EPI_MASK_ADD, FLOW_EPI_ADD = 5, 6, 7
FLOW_ACT_NONE, FLOW_ACT_RELU = 0, 1                                                                          # EHM_FLOW_ACT_*
FLOW_RED_COLS, FLOW_RED_ITEM, FLOW_RED_GATE = 0, 1, 2                                                        # EHM_FLOW_RED_*


class SceneDesc(C.Structure):
    """ehm_scene_desc"""
    _fields_ = [("verts", C.c_void_p), ("total_verts", C.c_int64), ("mesh_offsets", C.c_void_p), ("num_meshes", C.c_int), ("max_mesh_verts", C.c_int64),
                ("groups", C.c_void_p), ("num_groups", C.c_int), ("params", C.c_void_p), ("mode", C.c_int), ("chain_len", C.c_int), ("B", C.c_int),
                ("target", C.c_int), ("stride", C.c_int), ("points", C.c_void_p), ("index", C.c_void_p), ("n_selected", C.c_void_p),
                ("status", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class ImagePatchDesc(C.Structure):
    """ehm_image_patch_desc"""
    _fields_ = [("frames", C.c_void_p), ("F", C.c_int), ("H", C.c_int), ("W", C.c_int), ("frame_index", C.c_void_p), ("params", C.c_void_p),
                ("B", C.c_int), ("P", C.c_int), ("quantize", C.c_int), ("mean", C.c_double * 3), ("std", C.c_double * 3), ("img", C.c_void_p)]


class RenderDesc(C.Structure):
    """ehm_render_desc"""
    _fields_ = ([(n, C.c_void_p) for n in ("vertices", "faces", "vf_offsets", "vf_faces", "vertex_colors", "fx", "fy", "cx", "cy", "frames", "frame_index")] +
                [(n, C.c_int) for n in ("B", "V", "F", "Fr", "H", "W", "smooth", "two_sided", "cull_backface")] +
                [("z_near", C.c_float), ("base_color", C.c_float * 3), ("light_dir", C.c_float * 3), ("ambient", C.c_float), ("diffuse", C.c_float),
                 ("bg_color", C.c_uint8 * 4), ("bin_capacity", C.c_int)] +
                [(n, C.c_void_p) for n in ("needed_capacity", "color", "depth", "face_index", "workspace")] + [("workspace_bytes", C.c_int64),
                                                                                                              ("clip_near", C.c_int)])


class JpegHeader(C.Structure):
    """ehm_jpeg_header"""
    _fields_ = ([(n, C.c_int32) for n in ("H", "W", "components", "hmax", "vmax", "mcus_x", "mcus_y", "restart_interval")] +
                [(n, C.c_int32 * 3) for n in ("h", "v", "blocks_x", "blocks_y", "quant_id")] +
                [("quant", (C.c_uint16 * 64) * 4), ("coef_count", C.c_int64)])


class JpegDecodeDesc(C.Structure):
    """ehm_jpeg_decode_desc"""
    _fields_ = [("coef", C.c_void_p), ("quant", C.c_void_p), ("H", C.c_int), ("W", C.c_int), ("components", C.c_int), ("hmax", C.c_int),
                ("vmax", C.c_int), ("F", C.c_int), ("frames", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class JpegForwardDesc(C.Structure):
    """ehm_jpeg_forward_desc"""
    _fields_ = [("frames", C.c_void_p), ("quant", C.c_void_p), ("H", C.c_int), ("W", C.c_int), ("hmax", C.c_int), ("vmax", C.c_int),
                ("F", C.c_int), ("rgb", C.c_int), ("coef", C.c_void_p)]


class JpegEntropyEncodeDesc(C.Structure):
    """ehm_jpeg_entropy_encode_desc"""
    _fields_ = [("coef", C.c_void_p), ("H", C.c_int), ("W", C.c_int), ("hmax", C.c_int), ("vmax", C.c_int), ("F", C.c_int),
                ("streams", C.c_void_p), ("capacity", C.c_int64), ("lengths", C.c_void_p), ("needed", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float

# name -> (restype, argtypes); every symbol include/egohmr_hip.h declares
PROTOTYPES = {
    "ehm_last_error": (C.c_char_p, []),
    "ehm_target_arch": (C.c_char_p, []),
    "ehm_build_features": (C.c_char_p, []),
    "ehm_rot6d_to_rotmat": (_I, [_P, _P, _L, _I, _P]),
    "ehm_rot6d_to_rotmat_bwd": (_I, [_P, _P, _P, _L, _I, _P]),
    "ehm_rotmat_to_angle_axis": (_I, [_P, _P, _L, _P]),
    "ehm_rotmat_to_angle_axis_bwd": (_I, [_P, _P, _P, _L, _P]),
    "ehm_smpl_create": (_I, [C.POINTER(_P), _P, _P, _P, _P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _I, _P]),
    "ehm_smpl_destroy": (None, [_P]),
    "ehm_smpl_forward": (_I, [_P, _P, _P, _P, _P, _P, _I, _P]),
    "ehm_smpl_forward_rot6d": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "ehm_gcn_create": (_I, [C.POINTER(_P), _P, C.POINTER(GConvParams), C.POINTER(GConvParams), _I, C.POINTER(GConvParams), _I, _P]),
    "ehm_gcn_destroy": (None, [_P]),
    "ehm_gcn_row_tile": (_I, []),
    "ehm_gcn_set_precision": (_I, [_P, _I]),
    "ehm_gcn_get_precision": (_I, [_P]),
    "ehm_gcn_set_uncond_mode": (_I, [_P, _I]),
    "ehm_gcn_set_pass_map": (_I, [_P, _P, _P, _I]),
    "ehm_gcn_set_nonlocal": (_I, [_P, C.POINTER(NonlocalParams)]),
    "ehm_gcn_reserve": (_I, [_P, _I, _I]),
    "ehm_gcn_activation_group": (_I, [_P]),
    "ehm_gcn_pack_activations": (_I, [_P, _P, _L, _I, _I, _P]),
    "ehm_gcn_unpack_activations": (_I, [_P, _P, _L, _I, _I, _P]),
    "ehm_gcn_pack_activations_checked": (_I, [_P, _P, _P, _L, _P]),
    "ehm_gcn_input_layer": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "ehm_gcn_input_layer_rows": (_I, [_P, _P, _P, _I, _P]),
    "ehm_gcn_hidden_layer": (_I, [_P, _I, _P, _P, _P, _L, _P]),
    "ehm_gcn_hidden_stack": (_I, [_P, C.POINTER(C.c_void_p), _L, C.POINTER(C.c_int), _P]),
    "ehm_gcn_stack_status": (_I, [_P, _P]),
    "ehm_gcn_stack_status_async": (_I, [_P, _P, _P]),
    "ehm_gcn_output_layer": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "ehm_gcn_output_layer_cfg": (_I, [_P, _P, _P, _P, _I, _I, _F, _F, _P]),
    "ehm_gcn_set_fuse_scales": (_I, [_P, _I, _F, _F]),
    "ehm_gcn_bwd_epilogue": (_I, [_P, _I, _P, _P, _P, _I, _I, _P]),
    "ehm_gcn_bwd_params_workspace_bytes": (_I, [_P, _I, _I, C.POINTER(C.c_int64)]),
    "ehm_gcn_bwd_params": (_I, [_P, _I, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _L, _P]),
    "ehm_gcn_train_workspace_bytes": (_I, [_P, _I, _I, C.POINTER(C.c_int64)]),
    "ehm_gcn_train_adjacency": (_I, [_P, _I, _P, _P]),
    "ehm_gcn_train_preact": (_I, [_P, _I, _P, _I, _I, _P, _P, _P, _L, _P]),
    "ehm_gcn_train_stats": (_I, [_P, _I, _P, _I, _I, C.c_double, C.c_double, _P, _P, _P, _P, _P, _L, _P]),
    "ehm_gcn_train_normalize": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _P]),
    "ehm_gcn_train_bn_backward": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _L, _P]),
    "ehm_gcn_train_bwd_epilogue": (_I, [_P, _I, _P, _P, _P, _I, _I, _P]),
    "ehm_gcn_train_bwd_params_workspace_bytes": (_I, [_P, _I, _I, C.POINTER(C.c_int64)]),
    "ehm_gcn_train_bwd_params": (_I, [_P, _I, _P, _P, _P, _I, _I, _P, _P, _P, _L, _P]),
    "ehm_gcn_train_stats_local": (_I, [_P, _I, _P, _I, _I, _P, _P, _L, _P]),
    "ehm_gcn_train_stats_merge": (_I, [_P, _I, _P, _P, _I, C.c_double, C.c_double, _P, _P, _P, _P, _P]),
    "ehm_gcn_train_bwd_local": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _L, _P]),
    "ehm_gcn_train_bwd_merge": (_I, [_P, _I, _P, _P, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _L, _P]),
    "ehm_linear_split": (_I, [C.POINTER(LinearDesc), _P]),
    "ehm_split_pack": (_I, [_P, _P, _L, _I, _I, _F, _P]),
    "ehm_skinny_gemm_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "ehm_resnet_stem_scratch_bytes": (C.c_size_t, [_I, _I, _I]),
    "ehm_resnet_stem": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "ehm_conv_x2_rows": (C.c_int64, [C.c_int64]),
    "ehm_conv_x2": (_I, [C.POINTER(ConvX2Desc), _P]),
    "ehm_conv_x2_workspace_bytes": (C.c_int64, [C.POINTER(ConvX2Desc)]),
    "ehm_conv_x2_workspace_status": (_I, [_P, _P, _P]),
    "ehm_x2_group_mean": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "ehm_conv_nhwc_split": (_I, [C.POINTER(ConvDesc), _P]),
    "ehm_nonlocal_attention": (_I, [_P, _P, _L, _I, _P]),
    "ehm_nonlocal_attention_backward": (_I, [_P, _P, _P, _L, _I, _P]),
    "ehm_nonlocal_bn_residual": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _P]),
    "ehm_pointnet_lift": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "ehm_pointnet_bwd_workspace_bytes": (_I, [_I, _I, _I, C.POINTER(C.c_int64)]),
    "ehm_pointnet_pool_argmax": (_I, [_P, _I, _P, _I, _I, _I, _I, _P, _L, _P]),
    "ehm_pointnet_bwd_scatter": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _L, _P]),
    "ehm_pointnet_bwd_gate": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _L, _P]),
    "ehm_pointnet_bwd_net0": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "ehm_pointnet_bwd_lift": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _L, _P]),
    "ehm_pointnet_bwd_wgrad_workspace_bytes": (_I, [_I, _I, _I, _I, C.POINTER(C.c_int64)]),
    "ehm_pointnet_bwd_wgrad": (_I, [_P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _L, _P]),
    "ehm_conv_bwd_gate": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ehm_conv_bwd_wgrad_workspace_bytes": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_int64)]),
    "ehm_conv_bwd_wgrad": (_I, [_P, _P, _L, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _L, _P]),
    "ehm_resnet_stem_backward_workspace_bytes": (_I, [_I, _I, _I, C.POINTER(C.c_int64)]),
    "ehm_resnet_stem_backward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _L, _P]),
    "ehm_resnet_stem_preact": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "ehm_resnet_stem_route": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "ehm_resnet_stem_wgrad": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _L, _P]),
    "ehm_bn2d_train_workspace_bytes": (_I, [_L, _I, C.POINTER(C.c_int64)]),
    "ehm_bn2d_train_stats": (_I, [_P, _I, _L, _L, _I, C.c_double, C.c_double, _P, _P, _P, _P, _P, _P, _P, _L, _P]),
    "ehm_bn2d_train_bwd_sums": (_I, [_P, _P, _I, _L, _L, _I, _P, _P, _P, _P, _P, _L, _P]),
    "ehm_bn2d_train_bwd_zbar": (_I, [_P, _P, _I, _L, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ehm_bn2d_train_stats_local": (_I, [_P, _I, _L, _L, _I, _P, _P, _L, _P]),
    "ehm_bn2d_train_stats_merge": (_I, [_P, _P, _I, _I, C.c_double, C.c_double, _P, _P, _P, _P, _P, _P, _P]),
    "ehm_bn2d_train_bwd_local": (_I, [_P, _P, _I, _L, _L, _I, _P, _P, _P, _P, _L, _P]),
    "ehm_bn2d_train_bwd_merge": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "ehm_bn2d_train_bwd_zbar_rows": (_I, [_P, _P, _I, _L, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _L, _P]),
    "ehm_ddpm_step": (_I, [_P, _P, _P, _P, _P, _F, _F, _F, _F, _F, _L, _P]),
    "ehm_ddim_step": (_I, [_P, _P, _P, _P, _F, _F, _F, _F, _F, _F, _L, _P]),
    "ehm_collision_proxy": (_I, [_P, _P, _P, _P, _I, _I, _I, _F, _P]),
    "ehm_collision_query": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _F, _I, _P]),
    "ehm_mesh_collision_query": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ehm_smpl_set_collision_mesh": (_I, [_P, _P, _I]),
    "ehm_smpl_backward_rot6d": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "ehm_guidance_grad_finish": (_I, [_P, _P, _P, _I, _F, _P]),
    "ehm_smpl_backward": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _L, _P]),
    "ehm_smpl_backward_workspace_bytes": (_I, [_P, _I, C.POINTER(C.c_int64)]),
    "ehm_smpl_backward_ordered": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _L, _P]),
    "ehm_smpl_backward_ordered_workspace_bytes": (_I, [_P, _I, C.POINTER(C.c_int64)]),
    "ehm_nn_dist2": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "ehm_eval_point_errors": (_I, [C.POINTER(EvalPointsDesc), _P]),
    "ehm_eval_procrustes": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "ehm_eval_procrustes_vis": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "ehm_eval_diversity": (_I, [_P, _P, _I, _P, _P, _I, _I, _I, _P]),
    "ehm_stage1_head": (_I, [C.POINTER(Stage1Desc), _P]),
    "ehm_flow_context": (_I, [C.POINTER(FlowContextDesc), _P]),
    "ehm_flow_gemm": (_I, [C.POINTER(FlowGemmDesc), _P]),
    "ehm_flow_finish": (_I, [_P, C.c_double, _P, _P, _P, _P, _P, _I, _P]),
    "ehm_flow_wgrad": (_I, [C.POINTER(FlowWgradDesc), _P]),
    "ehm_flow_reduce": (_I, [C.POINTER(FlowReduceDesc), _P]),
    "ehm_flow_finish_backward": (_I, [_P] * 10 + [_I, _P]),
    "ehm_scene_workspace_bytes": (_I, [C.POINTER(SceneDesc), C.POINTER(C.c_int64)]),
    "ehm_scene_select": (_I, [C.POINTER(SceneDesc), _P]),
    "ehm_image_patch": (_I, [C.POINTER(ImagePatchDesc), _P]),
    "ehm_scene_augment": (_I, [_P, _I, _P, _P, _I, _I, _I, _P]),
    "ehm_jpeg_read_header": (_I, [_P, _L, C.POINTER(JpegHeader)]),
    "ehm_jpeg_entropy_decode": (_I, [_P, _L, C.POINTER(JpegHeader), _P, _L]),
    "ehm_jpeg_workspace_bytes": (_I, [C.POINTER(JpegDecodeDesc), C.POINTER(C.c_int64)]),
    "ehm_jpeg_decode": (_I, [C.POINTER(JpegDecodeDesc), _P]),
    "ehm_jpeg_quality_tables": (_I, [_I, _P]),
    "ehm_jpeg_write_header": (_I, [_I, _I, _I, _I, _P, _P, _L, C.POINTER(C.c_int64)]),
    "ehm_jpeg_forward": (_I, [C.POINTER(JpegForwardDesc), _P]),
    "ehm_jpeg_entropy_encode_workspace_bytes": (_I, [C.POINTER(JpegEntropyEncodeDesc), C.POINTER(C.c_int64)]),
    "ehm_jpeg_entropy_encode": (_I, [C.POINTER(JpegEntropyEncodeDesc), _P]),
    "ehm_render_workspace_bytes": (_I, [C.POINTER(RenderDesc), C.POINTER(C.c_int64)]),
    "ehm_render": (_I, [C.POINTER(RenderDesc), _P]),
    "ehm_sample_workspace_bytes": (_L, [C.POINTER(SampleDesc), _I, _I]),
    "ehm_sample_loop": (_I, [_P, _P, C.POINTER(SampleDesc), C.POINTER(StepCoefs)] + [_P] * 18 + [_L, _P]),
    "ehm_item_prep": (_I, [C.POINTER(ItemPrepDesc), _P]),
    "ehm_pack_outputs": (_I, [C.POINTER(PackDesc), _P]),
    "ehm_val_losses_workspace_bytes": (_I, [_I, _I, C.POINTER(C.c_int64)]),
    "ehm_val_losses": (_I, [C.POINTER(ValLossesDesc), _P]),
    "ehm_val_losses_backward_workspace_bytes": (_I, [_I, _I, C.POINTER(C.c_int64)]),
    "ehm_val_losses_backward": (_I, [C.POINTER(ValLossesBwdDesc), _P]),
    "ehm_scene_cap_points": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "ehm_cond_assemble": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _I, _P, _I, _I, _I, _P]),
    "ehm_cond_assemble_backward": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _P]),
    "ehm_profile_begin": (_I, []),
    "ehm_profile_end": (_I, [C.POINTER(C.c_double), C.POINTER(C.c_int64), _I]),
}
MESH_COLLISION_FACE_CHUNK, MESH_COLLISION_POINT_BLOCK = 512, 256     # EHM_MESH_COLLISION_* of the header (tests size their edge cases by them)
JPEG_ENC_HEADER_BYTES, JPEG_ENC_SCAN_CHUNK, JPEG_ENC_STUFF_CHUNK, JPEG_ENC_MAX_BLOCK_BYTES = 623, 256, 4096, 208   # EHM_JPEG_ENC_* of the header
PROF_CLASSES = ("input", "chain_f16x3", "chain_f16", "hidden_f32", "out_dot", "step_body", "skin_input", "guidance", "reserved_8", "reserved_9",
                "guid_nearest", "guid_skin_bwd", "guid_posefeat_bwd", "step_fused", "guid_nearest_evals",   # EHM_PROF_* of the header ("guid_nearest_evals" is a COUNT in `launches`)
                "chain_f16x2")
# the entry points that return a value (a size, a tile, a mode) rather than a status: negative = error.  Every other int-returning one is a status
VALUE_FUNCTIONS = frozenset({"ehm_gcn_row_tile", "ehm_gcn_get_precision", "ehm_gcn_activation_group", "ehm_conv_x2_rows", "ehm_conv_x2_workspace_bytes",
                             "ehm_sample_workspace_bytes", "ehm_resnet_stem_scratch_bytes"})

_lib = None
_api = None


def lib() -> C.CDLL:
    """The loaded library.  Raises EgoHMRHipError when it is absent - never falls back."""
    global _lib, _api
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EgoHMRHipError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  egohmr_amd has no CPU/eager fallback.")
        try:
            handle = C.CDLL(LIB_PATH)
        except OSError as e:
            raise EgoHMRHipError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in PROTOTYPES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise EgoHMRHipError(f"{LIB_PATH} does not export {name}; rebuild it") from e
            fn.restype = res
            fn.argtypes = args
        if handle.ehm_target_arch() != b"gfx950":
            raise EgoHMRHipError("libegohmr_hip.so was not built for gfx950")
        _api = SimpleNamespace(**{name: _checked(name, getattr(handle, name)) for name in PROTOTYPES})
        _lib = handle
    return _lib


def api() -> SimpleNamespace:
    """The checked view of the library (module docstring): one callable per PROTOTYPES entry."""
    lib()
    return _api


def _error(rc: int, function: str) -> EgoHMRHipError:
    msg = lib().ehm_last_error()
    cls = EgoHMRRangeError if rc == -34 else EgoHMRHipError
    return cls(f"{function} failed (rc={rc}): {msg.decode() if msg else ''}", rc=rc, function=function)


def _checked(name, fn):
    unchecked, value = PROTOTYPES[name][0] in (None, C.c_char_p), name in VALUE_FUNCTIONS

    def call(*args):
        # (the tensors are converted here, not in an argtype's from_param: an exception raised there reaches the caller as ctypes.ArgumentError)
        rc = fn(*[ptr(a) if isinstance(a, torch.Tensor) else a for a in args])
        if not unchecked and (rc < 0 if value else rc != 0):
            raise _error(rc, name)
        return rc
    call.__name__ = name
    return call


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise _error(rc, what or "libegohmr_hip")


class Handle:
    """Owner of an opaque native object: pointer, destroy function, the tensors that must outlive it; passes as the pointer (NULL once closed).
    `serial` is unique in the process - unlike the host address, which a handle created after a destroy can reuse - for cache keys."""
    _serials = itertools.count(1)

    def __init__(self, ptr, destroy, keep=()):
        self.ptr, self._destroy, self.keep = ptr, destroy, list(keep)
        self.serial = next(Handle._serials)

    @property
    def _as_parameter_(self):
        return self.ptr

    def close(self):
        p, self.ptr = self.ptr, None
        if p is not None:
            self._destroy(p)
        self.keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:                 # (interpreter teardown: the library may be gone already)
            pass


def ptr(t) -> int:
    """Device pointer of a contiguous float32/uint8 CUDA(HIP) tensor (0 for None)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise EgoHMRHipError("egohmr_amd kernels need tensors on a HIP device (got a CPU tensor); there is no CPU path")
    if not t.is_contiguous():
        raise EgoHMRHipError("tensor handed to the C ABI must be contiguous")
    return t.data_ptr()


class TensorKey:
    """(data_ptr, _version) of every parameter and buffer of some modules, as a cache key, without walking the module tree each time:
    `Module.parameters()` costs ~0.9 ms for ResNet-50 + the PointNet and was evaluated several times per sampling call with the GPU
    idle behind it.  The slots (owner dict, name) are collected once; a replaced Parameter object, an in-place update (_version) and a
    move to another device / dtype (data_ptr) all change the key.  Modules or parameters ADDED later are not seen: call refresh()."""

    def __init__(self, *modules):
        self.modules = modules
        self.refresh()

    def refresh(self):
        self.slots = []
        seen = set()
        for mod in self.modules:
            for m in mod.modules():
                if id(m) in seen:
                    continue
                seen.add(id(m))
                self.slots += [(m._parameters, n) for n in m._parameters] + [(m._buffers, n) for n in m._buffers]

    def __call__(self):
        out = []
        for d, n in self.slots:
            t = d.get(n)
            if t is not None:
                out.append((t.data_ptr(), t._version))
        return tuple(out)


def f32(t, device=None):
    """contiguous float32 view/copy on the device."""
    t = t.detach()
    if device is not None and t.device != device:
        t = t.to(device)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def stream_ptr() -> int:
    """The current stream (evaluated before a native call validates its tensors: without a HIP device, the package's error is raised here)."""
    try:
        return torch.cuda.current_stream().cuda_stream
    except RuntimeError as e:
        raise EgoHMRHipError(f"egohmr_amd kernels need a HIP device; there is no CPU path ({e})") from e


def on_device(dev):
    """Context for a native call: the HIP device of the tensors it is given becomes the current one (the library launches on the CURRENT
    device's stream; a model living on cuda:1 of a process whose current device is cuda:0 must not launch there).  CPU devices pass through -
    the call sites reject CPU tensors themselves (EgoHMRHipError)."""
    import contextlib
    dev = torch.device(dev) if not isinstance(dev, torch.device) else dev
    return torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()
