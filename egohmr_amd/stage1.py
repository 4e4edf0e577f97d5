"""Stage 1 of the reference's two-stage evaluation: the body translation a ``--two_stage`` stage-2 run conditions on.

The reference gets it from its ProHMR-scene model (models/prohmr/prohmr_scene.py) run by test_prohmr_scene.py, which writes
``results.pkl['pred_cam_full_list']`` (:417-426).  Only the deterministic half of that model feeds the translation:
``pred_cam = FCHead(feats)`` (models/prohmr/smpl_flow.py:88-90, fc_head.py:46-50) on the conditioning features of
prohmr_scene.py:111-130, converted to the full-image camera by convert_pare_to_full_img_cam (test_prohmr_scene.py:175-213).  The
normalizing flow (pose samples, log-prob) and the stage-1 metrics are not built: stage 2 never reads them.

    ResNet-50 (img) and ResnetPointnet(512, 256) (scene)   the encoders of egohmr_amd.encoders, same kernels as EgoHMR's
    context assembly + FCHead + camera conversion          one launch of ehm_stage1_head (csrc/stage1.hip)
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from .encoders import ResNet50Features, ResnetPointnet

IMG_DIM, HIDDEN, CROP_RES = 2048, 1024, 224      # configs/prohmr.yaml: MODEL.FLOW.CONTEXT_FEATURES, MODEL.FC_HEAD.NUM_FEATURES, MODEL.IMAGE_SIZE


class _FCHead(nn.Module):
    """models/prohmr/fc_head.py: Linear(ctx, 1024) - ReLU - Linear(1024, 13) and the mean-parameter buffers (a parameter container)."""

    def __init__(self, ctx_dim: int):
        super().__init__()
        self.layers = nn.Sequential(nn.Linear(ctx_dim, HIDDEN), nn.ReLU(inplace=False), nn.Linear(HIDDEN, 13))
        self.register_buffer("init_cam", torch.zeros(1, 1, 3))
        self.register_buffer("init_betas", torch.zeros(1, 1, 10))


class _Flow(nn.Module):
    """The `flow` submodule of the reference (SMPLFlow) reduced to its `fc_head`: checkpoint names stay `flow.fc_head.*`."""

    def __init__(self, ctx_dim: int):
        super().__init__()
        self.fc_head = _FCHead(ctx_dim)


class ProHMRSceneTransl(nn.Module):
    """The stage-1 camera translation of ProHMRScene (prohmr_scene.py) with the reference's state_dict names: ``backbone``, ``scene_enc``,
    ``flow.fc_head``.  Load a ProHMR-scene checkpoint with egohmr_amd.io.load_stage1_checkpoint.

    ``forward(batch)`` reads ``img`` [B,3,224,224], ``scene_pcd_verts_full`` [B,N,3], ``fx``, ``cam_cx``, ``cam_cy``, ``box_size`` [B] and
    ``box_center`` [B,2] and returns ``pred_cam`` [B,3] (the weak-perspective camera of the mode, z = 0), ``pred_cam_full`` [B,3] (the body
    translation in the camera frame, what results.pkl stores) and ``pred_betas`` [B,10].

    Stage 1 takes its OWN batch: it reads the whole-scene cloud (test_prohmr_scene.py:41, scene_type='whole_scene': the 20 000 scene points in
    front of the camera), while stage 2 reads the 2 m cube cropped around this stage's translation.  The reference runs two scripts over two
    dataset configurations; so does a caller of this package.  The scene frame is the camera frame (scene_cano=False, the
    script's default)."""

    def __init__(self, with_focal_length: bool = True, with_bbox_info: bool = True, with_cam_center: bool = True, fx_norm_coeff: float = 1500.0,
                 scene_feat_dim: int = 512, device=None):
        super().__init__()
        self.with_focal_length, self.with_bbox_info, self.with_cam_center = bool(with_focal_length), bool(with_bbox_info), bool(with_cam_center)
        self.fx_norm_coeff = float(fx_norm_coeff)
        self.scene_feat_dim = int(scene_feat_dim)
        self.context_dim = (IMG_DIM + self.scene_feat_dim + (1 if self.with_focal_length else 0) + (3 if self.with_bbox_info else 0)
                            + (2 if self.with_cam_center else 0))          # prohmr_scene.py:36-45
        self.backbone = ResNet50Features()
        self.scene_enc = ResnetPointnet(out_dim=self.scene_feat_dim, hidden_dim=256)
        self.flow = _Flow(self.context_dim)
        # arithmetic of the two encoders, as EgoHMR.encoder_precision: 'f16x3' (split-f16, f32 grade) | 'f16' (plain f16, NOT parity grade)
        self.encoder_precision = "f16x3"
        self._head_key_fn, self._head_key, self._head = None, None, None
        if device is not None:
            self.to(device)
        self.eval()

    def _head_weights(self, dev):
        """W1 transposed to [K, 1024] (the kernel's layout) and the other head tensors as contiguous float32, rebuilt when a weight changes."""
        if self._head_key_fn is None:
            self._head_key_fn = _lib.TensorKey(self.flow)
        key = self._head_key_fn() + (str(dev),)
        if self._head_key != key:
            h = self.flow.fc_head
            W1 = h.layers[0].weight
            if tuple(W1.shape) != (HIDDEN, self.context_dim):
                raise ValueError(f"flow.fc_head.layers.0.weight is {tuple(W1.shape)}, the context flags need ({HIDDEN}, {self.context_dim})")
            self._head = dict(W1t=_lib.f32(W1, dev).t().contiguous(), b1=_lib.f32(h.layers[0].bias, dev), W2=_lib.f32(h.layers[2].weight, dev),
                              b2=_lib.f32(h.layers[2].bias, dev), init_cam=_lib.f32(h.init_cam, dev).reshape(3),
                              init_betas=_lib.f32(h.init_betas, dev).reshape(10))
            self._head_key = key
        return self._head

    def head(self, img_feats, scene_feats, fx, cam_cx, cam_cy, box_center, box_size) -> dict:
        """ehm_stage1_head on given features: context assembly, FCHead and the camera conversion (one launch)."""
        dev = img_feats.device
        with _lib.on_device(dev):
            st = _lib.stream_ptr()
            B = img_feats.shape[0]
            img, scene = _lib.f32(img_feats, dev), _lib.f32(scene_feats, dev)
            if img.shape != (B, IMG_DIM) or scene.shape != (B, self.scene_feat_dim):
                raise ValueError(f"features {tuple(img.shape)} / {tuple(scene.shape)}, expected [B,{IMG_DIM}] / [B,{self.scene_feat_dim}]")
            sc = [_lib.f32(x, dev).reshape(B) for x in (fx, cam_cx, cam_cy, box_size)]
            bc = _lib.f32(box_center, dev).reshape(B, 2)
            w = self._head_weights(dev)
            out = {"pred_cam": torch.empty(B, 3, device=dev), "pred_cam_full": torch.empty(B, 3, device=dev), "pred_betas": torch.empty(B, 10, device=dev)}
            P = _lib.ptr
            d = _lib.Stage1Desc(img_feats=P(img), scene_feats=P(scene), fx=P(sc[0]), cam_cx=P(sc[1]), cam_cy=P(sc[2]), box_center=P(bc), box_size=P(sc[3]),
                                W1t=P(w["W1t"]), b1=P(w["b1"]), W2=P(w["W2"]), b2=P(w["b2"]), init_cam=P(w["init_cam"]), init_betas=P(w["init_betas"]),
                                pred_cam=P(out["pred_cam"]), pred_cam_full=P(out["pred_cam_full"]), pred_betas=P(out["pred_betas"]),
                                fx_norm=self.fx_norm_coeff, crop_res=float(CROP_RES), with_cam_center=int(self.with_cam_center),
                                with_bbox_info=int(self.with_bbox_info), with_focal_length=int(self.with_focal_length), img_dim=IMG_DIM,
                                scene_dim=self.scene_feat_dim, hidden=HIDDEN, B=B)
            _lib.api().ehm_stage1_head(C.byref(d), st)
        return out

    @torch.no_grad()
    def forward(self, batch) -> dict:
        if self.encoder_precision not in ("f16x3", "f16"):
            raise ValueError(f"encoder_precision must be 'f16x3' or 'f16', not {self.encoder_precision!r}")
        self.backbone.hi_only = self.scene_enc.hi_only = self.encoder_precision == "f16"
        img = batch["img"]
        if not img.is_cuda:
            raise _lib.EgoHMRHipError("ProHMRSceneTransl runs on the HIP kernels only (got a CPU tensor); there is no CPU path")
        if img.shape[0] == 0:
            raise ValueError("empty batch")
        with _lib.on_device(img.device):
            img_feats = self.backbone(img)                                         # prohmr_scene.py:111
            scene_feats = self.scene_enc(batch["scene_pcd_verts_full"])            # :127
        return self.head(img_feats, scene_feats, batch["fx"], batch["cam_cx"], batch["cam_cy"], batch["box_center"], batch["box_size"])
