#!/usr/bin/env python3
"""Generate tests/golden/g19_stage1_*.npz and g20_procrustes_vis.npz by running the REFERENCE's own code on the CPU.

    python tools/make_stage1_golden.py /path/to/EgoHMR-reference        # from the repo root; rewrites the three files

Build-container tool: no GPU test and no product code reads it (the tests read the .npz files it writes).  Like oracle/make_golden.py,
what it stores is data only - seeds, small inputs, the reference's outputs - and the weights are regenerated from
egohmr_amd.synthetic.make_stage1_state_dict(seed); per-key sums pin that regeneration.

g19 (stage-1 translation): ProHMRScene.forward_step(batch, train=False) (models/prohmr/prohmr_scene.py) with NUM_TEST_SAMPLES = 1 (the mode,
z = 0), then test_prohmr_scene.py:175-213 (convert_pare_to_full_img_cam).  Stubs installed before the import: ``yacs`` (a CfgNode that is a
namespace), ``nflows.flows.ConditionalGlow`` (zero samples and log-probs: pred_cam never reads them), ``smplx`` (a body model returning zero
joints and vertices: pred_cam never reads them either), ``torch.utils.model_zoo.load_url`` (no ImageNet download) and a synthetic
smpl_mean_params.npz (cam ~ [0.9, 0, 0]; the head's init buffers are overwritten by load_state_dict anyway).  Besides the float32 run it
stores the reference's FCHead and convert_pare_to_full_img_cam evaluated in float64 on the stored float32 context (`*_f64`).

g20 (visible-joint Procrustes): utils/pose_utils.py reconstruction_error_with_vis_mask on float64 copies of random float32 clouds.
"""
from __future__ import annotations

import os
import sys
import tempfile
import types
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)

from egohmr_amd import synthetic as syn  # noqa: E402

B1, N_SCENE, BATCH_SEED, WEIGHT_SEED = 5, 20000, 19, 0
FLAG_SETS = {"all_on": (True, True, True), "all_off": (False, False, False)}     # (with_focal_length, with_bbox_info, with_cam_center)


class _ZeroBody(nn.Module):
    def forward(self, betas=None, body_pose=None, global_orient=None, **kw):
        n = betas.shape[0]
        return SimpleNamespace(joints=torch.zeros(n, 45, 3), vertices=torch.zeros(n, 6890, 3))


class _ZeroGlow(nn.Module):
    def __init__(self, dim, *a, **k):
        super().__init__()
        self.dim = dim

    def sample_and_log_prob(self, num_samples, context=None, noise=None):
        n = context.shape[0] * num_samples
        return torch.zeros(n, self.dim), torch.zeros(context.shape[0], num_samples), noise


def install_stubs(ref):
    yacs, yacs_config = types.ModuleType("yacs"), types.ModuleType("yacs.config")
    yacs_config.CfgNode = SimpleNamespace
    yacs.config = yacs_config
    nflows, nflows_flows = types.ModuleType("nflows"), types.ModuleType("nflows.flows")
    nflows_flows.ConditionalGlow = _ZeroGlow
    nflows.flows = nflows_flows
    smplx = types.ModuleType("smplx")
    smplx.create = lambda *a, **k: _ZeroBody()
    sys.modules.update({"yacs": yacs, "yacs.config": yacs_config, "nflows": nflows, "nflows.flows": nflows_flows, "smplx": smplx})
    import torch.utils.model_zoo as mz
    mz.load_url = lambda *a, **k: {}
    sys.path.insert(0, ref)


def ref_cfg(mean_params):
    N = SimpleNamespace
    return N(MODEL=N(BACKBONE=N(NUM_LAYERS=50), FLOW=N(DIM=144, LAYER_HIDDEN_FEATURES=1024, NUM_LAYERS=4, LAYER_DEPTH=2, CONTEXT_FEATURES=2048),
                     FC_HEAD=N(NUM_FEATURES=1024), IMAGE_SIZE=224),
             SMPL=N(MEAN_PARAMS=mean_params), CAM=N(FX_NORM_COEFF=1500.0), EXTRA=N(FOCAL_LENGTH=5000.0),
             TRAIN=N(NUM_TEST_SAMPLES=1, NUM_TRAIN_SAMPLES=1, LR=1e-4, WEIGHT_DECAY=1e-4))


def stage1_batch():
    """The stage-1 inputs: image and whole-scene cloud from synthetic.make_batch(B1, N_SCENE, BATCH_SEED), camera / box scalars drawn here (stored)."""
    b = syn.make_batch(B1, N_SCENE, seed=BATCH_SEED)
    g = np.random.Generator(np.random.PCG64(9100))
    cam = {"fx": g.uniform(0.9, 1.1, B1).astype(np.float32), "cam_cx": g.uniform(900, 1000, B1).astype(np.float32),
           "cam_cy": g.uniform(500, 580, B1).astype(np.float32),
           "box_center": np.stack([g.uniform(400, 1500, B1), g.uniform(200, 900, B1)], -1).astype(np.float32),
           "box_size": g.uniform(150, 600, B1).astype(np.float32)}
    return b["img"], b["scene_pcd_verts_full"], cam


def g19(tag, flags, mean_params):
    from models.prohmr.prohmr_scene import ProHMRScene
    from models.prohmr.fc_head import FCHead
    from utils.geometry import convert_pare_to_full_img_cam
    fl, bb, cc = flags
    cfg = ref_cfg(mean_params)
    torch.manual_seed(0)
    model = ProHMRScene(cfg, device=torch.device("cpu"), with_focal_length=fl, with_bbox_info=bb, with_cam_center=cc, scene_feat_dim=512)
    sd = syn.make_stage1_state_dict(WEIGHT_SEED, with_focal_length=fl, with_bbox_info=bb, with_cam_center=cc)
    ref_sd = model.state_dict()
    for k, v in sd.items():                                   # the product's key list IS a subset of the reference's, with the same shapes
        assert k in ref_sd and tuple(ref_sd[k].shape) == v.shape, k
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys
    model.initialized |= True                                 # (ActNorm initialisation of the flow: stubbed)
    model.eval()
    img, scene, cam = stage1_batch()
    batch = {"img": torch.from_numpy(img), "scene_pcd_verts_full": torch.from_numpy(scene), **{k: torch.from_numpy(v) for k, v in cam.items()}}
    with torch.no_grad():
        out = model.forward_step(batch, train=False)
        pred_cam = out["pred_cam"][:, 0]                                                           # test_prohmr_scene.py:202 (mode)
        focal = batch["fx"] * cfg.CAM.FX_NORM_COEFF
        full = convert_pare_to_full_img_cam(pare_cam=pred_cam, bbox_height=batch["box_size"], bbox_center=batch["box_center"],
                                            img_w=batch["cam_cx"] * 2, img_h=batch["cam_cy"] * 2, focal_length=focal,
                                            crop_res=cfg.MODEL.IMAGE_SIZE)                          # :209-213
        # float64: the reference's own head and conversion on the stored float32 context
        head = FCHead(cfg, model.flow.fc_head.layers[0].in_features).double()
        head.load_state_dict({k: v.double() for k, v in model.flow.fc_head.state_dict().items()})
        ctx64 = out["conditioning_feats"].double()
        betas64, cam64 = head({"body_pose": torch.zeros(B1, 1)}, ctx64)
        full64 = convert_pare_to_full_img_cam(pare_cam=cam64[:, 0], bbox_height=batch["box_size"].double(), bbox_center=batch["box_center"].double(),
                                              img_w=batch["cam_cx"].double() * 2, img_h=batch["cam_cy"].double() * 2,
                                              focal_length=batch["fx"].double() * cfg.CAM.FX_NORM_COEFF, crop_res=cfg.MODEL.IMAGE_SIZE)
    keys = [k for k, _ in syn.stage1_manifest(with_focal_length=fl, with_bbox_info=bb, with_cam_center=cc)]
    arrays = dict(batch_seed=BATCH_SEED, num_scene_points=N_SCENE, weight_seed=WEIGHT_SEED, flags=np.array(flags), fx_norm_coeff=1500.0,
                  key_names=np.array(keys), key_shapes=np.array([str(tuple(sd[k].shape)) for k in keys]),
                  key_sums=np.array([float(np.asarray(sd[k], np.float64).sum()) for k in keys]),
                  conditioning_feats=out["conditioning_feats"].numpy(), pred_cam=pred_cam.numpy(), pred_cam_full=full.numpy(),
                  pred_betas=out["pred_smpl_params"]["betas"][:, 0].numpy(), pred_cam_f64=cam64[:, 0].numpy(), pred_betas_f64=betas64[:, 0].numpy(),
                  pred_cam_full_f64=full64.numpy(), **{k: v for k, v in cam.items()})
    path = os.path.join(OUT, f"g19_stage1_{tag}.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: pred_cam {pred_cam.numpy().round(4).tolist()}\n  pred_cam_full {full.numpy().round(3).tolist()}")


def g20():
    from utils.pose_utils import reconstruction_error_with_vis_mask
    g = np.random.Generator(np.random.PCG64(9200))
    cases = {}
    J = 24
    base = g.normal(scale=0.3, size=(J, 3))
    # per-item masks: all visible, random, exactly 2 visible, and a planar (rank-2) prediction with half visible
    masks, preds, gts = [], [], []
    for kind in ("all", "random", "random", "two", "two", "planar", "all", "random"):
        gt = base + g.normal(scale=0.05, size=(J, 3))
        R, _ = np.linalg.qr(g.normal(size=(3, 3)))
        pred = 1.1 * gt @ R.T + g.normal(scale=0.04, size=(J, 3)) + g.normal(size=3)
        m = np.ones(J, bool)
        if kind == "random":
            m = g.random(J) < 0.6
        elif kind == "two":
            m = np.zeros(J, bool)
            m[g.choice(J, 2, replace=False)] = True
        elif kind == "planar":
            pred[:, 2] = 0.0
            m = g.random(J) < 0.5
        masks.append(m), preds.append(pred), gts.append(gt)
    pred = np.array(preds, np.float32)
    gt = np.array(gts, np.float32)
    mask = np.array(masks)
    m3 = np.repeat(mask[:, :, None], 3, axis=2)
    per_joint = reconstruction_error_with_vis_mask(m3, pred.astype(np.float64), gt.astype(np.float64), avg_joint=False)
    cases.update(pred=pred, gt=gt, mask=mask, per_joint=per_joint, mean=per_joint.mean(-1), vis_sum=(per_joint * mask).sum(-1),
                 invis_sum=(per_joint * ~mask).sum(-1))
    # J = 45 (all SMPL joints), two samples per item sharing the item's mask (test_egohmr.py:427-431 repeats it over S)
    B, S, J2 = 3, 2, 45
    gt45 = g.normal(scale=0.3, size=(B, J2, 3)).astype(np.float32)
    pred45 = (gt45[:, None] * 0.9 + g.normal(scale=0.05, size=(B, S, J2, 3))).astype(np.float32)
    mask45 = g.random((B, J2)) < 0.7
    m45 = np.repeat(np.repeat(mask45[:, None, :, None], S, 1), 3, 3).reshape(B * S, J2, 3)
    pj45 = reconstruction_error_with_vis_mask(m45, pred45.reshape(B * S, J2, 3).astype(np.float64),
                                              np.repeat(gt45[:, None], S, 1).reshape(B * S, J2, 3).astype(np.float64), avg_joint=False)
    cases.update(pred45=pred45, gt45=gt45, mask45=mask45, per_joint45=pj45.reshape(B, S, J2))
    path = os.path.join(OUT, "g20_procrustes_vis.npz")
    np.savez_compressed(path, **cases)
    print(f"{path}: mean {cases['mean'].round(4).tolist()}")


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EGOHMR_REFERENCE", "")
    if not ref or not os.path.isdir(os.path.join(ref, "models", "prohmr")):
        sys.exit("usage: python tools/make_stage1_golden.py <path to the reference EgoHMR checkout>")
    install_stubs(ref)
    with tempfile.TemporaryDirectory() as tmp:
        mp = os.path.join(tmp, "smpl_mean_params.npz")
        np.savez(mp, cam=np.array([0.9, 0.0, 0.0], np.float32), shape=np.zeros(10, np.float32), pose=np.zeros(144, np.float32))
        for tag, flags in FLAG_SETS.items():
            g19(tag, flags, mp)
    g20()


if __name__ == "__main__":
    main()
