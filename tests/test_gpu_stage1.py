"""GPU: stage-1 translation (ehm_stage1_head, egohmr_amd.stage1.ProHMRSceneTransl, Stage1Driver -> results.pkl -> Stage2Driver(two_stage=True))
and the visible-joint PA-MPJPE (ehm_eval_procrustes_vis, Stage2Driver(eval_with_vis_mask_pa=True)) against the reference's goldens
(tools/make_stage1_golden.py) and the float64 / numpy restatements of tests/test_stage1_cpu.py."""
import itertools
import os

import numpy as np
import pytest
import torch

from egohmr_amd import synthetic as syn
from tests.test_stage1_cpu import FLAGS, procrustes_vis_np, stage1_head_f64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _head_weights(g, K, zero_scale=False):
    sd = {"flow.fc_head.layers.0.weight": g.normal(scale=1 / np.sqrt(K), size=(1024, K)), "flow.fc_head.layers.0.bias": g.normal(scale=0.05, size=1024),
          "flow.fc_head.layers.2.weight": g.normal(scale=0.04 / 32, size=(13, 1024)), "flow.fc_head.layers.2.bias": g.normal(scale=0.01, size=13),
          "flow.fc_head.init_betas": g.normal(scale=0.5, size=(1, 1, 10)), "flow.fc_head.init_cam": np.array([0.9, 0.01, -0.02]).reshape(1, 1, 3)}
    if zero_scale:                      # s = off[10] + init_cam[0] = 0 exactly: the reference's unclamped conversion gives inf
        sd["flow.fc_head.layers.2.weight"][10] = 0.0
        sd["flow.fc_head.layers.2.bias"][10] = 0.0
        sd["flow.fc_head.init_cam"][0, 0, 0] = 0.0
    return {k: v.astype(np.float32) for k, v in sd.items()}


def _inputs(g, B):
    return dict(img_feats=g.uniform(0, 2, size=(B, 2048)).astype(np.float32), scene_feats=g.normal(size=(B, 512)).astype(np.float32),
                fx=g.uniform(0.8, 1.2, B).astype(np.float32), cam_cx=g.uniform(900, 1000, B).astype(np.float32),
                cam_cy=g.uniform(500, 580, B).astype(np.float32),
                box_center=np.stack([g.uniform(300, 1600, B), g.uniform(150, 950, B)], -1).astype(np.float32), box_size=g.uniform(120, 700, B).astype(np.float32))


@pytest.mark.parametrize("flags", list(itertools.product((False, True), repeat=3)), ids=lambda f: "fl{}bb{}cc{}".format(*map(int, f)))
def test_head_kernel_matches_float64_restatement(dev, flags):
    from egohmr_amd.stage1 import ProHMRSceneTransl
    from tests.test_stage1_cpu import stage1_context_lead
    fl, bb, cc = flags
    m = ProHMRSceneTransl(with_focal_length=fl, with_bbox_info=bb, with_cam_center=cc).to(dev)
    g = np.random.Generator(np.random.PCG64(100 + 4 * fl + 2 * bb + cc))
    worst = 0.0
    for B, zero_scale in ((1, False), (7, False), (256, False), (257, False), (7, True)):
        sd = _head_weights(g, m.context_dim, zero_scale)
        m.flow.fc_head.load_state_dict({k[len("flow.fc_head."):]: torch.from_numpy(v) for k, v in sd.items()})
        x = _inputs(g, B)
        out = m.head(*(torch.from_numpy(x[k]).to(dev) for k in ("img_feats", "scene_feats", "fx", "cam_cx", "cam_cy", "box_center", "box_size")))
        lead = stage1_context_lead(x["fx"], x["cam_cx"], x["cam_cy"], x["box_center"], x["box_size"], with_focal_length=fl, with_bbox_info=bb,
                                   with_cam_center=cc, dtype=np.float32)
        ctx = np.concatenate([lead, x["img_feats"], x["scene_feats"]], 1)
        cam, full, betas = stage1_head_f64(ctx, sd, x["fx"], x["cam_cx"], x["cam_cy"], x["box_center"], x["box_size"])
        got = out["pred_cam_full"].cpu().numpy().astype(np.float64)
        if zero_scale:
            assert np.isinf(full).all() and np.array_equal(np.isinf(got), np.isinf(full)) and np.array_equal(np.sign(got), np.sign(full)), (got, full)
            continue
        assert 0.6 < cam[:, 0].min() and cam[:, 0].max() < 1.2                       # (a camera in the range the conversion is meant for)
        np.testing.assert_allclose(got, full, rtol=0, atol=1e-5)
        np.testing.assert_allclose(out["pred_cam"].cpu().numpy(), cam, rtol=0, atol=1e-6)
        np.testing.assert_allclose(out["pred_betas"].cpu().numpy(), betas, rtol=0, atol=1e-5)
        worst = max(worst, float(np.abs(got - full).max()))
    print(f"stage-1 head, flags {flags}: max |pred_cam_full - float64| = {worst:.2e} m")


def _g19_batch(g, dev):
    b = syn.make_batch(5, int(g["num_scene_points"]), seed=int(g["batch_seed"]))
    batch = {"img": b["img"], "scene_pcd_verts_full": b["scene_pcd_verts_full"], **{k: g[k] for k in ("fx", "cam_cx", "cam_cy", "box_center", "box_size")}}
    return {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in batch.items()}


def _stage1_model(tag, dev):
    from egohmr_amd import io as eio
    from egohmr_amd.stage1 import ProHMRSceneTransl
    m = ProHMRSceneTransl(**FLAGS[tag])
    eio.load_stage1_checkpoint(m, {"state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in syn.make_stage1_state_dict(0, **FLAGS[tag]).items()}})
    return m.to(dev)


@pytest.mark.parametrize("tag", list(FLAGS))
def test_full_model_matches_reference_golden(dev, golden_dir, tag):
    g = np.load(os.path.join(golden_dir, f"g19_stage1_{tag}.npz"))
    m = _stage1_model(tag, dev)
    out = m(_g19_batch(g, dev))
    err = float(np.abs(out["pred_cam_full"].cpu().numpy() - g["pred_cam_full"]).max())
    ecam = float(np.abs(out["pred_cam"].cpu().numpy() - g["pred_cam"]).max())
    print(f"g19 {tag}: max |pred_cam_full - reference| = {err:.2e} m, max |pred_cam - reference| = {ecam:.2e}")
    assert err <= 1e-4
    np.testing.assert_allclose(out["pred_betas"].cpu().numpy(), g["pred_betas"], rtol=0, atol=1e-4)


# --------------------------------------------------------------------------------------------- stage 2 on stage 1's results
@pytest.fixture(scope="module")
def stage2(dev, synth_weights, smpl_asset):
    from egohmr_amd import smpl as smpl_mod
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import build_synthetic_model
    B, N, S, n, rs = 5, 1024, 2, 50, "ddim5"
    model = build_synthetic_model(dev, 0, state_dict=synth_weights, smpl_asset=smpl_asset)
    bnp = syn.make_batch(B, N, seed=23, vis_prob=0.5)
    gt = syn.make_gt_annotations(B, seed=23)
    bnp["smpl_params"].update({k: gt[k] for k in ("global_orient", "body_pose", "betas")})
    bnp["gender"] = gt["gender"]
    bnp["smpl_params"]["transl"][0, 0] = 1.9            # two bodies partly out of the 1920 x 1080 frame: invisible joints (test_egohmr.py:374-389)
    bnp["smpl_params"]["transl"][1, 1] = 1.1
    assets = {gname: syn.make_smpl_asset(i) for i, gname in enumerate(("neutral", "male", "female"))}
    assets["neutral"] = smpl_asset
    smpls = {k: smpl_mod.create(asset=a, gender=k).to(dev) for k, a in assets.items()}
    d = create_gaussian_diffusion(num_diffusion_timesteps=n, timestep_respacing=rs)
    noises = [syn.make_noise_stack(d.num_timesteps, B, seed=23 + 10 * s) for s in range(S)]
    return dict(model=model, diffusion=d, smpls=smpls, bnp=bnp, noises=noises, S=S, rs=rs)


def test_results_file_feeds_stage2_bit_equal(dev, golden_dir, stage2, tmp_path):
    from egohmr_amd import io as eio
    from egohmr_amd.driver import Stage1Driver, Stage2Driver
    from egohmr_amd.factory import batch_to_device
    g = np.load(os.path.join(golden_dir, "g19_stage1_all_on.npz"))
    s1 = Stage1Driver(_stage1_model("all_on", dev))
    direct = s1.step(_g19_batch(g, dev))["pred_cam_full"]
    path = s1.save(str(tmp_path), "unit")
    assert path.endswith(os.path.join("output_prohmr_scene_unit", "results.pkl"))
    loaded = eio.load_stage1_cam(path)
    assert np.array_equal(loaded, direct.cpu().numpy())
    sm, S, rs = stage2["smpls"], stage2["S"], stage2["rs"]
    outs = []
    for transl in (torch.from_numpy(loaded).to(dev), direct):
        drv = Stage2Driver(stage2["model"], stage2["diffusion"], sm["neutral"], sm["male"], sm["female"], num_samples=S, timestep_respacing=rs,
                           eval_contact_score=False, two_stage=True)
        b = batch_to_device(stage2["bnp"], dev)
        b["stage1_transl_full"] = transl
        outs.append((drv.step(b, [torch.from_numpy(z).to(dev) for z in stage2["noises"]]), drv.results()))
    (a, ra), (c, rc) = outs
    for k in ("betas", "global_orient", "body_pose"):
        assert torch.equal(a["pred"][k], c["pred"][k]), k
    for k in ("g_mpjpe", "mpjpe", "pa_mpjpe", "v2v", "pa_mpjpe_vis_sum", "pa_mpjpe_invis_sum"):
        assert torch.equal(a[k], c[k]), k
    assert torch.equal(a["decoded"]["joints_full"], c["decoded"]["joints_full"])
    assert np.array_equal(ra["pred_cam_full_list"], rc["pred_cam_full_list"]) and np.array_equal(ra["pred_cam_full_list"], loaded)


def test_driver_visible_joint_pa_mpjpe_matches_restatement(dev, stage2):
    from egohmr_amd.driver import Stage2Driver
    from egohmr_amd.factory import batch_to_device
    sm, S, rs = stage2["smpls"], stage2["S"], stage2["rs"]
    res = {}
    for vis_pa in (False, True):
        drv = Stage2Driver(stage2["model"], stage2["diffusion"], sm["neutral"], sm["male"], sm["female"], num_samples=S, timestep_respacing=rs,
                           eval_contact_score=False, eval_with_vis_mask_pa=vis_pa)
        res[vis_pa] = drv.step(batch_to_device(stage2["bnp"], dev), [torch.from_numpy(z).to(dev) for z in stage2["noises"]])
    r = res[True]
    jvis = r["joint_vis_mask"].cpu().numpy()
    B = jvis.shape[0]
    assert 0 < jvis.sum() < jvis.size and not jvis.all(1).all()                  # some items with invisible joints: the two alignments differ
    pred = r["decoded"]["joints_align"][:, :, :24].cpu().numpy().reshape(B * S, 24, 3)
    gt = np.repeat(r["gt"]["joints_align"][:, None, :24].cpu().numpy(), S, 1).reshape(B * S, 24, 3)
    pj = procrustes_vis_np(np.repeat(jvis[:, None], S, 1).reshape(B * S, 24), pred, gt).reshape(B, S, 24)   # test_egohmr.py:427-437
    np.testing.assert_allclose(r["pa_mpjpe"].cpu().numpy(), pj.mean(-1), rtol=0, atol=1e-6)
    np.testing.assert_allclose(r["pa_mpjpe_vis_sum"].cpu().numpy(), (pj * jvis[:, None]).sum(-1), rtol=0, atol=1e-5)
    np.testing.assert_allclose(r["pa_mpjpe_invis_sum"].cpu().numpy(), (pj * ~jvis[:, None]).sum(-1), rtol=0, atol=1e-5)
    for k in ("g_mpjpe", "mpjpe", "v2v"):                                        # only PA-MPJPE changes
        assert torch.equal(r[k], res[False][k]), k
    assert float((r["pa_mpjpe"] - res[False]["pa_mpjpe"]).abs().max()) > 1e-4


# --------------------------------------------------------------------------------------------- the masked Procrustes kernel
def test_procrustes_vis_kernel_matches_reference_golden(dev, golden_dir):
    from egohmr_amd import metrics as M
    g = np.load(os.path.join(golden_dir, "g20_procrustes_vis.npz"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mask = t(g["mask"])
    r = M.procrustes(t(g["pred"][:, None]), t(g["gt"]), mask=mask, align_mask=mask, per_joint=True)
    np.testing.assert_allclose(r["per_joint"][:, 0].cpu().numpy(), g["per_joint"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(r["mean"][:, 0].cpu().numpy(), g["mean"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(r["vis_sum"][:, 0].cpu().numpy(), g["vis_sum"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(r["invis_sum"][:, 0].cpu().numpy(), g["invis_sum"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(r["per_joint"][:, 0].cpu().numpy(), procrustes_vis_np(g["mask"], g["pred"], g["gt"]), rtol=0, atol=1e-6)
    # J = 45, two samples per item sharing its mask (no J <= 32 limit on this entry)
    m45 = t(g["mask45"])
    r45 = M.procrustes(t(g["pred45"]), t(g["gt45"]), align_mask=m45, per_joint=True)
    np.testing.assert_allclose(r45["per_joint"].cpu().numpy(), g["per_joint45"], rtol=0, atol=1e-6)
    with pytest.raises(ValueError):
        M.procrustes(t(g["pred"][:, None]), t(g["gt"]), mask=mask.clone(), align_mask=mask)


def test_procrustes_vis_kernel_edges(dev, golden_dir):
    from egohmr_amd import metrics as M
    g = np.load(os.path.join(golden_dir, "g20_procrustes_vis.npz"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pred, gt = t(g["pred"][:, None]), t(g["gt"])
    n, J = g["mask"].shape
    # all visible: the plain alignment (ehm_eval_procrustes)
    ones = torch.ones(n, J, dtype=torch.bool, device=dev)
    a = M.procrustes(pred, gt, align_mask=ones, per_joint=True, aligned=True)
    b = M.procrustes(pred, gt, mask=ones, per_joint=True, aligned=True)
    for k in ("per_joint", "aligned", "mean", "vis_sum", "invis_sum"):
        np.testing.assert_allclose(a[k].cpu().numpy(), b[k].cpu().numpy(), rtol=0, atol=1e-6, err_msg=k)
    # no visible joint in item 2: NaN there (var1 = 0, as the reference), the other items untouched
    m = torch.from_numpy(g["mask"]).to(dev).clone()
    m[2] = False
    r = M.procrustes(pred, gt, align_mask=m, per_joint=True)
    assert torch.isnan(r["per_joint"][2]).all() and torch.isnan(r["mean"][2]).all()
    assert torch.isnan(r["vis_sum"][2]).all() and torch.isnan(r["invis_sum"][2]).all()
    keep = [i for i in range(n) if i != 2]
    np.testing.assert_allclose(r["per_joint"][keep, 0].cpu().numpy(), g["per_joint"][keep], rtol=0, atol=1e-6)
