"""GPU: the stage-1 pose flow (csrc/flow.hip: ehm_flow_context, ehm_flow_gemm, ehm_flow_finish; egohmr_amd.stage1.GlowFlow / ProHMRScene;
Stage1Driver's metrics) against the float64 restatement tests/flow_ref.py.

The bar of a tensor is 8 x the largest distance of flow_ref's float32 run from its float64 run on the same inputs, computed here, per case: the
factor the project allows a free-running float32 chain whose summation order differs from the reference's.  Every test prints the
measured error next to its bar.  The shapes are the smallest that reach every edge: R below, across and two tiles of 32 rows, S = 5 so that an
item (r // S) straddles a tile boundary, every (K, N) of the chain, the padded-K context (ctx = 2566) and the exact one (2560)."""
import ctypes as C

import numpy as np
import pytest
import torch

from egohmr_amd import synthetic as syn
from tests import flow_ref as fr

pytestmark = pytest.mark.gpu

ALL_ON = dict(with_focal_length=True, with_bbox_info=True, with_cam_center=True)
ALL_OFF = dict(with_focal_length=False, with_bbox_info=False, with_cam_center=False)
SENTINEL = 12345.0
ODD = np.arange(1, 144, 2)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _check(name, got, want, bar):
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    print(f"{name}: error {err:.2e}, bar {bar:.2e}")
    assert np.isfinite(np.asarray(got)).all() and err <= bar, (name, err, bar)
    return err


# --------------------------------------------------------------------------------------------- ehm_flow_gemm
# (K, N, ldw, prologue, epilogue, gather, scatter): every product of the chain with the steps it carries
GEMM_CASES = {
    "first_layer": (72, 1024, 1024, "none", "item_add", True, False),        # the 72 identity columns out of the 144-wide state, plus the context term
    "hidden_relu": (1024, 1024, 1024, "relu", "bias", False, False),         # linear_layers.0
    "hidden_bn_glu": (1024, 1024, 1024, "bn_relu", "glu_res", False, False),  # linear_layers.1 behind a BatchNorm, GLU gate and residual in place
    "last_layer_add": (1024, 72, 96, "none", "scatter_add", False, True),    # final_layer plus the coupling update, in place on the state
    "last_layer_sub": (1024, 72, 96, "none", "scatter_sub", False, True),
    "affine": (144, 144, 160, "none", "bias", False, False),                 # state A^T + c
    "affine_inverse": (144, 144, 160, "shift", "bias", False, False),        # (state - c) Ainv^T
}
PRO = {"none": 0, "relu": 1, "bn_relu": 2, "shift": 3}
EPI = {"bias": 0, "item_add": 1, "glu_res": 2, "scatter_add": 3, "scatter_sub": 4}


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("case", list(GEMM_CASES))
def test_flow_gemm_matches_float64(dev, case, S):
    from egohmr_amd import _lib
    K, N, ldw, pro, epi, gather, scatter = GEMM_CASES[case]
    g = np.random.Generator(np.random.PCG64(sum(map(ord, case)) + S))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    W = np.zeros((K, ldw), np.float32)
    W[:, :N] = g.normal(scale=1 / np.sqrt(K), size=(K, N))
    bias = f32(g.normal(scale=0.05, size=N))
    ps, po = (f32(g.uniform(0.6, 1.4, size=K)), f32(g.normal(scale=0.2, size=K))) if pro in ("bn_relu", "shift") else (None, None)
    idx_in, idx_out = (ODD.astype(np.int32) if gather else None), (ODD.astype(np.int32) if scatter else None)
    ldx = 144 if gather else K
    ldy = 144 if scatter else N + 8                                   # (a row longer than N: the columns behind N must stay)
    ld_item = N + 32
    Wd, bd, psd, pod, gi, si = t(W), t(bias), t(ps), t(po), t(idx_in), t(idx_out)
    for R in (1, 31, 33, 65):
        guard = 3
        X = f32(g.normal(size=(R + guard, ldx)))
        X[R:] = np.nan                                               # rows >= R: whatever is there must not reach a live output
        item = f32(g.normal(size=(-(-R // S), ld_item)))
        Y0 = f32(g.normal(size=(R + guard, ldy))) if epi in ("glu_res", "scatter_add", "scatter_sub") else np.full((R + guard, ldy), SENTINEL, np.float32)
        Y0[R:] = SENTINEL
        Xd, Yd, itd = t(X), t(Y0.copy()), t(item)
        d = _lib.FlowGemmDesc(X=_lib.ptr(Xd), gather=_lib.ptr(gi), W=_lib.ptr(Wd), bias=_lib.ptr(bd), pro_scale=_lib.ptr(psd), pro_shift=_lib.ptr(pod),
                              item=_lib.ptr(itd) if epi in ("item_add", "glu_res") else None, scatter=_lib.ptr(si), Y=_lib.ptr(Yd), R=R, K=K, N=N, S=S,
                              ldx=ldx, ldw=ldw, ldy=ldy, ld_item=ld_item, prologue=PRO[pro], epilogue=EPI[epi])
        _lib.api().ehm_flow_gemm(C.byref(d), _lib.stream_ptr())
        torch.cuda.synchronize()
        got = Yd.cpu().numpy()
        kw = dict(bias=bias, gather=idx_in, prologue=pro, pro_scale=ps, pro_shift=po, epilogue=epi, item=item[:, :N], scatter=idx_out, S=S)
        y_in = Y0[:R] if scatter else Y0[:R, :N]
        want = fr.flow_gemm(X[:R], W[:, :N], Y=y_in, **kw)
        bar = 8 * float(np.abs(fr.flow_gemm(X[:R], W[:, :N], Y=y_in, dtype=np.float32, **kw) - want).max())
        _check(f"{case} S = {S} R = {R}", got[:R] if scatter else got[:R, :N], want, bar)
        assert np.array_equal(got[R:], Y0[R:]), "rows >= R were written"
        if scatter:
            assert np.array_equal(got[:R, 0::2], Y0[:R, 0::2]), "columns outside the scatter list were written"
        else:
            assert np.array_equal(got[:R, N:], Y0[:R, N:]), "columns >= N were written"


def test_flow_context_is_the_heads_context_with_a_zero_pad(dev):
    from egohmr_amd.stage1 import ProHMRScene
    from tests.test_stage1_cpu import stage1_context_lead
    g = np.random.Generator(np.random.PCG64(77))
    B = 3
    x = dict(img_feats=g.uniform(0, 2, size=(B, 2048)).astype(np.float32), scene_feats=g.normal(size=(B, 512)).astype(np.float32),
             fx=g.uniform(0.8, 1.2, B).astype(np.float32), cam_cx=g.uniform(900, 1000, B).astype(np.float32), cam_cy=g.uniform(500, 580, B).astype(np.float32),
             box_center=np.stack([g.uniform(300, 1600, B), g.uniform(150, 950, B)], -1).astype(np.float32), box_size=g.uniform(120, 700, B).astype(np.float32))
    for flags in (ALL_ON, ALL_OFF, dict(with_focal_length=True, with_bbox_info=False, with_cam_center=True)):
        m = ProHMRScene(**flags).to(dev)
        out = m.conditioning(*(torch.from_numpy(x[k]).to(dev) for k in ("img_feats", "scene_feats", "fx", "cam_cx", "cam_cy", "box_center", "box_size"))).cpu().numpy()
        lead = stage1_context_lead(x["fx"], x["cam_cx"], x["cam_cy"], x["box_center"], x["box_size"], dtype=np.float64, **flags)
        n = lead.shape[1]
        assert out.shape == (B, -(-m.context_dim // 32) * 32) and n + 2560 == m.context_dim
        np.testing.assert_allclose(out[:, :n], lead, rtol=2e-7, atol=0)
        assert np.array_equal(out[:, n:n + 2048], x["img_feats"]) and np.array_equal(out[:, n + 2048:n + 2560], x["scene_feats"])
        assert not out[:, m.context_dim:].any()


# --------------------------------------------------------------------------------------------- whole directions
B_DIR, S_DIR = 3, 5
DIRECTION_CASES = {"all_on": (ALL_ON, False), "all_on_bn": (ALL_ON, True), "all_off": (ALL_OFF, False), "all_off_bn": (ALL_OFF, True)}
# The rotations are compared at atol 2e-6.  A Gram-Schmidt step in float32 loses about 2 ulp / sin(angle between the joint's two vectors), so that
# tolerance holds for sines above ~0.06; 360 random joints nearly always hold a smaller one.  The inputs' seeds are therefore those, of 400 .. 411,
# at which the FLOAT64 reference's samples keep every sine above 0.1 (asserted below; nothing of the device enters the choice).
INPUT_SEEDS = {"all_on": 402, "all_on_bn": 407, "all_off": 409, "all_off_bn": 407}
MIN_SINE = 0.1
_direction_cache = {}


def _context_rows(g, B, ctx):
    return np.concatenate([g.normal(scale=0.3, size=(B, ctx - 2560)), g.uniform(0, 2, size=(B, 2048)), g.normal(size=(B, 512))], 1).astype(np.float32)


def _flow_on_device(sd, ctx, bn, dev):
    from egohmr_amd.stage1 import GlowFlow
    f = GlowFlow(ctx, batch_norm=bn)
    f.load_state_dict({k[len("flow.flow."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return f.to(dev)


def _sines(x):
    """The sine between the two 3-vectors of every joint of the 6-D poses x [..., 144], [n]: the conditioning of its Gram-Schmidt step."""
    p = np.asarray(x, np.float64).reshape(-1, 6)
    c = np.cross(p[:, :3], p[:, 3:])
    return np.linalg.norm(c, axis=1) / np.linalg.norm(p[:, :3], axis=1) / np.linalg.norm(p[:, 3:], axis=1)


def direction_case(name, dev):
    """Weights, inputs and the float64 / float32 references of one case, computed once and shared (never modified)."""
    if name not in _direction_cache:
        flags, bn = DIRECTION_CASES[name]
        seed = 10 + list(DIRECTION_CASES).index(name)
        sd = syn.make_stage1_flow_state_dict(seed, batch_norm=bn, **flags)
        ctx = syn.stage1_context_dim(**flags)
        g = np.random.Generator(np.random.PCG64(INPUT_SEEDS[name]))
        c = _context_rows(g, B_DIR, ctx)
        z = g.normal(size=(B_DIR, S_DIR, 144)).astype(np.float32)
        z[:, 0] = 0.0
        zr, cr = z.reshape(-1, 144), np.repeat(c, S_DIR, 0)
        x64, lp64 = fr.sample_and_log_prob(sd, zr, cr)
        x32, lp32 = fr.sample_and_log_prob(sd, zr, cr, np.float32)
        _direction_cache[name] = dict(sd=sd, ctx=ctx, c=c, z=z, cr=cr, x64=x64, lp64=lp64, bar_x=8 * float(np.abs(x32 - x64).max()),
                                      bar_lp=8 * float(np.abs(lp32 - lp64).max()), flow=_flow_on_device(sd, ctx, bn, dev))
    return _direction_cache[name]


@pytest.mark.parametrize("name", list(DIRECTION_CASES))
def test_directions_match_float64(dev, name):
    k = direction_case(name, dev)
    flow, t = k["flow"], lambda a: torch.from_numpy(a).to(dev)
    out = flow.sample_and_log_prob(t(k["c"]), z=t(k["z"]))
    p6 = out["pred_pose_6d"].cpu().numpy()
    assert p6.shape == (B_DIR, S_DIR, 144) and out["log_prob"].shape == (B_DIR, S_DIR) and torch.equal(out["z"], t(k["z"]))
    assert out["global_orient"].shape == (B_DIR, S_DIR, 1, 3, 3) and out["body_pose"].shape == (B_DIR, S_DIR, 23, 3, 3)
    _check(f"{name}: pred_pose_6d", p6.reshape(-1, 144), k["x64"], k["bar_x"])
    _check(f"{name}: log_prob (sampling)", out["log_prob"].cpu().numpy().reshape(-1), k["lp64"], k["bar_lp"])
    # the rotations, teacher-forced: the float64 'prohmr' rule on the device's own pred_pose_6d (well-conditioned Gram-Schmidt steps only)
    assert _sines(k["x64"]).min() > MIN_SINE, "a sampled joint's two vectors are nearly parallel: the 2e-6 below assumes they are not"
    rot = torch.cat([out["global_orient"], out["body_pose"]], 2).cpu().numpy().reshape(-1, 3, 3)
    err = float(np.abs(rot - fr.rot6d_prohmr(p6)).max())
    print(f"{name}: rotations against float64 on the device's pose: {err:.2e} (atol 2e-6), smallest sine {_sines(k['x64']).min():.3f}")
    assert err <= 2e-6
    # the forward direction on the device's own samples
    xr = p6.reshape(-1, 144)
    lpf64, z64 = fr.log_prob(k["sd"], xr, k["cr"])
    lpf32, z32 = fr.log_prob(k["sd"], xr, k["cr"], np.float32)
    bar_z, bar_lpf = 8 * float(np.abs(z32 - z64).max()), 8 * float(np.abs(lpf32 - lpf64).max())
    lp_d, z_d = flow.log_prob(out["pred_pose_6d"], t(k["c"]))
    assert lp_d.shape == (B_DIR, S_DIR) and z_d.shape == (B_DIR, S_DIR, 144)
    _check(f"{name}: z (forward)", z_d.cpu().numpy().reshape(-1, 144), z64, bar_z)
    _check(f"{name}: log_prob (forward)", lp_d.cpu().numpy().reshape(-1), lpf64, bar_lpf)
    # the device round trip, and the two directions' log_prob of the same rows (the forward side's bar: its z carries the chain's error)
    _check(f"{name}: round trip z", z_d.cpu().numpy(), k["z"].astype(np.float64), 2 * bar_z)
    _check(f"{name}: log_prob, sampling side against forward side", lp_d.cpu().numpy(), out["log_prob"].cpu().numpy().astype(np.float64), bar_lpf)


@pytest.mark.parametrize("name", ["all_on", "all_off_bn"])
def test_directions_are_deterministic_and_the_mode_does_not_depend_on_S(dev, name):
    k = direction_case(name, dev)
    flow, c, z = k["flow"], torch.from_numpy(k["c"]).to(dev), torch.from_numpy(k["z"]).to(dev)
    a, b = flow.sample_and_log_prob(c, z=z), flow.sample_and_log_prob(c, z=z)
    for key in ("pred_pose_6d", "log_prob", "global_orient", "body_pose"):
        assert torch.equal(a[key], b[key]), key
    (lp1, z1), (lp2, z2) = flow.log_prob(a["pred_pose_6d"], c), flow.log_prob(a["pred_pose_6d"], c)
    assert torch.equal(lp1, lp2) and torch.equal(z1, z2)
    mode = flow.sample_and_log_prob(c, z=torch.zeros(B_DIR, 1, 144, device=dev))
    for key in ("pred_pose_6d", "log_prob", "global_orient", "body_pose"):
        assert torch.equal(mode[key][:, 0], a[key][:, 0]), key
    drawn = flow.sample_and_log_prob(c, num_samples=2)
    assert drawn["z"].shape == (B_DIR, 2, 144) and drawn["pred_pose_6d"].shape == (B_DIR, 2, 144) and bool(torch.isfinite(drawn["log_prob"]).all())


# --------------------------------------------------------------------------------------------- ProHMRScene.forward
@pytest.fixture(scope="module")
def scene_setup(dev, smpl_asset):
    from egohmr_amd import io as eio
    from egohmr_amd import smpl as smpl_mod
    from egohmr_amd.factory import batch_to_device
    from egohmr_amd.stage1 import ProHMRScene, ProHMRSceneTransl
    sd = {**syn.make_stage1_state_dict(0), **syn.make_stage1_flow_state_dict(0)}
    ck = {"state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}
    smpl = smpl_mod.create(asset=smpl_asset, gender="neutral").to(dev)
    model = ProHMRScene(smpl=smpl)
    eio.load_stage1_checkpoint(model, ck, flow=True)
    transl = ProHMRSceneTransl()
    eio.load_stage1_checkpoint(transl, ck)
    b = syn.make_batch(3, 256, seed=31)
    gt = syn.make_gt_annotations(3, seed=31)
    b["smpl_params"].update({k: gt[k] for k in ("global_orient", "body_pose", "betas")})
    b["gender"] = gt["gender"]
    return dict(sd=sd, model=model.to(dev), transl=transl.to(dev), smpl=smpl, batch=batch_to_device(b, dev))


def _first(batch, n):
    return {k: ({kk: vv[:n] for kk, vv in v.items()} if isinstance(v, dict) else v[:n]) for k, v in batch.items()}


def test_prohmr_scene_forward(dev, scene_setup, smpl_asset):
    from tests import smpl_ref as R
    from types import SimpleNamespace
    model, B, S = scene_setup["model"], 2, 3
    batch = _first(scene_setup["batch"], B)
    z = torch.from_numpy(np.random.Generator(np.random.PCG64(8)).normal(size=(B, S, 144)).astype(np.float32)).to(dev)
    z[:, 0] = 0
    out = model(batch, z=z)
    V, ctx = smpl_asset["v_template"].shape[0], 2566
    shapes = {"pred_cam": (B, S, 3), "log_prob": (B, S), "conditioning_feats": (B, ctx), "pred_pose_6d": (B, S, 144), "pred_keypoints_3d": (B, S, 45, 3),
              "pred_vertices": (B, S, V, 3), "pred_cam_t": (B, S, 3), "pred_cam_t_full": (B, S, 3), "pred_keypoints_3d_full": (B, S, 45, 3),
              "pred_keypoints_2d_full": (B, S, 45, 2), "pred_keypoints_2d": (B, S, 45, 2), "pred_cam_full": (B, 3), "pred_betas": (B, 10)}
    assert set(out) == set(shapes) | {"pred_smpl_params"}
    assert {k: tuple(out[k].shape) for k in shapes} == shapes
    sp = out["pred_smpl_params"]
    assert {k: tuple(v.shape) for k, v in sp.items()} == {"global_orient": (B, S, 1, 3, 3), "body_pose": (B, S, 23, 3, 3), "betas": (B, S, 10)}
    # the camera and the betas: the bits of ProHMRSceneTransl on the same weights, broadcast over the samples
    ref = scene_setup["transl"](batch)
    assert torch.equal(out["pred_cam_full"], ref["pred_cam_full"]) and torch.equal(out["pred_betas"], ref["pred_betas"])
    for s in range(S):
        assert torch.equal(out["pred_cam"][:, s], ref["pred_cam"]) and torch.equal(sp["betas"][:, s], ref["pred_betas"])
        assert torch.equal(out["pred_cam_t_full"][:, s], ref["pred_cam_full"])
    # the flow, teacher-forced on the returned conditioning_feats
    c = out["conditioning_feats"].cpu().numpy()
    cr, zr = np.repeat(c, S, 0), z.cpu().numpy().reshape(-1, 144)
    x64, lp64 = fr.sample_and_log_prob(scene_setup["sd"], zr, cr)
    x32, lp32 = fr.sample_and_log_prob(scene_setup["sd"], zr, cr, np.float32)
    _check("forward: pred_pose_6d", out["pred_pose_6d"].cpu().numpy().reshape(-1, 144), x64, 8 * float(np.abs(x32 - x64).max()))
    _check("forward: log_prob", out["log_prob"].cpu().numpy().reshape(-1), lp64, 8 * float(np.abs(lp32 - lp64).max()))
    rot = torch.cat([sp["global_orient"], sp["body_pose"]], 2).cpu().numpy().reshape(B * S, 24, 3, 3)
    # (here the context comes from the encoders and the joints are taken as they fall: 2e-6 on the well-conditioned ones, and on EVERY joint the
    # first-order bound of the float32 Gram-Schmidt chain at its own sine - u = 2^-24; b1 within 3 u; d = b1 . a2 within 6 u |a2|; a2 - d b1 within
    # 11 u |a2| a component, 19 u |a2| in norm, against a length of |a2| sine; normalised + 3 u; the cross product doubles it: 40 u / sine + 10 u)
    sines = _sines(out["pred_pose_6d"].cpu().numpy())
    well = sines > MIN_SINE
    assert well.mean() > 0.9
    rot_err = np.abs(rot.reshape(-1, 3, 3) - fr.rot6d_prohmr(out["pred_pose_6d"].cpu().numpy())).max((1, 2))
    print(f"forward: rotations, {well.sum()} joints of {well.size} above sine {MIN_SINE}: {rot_err[well].max():.2e} (atol 2e-6); all joints, error / "
          f"(40 u / sine + 10 u): {(rot_err / ((40 / sines + 10) * 2.0 ** -24)).max():.3f}, smallest sine {sines.min():.4f}")
    assert rot_err[well].max() <= 2e-6
    assert (rot_err <= (40 / sines + 10) * 2.0 ** -24).all()
    # the SMPL decode against the float64 oracle on the returned rotations and betas, under the bound of tests/test_gpu_smpl_forward.py
    betas = sp["betas"].cpu().numpy().reshape(B * S, 10)
    got = SimpleNamespace(vertices=out["pred_vertices"].cpu().numpy().reshape(B * S, V, 3), joints=out["pred_keypoints_3d"].cpu().numpy().reshape(B * S, 45, 3), A=None)
    assert R.path_of(smpl_asset, B * S) == "valu"
    r = R.ratios(got, R.bound_valu(smpl_asset, betas, rot))
    print("forward: SMPL decode, error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    # the garnish follows its definition (prohmr_scene.py:187-222) on the returned tensors
    focal = (batch["fx"] * 1500.0).reshape(B, 1)
    want_t = torch.stack([out["pred_cam"][:, :, 1], out["pred_cam"][:, :, 2], 2 * focal / (224 * out["pred_cam"][:, :, 0] + 1e-9)], -1)
    torch.testing.assert_close(out["pred_cam_t"], want_t, rtol=1e-6, atol=0)
    torch.testing.assert_close(out["pred_keypoints_3d_full"], out["pred_keypoints_3d"] + ref["pred_cam_full"][:, None, None], rtol=0, atol=0)
    p = (out["pred_keypoints_3d"] + want_t[:, :, None]).double()
    want_2d = (focal.double()[:, :, None, None] * p[..., :2] / p[..., 2:]) / 224
    torch.testing.assert_close(out["pred_keypoints_2d"].double(), want_2d, rtol=1e-5, atol=1e-6)
    pf = out["pred_keypoints_3d_full"].double()
    cen = torch.stack([batch["cam_cx"], batch["cam_cy"]], -1).double()[:, None, None]
    uv = focal.double()[:, :, None, None] * pf[..., :2] / pf[..., 2:] + cen
    want_full = torch.stack([uv[..., 0] / 1920 - 0.5, uv[..., 1] / 1080 - 0.5], -1)
    torch.testing.assert_close(out["pred_keypoints_2d_full"].double(), want_full, rtol=1e-5, atol=1e-6)
    # an explicit z: two calls, the same bits
    again = model(batch, z=z)
    for key in shapes:
        assert torch.equal(out[key], again[key]), key
    # log_prob of the returned samples gives the noise back (smpl_flow.py:31-50's interface)
    lp, zb = model.log_prob({"global_orient": out["pred_pose_6d"][:, :, :6], "body_pose": out["pred_pose_6d"][:, :, 6:]}, out["conditioning_feats"])
    assert lp.shape == (B, S) and float((zb - z).abs().max()) < 1e-3


def test_loader_loads_into_a_model_already_on_the_device(dev, scene_setup):
    """INTEGRATION.md's order: ProHMRScene(...).to(device), then load_stage1_checkpoint(..., flow=True) - the model's own buffers are device tensors."""
    from egohmr_amd import io as eio
    from egohmr_amd.stage1 import ProHMRScene
    ck = {"state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in scene_setup["sd"].items()}}
    m = ProHMRScene(smpl=scene_setup["smpl"]).to(dev)
    assert eio.load_stage1_checkpoint(m, ck, flow=True) == sorted(scene_setup["sd"])
    want = scene_setup["model"].state_dict()
    got = m.state_dict()
    assert all(v.is_cuda and torch.equal(v, want[k]) for k, v in got.items())
    # a checkpoint whose tensors live on the device as well, and the refusals that read a value there
    on_dev = {"state_dict": {k: v.to(dev) for k, v in ck["state_dict"].items()}}
    assert eio.load_stage1_checkpoint(m, on_dev, flow=True) == sorted(scene_setup["sd"])
    on_dev["state_dict"]["flow.flow._transform._transforms.6.initialized"] = torch.tensor(False, device=dev)
    with pytest.raises(ValueError, match="initialized == False"):
        eio.load_stage1_checkpoint(m, on_dev, flow=True)
    batch = _first(scene_setup["batch"], 2)
    z = torch.zeros(2, 2, 144, device=dev)
    z[:, 1] = 0.25
    a, b = m(batch, z=z), scene_setup["model"](batch, z=z)
    assert torch.equal(a["pred_pose_6d"], b["pred_pose_6d"]) and torch.equal(a["log_prob"], b["log_prob"]) and torch.equal(a["pred_cam_full"], b["pred_cam_full"])


def test_prohmr_scene_draws_from_the_global_generator(dev, scene_setup):
    model, B, S = scene_setup["model"], 2, 3
    batch = _first(scene_setup["batch"], B)
    torch.manual_seed(1234)
    out = model(batch, num_samples=S)
    after = torch.randn(4, device=dev)
    torch.manual_seed(1234)
    drawn = torch.randn(B * (S - 1), 144, device=dev)
    assert torch.equal(after, torch.randn(4, device=dev)), "the draw did not consume exactly B (S - 1) 144 normals"
    z = torch.zeros(B, S, 144, device=dev)
    z[:, 1:] = drawn.reshape(B, S - 1, 144)
    want = model(batch, z=z)
    assert torch.equal(out["pred_pose_6d"], want["pred_pose_6d"]) and torch.equal(out["log_prob"], want["log_prob"])
    one = model(batch, num_samples=1)
    assert torch.equal(one["pred_pose_6d"][:, 0], out["pred_pose_6d"][:, 0]) and torch.equal(one["log_prob"][:, 0], out["log_prob"][:, 0])


# --------------------------------------------------------------------------------------------- Stage1Driver's metrics
def _procrustes_np(S1, S2):
    """utils/pose_utils.py:10-66 for one pair of [n,3] clouds, float64: the similarity transform of S1 closest to S2."""
    mu1, mu2 = S1.mean(0), S2.mean(0)
    X1, X2 = S1 - mu1, S2 - mu2
    K = X1.T @ X2
    U, _, Vh = np.linalg.svd(K)
    Z = np.eye(3)
    Z[-1, -1] = np.sign(np.linalg.det(U @ Vh))
    Rm = Vh.T @ Z @ U.T
    scale = np.trace(Rm @ K) / (X1 ** 2).sum()
    return scale * S1 @ Rm.T + (mu2 - scale * Rm @ mu1)


def test_stage1_driver_metrics_match_the_numpy_restatement(dev, scene_setup, smpl_asset):
    from egohmr_amd import smpl as smpl_mod
    from egohmr_amd.driver import Stage1Driver
    smpls = {"neutral": scene_setup["smpl"], **{k: smpl_mod.create(asset=syn.make_smpl_asset(i), gender=k).to(dev) for i, k in ((1, "male"), (2, "female"))}}
    batch, B = scene_setup["batch"], 3
    drv = Stage1Driver(scene_setup["model"], smpls["neutral"], smpls["male"], smpls["female"], num_samples=2)
    z = torch.zeros(B, 2, 144, device=dev)
    z[:, 1] = 0.5
    r = drv.step(batch, z=z)
    assert set(batch["gender"].tolist()) == {0, 1}                     # both body models are in play
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    # test_prohmr_scene.py:195-232 restated on the model's outputs (the SMPL kernels have their own tests): mode bodies, male / female ground truth
    sp = r["pred_smpl_params"]
    o = smpls["neutral"](betas=sp["betas"][:, 0].contiguous(), body_pose=sp["body_pose"][:, 0].contiguous(), global_orient=sp["global_orient"][:, 0].contiguous(),
                         pose2rot=False)
    pj, pv, cam = f64(o.joints)[:, :24], f64(o.vertices), f64(r["pred_cam_full"])
    kw = dict(global_orient=batch["smpl_params"]["global_orient"], transl=batch["smpl_params"]["transl"], body_pose=batch["smpl_params"]["body_pose"],
              betas=batch["smpl_params"]["betas"])
    male, female = smpls["male"](**kw), smpls["female"](**kw)
    fem = f64(batch["gender"]) == 1
    gj = np.where(fem[:, None, None], f64(female.joints), f64(male.joints))[:, :24]
    gv = np.where(fem[:, None, None], f64(female.vertices), f64(male.vertices))
    pja, pva, gja, gva = pj - pj[:, :1], pv - pj[:, :1], gj - gj[:, :1], gv - gj[:, :1]
    err = lambda a, b: np.sqrt(((a - b) ** 2).sum(-1)).mean(-1)
    want = {"g_mpjpe": err(pj + cam[:, None], gj), "mpjpe": err(pja, gja),                                                   # :293-300
            "pa_mpjpe": np.array([err(_procrustes_np(pja[i], gja[i]), gja[i]) for i in range(B)]),                          # :303-306
            "g_v2v": err(pv + cam[:, None], gv), "v2v": err(pva, gva),                                                       # :309-316
            "pa_v2v": np.array([err(_procrustes_np(pva[i], gva[i]), gva[i]) for i in range(B)])}                            # :319-321
    for k, w in want.items():
        got = f64(r[k])
        print(f"{k}: {got} against {w}")
        assert got.shape == (B,)
        np.testing.assert_allclose(got, w, rtol=0, atol=1e-6, err_msg=k)
    drv.step(batch, z=z)
    s = drv.summary()
    assert list(s) == ["G-MPJPE", "MPJPE", "PA-MPJPE", "G-V2V", "V2V", "PA-V2V"]
    for (name, key) in Stage1Driver.METRICS:
        np.testing.assert_allclose(s[name], 1000 * want[key].mean(), rtol=0, atol=1e-3, err_msg=name)     # millimetres: 1e-6 m on the mean
    assert drv.results()["pred_cam_full_list"].shape == (2 * B, 3)
    # without the body models it is the translation driver, on either model
    plain = Stage1Driver(scene_setup["transl"])
    assert torch.equal(plain.step(batch)["pred_cam_full"], r["pred_cam_full"]) and plain.summary() == {}
