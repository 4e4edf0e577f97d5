"""GPU: behaviour of the reference's call surface beyond plain parity - RNG draw order, dump_steps, skip_timesteps /
init_data, multiple samples per item, error behaviour, konia rotmat->axis-angle, SMPL_*.pkl loading without chumpy."""
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch

from egohmr_amd import synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, synth_weights, smpl_asset):
    from egohmr_amd.factory import build_synthetic_model
    return build_synthetic_model(dev, 0, diffuse_fuse=True, state_dict=synth_weights, smpl_asset=smpl_asset)


def _batch(dev, B=3, N=512, seed=9):
    from egohmr_amd.factory import batch_to_device
    return batch_to_device(syn.make_batch(B, N, seed=seed), dev)


@pytest.mark.parametrize("rs", ["", "ddim5"])
def test_rng_draw_order_matches_reference(dev, model, rs):
    """Without an explicit noise stack the sampler must consume torch's generator exactly like the reference:
    randn(*shape) once, then randn_like once per step including t == 0 (gaussian_diffusion.py:478,331,547)."""
    from egohmr_amd.diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion(num_diffusion_timesteps=20, timestep_respacing=rs)
    B = 3
    torch.manual_seed(1234)
    rows = [torch.randn(B, 144, device=dev)]
    for _ in range(d.num_timesteps):
        rows.append(torch.randn_like(rows[0]))
    after = torch.randn(4, device=dev)                      # generator position after the loop
    expect = d.val_losses(model, _batch(dev), shape=[B, 144], timestep_respacing=rs, compute_loss=False, noise_stack=torch.stack(rows))
    for fused in (True, False):
        d.allow_fused = fused
        torch.manual_seed(1234)
        got = d.val_losses(model, _batch(dev), shape=[B, 144], timestep_respacing=rs, compute_loss=False)
        assert torch.equal(torch.randn(4, device=dev), after), "generator consumed differently from the reference's loop"
        np.testing.assert_allclose(got["pred_vertices"].cpu().numpy(), expect["pred_vertices"].cpu().numpy(), atol=2e-6)


def test_dump_steps_and_progressive_loop(dev, model):
    from egohmr_amd.diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion(num_diffusion_timesteps=10, timestep_respacing="")
    B = 2
    noise = torch.from_numpy(syn.make_noise_stack(10, B, seed=3)).to(dev)
    b = _batch(dev, B)
    steps = list(d.p_sample_loop_progressive(model, b, [B, 144], noise_stack=noise))
    assert len(steps) == 10 and set(steps[0]) == {"sample", "pred_xstart", "other_outputs"}
    dump = d.p_sample_loop(model, _batch(dev, B), [B, 144], dump_steps=[0, 4, 9], noise_stack=noise)
    assert isinstance(dump, list) and len(dump) == 3
    for got, k in zip(dump, (0, 4, 9)):
        np.testing.assert_allclose(got.cpu().numpy(), steps[k]["sample"].cpu().numpy(), atol=1e-6)
    old = model.f16x3_last_steps
    model.f16x3_last_steps = None                        # route equivalence: the step-wise route has no precision schedule
    try:
        fused = model.fused_sampler.run(d, _batch(dev, B), noise, ddim=False)
    finally:
        model.f16x3_last_steps = old
    np.testing.assert_allclose(fused["sample"].cpu().numpy(), steps[-1]["sample"].cpu().numpy(), atol=2e-6)
    sched = model.fused_sampler.run(d, _batch(dev, B), noise, ddim=False)              # default schedule (k = 4 of 10): within its measured error
    np.testing.assert_allclose(sched["sample"].cpu().numpy(), steps[-1]["sample"].cpu().numpy(), atol=2e-5)


def test_skip_timesteps_and_init_data(dev, model):
    from egohmr_amd.diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion(num_diffusion_timesteps=10, timestep_respacing="")
    B = 2
    calls = []
    orig = model.forward

    def spy(batch, t, **kw):
        calls.append(int(t[0]))
        return orig(batch, t, **kw)

    model.forward = spy
    try:
        torch.manual_seed(0)
        init = torch.zeros(B, 144, device=dev)
        out = d.p_sample_loop(model, _batch(dev, B), [B, 144], skip_timesteps=7, init_data=init)
    finally:
        model.forward = orig
    assert calls == [2, 1, 0]                                   # indices T-1-skip .. 0 (gaussian_diffusion.py:483)
    assert torch.isfinite(out["sample"]).all() and out["sample"].shape == (B, 144)


def test_multiple_samples_share_conditioning(dev, model):
    """test_egohmr.py:251-266: S sequential val_losses calls over the SAME batch object; conditioning is encoded once."""
    from egohmr_amd.diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="ddim5")
    B, S = 3, 4
    b = _batch(dev, B)
    outs = []
    n_enc = []
    orig = model.fused_sampler._backbone_fn

    def count():
        n_enc.append(1)
        return orig()

    model.fused_sampler._backbone_fn = count
    try:
        for s in range(S):
            outs.append(d.val_losses(model, b, shape=[B, 144], timestep_respacing="ddim5", compute_loss=False,
                                     noise_stack=torch.from_numpy(syn.make_noise_stack(5, B, seed=100 + s)).to(dev)))
    finally:
        model.fused_sampler._backbone_fn = orig
    assert len(n_enc) == 1
    poses = torch.stack([o["pred_smpl_params"]["body_pose"] for o in outs], dim=1)       # [B,S,23,3,3]
    assert poses.shape == (B, S, 23, 3, 3) and float((poses[:, 0] - poses[:, 1]).abs().max()) > 1e-4   # different noise -> different samples
    betas = torch.stack([o["pred_smpl_params"]["betas"] for o in outs], dim=1)
    assert float((betas - betas[:, :1]).abs().max()) == 0.0                             # betas do not depend on the sample


def test_conditioning_cache_sees_weight_changes(dev):
    """The conditioning cached by FusedSampler.prepare is keyed on the version of every weight it passes through (_lib.TensorKey): an
    in-place update, a replaced Parameter object and a load_state_dict each force a re-encode; an untouched model does not."""
    from egohmr_amd.factory import build_synthetic_model
    m = build_synthetic_model(dev, 3)
    fs = m.fused_sampler
    b = _batch(dev, 2)
    p0 = fs.prepare(b)
    assert fs.prepare(b) is p0                                               # unchanged: cache hit
    f0 = p0.img_feats.clone()
    with torch.no_grad():
        m.backbone.layer4[2].conv3.weight.mul_(1.5)                          # in-place: _version bump
    p1 = fs.prepare(b)
    assert p1 is not p0 and float((p1.img_feats - f0).abs().max()) > 0
    f1 = p1.img_feats.clone()
    w = m.backbone.layer4[2].conv3.weight
    m.backbone.layer4[2].conv3.weight = torch.nn.Parameter((w.detach() / 1.5).clone())   # replaced Parameter object
    p2 = fs.prepare(b)
    assert p2 is not p1
    np.testing.assert_allclose(p2.img_feats.cpu().numpy(), f0.cpu().numpy(), atol=2e-5)   # back to the original weights
    s0 = p2.scene_feats.clone()
    sd = {k: v.clone() for k, v in m.scene_enc.state_dict().items()}
    sd["fc_c.bias"] += 1.0
    m.scene_enc.load_state_dict(sd)                                          # load_state_dict copies in place
    p3 = fs.prepare(b)
    assert p3 is not p2
    np.testing.assert_allclose((p3.scene_feats - s0).cpu().numpy(), 1.0, atol=1e-5)
    h0 = p3.h_img.clone()
    with torch.no_grad():
        m.diffusion_model.gconv_input[0].gconv.W.mul_(2.0)                   # denoiser weights: the projections are re-folded
    p4 = fs.prepare(b)
    assert p4 is not p3 and float((p4.h_img - 2.0 * h0).abs().max()) < 1e-4 * float(h0.abs().max())
    assert float((f1 - f0).abs().max()) > 0


@pytest.mark.parametrize("guided", [False, True])
def test_run_samples_equals_sequential_runs(dev, model, guided):
    """FusedSampler.run_samples (S samples of a batch as one loop over S*B bodies, conditioning replicated by index) against the
    reference's structure - S sequential loops over the same batch (test_egohmr.py:251-266): bit-equal without guidance (the per-body
    arithmetic does not depend on the batch), within the float-atomics noise of the collision gradient with it."""
    from egohmr_amd.diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion(num_diffusion_timesteps=20, timestep_respacing="")
    B, S, T = 5, 3, 20
    b = _batch(dev, B, N=600)
    if guided:
        b["scene_pcd_verts_full"][:, :200, 1] = b["smpl_params"]["transl"][:, None, 1] - 0.6
    noises = [torch.from_numpy(syn.make_noise_stack(T, B, seed=300 + s)).to(dev) for s in range(S)]
    fs = model.fused_sampler
    seq = [fs.run(d, b, noises[s], ddim=False, guided=guided, cond_grad_weight=2.0 if guided else 1.0) for s in range(S)]
    keys_before = set(b.keys())
    bat = fs.run_samples(d, b, noises, ddim=False, guided=guided, cond_grad_weight=2.0 if guided else 1.0)
    assert len(bat) == S and set(b.keys()) == keys_before                               # the caller's batch is not touched
    for s in range(S):
        for k in ("pred_x_start", "pred_vertices", "pred_keypoints_3d", "pred_keypoints_2d_full", "pred_pose_6d"):
            x, y = bat[s]["other_outputs"][k], seq[s]["other_outputs"][k]
            assert x.shape == y.shape
            if guided:
                np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), atol=2e-5)
            else:
                assert torch.equal(x, y), k
        assert torch.equal(bat[s]["other_outputs"]["pred_smpl_params"]["betas"], seq[s]["other_outputs"]["pred_smpl_params"]["betas"])
        if not guided:
            assert torch.equal(bat[s]["sample"], seq[s]["sample"])
    assert float((seq[0]["sample"] - seq[1]["sample"]).abs().max()) > 1e-3              # different noise, different samples


def test_precision_schedule_leaves_the_gcn_handle_as_it_was(dev, model):
    """A sampling call with a precision schedule (plain f16 on the leading steps, split-f16 on the rest) runs every step on its own copy of the
    handle's settings: afterwards the handle reports the precision set before the call, and a granular denoiser evaluation is bit-equal to the
    same evaluation made before it."""
    from egohmr_amd import _lib
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.model import PRECISIONS
    d = create_gaussian_diffusion(num_diffusion_timesteps=20, timestep_respacing="")
    B, lowprec = 4, 12
    b = _batch(dev, B)
    noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B, seed=51)).to(dev)
    fs, L = model.fused_sampler, _lib.lib()
    old = model.gcn_precision
    model.gcn_precision = "f16x3"
    try:
        st = fs.prepare(b)
        tv = fs.timestep_vectors(torch.tensor([7], device=dev))[0]
        x_t = noise[0].contiguous()
        before = fs.denoise_once(st, x_t, tv, 2).clone()
        fs.run(d, b, noise, ddim=False, lowprec=lowprec)
        assert fs.last_lowprec == lowprec
        assert L.ehm_gcn_get_precision(fs._gcn) == PRECISIONS["f16x3"]          # the raw handle: fs.gcn() would set the model's precision again
        after = fs.denoise_once(st, x_t, tv, 2)
    finally:
        model.gcn_precision = old
    assert torch.equal(after, before)


def test_deferred_status_pipeline(dev, model):
    """run(..., defer_status=True): no host wait at the end of the call; the chain-status word is looked at by the next call or by
    check_status().  Same results as the synchronous route."""
    from egohmr_amd.diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="ddim5")
    B = 4
    b = _batch(dev, B)
    noise = torch.from_numpy(syn.make_noise_stack(5, B, seed=41)).to(dev)
    fs = model.fused_sampler
    ref = fs.run(d, b, noise, ddim=True)
    outs = [fs.run(d, b, noise, ddim=True, defer_status=True) for _ in range(3)]
    assert fs._status_event is not None
    fs.check_status()
    assert fs._status_event is None and int(fs._status_host[0]) == 0
    for o in outs:
        assert torch.equal(o["other_outputs"]["pred_vertices"], ref["other_outputs"]["pred_vertices"])
    fs.check_status()                                                        # idempotent


def test_error_behaviour(dev, model):
    from egohmr_amd import _lib
    from egohmr_amd.diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion(num_diffusion_timesteps=10, timestep_respacing="")
    with pytest.raises(SystemExit):                               # gaussian_diffusion.py:774-775 prints and exits
        d.val_losses(model, _batch(dev), shape=[3, 144], timestep_respacing="bogus", compute_loss=False)
    with pytest.raises(ValueError):
        create_gaussian_diffusion(num_diffusion_timesteps=10, timestep_respacing="ddim7")
    with pytest.raises(_lib.EgoHMRHipError):                      # CPU tensors never fall back to eager
        model.scene_enc(torch.zeros(1, 128, 3))
    out = d.ddim_sample_loop(model, _batch(dev), [3, 144], cond_fn_with_grad=True)     # ddim_sample_with_grad exists (golden G12)
    assert torch.isfinite(out["sample"]).all()
    with pytest.raises(NotImplementedError):
        d.training_losses(model, _batch(dev), torch.zeros(3, dtype=torch.long))           # training is out of scope
    empty = {k: ({kk: vv[:0] for kk, vv in v.items()} if isinstance(v, dict) else v[:0]) for k, v in _batch(dev).items()}
    with pytest.raises(ValueError, match="empty batch"):          # the reference fails too (egohmr.py:233: reshape of [0, 144] to [0, 24, -1])
        d.p_sample_loop(model, empty, [0, 144])
    with pytest.raises(IndexError):                                # gaussian_diffusion.py:160 indexes posterior_variance[1]: one-step chains fail there too
        create_gaussian_diffusion(num_diffusion_timesteps=1, timestep_respacing="")


def test_rotation_matrix_to_angle_axis_vs_reference_golden(golden_dir, dev):
    from egohmr_amd.geometry import rotation_matrix_to_angle_axis
    g = np.load(os.path.join(golden_dir, "g3_rotmat_to_aa.npz"))
    out = rotation_matrix_to_angle_axis(torch.from_numpy(g["R"]).to(dev))
    np.testing.assert_allclose(out.cpu().numpy(), g["aa"], atol=2e-5)


def test_rotation_matrix_to_angle_axis_kernel_all_branches_and_vjp(dev):
    """ehm_rotmat_to_angle_axis / _bwd against the CPU restatement of utils/konia_transform.py:316-340 and ITS autograd: random rotations (every quaternion
    branch: trace > 0 and the three leading-component cases near 180 degrees), the identity (k = 2 branch region), non-orthonormal input (the function is
    defined on any 3 x 3), batch shapes."""
    from egohmr_amd.geometry import rotation_matrix_to_angle_axis
    from oracle import geometry as og
    g = torch.Generator().manual_seed(4)
    aa = torch.randn(4000, 3, generator=g)
    aa = aa / aa.norm(dim=1, keepdim=True) * torch.cat([torch.rand(2000, generator=g) * 3.1, 3.1 + torch.rand(2000, generator=g) * 0.04]).unsqueeze(1)   # half near pi
    K = torch.zeros(4000, 3, 3)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -aa[:, 2], aa[:, 1], aa[:, 2], -aa[:, 0], -aa[:, 1], aa[:, 0]
    R = torch.linalg.matrix_exp(K.double()).float()
    R = torch.cat([R, torch.eye(3).unsqueeze(0), R[:50] + 0.05 * torch.randn(50, 3, 3, generator=g)], 0)
    m = R.reshape(-1, 9)
    tr = m[:, 0] + m[:, 4] + m[:, 8]
    br = torch.where(tr > 0, 0, torch.where((m[:, 0] > m[:, 4]) & (m[:, 0] > m[:, 8]), 1, torch.where(m[:, 4] > m[:, 8], 2, 3)))
    assert all(int((br == k).sum()) > 20 for k in range(4)), [int((br == k).sum()) for k in range(4)]      # every branch is exercised
    Rc = R.clone().requires_grad_(True)
    want = og.rotation_matrix_to_angle_axis(Rc)
    w = torch.randn(want.shape, generator=g)
    (want * w).sum().backward()
    Rd = R.to(dev).requires_grad_(True)
    got = rotation_matrix_to_angle_axis(Rd)
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().numpy(), atol=2e-5, rtol=1e-5)
    (got * w.to(dev)).sum().backward()
    gw, gg = Rc.grad.numpy(), Rd.grad.cpu().numpy()
    scale = np.abs(gw).max(axis=(1, 2), keepdims=True) + 1e-6
    assert np.abs(gg - gw).max() / 1.0 < 5e-3 * np.abs(gw).max(), (np.abs(gg - gw).max(), np.abs(gw).max())
    assert (np.abs(gg - gw) / scale).max() < 2e-3                                            # per matrix, relative to its own largest entry
    assert rotation_matrix_to_angle_axis(R[:24].reshape(2, 12, 3, 3).to(dev)).shape == (2, 12, 3)
    with pytest.raises(ValueError):
        rotation_matrix_to_angle_axis(torch.zeros(4, 3, 2, device=dev))


def test_smpl_pkl_loads_without_chumpy(tmp_path, dev, smpl_asset):
    """official SMPL_*.pkl files are chumpy-pickled; the loader must read them with chumpy absent."""
    from egohmr_amd import smpl as smpl_mod
    import scipy.sparse as sp
    fake = types.ModuleType("chumpy")
    fake_ch = types.ModuleType("chumpy.ch")

    class Ch:                                   # minimal stand-in that pickles like chumpy.ch.Ch (state dict with the array in 'x')
        def __init__(self, x):
            self.x = np.asarray(x)

        def __getstate__(self):
            return {"x": self.x, "_dirty_vars": set()}

    Ch.__module__, Ch.__qualname__ = "chumpy.ch", "Ch"
    fake_ch.Ch = Ch
    fake.ch = fake_ch
    sys.modules["chumpy"], sys.modules["chumpy.ch"] = fake, fake_ch
    V = 6890
    a = smpl_asset
    kin = np.stack([np.concatenate([[2 ** 32 - 1], a["parents"][1:]]), np.arange(24)]).astype(np.uint32)
    posedirs_pkl = a["posedirs"].T.reshape(V, 3, 207)                      # pkl layout [V,3,207]
    d = {"v_template": a["v_template"].astype(np.float64), "shapedirs": Ch(np.concatenate([a["shapedirs"], np.zeros((V, 3, 290))], -1)),
         "posedirs": posedirs_pkl.astype(np.float64), "J_regressor": sp.csc_matrix(a["J_regressor"].astype(np.float64)),
         "weights": a["lbs_weights"].astype(np.float64), "kintree_table": kin, "f": a["faces"].astype(np.uint32)}
    os.makedirs(tmp_path / "smpl")
    with open(tmp_path / "smpl" / "SMPL_NEUTRAL.pkl", "wb") as f:
        pickle.dump(d, f, protocol=2)
    del sys.modules["chumpy"], sys.modules["chumpy.ch"]
    m = smpl_mod.create(str(tmp_path / "smpl"), model_type="smpl", gender="neutral").to(dev)
    ref = smpl_mod.create(asset=smpl_asset).to(dev)
    for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"):
        np.testing.assert_allclose(getattr(m, k).cpu().numpy(), getattr(ref, k).cpu().numpy(), atol=1e-7, err_msg=k)
    assert m.parents.tolist() == ref.parents.tolist() and m.faces.shape == (13776, 3)
    betas = torch.zeros(1, 10, device=dev)
    I = torch.eye(3, device=dev).expand(1, 24, 3, 3).contiguous()
    np.testing.assert_allclose(m(betas=betas, body_pose=I[:, 1:], global_orient=I[:, :1], pose2rot=False).vertices.cpu().numpy(),
                               ref(betas=betas, body_pose=I[:, 1:], global_orient=I[:, :1], pose2rot=False).vertices.cpu().numpy(), atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f16x3", "f16"])
@pytest.mark.parametrize("B,passes", [(8, 2), (256, 2), (21, 1), (300, 2)])
def test_hidden_stack_chained_equals_layer_by_layer(B, passes, prec):
    """ehm_gcn_hidden_stack (one chained launch, per-row-tile counters, next tile's operands fetched under the epilogue) == the
    same convs launched one by one: same tile code, so bit-identical; and no producer wait may time out (B=300 exceeds the
    scratch reserved at create: the handle grows it)."""
    import ctypes as C
    from egohmr_amd import _lib
    from egohmr_amd.factory import build_synthetic_model
    from egohmr_amd.model import PRECISIONS
    dev = torch.device("cuda:0")
    model = build_synthetic_model(dev, 0)
    model.gcn_precision = prec
    L = _lib.lib()
    h = model.fused_sampler.gcn()
    assert L.ehm_gcn_get_precision(h) == PRECISIONS[prec]
    hid, tile = model.diffusion_model.hid_dim, L.ehm_gcn_row_tile()
    rows = passes * B * 24
    rows_pad = (rows + tile - 1) // tile * tile
    g = torch.Generator(device=dev).manual_seed(3)
    x0 = torch.relu(torch.randn(rows_pad, hid, device=dev, generator=g)) * 0.5
    x0[rows:] = 0
    X0 = torch.empty_like(x0)
    _lib.check(L.ehm_gcn_pack_activations(x0.data_ptr(), X0.data_ptr(), rows_pad, hid, L.ehm_gcn_activation_group(h), None))
    # reference: one launch per conv
    ref = [X0.clone(), torch.zeros_like(X0), torch.zeros_like(X0)]
    cur = 0
    for blk in range(model.diffusion_model.num_layers):
        y2 = 2 if cur == 0 else 0
        _lib.check(L.ehm_gcn_hidden_layer(h, 2 * blk, ref[cur].data_ptr(), None, ref[1].data_ptr(), rows_pad, None))
        _lib.check(L.ehm_gcn_hidden_layer(h, 2 * blk + 1, ref[1].data_ptr(), ref[cur].data_ptr(), ref[y2].data_ptr(), rows_pad, None))
        cur = y2
    torch.cuda.synchronize()
    for rep in range(3):      # repeated launches reuse (and re-zero) the counters
        bufs_t = [X0.clone(), torch.full_like(X0, float("nan")), torch.full_like(X0, float("nan"))]
        bufs = (C.c_void_p * 3)(*[t.data_ptr() for t in bufs_t])
        res = C.c_int(-1)
        _lib.check(L.ehm_gcn_hidden_stack(h, bufs, rows_pad, C.byref(res), None))
        _lib.check(L.ehm_gcn_stack_status(h, None))
        assert res.value == cur
        assert torch.equal(bufs_t[res.value].view(torch.int32), ref[cur].view(torch.int32)), f"rep {rep}"   # (bit patterns: f16 rows in mode 2)


@pytest.mark.gpu
@pytest.mark.parametrize("nonlocal_layer", [False, True])
def test_modulated_gcn_forward_standalone_vs_oracle(nonlocal_layer):
    """ModulatedGCN.forward called on its own with a full [B, 24, 3718] feature (modulated_gcn.py:99-116; VERDICT r05 missing item 5): the general input conv
    (split-f16 GEMM + ehm_gcn_input_layer_rows), the chained residual blocks, the optional non-local block and the output conv against the float64
    oracle, in the f32-grade modes; B not a multiple of the row tile; plain f16 runs and stays within its loose bound; bad shapes / CPU tensors raise."""
    from egohmr_amd import _lib, synthetic as syn
    from egohmr_amd.factory import build_synthetic_model
    from oracle import model as om
    dev = torch.device("cuda:0")
    sd = syn.make_state_dict(0, nonlocal_layer=nonlocal_layer)
    model = build_synthetic_model(dev, 0, gcn_nonlocal_layer=nonlocal_layer)
    dm = model.diffusion_model
    g = torch.Generator().manual_seed(2)
    B = 11
    x = torch.randn(B, 24, dm.in_dim, generator=g) * 0.5
    sd64 = {k: torch.as_tensor(v).double() for k, v in sd.items() if k.startswith("diffusion_model.")}
    want = om.modulated_gcn(sd64, x.double(), om.smpl_adjacency(torch.float64), nonlocal_layer=nonlocal_layer)
    scale = float(want.abs().max())
    for prec, tol in (("f16x3", 5e-5), ("f32", 5e-5)):
        dm.precision = prec
        got = dm(x.to(dev))
        assert got.shape == (B, 24, 6)
        err = float((got.cpu().double() - want).abs().max())
        print(f"ModulatedGCN.forward[{prec}, non_local={nonlocal_layer}] max|err| vs fp64 = {err:.2e} (|y|max {scale:.2f})")
        assert err < tol * max(1.0, scale), (prec, err)
    if not nonlocal_layer:
        dm.precision = "f16"
        assert float((dm(x.to(dev)).cpu().double() - want).abs().max()) < 3e-2 * max(1.0, scale)
        # the sampler's handle is another one: the module call leaves EgoHMR.forward untouched (bit-equal before / after)
    dm.precision = "f16x3"
    assert torch.equal(dm(x.to(dev)), dm(x.to(dev)))                                       # deterministic
    with pytest.raises(ValueError):
        dm(torch.zeros(2, 24, 17, device=dev))
    with pytest.raises(_lib.EgoHMRHipError):
        dm(x)


def test_non_local_gcn_block_vs_oracle():
    """gcn_nonlocal_layer=True (ModulatedGCN + NONLocalBlock2D, modulated_gcn.py:93-110; the oracle's block is pinned by the
    reference golden G13): EgoHMR.forward and a short DDIM loop against the oracle - on the step-wise route AND on the one-call loop
    (ehm_gcn_set_nonlocal: the block runs inside ehm_sample_loop), which agree; plain f16 features are refused."""
    from egohmr_amd import _lib, synthetic as syn
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device, build_synthetic_model
    from oracle import model as om, sampler as osampler, schedule as osched
    dev = torch.device("cuda:0")
    B, N = 3, 512
    sd, asset = syn.make_state_dict(0, nonlocal_layer=True), syn.make_smpl_asset(0)
    assert any(k.startswith("diffusion_model.non_local.W.1.") for k in sd)
    mean, std = syn.make_body_rep_stats(0)
    model = build_synthetic_model(dev, 0, gcn_nonlocal_layer=True)
    ref = om.EgoHMROracle(sd, asset, mean, std, faithful=False, gcn_nonlocal_layer=True)
    ref0 = om.EgoHMROracle(sd, asset, mean, std, faithful=False, gcn_nonlocal_layer=False)
    bnp = syn.make_batch(B, num_scene_points=N, seed=5)
    x_t = np.random.Generator(np.random.PCG64(5)).normal(size=(B, 144)).astype(np.float32)
    t = torch.full((B,), 17, dtype=torch.long)
    tb = {k: ({kk: torch.from_numpy(vv) for kk, vv in v.items()} if isinstance(v, dict) else torch.from_numpy(v)) for k, v in bnp.items()}
    tb["x_t"] = torch.from_numpy(x_t)
    ref.validation_setup(); ref0.validation_setup()
    o_ref = ref(tb, t)
    o_ref0 = ref0(dict(tb), t)
    assert float((o_ref["pred_x_start"] - o_ref0["pred_x_start"]).abs().max()) > 1e-3          # the block matters with these weights
    b = batch_to_device(bnp, dev)
    b["x_t"] = torch.from_numpy(x_t).to(dev)
    o = model(b, t.to(dev))
    # the attention logits are O(50) with these weights, so float32 rounding of a 512-term dot product is amplified by the softmax:
    # judge both float32 implementations against the float64 oracle
    ref64 = om.EgoHMROracle(sd, asset, mean, std, faithful=False, gcn_nonlocal_layer=True, dtype=torch.float64)
    ref64.validation_setup()
    tb64 = {k: ({kk: vv.double() for kk, vv in v.items()} if isinstance(v, dict) else (v.double() if v.dtype == torch.float32 else v)) for k, v in tb.items()}
    o64 = ref64(tb64, t)
    e_hip = float((o["pred_x_start"].cpu().double() - o64["pred_x_start"]).abs().max())
    e_f32 = float((o_ref["pred_x_start"].double() - o64["pred_x_start"]).abs().max())
    print(f"non-local forward: max|x0 - fp64| hip {e_hip:.2e}, float32 oracle {e_f32:.2e}")
    assert e_hip <= max(3.0 * e_f32, 5e-5)
    np.testing.assert_allclose(o["pred_vertices"].cpu().numpy(), o64["pred_vertices"].float().numpy(), atol=1e-4)
    # sampling: the one-call loop (default route of the API) and the step-wise route, both against the oracle
    d = create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="ddim5")
    noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B, seed=9))
    out = d.val_losses(model, batch_to_device(bnp, dev), shape=[B, 144], clip_denoised=False, timestep_respacing="ddim5", compute_loss=False,
                       noise_stack=noise.to(dev))
    assert model.fused_sampler.last_lowprec == 0                       # float32 features for the block: no plain-f16 step
    tab = osched.make_tables(50, "ddim5")
    tb2 = {k: ({kk: torch.from_numpy(vv) for kk, vv in v.items()} if isinstance(v, dict) else torch.from_numpy(v)) for k, v in bnp.items()}
    o2 = osampler.val_losses(ref, tb2, tab, noise, "ddim5")
    np.testing.assert_allclose(out["pred_vertices"].cpu().numpy(), o2["pred_vertices"].numpy(), atol=1e-4)
    d.allow_fused = False
    out_sw = d.val_losses(model, batch_to_device(bnp, dev), shape=[B, 144], clip_denoised=False, timestep_respacing="ddim5", compute_loss=False,
                          noise_stack=noise.to(dev))
    np.testing.assert_allclose(out_sw["pred_vertices"].cpu().numpy(), out["pred_vertices"].cpu().numpy(), atol=2e-5)
    d.allow_fused = True
    for prec in ("f32",):                                              # the f32-MFMA mode carries the block too
        model.gcn_precision = prec
        o3 = model.fused_sampler.run(d, batch_to_device(bnp, dev), noise.to(dev), ddim=True)["other_outputs"]
        np.testing.assert_allclose(o3["pred_vertices"].cpu().numpy(), o2["pred_vertices"].numpy(), atol=1e-4)
    model.gcn_precision = "f16"
    with pytest.raises(_lib.EgoHMRHipError):
        model.fused_sampler.run(d, batch_to_device(bnp, dev), noise.to(dev), ddim=True)
    model.gcn_precision = "f16x3"


@pytest.mark.gpu
def test_full_size_properties_c2():
    """BASELINE config 2 at full size (B=256, N=4096, DDIM-10 of 100), where the oracle is too slow to run: size-independent
    properties instead - (i) determinism: the same inputs and noise give bit-identical results twice; (ii) batch independence: items
    are independent, so the first 32 items of the B=256 run equal a B=32 run on exactly those inputs and noise rows (same kernels:
    MFMA skinning needs B >= 24); (iii) every output is finite and the rotations are orthonormal."""
    from egohmr_amd import synthetic as syn
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device, build_synthetic_model
    dev = torch.device("cuda:0")
    model = build_synthetic_model(dev, 0)
    d = create_gaussian_diffusion(num_diffusion_timesteps=100, timestep_respacing="ddim10")
    B, N, S = 256, 4096, 32
    bnp = syn.make_batch(B, num_scene_points=N, seed=77)
    noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B, seed=77))

    def sub(x):
        return {k: sub(v) for k, v in x.items()} if isinstance(x, dict) else x[:S]

    def run(b, nz):
        model.fused_sampler.invalidate()
        return d.val_losses(model, batch_to_device(b, dev), shape=[nz.shape[1], 144], clip_denoised=False, timestep_respacing="ddim10",
                            compute_loss=False, noise_stack=nz.to(dev))

    o1 = run(bnp, noise)
    o2 = run(bnp, noise)
    for k in ("pred_x_start", "pred_vertices", "pred_keypoints_3d"):
        assert torch.equal(o1[k], o2[k]), k                                             # (i)
    os_ = run(sub(bnp), noise[:, :S].contiguous())
    np.testing.assert_allclose(os_["pred_x_start"].cpu().numpy(), o1["pred_x_start"][:S].cpu().numpy(), atol=2e-5)   # (ii)
    np.testing.assert_allclose(os_["pred_vertices"].cpu().numpy(), o1["pred_vertices"][:S].cpu().numpy(), atol=2e-5)
    assert all(torch.isfinite(o1[k]).all() for k in ("pred_x_start", "pred_vertices", "pred_keypoints_3d"))            # (iii)
    R = torch.cat([o1["pred_smpl_params"]["global_orient"], o1["pred_smpl_params"]["body_pose"]], 1).reshape(-1, 3, 3)
    eye = torch.eye(3, device=R.device).expand_as(R)
    ortho, det = float((R @ R.transpose(1, 2) - eye).abs().max()), float((torch.linalg.det(R) - 1).abs().max())
    print(f"C2 full size: max|RR^T - I| = {ortho:.2e}, max|det - 1| = {det:.2e}")
    assert ortho < 1e-4 and det < 1e-4      # float32 Gram-Schmidt of nearly parallel 6-D pairs (geometry.py:61-66) is not tighter than this


@pytest.mark.gpu
def test_hip_graph_replay_equals_eager_enqueue():
    """EgoHMR.use_hip_graph: the whole sampling loop captured once into a hipGraph (persistent buffers, inputs copied in, results copied
    out) and replayed must reproduce the eager enqueue bit for bit, call after call, and for a second input batch of the same shape."""
    from egohmr_amd import synthetic as syn
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device, build_synthetic_model
    dev = torch.device("cuda:0")
    model = build_synthetic_model(dev, 0)
    d = create_gaussian_diffusion(num_diffusion_timesteps=100, timestep_respacing="ddim10")
    outs = {}
    for seed in (3, 4):
        b = batch_to_device(syn.make_batch(6, 1024, seed=seed), dev)
        noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, 6, seed=seed)).to(dev)
        for mode in (False, True, True):
            model.use_hip_graph = mode
            o = model.fused_sampler.run(d, b, noise, ddim=True)["other_outputs"]
            outs.setdefault(seed, []).append((o["pred_vertices"].clone(), o["pred_x_start"].clone()))
    assert len(model.fused_sampler._graphs) == 1                       # one capture served both batches
    for seed, runs in outs.items():
        for v, x in runs[1:]:
            assert torch.equal(v, runs[0][0]) and torch.equal(x, runs[0][1]), seed
    assert not torch.equal(outs[3][0][0], outs[4][0][0])
    # an in-place SMPL edit recreates the SMPL handle (its host address may be the destroyed one's): the graph route must capture again
    model.smpl.v_template.add_(1e-3)
    verts = {}
    for mode in (True, False):
        model.use_hip_graph = mode
        verts[mode] = model.fused_sampler.run(d, b, noise, ddim=True)["other_outputs"]["pred_vertices"].clone()
        if mode:
            assert len(model.fused_sampler._graphs) == 2
    assert torch.equal(verts[True], verts[False]) and not torch.equal(verts[False], outs[4][0][0])


@pytest.mark.gpu
def test_pass_pruning_is_exact():
    """Items whose 24 SMPL joints are all visible take every output entry from the conditional pass (egohmr.py:249-254), so their
    image-masked pass is skipped (ehm_gcn_set_pass_map): the sampled bodies must equal the unpruned run bit for bit - for a mixed
    batch, an all-visible batch (no second pass at all) and a batch without any prunable item - through the fused loop and forward()."""
    from egohmr_amd import synthetic as syn
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device, build_synthetic_model
    dev = torch.device("cuda:0")
    model = build_synthetic_model(dev, 0)
    d = create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="ddim5")
    B = 11
    noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B, seed=9)).to(dev)
    for case, visible in (("mixed", [0, 3, 4, 10]), ("all", list(range(B))), ("none", [])):
        bnp = syn.make_batch(B, 1024, seed=9)
        bnp["orig_keypoints_2d"][:, 9, 2] = 0.0                     # make sure nobody is all-visible by accident ...
        bnp["orig_keypoints_2d"][visible, :, 2] = 1.0               # ... except the chosen items
        b = batch_to_device(bnp, dev)
        outs = {}
        for prune in (False, True):
            model.prune_passes = prune
            model.fused_sampler.invalidate()
            o = model.fused_sampler.run(d, b, noise, ddim=True)["other_outputs"]
            b["x_t"] = noise[0]
            f = model(b, torch.full((B,), 7, device=dev))
            outs[prune] = (o["pred_x_start"].clone(), o["pred_vertices"].clone(), f["pred_x_start"].clone())
            st = model.fused_sampler.prepare(b)
            assert st.num_masked == B - len(visible), case
        for a, c in zip(outs[False], outs[True]):
            assert torch.equal(a, c), case
    model.prune_passes = True
