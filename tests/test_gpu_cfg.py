"""GPU (MI355X): classifier-free guidance scales on the visibility fuse, x0 = u + s (c - u) per joint with s = s_vis on visible and s_inv on
invisible joints (EgoHMR.guidance_param_visible / guidance_param, diffusion.ClassifierFreeSampleModel; csrc/step_dev.h, csrc/gcn.hip).

Against float64 (tests/cfg_ref.py: CFGOracle) and what the reference's own forward pins of c and u (tests/golden/g22_cfg_passes.npz); the exact
identities of the rule; bit-equality of the sampler's routes under scales; the pass counts; whole loops against the float64 sampler.
Shapes: B = 3 for a forward, B = 4 / 5 for loops - the fuse is per body and does not depend on the block width of the step kernel."""
import os

import numpy as np
import pytest
import torch

import cfg_ref as R
from egohmr_amd import synthetic as syn

pytestmark = pytest.mark.gpu

VJ_TOL = 1e-4          # tests/test_gpu_parity.py: vertices / joints of one forward
X0_TOL = 5e-5          # ... and its pred_x_start (_check_out)
N_ORIG = 50
# Loops vs float64: the device may be 8 times as far from the float64 CFGOracle loop as the float32 CFGOracle loop is on the CPU (the loop
# amplifies rounding by the model's own gain, which s multiplies).  Measured float32 distances to the float64 loop (max over pred_x_start, the
# joints and the first 64 vertices; B = 4, scales (2.5, 0.5), the sensitive weights of 50 steps, the inputs of _loop_inputs; the reference side
# stays finite, max |x0| 4.9 / 6.6):
F32_LOOP_DIST = {"ddim5": 9.489e-6, "": 1.568e-5}      # DDIM-5 of 50, DDPM-50
LOOP_MARGIN = 8.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, smpl_asset):
    """The plain synthetic network (weights seeded as G10) with the fuse."""
    from egohmr_amd.factory import build_synthetic_model
    m = build_synthetic_model(dev, 0, smpl_asset=smpl_asset, diffuse_fuse=True)
    m.f16x3_last_steps = None
    return m


@pytest.fixture(scope="module")
def model_sens(dev, smpl_asset):
    """The x_t-sensitive, trained-like denoiser (loops)."""
    from egohmr_amd.factory import build_synthetic_model
    m = build_synthetic_model(dev, 0, smpl_asset=smpl_asset, diffuse_fuse=True, sensitive=dict(num_diffusion_timesteps=N_ORIG))
    m.f16x3_last_steps = None
    return m


@pytest.fixture(autouse=True)
def _defaults(model, model_sens):
    yield
    for m in (model, model_sens):
        m.guidance_param, m.guidance_param_visible, m.outer_guidance, m.force_cfg_kernels = 0.0, 1.0, 1.0, False
        m.only_mask_img_cond, m.diffuse_fuse, m.gcn_precision, m.per_step_launches, m.prune_passes = True, True, "f16x3", False, True
        m.use_hip_graph, m.loop_bodies, m.lbs_every_step = False, 256, True


def _scales(m, pair):
    m.guidance_param_visible, m.guidance_param = pair


@pytest.fixture(scope="module")
def batch3(dev):
    from egohmr_amd.factory import batch_to_device
    b_np, x_t = R.make_batch3()
    tb = batch_to_device(b_np, dev)
    tb["x_t"] = torch.from_numpy(x_t).to(dev)
    return b_np, x_t, tb


@pytest.fixture(scope="module")
def oracle64():
    """One float64 CFGOracle (its encoders run once per batch object); results cached per (only_mask_img_cond, scales)."""
    o = R.make_oracle(torch.float64)
    b_np, x_t = R.make_batch3()
    tb = R.to_torch(b_np)
    tb["x_t"] = torch.from_numpy(x_t)
    cache = {}

    def get(omi, pair):
        if (omi, pair) not in cache:
            o.only_mask_img_cond, o.s_vis, o.s_inv = omi, float(pair[0]), float(pair[1])
            with torch.no_grad():
                r = o(tb, torch.full((R.B3,), R.TIMESTEP, dtype=torch.long))
            cache[(omi, pair)] = {k: r[k].clone() for k in ("pred_x_start", "pred_vertices", "pred_keypoints_3d")}
            cache["vis"] = tb["vis_mask_smpl"].clone()
        return cache[(omi, pair)], cache["vis"]
    return get


def _forward(m, tb, **kw):
    out = m(dict(tb), torch.full((R.B3,), R.TIMESTEP, device=m.device, dtype=torch.long), **kw)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------- 1. forward vs float64 and vs the golden
@pytest.mark.parametrize("omi", [True, False])
@pytest.mark.parametrize("prec", ["f16x3", "f32"])
def test_forward_under_scales_vs_float64_and_the_reference_golden(model, batch3, oracle64, golden_dir, omi, prec):
    g = np.load(os.path.join(golden_dir, "g22_cfg_passes.npz"))
    gv, cov = g["vis"], g["covered"]
    gc, gu = g["c"].astype(np.float64), g["u_free"].astype(np.float64)
    model.only_mask_img_cond, model.gcn_precision = omi, prec
    for pair in R.SCALE_PAIRS:
        _scales(model, pair)
        out = _forward(model, batch3[2])
        ref, vis = oracle64(omi, pair)
        assert np.array_equal(out_vis := batch_vis(model, batch3[2]), vis.numpy()) and np.array_equal(out_vis, gv)
        x0 = out["pred_x_start"].double().cpu().reshape(R.B3, 24, 6)
        d = (x0 - ref["pred_x_start"].reshape(R.B3, 24, 6)).abs().amax(dim=2)              # [B,24]
        for name, sel, s in (("visible", vis, pair[0]), ("invisible", ~vis, pair[1])):
            worst = float(d[sel].max()) if bool(sel.any()) else 0.0
            print(f"omi {omi} {prec} scales {pair} {name}: max |x0 - f64| = {worst:.3e}, bar {R.bar(s, X0_TOL):.3e}")
            assert worst <= R.bar(s, X0_TOL), (pair, name, worst)
        factor = max(R.bar(pair[0], 1.0), R.bar(pair[1], 1.0))
        for k in ("pred_vertices", "pred_keypoints_3d"):
            worst = float((out[k].double().cpu() - ref[k]).abs().max())
            print(f"   {k}: {worst:.3e}, bar {factor * VJ_TOL:.3e}")
            assert worst <= factor * VJ_TOL, (pair, k, worst)
        if omi:                                   # the reference's own c and u (its test-time flags mask the image only)
            x0n = x0.numpy()
            for name, sel, s in (("visible", gv & cov, pair[0]), ("invisible", ~gv & cov, pair[1])):
                worst = float(np.abs(x0n - (gu + s * (gc - gu)))[sel].max()) if sel.any() else 0.0
                print(f"   golden {name}: {int(sel.sum())} joints, {worst:.3e}, bar {R.bar(s, X0_TOL):.3e}")
                assert worst <= R.bar(s, X0_TOL), (pair, name, worst)


def batch_vis(m, tb):
    return m.fused_sampler.prepare(tb).vis_bool.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 2. exact identities
KEYS = ("pred_x_start", "pred_vertices", "pred_keypoints_3d", "pred_pose_6d", "pred_keypoints_2d_full")


def _same(a, b, keys=KEYS):
    for k in keys:
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


def _differ(a, b):
    assert float((a["pred_x_start"] - b["pred_x_start"]).abs().max()) > 1e-4


def _loop_inputs(dev, B, respacing, seed=21, n=N_ORIG):
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device
    d = create_gaussian_diffusion(num_diffusion_timesteps=n, timestep_respacing=respacing)
    b = syn.make_batch(B, 512, seed=seed)
    b["orig_keypoints_2d"][:2, :, 2] = 1.0                                   # two all-visible items (pass pruning)
    noise = syn.make_noise_stack(d.num_timesteps, B, seed=seed)
    return d, b, batch_to_device(b, dev), torch.from_numpy(noise).to(dev), noise


def _loop(m, d, batch, noise, respacing, which="val_losses", wrap=None, **kw):
    fs = m.fused_sampler
    fs.invalidate()
    target = wrap if wrap is not None else m
    B = noise.shape[1]
    if which == "val_losses":
        o = d.val_losses(target, dict(batch), shape=[B, 144], clip_denoised=False, timestep_respacing=respacing, compute_loss=False, noise_stack=noise, **kw)
    elif which == "p_sample_loop":
        o = d.p_sample_loop(target, dict(batch), [B, 144], noise_stack=noise, **kw)["other_outputs"]
    else:
        o = d.ddim_sample_loop(target, dict(batch), [B, 144], noise_stack=noise, **kw)["other_outputs"]
    torch.cuda.synchronize()
    return {k: o[k].clone() for k in KEYS}


def test_identities_of_one_forward(model, batch3):
    tb = batch3[2]
    default = _forward(model, tb)
    model.force_cfg_kernels = True                       # (1, 0) through the guidance kernel = the select
    _same(_forward(model, tb), default)
    model.force_cfg_kernels = False
    cond = _forward(model, tb, eval_with_uncond=False)
    _differ(cond, default)
    _scales(model, (1.0, 1.0))                           # (1, 1) = the conditional output alone: one pass
    _same(_forward(model, tb), cond)
    _scales(model, (0.0, 0.0))                           # force_mask = scales (0, 0)
    zero = _forward(model, tb)
    _scales(model, (1.0, 0.0))
    masked = _forward(model, tb, force_mask=True)
    _same(masked, zero)
    _differ(masked, default)
    _scales(model, (2.5, 0.5))                           # ... whatever the model's own scales are
    _same(_forward(model, tb, force_mask=True), zero)
    with pytest.raises(ValueError):
        _scales(model, (float("nan"), 0.0))
        _forward(model, tb)


def test_identities_in_loops(model_sens, dev):
    m = model_sens
    d, _, batch, noise, _ = _loop_inputs(dev, 5, "ddim5")
    default = _loop(m, d, batch, noise, "ddim5")
    m.force_cfg_kernels = True
    _same(_loop(m, d, batch, noise, "ddim5"), default)
    m.force_cfg_kernels = False
    _scales(m, (1.0, 1.0))
    one = _loop(m, d, batch, noise, "ddim5")
    _scales(m, (1.0, 0.0))
    m.diffuse_fuse = False                               # (1, 1) in a loop = a model without the fuse
    _same(_loop(m, d, batch, noise, "ddim5"), one)
    _differ(one, default)


@pytest.mark.parametrize("which,respacing", [("forward", None), ("p_sample_loop", ""), ("ddim_sample_loop", "ddim5"), ("val_losses", "ddim5")])
def test_wrapper_equals_the_model_with_the_effective_scales(model_sens, dev, batch3, which, respacing):
    from egohmr_amd import ClassifierFreeSampleModel
    m = model_sens
    w = ClassifierFreeSampleModel(m, guidance_param=2.0)
    if which == "forward":
        run = lambda target: {k: v.clone() for k, v in _fwd(target, batch3[2]).items() if k in KEYS}
    else:
        n = 10 if respacing == "" else N_ORIG            # (ancestral: 10 steps)
        d, _, batch, noise, _ = _loop_inputs(dev, 4, respacing, n=n)
        run = lambda target: _loop(m, d, batch, noise, respacing, which=which, wrap=target)
    _scales(m, (1.25, 0.25))
    wrapped = run(w)
    assert m.outer_guidance == 1.0
    plain = run(m)
    _scales(m, (2.5, 0.5))                               # s_vis = w * guidance_param_visible, s_inv = w * guidance_param
    _same(wrapped, run(m))
    _differ(wrapped, plain)
    m.diffuse_fuse = False                               # without the fuse: w on all joints
    _scales(m, (1.0, 0.0))
    wrapped = run(w)
    m.diffuse_fuse = True
    _scales(m, (2.0, 2.0))
    _same(wrapped, run(m))


def _fwd(target, tb):
    out = target(dict(tb), torch.full((R.B3,), R.TIMESTEP, device=tb["x_t"].device, dtype=torch.long))
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------- 3. the routes agree bit for bit under scales
@pytest.mark.parametrize("respacing,B,lbs,pair", [
    ("ddim5", 5, True, (2.5, 0.5)), ("", 5, True, (2.5, 0.5)),      # below the deferred skinning's batch size both sides take step_body_cfg_kernel ...
    ("ddim5", 5, False, (2.5, 0.5)),                                 # ... unless the steps do not skin: step_fused_kernel<.., CFG> on all but the last step
    ("ddim5", 26, True, (2.5, 0.5)), ("", 26, True, (2.5, 0.5)),    # deferred skinning: the fused launch on every step (a ragged 32-body skinning tile)
    ("ddim5", 26, True, (1.0, 0.5)),                                 # ... with pruned items (slot < 0: their zero second-pass rows are never read)
    ("ddim5", 26, True, (0.0, 0.0)),                                 # ... and the masked output alone
])
def test_fused_step_equals_per_step_launches_under_scales(model_sens, dev, respacing, B, lbs, pair):
    m = model_sens
    d, _, batch, noise, _ = _loop_inputs(dev, B, respacing, n=N_ORIG if respacing else 10)
    _scales(m, pair)
    m.lbs_every_step = lbs
    fused = _loop(m, d, batch, noise, respacing)
    m.per_step_launches = True
    _same(_loop(m, d, batch, noise, respacing), fused)
    assert all(torch.isfinite(v).all() for v in fused.values())
    if pair == (1.0, 0.5):                                           # the fused launch with the select, forced through the guidance kernel
        _scales(m, (1.0, 0.0))
        m.per_step_launches = False
        sel = _loop(m, d, batch, noise, respacing)
        m.force_cfg_kernels = True
        _same(_loop(m, d, batch, noise, respacing), sel)
        _differ(sel, fused)


def test_fused_step_256_thread_form_under_scales(model_sens, dev):
    """launch_fused (csrc/step.hip) gives the guidance kernels 1024 threads per body up to one body per CU and 256 beyond: B = CUs + 1."""
    m = model_sens
    B = torch.cuda.get_device_properties(dev).multi_processor_count + 1
    d, _, batch, noise, _ = _loop_inputs(dev, B, "ddim5")
    _scales(m, (2.5, 0.5))
    fused = _loop(m, d, batch, noise, "ddim5")
    m.per_step_launches = True
    _same(_loop(m, d, batch, noise, "ddim5"), fused)


def test_pruned_passes_equal_unpruned_under_scales(model_sens, dev):
    m = model_sens
    d, _, batch, noise, _ = _loop_inputs(dev, 5, "ddim5")                # two all-visible items
    _scales(m, (1.0, 0.5))
    pruned = _loop(m, d, batch, noise, "ddim5")
    m.prune_passes = False
    _same(_loop(m, d, batch, noise, "ddim5"), pruned)
    m.per_step_launches = True
    _same(_loop(m, d, batch, noise, "ddim5"), pruned)
    m.prune_passes = True
    _same(_loop(m, d, batch, noise, "ddim5"), pruned)
    tb = dict(batch, x_t=noise[0])                                       # ... and one forward
    t = torch.full((5,), R.TIMESTEP, device=dev, dtype=torch.long)
    a = m(dict(tb), t)
    m.prune_passes = False
    _same(m(dict(tb), t), a)


def test_chunked_samples_equal_one_chunk_under_scales(model_sens, dev):
    m = model_sens
    d, _, batch, noise, _ = _loop_inputs(dev, 4, "ddim5")
    stacks = [noise, torch.from_numpy(syn.make_noise_stack(d.num_timesteps, 4, seed=22)).to(dev), torch.from_numpy(syn.make_noise_stack(d.num_timesteps, 4, seed=23)).to(dev)]
    _scales(m, (2.5, 0.5))
    res = {}
    for width in (0, 8, 4):                                              # all 12 bodies in one loop; two samples per loop; one
        m.loop_bodies = width
        m.fused_sampler.invalidate()
        outs = m.fused_sampler.run_samples(d, dict(batch), stacks, ddim=True)
        torch.cuda.synchronize()
        res[width] = [{k: o["other_outputs"][k].clone() for k in KEYS} for o in outs]
    for width in (8, 4):
        for a, b in zip(res[width], res[0]):
            _same(a, b)


def test_hip_graph_replay_under_scales_and_its_key(model_sens, dev):
    m = model_sens
    d, _, batch, noise, _ = _loop_inputs(dev, 4, "ddim5")
    _scales(m, (2.5, 0.5))
    eager = _loop(m, d, batch, noise, "ddim5")
    _scales(m, (2.5, 0.25))
    eager2 = _loop(m, d, batch, noise, "ddim5")
    m.use_hip_graph = True
    _scales(m, (2.5, 0.5))
    _same(_loop(m, d, batch, noise, "ddim5"), eager)
    _same(_loop(m, d, batch, noise, "ddim5"), eager)                    # the replay
    _scales(m, (2.5, 0.25))                                              # a changed scale is another graph, not a replay of the first
    g2 = _loop(m, d, batch, noise, "ddim5")
    _same(g2, eager2)
    _differ(g2, eager)


# ---------------------------------------------------------------------------------------------- 4. pass counts
def test_pass_counts(model_sens, dev):
    m = model_sens
    fs = m.fused_sampler
    d, b_np, batch, noise, _ = _loop_inputs(dev, 5, "ddim5")
    assert int((~m.visibility(batch).all(dim=1)).sum()) == 3             # items with an invisible joint

    def describe():
        st = fs.prepare(dict(batch))
        return fs._describe(st=st, T=5, ddim=True, any_guided=False, denom_items=5, lowprec=0, nonlocal_ci=0)[0]
    for pair, passes, masked, cfg in (((1.0, 0.0), 2, 3, 0), ((1.0, 0.5), 2, 3, 1), ((2.5, 0.0), 2, 5, 1), ((0.5, 0.5), 2, 5, 1), ((1.0, 1.0), 1, -1, 0)):
        _scales(m, pair)
        desc = describe()
        assert desc.passes == passes and fs.last_fuse[0] == cfg, pair
        if passes == 2:
            assert desc.num_masked == masked, (pair, desc.num_masked)
        assert fs.last_fuse[1:] == (pair if cfg else (1.0, 0.0))          # what the handle was given (ehm_gcn_set_fuse_scales)
    _scales(m, (1.0, 0.0))
    m.diffuse_fuse = False                                               # a model without the fuse under a wrapper's scale: two passes, every item
    m.outer_guidance = 2.5
    desc = describe()
    assert desc.passes == 2 and desc.num_masked == 5 and fs.last_fuse == (1, 2.5, 2.5)


# ---------------------------------------------------------------------------------------------- 5. loops vs float64
@pytest.mark.parametrize("respacing", ["ddim5", ""])
def test_loops_under_scales_vs_the_float64_sampler(model_sens, dev, smpl_asset, respacing):
    from oracle import sampler as osamp, schedule as osched
    m = model_sens
    B = 4
    d, b_np, batch, noise, noise_np = _loop_inputs(dev, B, respacing)
    _scales(m, (2.5, 0.5))
    out = _loop(m, d, batch, noise, respacing)
    mean, std = syn.make_body_rep_stats(0)
    o = R.CFGOracle(syn.make_sensitive_state_dict(0, num_diffusion_timesteps=N_ORIG), smpl_asset, mean, std, dtype=torch.float64, faithful=False,
                    s_vis=2.5, s_inv=0.5)
    ref = osamp.val_losses(o, R.to_torch(b_np), osched.make_tables(N_ORIG, respacing), torch.from_numpy(noise_np).double(), respacing)
    assert all(torch.isfinite(ref[k]).all() for k in ("pred_x_start", "pred_vertices"))
    dist = max(float((out[k].double().cpu() - ref[k]).abs().max()) for k in ("pred_x_start", "pred_keypoints_3d"))
    dist = max(dist, float((out["pred_vertices"][:, :64].double().cpu() - ref["pred_vertices"][:, :64]).abs().max()))
    bar = LOOP_MARGIN * F32_LOOP_DIST[respacing]
    print(f"{respacing or 'ddpm50'}: device vs float64 {dist:.3e}, bar {bar:.3e} (float32 oracle: {F32_LOOP_DIST[respacing]:.3e})")
    assert dist <= bar


# ---------------------------------------------------------------------------------------------- 6. collision-guided loop
@pytest.mark.parametrize("lbs", [True, False])
def test_guided_loop_under_scales_fused_equals_per_step(model_sens, dev, lbs):
    """Guided DDPM at B = 4 under scales (2.5, 0.5): the fused route equals the per-step route bit for bit, both finite.
    The collision gradient (unchanged here) is accumulated with float atomics, so on a scene with many contacts two runs of the SAME route differ
    in the last bits (tests/test_gpu_step_fused.py holds such loops to 2e-5).  Bit-equality is asked on a scene where the sums are order-free: every
    scene point lies far outside the bodies' boxes but two per item, placed 1 cm off two vertices of the item's unguided body - at most two non-zero
    addends meet in any accumulator (the item's loss, a vertex's gradient, a joint's transform gradient), and a + b = b + a.
    lbs = False: the steps do not skin, so that B = 4 takes the fused step launch on all but the last step (with per-step skinning both sides run
    step_body_cfg_kernel below the deferred skinning's batch size)."""
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device
    m = model_sens
    d = create_gaussian_diffusion(num_diffusion_timesteps=20, timestep_respacing="")
    B = 4
    b_np = syn.make_batch(B, 1024, seed=9)
    noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B, seed=9)).to(dev)
    _scales(m, (2.5, 0.5))
    m.lbs_every_step = lbs
    unguided = _loop(m, d, batch_to_device(b_np, dev), noise, "")
    verts = unguided["pred_vertices"].cpu().numpy()                          # body frame: the scene is compared with it after `- transl` (scene_cano)
    transl = b_np["smpl_params"]["transl"]
    scene = np.broadcast_to(transl[:, None, :] + 50.0, b_np["scene_pcd_verts_full"].shape).copy()
    scene[:, 0] = verts[:, 100] + transl + np.float32([0.01, 0.0, 0.0])
    scene[:, 1] = verts[:, 4000] + transl + np.float32([0.0, 0.01, 0.0])
    batch = batch_to_device(dict(b_np, scene_pcd_verts_full=scene.astype(np.float32)), dev)
    kw = dict(cond_fn_with_grad=True, cond_grad_weight=0.3)
    fused = _loop(m, d, batch, noise, "", **kw)
    m.per_step_launches = True
    per_step = _loop(m, d, batch, noise, "", **kw)
    assert all(torch.isfinite(v).all() for v in fused.values()) and all(torch.isfinite(v).all() for v in per_step.values())
    _same(fused, per_step)
    live = float((fused["pred_x_start"] - unguided["pred_x_start"]).abs().max())
    print(f"guided vs unguided pred_x_start: {live:.3e}")
    assert live > 1e-5                                                        # the guidance is live
