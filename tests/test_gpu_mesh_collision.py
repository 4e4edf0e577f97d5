"""GPU (MI355X): the mesh collision term (csrc/mesh_collision.hip; the rule: include/egohmr_hip.h) against its float64 restatement
(tests/mesh_collision_ref.py), and its way through the Python surface under EgoHMR.collision_proxy = 'mesh'.

Error bars: hits are EQUAL to the reference's; loss and gverts are held to 4 x the error of the float32 NumPy restatement against float64 on the same
inputs, per tensor, as a max-norm relative to the tensor's largest magnitude (the 4 covers the kernel's other summation order and its fused
multiply-adds).  The inputs are filtered, never the outputs: points within 1e-4 m of the surface, with |w - 0.5| < 1e-3 or on the medial axis are
dropped from a cloud before the kernel sees it (mesh_collision_ref.filter_cloud), and the dropped share is asserted to be at most 1 %."""
import functools

import numpy as np
import pytest
import torch

from egohmr_amd import synthetic as syn
from tests import mesh_collision_ref as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 4.0


def _query(verts, faces, scene, all_points, want_grad=True, want_hits=True):
    """ehm_mesh_collision_query on float32 copies -> (loss [B], gverts [B,V,3] or None, hits [B] or None) as NumPy."""
    from egohmr_amd import _lib
    v = torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(DEV)
    s = torch.from_numpy(np.ascontiguousarray(scene, np.float32)).to(DEV)
    f = torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(DEV)
    B, V, N = v.shape[0], v.shape[1], s.shape[1]
    loss = torch.full((B,), float("nan"), device=DEV)
    g = torch.full((B, V, 3), float("nan"), device=DEV) if want_grad else None
    h = torch.full((B,), -7, device=DEV, dtype=torch.int32) if want_hits else None
    _lib.api().ehm_mesh_collision_query(v, f, s, loss, g, h, B, V, len(faces), N, int(all_points), _lib.stream_ptr())
    torch.cuda.synchronize()
    return loss.cpu().numpy(), None if g is None else g.cpu().numpy(), None if h is None else h.cpu().numpy()


def _refs(verts, faces, scene, all_points):
    v, s = np.asarray(verts, np.float32), np.asarray(scene, np.float32)
    return M.mesh_collision_ref(v, faces, s, all_points), M.mesh_collision_ref(v, faces, s, all_points, dtype=np.float32)


def _check(name, got, r64, r32):
    loss, g, h = got
    np.testing.assert_array_equal(h, r64["hits"])
    np.testing.assert_array_equal(r32["hits"], r64["hits"])                       # (the filter's job: the yardstick itself is unambiguous)
    for key, x in (("loss", loss), ("gverts", g)):
        e32, ek = M.rel_err(r32[key], r64[key]), M.rel_err(x, r64[key])
        print(f"{name} {key}: float32 NumPy {e32:.3e}, kernel {ek:.3e}, bar {BAR * e32:.3e}")
        assert np.isfinite(x).all() and ek <= BAR * e32, (name, key, ek, e32)


@functools.lru_cache(maxsize=None)
def _case(stacks, slices, n, seed=3):
    """Three bodies (as is; scaled by 0.7 and shifted; 10 m away) around one filtered cloud of n points uniform in [-0.8, 0.8]^3, and the float64 and
    float32 restatements of every (body, point) pair, computed once for all the tests of the case."""
    v, f = M.peanut(stacks, slices)
    bodies = np.stack([v, 0.7 * v + [0.05, -0.03, 0.02], v + 10.0]).astype(np.float32)
    cand = np.random.Generator(np.random.PCG64(seed)).uniform(-0.8, 0.8, size=(n + n // 20, 3)).astype(np.float32)
    pts, dropped, per64 = M.filter_cloud(bodies[:2], f, cand, n)
    assert dropped <= 0.01, dropped
    scene = np.broadcast_to(pts.astype(np.float32), (3, n, 3)).copy()
    per64.append(M.body_points(bodies[2], f, scene[2]))
    return bodies, f, scene, (per64, M.per_body(bodies, f, scene, np.float32))


def _case_refs(case, all_points):
    bodies, f, scene, (per64, per32) = case
    return M.mesh_collision_ref(bodies, f, scene, all_points, per=per64), M.mesh_collision_ref(bodies, f, scene, all_points, np.float32, per=per32)


@pytest.mark.parametrize("all_points", [False, True])
@pytest.mark.parametrize("mesh", [(8, 12), (24, 32)])
def test_kernel_vs_float64(mesh, all_points):
    case = _case(*mesh, 3000)
    bodies, f, scene = case[:3]
    assert len(f) == {(8, 12): 168, (24, 32): 1472}[mesh]
    r64, r32 = _case_refs(case, all_points)
    assert r64["hits"][0] > 100 and r64["hits"][1] > 30 and r64["hits"][2] == 0
    got = _query(bodies, f, scene, all_points)
    _check(f"F={len(f)} all_points={all_points}", got, r64, r32)
    assert got[0][2] == 0 and not got[1][2].any() and got[2][2] == 0               # the far body: exact zeros
    if not all_points:
        assert not r64["selected"][2].any() and r64["selected"][0].sum() < 3000


@pytest.mark.parametrize("F", ["chunk-1", "chunk", "chunk+1"])
def test_face_counts_around_the_lds_chunk(F):
    """The first F faces of the 1472-face peanut (not closed: w is fractional, the rule is defined all the same)."""
    from egohmr_amd import _lib
    F = _lib.MESH_COLLISION_FACE_CHUNK + {"chunk-1": -1, "chunk": 0, "chunk+1": 1}[F]
    v, f = M.peanut(24, 32)
    v, f = v.astype(np.float32), f[:F]
    cand = np.random.Generator(np.random.PCG64(11)).uniform(-0.8, 0.8, size=(630, 3)).astype(np.float32)
    pts, dropped, _ = M.filter_cloud(v[None], f, cand, 600)
    assert dropped <= 0.01
    scene = pts.astype(np.float32)[None]
    r64, r32 = _refs(v[None], f, scene, True)
    assert r64["hits"][0] > 10
    _check(f"F={F}", _query(v[None], f, scene, True), r64, r32)


def test_single_triangle_single_point_and_null_outputs():
    v, f = M.peanut(8, 12)
    v = v.astype(np.float32)
    bodies, _, scene = _case(8, 12, 3000)[:3]
    # F = 1: a triangle encloses nothing
    loss, g, h = _query(bodies, f[:1], scene, True)
    assert (loss == 0).all() and not g.any() and (h == 0).all()
    # N = 1: one point inside a lobe (off the axis: the axis of a body of revolution is its medial axis; the filter confirms it)
    p = M.filter_cloud(v[None], f, np.array([[0.09, -0.06, 0.5]], np.float32), 1)[0].astype(np.float32)[None]
    r64, r32 = _refs(v[None], f, p, False)
    assert r64["hits"][0] == 1
    _check("N=1", _query(v[None], f, p, False), r64, r32)
    # gverts = NULL, hits = NULL: the loss is the same bits
    full = _query(bodies, f, scene, False)
    for wg, wh in ((False, True), (True, False), (False, False)):
        part = _query(bodies, f, scene, False, want_grad=wg, want_hits=wh)
        np.testing.assert_array_equal(part[0], full[0])
        assert (part[1] is None) == (not wg) and (part[2] is None) == (not wh)
        if wh:
            np.testing.assert_array_equal(part[2], full[2])
    np.testing.assert_array_equal(_query(bodies, f, scene, False)[0], full[0])     # loss and hits: a fixed order, the same bits again


@pytest.mark.parametrize("n", ["block", "block+1"])
def test_selected_counts_at_the_point_block(n):
    """all_points with N = one block of points and one more: the second block holds a single point."""
    from egohmr_amd import _lib
    n = _lib.MESH_COLLISION_POINT_BLOCK + (n == "block+1")
    bodies, f, scene = _case(8, 12, 3000)[:3]
    sc = scene[:1, :n].copy()
    # the last point (the lone one of the second block) is a hit: inside a lobe, off its axis, and it passes the filter
    sc[0, -1] = M.filter_cloud(bodies[:1], f, np.array([[0.11, 0.05, -0.5]], np.float32), 1)[0][0]
    r64, r32 = _refs(bodies[:1], f, sc, True)
    assert r64["w"][0, -1] > 0.99 and r64["d"][0, -1] > 0.05
    _check(f"N={n}", _query(bodies[:1], f, sc, True), r64, r32)
    # ... and none selected: the bounding-box route on a cloud that misses the box
    loss, g, h = _query(bodies[:1], f, sc + 5.0, False)
    assert loss[0] == 0 and not g.any() and h[0] == 0


def test_repeated_indices_give_finite_outputs():
    bodies, f, scene = _case(8, 12, 3000)[:3]
    soup = np.concatenate([[[3, 3, 7]], f, [[5, 9, 5], [2, 2, 2]]])                # degenerate faces first, inside and last
    r64, r32 = _refs(bodies, soup, scene, False)
    _check("repeated indices", _query(bodies, soup, scene, False), r64, r32)
    # the synthetic asset's random faces (repeats among them; not closed): finite, whatever they mean
    asset = syn.make_smpl_asset(0)
    rf = np.asarray(asset["faces"])
    assert ((rf[:, 0] == rf[:, 1]) | (rf[:, 1] == rf[:, 2]) | (rf[:, 0] == rf[:, 2])).any()
    vt = np.asarray(asset["v_template"], np.float32)[None]
    pts = np.random.Generator(np.random.PCG64(5)).uniform(-0.5, 0.5, size=(1, 300, 3)).astype(np.float32)
    loss, g, h = _query(vt, rf, pts, False)
    assert np.isfinite(loss).all() and np.isfinite(g).all() and 0 <= h[0] <= 300


def test_body_size_vs_float64():
    """SMPL's counts (6890 vertices, 13 776 faces): the index range, 27 LDS chunks, the gather from a body that does not fit the LDS."""
    v, f = M.peanut(85, 82)
    assert v.shape == (6890, 3) and f.shape == (13776, 3)
    bodies = np.stack([v, 0.7 * v + [0.05, -0.03, 0.02]]).astype(np.float32)
    cand = np.random.Generator(np.random.PCG64(3)).uniform(-0.8, 0.8, size=(540, 3)).astype(np.float32)
    pts, dropped, per64 = M.filter_cloud(bodies, f, cand, 512)
    assert dropped <= 0.01, dropped
    scene = np.broadcast_to(pts.astype(np.float32), (2, 512, 3)).copy()
    r64 = M.mesh_collision_ref(bodies, f, scene, per=per64)
    r32 = M.mesh_collision_ref(bodies, f, scene, dtype=np.float32)                  # (the bounding boxes' points only)
    assert r64["hits"].min() >= 10
    _check("V=6890 F=13776", _query(bodies, f, scene, False), r64, r32)


# ------------------------------------------------------------------------------------------------ plumbing
B_, N_ = 4, 256


@functools.lru_cache(maxsize=None)
def _asset():
    """The synthetic asset with a closed surface: uv_sphere(85, 82)'s connectivity, the peanut's vertices as the template (1.45 m tall)."""
    a = dict(syn.make_smpl_asset(0))
    v, f = M.peanut(85, 82)
    a["faces"], a["v_template"] = f.astype(np.int64), v.astype(np.float32)
    return a


def _model(volsmpl=False):
    from egohmr_amd.factory import build_synthetic_model
    m = build_synthetic_model(torch.device(DEV), 0, diffuse_fuse=True, state_dict=syn.make_state_dict(0), smpl_asset=_asset(), volsmpl=volsmpl)
    m.f16x3_last_steps = None                         # every step f32-grade: the two routes below run the same arithmetic, no calibration run
    return m


def _batch():
    from egohmr_amd.factory import batch_to_device
    bnp = syn.make_batch(B_, N_, seed=61)
    g = np.random.Generator(np.random.PCG64(61))
    t = bnp["smpl_params"]["transl"][:, None, :]
    bnp["scene_pcd_verts_full"][:, : 2 * N_ // 3] = (t + g.uniform(-0.5, 0.5, size=(B_, 2 * N_ // 3, 3))).astype(np.float32)   # points in and around the body
    return batch_to_device(bnp, torch.device(DEV))


def _entry(model, verts, scene, all_points=False):
    from egohmr_amd import _lib
    verts, scene = _lib.f32(verts, model.device), _lib.f32(scene, model.device)
    B, V, N = verts.shape[0], verts.shape[1], scene.shape[1]
    f = model.smpl.collision_faces()
    loss, g, h = torch.empty(B, device=DEV), torch.empty(B, V, 3, device=DEV), torch.empty(B, device=DEV, dtype=torch.int32)
    _lib.api().ehm_mesh_collision_query(verts, f, scene, loss, g, h, B, V, f.shape[0], N, int(all_points), _lib.stream_ptr())
    return loss, g, h


def _sample(model, d, b, noise, rs, fused, w=None):
    d.allow_fused = fused
    kw = {} if w is None else dict(cond_grad_weight=w)
    o = d.val_losses(model, dict(b), shape=[B_, 144], clip_denoised=False, timestep_respacing=rs, compute_loss=False, cond_fn_with_grad=True,
                     noise_stack=noise, **kw)
    d.allow_fused = True
    return {k: o[k].detach().clone() for k in ("pred_x_start", "pred_vertices", "pred_keypoints_3d")}


@pytest.mark.parametrize("sampler", ["ddpm12", "ddim10"])
def test_guided_loop_one_call_equals_step_by_step_and_differs_from_vertex(sampler):
    from egohmr_amd.diffusion import create_gaussian_diffusion
    n, rs, w = (12, "", 5.0) if sampler == "ddpm12" else (50, "ddim10", None)
    d = create_gaussian_diffusion(num_diffusion_timesteps=n, timestep_respacing=rs)
    b = _batch()
    noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B_, seed=61)).to(DEV)
    model = _model()
    model.collision_proxy = "mesh"
    assert model.fused_sampler.guided_steps(d, sampler == "ddim10", 1.0, True) == (11 if sampler == "ddpm12" else 4)
    one, steps = _sample(model, d, b, noise, rs, True, w), _sample(model, d, b, noise, rs, False, w)
    # the bounds of tests/test_gpu_guidance.py::test_guided_ddpm_vs_reference_golden (fused and generic route against one golden: 2e-4 on x0, 1e-4 on
    # vertices and joints), here between the two routes directly
    c = lambda t: t.cpu().numpy()
    np.testing.assert_allclose(c(one["pred_x_start"]), c(steps["pred_x_start"]), atol=2e-4)
    np.testing.assert_allclose(c(one["pred_vertices"]), c(steps["pred_vertices"]), atol=1e-4)
    np.testing.assert_allclose(c(one["pred_keypoints_3d"]), c(steps["pred_keypoints_3d"]), atol=1e-4)
    # not vacuous: the final bodies collide on at least half the items, and the mesh term steers differently from the vertex proxy
    _, _, h = _entry(model, one["pred_vertices"], model.scene_pcd_verts)
    assert int((h > 0).sum()) >= B_ // 2, h.tolist()
    never = _model()                                                                # a model that never left 'vertex'
    ref_vertex = _sample(never, d, b, noise, rs, True, w)
    # (by more than the 2e-4 within which the two routes of ONE term agree above: a difference the routes' rounding does not explain)
    assert float((ref_vertex["pred_x_start"] - one["pred_x_start"]).abs().max()) > 2e-4
    # ... and the mesh guidance is live in the one-call loop: the bound of tests/test_gpu_guidance.py::test_guided_ddim_vs_reference_golden
    un = model.fused_sampler.run(d, dict(b), noise, ddim=sampler == "ddim10", guided=False)["other_outputs"]["pred_x_start"]
    assert float((un - one["pred_x_start"]).abs().max()) > 2e-5
    # switching back runs the vertex proxy again.  On THIS scene no two calls of the vertex-guided loop give the same bits, whatever the model: hundreds
    # of points press on each body and skin_bwd_kernel / nearest_grid_kernel add their shares with float atomics (measured on an MI355X: one model that
    # never left 'vertex', two calls: 1.9e-5 apart in x0 under DDPM-12, 2.9e-7 under DDIM-10; switched back against never switched: 1.5e-6 / 3.3e-7).
    # Here the routes' bound; the bit-for-bit statement is tested below where the vertex loop has bits to reproduce.
    model.collision_proxy = "vertex"
    back = _sample(model, d, b, noise, rs, True, w)
    np.testing.assert_allclose(c(back["pred_x_start"]), c(ref_vertex["pred_x_start"]), atol=2e-4)


@pytest.mark.parametrize("sampler", ["ddpm12", "ddim10"])
def test_switching_back_to_vertex_reproduces_the_bits(sampler):
    """A model switched to 'mesh' and back against a model that never left 'vertex', bit for bit - on a scene where the vertex-guided loop is
    reproducible at all: at most two scene points per item are within reach of the body (two addends commute; every other point lies 10 m away), so
    none of its float-atomic sums depends on the order of arrival."""
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device
    n, rs, w = (12, "", 5.0) if sampler == "ddpm12" else (50, "ddim10", None)
    ddim = sampler == "ddim10"
    d = create_gaussian_diffusion(num_diffusion_timesteps=n, timestep_respacing=rs)
    noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B_, seed=61)).to(DEV)
    never, model = _model(), _model()
    bnp = syn.make_batch(B_, N_, seed=61)
    t = bnp["smpl_params"]["transl"][:, None, :]
    bnp["scene_pcd_verts_full"] = (np.broadcast_to(t, (B_, N_, 3)) + 10.0).astype(np.float32)
    for _ in range(2):                                # two scene points per item ON the unguided body (the scene conditions the body: place them twice)
        b = batch_to_device(bnp, torch.device(DEV))
        v = never.fused_sampler.run(d, dict(b), noise, ddim=ddim, guided=False)["other_outputs"]["pred_vertices"].cpu().numpy()
        bnp["scene_pcd_verts_full"][:, :2] = v[:, [100, 3000]] + t
    b = batch_to_device(bnp, torch.device(DEV))
    un = never.fused_sampler.run(d, dict(b), noise, ddim=ddim, guided=False)["other_outputs"]["pred_x_start"]
    ref_vertex = _sample(never, d, b, noise, rs, True, w)
    assert not torch.equal(ref_vertex["pred_x_start"], un)                        # the vertex guidance is live on this scene
    for k in ref_vertex:
        assert torch.equal(_sample(never, d, b, noise, rs, True, w)[k], ref_vertex[k]), k      # ... and has bits to reproduce
    model.collision_proxy = "mesh"
    mesh = _sample(model, d, b, noise, rs, True, w)
    model.collision_proxy = "vertex"
    back = _sample(model, d, b, noise, rs, True, w)
    for k in back:
        assert torch.equal(back[k], ref_vertex[k]), k
    assert not torch.equal(mesh["pred_x_start"], ref_vertex["pred_x_start"])      # (the mesh term was not the vertex proxy)


def test_metrics_and_penetration_term_are_the_entry():
    from egohmr_amd import loss_grad
    from egohmr_amd.diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="ddim5")
    b = _batch()
    noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B_, seed=61)).to(DEV)
    for volsmpl in (False, True):
        model = _model(volsmpl)
        out = d.val_losses(model, dict(b), shape=[B_, 144], clip_denoised=False, timestep_respacing="ddim5", compute_loss=False, noise_stack=noise)
        verts, scene = out["pred_vertices"], model.scene_pcd_verts
        vertex_metric = model.eval_coll(out)
        model.collision_proxy = "mesh"
        loss, g, h = _entry(model, verts, scene)
        assert int((h > 0).sum()) >= B_ // 2, h.tolist()
        p = out["pred_smpl_params"]
        so = model.smpl(betas=p["betas"], body_pose=p["body_pose"], global_orient=p["global_orient"], pose2rot=False)      # eval_coll's own bodies
        want = (_entry(model, so.vertices, scene)[2].float() / N_).tolist()
        assert model.eval_coll(out) == want and want != vertex_metric
        if volsmpl:
            assert model.eval_coll_volsmpl(out) == want                             # `sdf < 0` read as inside, bbox-selected points
        term, gv = model._penetration_term_proxy(verts, want_grad=True)
        assert torch.equal(term, loss)                                              # (a fixed order: the same bits)
        np.testing.assert_allclose(gv.cpu().numpy(), g.cpu().numpy(), rtol=0, atol=1e-6 * float(g.abs().max()))           # float atomics: last-bit spread
        vq = verts.detach().clone().requires_grad_()
        cot = torch.linspace(0.5, 2.0, B_, device=DEV)
        t2 = loss_grad.ProxyPenetration.apply(model, vq)
        (t2 * cot).sum().backward()
        assert torch.equal(t2.detach(), loss)
        np.testing.assert_allclose(vq.grad.cpu().numpy(), (cot[:, None, None] * g).cpu().numpy(), rtol=0, atol=2e-6 * float(g.abs().max()))
        assert float(g.abs().max()) > 0
        # guide_coll: the stand-alone pieces under 'mesh' give a live gradient on the kept joints only
        bb = dict(b)
        bb["x_t"] = noise[0] * 0.5
        tt = torch.full((B_,), 3, device=DEV)
        grad = model.guide_coll(bb, model(bb, tt), tt).reshape(B_, 24, 6)
        assert float(grad.abs().max()) > 0 and float(grad[:, [0, 3, 6, 9] + list(range(12, 24))].abs().max()) == 0


def test_attached_collision_model_ignores_the_switch():
    class Stub:
        calls = 0

        def collision_loss(self, points, smpl_output, ret_collision_mask=None):
            Stub.calls += 1
            return (smpl_output.vertices.mean(1)[:, None, :] - points).pow(2).sum(-1).mean(-1)

        def query(self, points, smpl_output):
            Stub.calls += 1
            return torch.ones(points.shape[:2], device=points.device)

    from egohmr_amd.diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="ddim5")
    b = _batch()
    noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B_, seed=61)).to(DEV)
    model = _model()
    model.collision_model = Stub()
    out = d.val_losses(model, dict(b), shape=[B_, 144], clip_denoised=False, timestep_respacing="ddim5", compute_loss=False, noise_stack=noise)
    bb = dict(b)
    bb["x_t"] = noise[0] * 0.5
    tt = torch.full((B_,), 3, device=DEV)
    res = {}
    for mode in ("vertex", "mesh"):
        model.collision_proxy = mode
        assert not model.mesh_collision()
        n0 = Stub.calls
        res[mode] = (model.eval_coll(out), model.guide_coll(bb, model(bb, tt), tt))
        assert Stub.calls > n0
    # (the gradient through the attached model ends in ehm_smpl_backward's float atomics: two calls agree to rounding, not to the bit)
    assert res["vertex"][0] == res["mesh"][0]
    np.testing.assert_allclose(res["mesh"][1].cpu().numpy(), res["vertex"][1].cpu().numpy(), rtol=0, atol=1e-5 * float(res["vertex"][1].abs().max()))
    assert float(res["vertex"][1].abs().max()) > 0
