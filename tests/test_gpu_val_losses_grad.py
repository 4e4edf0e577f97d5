"""GPU (MI355X): the VJP of EgoHMR.compute_loss's total (csrc/loss.hip: ehm_val_losses_backward) against float64 torch.autograd on the restatement of
tests/val_losses_grad_ref.py, its NULL outputs, reproducibility and NaN rule; the autograd route of compute_loss; EgoHMR.decode_output against the product's
own forward; x_0 -> rot6d -> SMPL -> loss end to end against the float64 oracle chain; the penetration term's gradient; the chain behind the denoiser.

Measured on an MI355X (docs/EXPERIMENTS.md R11.1): kernel against float64, all 36 cases, every element: largest |g - ref| / |ref| 5.89e-08 against the bound 2^-23 = 1.19e-07
(one float32 rounding; pelvis-joint elements alone 5.79e-08: their sums need no wider bound); every figure of the chain tests is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import val_losses_grad_ref as G  # noqa: E402
import val_losses_ref as R  # noqa: E402
from egohmr_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

WEIGHTS = [R.CASE_WEIGHTS[k] for k in R.WEIGHT_NAMES]
NAMES = G.PREDICTIONS + ("penetration",)
# the kernel forms every element in float64 and rounds it to float32 once: half a float32 spacing, 2^-24 |ref|; the bound is one spacing, plus one float32
# denormal for an element whose float64 value is below the float32 range
KERNEL_RTOL, F32_DENORMAL = 2.0 ** -23, 2.0 ** -149
VJP_ATOL_REL, VJP_RTOL = 2e-4, 2e-3                          # the project's bar for the SMPL / rot6d VJP chains (tests/test_gpu_smpl_autograd.py): a ceiling
SHAPES = [(1, 1, 11), (2, 7, 12), (5, 7, 13), (3, 1366, 14), (3, 6890, 15), (4, 1023, 16)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _to_dev(inp, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inp.items()}


def _native_grads(t, gloss, dev, want=NAMES):
    """ehm_val_losses_backward into NaN-filled outputs -> {name: numpy}."""
    from egohmr_amd.loss_grad import val_losses_grad_native
    B = t["pred_vertices"].shape[0]
    out = {k: torch.full((B,) if k == "penetration" else tuple(t[k].shape), float("nan"), device=dev) for k in want}
    g = val_losses_grad_native(t, WEIGHTS, None if gloss is None else torch.tensor([gloss], device=dev, dtype=torch.float32), want, out)
    torch.cuda.synchronize()
    assert all(g[k] is out[k] for k in want)
    return {k: v.cpu().numpy() for k, v in g.items()}


def l1_margin(inp):
    """Smallest |argument| of an L1 term (float64), the structural zeros of joint 0 in the pelvis-aligned term apart."""
    f = {k: np.asarray(v, np.float64) for k, v in inp.items() if k != "gender"}
    fem = (np.asarray(inp["gender"]) == 1)[:, None, None]
    gv, gj = np.where(fem, f["gt_vertices_female"], f["gt_vertices_male"]), np.where(fem, f["gt_joints_female"], f["gt_joints_male"])
    p3, g3 = f["pred_keypoints_3d"][:, :24], f["keypoints_3d"][:, :24]
    ds = [(f["pred_vertices"] - p3[:, [0]]) - (gv - gj[:, [0]]), ((p3 - p3[:, [0]]) - (g3 - g3[:, [0]]))[:, 1:],
          f["pred_keypoints_3d_full"][:, :24] - f["keypoints_3d_full"][:, :24], f["pred_keypoints_2d_full"][:, R.SMPL_TO_OPENPOSE] - f["keypoints_2d"][:, :25, :2]]
    return min(float(np.abs(d).min()) for d in ds)


# ---------------------------------------------------------------------------------------------- a. the kernel against float64
@pytest.mark.parametrize("genders", ["mixed", "male", "female"])
@pytest.mark.parametrize("gloss", [None, 0.37])
@pytest.mark.parametrize("B,V,seed", SHAPES)
def test_kernel_against_float64(dev, B, V, seed, gloss, genders):
    """Every element of every gradient array, no exclusions.  Measured on an MI355X: 5.89e-08 relative at most over the 36 cases, 5.79e-08 on the pelvis-joint elements."""
    inp = R.random_kernel_inputs(B, V, seed, genders)
    assert l1_margin(inp) > 1e-6                                # no sign can differ between float32-input float64 arithmetic on the two sides
    pen = np.random.default_rng(seed + 1).uniform(0.0, 2.0, size=B)
    gl = 1.0 if gloss is None else float(np.float32(gloss))
    ref = G.val_losses_grads64(inp, WEIGHTS, gl, pen)
    got = _native_grads(_to_dev(inp, dev), gloss, dev)
    worst = {}
    for k in NAMES:
        assert got[k].shape == ref[k].shape and got[k].dtype == np.float32, k
        err = np.abs(got[k].astype(np.float64) - ref[k])
        worst[k] = float((err / np.maximum(np.abs(ref[k]), 1e-300)).max())
        bad = ~(err <= KERNEL_RTOL * np.abs(ref[k]) + F32_DENORMAL)            # (a NaN left in an output fails here)
        assert not bad.any(), f"{k}: {int(bad.sum())} elements off, first at {np.argwhere(bad)[0].tolist()}, largest relative deviation {worst[k]:.3e}"
    pelvis = np.abs(got["pred_keypoints_3d"][:, 0].astype(np.float64) - ref["pred_keypoints_3d"][:, 0]) / np.maximum(np.abs(ref["pred_keypoints_3d"][:, 0]), 1e-300)
    print(f"B={B} V={V} gloss={gl:g} {genders}: largest relative deviation {max(worst.values()):.3e} (bound {KERNEL_RTOL:.3e}); pelvis joint {float(pelvis.max()):.3e}")
    # written in full: joints 24.. and the 2-D joints outside smpl_to_openpose are exact zeros
    assert not got["pred_keypoints_3d"][:, 24:].any() and not got["pred_keypoints_3d_full"][:, 24:].any()
    outside = [j for j in range(45) if j not in R.SMPL_TO_OPENPOSE]
    assert not got["pred_keypoints_2d_full"][:, outside].any()


# ---------------------------------------------------------------------------------------------- b. NULL outputs, reproducibility
def test_null_outputs_and_bit_equality(dev):
    inp = R.random_kernel_inputs(3, 1366, 14, "mixed")
    t = _to_dev(inp, dev)
    full, again = _native_grads(t, 0.37, dev), _native_grads(t, 0.37, dev)
    for k in NAMES:
        assert np.array_equal(full[k].view(np.uint32), again[k].view(np.uint32)), k
    for skip in NAMES:
        part = _native_grads(t, 0.37, dev, tuple(k for k in NAMES if k != skip))
        assert skip not in part
        for k in part:
            assert np.array_equal(full[k].view(np.uint32), part[k].view(np.uint32)), (skip, k)
    rest = tuple(k for k in NAMES if k not in ("pred_vertices", "pred_keypoints_3d"))
    part = _native_grads(t, 0.37, dev, rest)                                    # no vertex pass at all
    for k in rest:
        assert np.array_equal(full[k].view(np.uint32), part[k].view(np.uint32)), k
    assert _native_grads(t, 0.37, dev, ()) == {}


# ---------------------------------------------------------------------------------------------- c. NaN containment
def test_nan_containment(dev):
    B, V = 4, 1023
    inp = R.random_kernel_inputs(B, V, 16, "mixed")
    base = _native_grads(_to_dev(inp, dev), None, dev)
    for b, v, c in ((1, 0, 0), (2, V - 1, 2), (3, 600, 1)):                     # a head or first-quad float, the tail, the aligned middle
        bad = dict(inp, pred_vertices=inp["pred_vertices"].copy())
        bad["pred_vertices"][b, v, c] = np.nan
        got = _native_grads(_to_dev(bad, dev), None, dev)
        where = np.zeros((B, V, 3), bool)
        where[b, v, c] = True
        assert np.array_equal(np.isnan(got["pred_vertices"]), where)
        assert np.array_equal(got["pred_vertices"][~where].view(np.uint32), base["pred_vertices"][~where].view(np.uint32))
        pj = np.zeros((B, 45, 3), bool)
        pj[b, 0, c] = True
        assert np.array_equal(np.isnan(got["pred_keypoints_3d"]), pj)
        assert np.array_equal(got["pred_keypoints_3d"][~pj].view(np.uint32), base["pred_keypoints_3d"][~pj].view(np.uint32))
        for k in NAMES[2:]:
            assert np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32)), k


# ---------------------------------------------------------------------------------------------- the model
def _model(dev, synth_weights, smpl_asset, **kw):
    from egohmr_amd.factory import build_synthetic_model
    return build_synthetic_model(dev, 0, diffuse_fuse=True, state_dict=synth_weights, smpl_asset=smpl_asset, smpl_asset_male=syn.make_smpl_asset(1),
                                 smpl_asset_female=syn.make_smpl_asset(2), start_coap_epoch=R.START_COAP_EPOCH, **{**R.CASE_WEIGHTS, **kw})


@pytest.fixture(scope="module")
def model(dev, synth_weights, smpl_asset):
    return _model(dev, synth_weights, smpl_asset)


def _batch(golden_dir, case, B, dev):
    """The first B items of a g21 golden's annotated batch (tests/val_losses_ref.golden_batch) on the device, and the golden."""
    from egohmr_amd.factory import batch_to_device
    g = np.load(os.path.join(golden_dir, f"g21_val_losses_{case}.npz"))
    b_np, flags = R.golden_batch(g)
    cut = lambda d: {k: (cut(v) if isinstance(v, dict) else v[:B]) for k, v in d.items()}
    batch = batch_to_device(cut(b_np), dev)
    batch["smpl_params_is_axis_angle"] = {k: v[:B] for k, v in flags.items()}
    batch["x_t"] = torch.from_numpy(g["x_t"][:B]).to(dev)
    return batch, g


def _flat_losses(o):
    return torch.stack([o["losses"][k] for k in R.LOSS_KEYS]).cpu().numpy()


# ---------------------------------------------------------------------------------------------- d. route choice
def test_route_choice_and_equal_bits(dev, golden_dir, model):
    from egohmr_amd.model import val_losses_native
    B = 3
    batch, g = _batch(golden_dir, "a", B, dev)
    out = model(batch, torch.full((B,), int(g["timestep"]), device=dev, dtype=torch.long))
    o = dict(out)
    loss = model.compute_loss(batch, o)                                          # gradients enabled, nothing requires grad: today's path
    assert loss.grad_fn is None and not loss.requires_grad and loss is o["losses"]["loss"]
    direct = val_losses_native(model.loss_inputs(batch, out), model.loss_weights(), None)
    assert np.array_equal(_flat_losses(o).view(np.uint32), direct["losses"].cpu().numpy().view(np.uint32))
    og = dict(out, pred_vertices=out["pred_vertices"].clone().requires_grad_())
    with torch.no_grad():
        assert model.compute_loss(batch, dict(og)).grad_fn is None               # requires grad, gradients disabled: today's path
    lg = model.compute_loss(batch, og)
    assert lg.grad_fn is not None and lg.shape == () and torch.equal(lg.detach(), loss)
    assert np.array_equal(_flat_losses(og).view(np.uint32), _flat_losses(o).view(np.uint32))
    assert all(not v.requires_grad for v in og["losses"].values()) and all(not v.requires_grad for v in og["losses_per_item"].values())
    assert not og["joint_vis_num_batch"].requires_grad and int(og["joint_vis_num_batch"]) == int(o["joint_vis_num_batch"])
    for k in o["losses_per_item"]:
        assert torch.equal(o["losses_per_item"][k], og["losses_per_item"][k]), k
    lg.backward()
    gv = og["pred_vertices"].grad
    assert gv.shape == out["pred_vertices"].shape and float(gv.abs().max()) > 0
    # the vertex gradient of the route = the kernel's, on the same arrays
    t = model.loss_inputs(batch, out)
    ref = _native_grads(t, None, dev, ("pred_vertices",))["pred_vertices"]
    assert np.array_equal(gv.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    (g2,) = torch.autograd.grad(model.compute_loss(batch, og) * model.compute_loss(batch, og), [og["pred_vertices"]], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        g2.sum().backward()


# ---------------------------------------------------------------------------------------------- e. decode_output against the product
def test_decode_output_matches_forward(dev, golden_dir, model):
    B = 3
    batch, g = _batch(golden_dir, "a", B, dev)
    o = model(batch, torch.full((B,), int(g["timestep"]), device=dev, dtype=torch.long))
    attrs = {k: getattr(model, k) for k in ("scene_pcd_verts", "input_transl", "focal_length", "camera_center_full")}
    with torch.no_grad():
        d = model.decode_output(batch, o["pred_x_start"])
    assert list(d) == list(o) and list(d["pred_smpl_params"]) == list(o["pred_smpl_params"])
    flat = lambda x: {**{k: v for k, v in x.items() if k != "pred_smpl_params"}, **x["pred_smpl_params"]}
    fo, fd = flat(o), flat(d)
    for k in fo:
        assert fd[k].shape == fo[k].shape and fd[k].dtype == fo[k].dtype and not fd[k].requires_grad, k
        err = float((fd[k] - fo[k]).abs().max())
        print(f"[decode] {k}: max|diff| {err:.3g} of max {float(fo[k].abs().max()):.3g}")
        assert err <= 1e-5, k
    dist = float((d["pred_vertices"] - o["pred_vertices"]).norm(dim=-1).max())
    print(f"[decode] largest vertex distance {dist:.3g} m (contract 1e-4 m)")
    assert dist <= 1e-4
    for k, v in attrs.items():
        assert float((getattr(model, k) - v).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max())), k
    assert torch.equal(model.smpl_output.vertices, d["pred_vertices"]) and model.smpl_output.full_pose.shape == (B, 24, 3, 3)


# ---------------------------------------------------------------------------------------------- f. end to end, x_0 -> loss
def _oracle_chain_grads(model, batch, x0, betas, out_dev, want_betas):
    """Float64 gradient of the loss w.r.t. x0 (and betas): the oracle chain (oracle/geometry, SMPLOracle, projection) from the same x0, with the loss
    cotangents of val_losses_torch64 evaluated AT THE DEVICE'S OWN float32 forward values injected as grad_outputs - so no sign of an L1 term can differ
    between the two sides because of the forwards' ~1e-6 m difference."""
    from oracle import geometry as ogeo
    from oracle.smpl import SMPLOracle
    B = x0.shape[0]
    t = {k: v.detach().cpu().numpy() for k, v in model.loss_inputs(batch, out_dev).items()}
    cot = G.val_losses_grads64(t, model.loss_weights())
    st = model.fused_sampler.prepare(batch)
    mean, std = (torch.from_numpy(a).double() for a in syn.make_body_rep_stats(0))
    x = x0.detach().cpu().double().requires_grad_()
    b = betas.detach().cpu().double().requires_grad_()
    pose6d = x * std + mean
    Rm = ogeo.rot6d_to_rotmat(pose6d, "diffusion").view(B, 24, 3, 3)
    so = SMPLOracle(syn.make_smpl_asset(0), torch.float64)(betas=b, body_pose=Rm[:, 1:], global_orient=Rm[:, [0]])
    transl = st.transl.cpu().double()
    focal, center = model.focal_length.detach().cpu().double(), model.camera_center_full.detach().cpu().double()
    kp2d = ogeo.perspective_projection(so.joints, transl, focal, center)
    kp2d = torch.stack([kp2d[..., 0] / 1920 - 0.5, kp2d[..., 1] / 1080 - 0.5], dim=-1)
    outs = [so.vertices, so.joints, so.joints + transl[:, None], kp2d, Rm[:, [0]].reshape(B, 9), Rm[:, 1:].reshape(B, 207), b, pose6d]
    gos = [torch.from_numpy(cot[k]).reshape(o.shape) for k, o in zip(G.PREDICTIONS, outs)]
    grads = torch.autograd.grad(outs, [x, b] if want_betas else [x], grad_outputs=gos)
    return [g.numpy() for g in grads]


def _check_vjp(tag, got, ref):
    S = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    print(f"[x0->loss] {tag}: max|err| {err:.3g} = {err / S:.3g} of max|ref| {S:.3g}")
    assert S > 0
    np.testing.assert_allclose(got, ref, atol=VJP_ATOL_REL * S, rtol=VJP_RTOL, err_msg=tag)


def _x0_loss_backward(model, batch, x0, betas=None, cur_epoch=0):
    x = x0.detach().clone().requires_grad_()
    b = None if betas is None else betas.detach().clone().requires_grad_()
    out = model.decode_output(batch, x, betas=b)
    loss = model.compute_loss(batch, out, cur_epoch=cur_epoch)
    assert loss.grad_fn is not None
    loss.backward()
    return x, b, out, loss


@pytest.fixture(scope="module")
def x0_case(dev, golden_dir, model):
    """B -> (batch, x0 of the product's forward, x0.grad of decode_output -> compute_loss -> backward): computed once per B, shared, left unchanged."""
    cache = {}

    def get(B):
        if B not in cache:
            batch, g = _batch(golden_dir, "a", B, dev)
            x0 = model(batch, torch.full((B,), int(g["timestep"]), device=dev, dtype=torch.long))["pred_x_start"]
            x, _, out, loss = _x0_loss_backward(model, batch, x0)
            cache[B] = (batch, x0, x.grad.clone(), out, loss.detach())
        return cache[B]
    return get


@pytest.mark.parametrize("B", [2, 5])
def test_x0_to_loss_against_the_float64_chain(dev, model, x0_case, B):
    batch, x0, gx, out, loss = x0_case(B)
    assert torch.isfinite(gx).all() and gx.shape == (B, 144)
    betas = model.fused_sampler.prepare(batch).betas
    (ref,) = _oracle_chain_grads(model, batch, x0, betas, out, want_betas=False)
    _check_vjp(f"B={B} x0.grad", gx.cpu().numpy().astype(np.float64), ref)
    # the value on this route = today's path on the same (detached) output
    plain = model.compute_loss(batch, {k: ({a: b.detach() for a, b in v.items()} if isinstance(v, dict) else v.detach()) for k, v in out.items()
                                       if k.startswith("pred_")})
    assert plain.grad_fn is None and torch.equal(plain, loss)
    # betas handed to decode_output as a leaf
    x, b, out_b, _ = _x0_loss_backward(model, batch, x0, betas=betas)
    ref_x, ref_b = _oracle_chain_grads(model, batch, x0, betas, out_b, want_betas=True)
    _check_vjp(f"B={B} x0.grad (betas a leaf)", x.grad.cpu().numpy().astype(np.float64), ref_x)
    _check_vjp(f"B={B} betas.grad", b.grad.cpu().numpy().astype(np.float64), ref_b)


# ---------------------------------------------------------------------------------------------- g. the penetration term
def test_penetration_gradient(dev, golden_dir, synth_weights, smpl_asset):
    """Case b's scene at cur_epoch >= start_coap_epoch.  Proxy route: x0.grad with the term on minus x0.grad with it off = weight / B times the guidance VJP
    of the same bodies (ehm_collision_query's vertex gradient on the capped points through ehm_smpl_backward_rot6d); with the proxy plugged in as
    collision_model (an adapter in plain torch) the gradient agrees with the proxy route.  Both at the VJP bar."""
    from egohmr_amd import _lib
    from test_gpu_smpl_autograd import ProxyAdapter
    B = 6
    m = _model(dev, synth_weights, smpl_asset)
    batch, g = _batch(golden_dir, "b", B, dev)
    x0 = m(batch, torch.full((B,), int(g["timestep"]), device=dev, dtype=torch.long))["pred_x_start"]
    off = _x0_loss_backward(m, batch, x0, cur_epoch=R.START_COAP_EPOCH - 1)[0].grad
    x, _, out, _ = _x0_loss_backward(m, batch, x0, cur_epoch=R.START_COAP_EPOCH)
    on = x.grad
    pen = out["losses_per_item"]["loss_coap_penetration"]
    assert float(pen[0]) > 0 and float(pen[1]) == 0 and float(out["losses"]["loss_coap_penetration"]) > 0
    # the existing guidance VJP of the same bodies
    term, gverts = m._penetration_term_proxy(out["pred_vertices"].detach(), want_grad=True)
    np.testing.assert_allclose(term.cpu().numpy(), pen.cpu().numpy(), rtol=1e-5, atol=0)     # (the proxy's loss is a float-atomic sum: two calls agree to the last bits only)
    mean, std = m._std_mean()
    gpose = torch.empty(B, 144, device=dev)
    betas = m.fused_sampler.prepare(batch).betas
    _lib.api().ehm_smpl_backward_rot6d(m.smpl.handle(), betas, x0.contiguous(), mean, std, gverts, gpose, B, _lib.stream_ptr())
    ref = (gpose * std).double().cpu().numpy() * (R.CASE_WEIGHTS["weight_coap_penetration"] / B)       # d pose6d / d x0 = std
    diff = (on.double() - off.double()).cpu().numpy()
    _check_vjp("penetration, proxy route: grad(on) - grad(off)", diff, ref)
    assert float(np.abs(diff[1]).max()) <= VJP_ATOL_REL * float(np.abs(ref).max())                       # item 1 selects no point
    # the same through an attached collision model
    m.collision_model = adapter = ProxyAdapter(m.collision_tau)
    try:
        xm, _, out_m, _ = _x0_loss_backward(m, batch, x0, cur_epoch=R.START_COAP_EPOCH)
    finally:
        m.collision_model = None
    assert 0 < adapter.loss_calls <= B                                                                   # one call per item whose box holds a scene point
    np.testing.assert_allclose(out_m["losses_per_item"]["loss_coap_penetration"].cpu().numpy(), pen.cpu().numpy(), rtol=1e-5, atol=0)
    _check_vjp("penetration, collision_model against the proxy route", xm.grad.double().cpu().numpy(), on.double().cpu().numpy())
    _check_vjp("penetration, collision_model: grad(on) - grad(off)", (xm.grad.double() - off.double()).cpu().numpy(), ref)


# ---------------------------------------------------------------------------------------------- h. behind the denoiser
def test_chain_behind_the_denoiser(dev, model, x0_case):
    """ModulatedGCN.forward -> decode_output -> compute_loss -> backward.  The composition only: x.grad equals GCNFunction's VJP applied to the cotangent the
    chain handed it, bit for bit (the SMPL VJP sums with float atomics, so that cotangent is compared with another run's only at the VJP bar)."""
    from egohmr_amd.model import ModulatedGCN, smpl_tree_adjacency
    B = 2
    batch, x0_f, gx_f, _, _ = x0_case(B)
    torch.manual_seed(7)
    gcn = ModulatedGCN(smpl_tree_adjacency(), in_dim=70, hid_dim=128, num_layers=1).to(dev).eval()
    x = torch.randn(B, 24, 70, device=dev).requires_grad_()
    x0 = gcn(x)
    assert x0.shape == (B, 24, 6) and x0.grad_fn is not None
    x0.retain_grad()
    out = model.decode_output(batch, x0.reshape(B, 144))
    model.compute_loss(batch, out).backward()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
    (ref,) = torch.autograd.grad(gcn(x), [x], grad_outputs=x0.grad)
    assert torch.equal(x.grad, ref)
    # fed case f's x0, the chain hands the denoiser case f's x0.grad
    leaf = x0_f.detach().clone().reshape(B, 24, 6).requires_grad_()
    model.compute_loss(batch, model.decode_output(batch, leaf.reshape(B, 144))).backward()
    _check_vjp("cotangent at the denoiser's output against case f", leaf.grad.reshape(B, 144).double().cpu().numpy(), gx_f.double().cpu().numpy())
