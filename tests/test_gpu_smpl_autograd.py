"""GPU (MI355X): the differentiable SMPL.forward (ehm_smpl_backward behind a torch.autograd.Function) against float64 autograd through
oracle.smpl.SMPLOracle, and the pluggable collision model (EgoHMR.collision_model): the reference's autograd route of guide_coll / eval_coll
with an adapter around the build's proxy, against the oracle, the built-in proxy route and the reference's own guided runs (goldens g9, g12).

The gradient bound is the bar of tests/test_gpu_guidance.py for these VJP kernels: atol = 2e-4 max|ref|, rtol = 2e-3 - a ceiling.  Every case prints
its measured max|err| / max|ref| before it asserts (docs/EXPERIMENTS.md R9.1 holds the figures of the MI355X run)."""
import os

import numpy as np
import pytest
import torch

from egohmr_amd import synthetic as syn

pytestmark = pytest.mark.gpu

VJP_ATOL_REL, VJP_RTOL = 2e-4, 2e-3


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, synth_weights, smpl_asset):
    from egohmr_amd.factory import build_synthetic_model
    return build_synthetic_model(dev, 0, diffuse_fuse=True, state_dict=synth_weights, smpl_asset=smpl_asset)


@pytest.fixture()
def plugged(model):
    """The shared model with a counting proxy adapter attached for one test."""
    model.collision_model = ProxyAdapter(model.collision_tau)
    try:
        yield model
    finally:
        model.collision_model = None
        model.guide_denom_override = None


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _dense_asset(smpl_asset):
    """tests/test_gpu_collision.py's body model: a third of the vertices carry six skinning weights (no sparse-4 packing, VALU skinning)."""
    asset = dict(smpl_asset)
    g = _rng(77)
    w = np.array(asset["lbs_weights"], dtype=np.float64).copy()
    for v in g.choice(w.shape[0], size=w.shape[0] // 3, replace=False):
        js = g.choice(w.shape[1], size=6, replace=False)
        w[v] = 0.0
        w[v, js] = g.uniform(0.05, 1.0, size=6)
        w[v] /= w[v].sum()
    asset["lbs_weights"] = w.astype(np.float32)
    return asset


# ------------------------------------------------------------------------------------------------ part 1: gradients against the float64 oracle
def _case(B, seed, V=6890, J=45):
    """Random rot6d-derived rotation matrices (float32 values, shared by both sides), betas, transl, dense cotangents on vertices and all joints."""
    from oracle import geometry as ogeo
    g = _rng(seed)
    f = lambda *s: torch.from_numpy(g.normal(size=s).astype(np.float32))
    R = ogeo.rot6d_to_rotmat(f(B, 144), "diffusion").view(B, 24, 3, 3).contiguous()
    return dict(R=R, betas=f(B, 10), transl=f(B, 3), gv=f(B, V, 3), gj=f(B, J, 3))


def _loss(out, gv, gj):
    terms = []
    if gv is not None:
        terms.append((out.vertices * gv).sum())
    if gj is not None:
        terms.append((out.joints * gj).sum())
    return sum(terms)


def _grads(smpl, c, to, use_gv=True, use_gj=True):
    """autograd.grad of (vertices . gv).sum() + (joints . gj).sum() w.r.t. global_orient, body_pose, betas, transl; `to` places / casts a tensor."""
    go, bp = to(c["R"][:, :1]).requires_grad_(), to(c["R"][:, 1:]).requires_grad_()
    betas, transl = to(c["betas"]).requires_grad_(), to(c["transl"]).requires_grad_()
    out = smpl(betas=betas, body_pose=bp, global_orient=go, transl=transl, pose2rot=False)
    g = torch.autograd.grad(_loss(out, to(c["gv"]) if use_gv else None, to(c["gj"]) if use_gj else None), [go, bp, betas, transl])
    return dict(zip(("global_orient", "body_pose", "betas", "transl"), (t.detach().double().cpu() for t in g)))


def _check(tag, got, ref):
    """Prints max|err| / max|ref| per output, then asserts the bound on each."""
    rel = {}
    for k in ref:
        S = float(ref[k].abs().max())
        rel[k] = float((got[k].double().cpu() - ref[k]).abs().max()) / S if S > 0 else float(got[k].abs().max())
    print(f"[smpl-vjp] {tag}: " + "  ".join(f"{k} {v:.3g}" for k, v in rel.items()))
    for k in ref:
        np.testing.assert_allclose(got[k].double().cpu().numpy(), ref[k].numpy(), atol=VJP_ATOL_REL * float(ref[k].abs().max()), rtol=VJP_RTOL, err_msg=f"{tag}: {k}")
    return rel


@pytest.mark.parametrize("cot", ["both", "vertices", "joints"])
@pytest.mark.parametrize("B", [2, 11, 257])
def test_forward_gradients_vs_fp64_oracle(dev, model, smpl_asset, B, cot):
    """global_orient, body_pose, betas and transl separately; vertices-only and joints-only cotangents reach the kernel as NULL inputs."""
    from oracle.smpl import SMPLOracle
    c = _case(B, 31 + B)
    use_gv, use_gj = cot in ("both", "vertices"), cot in ("both", "joints")
    ref = _grads(SMPLOracle(smpl_asset, torch.float64), c, lambda t: t.double().clone(), use_gv, use_gj)
    got = _grads(model.smpl, c, lambda t: t.to(dev).clone(), use_gv, use_gj)
    assert all(float(v.abs().max()) > 0 for v in ref.values())
    _check(f"B={B} {cot}", got, ref)


def test_forward_gradients_axis_angle_inputs(dev, model, smpl_asset):
    """pose2rot=True: aa_to_rotmat is plain torch, so the gradient reaches the axis-angle inputs."""
    from egohmr_amd.geometry import aa_to_rotmat
    from oracle.smpl import SMPLOracle
    B = 7
    g = _rng(41)
    f = lambda *s: torch.from_numpy(g.normal(scale=0.6, size=s).astype(np.float32))
    go, bp, betas, gv, gj = f(B, 3), f(B, 69), f(B, 10), f(B, 6890, 3), f(B, 45, 3)
    a, b, c = go.double().requires_grad_(), bp.double().requires_grad_(), betas.double().requires_grad_()
    o = SMPLOracle(smpl_asset, torch.float64)(betas=c, body_pose=aa_to_rotmat(b.reshape(-1, 3)).view(B, 23, 3, 3), global_orient=aa_to_rotmat(a.reshape(-1, 3)).view(B, 1, 3, 3))
    ref = dict(zip(("global_orient", "body_pose", "betas"), torch.autograd.grad(_loss(o, gv.double(), gj.double()), [a, b, c])))
    a, b, c = (t.to(dev).requires_grad_() for t in (go, bp, betas))
    o = model.smpl(betas=c, body_pose=b, global_orient=a)
    got = dict(zip(("global_orient", "body_pose", "betas"), torch.autograd.grad(_loss(o, gv.to(dev), gj.to(dev)), [a, b, c])))
    _check("axis-angle in", got, ref)


def test_full_pose_stays_in_the_graph(dev, model, smpl_asset):
    """return_full_pose=True -> rotation_matrix_to_angle_axis(full_pose) with a cotangent on the axis-angle output backpropagates into the same inputs."""
    from egohmr_amd.geometry import rotation_matrix_to_angle_axis
    from oracle import geometry as ogeo
    from oracle.smpl import SMPLOracle
    B = 9
    c = _case(B, 51)
    ga = torch.from_numpy(_rng(52).normal(size=(B, 24, 3)).astype(np.float32))

    def run(smpl, aa_fn, to):
        go, bp, betas = to(c["R"][:, :1]).requires_grad_(), to(c["R"][:, 1:]).requires_grad_(), to(c["betas"]).requires_grad_()
        o = smpl(betas=betas, body_pose=bp, global_orient=go, return_full_pose=True, pose2rot=False)
        aa = aa_fn(o.full_pose.reshape(-1, 3, 3)).reshape(B, 24, 3)
        loss = (aa * to(ga)).sum() + (o.vertices * to(c["gv"])).sum()
        return dict(zip(("global_orient", "body_pose", "betas"), torch.autograd.grad(loss, [go, bp, betas])))
    ref = run(SMPLOracle(smpl_asset, torch.float64), ogeo.rotation_matrix_to_angle_axis, lambda t: t.double().clone())
    got = run(model.smpl, rotation_matrix_to_angle_axis, lambda t: t.to(dev).clone())
    _check("full_pose -> axis-angle", got, ref)
    # the axis-angle cotangent alone (no vertex / joint cotangent at all: the SMPL node gets no gradient and must not be asked for one)
    go = c["R"][:, :1].to(dev).requires_grad_()
    o = model.smpl(betas=c["betas"].to(dev), body_pose=c["R"][:, 1:].to(dev), global_orient=go, return_full_pose=True, pose2rot=False)
    (rotation_matrix_to_angle_axis(o.full_pose.reshape(-1, 3, 3)).reshape(B, 24, 3)[:, 0] * ga[:, 0].to(dev)).sum().backward()
    assert float(go.grad.abs().max()) > 0


def test_expanded_betas_reduce(dev, model, smpl_asset):
    """betas [1,10] against B poses: the gradient is the sum over the bodies."""
    from oracle.smpl import SMPLOracle
    B = 11
    c = _case(B, 61)
    b1 = c["betas"][:1]

    def run(smpl, to):
        betas, bp = to(b1).requires_grad_(), to(c["R"][:, 1:]).requires_grad_()
        o = smpl(betas=betas if smpl is model.smpl else betas.expand(B, -1), body_pose=bp, global_orient=to(c["R"][:, :1]), pose2rot=False)
        return dict(zip(("betas", "body_pose"), torch.autograd.grad(_loss(o, to(c["gv"]), to(c["gj"])), [betas, bp])))
    ref = run(SMPLOracle(smpl_asset, torch.float64), lambda t: t.double().clone())
    got = run(model.smpl, lambda t: t.to(dev).clone())
    assert got["betas"].shape == (1, 10)
    _check("expanded betas", got, ref)


@pytest.mark.parametrize("B", [9, 33])
def test_forward_gradients_dense_skinning_weights(dev, smpl_asset, B):
    from egohmr_amd.smpl import SMPL
    from oracle.smpl import SMPLOracle
    asset = _dense_asset(smpl_asset)
    smpl = SMPL(asset).to(dev)
    c = _case(B, 71 + B)
    ref = _grads(SMPLOracle(asset, torch.float64), c, lambda t: t.double().clone())
    got = _grads(smpl, c, lambda t: t.to(dev).clone())
    _check(f"dense weights B={B}", got, ref)


@pytest.mark.parametrize("B", [2, 33])
def test_autograd_route_equals_the_rot6d_vjp(dev, model, B):
    """autograd.grad through rot6d_to_rotmat -> SMPL.forward with a vertex cotangent = ehm_smpl_backward_rot6d on the same inputs."""
    from egohmr_amd import _lib
    from egohmr_amd.geometry import rot6d_to_rotmat
    g = _rng(81 + B)
    f = lambda *s: torch.from_numpy(g.normal(size=s).astype(np.float32)).to(dev)
    x, betas, gv = f(B, 144), f(B, 10), f(B, 6890, 3)
    mean, std = (torch.from_numpy(a).to(dev) for a in syn.make_body_rep_stats(0))
    ref = torch.empty(B, 144, device=dev)
    _lib.api().ehm_smpl_backward_rot6d(model.smpl.handle(), betas, x, mean, std, gv, ref, B, _lib.stream_ptr())
    p6 = (x * std + mean).requires_grad_()
    R = rot6d_to_rotmat(p6.reshape(-1, 6), "diffusion").view(B, 24, 3, 3)
    o = model.smpl(betas=betas, body_pose=R[:, 1:], global_orient=R[:, [0]], pose2rot=False)
    got = torch.autograd.grad((o.vertices * gv).sum(), [p6])[0]
    _check(f"vs rot6d VJP B={B}", {"pose6d": got}, {"pose6d": ref.double().cpu()})


def test_double_backward_is_refused(dev, model):
    c = _case(2, 91)
    go = c["R"][:, :1].to(dev).requires_grad_()
    o = model.smpl(betas=c["betas"].to(dev), body_pose=c["R"][:, 1:].to(dev), global_orient=go, pose2rot=False)
    (g,) = torch.autograd.grad(o.joints.square().sum(), [go], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        g.sum().backward()


def _backward_twice(dev, model, c, gv, gj):
    """Two backward passes over the same inputs -> ({name: first}, {name: second})."""
    runs = []
    for _ in range(2):
        go, bp, betas = (t.to(dev).clone().requires_grad_() for t in (c["R"][:, :1], c["R"][:, 1:], c["betas"]))
        o = model.smpl(betas=betas, body_pose=bp, global_orient=go, pose2rot=False)
        g = torch.autograd.grad(_loss(o, None if gv is None else gv.to(dev), None if gj is None else gj.to(dev)), [go, bp, betas])
        runs.append(dict(zip(("global_orient", "body_pose", "betas"), (t.detach().cpu() for t in g))))
    return runs


def test_backward_twice_is_bit_equal_where_the_sums_are_defined(dev, model):
    """What ehm_smpl_backward promises about reproducibility, no more: its own kernels sum in a fixed order, but the per-joint transform gradients gA come
    from skin_bwd_kernel's float atomics.  A sum of at most two float terms does not depend on their order, so with two hot vertices per body, or a
    cotangent on the 24 posed joints alone (no vertex gradient at all: gA = 0), two calls give the same bits in grotmats AND gbetas."""
    B = 33
    c = _case(B, 111)
    picks = [0, c["gv"].shape[1] - 1]                                       # the first and the last vertex: different skinning tiles
    gv = torch.zeros_like(c["gv"])
    gv[:, picks] = c["gv"][:, picks]
    gj24 = c["gj"].clone()
    gj24[:, 24:] = 0                                                        # the vertex-picked joints would make 21 more hot vertices
    for tag, a, b in (("two hot vertices", gv, None), ("two hot vertices + 24 posed joints", gv, gj24), ("24 posed joints", None, gj24)):
        first, second = _backward_twice(dev, model, c, a, b)
        for k in first:
            assert float(first[k].abs().max()) > 0, (tag, k)
            assert torch.equal(first[k], second[k]), (tag, k)


def test_backward_twice_dense_cotangent_spread(dev, model):
    """A dense cotangent (the case autograd creates): thousands of vertices per joint go through skin_bwd_kernel's float atomics, so two calls agree only
    up to the order of float32 additions.  Prints the measured spread; holds it to the bar of these VJP kernels (the ceiling of the oracle tests), since
    reordering n terms moves a float32 sum by up to (n - 1) 2^-24 sum|terms| and no bound of a few units in the last place holds by construction."""
    c = _case(64, 112)
    first, second = _backward_twice(dev, model, c, c["gv"], c["gj"])
    for k in first:
        S = float(first[k].abs().max())
        print(f"[smpl-vjp] run-twice spread, dense cotangent, {k}: {float((first[k] - second[k]).abs().max()) / S:.3g} of max|grad|")
        np.testing.assert_allclose(second[k].numpy(), first[k].numpy(), atol=VJP_ATOL_REL * S, rtol=VJP_RTOL, err_msg=k)


# ------------------------------------------------------------------------------------------------ part 2: no behaviour change
def test_forward_without_grad_is_the_plain_kernel_call(dev, model):
    from egohmr_amd import _lib
    B = 33
    c = {k: v.to(dev) for k, v in _case(B, 101).items()}
    verts, joints = torch.empty(B, 6890, 3, device=dev), torch.empty(B, 45, 3, device=dev)
    _lib.api().ehm_smpl_forward(model.smpl.handle(), c["betas"], c["R"], verts, joints, None, B, _lib.stream_ptr())
    kw = dict(body_pose=c["R"][:, 1:], global_orient=c["R"][:, :1], pose2rot=False)
    with torch.enable_grad():
        o = model.smpl(betas=c["betas"], **kw)                                   # gradients enabled, nothing requires grad
    assert not o.vertices.requires_grad and torch.equal(o.vertices, verts) and torch.equal(o.joints, joints)
    with torch.no_grad():
        o = model.smpl(betas=c["betas"].clone().requires_grad_(), **kw)          # requires grad, gradients disabled
    assert not o.vertices.requires_grad and torch.equal(o.vertices, verts) and torch.equal(o.joints, joints)
    o = model.smpl(betas=c["betas"].clone().requires_grad_(), **kw)              # the differentiable route computes the same bits
    assert o.vertices.requires_grad and torch.equal(o.vertices.detach(), verts) and torch.equal(o.joints.detach(), joints)


def guide_case(dev, model):
    """The seeded case behind tests/golden/g13_parent_guide_coll.npz: guide_coll ('x_t', 'x_0') and eval_coll of the build's proxy route."""
    from egohmr_amd.factory import batch_to_device
    B, N = 4, 2048
    bnp = syn.make_batch(B, N, seed=61)
    bnp["scene_pcd_verts_full"][:, : N // 3, 1] = bnp["smpl_params"]["transl"][:, None, 1] - 0.6
    gb = batch_to_device(bnp, dev)
    gb["x_t"] = (torch.from_numpy(syn.make_noise_stack(0, B, seed=61)[0]) * 0.5).to(dev)
    t = torch.full((B,), 3, dtype=torch.long, device=dev)
    go = model(gb, t)
    return gb, go, t


def guide_case_outputs(dev, model):
    gb, go, t = guide_case(dev, model)
    return {"grad_x_t": model.guide_coll(gb, go, t, compute_grad="x_t").cpu().numpy(),
            "grad_x_0": model.guide_coll(gb, go, t, compute_grad="x_0").cpu().numpy(),
            "coll": np.asarray(model.eval_coll(go), dtype=np.float64)}


def sparse_guide_case_outputs(dev, model):
    """The seeded case behind tests/golden/g14_parent_guide_coll_sparse.npz: guide_coll ('x_t', 'x_0') and eval_coll of the build's proxy route on a
    scene whose result is DEFINED bit for bit.  The route accumulates with float atomics (skin_bwd_kernel's gA, the collision search's loss and vertex
    gradient), so a sum of three or more terms depends on the launch's scheduling; a sum of at most two does not (0 + a + b = 0 + b + a).  Here every item
    has exactly two scene points near its body - one by a left-foot vertex, one by a right-foot vertex, 2 cm towards the centroid (so inside the
    bounding box and under tau = 5 cm) - and every other point far away: two hit points, at most two terms in every accumulator.  The feet hang below
    the leg joints that the guidance keeps (1, 2, 4, 5, 7, 8, 10, 11), so the gradient is not zero."""
    from egohmr_amd.geometry import rot6d_to_rotmat
    gb, go, t = guide_case(dev, model)
    st = model.fused_sampler.prepare(gb)
    assert model.fused_sampler.prepare(gb) is st                           # the cached conditioning of this batch: guide_coll reads its scene
    mean, std = model._std_mean()
    betas = go["pred_smpl_params"]["betas"]
    owner = model.smpl.lbs_weights.argmax(1)
    picks = [int(torch.nonzero(owner == j)[0]) for j in (10, 11)]          # first vertex owned by the left / right foot joint
    dense, out = st.scene, {}
    B = dense.shape[0]
    try:
        for mode, x in (("x_t", gb["x_t"]), ("x_0", go["pred_x_start"])):
            with torch.no_grad():
                R = rot6d_to_rotmat((x * std + mean).reshape(-1, 6), "diffusion").view(B, 24, 3, 3)
                verts = model.smpl(betas=betas, body_pose=R[:, 1:], global_orient=R[:, [0]], pose2rot=False).vertices
            scene = torch.full_like(dense, 50.0)
            centre = verts.mean(1)
            for k, vid in enumerate(picks):
                d = centre - verts[:, vid]
                scene[:, k] = verts[:, vid] + 0.02 * d / d.norm(dim=1, keepdim=True)
            st.scene = model.scene_pcd_verts = scene.contiguous()
            out["grad_" + mode] = model.guide_coll(gb, go, t, compute_grad=mode).cpu().numpy()
            if mode == "x_0":
                out["coll"] = np.asarray(model.eval_coll(go), dtype=np.float64)
    finally:
        st.scene = model.scene_pcd_verts = dense
    return out


def _parent_diffs(golden_dir, name, out):
    g = np.load(os.path.join(golden_dir, name))
    for k in ("grad_x_t", "grad_x_0", "coll"):
        print(f"[parent] {name} {k}: max|diff| {np.abs(out[k] - g[k]).max():.3g} of max {np.abs(g[k]).max():.3g}")
    assert float(np.abs(g["grad_x_t"]).max()) > 0 and float(np.abs(g["grad_x_0"]).max()) > 0 and float(g["coll"].max()) > 0
    return g


def test_proxy_route_is_bit_equal_to_the_parent(golden_dir, dev, model):
    """collision_model = None: guide_coll ('x_t' and 'x_0') and eval_coll give the bits the parent commit gave, checked against tensors dumped from a
    parent build on the same seeded inputs (g14; sparse_guide_case_outputs says why that scene has two hit points per item)."""
    assert model.collision_model is None
    out = sparse_guide_case_outputs(dev, model)
    g = _parent_diffs(golden_dir, "g14_parent_guide_coll_sparse.npz", out)
    assert np.count_nonzero(g["coll"]) == len(g["coll"])                   # every item is hit
    for k in ("grad_x_t", "grad_x_0", "coll"):
        assert np.array_equal(out[k], g[k]), k


def test_proxy_route_on_a_dense_scene_vs_the_parent(golden_dir, dev, model):
    """The same against the parent's dump of the DENSE scene of test_guide_coll_vs_oracle (g13: ~700 scene points in the body's box).  eval_coll
    counts in integers and is bit-equal.  The gradient there is a float-atomic sum of hundreds of terms and is not defined to the last bit on any
    build: the PARENT build differs from itself by 1.5e-8 .. 5.2e-8 between two calls of one process and by 1.5e-8 / 2.3e-8 between two processes
    (max|grad| 0.145; MI355X), this build from the parent's dump by 1.7e-8 .. 6.6e-8: the same last-bit noise.  Reordering a float32 sum of n terms moves
    it by up to (n - 1) 2^-24 sum|terms|, with n up to the 6890 vertices of a joint's accumulator, so no bound of a few units in the last place holds by
    construction; the gradient is held to the project's bar for these VJP kernels (tests/test_gpu_guidance.py: atol = 2e-4 max|ref|, rtol = 2e-3), the
    zeroed joints stay exactly zero, and the bit-equality itself is asserted on the sparse scene above."""
    assert model.collision_model is None
    out = guide_case_outputs(dev, model)
    again = guide_case_outputs(dev, model)
    for k in ("grad_x_t", "grad_x_0"):                                     # this build against itself: the spread the prose above speaks of, measured here
        print(f"[parent] {k}: two calls of this build differ by {np.abs(out[k] - again[k]).max():.3g} of max {np.abs(out[k]).max():.3g}")
    g = _parent_diffs(golden_dir, "g13_parent_guide_coll.npz", out)
    assert np.array_equal(out["coll"], g["coll"])
    for k in ("grad_x_t", "grad_x_0"):
        assert float(np.abs(out[k].reshape(-1, 24, 6)[:, ZERO_JOINTS]).max()) == 0.0, k
        np.testing.assert_allclose(out[k], g[k], atol=VJP_ATOL_REL * float(np.abs(g[k]).max()), rtol=VJP_RTOL, err_msg=k)


# ------------------------------------------------------------------------------------------------ part 3: the plug-in route
def _proxy_min_dist(points, verts):
    """oracle.collision.proxy_min_dist on whatever device the inputs are."""
    out = []
    for s in range(0, points.shape[0], 1024):
        diff = points[s:s + 1024, None, :] - verts[None, :, :]
        out.append(torch.sqrt((diff * diff).sum(-1).min(dim=1).values + 1e-12))
    return torch.cat(out) if out else points.new_zeros(0)


def _proxy_loss(points, verts, tau):
    """oracle.collision.proxy_collision_loss, device-clean: points [1,n,3], verts [1,V,3] -> scalar; the gradient goes to the arg-min vertex."""
    return (torch.relu(tau - _proxy_min_dist(points[0], verts[0])) ** 2).sum()


class ProxyAdapter:
    """The build's proxy behind the two calls the reference makes on `self.smpl.coap`, in plain differentiable torch; counts its calls."""

    def __init__(self, tau):
        self.tau, self.loss_calls, self.query_calls = float(tau), 0, 0

    def collision_loss(self, points, smpl_output, ret_collision_mask=None):
        assert ret_collision_mask is None and points.dim() == 3 and points.shape[0] == 1 and points.shape[1] > 0
        assert smpl_output.vertices.shape[0] == 1 and smpl_output.joints.shape == (1, 45, 3) and smpl_output.full_pose.shape == (1, 72)
        self.loss_calls += 1
        return _proxy_loss(points, smpl_output.vertices, self.tau)

    def query(self, points, smpl_output):
        assert points.shape[0] == 1 and smpl_output.full_pose.shape == (1, 72)
        self.query_calls += 1
        return (_proxy_min_dist(points[0], smpl_output.vertices[0]) < self.tau).float().unsqueeze(0)


class BatchedProxyAdapter(ProxyAdapter):
    """The VolumetricSMPL-shaped calls: collision_loss(points [B,N,3], smpl_output of B bodies) -> [B]; query_fast -> signed distance."""

    def collision_loss(self, points, smpl_output, ret_collision_mask=None):
        B = points.shape[0]
        assert smpl_output.vertices.shape[0] == B and smpl_output.full_pose.shape == (B, 72)
        self.loss_calls += 1
        return torch.stack([_proxy_loss(points[[b]], smpl_output.vertices[[b]], self.tau) for b in range(B)])

    def query_fast(self, points, smpl_output):
        self.query_calls += 1
        return (_proxy_min_dist(points[0], smpl_output.vertices[0]) - self.tau).unsqueeze(0)


ZERO_JOINTS = [0, 3, 6, 9] + list(range(12, 24))


def test_plugged_guide_coll_vs_oracle_and_proxy_route(dev, model, plugged, synth_weights, smpl_asset):
    """The autograd route (adapter) against EgoHMROracle.guide_coll with the tolerance of test_guide_coll_vs_oracle, and against the built-in proxy
    route: two independent implementations of one function."""
    from oracle import model as om
    from oracle.collision import proxy_collision_loss
    B, N = 4, 2048
    bnp = syn.make_batch(B, N, seed=61)
    bnp["scene_pcd_verts_full"][:, : N // 3, 1] = bnp["smpl_params"]["transl"][:, None, 1] - 0.6
    mean, std = syn.make_body_rep_stats(0)
    ref = om.EgoHMROracle(synth_weights, smpl_asset, mean, std, faithful=False, collision_loss=proxy_collision_loss)
    tb = {k: ({kk: torch.from_numpy(vv) for kk, vv in v.items()} if isinstance(v, dict) else torch.from_numpy(v)) for k, v in bnp.items()}
    tb["x_t"] = torch.from_numpy(syn.make_noise_stack(0, B, seed=61)[0]) * 0.5
    tc = torch.full((B,), 3, dtype=torch.long)
    ro = ref(tb, tc)
    gb, go, t = guide_case(dev, model)
    for mode in ("x_t", "x_0"):
        g_ref, _ = ref.guide_coll(tb, ro, tc, compute_grad=mode)
        scale = float(g_ref.abs().max())
        assert scale > 0
        calls = plugged.collision_model.loss_calls
        g = plugged.guide_coll(gb, go, t, compute_grad=mode)
        assert g.shape == (B, 144) and 0 < plugged.collision_model.loss_calls - calls <= B
        plugged.collision_model, adapter = None, plugged.collision_model
        g_proxy = model.guide_coll(gb, go, t, compute_grad=mode)
        plugged.collision_model = adapter
        print(f"[plug-in] guide_coll {mode}: vs oracle {float((g.cpu() - g_ref).abs().max()) / scale:.3g}, vs proxy route {float((g - g_proxy).abs().max()) / scale:.3g} of max|ref|")
        np.testing.assert_allclose(g.cpu().numpy(), g_ref.numpy(), atol=2e-3 * scale, rtol=5e-3)
        np.testing.assert_allclose(g.cpu().numpy(), g_proxy.cpu().numpy(), atol=2e-3 * scale, rtol=5e-3)
        assert float(g.reshape(B, 24, 6)[:, ZERO_JOINTS].abs().max()) == 0.0
    # guide_denom_override replaces the denominator of `-loss.mean()` as on the proxy route
    g = plugged.guide_coll(gb, go, t)
    plugged.guide_denom_override = 2 * B
    g2 = plugged.guide_coll(gb, go, t)
    np.testing.assert_allclose(g2.cpu().numpy() * 2, g.cpu().numpy(), rtol=1e-5, atol=1e-6 * float(g.abs().max()))


def _count_nonempty(model, records):
    """Independent of the route under test: the items of every recorded guided step whose vertex bounding box holds a scene point."""
    from egohmr_amd.geometry import rot6d_to_rotmat
    mean, std = model._std_mean()
    n = 0
    with torch.no_grad():
        for x, betas in records:
            B = x.shape[0]
            R = rot6d_to_rotmat((x * std + mean).reshape(-1, 6), "diffusion").view(B, 24, 3, 3)
            v = model.smpl(betas=betas, body_pose=R[:, 1:], global_orient=R[:, [0]], pose2rot=False).vertices
            sc = model.scene_pcd_verts
            inside = ((sc >= v.min(1, keepdim=True).values) & (sc <= v.max(1, keepdim=True).values)).all(-1)
            n += int(inside.any(1).sum())
    return n


def _golden_run(golden_dir, dev, model, name, respacing_key):
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device
    g = np.load(os.path.join(golden_dir, name))
    B, N, n = int(g["B"]), int(g["N"]), int(g["n"])
    rs = str(g[respacing_key]) if respacing_key else ""
    d = create_gaussian_diffusion(num_diffusion_timesteps=n, timestep_respacing=rs)
    bnp = syn.make_batch(B, num_scene_points=N, seed=int(g["batch_seed"]))
    bnp["scene_pcd_verts_full"][:, : N // 3, 1] = bnp["smpl_params"]["transl"][:, None, 1] - 0.6
    b = batch_to_device(bnp, dev)
    noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B, seed=int(g["noise_seed"]))).to(dev)
    records, inner = [], model.guide_coll

    def recording(batch, output, t, compute_grad="x_t"):
        records.append((batch["x_t"].detach().clone(), output["pred_smpl_params"]["betas"].detach().clone()))
        return inner(batch, output, t, compute_grad=compute_grad)
    model.guide_coll = recording
    try:
        kw = dict(cond_grad_weight=float(g["cond_grad_weight"])) if not rs else {}
        o = d.val_losses(model, b, shape=[B, 144], clip_denoised=False, timestep_respacing=rs, compute_loss=False, cond_fn_with_grad=True,
                         noise_stack=noise, **kw)
    finally:
        del model.guide_coll
    c = lambda t: t.detach().cpu().numpy()
    for k, got in (("pred_x_start", c(o["pred_x_start"])), ("verts_head", c(o["pred_vertices"][:, :64])), ("joints", c(o["pred_keypoints_3d"]))):
        print(f"[plug-in] {name} {k}: max|diff| {np.abs(got - g[k]).max():.3g}")
    np.testing.assert_allclose(c(o["pred_x_start"]), g["pred_x_start"], atol=2e-4)
    np.testing.assert_allclose(c(o["pred_vertices"][:, :64]), g["verts_head"], atol=1e-4)
    np.testing.assert_allclose(c(o["pred_keypoints_3d"]), g["joints"], atol=1e-4)
    return B, records


def test_plugged_guided_ddpm_vs_reference_golden(golden_dir, dev, plugged):
    """val_losses(cond_fn_with_grad=True) with the adapter attached takes the per-step route (allow_fused untouched) and meets the bounds of
    test_guided_ddpm_vs_reference_golden[generic] on the reference's own run g9; every guided step went through the adapter and autograd:
    11 guided steps x the items whose box is not empty."""
    B, records = _golden_run(golden_dir, dev, plugged, "g9_e2e_ddpm50_guided.npz", None)
    assert len(records) == 11
    expect = _count_nonempty(plugged, records)
    print(f"[plug-in] g9: {plugged.collision_model.loss_calls} adapter calls, {expect} non-empty boxes in 11 guided steps of {B} items")
    assert 0 < expect <= 11 * B and plugged.collision_model.loss_calls == expect


def test_plugged_guided_ddim_vs_reference_golden(golden_dir, dev, plugged):
    """The same for ddim_sample_with_grad (golden g12): the last four respaced steps are guided."""
    B, records = _golden_run(golden_dir, dev, plugged, "g12_e2e_ddim10_guided.npz", "respacing")
    assert len(records) == 4
    expect = _count_nonempty(plugged, records)
    print(f"[plug-in] g12: {plugged.collision_model.loss_calls} adapter calls, {expect} non-empty boxes in 4 guided steps of {B} items")
    assert 0 < expect <= 4 * B and plugged.collision_model.loss_calls == expect


def test_plugged_eval_coll_and_penetration_term(dev, model, plugged):
    gb, go, t = guide_case(dev, model)
    adapter, plugged.collision_model = plugged.collision_model, None
    share_proxy = model.eval_coll(go)
    pen_proxy = model._penetration_term()
    plugged.collision_model = adapter
    share = plugged.eval_coll(go)
    pen = plugged._penetration_term()
    print(f"[plug-in] eval_coll adapter {share} proxy {share_proxy}; penetration adapter {pen.tolist()} proxy {pen_proxy.tolist()}")
    assert max(share_proxy) > 0 and 0 < adapter.query_calls <= len(share)
    assert share == share_proxy
    np.testing.assert_allclose(pen.cpu().numpy(), pen_proxy.cpu().numpy(), rtol=2e-4, atol=1e-7)      # the bar of test_collision_proxy_vs_oracle for the loss
    # the 4000-point cap of egohmr.py:411-412: points of INDEX >= cap are dropped once more than cap are selected
    item = type("O", (), {"vertices": torch.tensor([[[0.0, 0, 0], [1, 1, 1]]], device=dev)})()
    scene = torch.full((1, 50, 3), 0.5, device=dev)
    scene[0, ::5] = 7.0                                                                                  # 40 of the 50 points are inside the box
    assert plugged._bbox_points(item, scene).shape == (1, 40, 3)
    assert plugged._bbox_points(item, scene.clone(), cap=20).shape == (1, 16, 3)                         # indices 0..19, of which 16 are inside
    assert plugged._bbox_points(item, scene + 10.0) is None


def test_plugged_compute_loss_penetration_term(golden_dir, dev, synth_weights, smpl_asset):
    """EgoHMR.compute_loss with a collision model attached: the penetration term of case b of the validation-loss goldens (item 0 selects more than 4000
    points and loses those of index >= 4000, item 1 selects nothing) through the adapter's collision_loss, against the float64 restatement on the
    product's own vertices at the bar of test_penetration_term_against_float64 (1e-5 relative), and against the proxy route."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import val_losses_ref as R
    from egohmr_amd.factory import batch_to_device, build_synthetic_model
    g = np.load(os.path.join(golden_dir, "g21_val_losses_b.npz"))
    B = int(g["B"])
    m = build_synthetic_model(dev, 0, diffuse_fuse=True, state_dict=synth_weights, smpl_asset=smpl_asset, smpl_asset_male=syn.make_smpl_asset(1),
                              smpl_asset_female=syn.make_smpl_asset(2), start_coap_epoch=R.START_COAP_EPOCH, **R.CASE_WEIGHTS)
    b_np, flags = R.golden_batch(g)
    batch = batch_to_device(b_np, dev)
    batch["smpl_params_is_axis_angle"] = flags
    batch["x_t"] = torch.from_numpy(g["x_t"]).to(dev)
    out = m(batch, torch.full((B,), int(g["timestep"]), device=dev, dtype=torch.long))
    m.compute_loss(batch, out, cur_epoch=R.START_COAP_EPOCH)
    proxy = out["losses_per_item"]["loss_coap_penetration"].cpu().numpy().copy()
    m.collision_model = ProxyAdapter(m.collision_tau)
    m.compute_loss(batch, out, cur_epoch=R.START_COAP_EPOCH)
    got = out["losses_per_item"]["loss_coap_penetration"].cpu().numpy()
    term, n_sel, _ = R.penetration_f64(m.smpl_output.vertices.cpu().numpy(), m.scene_pcd_verts.cpu().numpy())
    print(f"[plug-in] compute_loss penetration per item: adapter {got.tolist()} proxy {proxy.tolist()} float64 {term.tolist()}")
    assert m.collision_model.loss_calls == int((n_sel > 0).sum()) and n_sel.max() > 4000 and got[1] == 0.0
    np.testing.assert_allclose(got, term, rtol=1e-5, atol=0)
    np.testing.assert_allclose(got, proxy, rtol=1e-5, atol=0)
    assert float(out["losses"]["loss_coap_penetration"]) > 0
    # before the start epoch the model is not asked
    calls = m.collision_model.loss_calls
    m.compute_loss(batch, out, cur_epoch=R.START_COAP_EPOCH - 1)
    assert m.collision_model.loss_calls == calls


def test_plugged_volsmpl_matches_its_proxy_route(dev, synth_weights, smpl_asset):
    """EgoHMRVolsmpl: ONE batched collision_loss(scene, smpl_output) over all points, -loss.sum(); eval_coll_volsmpl through an sdf < 0 query."""
    from egohmr_amd.factory import build_synthetic_model
    m = build_synthetic_model(dev, 0, diffuse_fuse=True, state_dict=synth_weights, smpl_asset=smpl_asset, volsmpl=True)
    gb, go, t = guide_case(dev, m)
    g_proxy, share_proxy = m.guide_coll(gb, go, t), m.eval_coll_volsmpl(go)
    m.collision_model = BatchedProxyAdapter(m.collision_tau)
    g, share = m.guide_coll(gb, go, t), m.eval_coll_volsmpl(go)
    scale = float(g_proxy.abs().max())
    print(f"[plug-in] volsmpl guide_coll vs proxy route {float((g - g_proxy).abs().max()) / scale:.3g} of max|ref|; shares {share} {share_proxy}")
    assert scale > 0 and m.collision_model.loss_calls == 1
    np.testing.assert_allclose(g.cpu().numpy(), g_proxy.cpu().numpy(), atol=2e-3 * scale, rtol=5e-3)
    assert float(g.reshape(-1, 24, 6)[:, ZERO_JOINTS].abs().max()) == 0.0
    assert share == share_proxy and max(share) > 0


def test_fused_run_refuses_a_guided_loop_with_a_collision_model(golden_dir, dev, plugged):
    from egohmr_amd import _lib
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device
    d = create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="")
    b = batch_to_device(syn.make_batch(2, num_scene_points=512, seed=5), dev)
    noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, 2, seed=6)).to(dev)
    with pytest.raises(_lib.EgoHMRHipError, match="collision_model"):
        plugged.fused_sampler.run(d, b, noise, ddim=False, guided=True)
    r = plugged.fused_sampler.run(d, b, noise, ddim=False, guided=False)                                # unguided loops stay fused
    assert torch.isfinite(r["sample"]).all() and plugged.collision_model.loss_calls == 0
