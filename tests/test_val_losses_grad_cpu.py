"""CPU: the gradient reference of the loss VJP (tests/val_losses_grad_ref.py) is pinned to the value reference that the g21 goldens pin
(tests/val_losses_ref.py); ehm_val_losses_backward and its workspace query are bound and refuse bad arguments before any device call; the autograd
route of EgoHMR.compute_loss refuses a double backward and CPU tensors."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import val_losses_grad_ref as G  # noqa: E402
import val_losses_ref as R  # noqa: E402

WEIGHTS = [R.CASE_WEIGHTS[k] for k in R.WEIGHT_NAMES]


@pytest.mark.parametrize("B,V,seed,genders", [(1, 1, 11, "mixed"), (5, 7, 13, "male"), (3, 1366, 14, "female"), (4, 1023, 16, "mixed")])
def test_torch_restatement_equals_the_value_reference(B, V, seed, genders):
    inp = R.random_kernel_inputs(B, V, seed, genders)
    pen = np.random.default_rng(seed + 1).uniform(0.0, 2.0, size=B)
    for p in (None, pen):
        ref = R.val_losses_f64(inp, WEIGHTS, p)["losses"]
        got = G.val_losses_torch64(G.as_f64(inp), WEIGHTS, None if p is None else torch.from_numpy(p))
        assert list(got) == list(R.LOSS_KEYS)
        for k in R.LOSS_KEYS:
            d = abs(float(got[k]) - ref[k]) / abs(ref[k]) if ref[k] != 0 else abs(float(got[k]))
            print(f"B={B} V={V} {k}: numpy {ref[k]:.17g} torch {float(got[k]):.17g} relative deviation {d:.3e}")
            assert d <= 1e-12, (k, d)


def test_gradient_reference_against_central_differences():
    """torch.autograd on the restatement is the reference of the GPU tests: its gradient of a smooth term and of an L1 term away from its kink equals a
    central difference of the restatement's own value (float64, step h = 1e-6: no truncation error for the L1 and quadratic terms, ~h^2 for the quartic one;
    what remains is the rounding of the two loss values, a few 2^-53 |loss| each, divided by 2 h)."""
    inp = R.random_kernel_inputs(2, 7, 12, "mixed")
    g = G.val_losses_grads64(inp, WEIGHTS, gloss=0.37)
    for name, idx in (("pred_betas", (1, 3)), ("pred_pose_6d", (0, 17)), ("pred_vertices", (1, 4, 2)), ("pred_keypoints_3d", (1, 0, 1)),
                      ("pred_keypoints_2d_full", (0, 24, 0))):
        vals = []
        for s in (1e-6, -1e-6):
            t = G.as_f64(inp)
            t[name][idx] += s
            vals.append(0.37 * float(G.val_losses_torch64(t, WEIGHTS)["loss"]))
        fd = (vals[0] - vals[1]) / 2e-6
        bound = 16 * 2.0 ** -53 * max(abs(v) for v in vals) / 2e-6 + 1e-9 * abs(fd)
        assert abs(fd - g[name][idx]) <= bound, (name, fd, g[name][idx], bound)


# ---------------------------------------------------------------------------------------------- the C entry points
def _dummy_desc(**kw):
    """An ehm_val_losses_bwd_desc that passes every check, on dummy (never dereferenced) addresses; each use breaks one rule, so no call reaches a launch."""
    from egohmr_amd import _lib
    f = dict(B=4, V=6890, pred_joints=45, gt_joints=45, kp3d_points=24, kp3d_full_points=24, kp2d_points=25, workspace_bytes=1 << 20)
    for i, (name, typ) in enumerate(_lib.ValLossesBwdDesc._fields_):
        if typ is ctypes.c_void_p:
            f[name] = 0x100000 * (i + 1)
    f.update(kw)
    return _lib.ValLossesBwdDesc(**f)


def test_backward_is_bound_and_rejects_bad_arguments_without_a_gpu():
    from egohmr_amd import _lib
    _lib.build()
    L, A = _lib.lib(), _lib.api()
    header = open(os.path.join(_lib.INCLUDE, "egohmr_hip.h")).read()
    for name in ("ehm_val_losses_backward", "ehm_val_losses_backward_workspace_bytes"):
        assert name + "(" in header and name in _lib.PROTOTYPES and name not in _lib.VALUE_FUNCTIONS and hasattr(L, name) and hasattr(A, name)
    assert "ehm_val_losses_bwd_desc" in header

    def refused(call_raw, call_checked, name):
        assert call_raw() == -22 and b"bad argument" in L.ehm_last_error()
        with pytest.raises(_lib.EgoHMRHipError, match=name) as e:
            call_checked()
        assert e.value.rc == -22 and e.value.function == name

    refused(lambda: L.ehm_val_losses_backward(None, None), lambda: A.ehm_val_losses_backward(None, None), "ehm_val_losses_backward")      # null descriptor
    inputs = [n for n in _lib.ValLossesBwdDesc.INPUTS if n not in ("focal", "center")]
    assert len(inputs) == 19
    bad = [dict(B=0), dict(B=-3), dict(V=0), dict(pred_joints=44), dict(gt_joints=23), dict(kp3d_points=23), dict(kp3d_full_points=23), dict(kp2d_points=24),
           dict(workspace_bytes=8), dict(workspace_bytes=4 * 6 * 16 - 1), dict(workspace=None), dict(workspace=0x100002),
           dict(g_pred_vertices=0x100004), dict(pred_vertices=0x100004), dict(gt_vertices_male=0x100008), dict(gt_vertices_female=0x10000c)]
    bad += [{n: None} for n in inputs]                                                                                                   # a missing input
    for kw in bad:
        d = _dummy_desc(**kw)
        refused(lambda: L.ehm_val_losses_backward(ctypes.byref(d), None), lambda: A.ehm_val_losses_backward(ctypes.byref(d), None), "ehm_val_losses_backward")
    nb = ctypes.c_int64(-1)
    for args in ((0, 6890, ctypes.byref(nb)), (4, 0, ctypes.byref(nb)), (4, 6890, None)):
        refused(lambda: L.ehm_val_losses_backward_workspace_bytes(*args), lambda: A.ehm_val_losses_backward_workspace_bytes(*args),
                "ehm_val_losses_backward_workspace_bytes")
    assert nb.value == -1
    # one 16-byte slot (three integer sign sums + the NaN flags) per block of 4096 floats of an item: 6 blocks per 6890-vertex body
    assert L.ehm_val_losses_backward_workspace_bytes(256, 6890, ctypes.byref(nb)) == 0 and nb.value == 256 * 6 * 16
    assert L.ehm_val_losses_backward_workspace_bytes(3, 37, ctypes.byref(nb)) == 0 and nb.value == 3 * 16
    assert ctypes.sizeof(_lib.ValLossesBwdDesc) == 7 * 4 + 4 + 22 * 8 + 9 * 8 + 8 + 8 + 9 * 8            # the header's layout (one int of padding)


# ---------------------------------------------------------------------------------------------- the autograd route
def _cpu_inputs(B=2, V=7):
    inp = R.random_kernel_inputs(B, V, 12)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in inp.items()}
    return {k: v for k, v in t.items() if k not in G.PREDICTIONS}, [t[k].clone().requires_grad_() for k in G.PREDICTIONS]


def test_double_backward_raises(monkeypatch):
    """The Function's backward is once_differentiable: differentiating its gradient raises.  The two native calls are replaced by stand-ins here (there is no
    GPU): what is tested is the Function's own wiring - which outputs carry a graph, what the backward hands back, the refusal of a second derivative."""
    from egohmr_amd import loss_grad, model

    def fake_forward(t, weights, penetration=None):
        B = t["pred_vertices"].shape[0]
        return dict(losses=torch.arange(11.0), joint_vis_num=torch.zeros(1, dtype=torch.int64), per_item=torch.zeros(B, 11),
                    per_item_vis=torch.zeros(B, dtype=torch.int64), vis_mask=torch.zeros(B, 24, dtype=torch.uint8))

    def fake_backward(t, weights, gloss=None, want=(), out=None):
        return {k: torch.full((t["pred_vertices"].shape[0],), 2.0) if k == "penetration" else torch.full_like(t[k], 3.0) for k in want}

    monkeypatch.setattr(model, "val_losses_native", fake_forward)
    monkeypatch.setattr(loss_grad, "val_losses_grad_native", fake_backward)
    consts, preds = _cpu_inputs()
    preds[2] = preds[2].detach()                                            # one prediction without grad: its gradient is not asked for
    pen = torch.zeros(2, requires_grad=True)
    outs = loss_grad.ValLossesFunction.apply(consts, WEIGHTS, pen, *preds)
    loss = outs[0]
    assert loss.grad_fn is not None and loss.shape == () and all(not o.requires_grad for o in outs[1:])
    asked = [p for p in preds if p.requires_grad] + [pen]
    grads = torch.autograd.grad([loss * loss], asked, create_graph=True)          # (the cotangent 2 loss is itself in the graph: a second derivative exists)
    assert all(float(g.detach().reshape(-1)[0]) == 3.0 for g in grads[:-1]) and float(grads[-1].detach()[0]) == 2.0
    assert all(g.shape == p.shape for g, p in zip(grads, asked))
    with pytest.raises(RuntimeError, match="once_differentiable"):
        grads[0].sum().backward()


def test_cpu_tensors_on_the_autograd_route_raise_the_package_error():
    from egohmr_amd import _lib, loss_grad
    _lib.build()
    consts, preds = _cpu_inputs()
    with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):
        loss_grad.ValLossesFunction.apply(consts, WEIGHTS, None, *preds)
    t = dict(consts, **dict(zip(G.PREDICTIONS, [p.detach() for p in preds])))
    with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):
        loss_grad.val_losses_grad_native(t, WEIGHTS)


def test_route_choice_without_a_device():
    from egohmr_amd.factory import build_synthetic_model
    m = build_synthetic_model("cpu", 0, **R.CASE_WEIGHTS, start_coap_epoch=R.START_COAP_EPOCH)
    z = lambda *s: torch.zeros(*s)
    out = dict(pred_vertices=z(2, 7, 3), pred_keypoints_3d=z(2, 45, 3), pred_keypoints_3d_full=z(2, 45, 3), pred_keypoints_2d_full=z(2, 45, 2),
               pred_pose_6d=z(2, 144), pred_smpl_params=dict(global_orient=z(2, 1, 3, 3), body_pose=z(2, 23, 3, 3), betas=z(2, 10)))
    assert not m._loss_wants_grad(out, False) and not m._loss_wants_grad(out, True)
    for k in ("pred_vertices", "pred_keypoints_3d", "pred_keypoints_3d_full", "pred_keypoints_2d_full", "pred_pose_6d"):
        o = dict(out, **{k: out[k].clone().requires_grad_()})
        assert m._loss_wants_grad(o, False)
        with torch.no_grad():
            assert not m._loss_wants_grad(o, False)
    for k in ("global_orient", "body_pose", "betas"):
        assert m._loss_wants_grad(dict(out, pred_smpl_params=dict(out["pred_smpl_params"], **{k: z(2, 10).requires_grad_()})), False)
    from egohmr_amd.smpl import SMPLOutput
    m.smpl_output = SMPLOutput(vertices=z(2, 7, 3).requires_grad_())
    assert m._loss_wants_grad(out, True) and not m._loss_wants_grad(out, False)        # the bodies count only while the penetration term is active
    with pytest.raises(NotImplementedError, match="compute_loss has a backward"):
        m.training_step()
    from egohmr_amd.diffusion import create_gaussian_diffusion
    with pytest.raises(NotImplementedError, match="compute_loss has a backward"):
        create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="").training_losses(m, {}, torch.zeros(2, dtype=torch.long))
