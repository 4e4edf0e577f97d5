"""GPU: the validation losses of EgoHMR.compute_loss on the device (csrc/loss.hip, ehm_val_losses) against the float64 restatement of
tests/val_losses_ref.py on identical inputs, their reproducibility and NaN rule, and end to end against the reference's own results
(tests/golden/g21_val_losses_*.npz).  Every test here fails without the feature (compute_loss used to return an empty dict)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import val_losses_ref as R  # noqa: E402
from egohmr_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

# One float32 rounding of a float64 sum.  Derived, not measured: the kernel accumulates in float64 (order error <= n 2^-53, 5e-10 at n = 5.3 M), every term is
# a sum of non-negative values and the weights are non-negative, so nothing cancels; `loss` is formed from the float64 sums and rounded once.
KERNEL_RTOL = 2.0 ** -23
# driver.validate adds three such float32 scalars on the device and divides once: three more float32 roundings of 2^-24 each, bounded by 2^-22 in all
VALIDATE_RTOL = 2.0 ** -22

# End to end against the reference (test 7): largest relative deviation per key over cases a, b (both epochs), c, measured on an MI355X (the values below);
# the bound is 4 x measured.  What differs: the reference's float32 summation, the two LBS implementations (~1e-6 m), the product's forward against the
# reference's (1-5e-6 m), quaternion aa_to_rotmat against smplx's Rodrigues in the ground-truth decode.  Both numbers of the comparison are float32, so a
# deviation is either 0 or at least one float32 spacing: two keys measured exactly 0, and 4 x 0 would demand bit equality with the reference's float32
# summation on every machine.  The bound therefore never goes below one float32 spacing, 2^-23 relative (the number format's resolution, not a measurement).
MEASURED_E2E_DEVIATION = {
    "loss": 1.264e-07, "loss_v2v": 9.780e-08, "loss_keypoints_3d": 8.631e-08, "loss_keypoints_3d_full": 8.465e-08, "loss_keypoints_2d_full": 0.0,
    "loss_betas": 9.160e-08, "loss_body_pose": 9.844e-08, "loss_global_orient": 6.276e-08, "loss_pose_6d_ortho": 1.059e-07,
    "loss_coap_penetration": 9.067e-08, "loss_keypoints_3d_vis_batch_sum": 0.0}
FLOAT32_SPACING = 2.0 ** -23
E2E_BOUND = {k: max(4 * v, FLOAT32_SPACING) for k, v in MEASURED_E2E_DEVIATION.items()}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _to_dev(inp, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inp.items()}


def _native(inp, weights, pen, dev):
    from egohmr_amd.model import val_losses_native
    res = val_losses_native(_to_dev(inp, dev), weights, None if pen is None else torch.from_numpy(pen).to(dev))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _close(got, ref, rtol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    worst = float((err / np.maximum(np.abs(ref), 1e-300)).max()) if err.size else 0.0
    assert np.all(err <= rtol * np.abs(ref)), f"{what}: relative deviation {worst:.3e} > {rtol:.3e}"
    return worst


def _check_against_restatement(got, ref, rtol=KERNEL_RTOL):
    worst = 0.0
    for i, k in enumerate(R.LOSS_KEYS):
        worst = max(worst, _close(got["losses"][i], ref["losses"][k], rtol, k), _close(got["per_item"][:, i], ref["per_item"][k], rtol, k + " per item"))
    assert np.array_equal(got["vis_mask"].astype(bool), ref["mask"]) and np.array_equal(got["per_item_vis"], ref["per_item_vis"])
    assert int(got["joint_vis_num"][0]) == ref["joint_vis_num"]
    return worst


def _weights(seed):
    return np.random.default_rng(seed).uniform(0.01, 2.0, size=9).tolist()


@pytest.mark.parametrize("genders", ["male", "female", "mixed"])
@pytest.mark.parametrize("V", [6890, 1000, 37])
@pytest.mark.parametrize("B", [1, 5, 256])
def test_kernel_against_float64_on_identical_inputs(dev, B, V, genders):
    seed = 1000 * B + V
    inp = R.random_kernel_inputs(B, V, seed, genders)
    pen = np.random.default_rng(seed + 1).uniform(0.0, 2.0, size=B).astype(np.float32)
    pen[0] = 0.0
    fem = inp["gender"] == 1
    gj = np.where(fem[:, None, None], inp["gt_joints_female"], inp["gt_joints_male"]).astype(np.float64)
    mask, margin = R.visibility(gj, inp["focal"].astype(np.float64), inp["center"].astype(np.float64))
    assert margin.min() > 1e-3                                  # float32 and float64 projections cannot disagree on the mask
    assert (inp["keypoints_2d"][:, :, 2] == 0).any()
    if B > 1:
        assert 0 < mask.sum() < B * 24
    w = _weights(seed)
    ref = R.val_losses_f64(inp, w, pen)
    got = _native(inp, w, pen, dev)
    worst = _check_against_restatement(got, ref)
    print(f"B={B} V={V} {genders}: largest relative deviation {worst:.3e} (bound {KERNEL_RTOL:.3e}), visible joints {ref['joint_vis_num']} of {B * 24}")
    # without the optional penetration array the term is 0
    got0 = _native(inp, w, None, dev)
    _check_against_restatement(got0, R.val_losses_f64(inp, w, None))


def test_only_the_selected_ground_truth_is_read(dev):
    """NaN in the body of the gender an item does NOT have changes nothing."""
    B, V = 5, 1000
    inp = R.random_kernel_inputs(B, V, 77, "mixed")
    w = _weights(77)
    base = _native(inp, w, None, dev)
    poisoned = dict(inp)
    fem = inp["gender"] == 1
    for k_m, k_f in (("gt_vertices_male", "gt_vertices_female"), ("gt_joints_male", "gt_joints_female")):
        m, f = inp[k_m].copy(), inp[k_f].copy()
        m[fem], f[~fem] = np.nan, np.nan
        poisoned[k_m], poisoned[k_f] = m, f
    got = _native(poisoned, w, None, dev)
    for k in base:
        assert np.array_equal(base[k], got[k]), k


def test_two_calls_are_bit_equal(dev):
    B, V = 256, 6890
    inp = R.random_kernel_inputs(B, V, 5, "mixed")
    w = _weights(5)
    pen = np.random.default_rng(6).uniform(0.0, 2.0, size=B).astype(np.float32)
    a, b = _native(inp, w, pen, dev), _native(inp, w, pen, dev)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_nan_rule(dev):
    B, V = 5, 1000
    inp = R.random_kernel_inputs(B, V, 31, "mixed")
    w = _weights(31)
    base = _native(inp, w, None, dev)
    # (1) every predicted array of item 2 NaN: its per-item values NaN (the handed-in penetration term apart), every batch scalar NaN, the others untouched
    bad = {k: (v.copy() if k.startswith("pred_") else v) for k, v in inp.items()}
    for k in bad:
        if k.startswith("pred_"):
            bad[k][2] = np.nan
    got = _native(bad, w, None, dev)
    pen_col = R.LOSS_KEYS.index("loss_coap_penetration")
    cols = [i for i in range(len(R.LOSS_KEYS)) if i != pen_col]
    assert np.isnan(got["per_item"][2, cols]).all() and np.isnan(got["losses"][cols]).all()
    others = [0, 1, 3, 4]
    assert np.array_equal(got["per_item"][others].view(np.uint32), base["per_item"][others].view(np.uint32))
    assert np.array_equal(got["vis_mask"], base["vis_mask"]) and int(got["joint_vis_num"][0]) == int(base["joint_vis_num"][0])
    # (2) a NaN only in an INVISIBLE joint still reaches loss_keypoints_3d_vis_batch_sum: the mask multiplies, it does not select
    invisible = np.argwhere(base["vis_mask"][:, 1:] == 0)
    assert len(invisible) > 0
    b, j = int(invisible[0][0]), int(invisible[0][1]) + 1
    bad = dict(inp, pred_keypoints_3d=inp["pred_keypoints_3d"].copy())
    bad["pred_keypoints_3d"][b, j, 1] = np.nan
    got = _native(bad, w, None, dev)
    vis_col = R.LOSS_KEYS.index("loss_keypoints_3d_vis_batch_sum")
    assert np.isnan(got["per_item"][b, vis_col]) and np.isnan(got["losses"][vis_col])
    # (3) an infinite vertex reaches loss_v2v and loss
    bad = dict(inp, pred_vertices=inp["pred_vertices"].copy())
    bad["pred_vertices"][4, V - 1, 2] = np.inf
    got = _native(bad, w, None, dev)
    assert np.isinf(got["losses"][1]) and np.isinf(got["losses"][0]) and np.isinf(got["per_item"][4, 1]) and np.isfinite(got["losses"][2:]).all()


def test_scene_cap_points(dev):
    """ehm_scene_cap_points: counts inside the box exact; an item over the cap loses its points of INDEX >= cap, every other item keeps all."""
    from egohmr_amd import _lib
    g = np.random.default_rng(3)
    B, V, N, cap = 4, 37, 1000, 100
    verts = g.uniform(-0.5, 0.5, size=(B, V, 3)).astype(np.float32)
    scene = g.uniform(-0.6, 0.6, size=(B, N, 3)).astype(np.float32)
    scene[1] += 5.0                                                      # nothing selected
    scene[2, :200] *= 0.1                                                # more than `cap` selected
    scene[3, :, 0] = np.where(np.arange(N) % 40 == 0, 0.0, 9.0)          # 25 selected, most at an index >= cap: all kept
    scene[3, :, 1:] *= 0.1
    lo, hi = verts.min(1, keepdims=True), verts.max(1, keepdims=True)
    inside = ((scene >= lo) & (scene <= hi)).all(-1)
    n = inside.sum(1)
    assert n[1] == 0 and n[2] > cap and n[0] > cap and 0 < n[3] < cap and inside[3, cap:].any()
    tv, ts = torch.from_numpy(verts).to(dev), torch.from_numpy(scene).to(dev)
    out, count = torch.empty_like(ts), torch.empty(B, device=dev, dtype=torch.int32)
    _lib.api().ehm_scene_cap_points(tv, ts, out, count, B, V, N, cap, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert count.cpu().numpy().tolist() == n.tolist()
    out = out.cpu().numpy()
    for b in range(B):
        if n[b] > cap:
            assert np.array_equal(out[b, :cap], scene[b, :cap]) and not ((out[b, cap:] >= lo[b]) & (out[b, cap:] <= hi[b])).all(-1).any()
        else:
            assert np.array_equal(out[b], scene[b])


# ------------------------------------------------------------------------------------------------ end to end
def _golden_model(dev, synth_weights, smpl_asset, volsmpl):
    from egohmr_amd.factory import build_synthetic_model
    return build_synthetic_model(dev, 0, diffuse_fuse=True, state_dict=synth_weights, smpl_asset=smpl_asset, volsmpl=volsmpl,
                                 smpl_asset_male=syn.make_smpl_asset(1), smpl_asset_female=syn.make_smpl_asset(2),
                                 start_coap_epoch=R.START_COAP_EPOCH, **R.CASE_WEIGHTS)


def _golden_batch(g, dev):
    from egohmr_amd.factory import batch_to_device
    b_np, flags = R.golden_batch(g)
    batch = batch_to_device(b_np, dev)
    batch["smpl_params_is_axis_angle"] = flags                       # host values, as the loader delivers them
    return batch


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_end_to_end_against_the_reference(dev, golden_dir, synth_weights, smpl_asset, case):
    from egohmr_amd.diffusion import create_gaussian_diffusion
    g = np.load(os.path.join(golden_dir, f"g21_val_losses_{case}.npz"))
    B = int(g["B"])
    model = _golden_model(dev, synth_weights, smpl_asset, volsmpl=bool(g["volsmpl"]))
    assert [getattr(model, k) for k in R.WEIGHT_NAMES] == g["weights"].tolist()
    batch = _golden_batch(g, dev)
    batch["x_t"] = torch.from_numpy(g["x_t"]).to(dev)
    model.validation_setup()
    out = model(batch, torch.full((B,), int(g["timestep"]), device=dev, dtype=torch.long))
    failures = []
    for i, e in enumerate(g["epochs"]):
        o = dict(out)
        loss = model.compute_loss(batch, o, cur_epoch=int(e))
        assert list(o["losses"]) == list(R.LOSS_KEYS) and loss is o["losses"]["loss"]
        assert all(v.shape == () and v.dtype == torch.float32 and v.is_cuda for v in o["losses"].values())
        assert o["joint_vis_num_batch"].shape == () and o["joint_vis_num_batch"].dtype == torch.int64 and o["joint_vis_num_batch"].is_cuda
        assert int(o["joint_vis_num_batch"]) == int(g["joint_vis_num_batch"][i])
        assert np.array_equal(o["losses_per_item"]["joint_vis_mask"].cpu().numpy(), g["mask"])
        for k, ref in zip(R.LOSS_KEYS, g["losses"][i].astype(np.float64)):
            got = float(o["losses"][k].double())
            d = abs(got - ref) / abs(ref) if ref != 0 else abs(got)
            print(f"case {case} epoch {e} {k}: reference {ref:.9g} product {got:.9g} relative deviation {d:.3e} (bound {E2E_BOUND[k]:.3e})")
            if not d <= E2E_BOUND[k]:
                failures.append((k, int(e), d))
        np.testing.assert_allclose(o["losses_per_item"]["loss_v2v"].double().mean().item(), float(o["losses"]["loss_v2v"]), rtol=1e-6)
    if case == "b":
        assert float(g["losses"][0][9]) > 0 and float(g["losses"][1][9]) == 0
    assert not failures, failures
    # the same through the sampling call: val_losses(compute_loss=True) on a short DDIM loop - keys, shapes, finite values
    d = create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="ddim5")
    noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B, seed=4)).to(dev)
    o = d.val_losses(model, _golden_batch(g, dev), shape=[B, 144], clip_denoised=False, timestep_respacing="ddim5", cur_epoch=R.START_COAP_EPOCH,
                     noise_stack=noise)
    assert list(o["losses"]) == list(R.LOSS_KEYS) and all(torch.isfinite(v).item() and v.shape == () for v in o["losses"].values())
    assert 0 < int(o["joint_vis_num_batch"]) <= B * 24 and o["losses_per_item"]["loss"].shape == (B,)
    if case == "b":
        assert float(o["losses"]["loss_coap_penetration"]) > 0


def test_penetration_term_against_float64(dev, golden_dir, synth_weights, smpl_asset):
    """The capped penetration term of case b per item against the float64 restatement on the product's own vertices: the cap rule is the reference's
    (item 0 loses its points of index >= 4000, items 2.. keep theirs, item 1 selects nothing -> 0).  The proxy's search is float32: 1e-5 relative."""
    g = np.load(os.path.join(golden_dir, "g21_val_losses_b.npz"))
    B = int(g["B"])
    model = _golden_model(dev, synth_weights, smpl_asset, volsmpl=False)
    batch = _golden_batch(g, dev)
    batch["x_t"] = torch.from_numpy(g["x_t"]).to(dev)
    out = model(batch, torch.full((B,), int(g["timestep"]), device=dev, dtype=torch.long))
    model.compute_loss(batch, out, cur_epoch=R.START_COAP_EPOCH)
    term, n_sel, n_hi = R.penetration_f64(model.smpl_output.vertices.cpu().numpy(), model.scene_pcd_verts.cpu().numpy())
    assert n_sel.tolist() == g["n_selected"].tolist() and n_hi.tolist() == g["n_selected_high"].tolist()
    got = out["losses_per_item"]["loss_coap_penetration"].cpu().numpy()
    print("penetration per item", got.tolist(), "float64", term.tolist())
    assert got[1] == 0.0 and term[1] == 0.0
    np.testing.assert_allclose(got, term, rtol=1e-5, atol=0)


def test_validate_over_three_batches(dev, golden_dir, synth_weights, smpl_asset):
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.driver import validate
    g = np.load(os.path.join(golden_dir, "g21_val_losses_a.npz"))
    B = int(g["B"])
    model = _golden_model(dev, synth_weights, smpl_asset, volsmpl=False)
    d = create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="ddim5")
    stacks = [torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B, seed=s)).to(dev) for s in (11, 12, 13)]
    batches = [_golden_batch(g, dev) for _ in stacks]
    res = validate(model, d, batches, timestep_respacing="ddim5", cur_epoch=0, noise_stacks=stacks)
    assert list(res) == list(R.LOSS_KEYS) + ["loss_keypoints_3d_vis", "joint_vis_num"] and isinstance(res["joint_vis_num"], int)
    # the restatement on the arrays each call fed the kernel, aggregated as train_egohmr.py:176-207
    refs = []
    for batch, stack in zip(batches, stacks):
        o = d.val_losses(model, batch, shape=[B, 144], clip_denoised=False, timestep_respacing="ddim5", compute_loss=False, noise_stack=stack)
        inp = {k: v.cpu().numpy() for k, v in model.loss_inputs(batch, o).items()}
        refs.append(R.val_losses_f64(inp, [R.CASE_WEIGHTS[k] for k in R.WEIGHT_NAMES], None))
    n_vis = sum(r["joint_vis_num"] for r in refs)
    assert res["joint_vis_num"] == n_vis
    for k in R.LOSS_KEYS:
        s = sum(r["losses"][k] for r in refs)
        _close(res[k], s if k == "loss_keypoints_3d_vis_batch_sum" else s / 3, VALIDATE_RTOL, k)
    _close(res["loss_keypoints_3d_vis"], sum(r["losses"]["loss_keypoints_3d_vis_batch_sum"] for r in refs) / n_vis * 1000, 2 * VALIDATE_RTOL, "loss_keypoints_3d_vis")
    assert len({r["losses"]["loss_v2v"] for r in refs}) == 3          # three different samples
