"""CPU: the validation losses of EgoHMR.compute_loss (egohmr.py:307-449) - the float64 restatement against the reference's own results
(tests/golden/g21_val_losses_*.npz, written by tests/make_loss_golden.py), the sampling-only rule, the C entry point's argument checks and
driver.validate's aggregation."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import val_losses_ref as R  # noqa: E402

# Largest relative deviation of the float64 restatement (oracle LBS in float64 on the golden's inputs) from the reference's float32 result, per key, over
# cases a, b (both epochs), c - measured (second column), bound = 4 x measured.  What differs: the reference's float32 arithmetic and summation.
MEASURED_RESTATEMENT_DEVIATION = {
    "loss": 1.28e-07, "loss_v2v": 1.04e-07, "loss_keypoints_3d": 2.40e-08, "loss_keypoints_3d_full": 7.13e-08, "loss_keypoints_2d_full": 1.42e-08,
    "loss_betas": 3.79e-08, "loss_body_pose": 3.74e-08, "loss_global_orient": 7.10e-08, "loss_pose_6d_ortho": 1.11e-07,
    "loss_coap_penetration": 8.60e-08, "loss_keypoints_3d_vis_batch_sum": 7.22e-08}
RESTATEMENT_BOUND = {k: 4 * v for k, v in MEASURED_RESTATEMENT_DEVIATION.items()}


def _golden(golden_dir, case):
    return np.load(os.path.join(golden_dir, f"g21_val_losses_{case}.npz"))


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_restatement_reproduces_the_reference(golden_dir, case):
    g = _golden(golden_dir, case)
    assert list(g["loss_keys"]) == list(R.LOSS_KEYS) and list(g["weight_names"]) == list(R.WEIGHT_NAMES)
    assert float(g["margin_px"]) >= 0.5                      # the fixture's condition: no projected joint near an image border
    inp = R.golden_inputs_cpu(g)
    scene = inp.pop("scene")
    for i, e in enumerate(g["epochs"]):
        pen = None
        if case == "b" and e >= int(g["start_coap_epoch"]):
            pen, n_sel, n_hi = R.penetration_f64(inp["pred_vertices"].astype(np.float32), scene)
            assert n_sel.tolist() == g["n_selected"].tolist() and n_hi.tolist() == g["n_selected_high"].tolist()
        r = R.val_losses_f64(inp, g["weights"], pen)
        assert np.array_equal(r["mask"], g["mask"]) and r["joint_vis_num"] == int(g["joint_vis_num_batch"][i])
        for k, ref in zip(R.LOSS_KEYS, g["losses"][i].astype(np.float64)):
            dev = abs(r["losses"][k] - ref) / abs(ref) if ref != 0 else abs(r["losses"][k])
            print(f"case {case} epoch {e} {k}: reference {ref:.9g} restatement {r['losses'][k]:.9g} relative deviation {dev:.3e}")
            assert dev <= RESTATEMENT_BOUND[k], (k, dev)
    if case == "b":
        assert g["losses"][0][9] > 0 and g["losses"][1][9] == 0


def _cpu_model(**kw):
    from egohmr_amd.factory import build_synthetic_model
    return build_synthetic_model("cpu", 0, **kw)


def test_sampling_only_batch_and_missing_annotations():
    m = _cpu_model(**R.CASE_WEIGHTS, start_coap_epoch=R.START_COAP_EPOCH)
    for k, v in R.CASE_WEIGHTS.items():
        assert getattr(m, k) == v
    assert m.start_coap_epoch == R.START_COAP_EPOCH
    out = {}
    loss = m.compute_loss({"img": torch.zeros(1)}, out)
    assert out["losses"] == {} and loss.shape == () and float(loss) == 0.0 and "joint_vis_num_batch" not in out
    batch = {"keypoints_3d": torch.zeros(2, 24, 3), "keypoints_3d_full": torch.zeros(2, 24, 3), "orig_keypoints_2d": torch.zeros(2, 25, 3),
             "smpl_params": {k: torch.zeros(2, n) for k, n in (("global_orient", 3), ("body_pose", 69), ("betas", 10), ("transl", 3))},
             "smpl_params_is_axis_angle": {"global_orient": np.ones(2, bool), "body_pose": np.ones(2, bool)}}
    with pytest.raises(KeyError, match="gender"):
        m.compute_loss(batch, {})
    full = dict(batch, gender=torch.zeros(2, dtype=torch.long))
    for k in ("keypoints_3d_full", "smpl_params_is_axis_angle"):
        with pytest.raises(KeyError, match=k):
            m.compute_loss({a: b for a, b in full.items() if a != k}, {})
    with pytest.raises(KeyError, match="betas"):
        m.compute_loss(dict(full, smpl_params={k: v for k, v in full["smpl_params"].items() if k != "betas"}), {})
    with pytest.raises(NotImplementedError, match="body_pose"):
        m.compute_loss(dict(full, smpl_params_is_axis_angle={"global_orient": np.ones(2, bool), "body_pose": np.array([True, False])}), {})


def test_ground_truth_bodies_stay_out_of_the_module_tree():
    from egohmr_amd import synthetic as syn
    m = _cpu_model(smpl_asset_male=syn.make_smpl_asset(1), smpl_asset_female=syn.make_smpl_asset(2))
    keys, n_params = set(m.state_dict()), len(list(m.parameters()))
    male, female = m.smpl_male, m.smpl_female
    assert male.gender == "male" and female.gender == "female" and m.smpl_male is male
    assert np.array_equal(male.v_template.numpy(), syn.make_smpl_asset(1)["v_template"])
    assert set(m.state_dict()) == keys and len(list(m.parameters())) == n_params
    assert not any("smpl_male" in k or "smpl_female" in k for k in keys) and not any(c is male or c is female for c in m.modules())
    # without explicit assets the constructor's rules hold: no file, no allow_synthetic_smpl -> an error, never a silent substitute
    with pytest.raises(FileNotFoundError):
        _cpu_model().smpl_male
    assert _cpu_model(allow_synthetic_smpl=True).smpl_female.gender == "female"


def _dummy_desc(**kw):
    """An ehm_val_losses_desc that passes every check, on dummy (never dereferenced) addresses; each use breaks one rule, so no call reaches a launch."""
    from egohmr_amd import _lib
    f = dict(B=4, V=6890, pred_joints=45, gt_joints=45, kp3d_points=24, kp3d_full_points=24, kp2d_points=25, workspace_bytes=1 << 20)
    for i, (name, typ) in enumerate(_lib.ValLossesDesc._fields_):
        if typ is ctypes.c_void_p:
            f[name] = 0x100000 * (i + 1)
    f.update(kw)
    return ctypes.byref(_lib.ValLossesDesc(**f))


def test_symbol_is_bound_and_rejects_bad_arguments_without_a_gpu():
    from egohmr_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(_lib.INCLUDE, "egohmr_hip.h")).read()
    for name in ("ehm_val_losses", "ehm_val_losses_workspace_bytes", "ehm_scene_cap_points"):
        assert name + "(" in header and name in _lib.PROTOTYPES and hasattr(L, name) and hasattr(_lib.api(), name)
    assert L.ehm_val_losses(None, None) == -22 and b"bad argument" in L.ehm_last_error()
    bad = [dict(B=0), dict(B=-3), dict(V=0), dict(pred_joints=44), dict(gt_joints=23), dict(kp3d_points=23), dict(kp3d_full_points=23), dict(kp2d_points=24),
           dict(workspace_bytes=8), dict(pred_vertices=0x100004), dict(workspace=0x100004)]
    required = [n for n, t in _lib.ValLossesDesc._fields_ if t is ctypes.c_void_p and n not in ("penetration", "vis_mask")]
    assert len(required) == 26
    bad += [{n: None} for n in required]
    for kw in bad:
        assert L.ehm_val_losses(_dummy_desc(**kw), None) == -22, kw
        assert b"bad argument" in L.ehm_last_error(), kw
    nb = ctypes.c_int64(0)
    assert L.ehm_val_losses_workspace_bytes(0, 6890, ctypes.byref(nb)) == -22 and L.ehm_val_losses_workspace_bytes(4, 0, ctypes.byref(nb)) == -22
    assert L.ehm_val_losses_workspace_bytes(4, 6890, None) == -22
    assert L.ehm_val_losses_workspace_bytes(256, 6890, ctypes.byref(nb)) == 0 and nb.value == (256 * 6 + 256 * 11) * 8   # 6 blocks of 4096 floats per body
    assert L.ehm_val_losses_workspace_bytes(3, 37, ctypes.byref(nb)) == 0 and nb.value == (3 + 3 * 11) * 8
    for args in ((None, 0x20000, 0x30000, 0x40000, 2, 10, 10, 4000), (0x10000, 0x20000, 0x30000, 0x40000, 0, 10, 10, 4000),
                 (0x10000, 0x20000, 0x30000, 0x40000, 2, 10, 0, 4000), (0x10000, 0x20000, 0x30000, None, 2, 10, 10, 4000)):
        assert L.ehm_scene_cap_points(*args, None) == -22, args
    assert tuple(_lib.LOSS_KEYS) == R.LOSS_KEYS


def test_validate_aggregation_against_a_hand_computed_dict():
    from egohmr_amd.driver import aggregate_val_losses
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    per_batch = [({"loss": t(2.0), "loss_v2v": t(0.5), "loss_keypoints_3d_vis_batch_sum": t(3.0)}, torch.tensor(40)),
                 ({"loss": t(4.0), "loss_v2v": t(0.25), "loss_keypoints_3d_vis_batch_sum": t(1.5)}, torch.tensor(20)),
                 ({"loss": t(6.0), "loss_v2v": t(0.75), "loss_keypoints_3d_vis_batch_sum": t(4.5)}, torch.tensor(30))]
    a = aggregate_val_losses(iter(per_batch))
    assert list(a) == ["loss", "loss_v2v", "loss_keypoints_3d_vis_batch_sum", "loss_keypoints_3d_vis", "joint_vis_num"]
    assert float(a["loss"]) == 4.0 and float(a["loss_v2v"]) == 0.5 and float(a["loss_keypoints_3d_vis_batch_sum"]) == 9.0
    assert float(a["loss_keypoints_3d_vis"]) == 100.0 and int(a["joint_vis_num"]) == 90
    assert float(per_batch[0][0]["loss"]) == 2.0                 # the batches' own tensors are not accumulated into
    with pytest.raises(ValueError):
        aggregate_val_losses(iter(()))
