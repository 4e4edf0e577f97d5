"""CPU: the numpy restatements of tests/prep_pack_ref.py against outputs the reference itself recorded (tests/golden/g10_forward.npz, written by
oracle/make_golden.py from EgoHMR.forward), so that tests/test_gpu_prep_pack.py does not compare the kernels with a mistaken restatement."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prep_pack_ref as R  # noqa: E402
from egohmr_amd import synthetic as syn  # noqa: E402

FX_NORM = 1500.0            # cfg.CAM.FX_NORM_COEFF


def _golden_batch(golden_dir):
    g = np.load(os.path.join(golden_dir, "g10_forward.npz"))
    b = syn.make_batch(3, num_scene_points=int(g["num_scene_points"]), seed=int(g["batch_seed"]))
    b["orig_keypoints_2d"][0, :, 2] = 1.0          # as oracle/make_golden.py g10_forward: all visible
    b["orig_keypoints_2d"][1, :, 2] = 0.0          # none visible (the pelvis is forced)
    return g, b


def test_item_prep_ref_visibility_is_the_references(golden_dir):
    # (the golden's model was built with pelvis_vis_loosen=True: egohmr.py:114)
    g, b = _golden_batch(golden_dir)
    rng = np.random.default_rng(0)
    r = R.item_prep_ref(b["orig_keypoints_2d"], R.OPENPOSE_TO_SMPL_LOOSE, 8, b["smpl_params"]["transl"], b["fx"], FX_NORM, rng.normal(size=(4, 3)),
                        rng.normal(size=4), rng.normal(size=(2, 4)), rng.normal(size=2), other_ld=3, other_col0=0)
    ref = g["fuse__vis_mask_smpl"]
    assert ref.shape == (3, 24) and ref[0].all() and not ref[1].all() and ref[1].any()      # the golden holds both edge items
    np.testing.assert_array_equal(r["vis"].astype(bool), ref)
    np.testing.assert_array_equal(r["need"], ~ref.all(axis=1))


def test_pack_ref_projection_is_the_references(golden_dir):
    """kp3d_full / kp2d_full of pack_ref from the reference's own joints against what the reference made of them (egohmr.py:294-301), bit for bit:
    the recorded values are those of one correctly rounded float32 operation after the other, in the order pack_ref (and the kernel) perform them.
    (The pack is fed `joints`, not `joints_full`: the latter is its `joints + transl`, and is compared as such.)"""
    g, b = _golden_batch(golden_dir)
    for tag in ("fuse__", "nofuse__"):
        j = g[tag + "joints"]
        B = j.shape[0]
        z = np.zeros((B, 144), np.float32)
        r = R.pack_ref(z, z, np.zeros((B, 24, 9), np.float32), np.zeros((B, 1, 3), np.float32), j, np.zeros((B, 10), np.float32),
                       b["smpl_params"]["transl"], b["fx"], b["cam_cx"], b["cam_cy"], FX_NORM)
        assert R.same_bits(r["kp3d_full"], g[tag + "joints_full"]).all()
        assert R.same_bits(r["focal"], np.full((B, 2), 1500.0, np.float32)).all()
        assert R.same_bits(r["center"], np.stack([b["cam_cx"], b["cam_cy"]], axis=1)).all()
        assert R.same_bits(r["kp2d_full"], g[tag + "kp2d_full"]).all()


def test_pass_map_ref_against_brute_force():
    for group in (1, 2, 4):
        for need in itertools.product((False, True), repeat=6):
            slot, items, count = R.pass_map_ref(need, group)
            want = [b for b in range(6) if any(need[b // group * group: b // group * group + group])]
            assert list(items) == want and count == len(want)
            assert list(slot) == [want.index(b) if b in want else -1 for b in range(6)]
