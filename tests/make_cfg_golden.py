#!/usr/bin/env python3
"""Write tests/golden/g22_cfg_passes.npz by running the REFERENCE's own, unmodified EgoHMR.forward on the CPU (models/egohmr/egohmr.py:173-303).
Test infrastructure, run by hand where the reference tree is present; not collected by pytest.

    python tests/make_cfg_golden.py            # from the repository root

The reference cannot be asked for its two denoiser outputs c (conditional) and u (masked) with a scale between them - `guidance_param = 0` is a
literal (:248) - but three calls of its forward pin both on the batch of tests/cfg_ref.py (weights and batch seeded as G10, B = 3):
  f       the default call: c on visible joints, u on invisible ones
  c       eval_with_uncond=False: c on every joint
  u_free  the default call on a copy of the batch whose keypoint confidences are all zero: u on every joint that batch leaves invisible
          (u is computed from the masked condition and does not depend on the visibility; only the forced joint(s) stay visible)
`covered` [24] marks the joints u_free holds u on; at least 20 of the 24 per item is checked here.  The expected value of a scale pair on a covered
joint is u_free + s (c - u_free), formed by the tests in float64.  The file holds arrays only.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import cfg_ref as R  # noqa: E402
from egohmr_amd import synthetic as syn  # noqa: E402
from oracle import make_golden as mg  # noqa: E402


def main():
    mg.install_shims(syn.make_smpl_asset(0))
    torch.manual_seed(0)
    model = mg.build_reference_model(syn.make_state_dict(0), syn.make_smpl_asset(0), *syn.make_body_rep_stats(0), diffuse_fuse=True)
    model.validation_setup()
    b_np, x_t = R.make_batch3()
    t = torch.full((R.B3,), R.TIMESTEP, dtype=torch.long)

    def run(b, **kw):
        tb = mg.to_torch_batch(b)
        tb["x_t"] = torch.from_numpy(x_t)
        with torch.no_grad():
            o = model(tb, t, **kw)
        return o["pred_x_start"].numpy().reshape(R.B3, 24, 6), tb["vis_mask_smpl"].numpy()

    f, vis = run(b_np)
    c, _ = run(b_np, eval_with_uncond=False)
    zero = dict(b_np, orig_keypoints_2d=b_np["orig_keypoints_2d"].copy())
    zero["orig_keypoints_2d"][:, :, 2] = 0.0
    u_free, vis_free = run(zero)
    covered = ~vis_free
    assert vis[0].all() and 0 < vis[1].sum() < 24 and vis[2].sum() == vis_free[2].sum(), vis.sum(1)
    assert (covered.sum(1) >= 20).all(), covered.sum(1)
    # the three runs agree where they must: f is c on visible joints and u_free on invisible covered ones
    assert np.array_equal(f[vis], c[vis]) and np.array_equal(f[~vis & covered], u_free[~vis & covered])
    print("visible joints per item", vis.sum(1).tolist(), "covered", covered.sum(1).tolist())
    mg.save("g22_cfg_passes", B=R.B3, seed=R.SEED, timestep=R.TIMESTEP, num_scene_points=R.NUM_SCENE_POINTS, x_t=x_t, vis=vis, covered=covered,
            f=f, c=c, u_free=u_free)


if __name__ == "__main__":
    main()
