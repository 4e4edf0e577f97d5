#!/usr/bin/env python3
"""Generate tests/golden/g21_procrustes_rank1.npz by running the REFERENCE's own code on the CPU.

    python tools/make_eval_golden.py /path/to/EgoHMR-reference        # from the repo root; rewrites the file

Build-container tool in the style of tools/make_stage1_golden.py: no test and no product code reads it (the tests read the .npz it writes), and what
it stores is data only.  The cases are the rank-deficient Procrustes pairs of tests/eval_ref.py (G21_CASES: a prediction on the x axis, a prediction
collapsed to two points, one and two visible joints, a ground truth collapsed to one point).  Their correlation matrix K has rank 1, 2 or 0, so
LAPACK's completion of the SVD is arbitrary; stored are the inputs and only the outputs the data DETERMINE (eval_ref.determined): the aligned cloud
of utils/pose_utils.py compute_similarity_transform, or of reconstruction_error_with_vis_mask the visible joint's error and the visible sum (one
visible joint) or every joint's error (two)."""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)

from tests import eval_ref  # noqa: E402


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EGOHMR_REFERENCE", "")
    if not ref or not os.path.isfile(os.path.join(ref, "utils", "pose_utils.py")):
        sys.exit("usage: python tools/make_eval_golden.py <path to the reference EgoHMR checkout>")
    sys.path.insert(0, ref)
    from utils.pose_utils import compute_similarity_transform, reconstruction_error_with_vis_mask
    cases = eval_ref.procrustes_cases()
    arrays = {"names": np.array(eval_ref.G21_CASES)}
    for name in eval_ref.G21_CASES:
        c = cases[name]
        p, g = c["pred"].astype(np.float64), c["gt"].astype(np.float64)
        if c["mask"] is None:
            out = {"aligned": compute_similarity_transform(p, g)[None, None]}
        else:
            m3 = np.repeat(c["mask"][None, :, None], 3, axis=2)
            e = reconstruction_error_with_vis_mask(m3, p[None], g[None], avg_joint=False)
            out = {"per_joint": e[None], "vis_sum": (e * c["mask"]).sum(-1)[None]}
            arrays[f"{name}_mask"] = c["mask"]
        arrays[f"{name}_pred"], arrays[f"{name}_gt"] = c["pred"], c["gt"]
        arrays[f"{name}_want"] = eval_ref.determined(c, out)
        print(name, c.get("compare"), arrays[f"{name}_want"].reshape(-1)[:4])
    path = os.path.join(OUT, "g21_procrustes_rank1.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
