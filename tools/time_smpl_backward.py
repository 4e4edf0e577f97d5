"""One SMPL backward at 1280 bodies with a dense vertex cotangent: the general VJP (ehm_smpl_backward) next to the 6-D one (ehm_smpl_backward_rot6d:
skin_bwd + posefeat_bwd + chain_bwd) and to the fixed-order variant of the general one (ehm_smpl_backward_ordered), in one run.  HIP events around each entry point; for per-kernel times run it under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_smpl_backward.py` (a run of its own).  Run from the repository root."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from egohmr_amd import _lib, synthetic as syn  # noqa: E402
from egohmr_amd.geometry import rot6d_to_rotmat  # noqa: E402
from egohmr_amd.smpl import SMPL  # noqa: E402

dev = torch.device("cuda:0")
B = 1280
smpl = SMPL(syn.make_smpl_asset(0)).to(dev)
g = torch.Generator(device="cpu").manual_seed(5)
x = torch.randn(B, 144, generator=g).to(dev)
betas = torch.randn(B, 10, generator=g).to(dev)
gv = torch.randn(B, 6890, 3, generator=g).to(dev)
gj = torch.randn(B, 45, 3, generator=g).to(dev)
mean, std = (torch.from_numpy(a).to(dev) for a in syn.make_body_rep_stats(0))
R = rot6d_to_rotmat((x * std + mean).reshape(-1, 6), "diffusion").view(B, 24, 3, 3).contiguous()
A, h, s = _lib.api(), smpl.handle(), _lib.stream_ptr()
nb = C.c_int64()
A.ehm_smpl_backward_workspace_bytes(h, B, C.byref(nb))
ws = torch.empty(nb.value, device=dev, dtype=torch.uint8)
nbo = C.c_int64()
A.ehm_smpl_backward_ordered_workspace_bytes(h, B, C.byref(nbo))
wso = torch.empty(nbo.value, device=dev, dtype=torch.uint8)
gb, gr, gp = torch.empty(B, 10, device=dev), torch.empty(B, 24, 3, 3, device=dev), torch.empty(B, 144, device=dev)


def timed(fn, n=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    e[0].record()
    for i in range(n):
        fn()
        e[i + 1].record()
    torch.cuda.synchronize()
    t = sorted(e[i].elapsed_time(e[i + 1]) for i in range(n))
    return t[len(t) // 2], t[0], t[-1]


cases = {
    "rot6d (parent's entry: verts -> pose6d)": lambda: A.ehm_smpl_backward_rot6d(h, betas, x, mean, std, gv, gp, B, s),
    "general: verts -> rotmats + betas": lambda: A.ehm_smpl_backward(h, betas, R, gv, None, gb, gr, B, ws, nb.value, s),
    "general: verts -> rotmats": lambda: A.ehm_smpl_backward(h, betas, R, gv, None, None, gr, B, ws, nb.value, s),
    "general: verts + joints -> rotmats + betas": lambda: A.ehm_smpl_backward(h, betas, R, gv, gj, gb, gr, B, ws, nb.value, s),
    "general, fixed order (ehm_smpl_backward_ordered): verts + joints -> rotmats + betas":
        lambda: A.ehm_smpl_backward_ordered(h, betas, R, gv, gj, gb, gr, B, wso, nbo.value, s),
    "general again: verts + joints -> rotmats + betas": lambda: A.ehm_smpl_backward(h, betas, R, gv, gj, gb, gr, B, ws, nb.value, s),
}
for k, fn in cases.items():
    med, lo, hi = timed(fn)
    print(f"[time] B={B} {k}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) of 10 calls, events around the whole entry point")
