#!/usr/bin/env python3
"""The autograd route of ModulatedGCN.forward (egohmr_amd/gcn_grad.py, csrc/gcn_bwd.hip) at the headline shape: B = 256, hid 1024, four blocks,
in_dim 3718.  One mode per process, so that a `rocprofv3 --kernel-trace --stats` run of its own sees that mode's kernels only:
    python tools/bench_gcn_grad.py fwd | bwd_x | bwd_full [--reps 5] [--batch 256]
fwd      = the differentiable forward alone
bwd_x    = the same forward + an input-only backward (gradient to x)
bwd_full = the same forward + a full backward (grad_params: W, M, adj2, bias of all convs, bn.weight / bn.bias)
Prints one JSON line: HIP-event time per iteration of the mode, and the bytes from shapes of the epilogue-backward kernel (2 x 4 N read + 8 N
written per row and conv).  A backward's kernel time = its mode's kernel sum minus the fwd mode's, from the two stats files."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from egohmr_amd.model import ModulatedGCN, smpl_tree_adjacency  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["fwd", "bwd_x", "bwd_full"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hid", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--in-dim", type=int, default=3718)
    ap.add_argument("--precision", default="f16x3")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = ModulatedGCN(smpl_tree_adjacency(), in_dim=a.in_dim, hid_dim=a.hid, num_layers=a.blocks).to(dev).eval()
    with torch.no_grad():                                   # trained-like statistics: activations stay O(1) through the blocks
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_var.uniform_(0.6, 1.4)
                mod.running_mean.normal_(0, 0.1)
    m.precision = a.precision
    m.grad_params = a.mode == "bwd_full"
    x = (torch.randn(a.batch, 24, a.in_dim, device=dev) * 0.5).requires_grad_()
    cot = torch.randn(a.batch, 24, 6, device=dev)

    def it():
        out = m(x)
        if a.mode != "fwd":
            out.backward(cot)
            x.grad = None
            m.zero_grad(set_to_none=True)

    for _ in range(2):
        it()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        it()
    e1.record()
    torch.cuda.synchronize()
    rows, convs = a.batch * 24, 1 + 2 * a.blocks
    print(json.dumps(dict(mode=a.mode, batch=a.batch, hid=a.hid, blocks=a.blocks, precision=a.precision, iterations=a.reps + 2,
                          ms_per_iteration=e0.elapsed_time(e1) / a.reps,
                          epilogue_bwd_bytes_per_hidden_conv=rows * 16 * a.hid, epilogue_bwd_launches_per_backward=convs + 1)))


if __name__ == "__main__":
    main()
