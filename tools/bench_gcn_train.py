#!/usr/bin/env python3
"""One forward + full backward of ModulatedGCN at the headline shape (B = 256, hid 1024, four blocks, in_dim 3718, grad_params = True) on the two
autograd routes: train-mode BatchNorm (ModulatedGCN.train_batchnorm: csrc/gcn_train.hip, batch statistics, backward through them, a handle of its own per
call) and eval-mode BatchNorm (frozen statistics: csrc/gcn_bwd.hip).
    python tools/bench_gcn_train.py [--rounds 3] [--reps 5] [--warmup 3] [--batch 256]
Every iteration is timed on its own with HIP events after a device synchronisation; prints one JSON line with the median, minimum and maximum per route and the
ratio of the medians.  The train-mode iterations include what an optimiser step forces on that route anyway: the handle and the packed weights are rebuilt
per call."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from egohmr_amd.model import ModulatedGCN, smpl_tree_adjacency  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed iterations per route and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hid", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--in-dim", type=int, default=3718)
    ap.add_argument("--precision", default="f16x3")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = ModulatedGCN(smpl_tree_adjacency(), in_dim=a.in_dim, hid_dim=a.hid, num_layers=a.blocks).to(dev)
    with torch.no_grad():                                   # trained-like statistics: activations stay O(1) through the blocks
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_var.uniform_(0.6, 1.4)
                mod.running_mean.normal_(0, 0.1)
    m.precision, m.grad_params, m.train_batchnorm = a.precision, True, True
    x = (torch.randn(a.batch, 24, a.in_dim, device=dev) * 0.5).requires_grad_()
    cot = torch.randn(a.batch, 24, 6, device=dev)

    def it():
        m(x).backward(cot)
        x.grad = None
        m.zero_grad(set_to_none=True)

    def route(train):
        m.train(train)
        for _ in range(a.warmup):
            it()
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            it()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return times

    ev, tr = [], []
    for _ in range(a.rounds):                               # the two routes alternate: a drift of the machine meets both
        ev += route(False)
        tr += route(True)
    ev, tr = [dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t)) for t in (ev, tr)]
    print(json.dumps(dict(batch=a.batch, hid=a.hid, blocks=a.blocks, in_dim=a.in_dim, precision=a.precision, rounds=a.rounds, reps=a.reps, warmup=a.warmup,
                          eval_autograd=ev, train_batchnorm=tr, ratio_train_over_eval=tr["median_ms"] / ev["median_ms"])))


if __name__ == "__main__":
    main()
