#!/usr/bin/env python
"""Time the stage-1 pose flow (egohmr_amd.stage1.GlowFlow, csrc/flow.hip) against the same chain in eager float32 torch, on one GPU.

    python tools/flow_bench.py [--batch 256] [--samples 5 1] [--runs 30] [--warmup 5] [--once DIRECTION S] [--backward]

For each S: one sampling direction and one log_prob direction on synthetic weights (all context flags on, ctx = 2566), the median of `--runs`
timed calls after `--warmup`, timed on the device (hip events around the call).  The eager chain is the definition of tests/flow_ref.py written
with torch ops: unfolded ActNorm and LULinear (triangular solves when sampling), torch.addmm for every layer, the context repeated per sample.
Prints one JSON line per (S, direction).  `--once sample|log_prob S` runs one sampling call (host preparation, first launches) and then ten un-timed calls
of that direction, nothing else: the command to put behind `rocprofv3 --kernel-trace --stats --` for the launch count and the kernels' time
shares (docs/EXPERIMENTS.md).

`--backward` times the training legs instead, forward plus backward with the parameter gradients on (GlowFlow.grad_params = True; every eager
tensor a leaf that requires grad - L and U themselves, which spares eager the scatter of their entries): `log_prob` is -log_prob.mean() of the
poses, `sample` the sum of pred_pose_6d and log_prob over the samples.  Same inputs, same event timing; with `--once` it is the profiled command
of a backward direction."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from egohmr_amd import synthetic as syn  # noqa: E402
from egohmr_amd.stage1 import GlowFlow  # noqa: E402

PRE = "flow.flow._transform._transforms."


class EagerFlow:
    """The chain in eager float32 torch, weights prepared once (L, U built from their entries; nothing folded)."""

    def __init__(self, sd, dev):
        t = lambda k: torch.from_numpy(np.asarray(sd[k])).to(dev)
        self.blocks = []
        tril, triu = torch.tril_indices(144, 144, -1, device=dev), torch.triu_indices(144, 144, 1, device=dev)
        for l in range(4):
            a, lu, cp = (f"{PRE}{3 * l + j}." for j in range(3))
            Lm, U = torch.eye(144, device=dev), torch.zeros(144, 144, device=dev)
            Lm[tril[0], tril[1]] = t(lu + "lower_entries")
            U[triu[0], triu[1]] = t(lu + "upper_entries")
            U += torch.diag(F.softplus(t(lu + "unconstrained_upper_diag")) + 1e-3)
            n = cp + "transform_net."
            self.blocks.append(dict(scale=t(a + "log_scale").exp(), shift=t(a + "shift"), L=Lm, U=U, bias=t(lu + "bias"), idf=t(cp + "identity_features"),
                                    trf=t(cp + "transform_features"), W0=t(n + "initial_layer.weight"), b0=t(n + "initial_layer.bias"),
                                    Wf=t(n + "final_layer.weight"), bf=t(n + "final_layer.bias"),
                                    res=[dict(W=[t(f"{n}blocks.{k}.linear_layers.{j}.weight") for j in range(2)],
                                              b=[t(f"{n}blocks.{k}.linear_layers.{j}.bias") for j in range(2)],
                                              Wc=t(f"{n}blocks.{k}.context_layer.weight"), bc=t(f"{n}blocks.{k}.context_layer.bias")) for k in range(2)]))

    @staticmethod
    def net(b, x_id, c):
        h = F.linear(torch.cat([x_id, c], 1), b["W0"], b["b0"])
        for r in b["res"]:
            u = F.linear(F.relu(h), r["W"][0], r["b"][0])
            u = F.linear(F.relu(u), r["W"][1], r["b"][1])
            h = h + F.glu(torch.cat([u, F.linear(c, r["Wc"], r["bc"])], 1), dim=1)
        return F.linear(h, b["Wf"], b["bf"])

    def require_grad(self):
        for b in self.blocks:
            for v in list(b.values()) + [t for r in b["res"] for t in r["W"] + r["b"] + [r["Wc"], r["bc"]]]:
                if isinstance(v, torch.Tensor) and v.is_floating_point():
                    v.requires_grad_(True)

    def zero_grad(self):
        for b in self.blocks:
            for v in list(b.values()) + [t for r in b["res"] for t in r["W"] + r["b"] + [r["Wc"], r["bc"]]]:
                if isinstance(v, torch.Tensor):
                    v.grad = None

    @torch.no_grad()
    def sample(self, c, z):
        return self.sample_graph(c, z)

    @torch.no_grad()
    def log_prob(self, c, x):
        return self.log_prob_graph(c, x)

    def sample_graph(self, c, z):
        S = z.shape[1]
        c, x = c.repeat_interleave(S, 0), z.reshape(-1, 144)
        lp = -0.5 * (x * x).sum(1)
        for b in reversed(self.blocks):
            x = x.clone()
            x[:, b["trf"]] = x[:, b["trf"]] - self.net(b, x[:, b["idf"]], c)
            y = torch.linalg.solve_triangular(b["L"], (x - b["bias"]).t(), upper=False, unitriangular=True)
            x = (torch.linalg.solve_triangular(b["U"], y, upper=True).t() - b["shift"]) / b["scale"]
        return x, lp

    def log_prob_graph(self, c, x):
        S = x.shape[1]
        c, x = c.repeat_interleave(S, 0), x.reshape(-1, 144)
        for b in self.blocks:
            x = F.linear(F.linear(b["scale"] * x + b["shift"], b["U"]), b["L"], b["bias"])
            x = x.clone()
            x[:, b["trf"]] = x[:, b["trf"]] + self.net(b, x[:, b["idf"]], c)
        return -0.5 * (x * x).sum(1), x


def median_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--samples", type=int, nargs="+", default=None, help="default: 5 1, with --backward 1 2 5")
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--once", nargs=2, metavar=("DIRECTION", "S"))
    ap.add_argument("--backward", action="store_true")
    args = ap.parse_args()
    if args.samples is None:
        args.samples = [1, 2, 5] if args.backward else [5, 1]
    if args.runs < 20:
        ap.error("--runs must be at least 20")
    dev = torch.device("cuda:0")
    sd = syn.make_stage1_flow_state_dict(0)
    flow = GlowFlow(2566)
    flow.load_state_dict({k[len("flow.flow."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    flow.to(dev)
    eager = EagerFlow(sd, dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    B = args.batch
    c = torch.cat([0.3 * torch.randn(B, 6, generator=g), 2 * torch.rand(B, 2048, generator=g), torch.randn(B, 512, generator=g)], 1).to(dev)
    def hip_step(direction, x, z):
        flow.zero_grad(set_to_none=True)
        if direction == "sample":
            o = flow.sample_and_log_prob(c, z=z)
            (o["pred_pose_6d"].sum() + o["log_prob"].sum()).backward()
        else:
            (-flow.log_prob(x, c)[0].mean()).backward()

    def eager_step(direction, x, z):
        eager.zero_grad()
        if direction == "sample":
            xe, lp = eager.sample_graph(c, z)
            (xe.sum() + lp.sum()).backward()
        else:
            (-eager.log_prob_graph(c, x)[0].mean()).backward()

    if args.backward:
        flow.grad_params = True
        eager.require_grad()
    if args.once:
        S = int(args.once[1])
        z = torch.randn(B, S, 144, generator=g).to(dev)
        with torch.no_grad():
            x = flow.sample_and_log_prob(c, z=z)["pred_pose_6d"]      # (the host preparation and the first launches)
        fn = (lambda: flow.sample_and_log_prob(c, z=z)) if args.once[0] == "sample" else (lambda: flow.log_prob(x, c))
        if args.backward:
            fn = lambda: hip_step(args.once[0], x, z)
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        return
    for S in args.samples:
        z = torch.randn(B, S, 144, generator=g).to(dev)
        with torch.no_grad():
            out = flow.sample_and_log_prob(c, z=z)
        x = out["pred_pose_6d"]
        xe, _ = eager.sample(c, z)
        agree = float((xe.reshape(B, S, 144) - x).abs().max())
        if args.backward:
            for name in ("sample", "log_prob"):
                h_med, h_min = median_ms(lambda: hip_step(name, x, z), args.runs, args.warmup)
                e_med, e_min = median_ms(lambda: eager_step(name, x, z), args.runs, args.warmup)
                print(json.dumps({"bench": "flow_backward", "direction": name, "B": B, "S": S, "rows": B * S, "runs": args.runs,
                                  "hip_ms_median": round(h_med, 4), "hip_ms_min": round(h_min, 4), "eager_ms_median": round(e_med, 4),
                                  "eager_ms_min": round(e_min, 4), "eager_over_hip": round(e_med / h_med, 3)}), flush=True)
            continue
        for name, hip, ref in (("sample", lambda: flow.sample_and_log_prob(c, z=z), lambda: eager.sample(c, z)),
                               ("log_prob", lambda: flow.log_prob(x, c), lambda: eager.log_prob(c, x))):
            h_med, h_min = median_ms(hip, args.runs, args.warmup)
            e_med, e_min = median_ms(ref, args.runs, args.warmup)
            print(json.dumps({"bench": "flow", "direction": name, "B": B, "S": S, "rows": B * S, "runs": args.runs, "hip_ms_median": round(h_med, 4),
                              "hip_ms_min": round(h_min, 4), "eager_ms_median": round(e_med, 4), "eager_ms_min": round(e_min, 4),
                              "eager_over_hip": round(e_med / h_med, 3), "max_abs_diff_sample_vs_eager": agree}), flush=True)


if __name__ == "__main__":
    main()
