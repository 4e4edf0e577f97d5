#!/usr/bin/env python3
"""CPU experiment behind the two-term split-f16 tier (docs/EXPERIMENTS.md R8): which of the two cross terms of a split-f16 product,
(ah + al)(wh + wl) ~ ah wh + ah wl + al wh, can the hidden graph convs of the denoiser do without, and for how many steps?

The float32 oracle's sampling loop (DDPM-100 on the x_t-sensitive weights, encoders hoisted) is run with the operands of the eight
gconv_layers.* convs rounded as a kernel that drops a term would see them, on chosen steps:
  * "activations hi only": x -> f16(x)              (drops al wh: a FRESH rounding error in every conv of every step)
  * "weights hi only":     W -> f16(64 W) / 64      (drops ah wl: the SAME perturbation in every step and pass - a coherent bias)
Distances are the final vertices / joints against the unpatched loop on the same noise.  Needs no GPU.  (It lives beside the tests because it imports the oracle, which tools/ must not: tests/test_cabi_cpu.py.)

    python tests/two_term_oracle_sweep.py [--batch 4] [--T 100] [--seed 100] [--out sweep.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Stepper:
    """the oracle model as the sampler sees it, counting the executed steps for the operand patch"""

    def __init__(self, model, state):
        self.model, self.state = model, state

    def __call__(self, batch, t):
        out = self.model(batch, t)
        self.state["step"] += 1
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--seed", type=int, default=100, help="batch and noise seed")
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from egohmr_amd import synthetic as syn
    from oracle import model as om, sampler as osamp, schedule as osched
    torch.set_grad_enabled(False)
    T, B = a.T, a.batch
    sd, asset = syn.make_sensitive_state_dict(0, T), syn.make_smpl_asset(0)
    mean, std = syn.make_body_rep_stats(0)
    ref = om.EgoHMROracle(sd, asset, mean, std, faithful=False)                      # faithful = False: the encoders run once per batch (hoisted)
    bnp = syn.make_batch(B, a.points, seed=a.seed)
    batch = {k: ({kk: torch.from_numpy(vv) for kk, vv in v.items()} if isinstance(v, dict) else torch.from_numpy(v)) for k, v in bnp.items()}
    noise = torch.from_numpy(syn.make_noise_stack(T, B, seed=a.seed))
    tables = osched.make_tables(T, "")

    hidden = [f"diffusion_model.gconv_layers.{b}.gconv{i}.gconv" for b in range(4) for i in (1, 2)]
    sd_whi = dict(ref.sd)
    for p in hidden:
        sd_whi[p + ".W"] = (ref.sd[p + ".W"] * 64).half().float() / 64
    state = {"step": 0, "act_hi": lambda k: False, "w_hi": lambda k: False}
    orig = om.modulated_graph_conv

    def patched(sd_, p, x, adj):
        if p in hidden:
            k = state["step"]
            if state["act_hi"](k):
                x = x.half().float()
            if state["w_hi"](k):
                sd_ = sd_whi
        return orig(sd_, p, x, adj)
    om.modulated_graph_conv = patched

    def loop(act_hi=lambda k: False, w_hi=lambda k: False):
        state.update(step=0, act_hi=act_hi, w_hi=w_hi)
        o = osamp.p_sample_loop(Stepper(ref, state), batch, tables, noise)["other_outputs"]
        return o["pred_vertices"].clone(), o["pred_keypoints_3d"].clone()

    base = loop()
    rows = []

    def row(name, **kw):
        v, j = loop(**kw)
        r = {"hidden_conv_product": name, "max_vertex_dist_mm": float((v - base[0]).norm(dim=-1).max()) * 1e3,
             "max_joint_dist_mm": float((j - base[1]).norm(dim=-1).max()) * 1e3, "B": B, "T": T, "seed": a.seed}
        rows.append(r)
        print(json.dumps(r), flush=True)

    always = lambda k: True
    row("weights hi only (drops ah*wl), all steps", w_hi=always)
    row("both hi only (plain f16), all steps", act_hi=always, w_hi=always)
    row("activations hi only (drops al*wh), all steps", act_hi=always)
    for n in (int(round(0.9 * T)), int(round(0.75 * T)), int(round(0.5 * T)), int(round(0.33 * T))):
        row(f"activations hi only on the first {n} steps, full on the last {T - n}", act_hi=lambda k, n=n: k < n)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
