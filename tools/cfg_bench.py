#!/usr/bin/env python3
"""What classifier-free guidance scales on the visibility fuse cost: DDIM-10 of 100 at B = 256, N = 4096, conditioning cached, HIP events around
one sampling call.  Scale pairs (s_vis, s_inv): (1, 0) the select; (1, 0.5) the guidance kernels with pass pruning as before; (2.5, 0) every
item takes the second pass.  The precision schedule is calibrated per pair (the pair is part of its key) before the timed calls.
1 warm-up, 5 timed calls, medians.
    python tools/cfg_bench.py [B]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egohmr_amd import synthetic as syn  # noqa: E402
from egohmr_amd.diffusion import create_gaussian_diffusion  # noqa: E402
from egohmr_amd.factory import batch_to_device, build_synthetic_model  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
dev = torch.device("cuda:0")
model = build_synthetic_model(dev, 0, diffuse_fuse=True, sensitive=dict(num_diffusion_timesteps=100))
d = create_gaussian_diffusion(num_diffusion_timesteps=100, timestep_respacing="ddim10")
batch = batch_to_device(syn.make_batch(B, 4096, seed=1), dev)
noise = torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B, seed=1)).to(dev)
fs = model.fused_sampler
rows = []
for pair in ((1.0, 0.0), (1.0, 0.5), (2.5, 0.0)):
    model.guidance_param_visible, model.guidance_param = pair
    info = fs.calibrate_schedule(d, batch, ddim=True)
    fs.run(d, batch, noise, ddim=True)                       # warm-up (the conditioning stays cached)
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fs.run(d, batch, noise, ddim=True)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    st = fs.prepare(batch)
    rows.append({"scales": pair, "median_ms": round(ms[2], 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3), "second_passes": st.num_masked,
                 "k": info["k"], "two_term_steps": info.get("two_term_steps", 0), "f16_steps": fs.last_lowprec})
print(json.dumps({"workload": f"B={B} DDIM-10 of 100, N=4096, conditioning cached, f16x3 with the calibrated schedule", "rows": rows}))
