#!/usr/bin/env python3
"""Benchmark of the EgoHMR stage-2 sampling hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One "step" = one whole sampling call over one batch of synthetic items already resident in HBM:
conditioning encoders (ResNet-50, scene PointNet, heads) once, then T denoising steps (Modulated-GCN,
two passes with diffuse_fuse, rot6d->rotmat + SMPL LBS in every step, sampler update), final decode, and
at N > 1 the single RCCL all-gather of the packed SMPL parameters.  The default workload is the one
BASELINE.json's metric is quoted on: 100-step DDPM, batch 256 per GPU, 1 sample/item, 4096 scene points.
Rank 0 prints ONE JSON line (contract in the task statement).  A plain run measures the headline alone (its `roofline` and `cpu_baseline`
are null); `--full` adds everything else: comparison legs, roofline and per-kernel figures from a profiled call, the CPU baselines,
BASELINE configs 2-5 and the evaluation block.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

WORKLOADS = {
    # name: (num_diffusion_timesteps, respacing, description)
    "ddpm100": (100, "", "B256 S1 DDPM-100 N4096 ResNet50+PointNet cond, diffuse_fuse(2 GCN passes), LBS every step, unguided"),
    "c2_ddim10": (100, "ddim10", "BASELINE config 2: B256 S1 DDIM-10 N4096 ResNet50+PointNet cond, diffuse_fuse, LBS every step"),
    "c1_ddim5": (50, "ddim5", "BASELINE config 1 shape: DDIM-5 of 50"),
    # BASELINE config 3: B128 items x 10 samples, full 100-step DDPM, collision guidance on the last 11 steps (proxy loss, EXPERIMENTS 3.5);
    # a "step" = one batch of items = its 10 guided samples, run as ONE fused loop over 1280 bodies on ONE conditioning pass (the reference
    # runs 10 sequential loops and re-encodes in every step of each)
    "c3_guided": (100, "", "BASELINE config 3: B128 x S10 DDPM-100, collision-guided (last 11 steps), conditioning encoded once per item"),
    # BASELINE config 4 at its per-GPU shard: DDIM-50 (respace.py: 'ddim50' of a 1000-step process), 5 samples per item in one fused loop over
    # 1280 bodies on one conditioning pass (test_egohmr.py:247-266); the 8-GPU part of the config is `--gpus 8` of this workload
    "c4_ddim50_s5": (1000, "ddim50", "BASELINE config 4 per-GPU shard: B256 x S5 DDIM-50 (of 1000), conditioning encoded once per item"),
    # BASELINE config 5 at its per-GPU shard (1024 items per node = 128 per GPU): the VolSMPL twin (egohmr_volsmpl.py:582-629: collision loss over ALL
    # scene points, -loss.sum()), full 1000-step DDPM, "fp16 denoiser + fp32 LBS" = --precision f16 (plain f16 operands and activations in the hidden
    # convs of every step; encoders, input / output convs, sampler update, LBS in f32-grade arithmetic).  NOT a parity tier: MPJPE to the f32-grade run reported
    "c5_volsmpl_ddpm1000": (1000, "", "BASELINE config 5 per-GPU shard: B128 S1 DDPM-1000, VolSMPL-style collision guidance (all scene points, sum reduction), fp16 denoiser + fp32 LBS"),
}
WORKLOAD_PRECISION = {"c5_volsmpl_ddpm1000": "f16"}       # the precision a workload NAMES (overrides --precision's default only); its encoders run the
                                                          # plain-f16 tier too (EgoHMR.encoder_precision = 'f16': "for THIS tier only")
PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: dense f32-input MFMA peak
PEAK_F16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense f16/bf16 MFMA peak (~2.5 PFLOP/s)


PEAK_HBM_GBS = 8000.0          # MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s achievable on a float4 copy)
# Numbers measured on OTHER boxes in earlier rounds (committed under profiles/): context for a reader, NOT evidence of this run.  They are printed
# under the one key `references_measured_elsewhere` and nothing in the line is derived from them.
REFERENCES_MEASURED_ELSEWHERE = {
    "note": "round-3 measurements on other MI355X boxes (profiles/r03_*): context only, nothing in this line is computed from them",
    "mfma_only_ceiling_tflops_at_the_1400W_cap": {"f16": 1772.0, "f16x3": 1815.0, "source": "profiles/r03_mfma_ceiling.jsonl, profiles/r03_power_probe.jsonl"},
    "vendor_f16_gemm_of_one_hidden_conv_no_epilogue_us": {"value": 53.4, "source": "profiles/r03_gemm_yardstick.jsonl (torch.matmul / hipBLASLt, [12288,1024]x[1024,2048])"},
    "eager_torch_f32_on_mi355x_bodies_per_s": {"reference_structured": 32.0, "encoders_hoisted": 280.0, "source": "profiles/r03_eager_gpu_yardstick.jsonl (no SMPL forward in its steps)"},
    "encoder_activations_as_plain_f16": {"max_vertex_dist_mm": [0.4, 1.4], "source": "profiles/r04_encoder_precision_*.jsonl: fails the 0.1 mm bar on both weight sets"},
}


COMPACT_LIMIT = 4096            # bytes: the driver parsed round 3's 9 KB line and not round 4's 24 KB one; the final stdout line stays far below both


def _num(x, nd=4):
    """A strict-JSON number (no NaN / Infinity), rounded to nd significant digits; None for anything else."""
    if isinstance(x, bool) or x is None:
        return x
    try:
        x = float(x)
    except (TypeError, ValueError):
        return None
    if x != x or x in (float("inf"), float("-inf")):
        return None
    return float(f"{x:.{nd}g}") if x != int(x) or abs(x) >= 1e15 else int(x)


def _short(s, n):
    s = str(s)
    return s if len(s) <= n else s[: n - 1] + "~"


def compact_line(d):
    """The LAST stdout line of a run: one JSON object <= COMPACT_LIMIT bytes with the contract's keys, `roofline` and `cpu_baseline`
    (the full detail object goes to bench_detail.json and to stderr).  Pure function of the detail dict (tests/test_bench_line_cpu.py)."""
    def roof(r, per_launch_convs=8):
        if not r:
            return None
        kname = r["kernel"].split(" ")[0] + (" " + r["kernel"].split(" ")[1] if r["kernel"].split(" ")[0].endswith(",") else "")
        o = {"bound": r["bound"], "kernel": _short(kname, 48), "achieved": _num(r["achieved"]), "peak": _num(r["peak"]), "unit": r["unit"], "frac": _num(r["frac"])}
        if "issued_mfma_frac" in r:
            o["issued_frac"] = _num(r["issued_mfma_frac"])
        o["traffic"] = _num(r.get("traffic") * per_launch_convs) if r.get("traffic") else None
        if r.get("avg_launch_ms") is not None:            # the detail object carries the time per conv; one launch = the 8 chained convs
            o["avg_launch_ms"] = _num(r["avg_launch_ms"] * per_launch_convs)
            o["flops_per_launch"] = _num(r["flops_per_launch"] * per_launch_convs)
        return o

    cfg = d.get("config") or {}
    out = {k: d.get(k) for k in ("metric",)}
    out["value"] = _num(d.get("value"), 6)
    out["unit"] = d.get("unit")
    out["n_gpus"] = d.get("n_gpus")
    out["n_ranks_seen"] = d.get("n_ranks_seen")
    out["steps"], out["warmup"] = d.get("steps"), d.get("warmup")
    out["ms_per_step"] = _num(d.get("ms_per_step"), 6)
    out["higher_is_better"], out["scaling"], out["vs_baseline"] = True, d.get("scaling", "weak"), None
    out["dtype"] = _short(d.get("dtype_short") or d.get("dtype"), 160)
    out["data"] = "synthetic"
    out["config"] = {"workload": _short(cfg.get("workload"), 150), "name": cfg.get("name"), "items_per_gpu": cfg.get("items_per_gpu"),
                     "samples_per_item": cfg.get("samples_per_item"), "denoising_steps": cfg.get("denoising_steps"), "scene_points": cfg.get("scene_points"),
                     "gcn_passes_per_step": cfg.get("gcn_passes_per_step"), "lbs_every_step": cfg.get("lbs_every_step"), "collision_guided": cfg.get("collision_guided"),
                     "gcn_precision": cfg.get("gcn_precision"), "f16x3_last_steps": cfg.get("f16x3_last_steps"), "parallelism": _short(cfg.get("parallelism"), 70)}
    out["roofline"] = roof(d.get("roofline"))
    cb = d.get("cpu_baseline")
    out["cpu_baseline"] = None if not cb else {"value": _num(cb["value"]), "unit": cb["unit"], "cores": cb["cores"], "kind": cb["kind"], "sample": _short(cb["sample"], 200)}
    if d.get("n_gpus", 1) > 1:
        out["per_rank_bodies_per_s"] = [_num(v) for v in (d.get("per_rank_bodies_per_s") or [])]
        out["all_gather_ms"] = _num(d.get("all_gather_ms"))
    bd = d.get("breakdown_ms") or {}
    if bd:
        out["encoders_ms"] = _num(bd.get("encoders_and_projections_once"))
    hb = d.get("roofline_hbm") or {}
    if hb:
        out["roofline_hbm"] = {k: {"frac": _num(v["frac"], 3), "us": _num(v["avg_launch_us"], 4)} for k, v in hb.items()}
    subs = {}
    for name, sub in (d.get("configs") or {}).items():
        r = sub.get("roofline") or {}
        e = {"value": _num(sub.get("value"), 6), "ms_per_step": _num(sub.get("ms_per_step"), 6), "roofline_frac": _num(r.get("frac")),
             "encoders_ms": _num((sub.get("breakdown_ms") or {}).get("encoders_and_projections_once"))}
        for extra in ("bodies_per_step", "body_denoising_steps_per_s", "mpjpe_vs_f32_path_mm", "gcn_precision", "encoder_precision", "guidance_weight", "guided_step_us"):
            if sub.get(extra) is not None:
                e[extra] = _num(sub[extra]) if not isinstance(sub[extra], str) else sub[extra]
        subs[name] = e
    if subs:
        out["configs"] = subs
    ev = d.get("evaluation_block") or {}
    if ev.get("contact_score"):
        out["evaluation_block"] = {"contact_ms_1280_bodies": _num(ev["contact_score"]["ms"]), "contact_frac_f32_vector_peak": _num(ev["contact_score"]["frac_of_f32_vector_peak"], 3),
                                   "pa_mpjpe_ms": _num(ev.get("pa_mpjpe_ms"), 3), "v2v_GBps": _num((ev.get("v2v") or {}).get("GB_per_s"))}
    legs = {}
    for name in ("all_steps_f16x3", "f32_mfma_path", "f16_denoiser_path", "fp16_tier", "schedule_at_contract_tol"):
        if d.get(name):
            legs[name] = {"value": _num(d[name]["value"]), "mpjpe_mm": _num((d[name].get("vs_default_path") or {}).get("mpjpe_mm"), 3)}
    if legs:
        out["legs"] = legs
    out["detail"] = "bench_detail.json"
    line = json.dumps(out, allow_nan=False, separators=(",", ":"))
    # belt and braces: drop optional blocks, longest first, until the line fits
    for k in ("evaluation_block", "legs", "roofline_hbm", "configs"):
        if len(line) <= COMPACT_LIMIT:
            break
        out.pop(k, None)
        line = json.dumps(out, allow_nan=False, separators=(",", ":"))
    assert len(line) <= COMPACT_LIMIT, len(line)
    return line


def emit(detail):
    """Full detail object -> bench_detail.json (repo root and gpurun_out/); stdout carries ONE line, the compact one (round 4's 24 KB
    line was not parsed by the driver).  EGOHMR_BENCH_DETAIL_STDERR=1 also copies the detail object to stderr."""
    full = json.dumps(detail)
    for path in (os.path.join(REPO, "bench_detail.json"), os.path.join(REPO, "gpurun_out", "bench_detail.json")):
        try:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as f:
                f.write(full + "\n")
        except OSError:
            pass
    if os.environ.get("EGOHMR_BENCH_DETAIL_STDERR"):
        print("bench.py detail: " + full, file=sys.stderr, flush=True)
    print(f"bench.py: full detail object ({len(full)} bytes) written to bench_detail.json", file=sys.stderr, flush=True)
    sys.stdout.flush()
    print(compact_line(detail), flush=True)


DUMP_LIMIT_BYTES = 64 << 20     # --dump-outputs: at most this much in all; above it every array keeps the same seeded sample of its rows
DUMP_SAMPLE_SEED = 0


def output_arrays(outs, gathered, limit=DUMP_LIMIT_BYTES):
    """What one sampling call hands its caller, as host arrays for --dump-outputs: the gathered packed SMPL parameters and every tensor of the
    S result dicts (sample, pred_xstart, other_outputs...), named by their key path ('s<k>.' in front when S > 1).  float64 stays float64,
    everything else becomes float32.  If the whole exceeds `limit` bytes, every array with more than one row keeps a fixed, seeded, sorted
    sample of its rows (axis 0), the same rows for arrays of the same length, so that the files of two runs compare element for element;
    the cap is hard (ValueError if single-row arrays alone exceed it)."""
    arrays = {}

    def add(name, v):
        if isinstance(v, dict):
            for k, vv in v.items():
                add(f"{name}.{k}" if name else k, vv)
        elif torch.is_tensor(v):
            t = v.detach()
            arrays[name] = t.cpu().numpy() if t.dtype == torch.float64 else t.float().cpu().numpy()

    add("gathered_smpl_params", gathered)
    for k, o in enumerate(outs):
        add(f"s{k}" if len(outs) > 1 else "", o)
    total = sum(a.nbytes for a in arrays.values())
    if total > limit:
        scale = limit / total
        rows = {}
        for name, a in arrays.items():
            if a.ndim and a.shape[0] > 1:
                n = a.shape[0]
                if n not in rows:
                    keep = max(1, int(n * scale))
                    rows[n] = np.sort(np.random.Generator(np.random.PCG64(DUMP_SAMPLE_SEED)).choice(n, keep, replace=False))
                arrays[name] = np.ascontiguousarray(a[rows[n]])
        # only arrays of one row (none of today's outputs: they are all batch-major) are kept whole: they must not break the cap
        total = sum(a.nbytes for a in arrays.values())
        if total > limit:
            raise ValueError(f"--dump-outputs: {total} bytes after sampling rows, more than the {limit} allowed")
    return arrays


def dump_outputs(out_dir, arrays):
    """--dump-outputs: one <name>.npy per array under out_dir."""
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    print(f"bench.py: {len(arrays)} output arrays ({sum(a.nbytes for a in arrays.values())} bytes) written to {out_dir}", file=sys.stderr, flush=True)


def self_launch(argv):
    """`python bench.py --gpus N` with N > 1 and no torchrun environment: start the N ranks ourselves (one process per GPU,
    RCCL over xGMI), exactly as the driver would: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py <argv>.
    Returns the exit code of the launcher, or None when this process is already a rank / a single-GPU run."""
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--gpus", type=int, default=1)
    n = ap.parse_known_args(argv)[0].gpus
    if n <= 1 or "WORLD_SIZE" in os.environ:
        return None
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on this host driver (RCCL needs it)
    # the rendezvous store binds port 0 itself and hands the port it got to the ranks: no free port is looked up here and bound again later,
    # which another process of a busy machine can take in between (the launch then fails)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--rdzv-backend=c10d", "--rdzv-endpoint=127.0.0.1:0",
           f"--rdzv-id=bench-{os.getpid()}", "--local-addr=127.0.0.1", os.path.abspath(__file__), *argv]
    print(f"bench.py: --gpus {n} without a torchrun environment: launching {n} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    return subprocess.call(cmd, env=env)


def hidden_layer_flops(virtual_bodies: int, hid: int) -> float:
    """per body-pass and hidden conv 24*2*hid^2 MAC (W0,W1) + 24*24*hid MAC (adjacency mix)."""
    return virtual_bodies * (24 * 2 * hid * hid + 24 * 24 * hid) * 2.0


def kernel_source_sha1():
    import hashlib
    with open(os.path.join(REPO, "egohmr_amd", "csrc", "gcn_tile.hip"), "rb") as f:
        return hashlib.sha1(f.read()).hexdigest()


def pmc_traffic(precision):
    """HBM-side bytes per hidden conv of the chained launch, from the committed rocprofv3 --pmc passes (FETCH_SIZE x2 gfx950
    correction + WRITE_SIZE, tools/pmc_round.sh -> profiles/pmc_traffic.json).  Counters cannot be read from inside this
    process, so the figure is only reported when it was collected for THIS kernel source (sha1 of csrc/gcn_tile.hip recorded next
    to it); otherwise None."""
    try:
        with open(os.path.join(REPO, "profiles", "pmc_traffic.json")) as f:
            e = json.load(f).get(precision, {})
    except OSError:
        return None
    return e.get("bytes_per_conv") if e.get("kernel_source_sha1") == kernel_source_sha1() else None


def cpu_baseline(n, rs, num_scene_points, budget_s, faithful=True):
    """The oracle on a bounded sample: B=4 items, as many leading steps of the same schedule as fit the time budget.
    faithful=True: like the reference (encoders inside every step, two GCN passes, eager torch-CPU); faithful=False: the same CPU
    arithmetic with the step-invariant encoders hoisted out of the loop - separates what hoisting buys from what the GPU buys."""
    from egohmr_amd import synthetic as syn
    from oracle import model as om, schedule as osched
    # eager torch-CPU on small batches is fastest at 16 threads on the MI355X host (measured 16/32/64: 0.28/0.20/0.10 bodies/s); use what helps and report it
    cores = int(os.environ.get("EGOHMR_CPU_THREADS", min(os.cpu_count() or 1, 16)))
    torch.set_num_threads(cores)
    B = 4
    sd, asset = syn.make_state_dict(0), syn.make_smpl_asset(0)
    mean, std = syn.make_body_rep_stats(0)
    ref = om.EgoHMROracle(sd, asset, mean, std, faithful=faithful)
    bnp = syn.make_batch(B, num_scene_points, seed=0)
    batch = {k: ({kk: torch.from_numpy(vv) for kk, vv in v.items()} if isinstance(v, dict) else torch.from_numpy(v)) for k, v in bnp.items()}
    tab = osched.make_tables(n, rs)
    T = tab.num_timesteps
    noise = torch.from_numpy(syn.make_noise_stack(T, B, seed=0))
    x = noise[0]
    done, t0 = 0, time.perf_counter()
    with torch.no_grad():
        for k, i in enumerate(range(T - 1, -1, -1)):
            batch["x_t"] = x
            mo = ref(batch, torch.full((B,), tab.timestep_map[i], dtype=torch.long))
            x = float(np.float32(tab.posterior_mean_coef1[i])) * mo["pred_x_start"] + float(np.float32(tab.posterior_mean_coef2[i])) * x \
                + (0.0 if i == 0 else 1.0) * float(np.exp(0.5 * np.float32(tab.posterior_log_variance_clipped[i]))) * noise[1 + k]
            done += 1
            if faithful and time.perf_counter() - t0 > budget_s and done >= 2:
                break
    dt = time.perf_counter() - t0
    if faithful:
        per_call = dt / done * T
        how = "reference-faithful: ResNet-50 + PointNet re-run every step"
    else:       # the first step carries the one-off encoders: time it apart
        per_call = dt if done == T else float("nan")
        how = "encoders hoisted (run once), otherwise the same eager CPU arithmetic"
    return {"value": B / per_call, "unit": "bodies/s", "cores": cores, "kind": "port",
            "sample": f"oracle/ (CPU restatement, {how}, 2 GCN passes, eager torch-CPU fp32, {cores} threads): B={B} items, "
                      f"{done} of {T} steps timed ({dt:.1f} s)" + (f", extrapolated linearly to {T} steps" if faithful and done < T else "")}


def measure(args, workload, steps, warmup, legs_on, cpu_seconds, dev, rank, world, tier_compare=True, dump_dir=None, full=False):
    """One workload end to end (model, inputs, calibration, warm-up, the timed region): the JSON object of rank 0.
    full: also the collective timing, the legs, the profiled call, the encoder split and the CPU baselines, behind the timed region.
    dump_dir: rank 0 writes what the last timed call returned there (output_arrays)."""
    if args.precision_given is None and workload in WORKLOAD_PRECISION:
        args = argparse.Namespace(**{**vars(args), "precision": WORKLOAD_PRECISION[workload]})
    from egohmr_amd import _lib
    from egohmr_amd import dist as edist
    from egohmr_amd import synthetic as syn
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device, build_synthetic_model

    n, rs, desc = WORKLOADS[workload]
    B, N = args.batch, args.scene_points
    S, guided, volsmpl = 1, False, False
    if workload == "c3_guided":
        S, guided = 10, True
        if args.batch == 256:
            B = 128
    elif workload == "c4_ddim50_s5":
        S = 5
    elif workload == "c5_volsmpl_ddpm1000":
        guided, volsmpl = True, True
        if args.batch == 256:
            B = 128
    sens = dict(num_diffusion_timesteps=n) if args.weights == "sensitive" else None
    model = build_synthetic_model(dev, 0, diffuse_fuse=True, sensitive=sens, volsmpl=volsmpl)
    model.lbs_every_step = not args.no_lbs_every_step
    if args.loop_bodies is not None:
        model.loop_bodies = int(args.loop_bodies)
    model.gcn_precision = args.precision
    if args.precision_given is None and workload in WORKLOAD_PRECISION:
        model.encoder_precision = "f16"
    if args.f16x3_last_steps is not None:
        model.f16x3_last_steps = int(args.f16x3_last_steps)
    diffusion = create_gaussian_diffusion(num_diffusion_timesteps=n, timestep_respacing=rs)
    T = diffusion.num_timesteps
    batch = batch_to_device(syn.make_batch(B, N, seed=100 + rank), dev)            # inputs resident in HBM before timing
    noise = torch.from_numpy(syn.make_noise_stack(T, B, seed=100 + rank)).to(dev)
    noises = [noise] + [torch.from_numpy(syn.make_noise_stack(T, B, seed=100 + rank + 1000 * k)).to(dev) for k in range(1, S)]
    if guided:   # put the floor through the bodies so that the collision term is live (as in the guided golden)
        batch["scene_pcd_verts_full"][:, : N // 3, 1] = batch["smpl_params"]["transl"][:, None, 1] - 0.6
    fs = model.fused_sampler
    ddim = bool(rs)
    # guidance strength: C3 as in the guided goldens (2.0); the VolSMPL twin's own default (30, times B through -loss.sum()) is a chaotic regime with
    # the build's proxy loss (docs/EXPERIMENTS.md 3.5), so C5 is timed at the weight its tight goldens use (0.5) - the kernels' work does not depend on it
    w_guid = (0.5 if volsmpl else 2.0) if guided else 1.0

    def one_call(m=model):
        f = m.fused_sampler
        f.invalidate()                                                               # conditioning is part of the job: re-encode
        # the S samples of an item share its conditioning and are independent given it: one fused loop over S*B bodies
        # (FusedSampler.run_samples; bit-equal to S sequential loops, tests/test_gpu_api.py)
        # defer_status: the chain-status word of this call is read when the next call starts (and by check_status() behind the timed
        # region) instead of with a host wait at the end of every call
        outs = f.run_samples(diffusion, batch, noises[:S], ddim=ddim, guided=guided, cond_grad_weight=w_guid, defer_status=True)
        packs = [edist.pack_params(o["other_outputs"]["pred_smpl_params"]) for o in outs]
        return edist.gather_packed(torch.cat(packs, 0)), outs

    def one_step(m=model):
        gathered, outs = one_call(m)
        return gathered, outs[-1]

    # the precision schedule of the default path is CALIBRATED on the loaded weights (FusedSampler.calibrate_schedule) - here, before the
    # warm-up, on the first items of this batch; it is a one-off per (checkpoint, sampler) and not part of a steady-state sampling call
    t_cal = None
    if args.precision == "f16x3" and model.f16x3_last_steps == "auto":
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        edist.agree_schedule(fs, diffusion, batch, ddim=ddim, guided=guided, cond_grad_weight=w_guid, denom_items=B)   # rank 0 measures, every rank adopts
        torch.cuda.synchronize()
        t_cal = time.perf_counter() - t1
    for _ in range(warmup):
        one_step()
    torch.cuda.synchronize()
    edist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        gathered, outs = one_call()
        if not dump_dir:
            outs = outs[-1:]                                                         # (only the last sample's dict is held across the next call)
    torch.cuda.synchronize()
    fs.check_status()                                                                # (inside the timed region: the last call's status word)
    edist.barrier()
    torch.cuda.synchronize()
    dt_rank = time.perf_counter() - t0
    res = outs[-1]
    if dump_dir and rank == 0:                                                       # (behind the timed region, before any other call)
        dump_outputs(dump_dir, output_arrays(outs, gathered))
    dt = edist.max_over_ranks(dt_rank, dev)
    per_rank = edist.gather_floats(B * S * steps / dt_rank, dev)                   # bodies/s of every rank (its own clock)
    assert torch.isfinite(res["other_outputs"]["pred_vertices"]).all()
    assert gathered.shape == (world * B * S, edist.PACKED_WIDTH)
    lowprec = fs.last_lowprec                                                        # leading steps on plain f16 operands in the timed calls
    sched = fs.schedule_info
    value = world * B * S * steps / dt
    k_last = T - lowprec
    passes = 2

    # the headline object: what the timed calls and the calibration before them measured, nothing that takes a launch of its own
    out = None
    if rank == 0:
        num_masked = fs.prepare(batch).num_masked                                   # (the last timed call's conditioning, still cached: no launch)
        out = {
            "metric": "sampled bodies/sec (100-step DDPM, batch 256)" if workload == "ddpm100" else f"sampled bodies/sec ({workload})",
            "value": value,
            "unit": "bodies/s",
            "n_gpus": world,
            "n_ranks_seen": world if world == 1 else int(torch.distributed.get_world_size()),
            "per_rank_bodies_per_s": per_rank, "all_gather_ms": None,
            "multi_gpu_note": None if world == 1 else ("weak scaling: every rank runs the whole N = 1 job on its own items, value = all items / the slowest rank's time; expect a "
                                                       "few percent below N x the one-GPU number: N sockets at their own 1400 W caps clock independently (box-to-box spread "
                                                       "was +-3 %), and each rank's Python thread enqueues ~200 launches per call"),
            "steps": steps,
            "warmup": warmup,
            "ms_per_step": dt / steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": {"f32": "f32",
                      "f16x3": "f32 results: denoiser GEMMs as 3x f16 MFMA on hi/lo-split operands (f32 accumulate) on the last "
                               f"{k_last} of {T} steps, plain f16 operands on the first {lowprec}; k = {k_last} is " +
                               ("given on the command line" if args.f16x3_last_steps is not None else "CALIBRATED on the loaded weights") +
                               f" to a {model.schedule_tol:g} m bar (final bodies vs the all-split loop; the contract bar is 1e-4 m: leg schedule_at_contract_tol; docs/EXPERIMENTS.md 3.6)",
                      "f16": "f16 denoiser GEMMs and activations (f32 accumulate) + f32 everything else"}[args.precision],
            "data": "synthetic",
            "full": bool(full),
            "config": {"workload": desc, "name": workload, "items_per_gpu": B, "samples_per_item": S, "samples_in_one_loop": bool(S > 1), "collision_guided": guided, "denoising_steps": T,
                       "scene_points": N, "gcn_passes_per_step": passes, "lbs_every_step": bool(model.lbs_every_step),
                       "gcn_precision": args.precision, "encoder_precision": model.encoder_precision, "guidance_weight": w_guid if guided else None, "f16x3_last_steps": k_last if args.precision == "f16x3" else None,
                       "f16x3_last_steps_policy": str(model.f16x3_last_steps),
                       "pass_pruning": {"items_without_second_pass": int(B - num_masked) if model.prune_passes else 0, "of": B,
                                        "note": "exact (egohmr.py:249-254): all-visible items skip the image-masked pass; the synthetic "
                                                "visibility draw (Bernoulli 0.6 per OpenPose joint, SURVEY 8d) almost never produces one"},
                       "weights": ("seeded synthetic, x_t-SENSITIVE (trained-like: d x0 / d x_t follows the MMSE gain of a Gaussian prior; synthetic.make_sensitive_state_dict)"
                                   if args.weights == "sensitive" else "seeded synthetic, plain random network (ignores x_t; rounds 1-2)") + " - no checkpoint offline",
                       "smpl": "synthetic SMPL-shaped asset",
                       "parallelism": f"items sharded x{world}, one RCCL all-gather of [B,226] at the end"},
            "schedule": None if args.precision != "f16x3" else {
                "f16x3_last_steps": k_last, "f16_steps": lowprec, "calibrated": sched is not None and args.f16x3_last_steps is None,
                "explicit_k_from_command_line": args.f16x3_last_steps,
                "schedule_calibrated_on": None if sched is None else f"the loaded ({args.weights}) weights, {sched['bodies']} items of this batch, 2 private noise draws, tol {sched['tol_m']:g} m",
                "calibration_seconds_once_per_checkpoint_and_sampler": t_cal, "calibration_trials": None if sched is None else sched["trials"]},
            "bodies_per_step": B * S,
            "body_denoising_steps_per_s": value * T,                      # makes loops of different length comparable (C5: 1000 steps per body)
        }
    if not full:
        return out

    # --full: everything else this workload reports, each with launches of its own behind the timed region
    if world > 1:                                                                    # the one collective of a call, timed apart (5 calls, barriers outside)
        pk = torch.cat([edist.pack_params(res["other_outputs"]["pred_smpl_params"])] * S, 0)
        edist.gather_packed(pk)
        torch.cuda.synchronize()
        edist.barrier()
        t1 = time.perf_counter()
        for _ in range(5):
            edist.gather_packed(pk)
        torch.cuda.synchronize()
        gather_ms = edist.max_over_ranks((time.perf_counter() - t1) / 5 * 1e3, dev)
        if rank == 0:
            out["all_gather_ms"] = gather_ms

    # comparison legs (rank-local, N=1 only): the same job, same noise, (a) WITHOUT the precision schedule (every step split-f16: f32-grade
    # for ANY weights), (b) with the hidden convs on the f32-input MFMA (exact f32 products), (c) on plain f16 operands in every step (the
    # "fp16 denoiser" of BASELINE config 5; NOT parity-grade) - each with its distance to the default path's vertices / joints - and (d) the
    # default path on the OTHER synthetic weight set (its own calibration)
    legs = {}
    if args.precision == "f16x3" and world == 1 and not (not legs_on):
        ref_v = res["other_outputs"]["pred_vertices"].float().clone()
        ref_j = res["other_outputs"]["pred_keypoints_3d"].float().clone()

        def leg(prec, last_steps, m=model, compare=True, enc="f16x3"):
            old = (m.gcn_precision, m.f16x3_last_steps, m.encoder_precision)
            m.gcn_precision, m.f16x3_last_steps, m.encoder_precision = prec, last_steps, enc
            try:
                one_step(m)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                _, r = one_step(m)
                torch.cuda.synchronize()
                m.fused_sampler.check_status()
                d = time.perf_counter() - t1
            finally:
                m.gcn_precision, m.f16x3_last_steps, m.encoder_precision = old
            out = {"value": B * S / d, "unit": "bodies/s", "ms_per_step": d * 1e3}
            if compare:
                v = r["other_outputs"]["pred_vertices"].float()
                dv = (v - ref_v).norm(dim=-1)                              # per-vertex distance [B, V], metres
                out["vs_default_path"] = {"max_vertex_dist_mm": float(dv.max()) * 1e3, "mean_v2v_mm": float(dv.mean()) * 1e3,
                                          "mpjpe_mm": float((r["other_outputs"]["pred_keypoints_3d"].float() - ref_j).norm(dim=-1).mean()) * 1e3}
            return out

        legs["all_steps_f16x3"] = leg("f16x3", None)
        legs["all_steps_f16x3"]["note"] = "every step in split-f16 (3 MFMA per product): f32-grade for ANY weights, no calibration involved"
        if S == 1:
            legs["f32_mfma_path"] = leg("f32", None)
        legs["f16_denoiser_path"] = leg("f16", None)
        legs["f16_denoiser_path"]["note"] = ("plain f16 operands and f16 activations in the hidden convs of EVERY step (f32 accumulate, everything "
                                             "else f32): BASELINE config 5's fp16 denoiser, not a parity path on its own")
        legs["fp16_tier"] = leg("f16", None, enc="f16")
        legs["fp16_tier"]["note"] = ("BASELINE config 5's fp16 tier as a whole: plain-f16 denoiser AND plain-f16 encoders (hi halves only: one MFMA per product, half the "
                                     "bytes), float32 LBS / sampler update.  NOT a parity path (reference-golden bound: tests/test_gpu_schedule.py::"
                                     "test_fp16_tier_mpjpe_bound_vs_reference_golden)")
        if workload == "ddpm100" and model.f16x3_last_steps == "auto":
            # the same job with the schedule calibrated to the north-star's OWN bar (1e-4 m -> criterion 5e-5 m) instead of the default 1e-5 m
            old_tol = model.schedule_tol
            model.schedule_tol = 1e-4
            try:
                info_c = fs.calibrate_schedule(diffusion, batch, ddim=ddim, guided=guided, cond_grad_weight=w_guid, denom_items=B)
                legs["schedule_at_contract_tol"] = leg("f16x3", "auto")
                legs["schedule_at_contract_tol"].update({
                    "tol_m": 1e-4, "criterion": info_c["criterion"], "calibrated_f16x3_last_steps": info_c["k"], "f16_steps": info_c["f16_steps"],
                    "calibration_trials": info_c["trials"],
                    "note": "default schedule_tol is 1e-5 m (10x stricter than the 1e-4 m contract); this leg shows what the contract bar itself would allow on "
                            "the loaded weights.  Reference-golden gates for mixed schedules: tests/test_gpu_schedule.py (G16, G17)"})
            finally:
                model.schedule_tol = old_tol
        if workload == "ddpm100":
            other = "insensitive" if args.weights == "sensitive" else "sensitive"
            m2 = build_synthetic_model(dev, 0, diffuse_fuse=True, sensitive=dict(num_diffusion_timesteps=n) if other == "sensitive" else None)
            m2.lbs_every_step = model.lbs_every_step
            info2 = m2.fused_sampler.calibrate_schedule(diffusion, batch, ddim=ddim, guided=guided, cond_grad_weight=w_guid, denom_items=B)
            legs[f"default_path_on_{other}_weights"] = leg("f16x3", "auto", m2, compare=False)
            _, r_sched = one_step(m2)
            m2.f16x3_last_steps = None
            _, r_all = one_step(m2)
            m2.f16x3_last_steps = "auto"
            dv2 = (r_sched["other_outputs"]["pred_vertices"].float() - r_all["other_outputs"]["pred_vertices"].float()).norm(dim=-1)
            legs[f"default_path_on_{other}_weights"].update({
                "vs_its_all_steps_f16x3_run": {"max_vertex_dist_mm": float(dv2.max()) * 1e3, "mean_v2v_mm": float(dv2.mean()) * 1e3},
                "calibrated_f16x3_last_steps": info2["k"], "measured_gain_dx0_dxt": m2.fused_sampler.measure_gain(batch, timesteps=(n - 1, n // 2, n // 10, 0)),
                "note": "the same job with the other synthetic weight set and ITS calibrated schedule (rounds 1-2 benchmarked the insensitive set with a constant k = 8)"})
            del m2
            torch.cuda.empty_cache()

    # (tier_compare: an explicit switch - this leg also runs for the sub-configs, which are measured with the other legs off: two more calls of the job)
    if args.precision == "f16" and world == 1 and tier_compare and workload in WORKLOAD_PRECISION:
        # the fp16-denoiser tier against the f32-grade run of the SAME job (same noise): what the tier costs in accuracy, next to what it buys
        j16 = res["other_outputs"]["pred_keypoints_3d"].float().clone()
        v16 = res["other_outputs"]["pred_vertices"].float().clone()
        old_p = (model.gcn_precision, model.f16x3_last_steps, model.encoder_precision)
        model.gcn_precision, model.f16x3_last_steps, model.encoder_precision = "f16x3", None, "f16x3"
        try:
            one_step()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            _, r32 = one_step()
            torch.cuda.synchronize()
            fs.check_status()
            d32 = time.perf_counter() - t1
        finally:
            model.gcn_precision, model.f16x3_last_steps, model.encoder_precision = old_p
        j32 = r32["other_outputs"]["pred_keypoints_3d"].float()
        legs["f32_grade_path_of_this_job"] = {
            "value": B * S / d32, "unit": "bodies/s", "ms_per_step": d32 * 1e3,
            "this_tier_vs_it": {"mpjpe_mm": float((j16 - j32).norm(dim=-1).mean()) * 1e3,
                                "max_vertex_dist_mm": float((v16 - r32["other_outputs"]["pred_vertices"].float()).norm(dim=-1).max()) * 1e3},
            "note": "every step split-f16 (f32-grade); reference-golden bound of the f16 tier on DDPM-1000: tests/test_gpu_configs.py::test_c5_fp16_denoiser_ddpm1000_mpjpe_bound"}

    # one PROFILED call (outside the timed region): every launch of the sampling loop bracketed by HIP events on the launch stream
    # (ehm_profile_begin / ehm_profile_end), summed per launch class -> the live per-kernel durations the roofline objects use
    import ctypes as C
    L = _lib.lib()
    torch.cuda.synchronize()
    _lib.check(L.ehm_profile_begin(), "ehm_profile_begin")
    one_step()
    torch.cuda.synchronize()
    ncls = len(_lib.PROF_CLASSES)
    ms_arr, cnt_arr = (C.c_double * ncls)(), (C.c_int64 * ncls)()
    _lib.check(L.ehm_profile_end(ms_arr, cnt_arr, ncls), "ehm_profile_end")
    prof = {c: {"ms_per_call": ms_arr[i], "launches_per_call": int(cnt_arr[i]), "avg_launch_us": (ms_arr[i] / cnt_arr[i] * 1e3) if cnt_arr[i] else None}
            for i, c in enumerate(_lib.PROF_CLASSES)}
    nearest_evals = prof.pop("guid_nearest_evals")["launches_per_call"]      # a COUNT (EHM_PROF_G_NEAREST_EVALS): point-to-vertex distance evaluations of the profiled call

    # split of one call (rank 0, informative)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    fs.invalidate()
    st = fs.prepare(batch)
    torch.cuda.synchronize()
    t_enc = time.perf_counter() - t1

    if rank == 0:
        hid = model.diffusion_model.hid_dim
        # samples of an item run in groups of loop_bodies // B per fused loop (FusedSampler.run_samples): a LAUNCH works on S_l samples' bodies
        lb = int(getattr(model, "loop_bodies", 0) or 0)
        g_s = S if (lb <= 0 or S == 1) else max(1, min(S, lb // B))
        n_groups = -(-S // g_s)
        S_l = S / n_groups                                                            # samples per launch (average when S % g_s != 0)
        vbodies = S_l * (B + (st.num_masked if model.prune_passes else B))          # body-passes per launch after pass pruning
        rows = vbodies * 24
        flops = hidden_layer_flops(vbodies, hid)
        n_hidden = 2 * model.diffusion_model.num_layers
        names = {"f32": "gcn_hidden_kernel (f32-input MFMA GEMM + fused modulated-adjacency/BN/ReLU epilogue), one launch per conv",
                 "f16x3": "gcn_hidden_chain_kernel<3, 4> (csrc/gcn_tile.hip): the 8 hidden convs of a GCN forward chained in one launch (4-wave 192x64 tiles); split-f16 "
                          "operands, 3 MFMA per algorithmic product, f32 accumulate, fused modulated-adjacency/BN/ReLU/residual epilogue",
                 "f16": "gcn_hidden_chain_kernel<1, 8> (csrc/gcn_tile.hip): the 8 hidden convs chained in one launch (8-wave 192x128 tiles); plain f16 operands and f16 "
                        "activations, f32 accumulate, adjacency mix on the matrix cores, fused BN/ReLU/residual epilogue"}
        cls_of = {"f32": "hidden_f32", "f16x3": "chain_f16x3", "f16": "chain_f16"}
        kernels = {}
        for prec, cls in cls_of.items():
            pr = prof[cls]
            lp = prof.get({"f16x3": "loop_f16x3", "f16": "loop_f16"}.get(prec, ""), {"launches_per_call": 0})
            if not pr["launches_per_call"] and not lp["launches_per_call"]:
                continue
            if lp["launches_per_call"] and not pr["launches_per_call"]:
                # the one-launch loop: the hidden convs are not separate launches; the span of the persistent launch divided by its steps x
                # convs is an UPPER bound of the conv time (it also contains the input convs, output responses and per-body steps of the run)
                pr = dict(lp, launches_per_call=T - (prof["chain_f16x3"]["launches_per_call"] + prof["chain_f16"]["launches_per_call"] + prof["hidden_f32"]["launches_per_call"]))
            kd = pr["ms_per_call"] * 1e-3 / pr["launches_per_call"] / n_hidden        # seconds per conv, in situ (the job's own activations and shape)
            peak = PEAK_F32_MFMA_TFLOPS if prec == "f32" else PEAK_F16_MFMA_TFLOPS
            per_prod = 3 if prec == "f16x3" else 1
            kernels[prec] = {"bound": "mfma", "kernel": names[prec], "achieved": flops / kd / 1e12, "peak": peak, "unit": "TFLOP/s", "frac": flops / kd / 1e12 / peak,
                             "mfma_flops_per_algorithmic_flop": per_prod, "issued_mfma_frac": flops * per_prod / kd / 1e12 / peak,
                             "traffic": pmc_traffic(prec) if (B, S) == (256, 1) else None, "avg_launch_ms": kd * 1e3,
                             "avg_launch_ms_is": "per conv = (HIP-event span of the chained launch, on the launch stream, inside a real sampling call) / 8",
                             "launches_per_call": pr["launches_per_call"], "ms_per_call": pr["ms_per_call"], "flops_per_launch": flops,
                             "formula": f"virtual_bodies*(24*2*hid^2 + 24*24*hid)*2, virtual_bodies = {vbodies} body-passes per launch (SURVEY 8d, hoisted)"}
        dominant = max(kernels, key=lambda k: kernels[k]["ms_per_call"])            # the kernel the job spends most time in
        # HBM-bound kernels of the step (per-kernel GB/s against 8 TB/s), algorithmic bytes per launch
        act_b = 2 if prof["chain_f16"]["launches_per_call"] >= prof["chain_f16x3"]["launches_per_call"] else 4   # bytes per activation element of the majority of steps
        nb = S_l * B
        hbm = {}

        def hbm_entry(cls, kernel, bytes_per_launch, what):
            pr = prof[cls]
            if pr["launches_per_call"]:
                t = pr["ms_per_call"] * 1e-3 / pr["launches_per_call"]
                hbm[cls] = {"bound": "hbm", "kernel": kernel, "achieved": bytes_per_launch / t / 1e9, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                            "frac": bytes_per_launch / t / 1e9 / PEAK_HBM_GBS, "avg_launch_us": t * 1e6, "launches_per_call": pr["launches_per_call"],
                            "algorithmic_bytes_per_launch": bytes_per_launch, "bytes_are": what}
        hbm_entry("out_dot", "gcn_out_dot_kernel (output conv responses [rows,hid] x [hid,12])", rows * hid * act_b + rows * 12 * 4,
                  f"rows*hid*{act_b} B activations read + rows*12*4 B responses written, rows = {rows}")
        n_skin = prof["skin_input"]["launches_per_call"]
        steps_per_skin = T * n_groups / n_skin if n_skin else 0
        if n_skin and n_skin < T * n_groups:      # deferred skinning: one launch covers steps_per_skin steps
            hbm_entry("skin_input", f"skin_mfma_kernel (LBS skinning of {steps_per_skin:g} steps x {nb} bodies in one launch, docs/EXPERIMENTS.md 3.7)",
                      steps_per_skin * nb * (6890 * 3 * 4 + 21 * 3 * 4 + 24 * 12 * 4 + 2 * 224 * 2) + 19.3e6,
                      "per body-step 82,680 B vertices + extra joints + transforms + blend coefficients (SURVEY 8d) + SMPL constants 19.3 MB once per launch")
            hbm_entry("input", "gcn_input_kernel (hoisted input conv of the next step: rank-6 update + adjacency mix + BN + ReLU, split-f16 rows out)",
                      rows * hid * (act_b if act_b == 2 else 4) + nb * 2 * 2 * hid * 4 + nb * 576,
                      "rows*hid activation rows written + h_img / h_oth slices + x_t read")
        else:
            hbm_entry("skin_input", "skin_input_kernel (LBS skinning of step t + input conv of step t+1)",
                      nb * (6890 * 3 * 4 + 21 * 3 * 4 + 24 * 12 * 4 + 2 * 224 * 2) + 19.3e6 + rows * hid * (act_b if act_b == 2 else 4) + nb * 2 * 2 * hid * 4,
                      "per body 82,680 B vertices + extra joints + transforms + blend coefficients (SURVEY 8d: ~84.1 KB/body-step incl. the inputs) + SMPL "
                      "constants 19.3 MB once per launch + the next step's input rows written (rows*hid) + h_img / h_oth read")
        if prof.get("step_fused", {}).get("launches_per_call"):
            hbm_entry("step_fused", "step_fused_kernel (a step's output-conv responses + output mix + sampler update, then the NEXT step's hoisted input conv; one block per body)",
                      rows * hid * act_b + rows * hid * (act_b if act_b == 2 else 4) + nb * (2 * 2 * hid * 4 + 4 * 576),
                      "rows*hid activation rows read (last hidden conv) + rows*hid rows written (next input) + h_img / h_oth slices + x_t / noise / x0 / x_next")
            n_pose = prof["step_body"]["launches_per_call"]
            if n_pose:
                hbm_entry("step_body", f"pose_steps_kernel (rot6d + 24-joint chain + blend fragments of {T * n_groups / n_pose:g} steps x {nb:g} bodies in one launch; one wave per body-step)",
                          T * n_groups / n_pose * nb * (576 + 40 + 864 + 1152 + 288 + 2 * 224 * 2), "per body-step: x0 576 B + betas + R + A + joints + blend-coefficient fragments")
        else:
            hbm_entry("step_body", "step_body_kernel (output mix + sampler update + rot6d + 24-joint chain; one wave per body)",
                      nb * (2 * 24 * 12 * 4 + 5 * 576 + 40 + 864 + 1152 + 288 + 2 * 224 * 2),
                      "per body: responses 2,304 B + x_t / noise / x0 / x_next / pose6d 5 x 576 B + betas + R + A + joints + blend-coefficient fragments (latency-bound: 1 wave per body)")
        # collision guidance (SURVEY 8d / north_star "scene-point Chamfer/SDF guidance reduction"): the three kernels a guided step spends its time in
        guid = {}
        if prof["guidance"]["launches_per_call"]:
            def g_entry(cls, kernel, bound, work, peak, unit, what):
                pr = prof[cls]
                if pr["launches_per_call"]:
                    t = pr["ms_per_call"] * 1e-3 / pr["launches_per_call"]
                    div = 1e9 if unit == "GB/s" else 1e12
                    guid[cls] = {"bound": bound, "kernel": kernel, "achieved": work / t / div, "peak": peak, "unit": unit, "frac": work / t / div / peak,
                                 "avg_launch_us": t * 1e6, "launches_per_call": pr["launches_per_call"], "algorithmic_work_per_launch": work, "work_is": what}
            # the search: counted IN the kernel (one evaluation = 3 subtractions + 3 multiply-adds + the comparison: 8 flop) against the float32
            # vector-ALU peak - the bytes it moves (vertices in, gradient out, 0.2 GB per step at 1280 bodies) are not what bounds it
            n_g = prof["guid_nearest"]["launches_per_call"]
            g_entry("guid_nearest", "bbox / select / nearest_grid_kernel (proxy loss: nearest body vertex of every selected scene point over a 27-cell neighbourhood "
                    "of an LDS-resident cell grid, loss and d loss / d verts)",
                    "valu_f32", 8.0 * nearest_evals / max(n_g, 1), PEAK_F32_MFMA_TFLOPS, "TFLOP/s",
                    f"8 flop x {nearest_evals / max(n_g, 1) / max(nb, 1):.0f} distance evaluations per body and guided step (counted in the kernel); peak = the f32 vector rate "
                    "(157.3 TFLOP/s).  One wave per point: the fraction says how little arithmetic a point is (tens of candidates) next to what it takes to find them")
            if "guid_nearest" in guid:
                guid["guid_nearest"]["distance_evaluations_per_launch"] = nearest_evals / max(n_g, 1)
            g_entry("guid_skin_bwd", "skin_bwd_kernel (VJP of the skinning: d loss / d transforms, d loss / d blended rest pose)",
                    "hbm", nb * (6890 * 12 * 3 + 24 * 12 * 4), PEAK_HBM_GBS, "GB/s",
                    "per body: vertex gradient read + rest-pose gradient written + the forward's blended rest vertices read (3 x 82,680 B) + transform gradient "
                    "(upper bound: blocks whose vertices carry no gradient stop after the first read)")
            g_entry("guid_posefeat_bwd", "posefeat_bwd_mfma_kernel + posefeat_sum_kernel ([bodies, 20670] x [20670, 207] contraction with the pose-corrective basis)",
                    "mfma", nb * 2.0 * 20670 * 207, PEAK_F32_MFMA_TFLOPS, "TFLOP/s",
                    "2 x bodies x 20670 x 207 flop, exact-f32 MFMA (v_mfma_f32_32x32x2_f32; 224 of 207 columns issued)")
            guid["guided_step_total_us"] = prof["guidance"]["ms_per_call"] / prof["guidance"]["launches_per_call"] * 1e3
        flops_per_body = {"ddpm100": 183.8e9, "c2_ddim10": 35.5e9}.get(workload)  # SURVEY 8d, hoisted, with diffuse_fuse
        guid_steps = prof["guidance"]["launches_per_call"]
        if out["schedule"] is not None:
            out["schedule"].update({
                "measured_gain_dx0_dxt": fs.measure_gain(batch, timesteps=sorted({diffusion.timestep_map[-1], diffusion.timestep_map[T // 2], diffusion.timestep_map[T // 10], 0}, reverse=True)),
                "gain_note": "directional || x0(x_t + d) - x0(x_t) || / || d || through the product's denoiser, per ORIGINAL timestep; ~1 at low noise = early rounding errors are carried"})
        out.update({
            "roofline": kernels[dominant],
            "roofline_other_kernel": {k: v for k, v in kernels.items() if k != dominant} or None,
            "roofline_hbm": hbm,
            "roofline_guidance": guid or None,
            "end_to_end": None if not flops_per_body else {"algorithmic_flops_per_body": flops_per_body, "achieved_tflops": value / world * flops_per_body / 1e12,
                                                           "flops_frac_of_f16_dense_peak": value / world * flops_per_body / 1e12 / PEAK_F16_MFMA_TFLOPS},
            "breakdown_ms": {"encoders_and_projections_once": t_enc * 1e3, "per_call_total": dt / steps * 1e3,
                             "sampling_loop_by_launch_class": {k: v for k, v in prof.items() if v["launches_per_call"]}},
            "target": {"north_star_bodies_per_s": 10000,
                       "parity_ceiling_bodies_per_s": (PEAK_F16_MFMA_TFLOPS / 3) * 1e12 / flops_per_body if flops_per_body else None,
                       "note": "with every product as 3 MFMA the dense f16 peak allows 833 TFLOP/s algorithmic = the ceiling above, so >= 10k bodies/s is out of "
                               "reach at f32-grade arithmetic on every step"},
        })
        out.update(legs)
        if cpu_seconds > 0 and world == 1:
            out["cpu_baseline"] = cpu_baseline(n, rs, N, cpu_seconds * 0.6)
            out["cpu_baseline_hoisted"] = cpu_baseline(n, rs, N, cpu_seconds * 0.4, faithful=False) if T <= 100 else None
        else:
            out["cpu_baseline"] = None
        if guid_steps:
            out["guided_step_us"] = prof["guidance"]["ms_per_call"] / guid_steps * 1e3
        if "f32_grade_path_of_this_job" in legs:
            out["mpjpe_vs_f32_path_mm"] = legs["f32_grade_path_of_this_job"]["this_tier_vs_it"]["mpjpe_mm"]
        if workload == "ddpm100":
            out["references_measured_elsewhere"] = REFERENCES_MEASURED_ELSEWHERE
        return out
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="ddpm100", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=256, help="items per GPU")
    ap.add_argument("--scene-points", type=int, default=4096)
    ap.add_argument("--full", action="store_true",
                    help="measure everything beyond the headline too: comparison legs, the profiled call behind the roofline and per-kernel figures, "
                         "the encoder split, the CPU baselines, BASELINE configs 2-5 and the evaluation block.  Without it a run sets up, warms up, "
                         "times --steps calls, writes --dump-outputs and prints the line (roofline and cpu_baseline null)")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="with --full: time budget of the CPU baseline leg (0 = skip)")
    ap.add_argument("--no-lbs-every-step", action="store_true")
    ap.add_argument("--precision", default=None, choices=["f32", "f16x3", "f16"],
                    help="arithmetic of the hidden GCN convs (docs/EXPERIMENTS.md 3.2): f32 MFMA | split-f16 MFMA (f32-grade) | plain f16 (not parity-grade)")
    ap.add_argument("--weights", default="sensitive", choices=["sensitive", "insensitive"],
                    help="synthetic denoiser weights: 'sensitive' = trained-like (d x0 / d x_t follows the MMSE gain of a Gaussian prior, ~1 at low noise: "
                         "early rounding errors are CARRIED), 'insensitive' = the plain random network of rounds 1-2 (ignores x_t: errors are contracted)")
    ap.add_argument("--f16x3-last-steps", type=int, default=None,
                    help="explicit k instead of the calibration (e.g. the k a previous run printed): no calibration launches, so that under rocprofv3 "
                         "every launch of a chain kernel is a full-size one and the kernel-stats average equals roofline.avg_launch_ms * 8")
    ap.add_argument("--loop-bodies", type=int, default=None, help="EgoHMR.loop_bodies for this run (bodies per fused loop of a multi-sample batch)")
    ap.add_argument("--no-legs", action="store_true", help="with --full: skip the comparison legs (all-f16x3, f32, f16, other weight set)")
    ap.add_argument("--no-configs", action="store_true", help="with --full, default workload only: do not append BASELINE configs 2-5 (configs.c2_ddim10 ... configs.c5_volsmpl_ddpm1000)")
    ap.add_argument("--launch-check", action="store_true", help="only initialise the ranks, report the world size, exit (works without a GPU: gloo)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed call of the headline workload returned to DIR/<name>.npy (float32 / float64, at most 64 MB: a fixed "
                         "seeded sample of the rows above that); the inputs are seeded, so two builds can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")        # (here, before self_launch: rejected once, not by every rank it would start)
    rc = self_launch(sys.argv[1:])
    if rc is not None:
        sys.exit(rc)
    args.precision_given = args.precision or os.environ.get("EGOHMR_GCN_PRECISION")
    args.precision = args.precision_given or "f16x3"

    from egohmr_amd import dist as edist

    rank, world, local = edist.init_from_env()
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but {world} rank(s) were started (WORLD_SIZE={os.environ.get('WORLD_SIZE')}); "
                         "start it as `python bench.py --gpus N` (it launches the ranks) or under torch.distributed.run with --nproc-per-node N")
    if args.launch_check:
        # over gloo the ranks meet in all-reduces of a CPU tensor, not in barrier(): torch's barrier() looks up the accelerator, which starts the
        # HIP runtime (and opens the GPU) in every rank of a check that is meant to run without one
        gloo = world > 1 and torch.distributed.get_backend() == "gloo"

        def meet():
            if not gloo:
                edist.barrier()
                return int(torch.distributed.get_world_size()) if world > 1 else 1
            t = torch.ones(1)
            torch.distributed.all_reduce(t)
            return int(t.item())

        seen = meet()
        if rank == 0:
            print(json.dumps({"launch_check": True, "n_gpus": world, "n_ranks_seen": seen, "backend": torch.distributed.get_backend() if world > 1 else None}))
        meet()
        if world > 1:
            # tear the group down before the interpreter does: a gloo group left to the exit handlers aborted ranks now and then
            # ("terminate called without an active exception", SIGABRT after the line was printed)
            torch.distributed.destroy_process_group()
        return
    assert torch.cuda.is_available(), "bench.py needs a HIP device; there is no CPU fallback"
    ndev = torch.cuda.device_count()
    if ndev < world and not os.environ.get("EGOHMR_BENCH_SHARE_GPU"):
        raise SystemExit(f"bench.py: {world} ranks but only {ndev} HIP device(s) visible (set EGOHMR_BENCH_SHARE_GPU=1 for a functional run that shares devices)")
    local %= ndev
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    assert torch.cuda.current_device() == local, (torch.cuda.current_device(), local)   # every native call launches on the CURRENT device's stream

    out = measure(args, args.workload, args.steps, args.warmup, not args.no_legs, args.cpu_seconds, dev, rank, world, dump_dir=args.dump_outputs, full=args.full)
    # --full: BASELINE configs 2-5 inside the same line (3 timed calls each, 2 for config 5, no legs)
    if args.full and args.workload == "ddpm100" and world == 1 and not args.no_configs:
        keep = ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "dtype", "config", "schedule", "roofline", "roofline_hbm", "roofline_guidance", "breakdown_ms",
                "bodies_per_step", "body_denoising_steps_per_s", "guided_step_us", "mpjpe_vs_f32_path_mm", "f32_grade_path_of_this_job")
        subs = {}
        for wl, nsteps in (("c2_ddim10", 3), ("c3_guided", 3), ("c4_ddim50_s5", 3), ("c5_volsmpl_ddpm1000", 2)):
            sub = measure(args, wl, nsteps, 1, False, 0.0, dev, rank, world, full=True)
            subs[wl] = {k: sub[k] for k in keep if k in sub}
            subs[wl]["gcn_precision"] = sub["config"]["gcn_precision"]
            subs[wl]["encoder_precision"] = sub["config"]["encoder_precision"]          # (C5 names the fp16 tier: its encoders run hi-only too)
            if sub["config"].get("guidance_weight") is not None:
                subs[wl]["guidance_weight"] = sub["config"]["guidance_weight"]          # (C5 is timed at 0.5, not the VolSMPL default 30: see w_guid)
        out["configs"] = subs
        # the evaluation block's kernels at config 3's shape (128 items x 10 samples, 20 000-point scenes as the reference's data): the contact score's
        # nearest-neighbour search against the f32 vector rate, V2V / MPJPE / PA-MPJPE / diversity (csrc/metrics.hip, csrc/eval.hip; test_egohmr.py:399-505)
        try:
            sys.path.insert(0, os.path.join(REPO, "tools"))
            import bench_metrics
            out["evaluation_block"] = bench_metrics.measure(128, 10, 20000, reps=3, dev=dev)
        except Exception as e:                                  # (a measurement aid: never lets the bench line fail)
            out["evaluation_block"] = {"error": repr(e)}
    if rank == 0:
        emit(out)
    edist.barrier()


if __name__ == "__main__":
    main()
