"""CPU: the LAST stdout line of bench.py is one compact strict-JSON object (the driver parsed round 3's 9 KB line and not
round 4's 24 KB one).  `bench.compact_line` is a pure function of the detail dict, so it is tested here on canned detail objects: the committed
default line of round 4 (24 KB), a worst case with every string blown up and non-finite numbers, and an N > 1 line."""
import copy
import glob
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
import bench  # noqa: E402

CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                 "roofline", "cpu_baseline")


def _canned():
    with open(os.path.join(REPO, "profiles", "r04e_bench_default_line.json")) as f:
        return json.load(f)


def _strict(line):
    def bad(c):
        raise ValueError(c)
    return json.loads(line, parse_constant=bad)          # NaN / Infinity / -Infinity are not JSON


def test_compact_line_of_the_round4_detail_object():
    d = _canned()
    assert len(json.dumps(d)) > 20000                     # the object the driver did not parse
    line = bench.compact_line(d)
    assert "\n" not in line and len(line) < 4096
    o = _strict(line)
    for k in CONTRACT_KEYS:
        assert k in o, k
    assert o["metric"] == d["metric"] and abs(o["value"] - d["value"]) < 1e-2 * d["value"]
    r = o["roofline"]
    assert set(r) >= {"bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms"}
    assert r["bound"] == "mfma" and r["kernel"].startswith("gcn_hidden_chain_kernel")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    # one launch = the 8 chained convs: the launch duration is what rocprofv3's per-kernel average shows
    assert abs(r["avg_launch_ms"] - 8 * d["roofline"]["avg_launch_ms"]) < 1e-2
    assert abs(r["flops_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e12 - r["achieved"]) < 0.01 * r["achieved"]
    c = o["cpu_baseline"]
    assert set(c) == {"value", "unit", "cores", "kind", "sample"} and c["kind"] in ("port", "reference") and len(c["sample"]) <= 200
    assert set(o["configs"]) == {"c2_ddim10", "c3_guided"}
    for sub in o["configs"].values():
        assert set(sub) >= {"value", "ms_per_step", "roofline_frac"}
    assert o["config"]["name"] == "ddpm100" and "workload" in o["config"]


def test_compact_line_worst_case_still_fits_and_is_strict_json():
    d = _canned()
    d["value"] = float("nan")
    d["roofline"]["traffic"] = float("inf")
    d["dtype"] = "x" * 5000
    d["config"]["workload"] = "w" * 5000
    d["cpu_baseline"]["sample"] = "s" * 5000
    d["roofline"]["kernel"] = "k" * 3000
    for i in range(40):                                   # many sub-configs: optional blocks are dropped until the line fits
        d["configs"][f"extra_{i}"] = copy.deepcopy(d["configs"]["c2_ddim10"])
    line = bench.compact_line(d)
    assert len(line) <= bench.COMPACT_LIMIT
    o = _strict(line)
    assert o["value"] is None and o["roofline"]["traffic"] is None
    for k in CONTRACT_KEYS:
        assert k in o, k


def test_compact_line_multi_gpu_keys():
    d = _canned()
    d.update(n_gpus=8, n_ranks_seen=8, per_rank_bodies_per_s=[2000.123456] * 8, all_gather_ms=0.1234567, cpu_baseline=None)
    d.pop("configs")
    o = _strict(bench.compact_line(d))
    assert o["n_gpus"] == 8 and o["n_ranks_seen"] == 8 and len(o["per_rank_bodies_per_s"]) == 8 and o["all_gather_ms"] is not None
    assert o["cpu_baseline"] is None and len(json.dumps(o)) < 4096


def test_compact_line_of_a_plain_run():
    """a run without --full measures the headline alone: its detail object has no roofline, legs, CPU baseline, breakdown or configs, and the
    line still carries every contract key (roofline and cpu_baseline null) with the headline's figures unchanged"""
    d = _canned()
    plain = {k: d[k] for k in ("metric", "value", "unit", "n_gpus", "n_ranks_seen", "per_rank_bodies_per_s", "all_gather_ms", "multi_gpu_note", "steps",
                               "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "schedule")}
    plain.update(full=False, bodies_per_step=256, body_denoising_steps_per_s=d["value"] * 100)
    o = _strict(bench.compact_line(plain))
    for k in CONTRACT_KEYS:
        assert k in o, k
    assert o["roofline"] is None and o["cpu_baseline"] is None
    assert not {"configs", "legs", "roofline_hbm", "evaluation_block", "encoders_ms"} & set(o)
    full = _strict(bench.compact_line(d))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert o[k] == full[k], k


def test_every_committed_round5_line_is_compact():
    """builder-run compact lines kept under profiles/ (r05*_line.json) obey the same bound"""
    for p in glob.glob(os.path.join(REPO, "profiles", "r05*_line.json")):
        with open(p) as f:
            txt = f.read().strip()
        assert len(txt) < 4096, p
        o = _strict(txt)
        assert o["roofline"] and math.isfinite(o["value"]), p


def _fake_outs(S, B, V=50):
    """result dicts shaped like FusedSampler.run_samples' (CPU tensors stand in for the device ones)"""
    g = torch.Generator().manual_seed(1)
    outs = []
    for _ in range(S):
        outs.append({"sample": torch.randn(B, 144, generator=g), "pred_xstart": torch.randn(B, 144, generator=g),
                     "other_outputs": {"pred_vertices": torch.randn(B, V, 3, generator=g),
                                       "pred_smpl_params": {"betas": torch.randn(B, 10, generator=g).double(), "body_pose": torch.randn(B, 23, 3, 3, generator=g)},
                                       "vis": torch.ones(B, 24, dtype=torch.bool), "note": "not an array"}})
    return outs, torch.randn(S * B, 226, generator=g)


def test_output_arrays_names_and_dtypes():
    outs, gathered = _fake_outs(1, 6)
    a = bench.output_arrays(outs, gathered)
    assert set(a) == {"gathered_smpl_params", "sample", "pred_xstart", "other_outputs.pred_vertices", "other_outputs.pred_smpl_params.betas",
                      "other_outputs.pred_smpl_params.body_pose", "other_outputs.vis"}
    assert a["other_outputs.pred_smpl_params.betas"].dtype == np.float64 and a["other_outputs.vis"].dtype == np.float32
    np.testing.assert_array_equal(a["other_outputs.pred_vertices"], outs[0]["other_outputs"]["pred_vertices"].numpy())
    np.testing.assert_array_equal(a["gathered_smpl_params"], gathered.numpy())
    outs, gathered = _fake_outs(3, 6)
    a = bench.output_arrays(outs, gathered)
    assert {"s0.sample", "s2.other_outputs.pred_vertices"} <= set(a) and "sample" not in a


def test_output_arrays_above_the_limit_keep_the_same_seeded_rows(tmp_path):
    outs, gathered = _fake_outs(2, 40)
    full = bench.output_arrays(outs, gathered, limit=1 << 30)
    limit = sum(x.nbytes for x in full.values()) // 4
    a = bench.output_arrays(outs, gathered, limit=limit)
    b = bench.output_arrays(outs, gathered, limit=limit)
    assert sum(x.nbytes for x in a.values()) <= limit
    assert a.keys() == full.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
        assert a[k].shape[1:] == full[k].shape[1:] and 1 <= a[k].shape[0] < full[k].shape[0]
    # rows are a sorted subset of the full output, the same ones for every array of the same length
    rows = [i for i in range(40) if any((full["s0.sample"][i] == r).all() for r in a["s0.sample"])]
    np.testing.assert_array_equal(a["s1.other_outputs.pred_vertices"], full["s1.other_outputs.pred_vertices"][rows])
    bench.dump_outputs(str(tmp_path / "d"), a)
    for k, v in a.items():
        np.testing.assert_array_equal(np.load(tmp_path / "d" / f"{k}.npy"), v)


def test_bench_rejects_zero_steps():
    """once, in the process it was given to: `--gpus 8 --steps 0` starts no ranks"""
    import subprocess
    for extra in ([], ["--gpus", "8"]):
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and r.stderr.count("--steps must be at least 1") == 1, r.stderr[-2000:]
        assert "launching" not in r.stderr


def test_output_arrays_cap_is_hard():
    """single-row arrays are never sampled: if they alone exceed the cap, output_arrays refuses instead of writing more"""
    big = {"sample": torch.zeros(1, 1000)}
    with pytest.raises(ValueError):
        bench.output_arrays([big], torch.zeros(1, 226), limit=2000)
