"""CPU: the host side of the two-term split-f16 tier - the second ladder search of the schedule calibration, how EgoHMR.f16x2_steps resolves to
ehm_sample_desc.twoterm_steps, the descriptor's ctypes mirror against the header, and the register / LDS budget of the two new kernels."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fs(**model):
    from egohmr_amd.fused import FusedSampler
    fs = object.__new__(FusedSampler)
    fs._model_ref = [SimpleNamespace(**{"gcn_precision": "f16x3", "f16x3_last_steps": "auto", "f16x2_steps": "auto", **model})]
    fs._sched_cache = {}
    return fs


def test_ladder_search_on_a_monotone_error():
    """err(m) of the schedule [f16 x (T - k)][two-term x (k - m)][three-term x m] falls with m: the search returns j = k - m for the smallest ladder entry
    m whose error passes on draw A and, from there upwards, on draw B; m = k (j = 0) is never evaluated - it passes by definition."""
    from egohmr_amd.fused import FusedSampler as F
    T = 100
    ladder = F._k_ladder(T)
    assert ladder[-1] == T and ladder == sorted(set(ladder)) and ladder[0] == 2
    calls = []

    def err(scale):
        def f(m):
            calls.append(m)
            assert m < k, "the error of the all-three-term schedule is 0 by definition and must not be measured"
            return scale * (k - m) / k                      # monotone: more three-term steps, less error
        return f
    for k in (T, 50, 28):
        sub = [m for m in ladder if m < k]
        # bar 0.5: passes where (k - m) / k <= 0.5
        want_m = min(m for m in sub + [k] if m == k or (k - m) / k <= 0.5)
        assert F.pick_two_term(ladder, k, err(1.0), err(1.0), 0.5) == k - want_m
        # draw B twice as bad: the climb moves m up until B passes too
        want_b = min(m for m in sub + [k] if m == k or 2.0 * (k - m) / k <= 0.5)
        assert F.pick_two_term(ladder, k, err(1.0), err(2.0), 0.5) == k - want_b
        assert want_b >= want_m
        # nothing passes: j = 0, today's schedule
        assert F.pick_two_term(ladder, k, err(1e9), err(1e9), 0.5) == 0
        # everything passes: all but the ladder's first entry two-term (the last steps always stay three-term)
        assert F.pick_two_term(ladder, k, err(0.0), err(0.0), 0.5) == k - ladder[0]
    # k at the ladder's floor: no candidate below it
    assert F.pick_two_term(ladder, ladder[0], err(0.0), err(0.0), 0.5) == 0
    assert len(calls) < 200                                   # bisection + climb, not a sweep per call


def test_f16x2_steps_resolves_like_the_issue_says():
    T = 100
    fs = _fs()
    key = ("some", "key")
    assert fs.twoterm_steps(T, 0, key=key) == 0                                     # 'auto' without a calibration
    fs._sched_cache[key] = {"k": 100, "two_term_steps": 33}
    assert fs.twoterm_steps(T, 0, key=key) == 33
    assert fs.twoterm_steps(T, 90, key=key) == 10                                   # never more than the split steps
    fs._sched_cache[key] = {"k": 100}                                               # an info dict measured before the tier existed
    assert fs.twoterm_steps(T, 0, key=key) == 0
    fs._sched_cache[key] = {"k": 100, "two_term_steps": 33}
    for explicit in (None, 100, 8):                                                 # an explicit k (or None) leaves j = 0 ...
        fs.model.f16x3_last_steps = explicit
        assert fs.twoterm_steps(T, 0, key=key) == 0
        fs.model.f16x2_steps = 5                                                    # ... unless j is explicit too
        assert fs.twoterm_steps(T, 0, key=key) == 5
        assert fs.twoterm_steps(T, 97, key=key) == 3
        fs.model.f16x2_steps = "auto"
    fs.model.f16x3_last_steps = "auto"
    fs.model.f16x2_steps = 0
    assert fs.twoterm_steps(T, 0, key=key) == 0
    fs.model.f16x2_steps, fs.model.gcn_precision = 5, "f16"
    assert fs.twoterm_steps(T, 0, key=key) == 0
    fs.model.gcn_precision = "f32"
    assert fs.twoterm_steps(T, 0, key=key) == 0


def test_sample_desc_mirror_matches_the_header(tmp_path):
    """sizeof(ehm_sample_desc) and the offset of its appended field, from a two-line C program, against _lib.SampleDesc."""
    from egohmr_amd import _lib
    src = tmp_path / "desc.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "egohmr_hip.h"\n'
                   'int main(void) { printf("%d %d %d %d\\n", (int)sizeof(ehm_sample_desc), (int)offsetof(ehm_sample_desc, twoterm_steps), '
                   "(int)EHM_PREC_F16X2, (int)EHM_PROF_N); return 0; }\n")
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    size, off, prec, nprof = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split())
    assert size == ctypes.sizeof(_lib.SampleDesc)
    assert off == _lib.SampleDesc.twoterm_steps.offset and _lib.SampleDesc._fields_[-1][0] == "twoterm_steps"      # appended: the older fields keep their offsets
    assert _lib.SampleDesc().twoterm_steps == 0                                                                    # a descriptor that never sets it: tier off
    from egohmr_amd.fused import PRECISIONS
    assert prec == PRECISIONS["f16x2"] == 3
    assert nprof == len(_lib.PROF_CLASSES) and _lib.PROF_CLASSES[-1] == "chain_f16x2" and _lib.PROF_CLASSES.index("chain_f16x3") == 1


def test_two_term_kernels_keep_two_blocks_per_cu():
    """gcn_hidden_chain_kernel<2, 4> and gcn_hidden_tile_kernel<2>: 80 KiB of LDS, at most 256 registers, no scratch (tests/test_occupancy_cpu.py's
    conditions for the tile engines)."""
    pytest.importorskip("msgpack")
    from egohmr_amd import _lib
    from test_occupancy_cpu import _device_kernels, _regs
    _lib.build()
    ks = {n: k for n, k in _device_kernels(_lib.LIB_PATH).items() if "gcn_hidden_chain_kernelILi2ELi4E" in n or "gcn_hidden_tile_kernelILi2E" in n}
    assert len(ks) == 2, sorted(ks)
    for name, k in ks.items():
        assert k[".max_flat_workgroup_size"] == 256, name
        assert k[".group_segment_fixed_size"] <= 80 * 1024, (name, k[".group_segment_fixed_size"])
        assert _regs(k) <= 256, (name, k[".vgpr_count"], k.get(".agpr_count", 0))
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
