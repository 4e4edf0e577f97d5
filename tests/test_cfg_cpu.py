"""CPU: classifier-free guidance scales on the visibility fuse - the table of EgoHMR.fuse_scales and the wrapper's composition, the rule for which
items need the masked pass, the reference of the GPU tests (tests/cfg_ref.py: CFGOracle) against itself, against EgoHMROracle and against what
the reference's own forward gives (tests/golden/g22_cfg_passes.npz), the schedule key, and the C ABI: the new symbols and the two descriptors."""
import ctypes
import itertools
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cfg_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "g22_cfg_passes.npz")


def _model(**attrs):
    """The scale helpers of EgoHMR on a bare namespace (no device, no weights)."""
    from egohmr_amd.model import EgoHMR

    class M(SimpleNamespace):
        fuse_scales = EgoHMR.fuse_scales
        sampling_scales = EgoHMR.sampling_scales
        fuse_passes = staticmethod(EgoHMR.fuse_passes)
    return M(**{"diffuse_fuse": True, "guidance_param": 0.0, "guidance_param_visible": 1.0, "outer_guidance": 1.0, **attrs})


# ---------------------------------------------------------------------------------------------- the table
def test_fuse_scales_table():
    m = _model()
    assert m.fuse_scales() == (1.0, 0.0) and m.fuse_passes(m.fuse_scales()) == 2          # the reference's fuse
    assert m.fuse_scales(eval_with_uncond=False) == (1.0, 1.0) and m.fuse_passes((1.0, 1.0)) == 1
    assert m.fuse_scales(force_mask=True) == (0.0, 0.0) and m.fuse_scales(False, True, outer=7.0) == (0.0, 0.0)
    m.guidance_param, m.guidance_param_visible = 0.5, 2.5
    assert m.fuse_scales() == (2.5, 0.5) and m.fuse_scales(outer=2.0) == (5.0, 1.0)
    assert m.fuse_scales(eval_with_uncond=False, outer=2.0) == (5.0, 5.0)
    n = _model(diffuse_fuse=False, guidance_param=0.5)
    assert n.fuse_scales() == (1.0, 1.0) and n.fuse_passes(n.fuse_scales()) == 1          # no fuse: one pass, as before
    assert n.fuse_scales(outer=2.5) == (2.5, 2.5) and n.fuse_passes((2.5, 2.5)) == 2       # ... under a wrapper: two
    assert n.fuse_scales(force_mask=True) == (0.0, 0.0)
    assert all(isinstance(v, float) for v in m.fuse_scales() + n.fuse_scales())
    # one pass exactly when both scales are 1.0
    for s in itertools.product((0.0, 0.5, 1.0, 2.5, -0.5), repeat=2):
        assert m.fuse_passes(s) == (1 if s == (1.0, 1.0) else 2)


@pytest.mark.parametrize("attr,bad", [("guidance_param", math.nan), ("guidance_param", math.inf), ("guidance_param_visible", -math.inf),
                                      ("guidance_param_visible", 1e39), ("outer_guidance", math.nan)])
def test_non_finite_scales_raise(attr, bad):
    m = _model(**{attr: bad})
    with pytest.raises(ValueError):
        m.sampling_scales()
    with pytest.raises(ValueError):
        _model().fuse_scales(outer=math.nan)


def test_wrapper_holds_the_model_sets_the_outer_scale_and_delegates():
    from egohmr_amd import ClassifierFreeSampleModel
    from egohmr_amd.model import EgoHMR

    class Inner(torch.nn.Module):
        fuse_scales, sampling_scales = EgoHMR.fuse_scales, EgoHMR.sampling_scales

        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(2, 2)
            self.diffuse_fuse, self.guidance_param, self.guidance_param_visible, self.outer_guidance = True, 0.25, 1.5, 1.0
            self.seen = []

        def forward(self, batch, timesteps):
            self.seen.append(self.sampling_scales())
            return {"pred_x_start": batch}

        def compute_loss(self, *a):
            return "inner compute_loss"

    inner = Inner()
    w = ClassifierFreeSampleModel(inner)
    assert w.guidance_param == 2.5 and w.model is inner and isinstance(w, torch.nn.Module)
    w = ClassifierFreeSampleModel(inner, guidance_param=2.0)
    assert w(3, None) == {"pred_x_start": 3} and inner.seen == [(3.0, 0.5)]              # s_vis = w * guidance_param_visible, s_inv = w * model.guidance_param
    assert inner.outer_guidance == 1.0                                                   # ... for the call only
    with w.guidance_scope():
        w(3, None)                                                                       # (a sampler's step around the forward: the scale is applied once)
    assert inner.seen[-1] == (3.0, 0.5) and inner.outer_guidance == 1.0
    assert ClassifierFreeSampleModel(w, 0.5)(3, None) and inner.seen[-1] == (1.5, 0.25)  # a wrapper around a wrapper multiplies, as U + w (F - U) does
    assert w.compute_loss() == "inner compute_loss" and w.diffuse_fuse is True and w.lin is inner.lin
    assert [id(p) for p in w.parameters()] == [id(p) for p in inner.parameters()]
    with pytest.raises(AttributeError):
        w.no_such_attribute


# ---------------------------------------------------------------------------------------------- the need rule
def test_need_rule_against_a_loop_over_joints():
    from egohmr_amd.fused import item_need, need_all_items, pass_map
    g = torch.Generator().manual_seed(5)
    vis = torch.rand(40, 24, generator=g) < 0.9
    vis[:7] = True                                                  # some items see every joint
    vis[7] = False
    vis[:, 0] = True                                                # the forced joint: every item sees at least one (egohmr.py:187)
    for s_vis, s_inv in itertools.product((1.0, 0.0, 0.5, 2.5, -0.5), repeat=2):
        if (s_vis, s_inv) == (1.0, 1.0):
            continue                                                # one pass: no map
        want = [any((s_vis if vis[b, j] else s_inv) != 1.0 for j in range(24)) for b in range(vis.shape[0])]
        got = item_need(vis, need_all_items((s_vis, s_inv)))
        assert got.tolist() == want, (s_vis, s_inv)
        if s_vis != 1.0:
            items, slot, n = pass_map(got)                          # every item: the identity map
            assert n == vis.shape[0] and slot.tolist() == list(range(n)) == items.tolist()
    assert item_need(vis, False).tolist() == (~vis.all(dim=1)).tolist()      # s_vis == 1: the pruning rule as it was


def test_prepared_batch_hands_its_need_rule_on():
    from test_prepared_cpu import _prepared
    from egohmr_amd.fused import pass_map
    st, need = _prepared(11, 0.3)
    assert st.need_all is False and st.with_need(False) is st
    al = st.with_need(True)
    assert al.need_all is True and al.num_masked == 11 and al.mask_slot.tolist() == list(range(11)) and al.h_img is st.h_img
    assert al.take(torch.tensor([3, 3, 0])).num_masked == 3 and al.take(4).need_all and al.tile(2).need_all
    assert al.tile(2).mask_slot.tolist() == list(range(22))
    back = al.with_need(False)
    items, slot, n = pass_map(need)
    assert back.num_masked == n and torch.equal(back.mask_slot, slot) and torch.equal(back.mask_items, items) and not back.need_all


# ---------------------------------------------------------------------------------------------- the reference of the GPU tests
@pytest.fixture(scope="module")
def case():
    b_np, x_t = R.make_batch3()
    batch = R.to_torch(b_np)
    batch["x_t"] = torch.from_numpy(x_t)
    return batch, torch.full((R.B3,), R.TIMESTEP, dtype=torch.long)


def _x0(oracle, case, s_vis, s_inv):
    oracle.s_vis, oracle.s_inv = float(s_vis), float(s_inv)
    with torch.no_grad():
        return oracle(case[0], case[1])["pred_x_start"].reshape(R.B3, 24, 6)


def test_wrapper_composition_equals_the_per_joint_rule_in_float64(case):
    """U + w (F - U) from three oracle calls = the rule with s_vis = w * guidance_param_visible, s_inv = w * guidance_param."""
    o = R.make_oracle(torch.float64)
    for gv, gi, w in ((1.0, 0.0, 2.5), (1.5, 0.25, 2.0), (1.0, 0.5, -0.5)):
        F, U = _x0(o, case, gv, gi), _x0(o, case, 0.0, 0.0)
        d = (U + w * (F - U) - _x0(o, case, w * gv, w * gi)).abs().max().item()
        print(f"gv {gv} gi {gi} w {w}: max |U + w (F - U) - rule| = {d:.3e}")
        assert d <= 1e-12
    # ... and without the fuse (one scale on all joints): F = c
    c = _x0(o, case, 1.0, 1.0)
    assert (U + 2.5 * (c - U) - _x0(o, case, 2.5, 2.5)).abs().max().item() <= 1e-12


def test_cfg_oracle_at_one_zero_is_the_oracle_bit_for_bit(case):
    from oracle.model import EgoHMROracle
    for dt in (torch.float32, torch.float64):
        a = R.make_oracle(dt)
        b = R.make_oracle(dt, cls=EgoHMROracle)
        with torch.no_grad():
            oa, ob = a(case[0], case[1]), b(case[0], case[1])
        for k in ("pred_x_start", "pred_vertices", "pred_keypoints_3d", "pred_pose_6d", "pred_keypoints_2d_full"):
            assert torch.equal(oa[k], ob[k]), (dt, k)
        # (1, 1) = the conditional output alone = an oracle without the fuse
        n = R.make_oracle(dt, cls=EgoHMROracle, diffuse_fuse=False)
        with torch.no_grad():
            assert torch.equal(_x0(a, case, 1.0, 1.0).reshape(R.B3, -1), n(case[0], case[1])["pred_x_start"])


def test_golden_covered_joints_against_cfg_oracle_float32(case):
    """What the reference's own forward pins of c and u (three unmodified calls) against CFGOracle float32: (|s| + |1 - s|) * 5e-5."""
    g = np.load(GOLDEN)
    vis, cov = g["vis"], g["covered"]
    assert (cov.sum(1) >= 20).all() and vis[0].all() and 0 < vis[1].sum() < 24 and vis[2].sum() == 24 - cov[2].sum()
    assert np.array_equal(g["x_t"], case[0]["x_t"].numpy())
    c, u = g["c"].astype(np.float64), g["u_free"].astype(np.float64)
    o = R.make_oracle(torch.float32)
    for s_vis, s_inv in [(1.0, 0.0)] + R.SCALE_PAIRS:
        x0 = _x0(o, case, s_vis, s_inv).numpy().astype(np.float64)
        assert np.array_equal(case[0]["vis_mask_smpl"].numpy(), vis)
        for name, sel, s in (("visible", vis & cov, s_vis), ("invisible", ~vis & cov, s_inv)):
            want = u + s * (c - u)
            d = np.abs(x0 - want)[sel].max() if sel.any() else 0.0
            print(f"scales ({s_vis}, {s_inv}) {name}: {int(sel.sum())} joints, max |d| = {d:.3e}, bar {R.bar(s):.3e}")
            assert d <= R.bar(s), (s_vis, s_inv, name)


# ---------------------------------------------------------------------------------------------- schedule key
def test_schedule_key_differs_between_scale_pairs():
    from egohmr_amd.fused import FusedSampler
    fs = object.__new__(FusedSampler)
    m = _model(guide_reduction="mean", guide_all_points=False, schedule_tol=1e-5, f16x2_steps="auto")
    fs._model_ref, fs._pk, fs._ck = [m], (lambda: ("weights",)), (lambda: ("cond weights",))
    d = SimpleNamespace(timestep_map=[0, 10, 20], original_num_steps=50, num_timesteps=3)
    keys = {}
    for pair in [(1.0, 0.0), (1.0, 0.5), (2.5, 0.0), (2.5, 0.5)]:
        m.guidance_param_visible, m.guidance_param = pair
        keys[pair] = fs.schedule_key(d, True, 0)
        assert fs.schedule_key(d, True, 0) == keys[pair]
    assert len(set(keys.values())) == 4
    m.guidance_param_visible, m.guidance_param, m.outer_guidance = 1.0, 0.2, 2.5          # a wrapper's scale: the effective pair counts
    assert fs.schedule_key(d, True, 0) == keys[(2.5, 0.5)]


# ---------------------------------------------------------------------------------------------- C ABI
def test_new_symbols_are_exported_and_refuse_bad_arguments():
    from egohmr_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert hasattr(L, "ehm_gcn_output_layer_cfg") and "ehm_gcn_output_layer_cfg" in _lib.PROTOTYPES
    assert L.ehm_gcn_output_layer_cfg(None, None, None, None, 3, 2, 1.0, 0.0, None) == -22
    assert b"bad argument" in L.ehm_last_error()
    assert hasattr(L, "ehm_gcn_set_fuse_scales") and "ehm_gcn_set_fuse_scales" in _lib.PROTOTYPES
    assert L.ehm_gcn_set_fuse_scales(None, 1, 2.5, 0.5) == -22


def test_descriptor_layouts_match_the_header(tmp_path):
    """sizeof and every field offset of ehm_sample_desc and ehm_item_prep_desc, from a compiled C program, against the ctypes mirrors; the new fields
    field of ehm_item_prep_desc is the last one and a zero-initialised descriptor is neutral."""
    from egohmr_amd import _lib
    pairs = [("ehm_sample_desc", _lib.SampleDesc), ("ehm_item_prep_desc", _lib.ItemPrepDesc)]
    body = []
    for cname, cls in pairs:
        body.append(f'  printf("%d", (int)sizeof({cname}));')
        body += [f'  printf(" %d", (int)offsetof({cname}, {n}));' for n, _ in cls._fields_]
        body.append('  printf("\\n");')
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "egohmr_hip.h"\nint main(void) {\n' + "\n".join(body) + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.strip().splitlines()
    for (cname, cls), line in zip(pairs, lines):
        nums = list(map(int, line.split()))
        assert nums[0] == ctypes.sizeof(cls), cname
        assert nums[1:] == [getattr(cls, n).offset for n, _ in cls._fields_], cname
    # ehm_sample_desc keeps its layout (the scales are a setting of the handle: ehm_gcn_set_fuse_scales); ehm_item_prep_desc grew at its end
    assert _lib.SampleDesc._fields_[-1][0] == "twoterm_steps" and ctypes.sizeof(_lib.SampleDesc) == 14 * 4
    assert _lib.ItemPrepDesc._fields_[-1][0] == "need_all" and _lib.ItemPrepDesc._fields_[-2][0] == "B" and _lib.ItemPrepDesc().need_all == 0


def test_guidance_kernels_do_not_spill():
    """The guidance instantiations of step_fused_kernel (template argument CFG = true), the per-step body kernel and the output mix: no scratch, the
    register budget of their launch bounds (tests/test_occupancy_cpu.py's reader of the code objects)."""
    pytest.importorskip("msgpack")
    from egohmr_amd import _lib
    from test_occupancy_cpu import _device_kernels, _regs
    _lib.build()
    ks = _device_kernels(_lib.LIB_PATH)
    fused = {n: k for n, k in ks.items() if "step_fused_kernel" in n and "ELb1EEEv" in n}
    assert len(fused) == 12, sorted(fused)                      # 2 input formats x 3 output formats x {1024, 256} threads
    for n, k in fused.items():
        assert k[".max_flat_workgroup_size"] in (256, 1024) and _regs(k) <= 128 and k[".private_segment_fixed_size"] == 0, (n, k)
        assert k[".group_segment_fixed_size"] <= (40 * 1024 if k[".max_flat_workgroup_size"] == 256 else 160 * 1024), n
    for pat in ("step_body_cfg_kernel", "gcn_out_mix_kernelILb1E"):
        (k,) = [k for n, k in ks.items() if pat in n]
        assert k[".private_segment_fixed_size"] == 0 and _regs(k) <= 128, pat
