"""GPU (MI355X): the SMPL VJP entries of csrc/guidance.hip - ehm_smpl_backward, ehm_smpl_backward_ordered, ehm_smpl_backward_rot6d, the seven kernels
behind them - through the C ABI (not the autograd wrapper), against the staged float64 restatement of tests/smpl_vjp_ref.py under its derived bound (the
module docstring there counts every constant against a source line; tests/test_smpl_vjp_ref_cpu.py shows on the CPU that the restatement equals float64
autograd and that the bound tells nine subtly broken kernels from the faithful one).  No comparison against float64 here uses a bare number: every one
is error <= bound, and the largest error / bound is printed.

Every output (grotmats, gbetas, gpose6d) sits between canary guards and is pre-filled with a sentinel; the caller-owned workspace is allocated at
exactly *_workspace_bytes between guards and filled with 0xFF bytes (NaN) before every call.  After each call the guards of outputs and workspace are
intact and no sentinel is left in a requested output.  The float64 reference is computed once per case on the CPU.

Shapes - the smallest that reach each path (smpl_vjp_ref.cases()):
  V = 1, 3, 4, 7, 8, 13   3 V % 8 = 3, 1, 4, 5, 0, 7: the partial last 8-k group of posefeat_bwd_mfma_kernel in the h = 0 half-wave only (<= 4), in both
                          (> 4), absent (0); fewer than 32 groups, so empty K chunks; one partial vertex tile; 3 V < 256 leaves lanes of shape_bwd_kernel idle
  V = 86                  33 groups: every K chunk holds one
  V = 255, 256, 257       the 256-vertex tile edge of the two skinning kernels
  V = 2305                10 vertex tiles over 16 slots: the second round of `(k / b_groups) * 8 + xcd` and 6 dead slots
  B = 1, 3, 4, 5, 7, 8, 9     shape_bwd_kernel's 4-body blocks, the skinning kernels' 8-body groups
  B = 31, 32, 33, 65          the pose-feature kernel's 32-body tiles, three tiles
every V at B in {1, 9, 33}, every B at V in {7, 257}, V = 2305 at B in {9, 65}.  Cotangent families (smpl_vjp_ref.cotangents): dense, vertices only
(gjoints NULL), joints only (gverts NULL), one non-zero vertex of one body (every other block takes the `any_grad` exit), a +0.0 body and a -0.0 body
(exact zeros out), the 24 posed joints only, the extra joints only.  Assets: sparse and dense weights, n_extra 5 (ids V - 1, 0, V - 1 again: a repeated
pick) and 0 (jstride 72).  Input families normal, betas5, identity.

Out of scope: the `vposed` path of skin_bwd_kernel (the forward's blended rest vertices read back instead of recomputed) is reachable only inside
ehm_sample_loop; test_guidance_gradient_inside_the_sample_loop_vs_fp64 (tests/test_gpu_collision.py) covers it.

Measured on an MI355X (largest error / bound per group; a figure above 1 would be a finding):
  (grotmats / gbetas; where one pair is given, both routes agree to the digits shown)
  shape matrix, 48 (V, B), dense cotangents    0.062 / 0.004 (V 3, B 33 / V 13, B 33); V = 2305: 0.002 / 0.000
  vertices only 0.015 / 0.002;  joints only 0.058 / 0.003;  the 24 posed joints only 0.078 / 0.003;  the extra joints only: atomic 0.024 / 0.002,
  ordered 0.042 / 0.004;  one non-zero vertex 0.048 / 0.008;  a +0.0 and a -0.0 body 0.017 / 0.002, their rows exact zeros
  dense weights 0.029 / 0.002;  n_extra = 0 (dense cotangents, joints only) 0.061 / 0.006;  betas x 5 and the identity pose 0.050 / 0.002
  one output a call, atomic route                0.027 / 0.002
  ehm_smpl_backward_rot6d, 9 (V, B)              gpose6d 0.018 (V 1, B 9); V = 2305: 0.001
  bit-equal: the ordered route called twice (every case); gbetas alone and grotmats alone against both (ordered; the workspace all NaN); a handle run at
  B = 65, 1, 33, 9 against a fresh one each; every body beside the one with a NaN in its cotangent, whose grotmats and gbetas are all NaN.
The figures equal the CPU emulation's in size (its largest: 0.075 / 0.008); the bound is a worst case over a few hundred roundings, the measured error
a random walk over them.  A kernel with any of the nine `drop` bugs is 172 to 131 000 times over the bound on its designated case (CPU emulation,
tests/test_smpl_vjp_ref_cpu.py).  Nothing was found: no guard of an output or of the workspace written, no element left unwritten, no NaN out of the
poisoned workspace, no ratio above 1.  87 tests, 6.5 s."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import smpl_ref as R
from tests import smpl_vjp_ref as VR
from tests.test_gpu_smpl_forward import Out, new_model, same_bits
from tests.test_gpu_trunk_autograd import guarded, guards_intact

pytestmark = pytest.mark.gpu

CASES = VR.cases()
ROUTES = ("atomic", "ordered")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _api():
    from egohmr_amd import _lib
    return _lib.api(), _lib


@functools.lru_cache(maxsize=None)
def _model(V, seed, n_extra, weights):
    return new_model(R.cached_asset(V, seed, n_extra, weights), torch.device("cuda:0"))


def _entry(route):
    A, _ = _api()
    return ((A.ehm_smpl_backward_workspace_bytes, A.ehm_smpl_backward) if route == "atomic" else
            (A.ehm_smpl_backward_ordered_workspace_bytes, A.ehm_smpl_backward_ordered))


def backward(model, dev, betas, rotmats, gverts, gjoints, route, want_rot=True, want_betas=True):
    """one call of the route's entry on guarded, sentinel-filled outputs and a guarded workspace of exactly the advertised size, filled with NaN
    -> SimpleNamespace(grotmats, gbetas) of device tensors (None where not asked for)"""
    _, L = _api()
    size_fn, fn = _entry(route)
    B = betas.shape[0]
    t = lambda a: None if a is None else torch.as_tensor(a).to(dev).contiguous()
    nb = C.c_int64()
    size_fn(model.handle(), B, C.byref(nb))
    assert nb.value > 0 and nb.value % 4 == 0
    ws_full, ws = guarded(dev, nb.value // 4)
    assert ws.data_ptr() % 16 == 0
    ws.view(torch.int32).fill_(-1)                                   # 0xFF bytes: every float of the workspace is a NaN
    rot, gb = (Out(dev, B, 24, 3, 3) if want_rot else None), (Out(dev, B, 10) if want_betas else None)
    fn(model.handle(), t(betas), t(rotmats), t(gverts), t(gjoints), gb.t if gb else None, rot.t if rot else None, B, ws, nb.value, L.stream_ptr())
    torch.cuda.synchronize()
    assert guards_intact(ws_full), f"{route}: a guard band of the workspace was written"
    return SimpleNamespace(grotmats=rot.check("grotmats") if rot else None, gbetas=gb.check("gbetas") if gb else None)


def _np(t):
    return None if t is None else t.cpu().numpy()


def report(name, r):
    print(f"{name}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, (name, r)


# ------------------------------------------------------------------------------------------------ 1. both entries against float64
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_backward_against_float64(dev, case):
    asset, x = case.asset(), case.inputs()
    gv, gj = case.cotangents()
    model = _model(case.V, case.asset_seed, case.n_extra, case.weights)
    ref = VR.reference(case.id)
    for route in ROUTES:
        out = backward(model, dev, x.betas, x.rotmats, gv, gj, route)
        bnd = VR.bound(asset, x.betas, x.rotmats, gv, gj, route)
        report(f"{case.id} [{route}]", VR.ratios(_np(out.grotmats), _np(out.gbetas), ref.grotmats, ref.gbetas, bnd))
        if case.cot == "zero_bodies":                   # a +0.0 body and a -0.0 body: nothing but zeros may come out (gjoints is NULL)
            for b in (VR.ZERO_BODY, VR.NEG_ZERO_BODY):
                assert bool((out.grotmats[b] == 0).all()) and bool((out.gbetas[b] == 0).all()), (route, b)
    again = backward(model, dev, x.betas, x.rotmats, gv, gj, "ordered")
    assert same_bits(again.grotmats, out.grotmats) and same_bits(again.gbetas, out.gbetas), "the ordered route gave other bits on a second call"


# ------------------------------------------------------------------------------------------------ 2. one output alone, on the poisoned workspace
ALONE = [c for c in CASES if c.group == "shape" and (c.V, c.B) in ((13, 9), (257, 33), (VR.V_LARGE, 9))]


@pytest.mark.parametrize("case", ALONE, ids=[c.id for c in ALONE])
def test_one_output_alone_gives_the_bits_of_both(dev, case):
    """grotmats = NULL skips the pose-feature launches: gpf in the workspace stays NaN and chain_bwd_rotmat_kernel must not read it"""
    x = case.inputs()
    gv, gj = case.cotangents()
    model = _model(case.V, case.asset_seed, case.n_extra, case.weights)
    both = backward(model, dev, x.betas, x.rotmats, gv, gj, "ordered")
    only_betas = backward(model, dev, x.betas, x.rotmats, gv, gj, "ordered", want_rot=False)
    only_rot = backward(model, dev, x.betas, x.rotmats, gv, gj, "ordered", want_betas=False)
    assert same_bits(only_betas.gbetas, both.gbetas), "gbetas alone"
    assert same_bits(only_rot.grotmats, both.grotmats), "grotmats alone"
    # the atomic route alone: the same launches, so under the same bound
    ref = VR.reference(case.id)
    bnd = VR.bound(case.asset(), x.betas, x.rotmats, gv, gj, "atomic")
    a_b = backward(model, dev, x.betas, x.rotmats, gv, gj, "atomic", want_rot=False)
    a_r = backward(model, dev, x.betas, x.rotmats, gv, gj, "atomic", want_betas=False)
    report(f"{case.id} [atomic, one output a call]", VR.ratios(_np(a_r.grotmats), _np(a_b.gbetas), ref.grotmats, ref.gbetas, bnd))


# ------------------------------------------------------------------------------------------------ 3. handle reuse
def test_handle_reuse_across_batch_sizes(dev):
    asset = R.cached_asset(257, 0, VR.N_EXTRA, "sparse")
    used = new_model(asset, dev)
    for B in (65, 1, 33, 9):
        x = R.inputs("normal", B, 16)
        gv, gj = VR.cotangents("dense", B, 257, VR.N_EXTRA, 16)
        got = backward(used, dev, x.betas, x.rotmats, gv, gj, "ordered")
        fresh = new_model(asset, dev)
        want = backward(fresh, dev, x.betas, x.rotmats, gv, gj, "ordered")
        assert same_bits(got.grotmats, want.grotmats) and same_bits(got.gbetas, want.gbetas), B
        fresh.handle().close()
    used.handle().close()


# ------------------------------------------------------------------------------------------------ 4. non-finite containment
@pytest.mark.parametrize("V,B,body", ((257, 9, 4), (13, 33, 32), (VR.V_LARGE, 9, 8)))     # inside an 8-body group / alone in the last group and tile
def test_one_poisoned_body_stays_alone(dev, V, B, body):
    """input data only: ONE NaN in one body's vertex cotangent (the last vertex, its y component)"""
    model = _model(V, 0, VR.N_EXTRA, "sparse")
    x = R.inputs("normal", B, 17)
    gv, gj = VR.cotangents("dense", B, V, VR.N_EXTRA, 17)
    clean = backward(model, dev, x.betas, x.rotmats, gv, gj, "ordered")
    bad_gv = gv.copy()
    bad_gv[body, V - 1, 1] = np.nan
    bad = backward(model, dev, x.betas, x.rotmats, bad_gv, gj, "ordered")
    others = [b for b in range(B) if b != body]
    if others:
        assert same_bits(bad.grotmats[others], clean.grotmats[others]) and same_bits(bad.gbetas[others], clean.gbetas[others])
    assert bool(torch.isnan(bad.grotmats[body]).all()) and bool(torch.isnan(bad.gbetas[body]).all()), "an output of the poisoned body is not NaN"


# ------------------------------------------------------------------------------------------------ 5. the rot6d entry
@pytest.mark.parametrize("V,B", VR.ROT6D_SHAPES)
def test_backward_rot6d(dev, V, B):
    A, L = _api()
    asset, betas, x, mean, std, gv = VR.rot6d_case(V, B)
    model = _model(V, 0, VR.N_EXTRA, "sparse")
    t = lambda a: torch.as_tensor(a).to(dev).contiguous()
    d_gv = t(gv)
    out = Out(dev, B, 144)
    A.ehm_smpl_backward_rot6d(model.handle(), t(betas), t(x), t(mean), t(std), d_gv, out.t, B, L.stream_ptr())
    torch.cuda.synchronize()
    got = out.check("gpose6d").cpu().numpy()
    assert np.array_equal(d_gv.cpu().numpy().view(np.int32), gv.view(np.int32)), "the caller's cotangent was written (the VJP works on a private copy)"
    ref = VR.backward_rot6d64(asset, betas, x, mean, std, gv)
    report(f"rot6d V = {V}, B = {B}", {"gpose6d": R.ratio(got, ref, VR.bound_rot6d(asset, betas, x, mean, std, gv))})
