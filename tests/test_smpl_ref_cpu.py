"""No GPU: the bound of tests/smpl_ref.py holds the faithful order of operations and tells a broken hi / lo split from it.

For every case of smpl_ref.cases() (the list tests/test_gpu_smpl_forward.py runs on the device) the numpy float32 / float16 emulation of the path the
case takes stays under `bound` / `bound_valu`; in every case tagged `blend` each broken variant of the split-f16 blend (the coefficients' lo halves
zeroed, the basis's lo halves zeroed, both cross products left out) exceeds `bound` on some vertex at least 4 times over.  Every figure is printed.
Beside that: the float64 reference agrees with the float32 oracle, make_asset keeps its promises, every input family is well conditioned as a 6-D
rotation, and round_once is a single rounding."""
import numpy as np
import pytest
import torch

from oracle.smpl import SMPLOracle
from tests import smpl_ref as R

CASES = R.cases()
DROPS = ("a_lo", "b_lo", "cross")
MUTANT_FACTOR = 4.0                     # a condition on the choice of inputs (the issue's figure), not a measurement


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_faithful_emulation_stays_under_the_bound(case):
    asset, x = case.asset(), case.inputs()
    path = R.path_of(asset, case.B)
    bnd = (R.bound if path == "mfma" else R.bound_valu)(asset, x.betas, x.rotmats)
    r = R.ratios(R.emulate(asset, x.betas, x.rotmats, path), bnd)
    print(f"{case.id} [{path}]: emulation / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) < 1.0, r


@pytest.mark.parametrize("case", [c for c in CASES if c.blend], ids=[c.id for c in CASES if c.blend])
def test_a_broken_split_misses_the_bound(case):
    asset, x = case.asset(), case.inputs()
    assert R.path_of(asset, case.B) == "mfma"
    bnd = R.bound(asset, x.betas, x.rotmats)
    ok = R.ratios(R.emulate(asset, x.betas, x.rotmats, "mfma"), bnd)["vertices"]
    got = {d: R.ratios(R.emulate(asset, x.betas, x.rotmats, "mfma", drop=d), bnd)["vertices"] for d in DROPS}
    print(f"{case.id}: vertices / bound: faithful {ok:.3f}, " + ", ".join(f"without {d} {v:.1f}" for d, v in got.items()))
    assert ok < 1.0
    for d, v in got.items():
        assert v >= MUTANT_FACTOR, (d, v)


def test_the_matrix_core_emulation_of_a_valu_case_is_under_its_bound_too():
    """the two bounds are two models: each path under its own at one shape both kernels can run (B = 33 through skin_kernel is what a dense asset does)"""
    asset, x = R.cached_asset(129, 0, R.N_EXTRA, "sparse"), R.inputs("normal", 33, 5)
    for path, bound in (("mfma", R.bound), ("valu", R.bound_valu)):
        r = R.ratios(R.emulate(asset, x.betas, x.rotmats, path), bound(asset, x.betas, x.rotmats))
        print(f"{path}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
        assert max(r.values()) < 1.0, (path, r)


def test_float64_reference_agrees_with_the_float32_oracle():
    asset, x = R.cached_asset(257, 0, R.N_EXTRA, "sparse"), R.inputs("normal", 5, 4)
    ref = R.forward64(asset, x.betas, x.rotmats)
    rot = torch.from_numpy(x.rotmats)
    o32 = SMPLOracle(asset)(torch.from_numpy(x.betas), rot[:, 1:], rot[:, :1])
    for name in ("vertices", "joints", "A"):
        d = float((getattr(o32, name).double() - getattr(ref, name)).abs().max())
        print(f"{name}: max|float32 oracle - float64| = {d:.3e}")
        assert d < 5e-6, (name, d)             # (the documented cross-check of the two references, tests/test_gpu_parity.py's atol)
    assert ref.joints.shape == (5, 24 + R.N_EXTRA, 3) and ref.vertices.dtype == torch.float64


@pytest.mark.parametrize("V", R.V_MATRIX + (8,))
@pytest.mark.parametrize("weights", ("sparse", "dense"))
def test_make_asset_keeps_its_promises(V, weights):
    a = R.make_asset(V, 0, R.N_EXTRA, weights)
    b = R.make_asset(V, 0, R.N_EXTRA, weights)
    for k, v in a.items():
        assert np.array_equal(v, b[k]), k                                          # deterministic
        assert v.dtype == (np.int64 if k in ("parents", "faces", "extra_joints_idxs") else np.float32), k
    assert a["v_template"].shape == (V, 3) and a["shapedirs"].shape == (V, 3, 10) and a["posedirs"].shape == (207, V * 3)
    Jr, W, ex = a["J_regressor"], a["lbs_weights"], a["extra_joints_idxs"]
    assert Jr.shape == (24, V) and (Jr >= 0).all() and np.allclose(Jr.sum(1), 1.0, atol=1e-6)      # convex rows
    assert W.shape == (V, 24) and (W >= 0).all() and np.allclose(W.sum(1), 1.0, atol=1e-6)
    assert len(ex) == R.N_EXTRA and ex.min() >= 0 and ex.max() < V and (V - 1) in ex and len(set(ex.tolist())) < len(ex)   # V - 1 is there, ids repeat
    assert list(a["parents"]) == R.PARENTS
    nnz = (W != 0).sum(1)
    assert nnz[0] == 1 and W[0, 23] == 1.0                                         # a row whose only weight is on joint 23
    if V >= 8:
        assert {1, 2, 3, 4} <= set(nnz.tolist())
        assert W[1, 0] > 0 and W[1, 23] > 0 and nnz[1] == 2 and nnz[2] == 1 and W[2, 0] == 1.0 and nnz[3] == 3 and W[3, 0] > 0
        assert (nnz.max() == 6) == (weights == "dense")
        slots = R.sparse_slots(W)
        assert (slots is None) == (weights == "dense")
        if slots is not None:                                                      # joint 0 live in slot 0 AND as the padding of the same row
            idx, val = slots
            assert idx[0, 1] == 0 and val[0, 1] > 0 and idx[1, 1] == 23 and (idx[2:, 1] == 0).all() and (val[2:, 1] == 0).all()
    assert len(R.make_asset(V, 0, 0, weights)["extra_joints_idxs"]) == 0


@pytest.mark.parametrize("family", R.FAMILIES)
def test_input_families_are_well_conditioned_rotations(family):
    for B in sorted({c.B for c in CASES}):
        x = R.inputs(family, B, 1)
        cond = float(R.conditioning(x.x6).max())
        assert cond <= 4.0, (family, B, cond)
        Rm = x.rotmats.astype(np.float64)
        assert np.abs(Rm @ Rm.transpose(0, 1, 3, 2) - np.eye(3)).max() < 1e-6
    print(f"{family}: conditioning <= {cond:.3f}")
    assert x.betas.dtype == np.float32 and x.rotmats.dtype == np.float32


@pytest.mark.parametrize("B", (7, 33))
def test_rot6d_inputs_are_well_conditioned_and_non_trivial(B):
    x, mean, std = R.rot6d_inputs(B, 0)
    r = R.rot6d64(x, mean, std)
    print(f"B = {B}: conditioning <= {r.cond.max():.3f}, largest R bound {r.E_R.max():.3e}")
    assert r.cond.max() <= 4.0
    assert np.abs(mean).min() > 0 and std.min() >= 0.05 and np.unique(std).size == 144 and np.unique(mean).size == 144
    assert np.abs(r.R @ r.R.transpose(0, 1, 3, 2) - np.eye(3)).max() < 1e-12
    assert r.E_R.max() < 64 * R.U                    # conditioning 4 keeps the bound at a few ulps


def test_round_once_is_one_rounding():
    """x * std + mean in exact rational arithmetic, rounded once, on random values and on constructed float32 ties"""
    from fractions import Fraction
    g = np.random.default_rng(0)
    x = g.normal(size=400).astype(np.float32)
    std = (0.1 + g.random(400)).astype(np.float32)
    mean = g.normal(size=400).astype(np.float32)
    x[:4] = np.float32(2.0 ** -12)
    std[:4] = np.float32(2.0 ** -12 + 2.0 ** -35)                 # product 2^-24 + 2^-47: just past half an ulp of 1
    mean[:4] = np.float32([1.0, -1.0, 1.0 + 2.0 ** -23, 2.0])
    x[4:8] = np.float32(1.0 + 2.0 ** -23)                         # product 1 + 2^-22 + 2^-46 under a large mean: the float64 sum itself is rounded
    std[4:8] = np.float32(1.0 + 2.0 ** -23)
    mean[4:8] = np.float32([2.0 ** 8, -2.0 ** 9, 2.0 ** 20, 3.0 * 2.0 ** 30])
    got = R.round_once(x, std, mean)

    def exact_round(v):
        lo = np.float32(float(v))                                 # float(Fraction) is correctly rounded to float64; narrow, then fix up exactly
        cands = sorted({lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))}, key=float)
        best = min(cands, key=lambda c: (abs(Fraction(float(c)) - v), int(np.float32(c).view(np.int32)) & 1))
        return np.float32(best)
    for i in range(400):
        v = Fraction(float(x[i])) * Fraction(float(std[i])) + Fraction(float(mean[i]))
        assert got[i] == exact_round(v), (i, got[i], float(v))
    assert got[0] == np.float32(1.0 + 2.0 ** -23)
