"""No GPU: conditions on tests/smpl_vjp_ref.py alone, and the evidence that its bound tells a subtly broken SMPL VJP from the faithful one.

For every case of smpl_vjp_ref.cases() (the list tests/test_gpu_smpl_vjp.py runs on the device): the staged float64 restatement equals float64 autograd
through oracle.smpl.SMPLOracle to rounding, and the numpy float32 emulation of the device's order of operations stays under the bound on both gA routes
(the largest error / bound is printed).  Every `drop` variant of the emulation - a plausible kernel bug each - is over the bound on its designated case,
on both routes; by how much is printed.  The rot6d restatement equals autograd through Gram-Schmidt as well."""
import numpy as np
import pytest

from tests import smpl_ref as R
from tests import smpl_vjp_ref as VR

CASES = VR.cases()
# float64 against float64: both sum the same terms in another order - a few hundred float64 roundings (2^-53 each) of sums whose majorant is M
F64_SLACK = 2.0 ** -40


def _scale(x):
    return max(float(np.abs(x).max()), 1e-300)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_restatement_equals_autograd_and_the_emulation_stays_under_the_bound(case):
    asset, x = case.asset(), case.inputs()
    gv, gj = case.cotangents()
    ref = VR.reference(case.id)
    ar, ab = VR.autograd64(asset, x.betas, x.rotmats, gv, gj)
    worst = {}
    for route in ("atomic", "ordered"):
        bnd = VR.bound(asset, x.betas, x.rotmats, gv, gj, route)
        if route == "atomic":                # restatement = autograd, against the majorant (an element whose majorant is zero is an exact zero in both)
            d_rot, d_b = np.abs(ar - ref.grotmats), np.abs(ab - ref.gbetas)
            assert (d_rot <= F64_SLACK * bnd.M_grotmats).all() and (d_b <= F64_SLACK * bnd.M_gbetas).all(), (d_rot.max(), d_b.max())
            print(f"{case.id}: |restatement - autograd| <= {d_rot.max():.2e} (grotmats, scale {_scale(ar):.2e}), {d_b.max():.2e} (gbetas, scale {_scale(ab):.2e})")
        grot, gb = VR.emulate(asset, x.betas, x.rotmats, gv, gj, route)
        worst[route] = VR.ratios(grot, gb, ref.grotmats, ref.gbetas, bnd)
    print(f"{case.id}: emulation / bound " + "; ".join(f"{rt}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) for rt, r in worst.items()))
    assert max(max(r.values()) for r in worst.values()) <= 1.0, worst


@pytest.mark.parametrize("drop,V,B,cot", VR.DESIGNATED, ids=[d[0] for d in VR.DESIGNATED])
def test_a_broken_kernel_misses_the_bound(drop, V, B, cot):
    case = next(c for c in CASES if (c.V, c.B, c.cot) == (V, B, cot) and c.weights == "sparse" and c.n_extra == VR.N_EXTRA and c.family == "normal")
    asset, x = case.asset(), case.inputs()
    gv, gj = case.cotangents()
    ref = VR.reference(case.id)
    for route in ("atomic", "ordered"):
        bnd = VR.bound(asset, x.betas, x.rotmats, gv, gj, route)
        ok = VR.ratios(*VR.emulate(asset, x.betas, x.rotmats, gv, gj, route), ref.grotmats, ref.gbetas, bnd)
        bad = VR.ratios(*VR.emulate(asset, x.betas, x.rotmats, gv, gj, route, drop=drop), ref.grotmats, ref.gbetas, bnd)
        print(f"{drop} on {case.id} [{route}]: faithful " + ", ".join(f"{k} {v:.3f}" for k, v in ok.items()) + "; broken " +
              ", ".join(f"{k} {v:.3g}" for k, v in bad.items()))
        assert max(ok.values()) <= 1.0 and max(bad.values()) > 1.0, (drop, route, ok, bad)


def test_the_designated_cases_reach_what_their_variant_breaks():
    for drop, V, B, cot in VR.DESIGNATED:
        G, Gfull, chunks = VR.pf_groups(V)
        if drop == "pf_tail":
            assert G > Gfull
        if drop == "tiles8":
            assert V > 8 * VR.VT
        if drop == "last8":
            assert B % VR.BG
        if drop == "last32":
            assert B % VR.PF_TILE
        if drop == "extra_once":
            ids = R.cached_asset(V, 0, VR.N_EXTRA, "sparse")["extra_joints_idxs"].tolist()
            assert len(set(ids)) < len(ids) and (V - 1) in ids


def test_the_shapes_reach_every_path():
    """the claims of the GPU test's shape table"""
    rem = {V: (3 * V) % 8 for V in VR.V_SMALL}
    assert [rem[V] for V in (1, 3, 4, 7, 8, 13)] == [3, 1, 4, 5, 0, 7]
    empty = lambda V: sum(g0 == g1 for g0, g1 in VR.pf_groups(V)[2])
    assert all(empty(V) > 0 for V in VR.V_SMALL if V < 86) and empty(86) == 0 and VR.pf_groups(86)[0] == 33
    assert all(sum(g1 - g0 for g0, g1 in VR.pf_groups(V)[2]) == VR.pf_groups(V)[0] for V in VR.V_SMALL + (VR.V_LARGE,))       # the chunks tile K
    assert -(-VR.V_LARGE // VR.VT) == 10
    k = VR.counts(R.cached_asset(VR.V_LARGE, 0, VR.N_EXTRA, "sparse"), "atomic")
    print(f"V = {VR.V_LARGE}: k_gA {k.gA} (atomic), {VR.counts(R.cached_asset(VR.V_LARGE, 0, VR.N_EXTRA, 'sparse'), 'ordered').gA} (ordered), k_pf {k.pf}, k_sb {k.sb}")


@pytest.mark.parametrize("V,B", ((1, 1), (257, 9)))
def test_rot6d_restatement_equals_autograd(V, B):
    asset, betas, x, mean, std, gv = VR.rot6d_case(V, B)
    got = VR.backward_rot6d64(asset, betas, x, mean, std, gv)
    want = VR.autograd_rot6d64(asset, betas, x, mean, std, gv)
    bnd = VR.bound_rot6d(asset, betas, x, mean, std, gv)
    d = np.abs(got - want)
    print(f"rot6d V = {V}, B = {B}: |restatement - autograd| <= {d.max():.2e} (scale {_scale(want):.2e}); smallest bound / scale {bnd.min() / _scale(want):.2e}")
    assert (d <= 2.0 ** -16 * bnd).all()                # float64 rounding against a float32 bound: 2^-29 u apart, 2^-16 of the bound is generous
    assert np.isfinite(bnd).all() and (bnd > 0).all()
