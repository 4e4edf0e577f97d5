"""CPU: the float64 references, rounding bounds and wrong variants of tests/eval_ref.py (what tests/test_gpu_eval.py holds the evaluation kernels to),
and the float64 Procrustes solve csrc/procrustes_solve.h through its stand-alone program tools/procrustes_check.cpp.

  * the references reproduce the reference's own goldens (g11, g20, g21);
  * a bound is not too tight: float32 numpy restatements of the three float32 kernels stay inside it on every case the GPU tests use, in two
    summation orders;
  * a bound is not too loose: every deliberately wrong variant misses it by 10 x or more on one of those cases;
  * for every rank-deficient Procrustes case the compared quantity does not depend on how the SVD's null space is completed (and what is NOT
    compared does);
  * the generic cases' singular values are separated, which the float64 bar's conditioning argument needs;
  * procrustes_check, built with AddressSanitizer + UBSan, matches the references on every case.  (The rank-1 cases fail this test with the svd3 that copied V into U
    for rank <= 1 - x_axis_line by 0.125 of the cloud scale, two_point_pred 0.023, one_visible 0.68, and gt_line 0.18 - checked once by building
    the program against that version; docs/EXPERIMENTS.md R29.2.)"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import eval_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = ("sequential", "pairwise")


@pytest.fixture(scope="module")
def cases():
    return R.procrustes_cases()


# ------------------------------------------------------------------------------------------------ goldens
def test_references_reproduce_the_goldens(golden_dir, cases):
    g = np.load(os.path.join(golden_dir, "g11_procrustes.npz"))
    w = R.procrustes(g["pred"][:, None], g["gt"])
    np.testing.assert_allclose(w["mean"][:, 0], g["pa_mpjpe"], rtol=1e-10, atol=1e-12)
    g = np.load(os.path.join(golden_dir, "g20_procrustes_vis.npz"))
    w = R.procrustes_vis(g["pred"][:, None], g["gt"], g["mask"])
    np.testing.assert_allclose(w["per_joint"][:, 0], g["per_joint"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(w["vis_sum"][:, 0], g["vis_sum"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(w["invis_sum"][:, 0], g["invis_sum"], rtol=0, atol=1e-12)
    w = R.procrustes_vis(g["pred45"], g["gt45"], g["mask45"])                   # S = 2 samples share the item's mask
    np.testing.assert_allclose(w["per_joint"], g["per_joint45"], rtol=0, atol=1e-12)
    g = np.load(os.path.join(golden_dir, "g21_procrustes_rank1.npz"))
    assert tuple(g["names"]) == R.G21_CASES
    for name in R.G21_CASES:
        c = cases[name]
        assert np.array_equal(g[f"{name}_pred"], c["pred"]) and np.array_equal(g[f"{name}_gt"], c["gt"]), name      # the recipe's inputs are these cases
        np.testing.assert_allclose(R.determined(c, R.case_want(c)), g[f"{name}_want"], rtol=0, atol=1e-12, err_msg=name)


# ------------------------------------------------------------------------------------------------ bounds: not too tight
def _worst(restate, want, keys):
    return {k: R.ratio(restate[k], want[k], want[k + "_bound"]) for k in keys}


def test_point_error_bound_holds_for_float32_restatements():
    worst = {}
    for name, kw in R.point_cases():
        want = R.point_errors(**kw)
        for order in ORDERS:
            for k, r in _worst(R.point_errors_f32(order=order, **kw), want, ("per_point", "mean", "vis_sum", "invis_sum")).items():
                assert r <= 1.0, (name, order, k, r)
                worst[k] = max(worst.get(k, 0.0), r)
    print("point errors, float32 restatement, worst error / bound:", worst)
    assert worst["per_point"] > 0.05 and worst["mean"] > 0.01          # (the restatement does round: a bound met by 0 would say nothing)


def test_diversity_bound_holds_for_float32_restatements():
    worst = {}
    for name, kw in R.diversity_cases():
        want = R.diversity(**kw)
        for order in ORDERS:
            for k, r in _worst(R.diversity_f32(order=order, **kw), want, ("std", "apd")).items():
                assert r <= 1.0, (name, order, k, r)
                worst[k] = max(worst.get(k, 0.0), r)
    print("diversity, float32 restatement, worst error / bound:", worst)
    assert worst["std"] > 0.01 and worst["apd"] > 0.01


def test_nn_bound_holds_for_float32_restatements():
    worst = 0.0
    for name, kw, planted in R.nn_cases():
        want = R.nn_dist2(**kw)
        for b, q, pos in planted:
            assert want["idx"][b, q] == pos, (name, b, q, pos)
        for order in ORDERS:
            got = R.nn_dist2_f32(order=order, **kw)
            r = R.ratio(got["dist2"], want["dist2"], want["dist2_bound"])
            assert r <= 1.0, (name, order, r)
            worst = max(worst, r)
    print("nn_dist2, float32 restatement, worst error / bound:", worst)
    assert worst > 0.05
    kw = R.nn_lattice_case()
    want, got = R.nn_dist2(**kw), R.nn_dist2_f32(**kw)
    assert np.array_equal(got["dist2"].astype(np.float64), want["dist2"]) and np.array_equal(got["idx"], want["idx"])
    assert (want["idx"][:, 0] == 0).all()                                 # of reference points 0, 2048 and 4099 (equal) the first wins


# ------------------------------------------------------------------------------------------------ bounds: not too loose
def _caught(case_list, ref, wrong, keys):
    """the largest error / bound of the wrong variant over the cases (a variant must be 10 x outside on one of them); a finite figure is preferred to
    the inf of a NaN that met a number (the NaN tails behind P, S = 1)"""
    worst, finite = 0.0, 0.0
    for item in case_list:
        kw = item[1]
        want, bad = ref(**kw), ref(wrong=wrong, **kw)
        r = max(R.ratio(bad[k], want[k], want[k + "_bound"]) for k in keys)
        worst = max(worst, r)
        if np.isfinite(r):
            finite = max(finite, r)
        if finite >= 10.0:
            return finite
    return worst


@pytest.mark.parametrize("wrong", R.POINT_WRONG)
def test_point_error_bound_catches(wrong):
    r = _caught(R.point_cases(), R.point_errors, wrong, ("per_point", "mean", "vis_sum", "invis_sum"))
    print(f"point errors, variant {wrong}: error / bound = {r:.3g}")
    assert r >= 10.0


@pytest.mark.parametrize("wrong", R.DIVERSITY_WRONG)
def test_diversity_bound_catches(wrong):
    r = _caught(R.diversity_cases(), R.diversity, wrong, ("std", "apd"))
    print(f"diversity, variant {wrong}: error / bound = {r:.3g}")
    assert r >= 10.0


def test_diversity_bound_catches_a_one_pass_variance_in_the_camera_frame():
    """sum(a^2) - S mu^2 in float32 cancels metres squared down to millimetres squared: inside the bound on O(1) clouds, far outside it in the
    camera frame - the regime is what makes the std test discriminate."""
    worst = {"unit": 0.0, "camera": 0.0}
    for name, kw in R.diversity_cases():
        if "_S1_" in name or "_none_" in name:
            continue
        want = R.diversity(**kw)
        regime = name.rsplit("_", 1)[1]
        worst[regime] = max(worst[regime], R.ratio(R.diversity_f32(one_pass=True, **kw)["std"], want["std"], want["std_bound"]))
    print("diversity, one-pass variance in float32: std error / bound", worst)
    assert worst["camera"] >= 10.0


def test_nn_bound_catches():
    r = _caught([c for c in R.nn_cases() if c[1]["y"].shape[1] in (2049, 4100)], R.nn_dist2, "skip_last_tile", ("dist2",))
    print(f"nn_dist2, variant skip_last_tile: error / bound = {r:.3g}")
    assert r >= 10.0
    kw = R.nn_lattice_case()                                              # the last minimum: the same distances, another index - the index bar is equality
    want, bad = R.nn_dist2(**kw), R.nn_dist2(wrong="last_min", **kw)
    assert np.array_equal(bad["dist2"], want["dist2"]) and (bad["idx"] != want["idx"]).sum() > 10


def _batch(cases, names, S):
    """B = len(names) items, S samples each: sample 0 is the case's prediction, the others are it moved a little (content differs per row)."""
    g = np.random.Generator(np.random.PCG64(77))
    gt = np.stack([cases[n]["gt"] for n in names])
    pred = np.stack([np.stack([cases[n]["pred"]] + [cases[n]["pred"] + g.normal(scale=0.05, size=cases[n]["pred"].shape).astype(np.float32)
                                                   for _ in range(S - 1)]) for n in names])
    return pred, gt


@pytest.mark.parametrize("wrong", R.PROCRUSTES_WRONG)
def test_procrustes_bar_catches(cases, wrong):
    names = ["generic", "mirrored", "planar_pred", "planar_gt", "similarity_copy"]
    pred, gt = _batch(cases, names, 3)
    want, bad = R.procrustes(pred, gt), R.procrustes(pred, gt, wrong=wrong)
    r = max(R.ratio(bad[k], want[k], R.procrustes_bar(want[k], gt)) for k in ("aligned", "per_joint", "mean"))
    mask = np.stack([cases["three_visible"]["mask"]] * len(names))
    wv, bv = R.procrustes_vis(pred, gt, mask), R.procrustes_vis(pred, gt, mask, wrong=wrong)
    rv = max(R.ratio(bv[k], wv[k], R.procrustes_bar(wv[k], gt)) for k in ("per_joint", "mean", "vis_sum"))
    print(f"procrustes, variant {wrong}: error / bar = {r:.3g} (plain), {rv:.3g} (visible-joint)")
    assert r >= 10.0 and rv >= 10.0


# ------------------------------------------------------------------------------------------------ rank-deficient cases
def test_rank_deficient_cases_compare_determined_quantities_only(cases):
    """Re-completing the null space of numpy's U and V by random orthogonal matrices leaves the compared quantity unchanged to 1e-12, and moves the
    quantities that are NOT compared: the invisible joints' errors with one visible joint, the aligned cloud for a collinear ground truth."""
    undetermined = {"one_visible": lambda c, o: o["per_joint"][0, 0][~c["mask"]], "gt_line": lambda c, o: o["aligned"][0, 0]}
    moved = {k: 0.0 for k in undetermined}
    for name, c in cases.items():
        if c["kind"] != "rank":
            continue
        base = R.case_want(c)
        for seed in range(8):
            again = R.case_want(c, recomplete=np.random.default_rng(seed))
            a, b = R.determined(c, base), R.determined(c, again)
            if c["compare"] == "nan":
                assert np.isnan(a).all() and np.isnan(b).all(), name
                continue
            np.testing.assert_allclose(b, a, rtol=0, atol=1e-12, err_msg=f"{name} seed {seed}")
            if name in undetermined:
                moved[name] = max(moved[name], float(np.abs(undetermined[name](c, again) - undetermined[name](c, base)).max()))
    print("moved by the re-completion (not compared):", moved)
    assert all(v > 1e-3 for v in moved.values()), moved
    one = cases["one_visible"]
    assert float(R.determined(one, R.case_want(one)).max()) < 1e-12           # a similarity aligns a single visible joint exactly


def test_generic_cases_are_well_conditioned(cases):
    for name, c in cases.items():
        if c["kind"] == "generic":
            g1, g2 = R.singular_gaps(c["pred"], c["gt"], c["mask"])
            assert g1 > 1e-3 and g2 > 1e-3, (name, g1, g2)


# ------------------------------------------------------------------------------------------------ the solve itself, on the host
def _out_of_aligned(c, aligned):
    e = np.sqrt(((aligned - c["gt"].astype(np.float64)) ** 2).sum(-1))
    m = np.ones(len(e), bool) if c["mask"] is None else c["mask"]
    return {"aligned": aligned[None, None], "per_joint": e[None, None], "vis_sum": np.array([[(e * m).sum()]])}


def test_sanitized_solve_matches_the_references(cases, golden_dir, tmp_path):
    """tools/procrustes_check.cpp under AddressSanitizer + UBSan (a plain host binary, nothing loaded into Python): csrc/procrustes_solve.h on every
    Procrustes case, J = 3 and J = 100 clouds and the g21 fixture, against the float64 references; bar 1e-12 x the cloud scale (float64 solve,
    gaps above 1e-3 or a determined quantity)."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tools/procrustes_check.cpp"
    exe = tmp_path / "procrustes_check"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(REPO, "egohmr_amd", "csrc"), os.path.join(REPO, "tools", "procrustes_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    names = list(cases)
    todo = [cases[n] for n in names]
    for J in (3, 100):
        extra = R.procrustes_cases(J=J, seed=100 + J)
        for n in ("generic", "mirrored", "x_axis_line", "one_visible", "gt_one_point"):
            names.append(f"{n}_J{J}")
            todo.append(extra[n])
    R.write_check_cases(str(tmp_path / "cases.txt"), todo)
    run = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr)
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    worst = {}
    for name, c, aligned in zip(names, todo, R.read_check_output(run.stdout, todo)):
        got, want = R.determined(c, _out_of_aligned(c, aligned)), R.determined(c, R.case_want(c))
        if c.get("compare") == "nan":
            assert np.isnan(aligned).all(), name
            continue
        scale = float(np.abs(c["gt"]).max())
        assert np.isfinite(aligned).all(), name
        worst[name] = float(np.abs(got - want).max()) / scale
        assert worst[name] <= 1e-12, (name, worst[name])
    print("procrustes_check against float64 numpy, |diff| / cloud scale:", {k: f"{v:.1e}" for k, v in worst.items()})
    g = np.load(os.path.join(golden_dir, "g21_procrustes_rank1.npz"))
    for name in R.G21_CASES:                                               # the reference's own numbers
        i = names.index(name)
        got = R.determined(todo[i], _out_of_aligned(todo[i], R.read_check_output(run.stdout, todo)[i]))
        np.testing.assert_allclose(got, g[f"{name}_want"], rtol=0, atol=1e-12, err_msg=name)
