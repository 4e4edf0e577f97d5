"""GPU: the evaluation kernels (csrc/eval.hip point_errors / procrustes / procrustes_vis / diversity, csrc/metrics.hip nn_dist2) against the float64
references of tests/eval_ref.py, at the thread-count and tile edges, with several samples per ground truth, unequal strides, both coordinate regimes
(O(1), and the camera frame: millimetres on top of metres) and the rank-deficient branches of the 3 x 3 solve.

Bars: the float32 kernels get the rounding bound eval_ref derives per output from the float64 intermediates of the case; the two float64 Procrustes
kernels get 2^-22 max(|want|, cloud scale) (eval_ref.procrustes_bar); NaN must meet NaN; indices and guard bytes are exact.  Every test prints its
worst error / bound; docs/EXPERIMENTS.md records the measured ones."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import eval_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.astype(np.uint8) if a.dtype == bool else a).to(dev)


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _guarded(n, dev, guard=64):
    """(float32 view of n elements, the whole byte buffer) with `guard` floats of 0xA5 bytes on either side"""
    buf = torch.full(((n + 2 * guard) * 4,), 0xA5, dtype=torch.uint8, device=dev)
    return buf.view(torch.float32)[guard:guard + n], buf, guard * 4


def _guards_intact(buf, gbytes):
    return bool((buf[:gbytes] == 0xA5).all()) and bool((buf[-gbytes:] == 0xA5).all())


# ------------------------------------------------------------------------------------------------ point errors
def _point_errors_abi(dev, kw, per_point=True, sums=True, outs=None):
    """ehm_eval_point_errors through its descriptor (egohmr_amd.metrics.point_errors always asks for the sums)"""
    from egohmr_amd import _lib
    pred, gt, P = _t(kw["pred"], dev), _t(kw["gt"], dev), kw["P"]
    B, S = pred.shape[:2]
    o = outs or {}
    mean = o.get("mean", torch.empty(B, S, device=dev))
    pp = o.get("per_point", torch.empty(B, S, P, device=dev)) if per_point else None
    vis, inv = (torch.empty(B, S, device=dev), torch.empty(B, S, device=dev)) if sums else (None, None)
    po, go, m = _t(kw.get("pred_origin"), dev), _t(kw.get("gt_origin"), dev), _t(kw.get("mask"), dev)
    d = _lib.EvalPointsDesc(_lib.ptr(pred), _lib.ptr(gt), _lib.ptr(po), _lib.ptr(go), _lib.ptr(m), _lib.ptr(pp), _lib.ptr(mean), _lib.ptr(vis), _lib.ptr(inv),
                            B, S, P, pred.shape[2], gt.shape[1], int(kw.get("origin_point", -1)))
    with _lib.on_device(dev):
        _lib.api().ehm_eval_point_errors(C.byref(d), _lib.stream_ptr())
    torch.cuda.synchronize()
    return {"per_point": pp, "mean": mean, "vis_sum": vis, "invis_sum": inv}


@pytest.mark.parametrize("regime", R.REGIMES)
def test_point_errors_match_float64_within_the_rounding_bound(dev, regime):
    worst = {}
    for name, kw in R.point_cases():
        if not name.endswith(regime):
            continue
        want = R.point_errors(**kw)
        got = _point_errors_abi(dev, kw)
        for k in ("per_point", "mean", "vis_sum", "invis_sum"):
            r = R.ratio(_np(got[k]), want[k], want[k + "_bound"])
            worst[k] = max(worst.get(k, 0.0), r)
            assert r <= 1.0, (name, k, r)
        lean = _point_errors_abi(dev, kw, per_point=False, sums=False)          # per_point, vis_sum, invis_sum NULL: the same mean, nothing else written
        assert torch.equal(lean["mean"], got["mean"]), name
    print(f"point_errors_kernel, {regime}: worst error / bound {({k: round(v, 3) for k, v in worst.items()})}")


def test_point_errors_wrapper_and_metrics_agree_with_the_descriptor_call(dev):
    from egohmr_amd import metrics as M
    name, kw = [c for c in R.point_cases() if c[0].startswith("P24_B2S33_pp45gp30_o0") and c[0].endswith("camera")][0]
    got = _point_errors_abi(dev, kw)
    r = M.point_errors(_t(kw["pred"], dev), _t(kw["gt"], dev), points=24, origin_point=0, mask=torch.from_numpy(kw["mask"]).to(dev), per_point=True)
    for k in ("per_point", "mean", "vis_sum", "invis_sum"):
        assert torch.equal(r[k], got[k]), k
    want = R.point_errors(**kw)
    mp = M.mpjpe(_t(kw["pred"], dev), _t(kw["gt"], dev)[:, None])            # 45 / 30 joints handed over, 24 count, the pelvis is joint 0
    assert R.ratio(_np(mp), want["mean"], want["mean_bound"]) <= 1.0


def test_point_errors_write_inside_their_buffers_and_refuse_bad_arguments(dev):
    from egohmr_amd import _lib
    name, kw = [c for c in R.point_cases() if c[0].startswith("P257_B3S4") and "both" in c[0] and c[0].endswith("unit")][0]
    B, S, P = 3, 4, 257
    pp, pp_buf, gb = _guarded(B * S * P, dev)
    mean, mean_buf, _ = _guarded(B * S, dev)
    got = _point_errors_abi(dev, kw, outs={"per_point": pp.view(B, S, P), "mean": mean.view(B, S)})
    assert _guards_intact(pp_buf, gb) and _guards_intact(mean_buf, gb)
    want = R.point_errors(**kw)
    assert R.ratio(_np(got["per_point"]), want["per_point"], want["per_point_bound"]) <= 1.0
    assert R.ratio(_np(got["mean"]), want["mean"], want["mean_bound"]) <= 1.0
    plain = {k: kw[k] for k in ("pred", "gt", "P")}
    for bad in (dict(plain, origin_point=P),                                          # origin_point >= P
                dict(plain, origin_point=0, pred_origin=kw["pred_origin"]),          # an origin index together with a pointer
                dict(plain, origin_point=0, gt_origin=kw["gt_origin"]),
                dict(plain, P=P + 1)):                                                # P > pred_points
        with pytest.raises(_lib.EgoHMRHipError):
            _point_errors_abi(dev, bad)


# ------------------------------------------------------------------------------------------------ Procrustes
def _near(g, gt, S):
    """S predictions per ground truth [B,J,3]: a similarity of it plus noise, different per row"""
    B, J = gt.shape[:2]
    pred = np.empty((B, S, J, 3), np.float32)
    for b in range(B):
        for s in range(S):
            pred[b, s] = 1.1 * gt[b] @ R._rot(g).T + g.normal(scale=0.04, size=(J, 3)) + g.normal(size=3)
    return pred


def _procrustes_abi(dev, pred, gt, mask=None, align=False, want=("aligned", "per_joint", "mean", "vis_sum", "invis_sum")):
    from egohmr_amd import _lib
    B, S, J = pred.shape[:3]
    shapes = {"aligned": (B, S, J, 3), "per_joint": (B, S, J), "mean": (B, S), "vis_sum": (B, S), "invis_sum": (B, S)}
    o = {k: (torch.full(shapes[k], 7.0, device=dev) if k in want else None) for k in shapes}
    fn = _lib.api().ehm_eval_procrustes_vis if align else _lib.api().ehm_eval_procrustes
    with _lib.on_device(dev):
        fn(_t(pred, dev), _t(gt, dev), _t(mask, dev), o["aligned"], o["per_joint"], o["mean"], o["vis_sum"], o["invis_sum"], B, S, J, _lib.stream_ptr())
    torch.cuda.synchronize()
    return o


def _procrustes_ratio(got, want, gt, keys):
    return {k: R.ratio(_np(got[k]), want[k], R.procrustes_bar(want[k], gt)) for k in keys}


ALL5 = ("aligned", "per_joint", "mean", "vis_sum", "invis_sum")


@pytest.mark.parametrize("B,S,J", [(1, 1, 24), (63, 1, 24), (64, 1, 24), (13, 5, 24), (26, 5, 24), (13, 5, 3), (13, 5, 4), (13, 5, 32), (13, 5, 45), (13, 5, 100)],
                         ids=lambda v: str(v))
def test_procrustes_thread_edges_and_joint_counts(dev, B, S, J):
    """n = B S of 1, 63, 64, 65, 130 (one thread per pair, 64 per block) with one ground truth per S samples, and J from 3 to 100 (no J <= 32 limit)."""
    g = np.random.Generator(np.random.PCG64(900 + 7 * B + S + 1000 * J))
    gt = g.normal(scale=0.3, size=(B, J, 3)).astype(np.float32)
    pred = _near(g, gt, S)
    mask = g.random((B, J)) < 0.5
    worst = {}
    for m in (mask, None):
        want = R.procrustes(pred, gt, mask=m)
        got = _procrustes_abi(dev, pred, gt, mask=m)
        for k, r in _procrustes_ratio(got, want, gt, ALL5).items():
            worst[k] = max(worst.get(k, 0.0), r)
    assert float(got["invis_sum"].abs().max()) == 0.0                            # (the last call) no mask: everything is visible
    print(f"procrustes_kernel B={B} S={S} J={J}: worst error / bar {({k: round(v, 4) for k, v in worst.items()})}")
    assert max(worst.values()) <= 1.0, worst


def test_procrustes_wrappers_take_45_joints(dev):
    from egohmr_amd import metrics as M
    g = np.random.Generator(np.random.PCG64(45))
    gt = g.normal(scale=0.3, size=(7, 45, 3)).astype(np.float32)
    pred = _near(g, gt, 1)
    want = R.procrustes(pred, gt)
    pa = M.pa_mpjpe(_t(pred[:, 0], dev), _t(gt, dev))
    al = M.similarity_align(_t(pred[:, 0], dev), _t(gt, dev))
    r = (R.ratio(_np(pa), want["mean"][:, 0], R.procrustes_bar(want["mean"][:, 0], gt)),
         R.ratio(_np(al), want["aligned"][:, 0], R.procrustes_bar(want["aligned"][:, 0], gt)))
    print(f"pa_mpjpe / similarity_align on 45 joints: error / bar {r}")
    assert max(r) <= 1.0


def test_procrustes_named_cases_compare_what_the_data_determine(dev, golden_dir):
    """Mirrored, planar and similarity-copy clouds, and the rank-deficient ones: a collinear prediction, a prediction of two points, a ground truth of
    one point (aligned = mu2), a collinear ground truth (only sum e^2 is determined) - each inside a batch of ordinary items; the reference's own
    numbers for the g21 cases."""
    cases = R.procrustes_cases()
    names = [n for n, c in cases.items() if c["mask"] is None and c.get("compare") != "nan"]
    order = ["generic"] + [n for n in names if n != "generic"] + ["generic"]
    pred = np.stack([cases[n]["pred"] for n in order])[:, None]
    gt = np.stack([cases[n]["gt"] for n in order])
    got = _procrustes_abi(dev, pred, gt)
    g21 = np.load(os.path.join(golden_dir, "g21_procrustes_rank1.npz"))
    worst = {}
    for i, n in enumerate(order):
        c = cases[n]
        out = {k: _np(got[k][i:i + 1]) for k in ALL5}
        assert np.isfinite(out["aligned"]).all() and np.isfinite(out["per_joint"]).all(), n
        have, want = R.determined(c, out), R.determined(c, R.case_want(c))
        scale = float(np.abs(c["gt"]).max()) ** (2 if c.get("compare") == "sum_e2" else 1)
        worst[n] = float((np.abs(have - want) / (2.0 ** -22 * np.maximum(np.abs(want), scale))).max())
        if n in R.G21_CASES:
            w21 = g21[f"{n}_want"]
            worst[n + "/g21"] = float((np.abs(have - w21) / (2.0 ** -22 * np.maximum(np.abs(w21), scale))).max())
    print(f"procrustes_kernel named cases: error / bar {({k: round(v, 4) for k, v in worst.items()})}")
    assert max(worst.values()) <= 1.0, worst
    sim = order.index("similarity_copy")
    assert float(got["mean"][sim]) <= 2.0 ** -22 * float(np.abs(gt[sim]).max())       # a similarity copy of the truth: error 0


def test_procrustes_one_point_prediction_is_nan_for_that_sample_only(dev):
    cases = R.procrustes_cases()
    g = np.random.Generator(np.random.PCG64(46))
    gt = np.stack([cases["generic"]["gt"], g.normal(scale=0.3, size=(24, 3)).astype(np.float32)])
    pred = _near(g, gt, 3)
    pred[0, 1] = cases["pred_one_point"]["pred"]
    mask = g.random((2, 24)) < 0.5
    got = _procrustes_abi(dev, pred, gt, mask=mask)
    want = R.procrustes(pred, gt, mask=mask)
    assert all(bool(torch.isnan(got[k][0, 1]).all()) for k in ALL5)
    r = _procrustes_ratio(got, want, gt, ALL5)                                        # (NaN must meet NaN, everything else its bar)
    print(f"procrustes_kernel with one NaN sample: error / bar {r}")
    assert max(r.values()) <= 1.0, r


def test_procrustes_each_output_alone_and_none_refused(dev):
    from egohmr_amd import _lib
    g = np.random.Generator(np.random.PCG64(47))
    gt = g.normal(scale=0.3, size=(5, 24, 3)).astype(np.float32)
    pred = _near(g, gt, 3)
    mask = g.random((5, 24)) < 0.5
    for align in (False, True):
        full = _procrustes_abi(dev, pred, gt, mask=mask, align=align)
        for k in ("aligned", "per_joint", "mean"):
            one = _procrustes_abi(dev, pred, gt, mask=mask, align=align, want=(k,))
            assert torch.equal(one[k], full[k]), (align, k)
        with pytest.raises(_lib.EgoHMRHipError):
            _procrustes_abi(dev, pred, gt, mask=mask, align=align, want=("vis_sum", "invis_sum"))
    with pytest.raises(_lib.EgoHMRHipError):
        _procrustes_abi(dev, pred[:, :, :2], gt[:, :2])                                # J = 2: refused by the plain entry


# ------------------------------------------------------------------------------------------------ masked Procrustes
def _vis_batch(g, B, S, J, counts):
    """items whose number of visible joints cycles through `counts` (None: a random mask, 'all': every joint), S samples sharing the item's mask"""
    gt = g.normal(scale=0.3, size=(B, J, 3)).astype(np.float32)
    pred = _near(g, gt, S)
    mask = np.zeros((B, J), bool)
    nvis = []
    for b in range(B):
        c = counts[b % len(counts)]
        if c is None:
            mask[b] = g.random(J) < 0.6
            mask[b, :min(J, 4)] = True
        elif c == "all":
            mask[b] = True
        else:
            mask[b, g.choice(J, c, replace=False)] = True
        nvis.append(int(mask[b].sum()))
    return pred, gt, mask, np.array(nvis)


@pytest.mark.parametrize("B,S,J", [(9, 3, 2), (9, 3, 24), (9, 3, 45), (9, 3, 100), (65, 1, 24), (22, 3, 24)], ids=lambda v: str(v))
def test_procrustes_vis_visible_counts(dev, B, S, J):
    """0, 1, 2, 3 and all visible joints next to ordinary items.  No visible joint: NaN everywhere, both sums included.  One visible joint: that joint is
    aligned exactly; its error and vis_sum are compared, the invisible joints' errors turn with a rotation the data leave free and must only be
    finite.  Two or more: everything."""
    g = np.random.Generator(np.random.PCG64(1200 + B + 10 * J))
    counts = [None, 0, 1, 2, "all", None] if J == 2 else [None, 0, 1, 2, 3, "all", None, 1, None]
    pred, gt, mask, nvis = _vis_batch(g, B, S, J, counts)
    want = R.procrustes_vis(pred, gt, mask)
    got = _procrustes_abi(dev, pred, gt, mask=mask, align=True)
    worst = {}
    for b in range(B):
        out = {k: _np(got[k][b]) for k in ALL5}
        if nvis[b] == 0:
            assert all(np.isnan(out[k]).all() for k in ALL5), b
            assert np.isnan(want["per_joint"][b]).all()
            continue
        assert all(np.isfinite(out[k]).all() for k in ALL5), (b, nvis[b])
        scale = float(np.abs(gt[b]).max())
        keys = ("per_joint", "mean", "vis_sum", "invis_sum")
        if nvis[b] == 1 and J > 1:
            out = {"per_joint": out["per_joint"][:, mask[b]], "vis_sum": out["vis_sum"]}
            wb = {"per_joint": want["per_joint"][b][:, mask[b]], "vis_sum": want["vis_sum"][b]}
            keys = ("per_joint", "vis_sum")
            assert float(out["per_joint"].max()) <= 2.0 ** -22 * scale             # aligned exactly
        else:
            wb = {k: want[k][b] for k in keys}
        for k in keys:
            r = float((np.abs(out[k] - wb[k]) / (2.0 ** -22 * np.maximum(np.abs(wb[k]), scale))).max())
            key = (k, min(int(nvis[b]), 4))
            worst[key] = max(worst.get(key, 0.0), r)
    print(f"procrustes_vis_kernel B={B} S={S} J={J}: worst error / bar by (output, visible joints; 4 = more) {({k: round(v, 4) for k, v in worst.items()})}")
    assert max(worst.values()) <= 1.0, worst


def test_procrustes_vis_g21_cases(dev, golden_dir):
    cases = R.procrustes_cases()
    g21 = np.load(os.path.join(golden_dir, "g21_procrustes_rank1.npz"))
    for n in ("one_visible", "two_visible", "three_visible", "masked_random"):
        c = cases[n]
        got = _procrustes_abi(dev, c["pred"][None, None], c["gt"][None], mask=c["mask"][None], align=True)
        out = {k: _np(got[k]) for k in ALL5}
        have = R.determined(c, out)
        scale = float(np.abs(c["gt"]).max())
        for want in [R.determined(c, R.case_want(c))] + ([g21[f"{n}_want"]] if n in R.G21_CASES else []):
            r = float((np.abs(have - want) / (2.0 ** -22 * np.maximum(np.abs(want), scale))).max())
            print(f"procrustes_vis_kernel {n}: error / bar {r:.4f}")
            assert r <= 1.0, (n, r)


# ------------------------------------------------------------------------------------------------ diversity
@pytest.mark.parametrize("regime", R.REGIMES)
def test_diversity_matches_float64_within_the_rounding_bound(dev, regime):
    from egohmr_amd import metrics as M
    worst = {}
    for name, kw in R.diversity_cases():
        if not name.endswith(regime):
            continue
        want = R.diversity(**kw)
        m = None if kw["mask"] is None else torch.from_numpy(kw["mask"]).to(dev)
        sd, apd = M.diversity(_t(kw["joints"], dev), m, invert=kw["invert"])
        for k, v in (("std", sd), ("apd", apd)):
            r = R.ratio(_np(v), want[k], want[k + "_bound"])
            worst[k] = max(worst.get(k, 0.0), r)
            assert r <= 1.0, (name, k, r, _np(v), want[k], want[k + "_bound"])
        if "_none_" in name or "_S1_" in name:
            assert bool(torch.isnan(sd).all()) and bool(torch.isnan(apd).all()), name
    print(f"diversity_kernel, {regime}: worst error / bound {({k: round(v, 4) for k, v in worst.items()})}")


def test_diversity_refuses_more_joints_than_lanes(dev):
    from egohmr_amd import _lib, metrics as M
    with pytest.raises(_lib.EgoHMRHipError):
        M.diversity(torch.zeros(2, 3, 65, 3, device=dev))


# ------------------------------------------------------------------------------------------------ nearest neighbour
@pytest.mark.parametrize("regime", R.REGIMES)
def test_nn_dist2_matches_float64_within_the_rounding_bound(dev, regime):
    from egohmr_amd import metrics as M
    worst, worst_idx = 0.0, 0.0
    for name, kw, planted in R.nn_cases():
        if not name.endswith(regime):
            continue
        want = R.nn_dist2(**kw)
        x, y = _t(kw["x"], dev), _t(kw["y"], dev)
        d, idx = M.nn_dist2(x, y, return_idx=True)
        r = R.ratio(_np(d), want["dist2"], want["dist2_bound"])
        worst = max(worst, r)
        assert r <= 1.0, (name, r)
        idx = idx.cpu().numpy().astype(np.int64)
        assert idx.min() >= 0 and idx.max() < kw["y"].shape[1], name
        picked = ((kw["x"].astype(np.float64) - np.take_along_axis(kw["y"].astype(np.float64), idx[..., None], 1)) ** 2).sum(-1)
        lim = want["dist2"] * (1 + R.RHO_NN) / (1 - R.RHO_NN) + 2.0 ** -126
        worst_idx = max(worst_idx, float((picked / lim).max()))
        assert (picked <= lim).all(), name                                       # the returned index attains the minimum
        for b, q, pos in planted:
            assert idx[b, q] == pos, (name, b, q, pos, idx[b, q])
        assert torch.equal(M.nn_dist2(x, y), d), name                            # idx NULL
    print(f"nn_dist2_kernel, {regime}: worst error / bound {worst:.3f}; true d2 of the returned index / its limit {worst_idx:.7f}")


def test_nn_dist2_integer_lattice_is_exact_and_first_minimum_wins(dev):
    from egohmr_amd import metrics as M
    kw = R.nn_lattice_case()
    want = R.nn_dist2(**kw)
    d, idx = M.nn_dist2(_t(kw["x"], dev), _t(kw["y"], dev), return_idx=True)
    assert np.array_equal(_np(d), want["dist2"])                                  # every operation exact: bit for bit
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), want["idx"])
    assert (want["idx"][:, 0] == 0).all()                                         # reference points 0, 2048 (next tile) and 4099 are the same point
    ties = int((R.nn_dist2(wrong="last_min", **kw)["idx"] != want["idx"]).sum())
    print(f"nn_dist2_kernel lattice: dist2 bit-equal, idx equal, {ties} queries with tied minima")
    assert ties > 10


def test_contact_score_is_strict_at_the_threshold(dev):
    from egohmr_amd import metrics as M
    x = torch.zeros(3, 2, 3, device=dev)
    x[:, 1, 0] = 10.0
    y = torch.tensor([[[0.5, 0.0, 0.0], [0.0, 3.0, 0.0]], [[0.0, -0.5, 0.0], [0.0, 0.0, 4.0]], [[0.0, 0.0, 0.25], [5.0, 0.0, 0.0]]], device=dev)
    assert M.contact_score(x, y, 0.25).cpu().tolist() == [False, False, True]   # d2 = 0.25 exactly is NOT < 0.25; 0.0625 is
