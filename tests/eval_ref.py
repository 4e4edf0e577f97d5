"""Float64 references, float32 rounding bounds and deliberately wrong variants for the evaluation kernels (csrc/eval.hip, csrc/metrics.hip):
point_errors_kernel, procrustes_kernel, procrustes_vis_kernel, diversity_kernel, nn_dist2_kernel.  numpy only; test infrastructure
(tests/test_eval_ref_cpu.py checks this module without a GPU, tests/test_gpu_eval.py checks the kernels against it).

Every reference takes the float32 inputs the kernel gets and computes from their exact values in float64.  The Procrustes references are
oracle.metrics.procrustes and tests.test_stage1_cpu.procrustes_vis_np (both pinned by goldens written by the reference itself); what this module
needs to vary inside them - the completion of a rank-deficient SVD, the wrong variants' Z - it varies by wrapping numpy.linalg.svd / det around
the call, not by restating the solve.

Rounding bounds of the three float32 kernels
--------------------------------------------
u = 2^-24 (round to nearest, float32); fl(x op y) = (x op y)(1 + d), |d| <= u, for +, -, *, / and sqrt (hipcc's defaults: IEEE division and
square root, no fast-math); gamma(k) = k u / (1 - k u) bounds the accumulated factor of k roundings.  A fused multiply-add rounds once where the
restated count has two, and every sum of squares or distances below has non-negative terms, so contraction only lowers the error.  FLUSH = 2^-63 is
sqrt of the smallest normal float32: what a sum of squares that underflows can cost a distance.

* distance of two float32 points, e = sqrt(dx^2 + dy^2 + dz^2) with computed differences dx^ = dx + Ddx:
    three products and two additions: the computed radicand is sum(d^_c^2) (1 + th), |th| <= gamma(3); the square root adds one rounding:
        e^ = |d^| sqrt(1 + th) (1 + d),     | |d^| - |d| | <= |Dd|   (triangle inequality of the Euclidean norm)
    so with EPS_NORM = sqrt(1 + gamma(3)) (1 + u) - 1 (about 2.5 u):     |e^ - e| <= |Dd| (1 + EPS_NORM) + e EPS_NORM + FLUSH.

* point errors: d = (p - op) - (g - og): a = fl(p - op) and b = fl(g - og) round once each WHEN an origin is subtracted (x - 0 is exact), the outer
  subtraction rounds once:  |Dd_c| <= u (|a_c| [origin] + |b_c| [origin]) (1 + u) + u |d_c|.
  Sums: a thread adds its ceil(P / 256) terms one after the other, the wave sum is 4 DPP steps + 3 additions of the row sums (WAVE_DEPTH = 7), the
  block adds the 4 wave sums (3 more): every term passes through at most depth = ceil(P / 256) + 10 additions, the terms are >= 0:
        |sum^ - sum| <= sum(De) + gamma(depth) sum(e + De);    mean = sum / P: one more rounding (P < 2^24 is exact in float32).
  vis_sum is the same sum over the masked terms; invis_sum = fl(sum_all^ - sum_vis^) inherits both sums' bounds plus one rounding of the difference.
  Without a mask vis_sum is the whole sum and invis_sum is exactly 0.

* diversity, per joint and coordinate, S samples a_s in one thread:
    mu^ = fl(sum / S): S additions + 1 division, terms of either sign:      Dmu = gamma(S + 1) mean|a_s|
    d^_s = fl(a_s - mu^):                                                    Dd_s = Dmu + u (|d_s| + Dmu)
    var^ = sum of S squares, a product and at most S additions each, then / (S - 1) and sqrt:
        sigma^ = sqrt(sum d^_s^2 (1 + th_s)) sqrt(1 + d) (1 + d') / sqrt(S - 1),   |th_s| <= gamma(S + 1)
        Dsigma = (|Dd|_2 (1 + eps) + sqrt(var) eps) / sqrt(S - 1),   1 + eps = sqrt((1 + gamma(S + 1)) (1 + u)) (1 + u)
    sd_j = (sigma_x + sigma_y + sigma_z) / 3: 2 additions + 1 division of non-negative terms: gamma(3)
    std = wave sum over the selected joints / count: WAVE_DEPTH additions + 1 division: gamma(8); the count is a sum of 0 / 1: exact.
  APD: dx = fl(u - v) rounds once per coordinate (|Dd| <= u e), the distance as above, times 2 (exact), summed over the Np = S (S - 1) / 2 pairs one
  after the other (gamma(Np)), then the wave sum and three divisions (count, S, S - 1; the last / 2 is exact): gamma(WAVE_DEPTH + 3).
  An empty selection or S = 1 is 0 / 0 = NaN in the kernel and in the reference alike; a bound is NaN there and NaN must meet NaN.

* nearest neighbour: dx = fl(px - X) rounds once, so the computed squared distance of EVERY candidate k is d2_k (1 + rho_k) with
  |rho_k| <= RHO_NN = (1 + u)^2 (1 + gamma(3)) - 1 (about 5 u).  The minimum of values each within a factor (1 +- RHO_NN) of the true ones is within
  that factor of the true minimum:  |dist2^ - dist2| <= RHO_NN dist2 (+ 2^-126 for underflow), whichever candidate wins.  The index is not
  determined when two candidates are closer than that; the candidate the kernel picks has a true d2 <= dist2 (1 + RHO_NN) / (1 - RHO_NN).
  With small integer coordinates every operation is exact: dist2 is bit-equal and idx is the first argmin.

The two Procrustes kernels compute in float64 and round once to float32 on store: their bar is procrustes_bar, 2^-22 max(|want|, cloud scale): the
store's 2^-24 relative plus a float64 solve whose error, for singular-value gaps above 1e-3 (test_eval_ref_cpu checks the cases), stays below 1e-12,
times four.
"""
import contextlib
import math

import numpy as np

from oracle import metrics as om
from tests.test_stage1_cpu import procrustes_vis_np

U = 2.0 ** -24
FLUSH = 2.0 ** -63
WAVE_DEPTH = 7                      # row16_sum's 4 DPP steps + the 3 additions of the 4 row sums (csrc/common.h wave_sum)
NN_TILE = 2048


def gamma(k):
    return k * U / (1.0 - k * U)


EPS_NORM = math.sqrt(1.0 + gamma(3)) * (1.0 + U) - 1.0
RHO_NN = (1.0 + U) ** 2 * (1.0 + gamma(3)) - 1.0


def ratio(got, want, bound):
    """max |got - want| / bound over the elements; NaN must meet NaN (else inf), a zero bound demands equality."""
    got, want, bound = np.broadcast_arrays(np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64))
    if got.size == 0:
        return 0.0
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return float("inf")
    ok = ~wn
    diff = np.abs(got[ok] - want[ok])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0.0, 0.0, diff / bound[ok])
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ point errors
POINT_WRONG = ("gt_row_bs", "drop_last", "stride_P", "mask_next", "origin_pred_only")


def point_errors(pred, gt, P, origin_point=-1, pred_origin=None, gt_origin=None, mask=None, wrong=None):
    """pred [B,S,PP,3], gt [B,GP,3] float32, the first P points of each; origins [B,S,3] / [B,3] or origin_point; mask [B,P] bool.
    -> dict of float64 per_point [B,S,P], mean, vis_sum, invis_sum [B,S] and `<name>_bound` for each.
    wrong: gt_row_bs (gt row (b S + s) mod B instead of b), drop_last (the last point left out of everything), stride_P (pred rows P apart instead of
    PP), mask_next (the next item's mask row), origin_pred_only (the gt origin not subtracted)."""
    assert wrong is None or wrong in POINT_WRONG
    B, S, PP = pred.shape[:3]
    p = np.asarray(pred, np.float64)
    if wrong == "stride_P":
        flat = p.reshape(-1)
        p = np.stack([flat[i * P * 3:(i + 1) * P * 3].reshape(P, 3) for i in range(B * S)]).reshape(B, S, P, 3)
    p = p[:, :, :P]
    g = np.asarray(gt, np.float64)[:, None, :P]
    if wrong == "gt_row_bs":
        g = np.asarray(gt, np.float64)[(np.arange(B * S) % B).reshape(B, S)][:, :, :P]
    op, og = np.zeros((B, S, 1, 3)), np.zeros((B, 1, 1, 3))
    has_op, has_og = pred_origin is not None or origin_point >= 0, gt_origin is not None or origin_point >= 0
    if pred_origin is not None:
        op = np.asarray(pred_origin, np.float64).reshape(B, S, 1, 3)
    if gt_origin is not None:
        og = np.asarray(gt_origin, np.float64).reshape(B, 1, 1, 3)
    if origin_point >= 0:
        op, og = p[:, :, origin_point:origin_point + 1], g[:, :, origin_point:origin_point + 1]
    if wrong == "origin_pred_only":
        og = np.zeros_like(og)
    a, b = p - op, g - og
    d = a - b
    e = np.sqrt((d * d).sum(-1))
    dd = (U * np.abs(a) * has_op + U * np.abs(b) * has_og) * (1 + U) + U * np.abs(d)
    de = np.sqrt((dd * dd).sum(-1)) * (1 + EPS_NORM) + e * EPS_NORM + FLUSH
    if wrong == "drop_last":
        e, de = e.copy(), de.copy()
        e[..., P - 1] = 0.0
        de[..., P - 1] = 0.0
    depth = -(-P // 256) + WAVE_DEPTH + 3
    tot, dtot = e.sum(-1), de.sum(-1)
    out = {"per_point": e, "per_point_bound": de, "mean": tot / P, "mean_bound": (dtot + gamma(depth + 1) * (tot + dtot)) / P}
    all_b = dtot + gamma(depth) * (tot + dtot)
    if mask is None:
        out.update(vis_sum=tot, vis_sum_bound=all_b, invis_sum=np.zeros_like(tot), invis_sum_bound=np.zeros_like(tot))
    else:
        m = np.asarray(mask, bool)
        if wrong == "mask_next":
            m = np.roll(m, -1, axis=0)
        m = m[:, None, :]
        vis, dv = (e * m).sum(-1), (de * m).sum(-1)
        vis_b = dv + gamma(depth) * (vis + dv)
        inv = (e * ~m).sum(-1)
        out.update(vis_sum=vis, vis_sum_bound=vis_b, invis_sum=inv, invis_sum_bound=all_b + vis_b + U * (inv + all_b + vis_b))
    return out


_f32 = np.float32


def _halve32(x):
    """float32 pairwise sum over the last axis: adjacent pairs, level by level (depth ceil(log2 n))."""
    x = np.asarray(x, _f32)
    while x.shape[-1] > 1:
        if x.shape[-1] % 2:
            x = np.concatenate([x, np.zeros(x.shape[:-1] + (1,), _f32)], -1)
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _wave_sum32(x):
    """csrc/common.h wave_sum on [..., 64] float32: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror, then rows 0 + 16 + 32 + 48."""
    x = np.asarray(x, _f32)
    lane = np.arange(64)
    for perm in (lane ^ 1, lane ^ 2, (lane & ~7) | (7 - (lane & 7)), (lane & ~15) | (15 - (lane & 15))):
        x = x + x[..., perm]
    return ((x[..., 0] + x[..., 16]) + x[..., 32]) + x[..., 48]


def _block_sum32(e, order):
    """The block's sum of e [..., P] float32.  'sequential': the kernel's own order (a thread adds its strided terms one after the other, wave_sum,
    the four wave sums left to right).  'pairwise': each thread's terms and the 256 partial sums by pairwise halving.  (One running sum over all P
    terms would be another algorithm: P - 1 additions deep where the kernel has ceil(P / 256) + 10.)"""
    P = e.shape[-1]
    R = -(-P // 256)
    e = np.concatenate([np.asarray(e, _f32), np.zeros(e.shape[:-1] + (R * 256 - P,), _f32)], -1).reshape(e.shape[:-1] + (R, 256))
    if order == "sequential":
        part = np.zeros(e.shape[:-2] + (256,), _f32)
        for r in range(R):
            part = part + e[..., r, :]
        w = _wave_sum32(part.reshape(part.shape[:-1] + (4, 64)))
        return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
    return _halve32(_halve32(np.swapaxes(e, -1, -2)))


def point_errors_f32(pred, gt, P, origin_point=-1, pred_origin=None, gt_origin=None, mask=None, order="sequential"):
    """point_errors_kernel restated in float32 numpy (every operation rounds to float32), sums in one of _block_sum32's two orders."""
    B, S = pred.shape[:2]
    p, g = np.asarray(pred, _f32)[:, :, :P], np.asarray(gt, _f32)[:, None, :P]
    op, og = np.zeros((B, S, 1, 3), _f32), np.zeros((B, 1, 1, 3), _f32)
    if pred_origin is not None:
        op = np.asarray(pred_origin, _f32).reshape(B, S, 1, 3)
    if gt_origin is not None:
        og = np.asarray(gt_origin, _f32).reshape(B, 1, 1, 3)
    if origin_point >= 0:
        op, og = p[:, :, origin_point:origin_point + 1], g[:, :, origin_point:origin_point + 1]
    d = (p - op) - (g - og)
    sq = d * d
    e = np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2] if order == "sequential" else sq[..., 0] + (sq[..., 1] + sq[..., 2]))
    assert e.dtype == _f32
    tot = _block_sum32(e, order)
    out = {"per_point": e, "mean": tot / _f32(P)}
    if mask is None:
        out.update(vis_sum=tot, invis_sum=np.zeros_like(tot))
    else:
        vis = _block_sum32(np.where(np.asarray(mask, bool)[:, None, :], e, _f32(0)), order)
        out.update(vis_sum=vis, invis_sum=tot - vis)
    return out


# ------------------------------------------------------------------------------------------------ diversity
DIVERSITY_WRONG = ("biased", "unordered", "div_J")


def diversity(joints, mask=None, invert=False, wrong=None):
    """joints [B,S,J,3] float32, mask [B,J] bool (None: all joints; invert: the unselected ones) -> dict std, apd [B] float64 + `_bound`s:
    the mean over the selected joints and the 3 coordinates of the unbiased std over the samples; the sum over ORDERED sample pairs and selected
    joints of the joint distance / n_selected / S / (S - 1) / 2 (the reference's normalisation, test_egohmr.py:471-494).
    wrong: biased (std with 1 / S), unordered (every pair once), div_J (divided by J, not by the selected count)."""
    assert wrong is None or wrong in DIVERSITY_WRONG
    a = np.asarray(joints, np.float64)
    B, S, J = a.shape[:3]
    sel = np.ones((B, J), bool) if mask is None else (np.asarray(mask, bool) != bool(invert))
    cnt = sel.sum(1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = a.mean(1)
        d = a - mu[:, None]
        var = (d * d).sum(1)
        den = S if wrong == "biased" else S - 1
        sig = np.sqrt(var / den)
        sd = sig.mean(-1)
        dmu = gamma(S + 1) * np.abs(a).mean(1)
        dd = dmu[:, None] + U * (np.abs(d) + dmu[:, None])
        eps = math.sqrt((1 + gamma(S + 1)) * (1 + U)) * (1 + U) - 1
        dsig = (np.sqrt((dd * dd).sum(1)) * (1 + eps) + np.sqrt(var) * eps) / np.sqrt(np.float64(den))
        dsd = (dsig.sum(-1) + gamma(3) * (sig + dsig).sum(-1)) / 3
        s0, ds0 = np.where(sel, sd, 0.0).sum(1), np.where(sel, dsd, 0.0).sum(1)
        div = np.float64(J) if wrong == "div_J" else cnt
        std, std_b = s0 / div, (ds0 + gamma(WAVE_DEPTH + 1) * (s0 + ds0)) / div
        i0, i1 = np.triu_indices(S, 1)
        e = np.sqrt(((a[:, i0] - a[:, i1]) ** 2).sum(-1))                       # [B,Np,J]
        de = U * e * (1 + EPS_NORM) + e * EPS_NORM + FLUSH
        w = 1.0 if wrong == "unordered" else 2.0
        pd, dpd = w * e.sum(1), w * de.sum(1)
        dpd = dpd + gamma(max(len(i0), 1)) * (pd + dpd)
        p0, dp0 = np.where(sel, pd, 0.0).sum(1), np.where(sel, dpd, 0.0).sum(1)
        norm = div * S * (S - 1) * 2
        apd, apd_b = p0 / norm, (dp0 + gamma(WAVE_DEPTH + 3) * (p0 + dp0)) / norm
    return {"std": std, "std_bound": std_b, "apd": apd, "apd_bound": apd_b}


def _seq32(x, axis):
    x = np.moveaxis(np.asarray(x, _f32), axis, 0)
    acc = np.zeros(x.shape[1:], _f32)
    for r in range(x.shape[0]):
        acc = acc + x[r]
    return acc


def diversity_f32(joints, mask=None, invert=False, order="sequential", one_pass=False):
    """diversity_kernel restated in float32 numpy; the sums over the samples and over the pairs run one after the other ('sequential', the kernel's
    order) or by pairwise halving.  one_pass: the variance as sum(a^2) - S mu^2 instead of the kernel's two passes - NOT the kernel; it is what the
    camera-frame cases exist to catch (test_eval_ref_cpu)."""
    a = np.asarray(joints, _f32)
    B, S, J = a.shape[:3]
    sel = np.ones((B, J), bool) if mask is None else (np.asarray(mask, bool) != bool(invert))
    red = (lambda x, axis: _seq32(x, axis)) if order == "sequential" else (lambda x, axis: _halve32(np.moveaxis(np.asarray(x, _f32), axis, -1)))
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = red(a, 1) / _f32(S)
        d = a - mu[:, None]
        ssq = np.maximum(red(a * a, 1) - _f32(S) * mu * mu, _f32(0)) if one_pass else red(d * d, 1)
        sig = np.sqrt(ssq / _f32(S - 1))
        sd = ((sig[..., 0] + sig[..., 1]) + sig[..., 2]) / _f32(3)
        i0, i1 = np.triu_indices(S, 1)
        df = a[:, i0] - a[:, i1]
        sq = df * df
        e = _f32(2) * np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])
        pd = red(e, 1) if len(i0) else np.zeros((B, J), _f32)

        def lanes(x):
            x = np.concatenate([np.where(sel, x, _f32(0)), np.zeros((B, 64 - J), _f32)], 1)
            return _wave_sum32(x) if order == "sequential" else _halve32(x)
        cnt = _f32(1) * sel.sum(1).astype(_f32)
        std = lanes(sd) / cnt
        apd = lanes(pd) / cnt / _f32(S) / _f32(S - 1) / _f32(2)
    assert std.dtype == _f32 and apd.dtype == _f32
    return {"std": std, "apd": apd}


# ------------------------------------------------------------------------------------------------ nearest neighbour
NN_WRONG = ("skip_last_tile", "last_min")


def nn_dist2(x, y, wrong=None):
    """x [B,P1,3], y [B,P2,3] float32 -> dict dist2 [B,P1] float64, idx [B,P1] (first minimum), dist2_bound.
    wrong: skip_last_tile (the last, partial tile of NN_TILE reference points is not searched), last_min (of equal minima the last one wins)."""
    assert wrong is None or wrong in NN_WRONG
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    P2 = y.shape[1]
    if wrong == "skip_last_tile" and P2 % NN_TILE:
        P2 = P2 // NN_TILE * NN_TILE
        if P2 == 0:
            d, idx = np.full(x.shape[:2], 3.4e38), np.zeros(x.shape[:2], np.int64)
            return {"dist2": d, "idx": idx, "dist2_bound": RHO_NN * d + 2.0 ** -126}
        y = y[:, :P2]
    if wrong == "last_min":
        d, idx = om.nn_dist2(x, y[:, ::-1])
        idx = P2 - 1 - idx
    else:
        d, idx = om.nn_dist2(x, y)
    return {"dist2": d, "idx": idx, "dist2_bound": RHO_NN * d + 2.0 ** -126}


def nn_dist2_f32(x, y, order="sequential"):
    """nn_dist2_kernel restated in float32 numpy: strict <, first minimum; the three squares added left to right or right to left."""
    x, y = np.asarray(x, _f32), np.asarray(y, _f32)
    d = np.empty(x.shape[:2], _f32)
    idx = np.empty(x.shape[:2], np.int64)
    for b in range(x.shape[0]):
        for s in range(0, x.shape[1], 256):
            df = x[b, s:s + 256, None, :] - y[b, None, :, :]
            sq = df * df
            d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2] if order == "sequential" else sq[..., 0] + (sq[..., 1] + sq[..., 2])
            idx[b, s:s + 256] = d2.argmin(1)
            d[b, s:s + 256] = d2.min(1)
    return {"dist2": d, "idx": idx}


# ------------------------------------------------------------------------------------------------ Procrustes
PROCRUSTES_WRONG = ("no_Z", "Z_largest", "b_mod")


def _rand_orth(rng, k):
    q, r = np.linalg.qr(rng.normal(size=(k, k)))
    return q * np.sign(np.diag(r))


@contextlib.contextmanager
def _linalg(svd=None, det=None):
    """numpy.linalg.svd / det replaced while the pinned references run (they look both up at call time)."""
    real = np.linalg.svd, np.linalg.det
    try:
        if svd is not None:
            np.linalg.svd = lambda K, *a, **k: svd(*real[0](K, *a, **k))
        if det is not None:
            np.linalg.det = lambda A, *a, **k: det(real[1](A, *a, **k))
        yield
    finally:
        np.linalg.svd, np.linalg.det = real


def _recompleted(rng, tol=1e-13):
    """An SVD whose null-space columns (singular value <= tol * the largest) are turned by a random orthogonal matrix, U's and V's independently:
    as valid a decomposition of a rank-deficient K as LAPACK's own."""
    def svd(U, s, Vh):
        shape = U.shape
        U, s2, Vh = U.reshape(-1, 3, 3).copy(), s.reshape(-1, 3), Vh.reshape(-1, 3, 3).copy()
        for i in range(len(U)):
            r = int((s2[i] > tol * s2[i, 0]).sum()) if s2[i, 0] > 0 else 0
            if r < 3:
                U[i][:, r:] = U[i][:, r:] @ _rand_orth(rng, 3 - r)
                Vh[i][r:, :] = _rand_orth(rng, 3 - r) @ Vh[i][r:, :]
        return U.reshape(shape), s, Vh.reshape(shape)
    return svd


def _solve_context(wrong, recomplete):
    if wrong == "no_Z":                                     # det(U V^T) taken for +1: R = V U^T, a reflection for a mirrored cloud
        return _linalg(det=np.abs)
    if wrong == "Z_largest":                                # the singular triplets in ascending order: the reference's Z[-1, -1] lands on the largest
        return _linalg(svd=lambda U, s, Vh: (U[..., ::-1], s[..., ::-1], Vh[..., ::-1, :]))
    if recomplete is not None:
        return _linalg(svd=_recompleted(recomplete))
    return contextlib.nullcontext()


def _gt_rows(B, S, wrong):
    i = np.arange(B * S)
    return i % B if wrong == "b_mod" else i // S


def _sums(e, mask, rows, B, S):
    """per_joint [n,J] -> dict per_joint [B,S,J], mean, vis_sum, invis_sum [B,S]"""
    m = np.ones(e.shape, bool) if mask is None else np.asarray(mask, bool)[rows]
    with np.errstate(invalid="ignore"):
        vis, inv = (e * m).sum(-1), (e * ~m).sum(-1)
    return {"per_joint": e.reshape(B, S, -1), "mean": e.mean(-1).reshape(B, S), "vis_sum": vis.reshape(B, S), "invis_sum": inv.reshape(B, S)}


def procrustes(pred, gt, mask=None, wrong=None, recomplete=None):
    """pred [B,S,J,3], gt [B,J,3] float32, mask [B,J] -> float64 aligned [B,S,J,3], per_joint [B,S,J], mean, vis_sum, invis_sum [B,S]
    (oracle.metrics.procrustes per pair).  wrong: no_Z, Z_largest, b_mod (gt row i mod B instead of i / S).  recomplete: a numpy Generator that
    re-completes the null space of every rank-deficient SVD (_recompleted)."""
    assert wrong is None or wrong in PROCRUSTES_WRONG
    B, S, J = pred.shape[:3]
    p = np.asarray(pred, np.float64).reshape(B * S, J, 3)
    rows = _gt_rows(B, S, wrong)
    g = np.asarray(gt, np.float64)[rows]
    with _solve_context(wrong, recomplete), np.errstate(divide="ignore", invalid="ignore"):
        al = np.stack([om.procrustes(p[i], g[i]) for i in range(B * S)])
    out = _sums(np.sqrt(((al - g) ** 2).sum(-1)), mask, rows, B, S)
    out["aligned"] = al.reshape(B, S, J, 3)
    return out


def procrustes_vis(pred, gt, align_mask, wrong=None, recomplete=None):
    """The visible-joint alignment: tests.test_stage1_cpu.procrustes_vis_np with the item's mask shared by its S samples; the same mask splits the sums
    by products, so a NaN error reaches both (test_egohmr.py:433-436).  No `aligned`: the pinned reference returns errors only."""
    assert wrong is None or wrong in PROCRUSTES_WRONG
    B, S, J = pred.shape[:3]
    rows = _gt_rows(B, S, wrong)
    m = np.asarray(align_mask, bool)
    with _solve_context(wrong, recomplete), np.errstate(divide="ignore", invalid="ignore"):
        e = procrustes_vis_np(m[rows], np.asarray(pred, np.float64).reshape(B * S, J, 3), np.asarray(gt, np.float64)[rows])
    return _sums(e, m, rows, B, S)


def procrustes_bar(want, gt):
    """2^-22 max(|want|, cloud scale) for an output whose leading axes are [B,S]: the cloud scale is the item's largest |gt coordinate| (the aligned
    points live in the frame of gt)."""
    want = np.asarray(want, np.float64)
    scale = np.abs(np.asarray(gt, np.float64)).reshape(len(gt), -1).max(1)
    scale = scale.reshape((len(gt),) + (1,) * (want.ndim - 1))
    return 2.0 ** -22 * np.maximum(np.nan_to_num(np.abs(want), nan=0.0), scale)


def singular_gaps(pred, gt, mask=None):
    """Relative gaps (s1 - s2) / s1, (s2 - s3) / s1 of K for one [J,3] pair (masked: the visible-joint alignment's K)."""
    w = np.ones((len(pred), 1)) if mask is None else np.asarray(mask, np.float64)[:, None]
    a, b = np.asarray(pred, np.float64) * w, np.asarray(gt, np.float64) * w
    s = np.linalg.svd((a - a.mean(0)).T @ (b - b.mean(0)), compute_uv=False)
    return (s[0] - s[1]) / s[0], (s[1] - s[2]) / s[0]


def _rot(g):
    q = _rand_orth(g, 3)
    return q * np.sign(np.linalg.det(q))


def procrustes_cases(J=24, seed=21):
    """Named single pairs (pred [J,3], gt [J,3] float32, mask [J] or None) for both Procrustes kernels.
    kind 'generic': every output is determined (and, but for the similarity copy's zero error, well conditioned);
    kind 'rank': K is rank deficient and `compare` names what the data determine:
        aligned      the whole aligned cloud (a collinear pred goes onto a line R fixes; K = 0 gives mu2)
        per_joint    every joint's error (rank 2 with the det constraint)
        vis_joint    the visible joint's error only (one visible joint: the invisible joints turn with the free rotation about the line)
        sum_e2       sum_j e_j^2 only (a collinear gt: the optimum's value is unique, the rotation about the line is free)
        nan          var1 = 0: everything NaN"""
    g = np.random.Generator(np.random.PCG64(seed))
    f = lambda a: np.asarray(a, np.float32)
    gt = f(g.normal(scale=0.3, size=(J, 3)))
    near = lambda: f(1.1 * gt @ _rot(g).T + g.normal(scale=0.04, size=(J, 3)) + g.normal(size=3))
    c = {}
    c["generic"] = dict(pred=near(), gt=gt, mask=None, kind="generic")
    c["mirrored"] = dict(pred=near() * f([1, 1, -1]), gt=gt, mask=None, kind="generic")
    p = near()
    p[:, 2] = 0.0
    c["planar_pred"] = dict(pred=p, gt=gt, mask=None, kind="generic")
    g2 = gt.copy()
    g2[:, 1] = 0.25
    c["planar_gt"] = dict(pred=near(), gt=g2, mask=None, kind="generic")
    c["similarity_copy"] = dict(pred=f(2.5 * gt @ _rot(g).T + np.array([0.3, -1.0, 2.0])), gt=gt, mask=None, kind="generic")
    m = g.random(J) < 0.6
    c["masked_random"] = dict(pred=near(), gt=gt, mask=m, kind="generic")
    m = np.zeros(J, bool)
    m[g.choice(J, 3, replace=False)] = True
    c["three_visible"] = dict(pred=near(), gt=gt, mask=m, kind="generic")
    # ---- rank deficient
    p = np.zeros((J, 3), np.float32)
    p[:, 0] = g.normal(size=J)
    c["x_axis_line"] = dict(pred=p, gt=gt, mask=None, kind="rank", compare="aligned")
    a, b = f(g.normal(size=(2, 3)))
    c["two_point_pred"] = dict(pred=f(np.where((np.arange(J) % 3 == 0)[:, None], a, b)), gt=gt, mask=None, kind="rank", compare="aligned")
    m = np.zeros(J, bool)
    m[g.integers(J)] = True
    c["one_visible"] = dict(pred=near(), gt=gt, mask=m, kind="rank", compare="vis_joint")
    m = np.zeros(J, bool)
    m[g.choice(J, 2, replace=False)] = True
    c["two_visible"] = dict(pred=near(), gt=gt, mask=m, kind="rank", compare="per_joint")
    c["gt_one_point"] = dict(pred=near(), gt=f(np.tile(g.normal(size=3), (J, 1))), mask=None, kind="rank", compare="aligned")
    gl = np.zeros((J, 3), np.float32)
    gl[:, 2] = g.normal(scale=0.3, size=J)
    c["gt_line"] = dict(pred=near(), gt=gl, mask=None, kind="rank", compare="sum_e2")
    c["pred_one_point"] = dict(pred=f(np.tile(g.normal(size=3), (J, 1))), gt=gt, mask=None, kind="rank", compare="nan")
    return c


G21_CASES = ("x_axis_line", "two_point_pred", "one_visible", "two_visible", "gt_one_point")


def case_want(case, recomplete=None, wrong=None):
    """The reference outputs of one procrustes_cases() entry as a [1,1,...] batch (masked entries: the visible-joint alignment)."""
    if case["mask"] is None:
        return procrustes(case["pred"][None, None], case["gt"][None], wrong=wrong, recomplete=recomplete)
    return procrustes_vis(case["pred"][None, None], case["gt"][None], case["mask"][None], wrong=wrong, recomplete=recomplete)


def determined(case, out):
    """What `compare` keeps of an output dict of the case (leading [1,1] stripped): the quantities the data determine."""
    kind = case.get("compare", "aligned" if case["mask"] is None else "per_joint")
    if kind == "aligned":
        return out["aligned"][0, 0]
    if kind == "per_joint":
        return out["per_joint"][0, 0]
    if kind == "vis_joint":
        return np.append(out["per_joint"][0, 0][case["mask"]], out["vis_sum"][0, 0])
    if kind == "sum_e2":
        return np.array([(out["per_joint"][0, 0] ** 2).sum()])
    return out["per_joint"][0, 0]          # nan


def write_check_cases(path, cases):
    """cases: list of procrustes_cases() entries -> the text format tools/procrustes_check.cpp reads."""
    with open(path, "w") as f:
        f.write(f"{len(cases)}\n")
        for c in cases:
            J = len(c["pred"])
            f.write(f"{J} {int(c['mask'] is not None)}\n")
            for j in range(J):
                vals = " ".join(f"{v:.9g}" for v in list(c["pred"][j]) + list(c["gt"][j]))
                f.write(f"{vals} {int(c['mask'][j]) if c['mask'] is not None else 1}\n")


def read_check_output(text, cases):
    rows = np.array([[float(v) for v in line.split()] for line in text.strip().splitlines()], np.float64)
    out, k = [], 0
    for c in cases:
        J = len(c["pred"])
        out.append(rows[k:k + J])
        k += J
    assert k == len(rows)
    return out


# ------------------------------------------------------------------------------------------------ the float32 kernels' cases
CAMERA = np.array([0.3, -1.0, 3.0])
REGIMES = ("unit", "camera")


def _clouds(g, regime, lead_pred, lead_gt, n):
    """pred [*lead_pred,n,3], gt [*lead_gt,n,3] float32 (lead_gt broadcasts into lead_pred by a middle axis of 1).  'unit': O(1) coordinates, independent
    clouds.  'camera': bodies about CAMERA metres from the origin, the prediction 5 - 10 mm off the truth."""
    if regime == "unit":
        return g.normal(size=(*lead_pred, n, 3)).astype(np.float32), g.normal(size=(*lead_gt, n, 3)).astype(np.float32)
    gt = (CAMERA + g.normal(scale=0.3, size=(*lead_gt, n, 3))).astype(np.float32)
    step = g.normal(size=(*lead_pred, n, 3))
    step *= g.uniform(5e-3, 10e-3, size=(*lead_pred, n, 1)) / np.linalg.norm(step, axis=-1, keepdims=True)
    return (gt[:, None] + step).astype(np.float32), gt


def point_cases():
    """(id, kwargs of point_errors) over the block-size edges of P, the (B, S) that show a wrong i / S, unequal strides with NaN tails, every origin
    form and mask kind, both regimes."""
    specs = [dict(P=P, BS=(3, 4)) for P in (1, 24, 255, 256, 257, 6890)]
    specs += [dict(P=257, BS=bs) for bs in ((1, 1), (2, 33))]
    specs += [dict(P=24, BS=(2, 33), PP=45, GP=30, origin_point=o) for o in (-1, 0, 23)]
    specs += [dict(P=257, BS=(3, 4), origins=o) for o in ("both", "pred", "gt")]
    specs += [dict(P=24, BS=(3, 4), mask=m) for m in ("absent", "all", "none")]
    out = []
    for k, sp in enumerate(specs):
        for regime in REGIMES:
            g = np.random.Generator(np.random.PCG64(5000 + 2 * k + (regime == "camera")))
            (B, S), P = sp["BS"], sp["P"]
            PP, GP = sp.get("PP", P), sp.get("GP", P)
            pred, gt = _clouds(g, regime, (B, S), (B,), max(PP, GP))
            pred, gt = np.ascontiguousarray(pred[:, :, :PP]), np.ascontiguousarray(gt[:, :GP])
            pred[:, :, P:], gt[:, P:] = np.nan, np.nan                      # the unused tail points
            kw = dict(pred=pred, gt=gt, P=P, origin_point=sp.get("origin_point", -1))
            o = sp.get("origins")
            if o in ("both", "pred"):
                kw["pred_origin"] = (pred[:, :, 0] + g.normal(scale=0.01, size=(B, S, 3))).astype(np.float32)
            if o in ("both", "gt"):
                kw["gt_origin"] = (gt[:, 0] + g.normal(scale=0.01, size=(B, 3))).astype(np.float32)
            mk = sp.get("mask", "random")
            kw["mask"] = {"absent": None, "all": np.ones((B, P), bool), "none": np.zeros((B, P), bool), "random": g.random((B, P)) < 0.5}[mk]
            name = f"P{P}_B{B}S{S}_pp{PP}gp{GP}_o{kw['origin_point']}{o or ''}_m{mk}_{regime}"
            out.append((name, kw))
    return out


def diversity_cases():
    """(id, kwargs of diversity): every J x S at B = 5 with a random selection, every selection kind at J = 24, S = 3, and B = 1; both regimes."""
    specs = [dict(J=J, S=S, B=5, sel="random") for J in (1, 24, 45, 63, 64) for S in (1, 2, 3, 50)]
    specs += [dict(J=24, S=3, B=5, sel=s) for s in ("absent", "all", "none", "single", "invert")]
    specs += [dict(J=J, S=S, B=1, sel="random") for J, S in ((24, 50), (64, 2))]
    out = []
    for k, sp in enumerate(specs):
        for regime in REGIMES:
            g = np.random.Generator(np.random.PCG64(6000 + 2 * k + (regime == "camera")))
            B, S, J = sp["B"], sp["S"], sp["J"]
            a, _ = _clouds(g, regime, (B, S), (B,), J)
            rnd = g.random((B, J)) < 0.6
            rnd[:, 0] |= ~rnd.any(1)                                        # ("none" is its own case)
            single = np.zeros((B, J), bool)
            single[np.arange(B), g.integers(J, size=B)] = True
            mask = {"absent": None, "all": np.ones((B, J), bool), "none": np.zeros((B, J), bool), "single": single, "random": rnd, "invert": rnd}[sp["sel"]]
            out.append((f"J{J}_S{S}_B{B}_{sp['sel']}_{regime}", dict(joints=a, mask=mask, invert=sp["sel"] == "invert")))
    return out


def nn_cases():
    """(id, kwargs of nn_dist2, planted) over the query-block edges of P1 and the tile edges of P2, both regimes; for P2 >= 2049 the nearest point of
    four queries is planted at reference index 0, 2047, 2048 and P2 - 1 (planted: list of (b, query, index))."""
    out = []
    k = 0
    for P1 in (1, 255, 256, 257, 600):
        for P2 in (1, 3, 4, 5, 2047, 2048, 2049, 4096, 4100):
            for regime in REGIMES:
                k += 1
                B = 3 if P1 == 257 else 1
                g = np.random.Generator(np.random.PCG64(7000 + k))
                if regime == "unit":
                    x, y = g.uniform(-1, 1, size=(B, P1, 3)).astype(np.float32), g.uniform(-1, 1, size=(B, P2, 3)).astype(np.float32)
                else:
                    x = (CAMERA + g.normal(scale=0.3, size=(B, P1, 3))).astype(np.float32)
                    y = (CAMERA + g.normal(scale=0.3, size=(B, P2, 3))).astype(np.float32)
                    n = min(P1, P2)                                             # scene points 5 - 10 mm from body vertices
                    step = g.normal(size=(B, n, 3))
                    step *= g.uniform(5e-3, 10e-3, size=(B, n, 1)) / np.linalg.norm(step, axis=-1, keepdims=True)
                    y[:, g.permutation(P2)[:n]] = (x[:, :n] + step).astype(np.float32)
                planted = []
                if P2 >= 2049 and P1 >= 4:
                    for q, pos in enumerate(sorted({0, 2047, 2048, P2 - 1})):
                        for b in range(B):
                            y[b, pos] = x[b, q] + np.float32(1e-4)
                            planted.append((b, q, pos))
                out.append((f"P1_{P1}_P2_{P2}_B{B}_{regime}", dict(x=x, y=y), planted))
    return out


def nn_lattice_case(seed=8):
    """Small integer coordinates: every difference, square and sum is exact in float32.  4100 reference points on a 17^3 lattice (duplicates, hence
    tied minima, are certain), 300 queries, plus constructed ties: queries midway between lattice points and a duplicate of reference point 0 at the
    very end and across the tile edge."""
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.integers(-8, 9, size=(2, 300, 3)).astype(np.float32)
    y = g.integers(-8, 9, size=(2, 4100, 3)).astype(np.float32)
    y[:, 2048], y[:, 4099] = y[:, 0], y[:, 0]
    x[:, 0] = y[:, 0]
    y[:, 2047], y[:, 2049] = x[:, 1] + np.float32([1, 0, 0]), x[:, 1] - np.float32([1, 0, 0])
    return dict(x=x, y=y)
