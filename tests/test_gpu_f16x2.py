"""GPU (MI355X): the two-term split-f16 tier of the hidden graph convs (csrc/gcn_tile.hip, P = 2; ehm_gcn_set_precision mode 3) and its place in
the calibrated precision schedule (ehm_sample_desc.twoterm_steps, EgoHMR.f16x2_steps).

A two-term product is a_hi * (w_hi + w_lo): the operands, buffers and stores of the three-term path, without the al * wh MFMAs and without the
reads of the activation lo fragments.  So
  * on activations whose lo halves are all zero the dropped term is exactly zero and the result must equal the three-term one element for element;
  * on general activations it is the three-term conv of the activations' f16 hi halves: checked against float64 of x_hi . W with the bound of the
    split-f16 conv test (tests/test_gpu_gcn.py::test_hidden_layer_vs_fp64, tier 'f16x3': `_hidden_tol`), which that test derives and this one reuses;
  * chained launch == per-conv launches, fused step launches == per-step launches, bit for bit, as for the other tiers.
Every test prints its figures before it asserts."""
import ctypes as C

import pytest
import torch

import test_gpu_gcn as tg                      # helpers only (layers, handle, pack / unpack, the float64 bound)
from egohmr_amd import synthetic as syn

pytestmark = pytest.mark.gpu

TILE = 192
F16X3, F16X2 = 1, 3                            # EHM_PREC_*


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from egohmr_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def adj(dev):
    from egohmr_amd.model import smpl_tree_adjacency
    return smpl_tree_adjacency().to(dev)


def _ck(rc, L):
    assert rc == 0, (rc, L.ehm_last_error())


def _handle(L, dev, adj, g, hid, n_hidden):
    layers = [tg._syn_layer(g, hid, hid, dev) for _ in range(n_hidden)]
    h, keep = tg._create(L, dev, adj, tg._syn_layer(g, hid, hid, dev), layers, tg._syn_layer(g, hid, 6, dev, bn=False), hid)
    return h, keep, layers


def _conv(L, h, prec, layer, Xp, Rp, rows_pad, hid, dev):
    """one hidden conv of the handle in precision `prec` -> the raw output buffer (one spare tile of NaN canary behind it, checked)"""
    _ck(L.ehm_gcn_set_precision(h, prec), L)
    Y = torch.full((rows_pad + TILE, hid), float("nan"), device=dev)
    _ck(L.ehm_gcn_hidden_layer(h, layer, Xp.data_ptr(), Rp.data_ptr() if Rp is not None else None, Y.data_ptr(), rows_pad, None), L)
    _ck(L.ehm_gcn_stack_status(h, None), L)
    assert torch.isnan(Y[rows_pad:]).all(), "write past rows_pad"
    return Y[:rows_pad]


# (rows, rows_pad): one row tile; 200 rows padded to two tiles (a ragged second tile)
ROWS = [(192, 192), (200, 384)]
# the last conv of the handle (layer 7) writes float32 rows, every other one X2 rows
LAYERS = [(2, "x2"), (7, "f32")]


@pytest.mark.parametrize("hid", [64, 192])
def test_dropped_term_is_exact_on_f16_activations(L, dev, adj, hid):
    """Activations exactly representable in f16 (every lo half 0): P = 2 == P = 3, element for element, no tolerance."""
    g = tg._rng(4200 + hid)
    h, keep, _ = _handle(L, dev, adj, g, hid, 8)
    try:
        for rows, rows_pad in ROWS:
            X = torch.zeros(rows_pad, hid, device=dev)
            X[:rows] = torch.relu(tg._t(g.normal(size=(rows, hid)), dev)).half().float()
            R = torch.zeros(rows_pad, hid, device=dev)
            R[:rows] = tg._t(g.normal(size=(rows, hid)), dev)                       # (the residual is read in full by both: any values)
            Xp, Rp = tg._pack(L, X, "x2"), tg._pack(L, R, "x2")
            lo = Xp.view(torch.int16).view(rows_pad, hid // 32, 2, 32)[:, :, 1]
            assert int(lo.abs().max()) == 0, "the test's activations must have zero lo halves"
            for layer, out_fmt in LAYERS:
                for res in (False, True):
                    y3 = _conv(L, h, F16X3, layer, Xp, Rp if res else None, rows_pad, hid, dev)
                    y2 = _conv(L, h, F16X2, layer, Xp, Rp if res else None, rows_pad, hid, dev)
                    ne = int((y2.view(torch.int32) != y3.view(torch.int32)).sum())
                    print(f"[exact hid={hid} rows={rows}/{rows_pad} layer={layer} ({out_fmt}) res={int(res)}] differing words: {ne}")
                    assert torch.isfinite(tg._unpack(L, y3, out_fmt, rows, hid)).all()
                    assert ne == 0
    finally:
        L.ehm_gcn_destroy(h)


@pytest.mark.parametrize("hid", [64, 192])
def test_general_activations_vs_fp64_of_the_hi_halves(L, dev, adj, hid):
    """General activations: P = 2 against float64 of x_hi . W (+ epilogue) within the split-f16 conv bound - and really another result than P = 3."""
    g = tg._rng(4300 + hid)
    h, keep, layers = _handle(L, dev, adj, g, hid, 8)
    try:
        for rows, rows_pad in ROWS:
            bodies = rows_pad // 24
            X = torch.zeros(rows_pad, hid, device=dev)
            X[:rows] = torch.relu(tg._t(g.normal(size=(rows, hid)), dev))
            R = torch.zeros(rows_pad, hid, device=dev)
            R[:rows] = torch.relu(tg._t(g.normal(size=(rows, hid)), dev))
            Xp, Rp = tg._pack(L, X, "x2"), tg._pack(L, R, "x2")
            # the hi halves as stored (X2 rows: 32 hi | 32 lo per 32 k).  Not rn_f16(hi + lo): where lo is exactly half an ulp of hi that tie rounds
            # to the even neighbour, which need not be hi
            Xhi = Xp.view(torch.float16).view(rows_pad, hid // 32, 2, 32)[:, :, 0].reshape(rows_pad, hid).double().view(bodies, 24, hid)
            assert float((Xhi.view(rows_pad, hid) - X.double()).abs().max()) > 0                     # (the lo halves are live)
            Rk = tg._unpack(L, Rp, "x2", rows_pad, hid).double().view(bodies, 24, hid)
            for layer, out_fmt in LAYERS:
                for res in (False, True):
                    y2 = _conv(L, h, F16X2, layer, Xp, Rp if res else None, rows_pad, hid, dev)
                    y3 = _conv(L, h, F16X3, layer, Xp, Rp if res else None, rows_pad, hid, dev)
                    got = tg._unpack(L, y2, out_fmt, rows_pad, hid).view(bodies, 24, hid)
                    ly = layers[layer]
                    ref, tol = tg._hidden_tol(Xhi, ly, adj, "f16x3", tg._w_scale(ly["W"]), Rk if res else None, out_fmt)
                    r, e = tg._ratio(got, ref, tol)
                    d23 = float((got.double() - tg._unpack(L, y3, out_fmt, rows_pad, hid).view(bodies, 24, hid).double()).abs().max())
                    print(f"[general hid={hid} rows={rows}/{rows_pad} layer={layer} ({out_fmt}) res={int(res)}] max|err| {e:.3e}  max err/bound {r:.3f}  "
                          f"max|P2 - P3| {d23:.3e}")
                    assert r <= 1.0, r
                    assert d23 > 0.0, "the two-term launch returned the three-term result"
    finally:
        L.ehm_gcn_destroy(h)


def test_chained_launch_equals_per_conv_launches(L, dev, adj):
    """gcn_hidden_chain_kernel<2, 4> over 4 hidden convs, 2 row tiles, hid 128 == the same convs one launch each (gcn_hidden_tile_kernel<2>)."""
    hid, rows, rows_pad, nl = 128, 16 * 24, 384, 4
    g = tg._rng(4400)
    h, keep, _ = _handle(L, dev, adj, g, hid, nl)
    try:
        _ck(L.ehm_gcn_set_precision(h, F16X2), L)
        X0 = torch.zeros(rows_pad, hid, device=dev)
        X0[:rows] = torch.relu(tg._t(g.normal(size=(rows, hid)), dev))
        X0p = tg._pack(L, X0, "x2")
        ref = [X0p.clone(), torch.zeros_like(X0p), torch.zeros_like(X0p)]
        cur = 0
        for blk in range(nl // 2):
            y2 = 2 if cur == 0 else 0
            for i, (src, res, dst) in enumerate(((cur, None, 1), (1, cur, y2))):
                _ck(L.ehm_gcn_hidden_layer(h, 2 * blk + i, ref[src].data_ptr(), ref[res].data_ptr() if res is not None else None, ref[dst].data_ptr(),
                                           rows_pad, None), L)
            cur = y2
        _ck(L.ehm_gcn_stack_status(h, None), L)
        bufs_t = [X0p.clone(), torch.full_like(X0p, float("nan")), torch.full_like(X0p, float("nan"))]
        bufs = (C.c_void_p * 3)(*[t.data_ptr() for t in bufs_t])
        resi = C.c_int(-1)
        _ck(L.ehm_gcn_hidden_stack(h, bufs, rows_pad, C.byref(resi), None), L)
        _ck(L.ehm_gcn_stack_status(h, None), L)
        assert resi.value == cur
        out = tg._unpack(L, bufs_t[cur], "f32", rows, hid)                          # the chain's last conv writes float32 rows
        ne = int((bufs_t[cur][:rows].view(torch.int32) != ref[cur][:rows].view(torch.int32)).sum())
        print(f"[chain<2, 4> hid={hid} convs={nl} row tiles={rows_pad // TILE}] differing words vs per-conv launches: {ne}; max|y| {float(out.abs().max()):.3f}")
        assert torch.isfinite(out).all() and float(out.abs().max()) > 0
        assert ne == 0
    finally:
        L.ehm_gcn_destroy(h)


# ------------------------------------------------------------------------------------------------ the sampling loop
@pytest.fixture(scope="module")
def model_sens(dev, smpl_asset):
    from egohmr_amd.factory import build_synthetic_model
    return build_synthetic_model(dev, 0, diffuse_fuse=True, smpl_asset=smpl_asset, sensitive=dict(num_diffusion_timesteps=100))


def _run(model, d, batch, noise, fused, **kw):
    model.per_step_launches = not fused
    try:
        fs = model.fused_sampler
        fs.invalidate()
        r = fs.run(d, dict(batch), noise, trace=True, **kw)
        torch.cuda.synchronize()
    finally:
        model.per_step_launches = False
    o = r["other_outputs"]
    return {"sample": r["sample"].clone(), "x0": r["pred_xstart"].clone(), "joints": o["pred_keypoints_3d"].clone(), "verts": o["pred_vertices"].clone(),
            "trace": fs.last_trace.clone()}


def _same(a, b, what):
    for k in a:
        d = float((a[k] - b[k]).abs().max())
        print(f"[{what}] {k}: max|diff| {d:.3e}")
        assert torch.equal(a[k], b[k]), (what, k, d)


# B = 3 sits below the batch size of the deferred (matrix-core) skinning, where a loop that skins every step has no fused step launch at all: the
# B = 3 case therefore runs with lbs_every_step off (fused launches on every step but the last); B = 24 adds the deferred-skinning form.
@pytest.mark.parametrize("B,lbs", [(3, False), (24, True)])
@pytest.mark.parametrize("ddim", [True, False])
def test_three_tier_loop_fused_equals_per_step_launches(dev, model_sens, monkeypatch, ddim, B, lbs):
    """T = 6, two passes, one all-visible item, schedule [f16 x 1][two-term x 2][three-term x 3]: fused step launches == per-step launches on sample,
    x0, joints and the x_t trace; twoterm_steps = 0 == the same loop through a descriptor that never sets the field."""
    from egohmr_amd import fused as fused_mod
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device
    d = create_gaussian_diffusion(num_diffusion_timesteps=60, timestep_respacing="ddim6") if ddim else create_gaussian_diffusion(num_diffusion_timesteps=6, timestep_respacing="")
    T = d.num_timesteps
    assert T == 6
    b = syn.make_batch(B, 256, seed=31)
    b["orig_keypoints_2d"][0, :, 2] = 1.0                                           # item 0: every joint visible (no second pass for it)
    batch = batch_to_device(b, dev)
    noise = torch.from_numpy(syn.make_noise_stack(T, B, seed=31)).to(dev)
    m = model_sens
    old = (m.lbs_every_step, m.gcn_precision)
    m.lbs_every_step, m.gcn_precision = lbs, "f16x3"
    try:
        fs = m.fused_sampler
        out = _run(m, d, batch, noise, True, ddim=ddim, lowprec=1, twoterm=2)
        assert (fs.last_lowprec, fs.last_twoterm) == (1, 2)
        ref = _run(m, d, batch, noise, False, ddim=ddim, lowprec=1, twoterm=2)
        assert torch.isfinite(out["verts"]).all()
        _same(out, ref, f"fused vs per-step, B={B} ddim={ddim}")
        two = _run(m, d, batch, noise, True, ddim=ddim, lowprec=1, twoterm=0)
        dd = float((two["sample"] - out["sample"]).abs().max())
        print(f"[two-term steps are live] max|sample(j = 2) - sample(j = 0)| = {dd:.3e}")
        assert dd > 0.0
        real = fused_mod._lib.SampleDesc

        def desc_without_field(**kw):
            assert kw.pop("twoterm_steps") == 0
            return real(**kw)
        monkeypatch.setattr(fused_mod._lib, "SampleDesc", desc_without_field)
        old_desc = _run(m, d, batch, noise, True, ddim=ddim, lowprec=1)
        monkeypatch.setattr(fused_mod._lib, "SampleDesc", real)
        _same(two, old_desc, f"twoterm_steps = 0 vs no field, B={B} ddim={ddim}")
    finally:
        m.lbs_every_step, m.gcn_precision = old


def test_two_term_steps_past_the_end_of_the_loop_are_refused(dev, model_sens):
    """ehm_sample_loop rejects lowprec_steps + twoterm_steps > num_steps (as it rejects the field outside a split-f16 loop) instead of clamping it."""
    from egohmr_amd import _lib
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device
    d = create_gaussian_diffusion(num_diffusion_timesteps=6, timestep_respacing="")
    batch = batch_to_device(syn.make_batch(3, 256, seed=32), dev)
    noise = torch.from_numpy(syn.make_noise_stack(6, 3, seed=32)).to(dev)
    with pytest.raises(_lib.EgoHMRHipError):
        model_sens.fused_sampler.run(d, dict(batch), noise, ddim=False, lowprec=5, twoterm=2)


def test_calibration_finds_the_same_k_and_a_safe_j(dev, model_sens):
    """Sensitive weights, B = 4, a 10-step DDIM respacing: k is what it is without the middle tier; the calibrated three-tier loop stays within
    2 x schedule_tol of the all-three-term loop on a third noise draw (the condition of tests/test_gpu_schedule.py); an explicit
    f16x3_last_steps = None runs every step three-term, bit for bit."""
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device
    m, fs = model_sens, model_sens.fused_sampler
    d = create_gaussian_diffusion(num_diffusion_timesteps=100, timestep_respacing="ddim10")
    T, B = d.num_timesteps, 4
    batch = batch_to_device(syn.make_batch(B, num_scene_points=256, seed=41), dev)
    noise = torch.from_numpy(syn.make_noise_stack(T, B, seed=43)).to(dev)               # a third draw: not one of the calibration's two
    old = (m.f16x2_steps, m.f16x3_last_steps)
    try:
        m.f16x2_steps = 0
        info0 = fs.calibrate_schedule(d, batch, ddim=True, force=True)
        m.f16x2_steps = "auto"
        info = fs.calibrate_schedule(d, batch, ddim=True, force=True)
        print(f"[calibration] k = {info['k']} (without the tier: {info0['k']}), j = {info['two_term_steps']} of T = {T}; trials {info['trials']}; "
              f"two-term trials {info['two_term_trials']}")
        assert info0["two_term_steps"] == 0 and info0["two_term_trials"] == []
        assert info["k"] == info0["k"]
        assert 0 <= info["two_term_steps"] <= info["k"]
        fs.invalidate()
        ref = fs.run(d, dict(batch), noise, ddim=True, lowprec=0)["other_outputs"]
        ref_v, ref_j = ref["pred_vertices"].clone(), ref["pred_keypoints_3d"].clone()
        o = fs.run(d, dict(batch), noise, ddim=True)["other_outputs"]                    # 'auto' / 'auto': the calibrated three-tier loop
        assert (fs.last_lowprec, fs.last_twoterm) == (T - info["k"], info["two_term_steps"])
        err = max(float((o["pred_vertices"] - ref_v).norm(dim=-1).max()), float((o["pred_keypoints_3d"] - ref_j).norm(dim=-1).max()))
        print(f"[calibration] three-tier loop vs all-three-term loop on a third draw: {err:.3e} m (schedule_tol {m.schedule_tol:g})")
        assert err <= 2 * m.schedule_tol, (info, err)
        m.f16x3_last_steps = None                                                        # explicit: no f16 step and no two-term step
        o2 = fs.run(d, dict(batch), noise, ddim=True)["other_outputs"]
        assert (fs.last_lowprec, fs.last_twoterm) == (0, 0)
        assert torch.equal(o2["pred_vertices"], ref_v) and torch.equal(o2["pred_keypoints_3d"], ref_j)
        m.f16x3_last_steps, m.f16x2_steps = 3, 2                                         # both explicit: [f16 x 7][two-term x 2][three-term x 1]
        fs.run(d, dict(batch), noise, ddim=True)
        assert (fs.last_lowprec, fs.last_twoterm) == (T - 3, 2)
    finally:
        m.f16x2_steps, m.f16x3_last_steps = old
