"""GPU (MI355X): the small per-item kernels at their own C entry points against the numpy restatements of tests/prep_pack_ref.py (which
tests/test_prep_pack_cpu.py pins to the reference's recorded outputs):

  ehm_item_prep      item_prep_kernel (visibility, TranslEnc, camera columns, zero fill, finite flag) + pass_map_kernel (chunks of 1024 items, pass groups)
  ehm_pack_outputs   the NaN rule, the R split, the projection, every NULL-able field, stride loops of more than one trip
  ehm_ddpm_step / ehm_ddim_step / ehm_guidance_grad_finish

Chains of correctly rounded float32 operations are compared bit for bit (NaN equals NaN); TranslEnc (FMA chains) and the DDPM step (expf) against
float64 within the bounds derived in prep_pack_ref.py.  Every output buffer carries a canary tail."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prep_pack_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = np.float32(-12345.678)      # what unwritten float32 memory must still hold
ISENT = -7                         # ... and unwritten int32 / uint8 memory
TAIL = 64                          # canary elements behind every output buffer
FX_NORM = 1500.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from egohmr_amd import _lib
    return _lib.api()


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _buf(dev, n, init=None, dtype=torch.float32, fill=None):
    """n elements (init, or the sentinel) + the canary tail, on the device."""
    fill = (float(SENT) if dtype == torch.float32 else ISENT & 0xFF if dtype == torch.uint8 else ISENT) if fill is None else fill
    b = torch.full((n + TAIL,), fill, dtype=dtype, device=dev)
    if init is not None:
        b[:n] = _t(np.asarray(init).reshape(-1), dev)
    return b


def _tail_intact(b, n):
    t = b[n:].cpu().numpy()
    want = np.full(TAIL, SENT if t.dtype == np.float32 else ISENT & 0xFF if t.dtype == np.uint8 else ISENT, t.dtype)
    return bool((t.view(np.uint8) == want.view(np.uint8)).all())


# ================================================================================================ ehm_item_prep
def _min_ld(col0, t_out, cam, bbox):
    return col0 + t_out + 1 + (2 if cam else 0) + (3 if bbox else 0)


def _prep_inputs(B, NK, seed):
    g = np.random.default_rng(seed)
    kp = np.zeros((B, NK, 3), np.float32)
    kp[:, :, :2] = g.uniform(0, 1920, size=(B, NK, 2))
    kp[:, :, 2] = g.choice(np.array([-1.0, 0.0, 1e-30, 0.7], np.float32), size=(B, NK))       # "> 0" decided at the edge
    if B > 1:
        kp[1, :, 2] = 0.7                                                                      # one item with every joint visible
    jm = g.permutation(NK)[:24].astype(np.int32)
    if 8 not in jm:
        jm[3] = 8                                                                              # the forced joint is among the mapped ones
    return dict(kp=kp, jm=jm, transl=g.uniform(-3, 3, size=(B, 3)).astype(np.float32), fx=g.uniform(0.5, 1.5, size=B).astype(np.float32),
                cx=g.uniform(900, 1000, size=B).astype(np.float32), cy=g.uniform(500, 600, size=B).astype(np.float32),
                bc=g.uniform(200, 1500, size=(B, 2)).astype(np.float32), bs=g.uniform(150, 600, size=B).astype(np.float32),
                img_sum=g.normal(size=B).astype(np.float32), scene_sum=g.normal(size=B).astype(np.float32))


def _transl_enc(t_hidden, t_out, transl, seed):
    g = np.random.default_rng(seed)
    w = [g.normal(scale=0.5, size=s).astype(np.float32) for s in ((t_hidden, 3), (t_hidden,), (t_out, t_hidden), (t_out,))]
    pre = float(w[0][-1].astype(np.float64) @ transl[0].astype(np.float64) + w[1][-1])
    if pre < 1.0:
        w[1][-1] += np.float32(1.0 - pre)          # the last hidden unit is active for item 0 (the test drops it from the reference)
    return w


def _item_prep(L, dev, i, w, cam, bbox, col0, ld, group=1, null_unused=True, img_sum=None, scene_sum=None):
    from egohmr_amd import _lib
    B, NK = i["kp"].shape[:2]
    t_hidden, t_out = w[0].shape[0], w[2].shape[0]
    P = _lib.ptr
    keep = {k: _t(i[k], dev) for k in ("kp", "jm", "transl", "fx", "cx", "cy", "bc", "bs")}
    keep.update(w=[_t(a, dev) for a in w], img=_t(img_sum, dev), scene=_t(scene_sum, dev))
    use_c, use_b = cam or not null_unused, bbox or not null_unused
    other = torch.full((B, ld), float(SENT), device=dev)
    vis, finite, need = _buf(dev, B * 24, dtype=torch.uint8), _buf(dev, B, dtype=torch.uint8), _buf(dev, B, dtype=torch.uint8)
    slot, items, count = (_buf(dev, n, dtype=torch.int32) for n in (B, B, 1))
    d = _lib.ItemPrepDesc(keypoints_2d=P(keep["kp"]), joint_map=P(keep["jm"]), NK=NK, force_visible=8, fx=P(keep["fx"]),
                          cx=P(keep["cx"]) if use_c else None, cy=P(keep["cy"]) if use_c else None, box_center=P(keep["bc"]) if use_b else None,
                          box_size=P(keep["bs"]) if use_b else None, transl=P(keep["transl"]), fx_norm=FX_NORM, with_bbox=int(bbox), with_cam_center=int(cam),
                          tW1=P(keep["w"][0]), tb1=P(keep["w"][1]), tW2=P(keep["w"][2]), tb2=P(keep["w"][3]), t_hidden=t_hidden, t_out=t_out,
                          img_rowsum=P(keep["img"]), scene_rowsum=P(keep["scene"]), other=P(other), other_ld=ld, other_col0=col0, vis=P(vis),
                          mask_slot=P(slot), mask_items=P(items), count=P(count), finite=P(finite), need_scratch=P(need), pass_group=group, B=B)
    L.ehm_item_prep(C.byref(d), _lib.stream_ptr())
    torch.cuda.synchronize()
    for b, n in ((vis, B * 24), (finite, B), (need, B), (slot, B), (items, B), (count, 1)):
        assert _tail_intact(b, n)
    return dict(other=other.cpu().numpy(), vis=vis[:B * 24].view(B, 24).cpu().numpy(), finite=finite[:B].cpu().numpy(), slot=slot[:B].cpu().numpy(),
                items=items[:B].cpu().numpy(), count=int(count[0]))


def _prep_ref(i, w, cam, bbox, col0, ld, **kw):
    return R.item_prep_ref(i["kp"], i["jm"], 8, i["transl"], i["fx"], FX_NORM, *w, other_ld=ld, other_col0=col0, cx=i["cx"], cy=i["cy"],
                           box_center=i["bc"], box_size=i["bs"], with_cam_center=cam, with_bbox=bbox, **kw)


@pytest.mark.parametrize("B", [1, 5, 130])
def test_item_prep_values(dev, L, B):
    worst = wrong = 0.0
    for NK in (25, 44):
        i = _prep_inputs(B, NK, 100 * B + NK)
        for t_hidden, t_out in ((64, 128), (128, 200), (7, 3)):
            w = _transl_enc(t_hidden, t_out, i["transl"], t_hidden)
            for cam, bbox, col0, pad in itertools.product((False, True), (False, True), (0, 37), (False, True)):
                ld = _min_ld(col0, t_out, cam, bbox)
                if pad:
                    ld = (ld + 31) // 32 * 32 + 32
                what = (B, NK, t_hidden, t_out, cam, bbox, col0, ld)
                got, ref = _item_prep(L, dev, i, w, cam, bbox, col0, ld), _prep_ref(i, w, cam, bbox, col0, ld)
                assert (got["vis"] == ref["vis"]).all(), what
                assert ((got["slot"] >= 0) == ref["need"]).all(), what
                assert (got["finite"] == 1).all() and (ref["finite"] == 1).all(), what
                o = got["other"]
                assert R.same_bits(o[:, :col0], np.full((B, col0), SENT)).all(), what                         # the caller's columns
                assert R.same_bits(o[:, col0 + t_out:], ref["cam"]).all(), what                              # camera columns + zero fill
                err = np.abs(o[:, col0:col0 + t_out].astype(np.float64) - ref["transl_enc"])
                assert (err <= ref["transl_bound"]).all(), (what, float((err / ref["transl_bound"]).max()))
                worst = max(worst, float((err / ref["transl_bound"]).max()))
                # the bound tells a wrong kernel: a reference without the last hidden unit is outside it
                short = _prep_ref(i, w, cam, bbox, col0, ld, hidden_units=t_hidden - 1)
                miss = float((np.abs(o[:, col0:col0 + t_out].astype(np.float64) - short["transl_enc"]) / ref["transl_bound"]).max())
                assert miss > 1.0, (what, miss)
                wrong = miss if wrong == 0.0 else min(wrong, miss)
    print(f"TranslEnc B={B}: worst error / bound = {worst:.4f}; a reference without its last hidden unit: >= {wrong:.3g} x bound")


def test_item_prep_finite_flag(dev, L):
    """The flag drops exactly for the item with a NaN / Inf COMPONENT (or row sum) that the call reads."""
    B, cam, bbox, t_out = 9, True, True, 3
    base = _prep_inputs(B, 25, 9)
    w = _transl_enc(7, t_out, base["transl"], 9)
    ld = _min_ld(0, t_out, cam, bbox)
    sums = dict(img_sum=base["img_sum"], scene_sum=base["scene_sum"])
    ones = np.ones(B, np.uint8)

    def run(i, cam=True, bbox=True, null_unused=True, **s):
        got = _item_prep(L, dev, i, w, cam, bbox, 0, _min_ld(0, t_out, cam, bbox), null_unused=null_unused, **s)
        ref = _prep_ref(i, w, cam, bbox, 0, _min_ld(0, t_out, cam, bbox), img_rowsum=s.get("img_sum"), scene_rowsum=s.get("scene_sum"))
        assert (got["finite"] == ref["finite"]).all(), (got["finite"], ref["finite"])
        return got["finite"]

    assert ld == 9 and (run(base, **sums) == ones).all()
    fields = [("transl", 0), ("transl", 1), ("transl", 2), ("fx", None), ("cx", None), ("cy", None), ("bc", 0), ("bc", 1), ("bs", None),
              ("img_sum", None), ("scene_sum", None)]
    for k, ((name, comp), val) in enumerate(itertools.product(fields, (np.nan, np.inf, -np.inf))):
        i = {n: a.copy() for n, a in base.items()}
        b = k % B
        i[name][(b,) if comp is None else (b, comp)] = val
        f = run(i, img_sum=i["img_sum"], scene_sum=i["scene_sum"])
        want = ones.copy()
        want[b] = 0
        assert (f == want).all(), (name, comp, val, f)
    # a switch that is off: poison behind the pointer it would read does not matter (pointers given, and NULL)
    i = {n: a.copy() for n, a in base.items()}
    i["cx"][2], i["cy"][3], i["bc"][4, 1], i["bs"][5] = np.nan, np.inf, -np.inf, np.nan
    assert (run(i, cam=False, bbox=False, null_unused=False, **sums) == ones).all()
    assert (run(i, cam=False, bbox=False, null_unused=True, **sums) == ones).all()
    want = ones.copy()
    want[[2, 3]] = 0
    assert (run(i, cam=True, bbox=False, null_unused=False, **sums) == want).all()
    # row sums: both NULL, and one NULL beside a poisoned other
    assert (run(base) == ones).all()
    bad = base["img_sum"].copy()
    bad[6] = np.nan
    want = ones.copy()
    want[6] = 0
    assert (run(base, scene_sum=bad) == want).all() and (run(base, img_sum=bad) == want).all()
    # finite components whose float32 SUM overflows are finite inputs
    i = {n: a.copy() for n, a in base.items()}
    i["transl"][1] = (3e38, 3e38, 0.0)
    i["bc"][7] = (3e38, 3e38)
    i["transl"][8] = (-3e38, -3e38, -3e38)
    assert (run(i, **sums) == ones).all()


def _need_patterns(B):
    g = np.random.default_rng(B)
    last, edge = np.zeros(B, bool), np.zeros(B, bool)
    last[-1] = True
    edge[[b for b in (1023, 1024) if b < B]] = True          # the last item of the first chunk of 1024 and the first of the second
    return {"none": np.zeros(B, bool), "all": np.ones(B, bool), "bernoulli": g.random(B) < 0.3, "last": last, "1023+1024": edge}


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1023, 1024, 1025, 2500])
def test_pass_map(dev, L, B):
    """need comes out of item_prep_kernel (driven through the confidences); the map must be exact for every chunk count and pass group."""
    i = _prep_inputs(B, 25, 7)
    i["jm"] = np.array(R.OPENPOSE_TO_SMPL, np.int32)
    w = _transl_enc(7, 3, i["transl"], 7)
    for (name, need), group in itertools.product(_need_patterns(B).items(), (1, 4, 32)):
        i["kp"][:, :, 2] = 0.7
        i["kp"][need, 12, 2] = 0.0                           # OpenPose joint 12 feeds SMPL joint 1
        got = _item_prep(L, dev, i, w, False, False, 0, 4, group=group)
        assert ((got["vis"] == 1).all(axis=1) == ~need).all(), (name, group)
        slot, items, count = R.pass_map_ref(need, group)
        assert got["count"] == count, (name, group, got["count"], count)
        assert (got["slot"] == slot).all(), (name, group)
        assert (got["items"][:count] == items).all(), (name, group)
        assert (got["items"][count:] == ISENT).all(), (name, group)
        has = got["slot"] >= 0                               # what ehm_gcn_set_pass_map requires of the two arrays
        assert (got["items"][got["slot"][has]] == np.flatnonzero(has)).all(), (name, group)


# ================================================================================================ ehm_pack_outputs
PACK_VARIANTS = [
    dict(),                                                                                             # every NULL-able field NULL
    dict(finite=True, x_final=True, finite_out=True),                                                   # two bad items by the flag; no last draw
    dict(chk=(1, 0, "mid", 0, np.nan), x_final=True, last_noise=True, finite_out=True),                 # (rows, row, item, element, value)
    dict(finite=True, chk=(3, 2, "last", 143, -np.inf), x_final=True, last_noise=True),
    dict(chk=(3, 1, "first", 143, np.nan), finite_out=True),
    dict(chk=(3, 0, "last", 0, -np.inf), x_final=True, finite_out=True),
    dict(chk=(3, None, None, 0, 0.0), finite=True, x_final=True, last_noise=True, finite_out=True),      # a clean chk: only the flagged items are bad
]
PACK_OUT = {"betas_out": 10, "global_orient": 9, "body_pose": 207, "focal": 2, "center": 2}              # per-item sizes; + kp3d_full 3 J, kp2d_full 2 J


def _pack_case(B, J, V, var, seed):
    g = np.random.default_rng(seed)
    n = lambda *s: g.normal(size=s).astype(np.float32)
    a = dict(x0=n(B, 144), pose6d=n(B, 144), R=n(B, 24, 9), verts=n(B, V, 3), joints=n(B, J, 3), betas_in=n(B, 10),
             transl=(np.array([0.0, 0.0, 3.0]) + g.uniform(-0.5, 0.5, size=(B, 3))).astype(np.float32), fx=g.uniform(0.5, 1.5, size=B).astype(np.float32),
             cx=g.uniform(900, 1000, size=B).astype(np.float32), cy=g.uniform(500, 600, size=B).astype(np.float32),
             finite=None, chk=None, last_noise=None, x_final=None)
    bad = np.zeros(B, bool)
    if var.get("finite"):
        bad[[0, B - 1]] = True                               # two bad items (one where B = 1)
        a["finite"] = (~bad).astype(np.uint8)
    if var.get("chk"):
        rows, row, item, el, val = var["chk"]
        a["chk"] = n(rows, B, 144)
        if row is not None:
            b = {"first": 0, "mid": B // 2, "last": B - 1}[item]
            a["chk"][row, b, el] = val
            bad[b] = True
    good = np.flatnonzero(~bad)
    if var.get("x_final"):
        a["x_final"] = n(B, 144)
    if var.get("last_noise"):
        a["last_noise"] = n(B, 144)
        if good.size:
            a["last_noise"][good[-1], 77] = np.nan           # the last step's draw poisons its own element only
    if good.size:                                            # a joint exactly in the camera plane, and one behind the camera
        b = good[0]
        a["joints"][b, 0, 2] = -a["transl"][b, 2]
        a["joints"][b, J - 1, 2] = -a["transl"][b, 2] - np.float32(1.0)
    return a, bad


def _run_pack(L, dev, a, var):
    from egohmr_amd import _lib
    B, J, V = a["x0"].shape[0], a["joints"].shape[1], a["verts"].shape[1]
    P = _lib.ptr
    sizes = dict(PACK_OUT, kp3d_full=3 * J, kp2d_full=2 * J)
    inplace = {k: _buf(dev, a[k].size, a[k]) for k in ("x0", "pose6d", "R", "verts", "joints")}
    if a["x_final"] is not None:
        inplace["x_final"] = _buf(dev, B * 144, a["x_final"])
    outs = {k: _buf(dev, B * n) for k, n in sizes.items()}
    fo = _buf(dev, B, dtype=torch.uint8) if var.get("finite_out") else None
    ro = {k: _t(a[k], dev) for k in ("finite", "chk", "last_noise", "betas_in", "transl", "fx", "cx", "cy")}
    d = _lib.PackDesc(B=B, J=J, V=V, finite=P(ro["finite"]), chk=P(ro["chk"]), chk_rows=0 if a["chk"] is None else a["chk"].shape[0],
                      last_noise=P(ro["last_noise"]), x_final=P(inplace.get("x_final")), x0=P(inplace["x0"]), pose6d=P(inplace["pose6d"]), R=P(inplace["R"]),
                      verts=P(inplace["verts"]), joints=P(inplace["joints"]), betas_in=P(ro["betas_in"]), betas_out=P(outs["betas_out"]), transl=P(ro["transl"]),
                      fx=P(ro["fx"]), cx=P(ro["cx"]), cy=P(ro["cy"]), fx_norm=FX_NORM, global_orient=P(outs["global_orient"]), body_pose=P(outs["body_pose"]),
                      kp3d_full=P(outs["kp3d_full"]), kp2d_full=P(outs["kp2d_full"]), focal=P(outs["focal"]), center=P(outs["center"]), finite_out=P(fo))
    L.ehm_pack_outputs(C.byref(d), _lib.stream_ptr())
    torch.cuda.synchronize()
    got = {}
    for k, b in {**inplace, **outs}.items():
        n = b.numel() - TAIL
        assert _tail_intact(b, n), k
        got[k] = b[:n].cpu().numpy()
    if fo is not None:
        assert _tail_intact(fo, B)
        got["finite_out"] = fo[:B].cpu().numpy()
    return got


@pytest.mark.parametrize("J,V", [(24, 1), (45, 431), (300, 100)])
@pytest.mark.parametrize("B", [1, 3, 257])
def test_pack_outputs(dev, L, B, J, V):
    for k, var in enumerate(PACK_VARIANTS):
        a, bad = _pack_case(B, J, V, var, 1000 * B + J + k)
        got = _run_pack(L, dev, a, var)
        ref = R.pack_ref(a["x0"], a["pose6d"], a["R"], a["verts"], a["joints"], a["betas_in"], a["transl"], a["fx"], a["cx"], a["cy"], FX_NORM,
                         finite=a["finite"], chk=a["chk"], last_noise=a["last_noise"], x_final=a["x_final"])
        assert (ref["finite_out"] == ~bad).all()
        for name, r in ref.items():
            if name not in got:
                assert name == "finite_out" and not var.get("finite_out")
                continue
            g = got[name].reshape(r.shape)
            if name == "finite_out":
                assert (g == r).all(), (k, name)
                continue
            same = R.same_bits(g, r)
            assert same.all(), (k, name, np.argwhere(~same)[:4].tolist())
            # the rule itself, not through the restatement: a bad item is NaN throughout except focal / center, a good item's buffers are its inputs
            if name in ("focal", "center"):
                assert np.isfinite(g).all(), (k, name)
            else:
                assert np.isnan(g[bad]).all(), (k, name)
            if name in a and a[name] is not None and name != "x_final":
                assert R.same_bits(g[~bad], a[name].reshape(r.shape)[~bad]).all(), (k, name)
        if "x_final" in got:
            xf, keep = got["x_final"].reshape(B, 144), np.ones((B, 144), bool)
            keep[bad] = False
            if a["last_noise"] is not None:
                keep &= np.isfinite(a["last_noise"])
            assert np.isnan(xf[~keep]).all() and R.same_bits(xf[keep], a["x_final"][keep]).all(), k
            assert (~keep).sum() == 144 * bad.sum() + (1 if a["last_noise"] is not None and not bad.all() else 0), k
        good = np.flatnonzero(~bad)
        if good.size:                                        # p.z == 0 and p.z < 0 give numpy's Inf / NaN pattern (compared above); they were really there
            p = got["kp3d_full"].reshape(B, J, 3)[good[0]]
            assert p[0, 2] == 0.0 and p[J - 1, 2] < -0.99 and not np.isfinite(got["kp2d_full"].reshape(B, J, 2)[good[0], 0]).any(), k


# ================================================================================================ sampler steps
STEP_SIZES = [0, 1, 255, 256, 257, 144 * 257]


@pytest.fixture(scope="module")
def coefs():
    from egohmr_amd.diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion(num_diffusion_timesteps=100, timestep_respacing="")
    T = d.num_timesteps
    assert T == 100
    return {(i, ddim): d.step_coefs(i, ddim, eta=0.5 if ddim else 0.0) for i in (T - 1, T // 2, 0) for ddim in (False, True)}    # first, middle, last


def _step_data(n, seed):
    g = np.random.default_rng(seed)
    return [g.normal(size=n).astype(np.float32) for _ in range(4)]          # x, x0, noise, grad


def _ddpm(L, dev, x, x0, noise, grad, c, gscale, alias):
    from egohmr_amd import _lib
    n = x.size
    xb, out = _buf(dev, n, x), _buf(dev, n)
    dst = xb if alias else out
    L.ehm_ddpm_step(xb, _buf(dev, n, x0), _buf(dev, n, noise), None if grad is None else _buf(dev, n, grad), dst, c.coef1, c.coef2, c.log_variance,
                    c.nonzero, gscale, n, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _tail_intact(xb, n) and _tail_intact(out, n)
    if not alias:
        assert R.same_bits(xb[:n].cpu().numpy(), x).all()
    return dst[:n].cpu().numpy()


def _ddim(L, dev, x, x0, noise, c, alias):
    from egohmr_amd import _lib
    n = x.size
    xb, out = _buf(dev, n, x), _buf(dev, n)
    dst = xb if alias else out
    L.ehm_ddim_step(xb, _buf(dev, n, x0), _buf(dev, n, noise), dst, c.sqrt_recip_ac, c.sqrt_recipm1_ac, c.sqrt_ac_prev, c.dir_coef, c.sigma, c.nonzero, n,
                    _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _tail_intact(xb, n) and _tail_intact(out, n)
    return dst[:n].cpu().numpy()


def _within(got, ref, bound):
    nan = np.isnan(ref)
    assert (np.isnan(got) == nan).all()
    err = np.abs(got.astype(np.float64) - ref)[~nan]
    assert (err <= bound[~nan]).all(), float((err / bound[~nan]).max())
    return float((err / bound[~nan]).max()) if err.size else 0.0


def test_ddpm_step(dev, L, coefs):
    worst = 0.0
    for n, (i, alias, with_grad) in itertools.product(STEP_SIZES, itertools.product((99, 50, 0), (False, True), (False, True))):
        c = coefs[(i, False)]
        assert c.nonzero == (0.0 if i == 0 else 1.0)
        x, x0, noise, grad = _step_data(n, n + i)
        # gaussian_diffusion.py:381 / :385: the guidance weight times the variance, or times 0.01 on the last steps
        gscale = (float(np.float32(0.3) * np.float32(c.variance)) if i >= 5 else float(np.float32(0.3 * 0.01))) if with_grad else 0.0
        got = _ddpm(L, dev, x, x0, noise, grad if with_grad else None, c, gscale, alias)
        ref, bound = R.ddpm_step_ref(x, x0, noise, grad if with_grad else None, c.coef1, c.coef2, c.log_variance, c.nonzero, gscale)
        worst = max(worst, _within(got, ref, bound))
        if n == 257 and with_grad and not alias:             # the bound tells a wrong step: a step without its gradient term is outside it
            short, _ = R.ddpm_step_ref(x, x0, noise, None, c.coef1, c.coef2, c.log_variance, c.nonzero, 0.0)
            assert (np.abs(got - short) > bound).any()
    print(f"DDPM step: worst error / bound = {worst:.4f}")
    # the last step multiplies its draw by nonzero = 0: a NaN draw reaches its own element only
    c = coefs[(0, False)]
    x, x0, noise, _ = _step_data(257, 5)
    noise[200] = np.nan
    got = _ddpm(L, dev, x, x0, noise, None, c, 0.0, False)
    assert np.isnan(got[200]) and np.isfinite(np.delete(got, 200)).all()
    _within(got, *R.ddpm_step_ref(x, x0, noise, None, c.coef1, c.coef2, c.log_variance, c.nonzero, 0.0))


def test_ddim_step(dev, L, coefs):
    for n, i, alias in itertools.product(STEP_SIZES, (99, 50, 0), (False, True)):
        c = coefs[(i, True)]
        assert c.nonzero == (0.0 if i == 0 else 1.0) and (c.sigma > 0 or i == 0)
        x, x0, noise, _ = _step_data(n, n + i + 1)
        got = _ddim(L, dev, x, x0, noise, c, alias)
        ref = R.ddim_step_ref(x, x0, noise, c.sqrt_recip_ac, c.sqrt_recipm1_ac, c.sqrt_ac_prev, c.dir_coef, c.sigma, c.nonzero)
        assert R.same_bits(got, ref).all(), (n, i, alias)
    c = coefs[(0, True)]
    x, x0, noise, _ = _step_data(257, 6)
    noise[256] = np.nan
    got = _ddim(L, dev, x, x0, noise, c, False)
    assert np.isnan(got[256]) and np.isfinite(got[:256]).all()
    assert R.same_bits(got, R.ddim_step_ref(x, x0, noise, c.sqrt_recip_ac, c.sqrt_recipm1_ac, c.sqrt_ac_prev, c.dir_coef, c.sigma, c.nonzero)).all()


def test_steps_refuse_bad_arguments(dev, coefs):
    from egohmr_amd import _lib
    raw, st = _lib.lib(), _lib.stream_ptr()
    b = [_buf(dev, 16) for _ in range(4)]
    p = [t.data_ptr() for t in b]
    c, k = coefs[(50, False)], coefs[(50, True)]
    dd = (c.coef1, c.coef2, c.log_variance, c.nonzero, 0.0)
    di = (k.sqrt_recip_ac, k.sqrt_recipm1_ac, k.sqrt_ac_prev, k.dir_coef, k.sigma, k.nonzero)
    assert raw.ehm_ddpm_step(None, p[1], p[2], None, p[3], *dd, 16, st) != 0
    assert raw.ehm_ddpm_step(p[0], p[1], p[2], None, p[3], *dd, -1, st) != 0
    assert raw.ehm_ddim_step(None, p[1], p[2], p[3], *di, 16, st) != 0
    assert raw.ehm_ddim_step(p[0], p[1], p[2], p[3], *di, -1, st) != 0
    torch.cuda.synchronize()
    for t in b:                                              # a refused call wrote nothing
        assert (t.cpu().numpy().view(np.uint32) == np.full(16 + TAIL, SENT).view(np.uint32)).all()


# ================================================================================================ ehm_guidance_grad_finish
@pytest.mark.parametrize("B", [1, 257])
def test_guidance_grad_finish(dev, L, B):
    from egohmr_amd import _lib
    g = np.random.default_rng(B).normal(size=(B, 144)).astype(np.float32)
    g[B - 1, 0 * 6 + 3] = np.nan                             # joints 0 and 23 are zeroed: their NaN does not reach the output
    g[0, 23 * 6 + 5] = np.nan
    g[B // 2, 4 * 6 + 1] = np.inf                            # a kept joint's does
    for denom in (1.0, float(B)):
        out, loss = _buf(dev, B * 144), _buf(dev, B, np.ones(B, np.float32))
        L.ehm_guidance_grad_finish(_buf(dev, B * 144, g), loss if denom == 1.0 else None, out, B, denom, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert _tail_intact(out, B * 144)
        got, ref = out[:B * 144].cpu().numpy().reshape(B, 144), R.grad_finish_ref(g, denom)
        assert R.same_bits(got, ref).all(), denom
        assert got[B - 1, 3] == 0.0 and got[0, 143] == 0.0 and got[B // 2, 25] == -np.inf
    out = _buf(dev, B * 144)
    assert _lib.lib().ehm_guidance_grad_finish(_buf(dev, B * 144, g).data_ptr(), None, out.data_ptr(), B, 0.0, _lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert R.same_bits(out.cpu().numpy(), np.full(B * 144 + TAIL, SENT)).all()
