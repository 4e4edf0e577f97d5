"""GPU (MI355X): BatchNorm2d of the ResNet-50 trunk on batch statistics (csrc/bn2d_train.hip through egohmr_amd/trunk_grad.py and
ResNet50Features.train_batchnorm, EgoHMR._set_train_modes) against the float64 restatement of tests/trunk_train_ref.py on the CPU.

The train-mode trunk amplifies a perturbation about 200 x in the forward and 400 x in the gradients, so a float32-grade run does not reproduce the float64
gradients of the whole trunk free running - torch's own float32 does not (0.13 .. 0.76 of a tensor's maximum on the worst tensor).  The gradients are
therefore checked kernel by kernel on shared operands and unit by unit on the DEVICE's own tensors (teacher forced: the float64 unit VJP gets the
device's saved input, raw conv output, gate and incoming cotangent); free running only the forward has a bar, 8 x the float32 CPU run's own error at
the same seed (X2 storage keeps 22 bits against float32's 24: 4 x, and 2 x slack); the free-running gradient errors are printed, not barred.

Bars: statistics within 4 float32 ulps of the float64 result (the only roundings are the float32 stores); running statistics within
2 * 2^-23 * max(|old|, |new term|) per call pair (each float32 store rounds by half an ulp of at most that magnitude: 2^-24 (0.9 |r1| + |r2|), doubled);
everything else the project's VJP bar, atol = 2e-4 max|ref|, rtol = 2e-3.  Every case prints what it measured."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_step_ref as TR  # noqa: E402
import val_losses_ref as VR  # noqa: E402
from egohmr_amd import synthetic as syn  # noqa: E402
from tests import trunk_grad_ref as R  # noqa: E402
from tests import trunk_train_ref as T  # noqa: E402
from tests.test_gpu_trunk_autograd import check, guarded, guards_intact, nchw, pack_x2, _f32, _rng  # noqa: E402

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
SHAPES = [(2, 64, 64), (3, 64, 32)]            # the smallest usable: 8 and 6 rows in layer 4 (two rows make the BatchNorm backward vanish identically)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def ulps(got, ref):
    """max over the elements of |got - ref| in units of the float32 spacing at |ref| (got: device float32, ref: float64 CPU)."""
    got = got.detach().double().cpu().numpy()
    ref = ref.numpy()
    sp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(got - ref) / sp))


def running_ok(tag, got, old, term, ref, calls=1, quiet=False):
    """got (device float32 buffer) against ref = the momentum rule in float64; old / term: the magnitudes that entered it."""
    bound = calls * 2 * EPS32 * torch.maximum(old.abs(), term.abs())
    err = (got.detach().double().cpu() - ref).abs()
    worst = float((err / bound).max())
    if not quiet:
        print(f"[{tag}] running statistic: worst error / bound = {worst:.2f}")
    return worst <= 1.0


# ---------------------------------------------------------------------------------------------- 1. the statistics kernel
@pytest.mark.parametrize("pixels,Cn,shift,x2", [(98, 64, 0.0, True), (8, 2048, 0.0, True), (2, 256, 0.0, True), (98, 64, 1e3, True), (98, 64, 0.0, False),
                                                (600, 64, 1e3, False)])
def test_stats_kernel(dev, pixels, Cn, shift, x2):
    from egohmr_amd import trunk_grad
    g = _rng(pixels * 7 + Cn + int(shift))
    sigma = g.uniform(0.5, 2.0, size=(1, Cn))
    x = torch.from_numpy((g.normal(size=(pixels, Cn)) * sigma + shift * sigma * np.sign(g.normal(size=(1, Cn)))).astype(np.float32))
    if x2:
        buf = pack_x2(x, dev)                                                  # the tile padding and the zero row hold NaN halves: garbage that must not count
        z64 = R.x2_decode(buf, pixels, Cn)
        assert buf.shape[0] > pixels
    else:
        full = torch.full((pixels + 64, Cn), float("nan"), device=dev)        # NaN rows behind the last one
        full[:pixels] = x.to(dev)
        buf, z64 = full[:pixels], x.double()
    bn = torch.nn.BatchNorm2d(Cn).to(dev)
    ref_bn = torch.nn.BatchNorm2d(Cn).double().train()
    with torch.no_grad():
        rm0, rv0 = _f32(g, Cn), _f32(g, Cn).abs() + 0.5
        bn.running_mean.copy_(rm0), bn.running_var.copy_(rv0), bn.num_batches_tracked.fill_(5)
        ref_bn.running_mean.copy_(rm0), ref_bn.running_var.copy_(rv0), ref_bn.num_batches_tracked.fill_(5)
    runs = [trunk_grad.bn_stats(buf, pixels, Cn, bn, x2=x2) for _ in range(2)]   # two consecutive calls: the same statistics, two running updates
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    mean, var, invstd = runs[0]
    rmean, rvar, rinv = T.row_stats(z64)
    u = [ulps(mean, rmean), ulps(var, rvar), ulps(invstd, rinv)]
    print(f"[stats pixels={pixels} C={Cn} shift={shift:g} x2={x2}] ulps: mean {u[0]:.2f}, var {u[1]:.2f}, invstd {u[2]:.2f}; max|mean|/sigma = {float((rmean.abs() * rinv).max()):.3g}")
    assert all(bool(torch.isfinite(t).all()) for t in runs[0]) and max(u) <= 4.0
    z4 = z64.t().reshape(1, Cn, pixels, 1)
    ref_bn(z4), ref_bn(z4)
    unb = rvar * pixels / (pixels - 1)
    assert running_ok("mean", bn.running_mean, rm0.double(), rmean, ref_bn.running_mean, calls=2)
    assert running_ok("var", bn.running_var, rv0.double(), unb, ref_bn.running_var, calls=2)
    assert int(bn.num_batches_tracked) == 7 == int(ref_bn.num_batches_tracked)
    # without a module: no running statistics, the same batch statistics
    free = trunk_grad.bn_stats(buf, pixels, Cn, None, x2=x2)
    assert all(torch.equal(a, b) for a, b in zip(free, runs[0]))


# ---------------------------------------------------------------------------------------------- 2. the backward kernels
@pytest.mark.parametrize("N,Ho,Wo,Cn,dil", [(2, 7, 7, 64, (14, 14)), (2, 2, 2, 256, (3, 3)), (2, 3, 3, 128, (5, 5)), (5, 14, 14, 64, None)])
def test_backward_kernels(dev, N, Ho, Wo, Cn, dil):
    from egohmr_amd import _lib, trunk_grad
    A = _lib.api()
    g = _rng(N * 1000 + Ho * 10 + Cn)
    pixels = N * Ho * Wo
    z = _f32(g, pixels, Cn) * torch.from_numpy(g.uniform(0.5, 2.0, size=(1, Cn)).astype(np.float32)) + _f32(g, 1, Cn)
    zbuf = pack_x2(z, dev)
    z64 = R.x2_decode(zbuf, pixels, Cn)
    G = _f32(g, pixels, Cn, scale=100.0)
    G[g.random((pixels, Cn)) < 0.4] = 0.0                                      # closed gates
    gamma = (_f32(g, Cn) * 0.3 + 1.0)
    gamma[1] = -0.5
    mean, var, invstd = trunk_grad.bn_stats(zbuf, pixels, Cn)
    Gd, gd = G.to(dev).view(N, Ho, Wo, Cn), gamma.to(dev)
    m64, i64, G64 = mean.double().cpu(), invstd.double().cpu(), G.double()
    xhat = (z64 - m64) * i64
    rb, rg = G64.sum(0), (G64 * xhat).sum(0)
    rz = (gamma.double() * i64) * (G64 - rb / pixels - xhat * rg / pixels)
    runs = []
    for _ in range(2):
        gb, gg = trunk_grad.bn_sums(Gd, zbuf, pixels, Cn, mean, invstd)
        full, out = guarded(dev, N, Ho, Wo, Cn)
        A.ehm_bn2d_train_bwd_zbar(Gd, zbuf, 1, zbuf.shape[0], mean, invstd, gd, gb, gg, None, out, N, Ho, Wo, Cn, Ho, Wo, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert guards_intact(full)
        runs.append((gb.clone(), gg.clone(), out.clone()))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))            # fixed order: bit-repeatable
    gb, gg, Z = runs[0]
    tag = f"bn2d bwd N={N} {Ho}x{Wo} C={Cn}"
    check(tag + " betabar", gb, rb)
    check(tag + " gammabar", gg, rg)
    check(tag + " zbar", Z.view(pixels, Cn), rz)
    assert torch.equal(trunk_grad.bn_zbar(Gd, zbuf, (N, Ho, Wo), Cn, mean, invstd, gd, gb, gg), Z)
    # float32 rows in place of the X2 buffer (the stem's form): the same values, so the same bits
    zf = z64.float().to(dev)
    gb2, gg2 = trunk_grad.bn_sums(Gd, zf, pixels, Cn, mean, invstd, x2=False)
    assert torch.equal(gb2, gb) and torch.equal(gg2, gg)
    assert torch.equal(trunk_grad.bn_zbar(Gd, zf, (N, Ho, Wo), Cn, mean, invstd, gd, gb, gg, x2=False), Z)
    if dil is not None:
        H, W = dil
        s = torch.tensor(0.25, device=dev)
        full, out = guarded(dev, N, H, W, Cn)
        A.ehm_bn2d_train_bwd_zbar(Gd, zbuf, 1, zbuf.shape[0], mean, invstd, gd, gb, gg, s, out, N, Ho, Wo, Cn, H, W, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert guards_intact(full)
        want = torch.zeros(N, H, W, Cn, device=dev)
        want[:, ::2, ::2][:, :Ho, :Wo] = Z * 0.25                               # a power of two: exact
        assert torch.equal(out, want)
        ref = torch.zeros(N, H, W, Cn, dtype=torch.float64)
        ref[:, ::2, ::2][:, :Ho, :Wo] = 0.25 * rz.view(N, Ho, Wo, Cn)
        check(tag + f" zbar dilated to {H}x{W}", out, ref)


# ---------------------------------------------------------------------------------------------- shared device runs
def decode_acts(rec, chans):
    return [nchw(R.x2_decode(buf, s[0] * s[1] * s[2], Cn), s, Cn) for (buf, s), Cn in zip(rec.acts, chans)]


def channels(m):
    out = [64]
    for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
        for blk in layer:
            out += [blk.conv1.out_channels, blk.conv2.out_channels, blk.conv3.out_channels]
    return out


_FORCED = {}


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def forced(dev, request):
    return device_run(dev, request.param)


@pytest.fixture(scope="module")
def forced0(dev):
    return device_run(dev, SHAPES[0])


def device_run(dev, shape):
    """One train-mode forward + backward on the device with everything kept and read back; computed once per shape, shared, left unchanged."""
    if shape not in _FORCED:
        _FORCED[shape] = _device_run(dev, shape)
    return _FORCED[shape]


def _device_run(dev, shape):
    from egohmr_amd import _lib, trunk_grad
    B, H, W = shape
    seed = 2
    sd = R.make_state(seed)
    m = T.load_module(sd, dev)
    img, gout = R.make_image(B, H, W, seed).float().to(dev), R.make_cotangent(B, seed).float().to(dev)
    U = trunk_grad.units(m)
    hook = []
    with _lib.on_device(dev):
        out, rec = trunk_grad.train_forward(m, img)
        trunk_grad._train_debug_hook = hook
        try:
            res = trunk_grad.trunk_backward_train(m, img, rec, gout, [None if u is None else (True, True, True) for u in U])
        finally:
            trunk_grad._train_debug_hook = None
        z_raw = trunk_grad.stem_preact(img, m.conv1.weight.detach().reshape(64, 147).t().contiguous(), torch.zeros(64, device=dev))
        z_route = trunk_grad.stem_preact(img, rec.stem_wt, rec.stem_b)
    torch.cuda.synchronize()
    return dict(sd=sd, m=m, img=img, gout=gout, out=out, rec=rec, res=res, hook={h[0]: h for h in hook}, U=U, z_raw=z_raw, z_route=z_route, shape=(B, H, W))


# ---------------------------------------------------------------------------------------------- 3. the fold invariant
def test_fold_invariant(dev, forced0):
    """The train-mode output has the bits of an eval-mode call on a copy whose running statistics are the stored batch (mean, biased var)."""
    from egohmr_amd import trunk_grad
    forced = forced0
    m, rec = forced["m"], forced["rec"]
    twin = copy.deepcopy(m)
    twin._fold_key_fn = twin._fold_key = twin._fold_fn = None
    twin.eval()
    with torch.no_grad():
        for u, e in zip(trunk_grad.units(twin), rec.bn):
            if u is not None:
                u[1].running_mean.copy_(e[2]), u[1].running_var.copy_(e[3])
    out = twin(forced["img"])
    torch.cuda.synchronize()
    assert torch.equal(out, forced["out"])
    assert not torch.equal(m.eval()(forced["img"]), forced["out"])             # ... and not those of the module's own running statistics
    m.train()


# ---------------------------------------------------------------------------------------------- 4. teacher-forced forward
def test_teacher_forced_forward(dev, forced):
    """Each of the 53 units' stored (mean, invstd) against float64 statistics of the device's own raw conv output; the running buffers against the
    momentum rule applied to the initial ones."""
    f = forced
    rec, U, sd = f["rec"], f["U"], f["sd"]
    names = R.unit_names()
    worst, fails, n = 0.0, [], 0
    for i, (u, e) in enumerate(zip(U, rec.bn)):
        assert (u is None) == (e is None)
        if u is None:
            continue
        n += 1
        z, zs, mean, var, invstd = e
        Co, pixels = u[0].out_channels, zs[0] * zs[1] * zs[2]
        z64 = f["z_raw"].double().cpu().view(pixels, 64) if i == 0 else R.x2_decode(z, pixels, Co)
        rmean, rvar, rinv = T.row_stats(z64)
        w = max(ulps(mean, rmean), ulps(var, rvar), ulps(invstd, rinv))
        worst = max(worst, w)
        bn = names[i][1]
        rm0, rv0 = sd[bn + ".running_mean"].float().double(), sd[bn + ".running_var"].float().double()
        rm, rv = T.running_update(rm0, rv0, rmean, rvar, pixels)
        ok = w <= 4.0 and running_ok(bn, u[1].running_mean, rm0, rmean, rm, quiet=True) and \
            running_ok(bn, u[1].running_var, rv0, rvar * pixels / (pixels - 1), rv, quiet=True)
        ok = ok and int(u[1].num_batches_tracked) == int(sd[bn + ".num_batches_tracked"]) + 1
        if not ok:
            fails.append(f"{bn} ({w:.2f} ulps)")
    print(f"[teacher-forced forward {f['shape']}] {n} units, worst statistic {worst:.2f} float32 ulps from float64")
    assert n == 53 and not fails, fails


# ---------------------------------------------------------------------------------------------- 5. teacher-forced backward
def test_teacher_forced_backward(dev, forced):
    """Every unit's zbar, wbar, gammabar, betabar and outgoing data gradient against the float64 unit VJP fed the device's x, z, gate and incoming
    cotangent.  This replaces a free-running gradient bar."""
    f = forced
    m, rec, U, res, hook = f["m"], f["rec"], f["U"], f["res"], f["hook"]
    acts = decode_acts(rec, channels(m))
    img64 = f["img"].double().cpu()
    fails = []
    cpu = lambda t: t.detach().double().cpu()
    nhwc = lambda t: cpu(t).permute(0, 3, 1, 2)

    def cot(i):
        """unit i's incoming cotangent as float64 NCHW with its power of two divided out"""
        g, cum = hook[i][1], float(hook[i][2])
        return cpu(g) / cum if g.dim() == 2 else nhwc(g) / cum

    def unit(i, x, gate_src, g, tag):
        conv, bn = U[i]
        z, zs = rec.bn[i][0], rec.bn[i][1]
        z64 = nchw(R.x2_decode(z, zs[0] * zs[1] * zs[2], conv.out_channels), zs, conv.out_channels)
        r = T.unit_vjp(cpu(conv.weight), cpu(bn.weight), x, z64, gate_src, g, conv.stride[0], conv.padding[0])
        check(f"{tag} zbar", nhwc(hook[i][3]) / float(hook[i][2]), r["zbar"], fails)
        check(f"{tag} wbar", res[i][0], r["wbar"], fails)
        check(f"{tag} gammabar", res[i][1], r["gammabar"], fails)
        check(f"{tag} betabar", res[i][2], r["betabar"], fails)
        return r

    names = R.unit_names()
    nb = (len(U) - 1) // 4
    for b in range(nb - 1, -1, -1):
        i1, i2, i3, id_ = 1 + 4 * b, 2 + 4 * b, 3 + 4 * b, 4 + 4 * b
        xin, a1, a2, y = acts[3 * b], acts[3 * b + 1], acts[3 * b + 2], acts[3 * b + 3]
        g = cot(i3)
        if g.dim() == 2:                                                       # the average pool's per-image cotangent
            g = (g / (y.shape[2] * y.shape[3])).view(*g.shape, 1, 1).expand_as(y)
        r3 = unit(i3, a2, y, g, names[i3][0])
        check(f"{names[i3][0]} xbar", cot(i2), r3["xbar"], fails)
        short = r3["G"]
        if U[id_] is not None:
            short = unit(id_, xin, y, g, names[id_][0])["xbar"]
        r2 = unit(i2, a1, a2, cot(i2), names[i2][0])
        check(f"{names[i2][0]} xbar", cot(i1), r2["xbar"], fails)
        r1 = unit(i1, xin, a1, cot(i1), names[i1][0])
        check(f"layer block {b} outgoing (conv1 xbar + shortcut)", cot(i3 - 4 if b > 0 else 0), r1["xbar"] + short, fails)
    # the stem: the device's own raw and folded pre-pool activations (the folded one routes the pooled cotangent)
    g0 = cot(0)
    gated = torch.where(acts[0] > 0, g0, torch.zeros_like(g0))
    conv, bn = U[0]
    r0 = T.stem_unit_vjp(cpu(conv.weight), cpu(bn.weight), img64, nhwc(f["z_raw"]), nhwc(f["z_route"]), gated)
    cum0 = float(hook[0][2])
    assert torch.equal(nhwc(hook[0][4]) != 0, r0["gz"] != 0)
    check("stem gz", nhwc(hook[0][4]) / cum0, r0["gz"], fails)
    check("stem zbar", nhwc(hook[0][3]) / cum0, r0["zbar"], fails)
    check("stem wbar", res[0][0], r0["wbar"], fails)
    check("stem gammabar", res[0][1], r0["gammabar"], fails)
    check("stem betabar", res[0][2], r0["betabar"], fails)
    assert len(hook) == 53 and not fails, fails


# ---------------------------------------------------------------------------------------------- 6. free running
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_free_running_forward(dev, seed):
    B, H, W = SHAPES[0]
    sd, img, gout = R.make_state(seed), R.make_image(B, H, W, seed), R.make_cotangent(B, seed)
    g64, out64 = T.autograd_grads(sd, img, gout, torch.float64)
    g32, out32 = T.autograd_grads(sd, img, gout, torch.float32)
    m = T.load_module(sd, dev)
    m.grad_params = True
    out = m(img.float().to(dev))
    out.backward(gout.float().to(dev))
    torch.cuda.synchronize()
    S = float(out64.abs().max())
    e32, edev = float((out32 - out64).abs().max()) / S, float((out.detach().double().cpu() - out64).abs().max()) / S
    rel = lambda a, n: float((a - g64[n]).abs().max() / g64[n].abs().max())
    d32 = sorted(rel(g32[n], n) for n in g64)
    ddev = sorted(rel(p.grad.double().cpu(), n) for n, p in m.named_parameters())
    print(f"[free running, seed {seed}] forward max|err|/max|ref|: device {edev:.2e}, float32 CPU {e32:.2e} (bar 8 x = {8 * e32:.2e}); gradients, recorded "
          f"not barred - worst / median tensor: device {ddev[-1]:.2e} / {ddev[len(ddev) // 2]:.2e}, float32 CPU {d32[-1]:.2e} / {d32[len(d32) // 2]:.2e}")
    assert edev <= 8 * e32


# ---------------------------------------------------------------------------------------------- 7. the route
def run_module(m, img, gout):
    m.zero_grad(set_to_none=True)
    out = m(img)
    out.backward(gout)
    torch.cuda.synchronize()
    return out, {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}


def test_route(dev, forced0):
    from egohmr_amd import _lib
    f = forced0
    sd, img, gout = f["sd"], f["img"], f["gout"]
    m = T.load_module(sd, dev, train_batchnorm=False)
    stats = lambda: {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    s0 = stats()
    frozen = m.eval()(img)
    # the switch off: .train() is ignored - the bits of today, the statistics untouched
    m.train()
    assert torch.equal(m(img), frozen) and all(torch.equal(v, s0[k]) for k, v in stats().items())
    # the switch on under no_grad: batch statistics, the running ones move, no graph
    m.train_batchnorm = True
    with torch.no_grad():
        ng = m(img)
    s1 = stats()
    assert ng.grad_fn is None and not ng.requires_grad
    assert not torch.equal(ng, frozen)                                         # (without the feature the train-mode output IS the running-statistics output)
    assert torch.equal(ng, f["out"])
    assert len(s1) == 3 * 53 and not [k for k, v in s1.items() if torch.equal(v, s0[k])]
    assert torch.equal(m(img), ng)                                             # grad mode on, grad_params off: still no graph, the same bits
    # with a graph: the same output bits; two calls give the same gradient bits; the product path's bits are the direct call's
    m.grad_params = True
    out, g1 = run_module(m, img, gout)
    assert out.grad_fn is not None and torch.equal(out.detach(), ng)
    _, g2 = run_module(m, img, gout)
    assert all(g1[n] is not None and torch.equal(g1[n], g2[n]) for n in g1) and len(g1) == 159
    direct = {}
    for u, r in zip(f["U"], f["res"]):
        if u is not None:
            for p, t in zip((u[0].weight, u[1].weight, u[1].bias), r):
                direct[id(p)] = t
    assert all(torch.equal(g1[n], direct[id(p)]) for n, p in f["m"].named_parameters())
    assert int(m.bn1.num_batches_tracked) == int(s0["bn1.num_batches_tracked"]) + 4
    # the next eval call folds the moved statistics
    assert not torch.equal(m.eval()(img), frozen)
    m.train()
    try:
        # a frozen unit: None for it, the others unchanged; only the top bias: nothing below runs
        blk = m.layer3[2]
        for p in (blk.conv2.weight, blk.bn2.weight, blk.bn2.bias):
            p.requires_grad_(False)
        _, g3 = run_module(m, img, gout)
        off = {"layer3.2.conv2.weight", "layer3.2.bn2.weight", "layer3.2.bn2.bias"}
        assert all((g3[n] is None) if n in off else torch.equal(g3[n], g1[n]) for n in g1)
        for p in m.parameters():
            p.requires_grad_(False)
        m.layer4[2].bn3.bias.requires_grad_(True)
        m.layer2[0].downsample[0].weight.requires_grad_(True)
        _, g4 = run_module(m, img, gout)
        assert sorted(n for n, v in g4.items() if v is not None) == ["layer2.0.downsample.0.weight", "layer4.2.bn3.bias"]
        assert all(torch.equal(g4[n], g1[n]) for n in ("layer2.0.downsample.0.weight", "layer4.2.bn3.bias"))
        for p in m.parameters():
            p.requires_grad_(False)
        assert m(img).grad_fn is None
        # a parameter changed between forward and backward is refused; the running statistics the forward itself moved are not
        for p in m.parameters():
            p.requires_grad_(True)
        out = m(img)
        keep = m.layer1[0].bn1.bias.detach().clone()
        with torch.no_grad():
            m.layer1[0].bn1.bias.add_(1.0)
        with pytest.raises(_lib.EgoHMRHipError, match="between the forward and the backward"):
            out.backward(gout)
        with torch.no_grad():
            m.layer1[0].bn1.bias.copy_(keep)
        _, g5 = run_module(m, img, gout)
        assert all(torch.equal(g5[n], g1[n]) for n in g1)
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            m(img[:1, :, :32, :32])
    finally:
        for p in m.parameters():
            p.requires_grad_(True)


# ---------------------------------------------------------------------------------------------- 8. the wiring behind EgoHMR
def test_training_step_on_batch_statistics(dev, golden_dir, synth_weights, smpl_asset):
    """Two training_steps from identical state with trunk_grad and backbone.train_batchnorm: the same gradient bits, the backbone in train mode, every
    running_mean moved, finite losses."""
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device, build_synthetic_model
    B = 2
    gd = np.load(os.path.join(golden_dir, "g21_val_losses_a.npz"))
    b_np, flags = VR.golden_batch(gd)
    cut = lambda d: {k: (cut(v) if isinstance(v, dict) else v[:B]) for k, v in d.items()}
    b_np = cut(b_np)
    b_np["img"] = _rng(3).normal(size=(B, 3, 64, 64)).astype(np.float32)
    batch = batch_to_device(b_np, dev)
    batch["smpl_params_is_axis_angle"] = {k: v[:B] for k, v in flags.items()}
    mean, std = syn.make_body_rep_stats(0)
    d = create_gaussian_diffusion(num_diffusion_timesteps=1000, timestep_respacing="", body_rep_mean=mean, body_rep_std=std)
    t = torch.tensor([0, 500]).to(dev)
    x_start = TR.x_start_of(b_np, mean, std).float()
    batch["x_t"] = d.q_sample(x_start, t.cpu(), noise=torch.from_numpy(_rng(5).normal(size=(B, 144)).astype(np.float32))).to(dev)
    m = build_synthetic_model(dev, 0, diffuse_fuse=True, state_dict=synth_weights, smpl_asset=smpl_asset, smpl_asset_male=syn.make_smpl_asset(1),
                              smpl_asset_female=syn.make_smpl_asset(2), start_coap_epoch=VR.START_COAP_EPOCH, **VR.CASE_WEIGHTS)
    m.frozen_trunk_training = True
    m.trunk_grad = True
    m.backbone.train_batchnorm = True
    initial = {n: v.detach().clone() for n, v in m.backbone.named_buffers() if n.endswith("running_mean")}

    def step():
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth_weights.items()}, strict=False)
        m.zero_grad(set_to_none=True)
        m.validation_setup()
        m.init_optimizers()
        torch.manual_seed(0)
        out = m.training_step(batch, t, 0)
        torch.cuda.synchronize()
        grads = {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}
        moved = [n for n, v in m.backbone.named_buffers() if n.endswith("running_mean") and not torch.equal(v, initial[n])]
        with torch.no_grad():
            loss = m.compute_loss(batch, out)
        return grads, m.backbone.training and all(mod.training for mod in m.backbone.modules()), moved, loss.detach().clone()

    try:
        (g1, mode1, moved1, loss1), (g2, mode2, moved2, loss2) = step(), step()
    finally:
        m.trunk_grad = False
        m.backbone.train_batchnorm = False
        m.validation_setup()
    assert mode1 and mode2 and not m.backbone.training
    assert len(initial) == 53 and len(moved1) == 53 and len(moved2) == 53
    assert bool(torch.isfinite(loss1).all()) and torch.equal(loss1, loss2)
    got = [n for n, v in g1.items() if v is not None]
    assert len([n for n in got if n.startswith("backbone.")]) == 159
    assert all(bool(torch.isfinite(g1[n]).all()) for n in got)
    differ = [n for n in g1 if (g1[n] is None) != (g2[n] is None) or (g1[n] is not None and not torch.equal(g1[n], g2[n]))]
    print(f"training_step on batch statistics: {len(got)} gradients, {len(differ)} differ between two steps from the same state; loss {float(loss1):.6g}")
    assert not differ, differ
