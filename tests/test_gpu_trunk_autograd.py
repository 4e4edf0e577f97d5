"""GPU (MI355X): the backward of the ResNet-50 trunk in eval mode (csrc/conv_bwd.hip through egohmr_amd/trunk_grad.py, the data gradients on
ehm_conv_nhwc_split), the autograd route of ResNet50Features.__call__ behind `grad_params`, and EgoHMR.trunk_grad, against the float64 restatement of
tests/trunk_grad_ref.py on the CPU.

Per kernel both sides share their operands (inputs are packed to X2 as the forward stores them and read back).  The whole trunk is checked twice: with
the device's own gates and pool arg-max handed to the float64 VJP chain (no case left out), and free running at the seed committed in
tests/test_trunk_autograd_cpu.py (E2E_SEED: a float32 run of the reference stays within a quarter of the bar there).

Bar: the project's VJP bar (tests/test_gpu_gcn_autograd.py, tests/test_gpu_pointnet_autograd.py): atol = 2e-4 max|ref|, rtol = 2e-3; the free-running
test per tensor in the max norm, max|g - ref| <= 2e-4 max|ref| (the form of tests/test_gpu_train_step.py).  Every case prints what it measured."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_step_ref as TR  # noqa: E402
import val_losses_ref as VR  # noqa: E402
from egohmr_amd import synthetic as syn  # noqa: E402
from tests import stem_ref as SR  # noqa: E402
from tests import trunk_grad_ref as R  # noqa: E402
from tests.test_trunk_autograd_cpu import ATOL, E2E_F32_ERROR, E2E_SEED, E2E_SHAPE, RTOL  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 12345.0
GUARD = 64                                 # floats in front of and behind every output (16-byte alignment kept)
NAN = float("nan")
STEM_WGRAD_BLOCKS = 256                    # the fixed grid of stem_bwd_wgrad_kernel (csrc/conv_bwd.hip: SB_BLOCKS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _rng(seed):
    return np.random.default_rng(seed)


def _f32(g, *shape, scale=1.0):
    return torch.from_numpy((g.normal(size=shape) * scale).astype(np.float32))


def guarded(dev, *shape):
    n = int(np.prod(shape))
    full = torch.full((n + 2 * GUARD,), CANARY, device=dev)
    return full, full[GUARD:GUARD + n].view(*shape)


def guards_intact(full):
    return bool((full[:GUARD] == CANARY).all()) and bool((full[-GUARD:] == CANARY).all())


def pack_x2(x, dev):
    """float32 [pixels, C] -> the X2 buffer of ehm_conv_x2_rows(pixels) rows as the forward stores it; the padding rows AND the zero row hold NaN halves."""
    from egohmr_amd import _lib
    A = _lib.api()
    pixels, Cn = x.shape
    rows = int(A.ehm_conv_x2_rows(pixels))
    buf = torch.empty(rows, Cn, device=dev)
    buf.view(torch.float16).fill_(NAN)
    A.ehm_split_pack(x.to(dev).contiguous(), buf, pixels, Cn, Cn, 1.0, _lib.stream_ptr())
    return buf


def check(tag, got, ref, fails=None):
    """got (device float32) against ref (float64 CPU) at the VJP bar; prints max|err| / max|ref|."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    S = float(ref.abs().max())
    err = (got - ref).abs()
    rel = float(err.max()) / S if S > 0 else float(err.max())
    ok = bool((err <= ATOL * S + RTOL * ref.abs()).all())
    print(f"[{tag}] max|err|/max|ref| = {rel:.2e} (max|ref| {S:.3g})")
    if fails is None:
        assert ok, f"{tag}: over the VJP bar ({rel:.2e})"
    elif not ok:
        fails.append(f"{tag} ({rel:.2e})")
    return rel


def nchw(t, shape, Cn):
    N, H, W = shape
    return t.view(N, H, W, Cn).permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------- 1. the gate kernel
GATE_CASES = [(1, 1, 1, 64, None), (2, 7, 7, 64, None), (3, 5, 3, 128, None), (2, 8, 8, 64, (16, 16)), (1, 4, 4, 64, (7, 7))]


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("N,Ho,Wo,Cn,dil", GATE_CASES)
def test_gate_kernel(dev, N, Ho, Wo, Cn, dil, per_image):
    from egohmr_amd import _lib
    A = _lib.api()
    g = _rng(N * 1000 + Ho * 10 + Cn + per_image)
    pixels = N * Ho * Wo
    y = _f32(g, pixels, Cn)
    y[g.random((pixels, Cn)) < 0.2] = 0.0                                  # exact zeros: closed
    y[:Ho * Wo, 0] = -y[:Ho * Wo, 0].abs()                                 # channel 0 of image 0: closed at every pixel (zeros and negatives)
    y[0, 1] = 0.0
    cot = _f32(g, N, Cn) if per_image else _f32(g, pixels, Cn)
    cot.view(-1)[0] = NAN                                                  # a NaN cotangent behind a closed gate (image 0, channel 0; per pixel: pixel 0)
    ybuf = pack_x2(y, dev)
    y64 = R.x2_decode(ybuf, pixels, Cn).view(N, Ho, Wo, Cn)
    assert torch.equal(y64.view(pixels, Cn) > 0, y > 0)                     # (hi + lo keeps 22 bits: the value may differ, the sign does not)
    scale = torch.tensor(0.25, device=dev)
    H, W = (Ho, Wo) if dil is None else dil
    full, out = guarded(dev, N, H, W, Cn)
    A.ehm_conv_bwd_gate(cot.to(dev), int(per_image), ybuf, scale, out, N, Ho, Wo, Cn, H, W, _lib.stream_ptr())
    torch.cuda.synchronize()
    c64 = cot.double().view(N, 1, 1, Cn) / (Ho * Wo) if per_image else cot.double().view(N, Ho, Wo, Cn)
    dense = torch.where(y64 > 0, (0.25 * c64).expand(N, Ho, Wo, Cn), torch.zeros(N, Ho, Wo, Cn, dtype=torch.float64))
    ref = dense
    if dil is not None:
        ref = torch.zeros(N, H, W, Cn, dtype=torch.float64)
        ref[:, ::2, ::2][:, :Ho, :Wo] = dense
    assert guards_intact(full) and bool(torch.isfinite(out).all())
    check(f"gate N={N} {Ho}x{Wo} C={Cn} dil={dil} per_image={per_image}", out, ref)
    if not per_image:
        assert torch.equal(out.cpu().double(), ref)                       # a power of two times a float32: exact
    assert torch.equal((out.cpu() != 0), (ref != 0))                      # the zeros of the dilated form and of the closed gates are exact zeros
    # scale = NULL is 1
    full2, out2 = guarded(dev, N, H, W, Cn)
    A.ehm_conv_bwd_gate(cot.to(dev), int(per_image), ybuf, None, out2, N, Ho, Wo, Cn, H, W, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert guards_intact(full2) and torch.equal(out2 * 0.25, out)


# ---------------------------------------------------------------------------------------------- 2. the weight gradient, 3. the data gradient
# (5, 14, 14, ...): 980 pixels = 16 split-K runs of 64 (the plan's shortest run) with a ragged last one of 20
CONV_CASES = [(1, 1, 1, 64, 64, 1, 1, 0), (1, 1, 1, 64, 64, 3, 1, 1), (2, 7, 7, 64, 128, 3, 1, 1), (3, 5, 3, 64, 64, 3, 1, 1), (2, 8, 8, 64, 64, 3, 2, 1),
              (1, 7, 7, 64, 64, 3, 2, 1), (2, 8, 8, 128, 256, 1, 2, 0), (5, 14, 14, 64, 64, 1, 1, 0)]


@pytest.mark.parametrize("N,H,W,Ci,Co,K,stride,pad", CONV_CASES)
def test_wgrad_kernel(dev, N, H, W, Ci, Co, K, stride, pad):
    from egohmr_amd import _lib
    A = _lib.api()
    g = _rng(N * 1000 + H * 10 + K + Co)
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    x = _f32(g, N * H * W, Ci)
    xbuf = pack_x2(x, dev)
    x64 = nchw(R.x2_decode(xbuf, N * H * W, Ci), (N, H, W), Ci)
    G = _f32(g, N, Ho, Wo, Co, scale=100.0)
    nb = C.c_int64(0)
    A.ehm_conv_bwd_wgrad_workspace_bytes(N, H, W, Ci, Co, K, stride, pad, C.byref(nb))
    ws = torch.full((nb.value // 4,), NAN, device=dev)
    runs = []
    for _ in range(2):
        fw, gw = guarded(dev, Co, K * K * Ci)
        fb, gb = guarded(dev, Co)
        A.ehm_conv_bwd_wgrad(G.to(dev), xbuf, xbuf.shape[0], gw, gb, N, H, W, Ci, Co, K, stride, pad, ws, nb.value, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert guards_intact(fw) and guards_intact(fb)
        runs.append((gw.clone(), gb.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])                 # fixed order: bit-repeatable
    G64 = G.double().permute(0, 3, 1, 2)
    _, rw, rb, _ = R.conv_vjp(torch.zeros(Co, Ci, K, K, dtype=torch.float64), x64, torch.ones_like(G64), G64, stride, pad, need_x=False)
    tag = f"wgrad N={N} {H}x{W} {Ci}->{Co} K={K} s={stride}"
    check(tag + " w", runs[0][0].view(Co, K, K, Ci).permute(0, 3, 1, 2), rw)
    check(tag + " b", runs[0][1], rb)
    # either output alone: the same bits
    fw, gw = guarded(dev, Co, K * K * Ci)
    A.ehm_conv_bwd_wgrad(G.to(dev), xbuf, xbuf.shape[0], gw, None, N, H, W, Ci, Co, K, stride, pad, ws, nb.value, _lib.stream_ptr())
    fb, gb = guarded(dev, Co)
    A.ehm_conv_bwd_wgrad(G.to(dev), None, 0, None, gb, N, H, W, Ci, Co, K, stride, pad, ws, nb.value, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert guards_intact(fw) and guards_intact(fb) and torch.equal(gw, runs[0][0]) and torch.equal(gb, runs[0][1])


@pytest.mark.parametrize("N,H,W,Ci,Co,K,stride,pad", CONV_CASES)
def test_data_gradient_through_the_conv_engine(dev, N, H, W, Ci, Co, K, stride, pad):
    from egohmr_amd import trunk_grad
    from egohmr_amd.split_gemm import pow2_scale
    g = _rng(N * 1000 + H * 10 + K + Co + 7)
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    wf = _f32(g, Co, Ci, K, K, scale=float(np.sqrt(2.0 / (Ci * K * K))))
    cot = _f32(g, N, Ho, Wo, Co, scale=1e-3)                                                            # small gradients: the power of two matters
    y = torch.ones(N * Ho * Wo, Co)
    y[g.random((N * Ho * Wo, Co)) < 0.3] = -1.0
    ybuf = pack_x2(y, dev)
    s = pow2_scale(cot.to(dev))
    assert 512.0 <= float(s) * float(cot.abs().max()) <= 1024.0
    Gd = trunk_grad.gate(cot.to(dev), ybuf, (N, Ho, Wo), Co, s, out_hw=(H, W) if stride == 2 else None)
    res = _f32(g, N, H, W, Ci)
    got = trunk_grad.dgrad(Gd, trunk_grad.dgrad_weight(wf.to(dev)), Co, Ci, K, pad, res=res.to(dev))
    torch.cuda.synchronize()
    y64 = nchw(y.double(), (N, Ho, Wo), Co)
    x_shape = torch.zeros(N, Ci, H, W, dtype=torch.float64)
    _, _, _, gx = R.conv_vjp(wf.double(), x_shape, y64, cot.double().permute(0, 3, 1, 2) * float(s), stride, pad)
    check(f"dgrad N={N} {H}x{W} {Ci}<-{Co} K={K} s={stride}", got.permute(0, 3, 1, 2), gx + res.double().permute(0, 3, 1, 2))


# ---------------------------------------------------------------------------------------------- 4. the stem
@functools.lru_cache(maxsize=1)
def stem_inputs(N, H, W):
    """(img, w, b, wt, z64, gated) of a stem backward case; the float64 activation is computed once for the tests that share a case"""
    g = _rng(N + H)
    img = _f32(g, N, 3, H, W)
    img[0, :, 4:28, 6:30] = 0.75                                           # a constant patch: the windows inside it hold ties
    w = _f32(g, 64, 3, 7, 7, scale=0.08)
    b = _f32(g, 64, scale=0.1)
    w[5], b[5] = 0.0, -1.0                                                 # an all-negative channel: every gate closed, every window a tie
    wt = w.reshape(64, 147).t().contiguous()
    z64 = torch.nn.functional.conv2d(img.double(), w.double(), b.double(), 2, 3)
    pooled = torch.nn.functional.max_pool2d(torch.relu(z64), 3, 2, 1)
    cot = _f32(g, N, H // 4, W // 4, 64)
    gated = torch.where(pooled.permute(0, 2, 3, 1) > 0, cot.double(), torch.zeros(1, dtype=torch.float64)).float().contiguous()
    assert not bool(gated[..., 5].any())
    return img, w, b, wt, z64, gated


# (11, 224, 224): image chunks of 10 + 1 (stem_plan: 8 Mi floats of pre-pool activations at a time), 1232 weight-gradient rows on the 256 blocks of
# stem_bwd_wgrad_kernel; (129, 64, 64): chunks of 128 + 1, 4128 rows.  From the second chunk on the kernel accumulates onto the partial sums before it
@pytest.mark.parametrize("N,H,W", [(1, 32, 32), (2, 64, 32), (11, 224, 224), (129, 64, 64)])
def test_stem_backward(dev, N, H, W):
    from egohmr_amd import trunk_grad
    img, w, b, wt, z64, gated = stem_inputs(N, H, W)
    if N > 2:                                                              # the cases that are here for their second turns: prove they take them
        assert N > SR.backward_chunk(H, W) and N * (H // 2) > STEM_WGRAD_BLOCKS
    runs = [trunk_grad.stem_backward(img.to(dev), wt.to(dev), b.to(dev), gated.to(dev), debug=True) for _ in range(2)]
    torch.cuda.synchronize()
    gw, gb, z, gz = runs[0]
    assert all(torch.equal(a, c) for a, c in zip(runs[0], runs[1]))
    zerr = float((z.double().cpu().permute(0, 3, 1, 2) - z64).abs().max() / z64.abs().max())
    print(f"stem N={N} {H}x{W}: recomputed pre-pool activation max|err|/max = {zerr:.2e}")
    assert zerr <= 1e-5
    # inside the constant patch the activation is constant (ties): bit-equal on the device as in float64
    zc = z.cpu()[0, 4:12, 5:13, :]
    assert bool((zc == zc[:1, :1]).all())
    # routing against float64 on the device's own activation (the patch's ties are exact there); the float64 activation's arg-max is counted beside it
    rw, rb, rgz = R.stem_vjp(img.double(), gated.double().permute(0, 3, 1, 2), z.double().cpu().permute(0, 3, 1, 2))
    assert torch.equal(gz.cpu().double().permute(0, 3, 1, 2) != 0, rgz != 0)
    check(f"stem N={N} {H}x{W} gz", gz.permute(0, 3, 1, 2), rgz)
    _, _, rgz64 = R.stem_vjp(img.double(), gated.double().permute(0, 3, 1, 2), z64)
    assert not bool(rgz[:, 5].any()) and bool(rgz[0, :, 4:12, 5:13].any())
    flips = int(((rgz64 != 0) != (rgz != 0)).sum())
    # a flip needs two candidates of a window closer than the recompute's error (zerr <= 1e-5 of the maximum, asserted above): with activations spread
    # over the maximum's range at most a few windows in 1e5 qualify; one in a thousand positions is a loose ceiling on that
    assert flips <= rgz.numel() // 1000
    print(f"stem N={N} {H}x{W}: arg-max positions that differ between the float32 and the float64 activation: {flips} of {rgz.numel()}")
    check(f"stem N={N} {H}x{W} w", gw, rw)
    check(f"stem N={N} {H}x{W} b", gb, rb)
    # either output alone
    only_w = trunk_grad.stem_backward(img.to(dev), wt.to(dev), b.to(dev), gated.to(dev), True, False)
    only_b = trunk_grad.stem_backward(img.to(dev), wt.to(dev), b.to(dev), gated.to(dev), False, True)
    assert only_w[1] is None and only_b[0] is None and torch.equal(only_w[0], gw) and torch.equal(only_b[1], gb)


def test_stem_backward_chunks_agree_with_whole_batch_steps(dev):
    """ehm_resnet_stem_backward (image chunks, partial sums accumulated from the second chunk on) against the three steps the train-mode BatchNorm route
    runs over the whole batch (ehm_resnet_stem_preact / _route / _wgrad): z and gz are per-pixel results and bit-equal; the weight and bias gradients
    are summed in different orders, so each is held to float64 at the VJP bar instead."""
    from egohmr_amd import _lib, trunk_grad
    A = _lib.api()
    N, H, W = 129, 64, 64
    assert N > SR.backward_chunk(H, W) and N * H // 2 > STEM_WGRAD_BLOCKS                                # a second chunk, a second row per block
    img, w, b, wt, z64, gated = stem_inputs(N, H, W)
    imgd, wtd, bd, gd = img.to(dev), wt.to(dev), b.to(dev), gated.to(dev)
    gw, gb, z, gz = trunk_grad.stem_backward(imgd, wtd, bd, gd, debug=True)
    fz, z2 = guarded(dev, N, H // 2, W // 2, 64)
    fgz, gz2 = guarded(dev, N, H // 2, W // 2, 64)
    fw, gw2 = guarded(dev, 64, 147)
    fb, gb2 = guarded(dev, 64)
    z2.fill_(NAN), gz2.fill_(NAN)
    ws = torch.full((trunk_grad.STEM_WGRAD_WS_FLOATS,), NAN, device=dev)
    A.ehm_resnet_stem_preact(imgd, wtd, bd, z2, N, H, W, _lib.stream_ptr())
    A.ehm_resnet_stem_route(z2, gd, gz2, N, H, W, _lib.stream_ptr())
    A.ehm_resnet_stem_wgrad(imgd, gz2, gw2, gb2, N, H, W, ws, ws.numel() * 4, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert all(guards_intact(f) for f in (fz, fgz, fw, fb))
    assert torch.equal(z.view(torch.int32), z2.view(torch.int32)) and torch.equal(gz.view(torch.int32), gz2.view(torch.int32))
    rw, rb, _ = R.stem_vjp(img.double(), gated.double().permute(0, 3, 1, 2), z.double().cpu().permute(0, 3, 1, 2))
    for tag, a, c in (("chunked", gw, gb), ("whole batch", gw2.view(64, 3, 7, 7), gb2)):
        check(f"stem N={N} {H}x{W} {tag} w", a, rw)
        check(f"stem N={N} {H}x{W} {tag} b", c, rb)


# ---------------------------------------------------------------------------------------------- 5. the whole trunk on the device's gates
def device_chain_reference(m, img, gout):
    """Forward on the device with the activations kept and read back; the float64 VJP chain of trunk_grad_ref on the device's gates and pool arg-max and on
    the folded float32 weights the device runs.  -> (forward output, {parameter name: float64 gradient})."""
    from egohmr_amd import _lib, trunk_grad
    fn = m.current()
    acts = []
    with _lib.on_device(img.device):
        out = fn(img, saved=acts)
        N, _, H, W = img.shape
        _, _, z, _ = trunk_grad.stem_backward(img, fn.stem_wt, fn.stem_b, torch.zeros(N, H // 4, W // 4, 64, device=img.device), debug=True)
    torch.cuda.synchronize()
    folded = {0: (fn.stem[0].double().cpu(), fn.stem[1].double().cpu())}
    for b, blk in enumerate(fn.blocks):
        for j, p in enumerate(blk):
            if p is not None:
                folded[1 + 4 * b + j] = (p[0].double().cpu(), p[1].double().cpu())
    chans = [64] + [c for blk in fn.blocks for c in (blk[0][0].shape[0], blk[1][0].shape[0], blk[2][0].shape[0])]
    acts64 = [nchw(R.x2_decode(buf, s[0] * s[1] * s[2], Cn), s, Cn) for (buf, s), Cn in zip(acts, chans)]
    res = R.trunk_vjp_chain(folded, img.double().cpu(), acts64, z.double().cpu().permute(0, 3, 1, 2), gout.double().cpu())
    sd = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    return out, R.unfold_all(sd, res)


def run_module(m, img, gout):
    m.zero_grad(set_to_none=True)
    out = m(img)
    out.backward(gout)
    torch.cuda.synchronize()
    return out, {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}


def compare_params(tag, got, ref, maxnorm=False):
    fails, worst = [], (0.0, "")
    for n, r in ref.items():
        assert got[n] is not None, f"{n} received no gradient"
        gd = got[n].double().cpu()
        S = float(r.abs().max())
        assert S > 0 and gd.shape == r.shape, n
        err = (gd - r).abs()
        rel = float(err.max()) / S
        worst = max(worst, (rel, n))
        ok = rel <= ATOL if maxnorm else bool((err <= ATOL * S + RTOL * r.abs()).all())
        if not ok:
            fails.append(f"{n} ({rel:.2e})")
    print(f"[{tag}] {len(ref)} tensors, worst max|err|/max|ref| = {worst[0]:.2e} at {worst[1]}")
    assert not fails, f"{tag}: over the bar: {fails}"


@pytest.mark.parametrize("B,H,W,seed", [(1, 32, 32, 1), (2, 64, 64, 2)])
def test_whole_trunk_on_the_devices_gates(dev, B, H, W, seed):
    sd = R.make_state(seed)
    m = R.load_module(sd, dev)
    m.grad_params = True
    img, gout = R.make_image(B, H, W, seed).float().to(dev), R.make_cotangent(B, seed).float().to(dev)
    out0, ref = device_chain_reference(m, img, gout)
    out, got = run_module(m, img, gout)
    assert out.grad_fn is not None and torch.equal(out.detach(), out0)
    assert len(ref) == 159
    compare_params(f"trunk, device gates, B={B} {H}x{W}", got, ref)


# ---------------------------------------------------------------------------------------------- 6. free running at the committed seed
@pytest.fixture(scope="module")
def e2e(dev):
    """E2E_SEED's module, inputs and float64 autograd reference: computed once, shared, left unchanged."""
    B, H, W = E2E_SHAPE
    sd = R.make_state(E2E_SEED)
    img, gout = R.make_image(B, H, W, E2E_SEED), R.make_cotangent(B, E2E_SEED)
    ref, out64 = R.autograd_grads(sd, img, gout)
    m = R.load_module(sd, dev)
    return dict(sd=sd, m=m, img=img.float().to(dev), gout=gout.float().to(dev), ref=ref, out64=out64)


def test_whole_trunk_free_running(dev, e2e):
    assert E2E_F32_ERROR <= ATOL / 4
    m = e2e["m"]
    m.grad_params = True
    out, got = run_module(m, e2e["img"], e2e["gout"])
    ferr = float((out.detach().double().cpu() - e2e["out64"]).abs().max() / e2e["out64"].abs().max())
    print(f"free running, seed {E2E_SEED}: forward max|err|/max|ref| = {ferr:.2e}")
    assert ferr <= 5e-5
    compare_params(f"trunk, free running, seed {E2E_SEED}", got, e2e["ref"], maxnorm=True)


# ---------------------------------------------------------------------------------------------- 7. route and bits
def test_route_and_bits(dev, e2e):
    m, img, gout = e2e["m"], e2e["img"], e2e["gout"]
    stats = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    m.grad_params = False
    plain = m(img)
    assert plain.grad_fn is None and not plain.requires_grad              # default-requires_grad parameters under grad mode: no graph
    m.grad_params = True
    with torch.no_grad():
        ng = m(img)
    assert ng.grad_fn is None and torch.equal(ng, plain)
    out, g1 = run_module(m, img, gout)
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)   # the same launches: the same bits
    _, g2 = run_module(m, img, gout)
    assert all(torch.equal(g1[n], g2[n]) for n in g1)                     # no atomics: bit-repeatable
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in stats.items()) and len(stats) == 3 * 53
    with pytest.raises(NotImplementedError, match="image gradient"):
        m(img.clone().requires_grad_())
    # a frozen conv: None for it, the others unchanged
    blk = m.layer3[2]
    frozen = [blk.conv2.weight, blk.bn2.weight, blk.bn2.bias]
    try:
        for p in frozen:
            p.requires_grad_(False)
        _, g3 = run_module(m, img, gout)
        names = {id(p): n for n, p in m.named_parameters()}
        for n in g1:
            if n in {names[id(p)] for p in frozen}:
                assert g3[n] is None, n
            else:
                assert torch.equal(g3[n], g1[n]), n
        # only the last block's bn3.bias trainable: nothing below it runs, one gradient comes back
        for p in m.parameters():
            p.requires_grad_(False)
        m.layer4[2].bn3.bias.requires_grad_(True)
        _, g4 = run_module(m, img, gout)
        assert [n for n, v in g4.items() if v is not None] == ["layer4.2.bn3.bias"] and torch.equal(g4["layer4.2.bn3.bias"], g1["layer4.2.bn3.bias"])
        for p in m.parameters():
            p.requires_grad_(False)
        assert m(img).grad_fn is None                                      # nothing requires grad: the no-graph route
        # bias-only fine-tuning: every conv weight and BatchNorm weight frozen, every BatchNorm bias trainable - the projection blocks' downsample
        # unit then wants the column sum conv3 already produced and nothing else; the 53 bias gradients have the full run's bits
        for n, p in m.named_parameters():
            p.requires_grad_(n.endswith(".bias"))
        _, g5 = run_module(m, img, gout)
        got = sorted(n for n, v in g5.items() if v is not None)
        assert got == sorted(n for n in g1 if n.endswith(".bias")) and len(got) == 53
        assert all(torch.equal(g5[n], g1[n]) for n in got)
        # ... and the mix the other way round at a projection block: its downsample weight alone
        for p in m.parameters():
            p.requires_grad_(False)
        m.layer2[0].downsample[0].weight.requires_grad_(True)
        m.layer2[0].bn3.bias.requires_grad_(True)
        _, g6 = run_module(m, img, gout)
        assert sorted(n for n, v in g6.items() if v is not None) == ["layer2.0.bn3.bias", "layer2.0.downsample.0.weight"]
        assert all(torch.equal(g6[n], g1[n]) for n in ("layer2.0.bn3.bias", "layer2.0.downsample.0.weight"))
        # a parameter changed between forward and backward is refused, not mixed with the forward's folded weights
        for p in m.parameters():
            p.requires_grad_(True)
        from egohmr_amd import _lib
        out = m(img)
        keep = m.layer1[0].bn1.bias.detach().clone()
        with torch.no_grad():
            m.layer1[0].bn1.bias.add_(1.0)
        with pytest.raises(_lib.EgoHMRHipError, match="between the forward and the backward"):
            out.backward(gout)
        with torch.no_grad():
            m.layer1[0].bn1.bias.copy_(keep)
        _, g7 = run_module(m, img, gout)                                   # restored: the full run again
        assert all(torch.equal(g7[n], g1[n]) for n in g1)
    finally:
        for p in m.parameters():
            p.requires_grad_(True)
        m.grad_params = False
        m.zero_grad(set_to_none=True)


# ---------------------------------------------------------------------------------------------- 7b. the fixed-order SMPL backward of the training route
def test_ordered_smpl_backward(dev, smpl_asset, monkeypatch):
    """SMPL.ordered_backward: off by default and then the entry point that always ran; on, a dense cotangent (thousands of vertices per joint) gives the
    same bits twice and agrees with the atomic route to the VJP bar (the two differ by the order of float32 additions only)."""
    from egohmr_amd import _lib
    from egohmr_amd.geometry import rot6d_to_rotmat
    from egohmr_amd.smpl import SMPL
    B = 9                                                                  # two body groups, the second ragged
    smpl = SMPL(smpl_asset).to(dev)
    g = torch.Generator().manual_seed(17)
    R = rot6d_to_rotmat(torch.randn(B * 24, 6, generator=g).to(dev), "diffusion").view(B, 24, 3, 3).contiguous()
    betas = torch.randn(B, 10, generator=g).to(dev)
    gv, gj = torch.randn(B, smpl.num_verts, 3, generator=g).to(dev), torch.randn(B, smpl.num_joints_out, 3, generator=g).to(dev)
    calls = []
    api = _lib.api()
    for name in ("ehm_smpl_backward", "ehm_smpl_backward_ordered"):
        monkeypatch.setattr(api, name, (lambda fn, name: lambda *a: (calls.append(name), fn(*a))[1])(getattr(api, name), name))

    def grads(ordered):
        smpl.ordered_backward = ordered
        go, bp, be = R[:, :1].clone().requires_grad_(), R[:, 1:].clone().requires_grad_(), betas.clone().requires_grad_()
        o = smpl(betas=be, body_pose=bp, global_orient=go, pose2rot=False)
        smpl.ordered_backward = False                                      # read at the forward: the backward keeps what the forward saw
        out = torch.autograd.grad((o.vertices * gv).sum() + (o.joints * gj).sum(), [go, bp, be])
        torch.cuda.synchronize()
        return out
    assert SMPL.ordered_backward is False
    plain = grads(False)
    assert calls == ["ehm_smpl_backward"]
    first, second = grads(True), grads(True)
    assert calls == ["ehm_smpl_backward", "ehm_smpl_backward_ordered", "ehm_smpl_backward_ordered"]
    for name, a, b, c in zip(("global_orient", "body_pose", "betas"), first, second, plain):
        assert torch.equal(a, b), name
        check(f"ordered SMPL backward against the atomic one, {name}", a, c.double().cpu())


# ---------------------------------------------------------------------------------------------- 8. the wiring behind EgoHMR.trunk_grad
@pytest.fixture(scope="module")
def wiring(dev, golden_dir, synth_weights, smpl_asset):
    """The synthetic model on a two-item batch with the smallest image the stem allows: one forward + compute_loss + backward with trunk_grad off, the same
    again (the route's own run-to-run difference), and one with trunk_grad on; computed once, shared, left unchanged."""
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device, build_synthetic_model
    B = 2
    gd = np.load(os.path.join(golden_dir, "g21_val_losses_a.npz"))
    b_np, flags = VR.golden_batch(gd)
    cut = lambda d: {k: (cut(v) if isinstance(v, dict) else v[:B]) for k, v in d.items()}
    b_np = cut(b_np)
    b_np["img"] = _rng(3).normal(size=(B, 3, 32, 32)).astype(np.float32)             # the smallest image the stem allows
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
    captured = {}

    def hook(mod, inp, out):
        if out.requires_grad:
            captured["img_feats"] = out.detach().clone()
            out.register_hook(lambda gr: captured.__setitem__("g_img", gr.detach().clone()))
    handle = m.backbone.register_forward_hook(hook)

    def reset(trunk_grad):
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth_weights.items()}, strict=False)
        m.zero_grad(set_to_none=True)
        m.validation_setup()
        m.trunk_grad = trunk_grad
        m.init_optimizers()

    def step(trunk_grad):
        reset(trunk_grad)
        m._set_train_modes()
        out = m(batch, t, eval_with_uncond=False)
        loss = m.compute_loss(batch, out)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}, len(m.opt_params)

    try:
        off, off_again = step(False), step(False)
        assert "g_img" not in captured                                              # the frozen route never calls the module
        on = step(True)
        modes = (m.backbone.training, m.backbone.grad_params)
    finally:
        handle.remove()
    yield dict(m=m, batch=batch, t=t, off=off, off_again=off_again, on=on, captured=captured, reset=reset, modes=modes)
    m.trunk_grad = False
    m.validation_setup()


def test_training_route_with_trunk_grad(dev, wiring):
    w = wiring
    m, (loss0, g0, n0), (loss1, g1, n1) = w["m"], w["off"], w["on"]
    n_all, n_bb = len(list(m.parameters())), len(list(m.backbone.parameters()))
    assert all(v is None for n, v in g0.items() if n.startswith("backbone.")) and n0 == n_all - n_bb and n1 == n_all
    assert w["modes"] == (False, False)                                             # eval mode; grad_params set for the call, restored after
    assert torch.equal(loss0, loss1)                                                # the same img_feats bits: the same forward
    # the backbone's gradients: the float64 VJP chain (device gates) of the cotangent that reached img_feats
    img = w["batch"]["img"].float().contiguous()
    out_chain, ref = device_chain_reference(m.backbone, img, w["captured"]["g_img"])
    assert torch.equal(out_chain, w["captured"]["img_feats"])
    compare_params("EgoHMR.trunk_grad backbone", {n[len("backbone."):]: v for n, v in g1.items() if n.startswith("backbone.")}, ref)
    # every other gradient: the one the frozen route gives, to the VJP bar (bit equality is the next test's)
    fails = []
    for n in g0:
        if not n.startswith("backbone.") and g0[n] is not None:
            check(n, g1[n], g0[n].double().cpu(), fails) if not torch.equal(g0[n], g1[n]) else None
    assert not fails, fails
    # one training_step: every conv weight and BatchNorm affine of the backbone moves, every buffer keeps its bits, the backbone stays in eval mode
    w["reset"](True)
    assert m.opt_params[0] is m.backbone.conv1.weight
    before_p = {n: p.detach().clone() for n, p in m.backbone.named_parameters()}
    before_b = {n: v.detach().clone() for n, v in m.backbone.named_buffers()}
    m.training_step(w["batch"], w["t"], 0)
    torch.cuda.synchronize()
    assert len(before_p) == 159 and not [n for n, p in m.backbone.named_parameters() if torch.equal(p.detach(), before_p[n])]
    assert len(before_b) == 159 and all(torch.equal(v, before_b[n]) for n, v in m.backbone.named_buffers())
    assert not m.backbone.training and all(not mod.training for mod in m.backbone.modules())


def test_training_route_other_gradients_are_bit_equal(dev, wiring):
    """With trunk_grad the loss and every non-backbone gradient have the bits of the trunk_grad = False run - and two trunk_grad = False runs have each
    other's: the route has no order-dependent sum (ehm_smpl_backward adds its skinning gradient in a fixed order; docs/EXPERIMENTS.md R16.4)."""
    (loss0, g0, _), (_, g0b, _), (loss1, g1, _) = wiring["off"], wiring["off_again"], wiring["on"]
    others = [n for n in g0 if not n.startswith("backbone.") and g0[n] is not None]
    rel = lambda a, b: float((a - b).abs().max() / a.abs().max())
    base = [rel(g0[n], g0b[n]) for n in others if not torch.equal(g0[n], g0b[n])]
    differ = [rel(g0[n], g1[n]) for n in others if not torch.equal(g0[n], g1[n])]
    print(f"{len(others)} non-backbone gradients; trunk_grad off twice: {len(base)} differ (max {max(base, default=0.0):.2e} of max|g|); "
          f"off against on: {len(differ)} differ (max {max(differ, default=0.0):.2e})")
    assert torch.equal(loss0, loss1)
    assert others and not base and not differ
