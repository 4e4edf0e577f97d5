"""GPU: the backward of the scene PointNet (csrc/pointnet_bwd.hip, egohmr_amd/pointnet_grad.py, ResnetPointnet.forward's autograd route) against
float64: every C entry alone, pointnet_backward on saved state built from the float64 forward (so both sides share every ReLU gate and every pooled
row), end to end through ResnetPointnet.__call__, the route selection, and bit-for-bit repeatability.

Bar of the gradients: the project's VJP bar, atol = 2e-4 max|ref|, rtol = 2e-3 (tests/test_gpu_gcn_autograd.py); every case prints what it measured.
The C entries around the GEMMs are float32 element-wise arithmetic and fixed-order float32 sums of at most 52 terms before float64 takes over (24 rows
of a lane + 8 row lanes, or 48 rows of a wave + 4 waves): their bound is the float32 one, 64 * 2^-24 * sum|terms| per output.
Shapes: H = 128 (the smallest the tile engine takes), out_dim = 64, N in {1, 5, 191, 192, 193, 400} (group padding of nearly a tile, 1 row, 0; 1, 2
and 3 row tiles per body), B in {1, 3}."""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

from tests import pointnet_grad_ref as R
from tests.test_pointnet_autograd_cpu import E2E_MARGIN, E2E_SEED

pytestmark = pytest.mark.gpu

H, OUT = 128, 64
NS, BS = (1, 5, 191, 192, 193, 400), (1, 3)
ATOL, RTOL = 2e-4, 2e-3
U32 = 64 * 2.0 ** -24
CANARY = 123456.0
GUARD = 64


def _dev():
    return torch.device("cuda")


def _lib():
    from egohmr_amd import _lib
    return _lib


def _rng(*key):
    return np.random.Generator(np.random.PCG64(zlib.crc32(repr(key).encode())))


def _npad(N):
    return (N + 191) // 192 * 192


def guarded(*shape, dtype=torch.float32):
    """(view of `shape`, whole buffer): the view sits between two guard bands of the canary."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), CANARY, dtype=dtype, device=_dev())
    return whole[GUARD:GUARD + n].view(*shape), whole


def guards_intact(whole):
    return bool((whole[:GUARD] == CANARY).all()) and bool((whole[-GUARD:] == CANARY).all())


def pack_x2(t):
    """float32 [M, C] -> the X2 split format (csrc/gcn_dev.h: per 32 columns, 32 f16 hi halves then 32 f16 lo halves; value = hi + lo) as a float32-sized
    buffer [M, C], the way the forward's stores split a value (hi = f16(v), lo = f16(v - hi))."""
    M, C = t.shape
    hi = t.half()
    lo = (t - hi.float()).half()
    x = torch.stack([hi.view(M, C // 32, 32), lo.view(M, C // 32, 32)], dim=2).contiguous()        # [M, C/32, 2, 32] halves
    return x.view(M, 2 * C).view(torch.float32).view(M, C)


def unpack_x2(buf):
    M, C = buf.shape
    x = buf.view(torch.float16).view(M, C // 32, 2, 32)
    return (x[:, :, 0].float() + x[:, :, 1].float()).reshape(M, C)


def padded(t, Np, fill):
    """[B, N, C] -> [B * Np, C] float32 on the device with `fill` in the padding rows."""
    B, N, C = t.shape
    out = torch.full((B, Np, C), fill, dtype=torch.float32, device=_dev())
    out[:, :N] = t.to(_dev(), torch.float32)
    return out.view(B * Np, C)


def valid(t, B, N):
    """[B * Np, C] -> ([B, N, C] valid rows, [B, Np - N, C] padding rows) on the CPU as float64."""
    t = t.view(B, -1, t.shape[-1]).cpu().double()
    return t[:, :N], t[:, N:]


def workspace(L, B, Np, C):
    nb = ctypes.c_int64(0)
    L.api().ehm_pointnet_bwd_workspace_bytes(B, Np, C, ctypes.byref(nb))
    return torch.empty(nb.value // 4, device=_dev()), nb.value


def sum_bound(terms, dims):
    return U32 * terms.abs().sum(dims) + 1e-30


GRID = [(B, N) for B in BS for N in NS]


# ---------------------------------------------------------------------------------------------- 1. each C entry alone
@pytest.mark.parametrize("x2", [0, 1])
@pytest.mark.parametrize("B,N", GRID)
def test_pool_argmax(B, N, x2):
    L = _lib()
    C, Np, g = H, _npad(N), _rng("argmax", B, N)
    # multiples of 1/64 below 2048/64: exact in f16, so both formats hold the same values - and natural ties are frequent
    net = torch.from_numpy(g.integers(-2000, 2000, size=(B, N, C)) / 64.0)
    if N >= 3:
        a, b, c = sorted(g.choice(N, 3, replace=False).tolist())
        net[:, a, 0] = net[:, b, 0] = 40.0                                # two equal maxima
        net[:, a, 1] = net[:, b, 1] = net[:, c, 1] = 41.0                 # three
        net[:, b, 5] = net[:, c, 5] = float("nan")                        # a NaN column: the lowest NaN row
        net[0, a, 6] = float("nan")
        net[0, b, 6] = 50.0                                               # a NaN beats a larger number behind it ...
        net[0, 0, 7] = 50.0
        net[0, c, 7] = float("nan")                                       # ... and in front of it
    net[:, 0, 2] = 42.0                                                   # the maximum in row 0
    net[:, N - 1, 3] = 43.0                                               # and in row N - 1
    net[:, :, 4] = -net[:, :, 4].abs() - 1.0                              # an all-negative column
    ref = R.argmax_lowest(net)
    if N >= 3:
        assert ref[:, 0].tolist() == [a] * B and ref[:, 1].tolist() == [a] * B and ref[:, 5].tolist() == [b] * B and ref[0, 6] == a and ref[0, 7] == c
    assert ref[:, 2].tolist() == [0] * B and ref[:, 3].tolist() == [N - 1] * B
    buf = padded(net, Np, 60000.0 if x2 else 1e30)                        # padding rows that would win (X2: the largest f16 magnitude around)
    if x2:
        buf = pack_x2(buf)
    arg, whole = guarded(B, C, dtype=torch.int32)
    ws, nb = workspace(L, B, Np, C)
    L.api().ehm_pointnet_pool_argmax(buf, x2, arg, B, N, Np, C, ws, nb, L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(arg.cpu().long(), ref)
    assert bool((whole[:GUARD] == int(CANARY)).all()) and bool((whole[-GUARD:] == int(CANARY)).all())


@pytest.mark.parametrize("with_gnet", [False, True])
@pytest.mark.parametrize("B,N", GRID)
def test_scatter(B, N, with_gnet):
    L = _lib()
    C, Np, g = H, _npad(N), _rng("scatter", B, N)
    gnet = torch.from_numpy(g.normal(size=(B, N, C))).float()
    gpool = torch.from_numpy(g.normal(size=(B, C))).float()
    arg = torch.from_numpy(g.integers(0, N, size=(B, C)))
    ref = (torch.arange(N).view(1, N, 1) == arg.unsqueeze(1)) * gpool.double().unsqueeze(1)
    if with_gnet:
        ref = ref + gnet.double()
    G, wG = guarded(B * Np, C)
    s, ws_ = guarded(C)
    sg, wsg = guarded(B, C)
    ws, nb = workspace(L, B, Np, C)
    L.api().ehm_pointnet_bwd_scatter(padded(gnet, Np, float("nan")) if with_gnet else None, gpool.to(_dev()), arg.int().to(_dev()), G, s, sg,
                                     B, N, Np, C, ws, nb, L.stream_ptr())
    torch.cuda.synchronize()
    got, pad = valid(G, B, N)
    assert torch.equal(got, ref.float().double())                          # one float32 addition: the rounded exact sum
    assert pad.numel() == 0 or bool((pad == 0).all())
    assert all(guards_intact(w) for w in (wG, ws_, wsg))
    e_g, e_t = (sg.cpu().double() - ref.sum(1)).abs(), (s.cpu().double() - ref.sum((0, 1))).abs()
    print(f"scatter B={B} N={N}: group sums {float(e_g.max()):.2e}, total {float(e_t.max()):.2e}")
    assert bool((e_g <= sum_bound(ref, 1)).all()) and bool((e_t <= sum_bound(ref, (0, 1))).all())
    # the sums are optional, and so is then the workspace
    G2, wG2 = guarded(B * Np, C)
    L.api().ehm_pointnet_bwd_scatter(None, gpool.to(_dev()), arg.int().to(_dev()), G2, None, None, B, N, Np, C, None, 0, L.stream_ptr())
    if not with_gnet:
        assert torch.equal(G2, G)
    assert guards_intact(wG2)


@pytest.mark.parametrize("x2,with_add", [(0, False), (1, False), (0, True), (1, True)])
@pytest.mark.parametrize("B,N", GRID)
def test_gate(B, N, x2, with_add):
    L = _lib()
    C, Np, g = (2 * H if not x2 else H), _npad(N), _rng("gate", B, N)      # float32 gate source: net0's width
    T = torch.from_numpy(g.normal(size=(B, N, C))).float()
    act = torch.from_numpy(g.normal(size=(B, N, C))).float()
    act[:, :, 3] = 0.0                                                     # a zero is not positive
    act[:, :, 4] = -0.0
    add = torch.from_numpy(g.normal(size=(B, N, C))).float()
    ts, as_ = 0.25, 8.0                                                    # powers of two, as pointnet_grad hands them over
    ref = torch.where(act > 0, T.double() * ts, torch.zeros((), dtype=torch.float64))
    if with_add:
        ref = ref + add.double() * as_
    a = padded(act, Np, 7.0)
    out, wo = guarded(B * Np, C)
    s, ws_ = guarded(C)
    sg, wsg = guarded(B, C)
    ws, nb = workspace(L, B, Np, C)
    dv = lambda v: torch.tensor(v, device=_dev())
    Td = padded(T, Np, float("nan"))
    args = (pack_x2(a) if x2 else a, x2, padded(add, Np, float("nan")) if with_add else None, dv(ts), dv(as_) if with_add else None)
    L.api().ehm_pointnet_bwd_gate(Td, *args, out, s, sg, B, N, Np, C, ws, nb, L.stream_ptr())
    torch.cuda.synchronize()
    got, pad = valid(out, B, N)
    err = (got - ref).abs()
    print(f"gate B={B} N={N} x2={x2} add={with_add}: max|err|/max|ref| = {float(err.max() / ref.abs().max()):.2e}")
    assert bool((err <= 2.0 ** -23 * ref.abs()).all())                     # float32 rounding of one product and one sum
    assert bool((got[:, :, 3:5] == (ref[:, :, 3:5])).all())
    assert pad.numel() == 0 or bool((pad == 0).all())
    assert all(guards_intact(w) for w in (wo, ws_, wsg))
    e_g, e_t = (sg.cpu().double() - ref.sum(1)).abs(), (s.cpu().double() - ref.sum((0, 1))).abs()
    assert bool((e_g <= sum_bound(ref, 1)).all()) and bool((e_t <= sum_bound(ref, (0, 1))).all())
    # in place, no sums, default factors
    L.api().ehm_pointnet_bwd_gate(Td, args[0], x2, None, None, None, Td, None, None, B, N, Np, C, None, 0, L.stream_ptr())
    got2, pad2 = valid(Td, B, N)
    assert torch.equal(got2, torch.where(act > 0, T, torch.zeros(())).double()) and (pad2.numel() == 0 or bool((pad2 == 0).all()))


@pytest.mark.parametrize("x2,relu,wide", [(1, 0, False), (1, 1, False), (0, 0, True)])
@pytest.mark.parametrize("B,N", GRID)
def test_wgrad(B, N, x2, relu, wide):
    """out = P^T act(Q) over the valid rows: the three uses (G^T relu(h) / G^T net, dh^T relu(net), block 0's dh^T relu(net0) on float32 rows, 2H wide)."""
    L = _lib()
    Cg, Ca, Np, g = H, (2 * H if wide else H), _npad(N), _rng("wgrad", B, N)
    P = torch.from_numpy(g.normal(size=(B, N, Cg))).float()
    Q = torch.from_numpy(g.normal(size=(B, N, Ca))).float()
    Qd = padded(Q, Np, float("nan"))                                       # padding rows must not enter, whatever they hold
    if x2:
        Qd = pack_x2(Qd)
        Q = unpack_x2(Qd).view(B, Np, Ca)[:, :N].cpu()                     # what the kernel reads: hi + lo
    Qa = Q.double().clamp_min(0) if relu else Q.double()
    ref = torch.einsum("bng,bna->ga", P.double(), Qa)
    mag = torch.einsum("bng,bna->ga", P.double().abs(), Qa.abs())
    ld = Ca + 128
    out, wo = guarded(Cg, ld)
    nb = ctypes.c_int64(0)
    L.api().ehm_pointnet_bwd_wgrad_workspace_bytes(B, Np, Cg, Ca, ctypes.byref(nb))
    ws = torch.empty(nb.value // 4, device=_dev())
    L.api().ehm_pointnet_bwd_wgrad(padded(P, Np, float("nan")), Qd, x2, relu, out, ld, B, N, Np, Cg, Ca, ws, nb.value, L.stream_ptr())
    torch.cuda.synchronize()
    err = (out[:, :Ca].cpu().double() - ref).abs()
    print(f"wgrad B={B} N={N} x2={x2} relu={relu}: max|err|/max|ref| = {float(err.max() / ref.abs().max()):.2e}")
    # a float32 fmaf chain over the rows of one run (at most one 192-row slab at these shapes), then float64 over the runs, one rounding of the result
    assert bool((err <= (192 + 2) * 2.0 ** -24 * mag + 1e-30).all())
    assert bool((out[:, Ca:] == CANARY).all()) and guards_intact(wo)       # the other columns of a wider matrix are left alone


@pytest.mark.parametrize("B,N", GRID)
def test_net0(B, N):
    L = _lib()
    C, Np, g = 2 * H, _npad(N), _rng("net0", B, N)
    p = torch.from_numpy(g.uniform(-1, 1, size=(B, N, 3))).float()
    W = torch.from_numpy(g.normal(size=(C, 3))).float()
    b = torch.from_numpy(g.normal(scale=0.05, size=(C,))).float()
    ref = p.double() @ W.double().T + b.double()
    mag = p.double().abs() @ W.double().abs().T + b.double().abs()
    n0, w0 = guarded(B * Np, C)
    r0, w1 = guarded(B * Np, C)
    L.api().ehm_pointnet_bwd_net0(p.to(_dev()), W.to(_dev()), b.to(_dev()), n0, r0, B, N, Np, C, L.stream_ptr())
    torch.cuda.synchronize()
    got, pad = valid(n0, B, N)
    gotr, padr = valid(r0, B, N)
    err = (got - ref).abs()
    print(f"net0 B={B} N={N}: max|err|/max|ref| = {float(err.max() / ref.abs().max()):.2e}")
    assert bool((err <= 4 * 2.0 ** -24 * mag).all())                       # three fused multiply-adds
    assert torch.equal(gotr, got.clamp_min(0))
    assert all(x.numel() == 0 or bool((x == 0).all()) for x in (pad, padr)) and guards_intact(w0) and guards_intact(w1)
    r1, w2 = guarded(B * Np, C)
    L.api().ehm_pointnet_bwd_net0(p.to(_dev()), W.to(_dev()), b.to(_dev()), None, r1, B, N, Np, C, L.stream_ptr())
    assert torch.equal(r1, r0) and guards_intact(w2)


@pytest.mark.parametrize("with_p", [False, True])
@pytest.mark.parametrize("B,N", GRID)
def test_lift(B, N, with_p):
    L = _lib()
    C, Np, g = (2 * H if with_p else H), _npad(N), _rng("lift", B, N)      # net0bar is 2H wide, G (block 0's shortcut factor) H
    X = torch.from_numpy(g.normal(size=(B, N, C))).float()
    p = torch.from_numpy(g.uniform(-1, 1, size=(B, N, 3))).float()
    W = torch.from_numpy(g.normal(size=(C, 3))).float()
    Xd, pd, Wd = X.double(), p.double(), W.double()
    gW, wW = guarded(C, 3)
    gb, wb = guarded(C)
    gp, wp = guarded(B, N, 3)
    ws, nb = workspace(L, B, Np, C)
    L.api().ehm_pointnet_bwd_lift(padded(X, Np, float("nan")), p.to(_dev()), W.to(_dev()) if with_p else None, gW, gb, gp if with_p else None,
                                  B, N, Np, C, ws, nb, L.stream_ptr())
    torch.cuda.synchronize()
    eW = (gW.cpu().double() - torch.einsum("bnc,bnk->ck", Xd, pd)).abs()
    eb = (gb.cpu().double() - Xd.sum((0, 1))).abs()
    print(f"lift B={B} N={N}: weight {float(eW.max()):.2e}, bias {float(eb.max()):.2e}")
    assert bool((eW <= U32 * torch.einsum("bnc,bnk->ck", Xd.abs(), pd.abs()) + 1e-30).all())
    assert bool((eb <= sum_bound(Xd, (0, 1))).all())
    if with_p:
        ep = (gp.cpu().double() - Xd @ Wd).abs()
        assert bool((ep <= U32 * (Xd.abs() @ Wd.abs()) + 1e-30).all())
    else:
        assert bool((gp == CANARY).all())                                  # not asked for: not written
    assert all(guards_intact(w) for w in (wW, wb, wp))
    if with_p:                                                             # each output alone
        gp2, wp2 = guarded(B, N, 3)
        L.api().ehm_pointnet_bwd_lift(padded(X, Np, 0.0), p.to(_dev()), W.to(_dev()), None, None, gp2, B, N, Np, C, ws, nb, L.stream_ptr())
        assert torch.equal(gp2, gp) and guards_intact(wp2)


# ---------------------------------------------------------------------------------------------- the module and its float64 reference
def make_module(sd, grad_params=True):
    from egohmr_amd.encoders import ResnetPointnet
    m = ResnetPointnet(out_dim=OUT, hidden_dim=H)
    m.load_state_dict({k[len(R.PREFIX):]: v.float() for k, v in sd.items()})
    m.grad_params = grad_params
    return m.to(_dev())


@functools.lru_cache(maxsize=None)
def reference(B, N, seed, zero_fc1, gscale):
    """float64 forward + autograd of one case, computed once: (sd, points, gout, out, intermediates, pbar, gradients)."""
    sd = R.make_weights(H, OUT, seed, zero_fc1=zero_fc1)
    p = R.make_points(B, N, seed).float().double()                         # what the float32 route is given, exactly
    gout = torch.from_numpy(_rng("gout", B, N, seed).normal(size=(B, OUT))).float().double() * gscale
    return (sd, p, gout) + R.autograd_reference(sd, p, gout)


def compare(tag, got_p, got, pbar, grads, names=R.PARAM_NAMES):
    worst = 0.0
    for name, a, r in [("p", got_p, pbar)] + [(n, got[R.PARAM_NAMES.index(n)], grads[n]) for n in names]:
        assert a is not None, name
        a = a.detach().cpu().double()
        assert a.shape == r.shape, (name, a.shape, r.shape)
        mx = float(r.abs().max())
        err = (a - r).abs()
        ratio = float(err.max()) / mx if mx > 0 else float(err.max())
        worst = max(worst, ratio)
        print(f"{tag} {name}: max|err|/max|ref| = {ratio:.2e}")
        assert bool((err <= ATOL * mx + RTOL * r.abs()).all()), (tag, name, ratio)
    return worst


def saved_from_float64(it, p, B, N):
    """The saved state of the autograd route built from the float64 forward: activations rounded to float32 and packed as the route stores them
    (garbage in the padding rows), the pooled vectors as float32, arg from float64."""
    Np = _npad(N)
    return dict(p=p.float().to(_dev()).contiguous(), B=B, N=N, Np=Np,
                rh=[pack_x2(padded(torch.relu(h), Np, 3.0)) for h in it["h"]], net=[pack_x2(padded(n, Np, 3.0)) for n in it["net"]],
                pooled=torch.stack(it["pooled"]).float().to(_dev()), arg=[a.int().to(_dev()) for a in it["arg"]])


REGIMES = {"synthetic": (False, 1.0), "fc1_zero": (True, 1.0), "tiny_gout": (False, 1e-9)}


# ---------------------------------------------------------------------------------------------- 2. pointnet_backward with shared gates
@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("B,N", [(B, N) for B in BS for N in (1, 193, 400)])
def test_backward_with_shared_gates(B, N, regime):
    from egohmr_amd import pointnet_grad
    zero_fc1, gscale = REGIMES[regime]
    sd, p, gout, out, it, pbar, grads = reference(B, N, 11, zero_fc1, gscale)
    m = make_module(sd)
    with torch.no_grad():
        gp, got = pointnet_grad.pointnet_backward(m, saved_from_float64(it, p, B, N), gout.float().to(_dev()), True, [True] * 24)
    torch.cuda.synchronize()
    compare(f"shared-gates B={B} N={N} {regime}", gp, got, pbar, grads)


def test_backward_takes_the_argmax_from_the_saved_net_when_none_is_given():
    from egohmr_amd import pointnet_grad
    B, N = 3, 193
    sd, p, gout, out, it, pbar, grads = reference(B, N, 11, False, 1.0)
    m = make_module(sd)
    sv = saved_from_float64(it, p, B, N)
    sv["arg"] = None
    with torch.no_grad():
        gp, got = pointnet_grad.pointnet_backward(m, sv, gout.float().to(_dev()), True, [True] * 24)
    compare("saved-net argmax", gp, got, pbar, grads)


# ---------------------------------------------------------------------------------------------- 3. end to end
def run_module(m, p64, gout64):
    p = p64.float().to(_dev()).requires_grad_()
    for q in m.parameters():
        q.grad = None
    c = m(p)
    c.backward(gout64.float().to(_dev()))
    torch.cuda.synchronize()
    return c, p


@pytest.mark.parametrize("B,N", list(E2E_SEED))
def test_end_to_end_through_the_module(B, N):
    seed = E2E_SEED[(B, N)]
    sd, p, gout, out, it, pbar, grads = reference(B, N, seed, False, 1.0)
    assert R.margin(sd, p) >= E2E_MARGIN                                   # on the float64 reference alone
    m = make_module(sd)
    c, pt = run_module(m, p, gout)
    assert c.grad_fn is not None and c.dtype == torch.float32 and c.shape == (B, OUT)
    with torch.no_grad():
        c0 = m(pt.detach())
    assert c0.grad_fn is None and torch.equal(c0, c.detach())              # the same launches: the same bits
    e = float((c.detach().cpu().double() - out).abs().max() / out.abs().max())
    print(f"e2e B={B} N={N} forward: max|err|/max|ref| = {e:.2e}")
    assert e < 1e-5
    got = [q.grad for q in m.grad_parameters()]
    compare(f"e2e B={B} N={N}", pt.grad, got, pbar, grads)


# ---------------------------------------------------------------------------------------------- 4. routing
def test_routing():
    from egohmr_amd import _lib as L
    B, N = 2, 3
    seed = E2E_SEED[(B, N)]
    sd, p, gout, out, it, pbar, grads = reference(B, N, seed, False, 1.0)
    # grad_params off: p only
    m = make_module(sd, grad_params=False)
    c, pt = run_module(m, p, gout)
    assert c.grad_fn is not None and all(q.grad is None for q in m.parameters())
    compare("routing p-only", pt.grad, [None] * 24, pbar, grads, names=())
    # grad mode on, default flags, p without requires_grad: today's route
    c = m(pt.detach())
    assert c.grad_fn is None and not c.requires_grad
    # no_grad with grad_params
    m.grad_params = True
    with torch.no_grad():
        c = m(pt.detach().requires_grad_())
    assert c.grad_fn is None
    # parameters alone ask for the route
    c = m(pt.detach())
    assert c.grad_fn is not None
    # a frozen parameter keeps .grad None; the others are as in the end-to-end test
    m.block_2.fc_0.weight.requires_grad_(False)
    c, pt2 = run_module(m, p, gout)
    assert m.block_2.fc_0.weight.grad is None
    names = tuple(n for n in R.PARAM_NAMES if n != "block_2.fc_0.weight")
    compare("routing frozen", pt2.grad, [q.grad for q in m.grad_parameters()], pbar, grads, names=names)
    # the plain-f16 tier is refused on the autograd route, by name
    m.hi_only = True
    with pytest.raises(L.EgoHMRHipError, match="hi_only"):
        m(pt.detach().requires_grad_())
    with torch.no_grad():
        assert m(pt.detach()).shape == (B, OUT)                             # and still runs without a gradient to compute


# ---------------------------------------------------------------------------------------------- 5. determinism
def test_two_backward_calls_give_the_same_bits():
    from egohmr_amd import pointnet_grad
    B, N = 3, 400
    sd, p, gout, out, it, pbar, grads = reference(B, N, 11, False, 1.0)
    m = make_module(sd)
    sv = saved_from_float64(it, p, B, N)
    sv["arg"] = None
    runs = []
    for _ in range(2):
        with torch.no_grad():
            gp, got = pointnet_grad.pointnet_backward(m, sv, gout.float().to(_dev()), True, [True] * 24)
        runs.append([gp] + got)
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 6. the packed operands follow an in-place update
def test_in_place_update_repacks_both_routes_operands():
    """A weight updated in place between two calls: the one cache key invalidates the forward's packed operands and the backward's - output, p.grad and the
    24 gradients equal, bit for bit, those of a fresh module that loaded the updated weights."""
    B, N = 2, 3
    sd, p, gout, out, it, pbar, grads = reference(B, N, E2E_SEED[(B, N)], False, 1.0)

    def run(m):
        c, pt = run_module(m, p, gout)
        return [c.detach(), pt.grad] + [q.grad for q in m.grad_parameters()]

    m = make_module(sd)
    before = run(m)
    with torch.no_grad():
        m.block_1.fc_1.weight.mul_(0.5)
    got = run(m)
    assert not torch.equal(got[0], before[0])
    fresh = make_module({R.PREFIX + k: v for k, v in m.state_dict().items()})
    want = run(fresh)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a is not None and torch.equal(a, b), i
