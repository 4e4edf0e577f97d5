"""GPU (MI355X), one process: the data-parallel BatchNorm entries of csrc/gcn_train.hip and csrc/bn2d_train.hip called directly - a z split into two row
shards, `local` on each, the outputs stacked as the all-gather would, `merge` - against float64 statistics / the float64 BatchNorm backward of the WHOLE z
(tests/bn_sync_ref.py), and with world = 1 bit for bit against the one-call entries.

Bars: var rtol 1e-5 and mean atol 1e-6 sqrt(var) (test_statistics_under_cancellation of tests/test_gpu_gcn_train.py, whose construction of a z with
|mean| / std = 30 and a correctly roundable mean is used here too); running statistics after two calls rtol 1e-5 + atol 1e-6 sqrt(running_var)
(test_running_statistics_after_two_calls there); the backward at the project's VJP bar, atol = 2e-4 max|ref|, rtol = 2e-3.

bn2d's channel counts: 64, 160 (one full 128-column block and a tail of 32) in both forms, and 136 (a tail of ONE 8-channel lane) as float32 rows - an X2
buffer's granule is 32 channels, so 136 cannot exist in that form and the entries refuse it (asserted).  Every case prints what it measured."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tests import bn_sync_ref as S  # noqa: E402
from tests import trunk_grad_ref as TG  # noqa: E402
from tests.test_gpu_gcn_train import _create, _layer  # noqa: E402
from tests.test_gpu_trunk_autograd import pack_x2  # noqa: E402

pytestmark = pytest.mark.gpu

VJP_ATOL_REL, VJP_RTOL = 2e-4, 2e-3
EPS, MOMENTUM = 1e-5, 0.1
CANARY = 12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def adj(dev):
    from egohmr_amd.model import smpl_tree_adjacency
    return smpl_tree_adjacency().to(dev)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def make_z(g, sizes, Cn, regime):
    """float32 rows [sum sizes, C].  'ratio30': every channel's |mean| / std = 30 over ALL rows, the mean m 2^k with m in [30, 31.9] (half a float32 ulp of
    it is then below 0.96e-6 std: a correctly rounded mean meets the bar).  'opposite': the first shard's mean at +30 sigma, the second's at -30 sigma of
    the within-shard spread.  'plain': O(1) means and spreads."""
    R = sum(sizes)
    r = g.normal(size=(R, Cn))
    if regime == "ratio30":
        r = (r - r.mean(0)) / r.std(0)
        mu = g.uniform(30.0, 31.9, size=Cn) * 2.0 ** g.integers(-2, 4, size=Cn) * g.choice([-1.0, 1.0], size=Cn)
        z = mu + np.abs(mu) / 30.0 * r
    elif regime == "opposite":
        sigma = g.uniform(0.5, 2.0, size=Cn)
        off = np.concatenate([np.full((n, 1), s) for n, s in zip(sizes, (30.0, -30.0))])
        z = sigma * (r + off)
    else:
        z = g.uniform(0.5, 2.0, size=Cn) * r + g.normal(size=Cn)
    return torch.from_numpy(z.astype(np.float32))


def check_stats(tag, mean, var, z64, regime):
    """mean / var float32 [C] on the device against float64 statistics of z64 [R, C] (CPU) at the issue's bars."""
    mean64, var64 = z64.mean(0), z64.var(0, unbiased=False)
    std64 = var64.sqrt()
    if regime == "ratio30":
        ratio = mean64.abs() / std64
        assert float(ratio.min()) > 29.5 and float(ratio.max()) < 30.5, (float(ratio.min()), float(ratio.max()))
        half_ulp = 2.0 ** (torch.floor(torch.log2(mean64.abs())) - 24)
        assert bool((half_ulp < 0.96e-6 * std64).all())                       # the premise: a correctly rounded mean meets the bar
    var, mean = var.double().cpu(), mean.double().cpu()
    print(f"[{tag}] max rel err of var {float(((var - var64).abs() / var64).max()):.2e}, max |mean err| / std {float(((mean - mean64).abs() / std64).max()):.2e}")
    np.testing.assert_allclose(var.numpy(), var64.numpy(), rtol=1e-5, atol=0, err_msg=tag)
    assert bool(((mean - mean64).abs() <= 1e-6 * std64).all()), tag


def check_running(tag, rm, rv, zs64, rm0, rv0):
    """Two successive calls: the device's running statistics against the float64 momentum rule on all rows of each call."""
    want_m, want_v = rm0.double().cpu().numpy(), rv0.double().cpu().numpy()
    for z64 in zs64:
        want_m, want_v = S.running_update(want_m, want_v, z64.mean(0).numpy(), z64.var(0, unbiased=False).numpy(), z64.shape[0], MOMENTUM)
    atol = 1e-6 * np.sqrt(want_v)
    for got, want, name in ((rm, want_m, "running_mean"), (rv, want_v, "running_var")):
        err = np.abs(got.double().cpu().numpy() - want)
        print(f"[{tag}] {name} after two calls: max err / (atol + rtol |ref|) = {float((err / (atol + 1e-5 * np.abs(want))).max()):.2e}")
        assert bool((err <= atol + 1e-5 * np.abs(want)).all()), (tag, name)


def check_vjp(tag, got, ref):
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    Sc = float(ref.abs().max())
    err = (got - ref).abs()
    print(f"[{tag}] max|err|/max|ref| = {float(err.max()) / Sc:.2e} (max|ref| {Sc:.3g})")
    assert bool((err <= VJP_ATOL_REL * Sc + VJP_RTOL * ref.abs()).all()), tag


def rows_of(*v):
    return (C.c_int64 * len(v))(*v)


def guarded(n, dev, dtype=torch.float32):
    full = torch.full((n + 16,), CANARY, device=dev, dtype=dtype)
    return full, full[:n]


# ---------------------------------------------------------------------------------------------- csrc/gcn_train.hip
HID = 256


class GCNCase:
    def __init__(self, dev, adj, seed):
        from egohmr_amd import _lib
        g = _rng(seed)
        self.dev, self.A, self.g = dev, _lib.api(), g
        self.layer = _layer("neg", g, HID, HID, dev)
        self.h = _create(dev, adj, self.layer, [], _layer("syn", g, HID, 6, dev, False), HID)

    def ws(self, bodies):
        nb = C.c_int64(0)
        self.A.ehm_gcn_train_workspace_bytes(self.h, -1, bodies, C.byref(nb))
        return torch.empty(nb.value // 8, device=self.dev, dtype=torch.float64), nb.value

    def stats_local(self, z, bodies):
        ws, nb = self.ws(bodies)
        full, local = guarded(2 * HID, self.dev, torch.float64)
        self.A.ehm_gcn_train_stats_local(self.h, -1, z, bodies, 0, local, ws, nb, None)
        assert bool((full[2 * HID:] == CANARY).all())
        return local.view(2, HID).clone()

    def stats_merge(self, gathered, rows, eps, momentum, rm=None, rv=None):
        fm, mean = guarded(HID, self.dev)
        fi, invstd = guarded(HID, self.dev)
        self.A.ehm_gcn_train_stats_merge(self.h, -1, gathered.contiguous(), rows_of(*rows), len(rows), eps, momentum, mean, invstd, rm, rv, None)
        assert bool((fm[HID:] == CANARY).all()) and bool((fi[HID:] == CANARY).all())
        return mean.clone(), invstd.clone()

    def bwd_local(self, gout, gate, z, mean, invstd, bodies):
        ws, nb = self.ws(bodies)
        local = torch.empty(2, HID, device=self.dev, dtype=torch.float64)
        self.A.ehm_gcn_train_bwd_local(self.h, -1, gout, gate, z, mean, invstd, bodies, local, ws, nb, None)
        return local

    def bwd_merge(self, gathered, rows, rank, gout, gate, z, mean, invstd, bodies):
        ws, nb = self.ws(bodies)
        fz, zbar = guarded(bodies * 24 * HID, self.dev)
        gw, gb = torch.empty(HID, device=self.dev), torch.empty(HID, device=self.dev)
        self.A.ehm_gcn_train_bwd_merge(self.h, -1, gathered.contiguous(), rows_of(*rows), len(rows), rank, gout, gate, z, mean, invstd, bodies, zbar, gw, gb,
                                       ws, nb, None)
        assert bool((fz[bodies * 24 * HID:] == CANARY).all())
        return zbar.view(bodies * 24, HID).clone(), gw, gb


@pytest.fixture(scope="module")
def gcn(dev, adj):
    c = GCNCase(dev, adj, 5)
    yield c
    torch.cuda.synchronize()
    c.h.close()


@pytest.mark.parametrize("regime", ["ratio30", "opposite"])
@pytest.mark.parametrize("split", [(3, 1), (2, 2)])
def test_gcn_forward_two_shards(dev, gcn, split, regime):
    g = _rng(sum(split) * 10 + split[0] + len(regime))
    rows = [24 * b for b in split]
    zs = [make_z(g, rows, HID, regime) for _ in range(2)]
    tag = f"gcn fwd bodies {split[0]}+{split[1]} {regime}"
    # eps = 0, momentum = 1: invstd gives the variance back and the running statistics ARE the batch's
    z = zs[0].to(dev)
    shards = [z[:rows[0]].contiguous(), z[rows[0]:].contiguous()]
    gathered = torch.stack([gcn.stats_local(s, b) for s, b in zip(shards, split)])
    rm, rv = torch.zeros(HID, device=dev), torch.zeros(HID, device=dev)
    mean, invstd = gcn.stats_merge(gathered, rows, 0.0, 1.0, rm, rv)
    again = gcn.stats_merge(gathered, rows, 0.0, 1.0)
    assert torch.equal(mean, again[0]) and torch.equal(invstd, again[1])          # every rank merges the same buffer: the same bits
    check_stats(tag, mean, 1.0 / invstd.double() ** 2, zs[0].double(), regime)
    R = sum(rows)
    assert torch.equal(rm, mean)
    np.testing.assert_allclose((rv.double() * (R - 1) / R).cpu().numpy(), zs[0].double().var(0, unbiased=False).numpy(), rtol=1e-5, atol=0)
    # two calls with the module's eps and momentum
    g0 = _rng(77)
    rm0 = torch.from_numpy(g0.normal(scale=0.1, size=HID).astype(np.float32)).to(dev)
    rv0 = torch.from_numpy(g0.uniform(0.6, 1.4, size=HID).astype(np.float32)).to(dev)
    rm, rv = rm0.clone(), rv0.clone()
    for zc in zs:
        zc = zc.to(dev)
        gathered = torch.stack([gcn.stats_local(zc[:rows[0]].contiguous(), split[0]), gcn.stats_local(zc[rows[0]:].contiguous(), split[1])])
        gcn.stats_merge(gathered, rows, EPS, MOMENTUM, rm, rv)
    check_running(tag, rm, rv, [zc.double() for zc in zs], rm0, rv0)


@pytest.mark.parametrize("regime", ["plain", "ratio30"])
def test_gcn_world_of_one_is_the_one_call_entry_bit_for_bit(dev, gcn, regime):
    bodies = 131                                                                   # one past the 128 body groups of the reductions
    g = _rng(131 + len(regime))
    z = make_z(g, [bodies * 24], HID, regime).to(dev)
    ws, nb = gcn.ws(bodies)
    mean1, inv1 = torch.empty(HID, device=dev), torch.empty(HID, device=dev)
    rm1, rv1 = torch.full((HID,), 0.25, device=dev), torch.full((HID,), 1.5, device=dev)
    gcn.A.ehm_gcn_train_stats(gcn.h, -1, z, bodies, 0, EPS, MOMENTUM, mean1, inv1, rm1, rv1, ws, nb, None)
    rm2, rv2 = torch.full((HID,), 0.25, device=dev), torch.full((HID,), 1.5, device=dev)
    mean2, inv2 = gcn.stats_merge(gcn.stats_local(z, bodies)[None], [bodies * 24], EPS, MOMENTUM, rm2, rv2)
    for a, b, name in ((mean1, mean2, "mean"), (inv1, inv2, "invstd"), (rm1, rm2, "running_mean"), (rv1, rv2, "running_var")):
        assert torch.equal(a, b), name
    gout = torch.from_numpy(g.normal(size=(bodies * 24, HID)).astype(np.float32)).to(dev)
    gate = torch.from_numpy(g.normal(size=(bodies * 24, HID)).astype(np.float32)).to(dev)
    zbar1, gw1, gb1 = torch.empty_like(z), torch.empty(HID, device=dev), torch.empty(HID, device=dev)
    gcn.A.ehm_gcn_train_bn_backward(gcn.h, -1, gout, gate, z, mean1, inv1, bodies, zbar1, gw1, gb1, ws, nb, None)
    local = gcn.bwd_local(gout, gate, z, mean1, inv1, bodies)
    zbar2, gw2, gb2 = gcn.bwd_merge(local[None], [bodies * 24], 0, gout, gate, z, mean1, inv1, bodies)
    assert torch.equal(zbar1, zbar2) and torch.equal(gw1, gw2) and torch.equal(gb1, gb2)


@pytest.mark.parametrize("regime", ["plain", "ratio30", "opposite"])
@pytest.mark.parametrize("split", [(3, 1), (2, 2)])
def test_gcn_backward_two_shards(dev, gcn, split, regime):
    g = _rng(sum(split) * 100 + split[0] + len(regime))
    rows = [24 * b for b in split]
    z = make_z(g, rows, HID, regime)
    gout = torch.from_numpy(g.normal(size=z.shape).astype(np.float32))
    gate = torch.from_numpy(g.normal(size=z.shape).astype(np.float32))
    gamma = gcn.layer["bn_weight"].double().cpu().numpy()
    ref_z, ref_b, ref_g = S.bn_backward((gout * (gate > 0)).numpy(), z.numpy(), gamma, EPS)
    cut = lambda t: [t[:rows[0]].contiguous().to(dev), t[rows[0]:].contiguous().to(dev)]
    zs, gos, gas = cut(z), cut(gout), cut(gate)
    mean, invstd = gcn.stats_merge(torch.stack([gcn.stats_local(s, b) for s, b in zip(zs, split)]), rows, EPS, MOMENTUM)
    gathered = torch.stack([gcn.bwd_local(gos[r], gas[r], zs[r], mean, invstd, split[r]) for r in range(2)])
    tag = f"gcn bwd bodies {split[0]}+{split[1]} {regime}"
    outs = [gcn.bwd_merge(gathered, rows, r, gos[r], gas[r], zs[r], mean, invstd, split[r]) for r in range(2)]
    at = 0
    for r in range(2):
        check_vjp(f"{tag} zbar of rank {r}", outs[r][0], ref_z[at:at + rows[r]])
        at += rows[r]
        # the parameter gradients a rank hands out are its OWN sums, as float32 of its float64 ones
        assert torch.equal(outs[r][1], gathered[r, 1].float()) and torch.equal(outs[r][2], gathered[r, 0].float())
    check_vjp(f"{tag} summed bn.weight gradient", outs[0][1].double() + outs[1][1].double(), ref_g)
    check_vjp(f"{tag} summed bn.bias gradient", outs[0][2].double() + outs[1][2].double(), ref_b)


def test_gcn_entries_refuse_bad_arguments(dev, gcn):
    from egohmr_amd import _lib
    A, h = gcn.A, gcn.h
    bodies = 2
    t = torch.zeros(bodies * 24, HID, device=dev)
    v = torch.zeros(HID, device=dev)
    loc = torch.zeros(2, HID, device=dev, dtype=torch.float64)
    gat = torch.zeros(2, 2, HID, device=dev, dtype=torch.float64)
    ws, nb = gcn.ws(bodies)
    odd = torch.zeros(2 * HID + 1, device=dev, dtype=torch.float32)[1:]            # 4 bytes off an 8-byte boundary
    bad = [lambda: A.ehm_gcn_train_stats_local(h, 1, t, bodies, 0, loc, ws, nb, None),                                   # no such hidden conv
           lambda: A.ehm_gcn_train_stats_local(h, -1, t, 0, 0, loc, ws, nb, None),
           lambda: A.ehm_gcn_train_stats_local(h, -1, t, bodies, 2, loc, ws, nb, None),
           lambda: A.ehm_gcn_train_stats_local(h, -1, t, bodies, 0, None, ws, nb, None),
           lambda: A.ehm_gcn_train_stats_local(h, -1, t, bodies, 0, odd, ws, nb, None),
           lambda: A.ehm_gcn_train_stats_local(h, -1, t, bodies, 0, loc, ws, 16, None),                                  # workspace too small
           lambda: A.ehm_gcn_train_stats_merge(h, -1, gat, rows_of(48, 48), 0, EPS, MOMENTUM, v, v.clone(), None, None, None),       # world >= 1
           lambda: A.ehm_gcn_train_stats_merge(h, -1, gat, rows_of(48, 0), 2, EPS, MOMENTUM, v, v.clone(), None, None, None),        # a rank without rows
           lambda: A.ehm_gcn_train_stats_merge(h, -1, gat, rows_of(48, 25), 2, EPS, MOMENTUM, v, v.clone(), None, None, None),       # no whole bodies
           lambda: A.ehm_gcn_train_stats_merge(h, -1, gat, None, 2, EPS, MOMENTUM, v, v.clone(), None, None, None),
           lambda: A.ehm_gcn_train_stats_merge(h, -1, gat, rows_of(48, 48), 2, EPS, MOMENTUM, v, v.clone(), v.clone(), None, None),  # one running statistic
           lambda: A.ehm_gcn_train_stats_merge(h, -1, gat, rows_of(48, 48), 2, -1.0, MOMENTUM, v, v.clone(), None, None, None),
           lambda: A.ehm_gcn_train_bwd_local(h, -1, t, t, t, v, v, bodies, None, ws, nb, None),
           lambda: A.ehm_gcn_train_bwd_local(h, -1, t, t, t, v, v, bodies, loc, ws, 16, None),
           lambda: A.ehm_gcn_train_bwd_merge(h, -1, gat, rows_of(48, 48), 2, 2, t, t, t, v, v, bodies, torch.zeros_like(t), None, None, ws, nb, None),   # rank
           lambda: A.ehm_gcn_train_bwd_merge(h, -1, gat, rows_of(72, 48), 2, 0, t, t, t, v, v, bodies, torch.zeros_like(t), None, None, ws, nb, None),   # rows[rank]
           lambda: A.ehm_gcn_train_bwd_merge(h, -1, gat, rows_of(48, 48), 2, 0, t, t, t, v, v, bodies, t, None, None, ws, nb, None)]        # zbar over its input
    for i, f in enumerate(bad):
        with pytest.raises(_lib.EgoHMRHipError) as e:
            f()
        assert e.value.rc == -22, i


# ---------------------------------------------------------------------------------------------- csrc/bn2d_train.hip
HW = 7
IMAGES = (2, 1)                                   # pixels 2 * 7 * 7 + 1 * 7 * 7


class BN2D:
    """One form of z: an X2 buffer per shard, or float32 rows."""

    def __init__(self, dev, Cn, x2):
        from egohmr_amd import _lib, trunk_grad
        self.dev, self.C, self.x2, self.A, self.tg = dev, Cn, x2, _lib.api(), trunk_grad

    def put(self, x):
        """float32 [pixels, C] on the CPU -> (the device form, the float64 values it holds)"""
        if self.x2:
            buf = pack_x2(x, self.dev)                   # the tile padding and the zero row hold NaN halves
            return buf, TG.x2_decode(buf, x.shape[0], self.C)
        full = torch.full((x.shape[0] + 8, self.C), float("nan"), device=self.dev)
        full[:x.shape[0]] = x.to(self.dev)
        return full[:x.shape[0]], x.double()

    def ws(self, pixels):
        return self.tg._bn_ws(pixels, self.C, self.dev)

    def stats_local(self, buf, pixels):
        ws, nb = self.ws(pixels)
        full, local = guarded(2 * self.C, self.dev, torch.float64)
        self.A.ehm_bn2d_train_stats_local(buf, int(self.x2), buf.shape[0], pixels, self.C, local, ws, nb, None)
        assert bool((full[2 * self.C:] == CANARY).all())
        return local.view(2, self.C).clone()

    def stats_merge(self, gathered, rows, eps, momentum, rm=None, rv=None, nbt=None):
        outs = [guarded(self.C, self.dev) for _ in range(3)]
        self.A.ehm_bn2d_train_stats_merge(gathered.contiguous(), rows_of(*rows), len(rows), self.C, eps, momentum, outs[0][1], outs[1][1], outs[2][1], rm, rv,
                                          nbt, None)
        assert all(bool((f[self.C:] == CANARY).all()) for f, _ in outs)
        return tuple(o.clone() for _, o in outs)

    def bwd_local(self, G, buf, pixels, mean, invstd):
        ws, nb = self.ws(pixels)
        local = torch.empty(2, self.C, device=self.dev, dtype=torch.float64)
        self.A.ehm_bn2d_train_bwd_local(G, buf, int(self.x2), buf.shape[0], pixels, self.C, mean, invstd, local, ws, nb, None)
        return local

    def bwd_merge(self, gathered, rank):
        o = [torch.empty(self.C, device=self.dev) for _ in range(4)]
        self.A.ehm_bn2d_train_bwd_merge(gathered.contiguous(), gathered.shape[0], rank, self.C, *o, None)
        return o

    def zbar(self, G, buf, shape, mean, invstd, gamma, gbeta, ggamma, total, scale=None, out_hw=None):
        return self.tg.bn_zbar(G, buf, shape, self.C, mean, invstd, gamma, gbeta, ggamma, scale=scale, out_hw=out_hw, x2=self.x2, total_rows=total)


FORMS = [(64, True), (64, False), (160, True), (160, False), (136, False)]


@pytest.mark.parametrize("regime", ["ratio30", "opposite"])
@pytest.mark.parametrize("Cn,x2", FORMS)
def test_bn2d_forward_two_shards(dev, Cn, x2, regime):
    b = BN2D(dev, Cn, x2)
    g = _rng(Cn * 3 + int(x2) + len(regime))
    rows = [n * HW * HW for n in IMAGES]
    tag = f"bn2d fwd C={Cn} {'X2' if x2 else 'f32'} pixels {rows[0]}+{rows[1]} {regime}"
    calls = []
    for _ in range(2):
        z = make_z(g, rows, Cn, regime)
        parts = [b.put(z[:rows[0]]), b.put(z[rows[0]:])]
        calls.append(([p[0] for p in parts], torch.cat([p[1] for p in parts])))
    bufs, z64 = calls[0]
    gathered = torch.stack([b.stats_local(buf, r) for buf, r in zip(bufs, rows)])
    rm, rv = torch.zeros(Cn, device=dev), torch.zeros(Cn, device=dev)
    nbt = torch.full((), 5, dtype=torch.int64, device=dev)
    mean, var, invstd = b.stats_merge(gathered, rows, 0.0, 1.0, rm, rv, nbt)
    assert all(torch.equal(p, q) for p, q in zip((mean, var, invstd), b.stats_merge(gathered, rows, 0.0, 1.0)))
    check_stats(tag, mean, var, z64, regime)
    R = sum(rows)
    np.testing.assert_allclose((1.0 / invstd.double() ** 2).cpu().numpy(), z64.var(0, unbiased=False).numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose((rv.double() * (R - 1) / R).cpu().numpy(), z64.var(0, unbiased=False).numpy(), rtol=1e-5, atol=0)
    assert torch.equal(rm, mean) and int(nbt) == 6
    g0 = _rng(78)
    rm0 = torch.from_numpy(g0.normal(scale=0.1, size=Cn).astype(np.float32)).to(dev)
    rv0 = torch.from_numpy(g0.uniform(0.6, 1.4, size=Cn).astype(np.float32)).to(dev)
    rm, rv = rm0.clone(), rv0.clone()
    for bufs, _ in calls:
        b.stats_merge(torch.stack([b.stats_local(buf, r) for buf, r in zip(bufs, rows)]), rows, EPS, MOMENTUM, rm, rv, nbt)
    check_running(tag, rm, rv, [c[1] for c in calls], rm0, rv0)
    assert int(nbt) == 8


@pytest.mark.parametrize("Cn,x2", [(64, True), (64, False), (160, True), (160, False)])
def test_bn2d_world_of_one_is_the_one_call_entries_bit_for_bit(dev, Cn, x2):
    """(the one-call entries take multiples of 32 channels only)"""
    b = BN2D(dev, Cn, x2)
    g = _rng(Cn + int(x2))
    N, pixels = 3, 3 * HW * HW
    for regime in ("plain", "ratio30"):
        buf, _ = b.put(make_z(g, [pixels], Cn, regime))
        bn = torch.nn.BatchNorm2d(Cn).to(dev)
        one = b.tg.bn_stats(buf, pixels, Cn, bn, x2=x2)
        rm, rv, nbt = torch.zeros(Cn, device=dev), torch.ones(Cn, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
        two = b.stats_merge(b.stats_local(buf, pixels)[None], [pixels], bn.eps, bn.momentum, rm, rv, nbt)
        assert all(torch.equal(p, q) for p, q in zip(one, two)), regime
        assert torch.equal(rm, bn.running_mean) and torch.equal(rv, bn.running_var) and int(nbt) == int(bn.num_batches_tracked) == 1
        mean, _, invstd = one
        G = torch.from_numpy(g.normal(scale=100.0, size=(pixels, Cn)).astype(np.float32))
        G[g.random((pixels, Cn)) < 0.4] = 0.0
        G = G.to(dev).view(N, HW, HW, Cn)
        gamma = torch.from_numpy((g.normal(size=Cn) * 0.3 + 1.0).astype(np.float32)).to(dev)
        gb1, gg1 = b.tg.bn_sums(G, buf, pixels, Cn, mean, invstd, x2=x2)
        gb2, gg2, ob, og = b.bwd_merge(b.bwd_local(G, buf, pixels, mean, invstd)[None], 0)
        assert torch.equal(gb1, gb2) and torch.equal(gg1, gg2) and torch.equal(gb1, ob) and torch.equal(gg1, og)
        s = torch.tensor(0.25, device=dev)
        for kw in (dict(), dict(scale=s, out_hw=(13, 13))):
            assert torch.equal(b.tg.bn_zbar(G, buf, (N, HW, HW), Cn, mean, invstd, gamma, gb1, gg1, x2=x2, **kw),
                               b.zbar(G, buf, (N, HW, HW), mean, invstd, gamma, gb2, gg2, pixels, **kw)), (regime, kw)


@pytest.mark.parametrize("regime", ["plain", "ratio30", "opposite"])
@pytest.mark.parametrize("Cn,x2", FORMS)
def test_bn2d_backward_two_shards(dev, Cn, x2, regime):
    b = BN2D(dev, Cn, x2)
    g = _rng(Cn * 5 + int(x2) + len(regime))
    rows = [n * HW * HW for n in IMAGES]
    R = sum(rows)
    z = make_z(g, rows, Cn, regime)
    parts = [b.put(z[:rows[0]]), b.put(z[rows[0]:])]
    z64 = torch.cat([p[1] for p in parts])
    G = torch.from_numpy(g.normal(scale=100.0, size=(R, Cn)).astype(np.float32))
    G[g.random((R, Cn)) < 0.4] = 0.0                                              # closed gates
    gamma = torch.from_numpy((g.normal(size=Cn) * 0.3 + 1.0).astype(np.float32))
    gamma[1] = -0.5
    ref_z, ref_b, ref_g = S.bn_backward(G.numpy(), z64.numpy(), gamma.numpy(), EPS)
    Gs = [G[:rows[0]].contiguous().to(dev).view(IMAGES[0], HW, HW, Cn), G[rows[0]:].contiguous().to(dev).view(IMAGES[1], HW, HW, Cn)]
    mean, var, invstd = b.stats_merge(torch.stack([b.stats_local(p[0], r) for p, r in zip(parts, rows)]), rows, EPS, MOMENTUM)
    gathered = torch.stack([b.bwd_local(Gs[r], parts[r][0], rows[r], mean, invstd) for r in range(2)])
    tag = f"bn2d bwd C={Cn} {'X2' if x2 else 'f32'} pixels {rows[0]}+{rows[1]} {regime}"
    own, at = [], 0
    for r in range(2):
        gb, gg, ob, og = b.bwd_merge(gathered, r)
        assert torch.equal(ob, gathered[r, 0].float()) and torch.equal(og, gathered[r, 1].float())
        own.append((ob, og))
        Z = b.zbar(Gs[r], parts[r][0], (IMAGES[r], HW, HW), mean, invstd, gamma.to(dev), gb, gg, R)
        check_vjp(f"{tag} zbar of rank {r}", Z.view(rows[r], Cn), ref_z[at:at + rows[r]])
        at += rows[r]
    check_vjp(f"{tag} all ranks' betabar", gb, ref_b)
    check_vjp(f"{tag} all ranks' gammabar", gg, ref_g)
    check_vjp(f"{tag} summed bn.bias gradient", own[0][0].double() + own[1][0].double(), ref_b)
    check_vjp(f"{tag} summed bn.weight gradient", own[0][1].double() + own[1][1].double(), ref_g)


def test_bn2d_one_row_per_rank_and_refusals(dev):
    """A rank may hold ONE row (a 32 x 32 image's layer 4); 136 channels cannot be an X2 buffer."""
    from egohmr_amd import _lib
    b = BN2D(dev, 64, False)
    g = _rng(3)
    z = make_z(g, [1, 1], 64, "plain")
    parts = [b.put(z[:1]), b.put(z[1:])]
    mean, var, invstd = b.stats_merge(torch.stack([b.stats_local(p[0], 1) for p in parts]), [1, 1], 0.0, 1.0)
    # two rows in all: a channel's |mean| / std is whatever the two values make it, so the mean's bar here is the float32 store's own rounding (one ulp)
    mean64, var64 = z.double().mean(0), z.double().var(0, unbiased=False)
    np.testing.assert_allclose(var.double().cpu().numpy(), var64.numpy(), rtol=1e-5, atol=0)
    assert bool(((mean.double().cpu() - mean64).abs() <= 2.0 ** -23 * mean64.abs()).all())
    A = _lib.api()
    ws, nb = b.ws(98)
    t = torch.zeros(194, 136, device=dev)
    loc = torch.zeros(2, 136, device=dev, dtype=torch.float64)
    v = torch.zeros(136, device=dev)
    bad = [lambda: A.ehm_bn2d_train_stats_local(t, 1, 194, 98, 136, loc, ws, 1 << 30, None),                  # X2 needs C % 32 == 0
           lambda: A.ehm_bn2d_train_bwd_local(t, t, 1, 194, 98, 136, v, v, loc, ws, 1 << 30, None),
           lambda: A.ehm_bn2d_train_stats_local(t, 0, 194, 0, 136, loc, ws, 1 << 30, None),                   # no rows
           lambda: A.ehm_bn2d_train_stats_local(t, 0, 194, 98, 136, loc, ws, 64, None),                       # workspace too small
           lambda: A.ehm_bn2d_train_stats_merge(loc[None], rows_of(1), 1, 136, EPS, MOMENTUM, v, v.clone(), v.clone(), None, None, None, None),   # one row in all
           lambda: A.ehm_bn2d_train_stats_merge(loc[None], rows_of(98), 0, 136, EPS, MOMENTUM, v, v.clone(), v.clone(), None, None, None, None),  # world >= 1
           lambda: A.ehm_bn2d_train_stats_merge(loc[None], rows_of(98, 0), 2, 136, EPS, MOMENTUM, v, v.clone(), v.clone(), None, None, None, None),
           lambda: A.ehm_bn2d_train_bwd_merge(loc[None], 1, 1, 136, v, v.clone(), None, None, None),            # rank outside the world
           lambda: A.ehm_bn2d_train_bwd_zbar_rows(t[:98], t, 0, 194, v, v, v, v, v, None, torch.zeros(98, 136, device=dev), 2, 7, 7, 136, 7, 7, 97, None)]
    for i, f in enumerate(bad):
        with pytest.raises(_lib.EgoHMRHipError) as e:
            f()
        assert e.value.rc == -22, i
