"""GPU (MI355X): the non-local block's backward behind ModulatedGCN.nonlocal_grad.

1. ehm_nonlocal_attention_backward (csrc/nonlocal_bwd.hip) against float64 of the same float32 inputs, in two regimes:
   "soft"    logits of standard deviation about 3 - what egohmr_amd.synthetic gives the block, and where training lives.  thetabar, phibar, gbar at the
             project's VJP bar (atol = 2e-4 max|ref|, rtol = 2e-3, per tensor).
   "peaked"  the construction of tests/test_gpu_linear.py::test_nonlocal_attention_vs_fp64: logits of standard deviation 40, the largest past 89, where exp
             overflows float32 without the max-subtraction.  gbar at the VJP bar.  thetabar / phibar = Fbar phi / Fbar^T theta with Fbar = P (.) (Pbar - D):
             Pbar - D cancels, so a correct float32 kernel cannot meet a bar relative to the cancelled result; the bound is built from the reference's
             float64 quantities alone, from that test's error model of a logit (an f32 fma chain over Ci channels: d <= 4 sqrt(Ci) 2^-24 (|l| + 4 r),
             r = sqrt(sum theta^2 phi^2), taken as its row maximum d_a) and the same model for Pbar (e_ab), to first order:
                 |dP_ab|    <= P_ab q_a,                 q_a = 2 d_a + 64 2^-24        (the softmax's Jacobian on a logit error; exp, normalisation)
                 |dD_a|     <= q_a S_a + sum_b P_ab e_ab + 32 2^-24 S_a,               S_a = sum_b P_ab (|Pbar_ab| + |D_a|)
                 |dFbar_ab| <= P_ab ((q_a + 8 2^-24)(|Pbar_ab| + |D_a|) + e_ab + |dD_a|)  =: E_ab
                 |dthetabar_ac| <= sum_b E_ab |phi_bc| + 32 2^-24 sum_b P_ab (|Pbar_ab| + |D_a|) |phi_bc|,   phibar alike over a with |theta_ac|
             doubled.  It is relative to sum_b P_ab (|Pbar_ab| + |D_a|) |phi_bc|, not to the cancelled result.
   All cases: canary rows behind the output untouched, a second call bit-equal.
2. gcn_grad.nonlocal_forward / nonlocal_backward against tests/nonlocal_ref.block in float64: the forward at 5e-5 max(1, max|ref|), all eleven gradients
   at the VJP bar, W.1's running statistics after two calls at rtol 1e-5 + atol 1e-6 sqrt(var) (the bars of tests/test_gpu_gcn_train.py).
   Gradients that are zero in exact arithmetic (tests/test_nonlocal_grad_cpu.py says why: phi.bias always; W.0.bias and g.bias under batch statistics) are
   held to the VJP bar's atol on the scale of the sum that does not cancel, and the reference's own to 1e-9 of it.
Every case prints its measured error ratios."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nonlocal_ref as NR  # noqa: E402

pytestmark = pytest.mark.gpu

VJP_ATOL_REL, VJP_RTOL = 2e-4, 2e-3
CANARY = -7.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _ratio(err, tol):
    return float((err / tol).max())


def vjp_ratio(got, ref):
    """max of |got - ref| / (atol + rtol |ref|) at the project's VJP bar (<= 1: met)"""
    ref = ref.double()
    return _ratio((got.double() - ref).abs(), VJP_ATOL_REL * float(ref.abs().max()) + VJP_RTOL * ref.abs())


# ---------------------------------------------------------------------------------------------- 1. the kernel
def _attention_reference(qkv, gy, bodies, Ci):
    th, ph, gv = (qkv[:, i * Ci:(i + 1) * Ci].double().view(bodies, 24, Ci) for i in range(3))
    yb = gy.double().view(bodies, 24, Ci)
    logit = th @ ph.transpose(1, 2)
    P = torch.softmax(logit, -1)
    Pb = yb @ gv.transpose(1, 2)
    D = (P * Pb).sum(-1, keepdim=True)
    Fb = P * (Pb - D)
    return dict(th=th, ph=ph, gv=gv, yb=yb, logit=logit, P=P, Pb=Pb, D=D, Fb=Fb, gth=Fb @ ph, gph=Fb.transpose(1, 2) @ th, gg=P.transpose(1, 2) @ yb)


def _peaked_bounds(r, Ci):
    """(bound of thetabar, bound of phibar) from the reference's float64 quantities alone: the module docstring's model"""
    u = 2.0 ** -24
    th, ph, gv, yb, P, Pb, D = r["th"], r["ph"], r["gv"], r["yb"], r["P"], r["Pb"], r["D"]
    chain = lambda val, a, b: 4 * math.sqrt(Ci) * u * (val.abs() + 4 * torch.sqrt((a * a) @ (b * b).transpose(1, 2)))
    d = chain(r["logit"], th, ph).amax(-1, keepdim=True)
    e = chain(Pb, yb, gv)
    q = 2 * d + 64 * u
    W = P * (Pb.abs() + D.abs())                          # the un-cancelled terms of Fbar
    S = W.sum(-1, keepdim=True)
    dD = q * S + (P * e).sum(-1, keepdim=True) + 32 * u * S
    E = (q + 8 * u) * W + P * (e + dD)
    return 2 * (E @ ph.abs() + 32 * u * (W @ ph.abs())), 2 * (E.transpose(1, 2) @ th.abs() + 32 * u * (W.transpose(1, 2) @ th.abs()))


@pytest.mark.parametrize("regime", ["soft", "peaked"])
@pytest.mark.parametrize("bodies", [1, 300])
@pytest.mark.parametrize("Ci", [32, 64, 96, 512])
def test_attention_backward_vs_fp64(dev, Ci, bodies, regime):
    from egohmr_amd import _lib
    A = _lib.api()
    g = torch.Generator(device=dev).manual_seed(Ci + bodies)
    rows = bodies * 24
    a = ((40.0 if regime == "peaked" else 3.0) / math.sqrt(Ci)) ** 0.5
    rnd = lambda: torch.randn(rows, Ci, generator=g, device=dev)
    qkv = torch.cat([rnd() * a, rnd() * a, rnd()], 1).contiguous()
    gy = rnd()
    r = _attention_reference(qkv, gy, bodies, Ci)
    lmax = float(r["logit"].abs().max())
    if regime == "peaked":
        assert lmax > 89.0                                    # exp overflows float32 without the max-subtraction
    else:
        assert 2.0 < float(r["logit"].std()) < 4.5 and lmax < 40.0
    buf = torch.full((rows + 2, 3 * Ci), CANARY, device=dev)          # two canary rows behind the output
    with _lib.on_device(dev):
        A.ehm_nonlocal_attention_backward(qkv, gy, buf, bodies, Ci, None)
        again = torch.full((rows + 2, 3 * Ci), CANARY, device=dev)
        A.ehm_nonlocal_attention_backward(qkv, gy, again, bodies, Ci, None)
    torch.cuda.synchronize()
    assert bool((buf[rows:] == CANARY).all()), "rows behind the output were written"
    assert torch.equal(buf, again), "two calls on the same inputs differ"
    got = buf[:rows].double()
    assert torch.isfinite(got).all()
    gth, gph, gg = (got[:, i * Ci:(i + 1) * Ci].reshape(bodies, 24, Ci) for i in range(3))
    tag = f"[non-local bwd {regime} Ci={Ci} bodies={bodies}] |logit|max = {lmax:.1f}"
    r_g = vjp_ratio(gg, r["gg"])
    if regime == "soft":
        r_t, r_p = vjp_ratio(gth, r["gth"]), vjp_ratio(gph, r["gph"])
        print(f"{tag}: err / VJP bar thetabar = {r_t:.3e}, phibar = {r_p:.3e}, gbar = {r_g:.3e}")
    else:
        bt, bp = _peaked_bounds(r, Ci)
        r_t, r_p = _ratio((gth - r["gth"]).abs(), bt), _ratio((gph - r["gph"]).abs(), bp)
        print(f"{tag}: err / bound thetabar = {r_t:.3e}, phibar = {r_p:.3e}; err / VJP bar gbar = {r_g:.3e}")
    assert r_t <= 1.0 and r_p <= 1.0 and r_g <= 1.0, (r_t, r_p, r_g)


# ---------------------------------------------------------------------------------------------- 2. the block's forward and backward
MOMENTUM = 0.1


def _block_module(sd, hid, dev):
    from egohmr_amd.model import _NonLocalBlock
    nl = _NonLocalBlock(hid)
    missing = nl.load_state_dict({k[len(NR.NL):]: v.float() for k, v in sd.items()}, strict=False)
    assert not missing.unexpected_keys and all("num_batches_tracked" in k for k in missing.missing_keys), missing
    return nl.to(dev)


def _zero_to_rounding(name, train):
    """the state-dict name of the gradient whose scale a gradient that is zero in exact arithmetic is held against, or None"""
    if name == "phi.bias":
        return "theta.bias"
    if train and name in ("W.0.bias", "g.bias"):
        return "W.1.bias"
    return None


def check_block_grads(tag, got, ref, train):
    """got / ref: dicts under 'x' and NR.BLOCK_PARAMS.  Asserts the VJP bar (and the zero-to-rounding rule) and prints every ratio."""
    worst = {}
    for k, r in ref.items():
        base = _zero_to_rounding(k, train)
        if base is None:
            worst[k] = vjp_ratio(got[k], r)
        else:
            scale = float(ref[base].abs().max())
            assert float(r.abs().max()) <= 1e-9 * scale, (k, "the reference's own is not zero to rounding")
            worst[k] = float(got[k].double().abs().max()) / (VJP_ATOL_REL * scale)
    print(f"{tag}: err / VJP bar " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def check_forward(tag, got, ref):
    bar = 5e-5 * max(1.0, float(ref.abs().max()))
    err = float((got.double() - ref).abs().max())
    print(f"{tag}: forward max err / bar = {err / bar:.3e}")
    assert err <= bar, (tag, err, bar)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("bodies", [1, 9, 33])
@pytest.mark.parametrize("hid", [64, 192, 1024])
def test_block_forward_backward_vs_fp64(dev, hid, bodies, train):
    """(The block's own GEMMs always run on the split-f16 engine: ModulatedGCN.precision selects the hidden convs' arithmetic, which the module tests of
    tests/test_gpu_nonlocal_module.py run in 'f16x3' and 'f32'.)"""
    from egohmr_amd import _lib, gcn_grad
    sd = NR.block_state(hid + bodies, hid)
    g = np.random.Generator(np.random.PCG64(7 * hid + bodies))
    rows = bodies * 24
    xs = [torch.from_numpy(g.normal(size=(bodies, 24, hid)).astype(np.float32)).double() for _ in range(2)]
    cot = torch.from_numpy(g.normal(size=(bodies, 24, hid)).astype(np.float32)).double()
    # the float64 reference: two calls (the running statistics), gradients of the first
    ref_sd = {k: v.clone().to(dev) for k, v in sd.items()}
    names = [NR.NL + k for k in NR.BLOCK_PARAMS]
    for n in names:
        ref_sd[n].requires_grad_(True)
    x0 = xs[0].to(dev).requires_grad_(True)
    out_ref = NR.block(ref_sd, x0, train, momentum=MOMENTUM)
    gs = torch.autograd.grad(out_ref, [x0] + [ref_sd[n] for n in names], cot.to(dev))
    ref = dict(zip(("x",) + NR.BLOCK_PARAMS, gs))
    with torch.no_grad():
        NR.block(ref_sd, xs[1].to(dev), train, momentum=MOMENTUM)
    # the HIP route
    nl = _block_module(sd, hid, dev).train(train)
    bn = nl.W[1]
    tag = f"[non-local block {'train' if train else 'eval'} hid={hid} bodies={bodies}]"
    with _lib.on_device(dev), torch.no_grad():
        nw = gcn_grad.NonLocalWeights(nl, dev)
        X = xs[0].float().to(dev).reshape(rows, hid).contiguous()
        out, st = gcn_grad.nonlocal_forward(nw, bn, X, bodies, train)
        r = gcn_grad.nonlocal_backward(nw, X, st, cot.float().to(dev).reshape(rows, hid).contiguous(), bodies)
        r2 = gcn_grad.nonlocal_backward(nw, X, st, cot.float().to(dev).reshape(rows, hid).contiguous(), bodies)
        gcn_grad.nonlocal_forward(nw, bn, xs[1].float().to(dev).reshape(rows, hid).contiguous(), bodies, train, save=False)
    torch.cuda.synchronize()
    check_forward(tag, out.view(bodies, 24, hid), out_ref.detach())
    got = {k: (v.view(bodies, 24, hid) if k == "x" else v) for k, v in r.items()}
    assert set(got) == set(ref) and all(got[k].shape == ref[k].shape for k in ref)
    for k in r:
        assert torch.equal(r[k], r2[k]), f"{k} differs between two identical calls"
    check_block_grads(tag, got, ref, train)
    if train:
        assert int(bn.num_batches_tracked) == 2
        want_m, want_v = ref_sd[NR.NL + "W.1.running_mean"], ref_sd[NR.NL + "W.1.running_var"]
        atol = 1e-6 * want_v.sqrt()
        for have, want, name in ((bn.running_mean, want_m, "running_mean"), (bn.running_var, want_v, "running_var")):
            err = (have.double() - want).abs()
            print(f"{tag} {name}: max err / (atol + rtol |ref|) = {float((err / (atol + 1e-5 * want.abs())).max()):.2e}")
            assert bool((err <= atol + 1e-5 * want.abs()).all()), name
        assert not torch.equal(bn.running_mean.double().cpu(), sd[NR.NL + "W.1.running_mean"])
    else:
        assert int(bn.num_batches_tracked) == 0 and torch.equal(bn.running_mean.double().cpu(), sd[NR.NL + "W.1.running_mean"])


def test_backward_computes_only_what_is_asked(dev):
    from egohmr_amd import _lib, gcn_grad
    hid, bodies = 64, 2
    sd = NR.block_state(5, hid)
    nl = _block_module(sd, hid, dev).eval()
    X = torch.randn(bodies * 24, hid, device=dev)
    G = torch.randn(bodies * 24, hid, device=dev)
    with _lib.on_device(dev), torch.no_grad():
        nw = gcn_grad.NonLocalWeights(nl, dev)
        _, st = gcn_grad.nonlocal_forward(nw, nl.W[1], X, bodies, False)
        full = gcn_grad.nonlocal_backward(nw, X, st, G, bodies)
        only_x = gcn_grad.nonlocal_backward(nw, X, st, G, bodies, True, (False,) * 10)
        only_beta = gcn_grad.nonlocal_backward(nw, X, st, G, bodies, False, (False,) * 9 + (True,))
        some = gcn_grad.nonlocal_backward(nw, X, st, G, bodies, False, (True, False, False, False, False, True, False, False, False, False))
    assert set(only_x) == {"x"} and torch.equal(only_x["x"], full["x"])
    assert set(only_beta) == {"W.1.bias"} and torch.equal(only_beta["W.1.bias"], full["W.1.bias"])
    assert set(some) == {"theta.weight", "g.bias"} and all(torch.equal(some[k], full[k]) for k in some)
