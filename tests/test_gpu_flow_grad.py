"""GPU: the backward of the stage-1 flow (csrc/flow.hip, egohmr_amd/flow_grad.py) against float64.

Every compared tensor has its own error bar, the project's rule for free-running float32 chains: 8 x the largest distance of a float32 reference
run from the float64 run on the same inputs, floored at one float32 ulp of the tensor's largest magnitude (flow_grad_ref.bar_of).  The reference is
the float64 run; error / bar is printed per tensor.  The kernels are tested one by one with their mask and gate operands given as data (both sides
read the same float32 mask: no kink can flip), then end to end on inputs whose ReLU inputs keep clear of zero (test_flow_grad_cpu.py asserts that
on the references; it is asserted here again).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from egohmr_amd import synthetic as syn
from tests import flow_grad_ref as gr
from tests.test_flow_grad_cpu import B, FLAGS, MIN_SINE, S, SEEDS

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
H, D, HALF = 1024, 144, 72
CTX = 2566                                          # all flags on: 2 + 3 + 1 + 2048 + 512, the context width of the real first layer
ODD, EVEN = np.arange(1, 144, 2).astype(np.int32), np.arange(0, 144, 2).astype(np.int32)
_f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _sig(x):
    return 1 / (1 + np.exp(-x))


def _check(name, got, want, bar):
    got = np.asarray(got, np.float64)
    err = float(np.abs(got - want).max())
    print(f"{name}: error {err:.2e}, bar {bar:.2e}, error / bar {err / bar:.3f}")
    assert np.isfinite(got).all() and err <= bar, (name, err, bar)
    return err / bar


def _flow_on_device(sd, ctx, dev, bn=False):
    from egohmr_amd.stage1 import GlowFlow
    f = GlowFlow(ctx, batch_norm=bn)
    f.load_state_dict({k[len("flow.flow."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if bn or "batch_norm" not in k}, strict=True)
    return f.to(dev)


# --------------------------------------------------------------------------------------------- the flow before any autograd call
@pytest.fixture(scope="module")
def setup(dev):
    """The end-to-end case, its float64 / float32 references with gradients (computed once, never modified), and - FIRST, before anything of this
    module has taken the autograd route - the no-graph outputs of both directions."""
    ctx = syn.stage1_context_dim(**FLAGS)
    assert ctx == CTX
    sd = syn.make_stage1_flow_state_dict(10, **FLAGS)
    flow = _flow_on_device(sd, ctx, dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    k = dict(sd=sd, ctx=ctx, flow=flow, dev=dev)
    for sampling in (False, True):
        c, rows = gr.inputs(SEEDS[sampling], B, S, ctx)
        with torch.no_grad():
            before = flow.sample_and_log_prob(t(c), z=t(rows)) if sampling else flow.log_prob(t(rows), t(c))
        g = np.random.Generator(np.random.PCG64(50 + sampling))
        shapes = [(B * S, 144), (B * S,), (B * S, 24, 3, 3)] if sampling else [(B * S,), (B * S, 144)]
        cots = [_f32(g.normal(size=s)) for s in shapes]
        r64, r32 = (gr.run(sd, c, rows, S, sampling, dt, cots) for dt in (torch.float64, torch.float32))
        k[sampling] = dict(c=c, rows=rows, before=before, cots=cots, r64=r64, r32=r32)
    return k


# --------------------------------------------------------------------------------------------- 1. the new modes of ehm_flow_gemm
# (K, N, ldw, gather, gate prologue, epilogue, scatter): the backward's data-gradient products at their real sizes
GEMM_CASES = {
    "last_layer_bwd": (72, 1024, 1024, True, False, "bias", False),            # dt_2 = ds[:, trf] Wf^T: the gather of the forward, W in torch layout
    "hidden_gate_mask": (1024, 1024, 1024, False, True, "mask", False),        # du1 = ((dt sigma) Wb^T) [u1 > 0]
    "hidden_mask_add": (1024, 1024, 1024, False, False, "mask_add", False),    # dt_k = dt_k+1 + (du1 Wa^T) [t_k > 0], in place
    "first_layer_bwd_add": (1024, 72, 72 + CTX, False, False, "scatter_add", True),   # ds[:, idf] += dt_0 Wx^T, W a window of [1024, 72 + ctx]
    "first_layer_bwd_sub": (1024, 72, 72 + CTX, False, False, "scatter_sub", True),
    "affine_bwd": (144, 144, 144, False, False, "bias", False),                # ds A, ldw = 144
    "context_sum": (1024, CTX, CTX, False, False, "add", False),               # dctx += dP_slot Wc, N = ctx, ldw = ctx
}
EPI = {"bias": 0, "scatter_add": 3, "scatter_sub": 4, "mask": 5, "mask_add": 6, "add": 7}


def _gemm_ref(X, W, dtype, gather, gate, S, epi, mask, add, scatter, Y):
    f = lambda a: np.asarray(a, dtype)
    A = f(X)[:, gather] if gather is not None else f(X)
    if gate is not None:
        A = A * _sig(f(gate))[np.arange(X.shape[0]) // S]
    v = A @ f(W)
    if epi == "bias":
        return v
    if epi == "mask":
        return v * (mask > 0)
    if epi == "mask_add":
        return f(add) + v * (mask > 0)
    if epi == "add":
        return f(add) + v
    out = np.array(Y, dtype)
    out[:, scatter] += v if epi == "scatter_add" else -v
    return out


@pytest.mark.parametrize("S_", [1, 5])
@pytest.mark.parametrize("case", list(GEMM_CASES))
def test_new_gemm_modes_match_float64(dev, case, S_):
    from egohmr_amd import _lib
    K, N, ldw, gather, gate, epi, scatter = GEMM_CASES[case]
    g = np.random.Generator(np.random.PCG64(sum(map(ord, case)) + S_))
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    W = _f32(g.normal(scale=1 / np.sqrt(K), size=(K, ldw)))          # (the columns behind N are live data of a wider matrix: they must not matter)
    idx_in, idx_out = (ODD if gather else None), (EVEN if scatter else None)
    ldx = 144 if gather else K
    ldy = 144 if scatter else N + 8
    Wd, gi, si = t(W), t(idx_in), t(idx_out)
    worst = 0.0
    for R in (1, 31, 33, 65):
        guard = 3
        X = _f32(g.normal(size=(R + guard, ldx)))
        X[R:] = np.nan
        item = _f32(g.normal(size=(-(-R // S_), K + 32))) if gate else None
        mask = _f32(g.normal(size=(R, N + 4))) if epi in ("mask", "mask_add") else None
        in_place = epi in ("mask_add", "add", "scatter_add", "scatter_sub")
        Y0 = _f32(g.normal(size=(R + guard, ldy))) if in_place else np.full((R + guard, ldy), SENTINEL, np.float32)
        Y0[R:] = SENTINEL
        Xd, Yd, itd, md = t(X), t(Y0.copy()), t(item), t(mask)
        d = _lib.FlowGemmDesc(X=_lib.ptr(Xd), gather=_lib.ptr(gi), W=_lib.ptr(Wd), item=_lib.ptr(itd), scatter=_lib.ptr(si), Y=_lib.ptr(Yd), R=R, K=K,
                              N=N, S=S_, ldx=ldx, ldw=ldw, ldy=ldy, ld_item=K + 32 if gate else 0, prologue=4 if gate else 0, epilogue=EPI[epi],
                              mask=_lib.ptr(md), ld_mask=N + 4 if mask is not None else 0, add=_lib.ptr(Yd) if epi in ("mask_add", "add") else None,
                              ld_add=ldy if epi in ("mask_add", "add") else 0, w_window=int(ldw % 32 != 0))
        _lib.api().ehm_flow_gemm(C.byref(d), _lib.stream_ptr())
        torch.cuda.synchronize()
        got = Yd.cpu().numpy()
        kw = dict(gather=idx_in, gate=None if item is None else item[:, :K], S=S_, epi=epi, mask=None if mask is None else mask[:, :N],
                  add=Y0[:R, :N], scatter=idx_out, Y=Y0[:R])
        want = _gemm_ref(X[:R], W[:, :N], np.float64, **kw)
        bar = gr.bar_of(_gemm_ref(X[:R], W[:, :N], np.float32, **kw), want)
        worst = max(worst, _check(f"{case} S = {S_} R = {R}", got[:R] if scatter else got[:R, :N], want, bar))
        assert np.array_equal(got[R:], Y0[R:]), "rows >= R were written"
        if scatter:
            assert np.array_equal(got[:R, 1::2], Y0[:R, 1::2]), "columns outside the scatter list were written"
        else:
            assert np.array_equal(got[:R, N:], Y0[:R, N:]), "columns >= N were written"
    print(f"{case} S = {S_}: largest error / bar {worst:.3f}")


def test_glu_with_a_kept_input_gives_the_in_place_bits_and_the_value_half(dev):
    from egohmr_amd import _lib
    g = np.random.Generator(np.random.PCG64(3))
    R, S_ = 33, 5
    t = lambda a: torch.from_numpy(_f32(a)).to(dev)
    X, W, bias, item, T = t(g.normal(size=(R, H))), t(g.normal(scale=1 / 32, size=(H, H))), t(g.normal(size=H)), t(g.normal(size=(7, H))), t(g.normal(size=(R, H)))
    base = dict(X=_lib.ptr(X), W=_lib.ptr(W), bias=_lib.ptr(bias), item=_lib.ptr(item), R=R, K=H, N=H, S=S_, ldx=H, ldw=H, ldy=H, ld_item=H, prologue=1,
                epilogue=2)
    Y1, Y2, aux = T.clone(), torch.full_like(T, SENTINEL), torch.full_like(T, SENTINEL)
    _lib.api().ehm_flow_gemm(C.byref(_lib.FlowGemmDesc(Y=_lib.ptr(Y1), **base)), _lib.stream_ptr())
    _lib.api().ehm_flow_gemm(C.byref(_lib.FlowGemmDesc(Y=_lib.ptr(Y2), add=_lib.ptr(T), ld_add=H, aux=_lib.ptr(aux), **base)), _lib.stream_ptr())
    assert torch.equal(Y1, Y2)
    u2 = torch.empty_like(T)
    _lib.api().ehm_flow_gemm(C.byref(_lib.FlowGemmDesc(Y=_lib.ptr(u2), **{**base, "epilogue": 0, "item": None})), _lib.stream_ptr())
    assert torch.equal(aux, u2)


# --------------------------------------------------------------------------------------------- 2. ehm_flow_wgrad and the reductions
# (Cg, Ca, gather on G, gather on X, gate, relu, x_shift, alpha, columns of the output matrix in front of / behind the window)
WGRAD_CASES = {
    "hidden_gate_relu": (1024, 1024, False, False, True, True, False, 1.0, 0, 0),      # dWb = (dt sigma)^T relu(u1)
    "last_layer": (72, 1024, True, False, False, False, False, -1.0, 0, 0),            # dWf = -ds[:, trf]^T t_2 (the sampling side's sign)
    "first_layer_window": (1024, 72, False, True, False, False, False, 1.0, 0, 19),    # dWx into columns 0 .. 71 of a wider gradient
    "affine_inverse": (144, 144, False, False, False, False, True, 1.0, 5, 3),         # dAinv = dx^T (s - c), inside a window
}


def _wgrad_ref(G, X, dtype, gg, gx, gate, S, relu, shift, alpha):
    f = lambda a: np.asarray(a, dtype)
    Gm = f(G)[:, gg] if gg is not None else f(G)
    if gate is not None:
        Gm = Gm * _sig(f(gate))[np.arange(G.shape[0]) // S]
    Xm = f(X)[:, gx] if gx is not None else f(X)
    if shift is not None:
        Xm = Xm - f(shift)
    if relu:
        Xm = np.maximum(Xm, 0)
    return dtype(alpha) * (Gm.T @ Xm)


def _run_wgrad(dev, G, X, out0, col0, Cg, Ca, S_, gg=None, gx=None, gate=None, relu=False, shift=None, alpha=1.0, beta=0.0):
    from egohmr_amd import _lib
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    Gd, Xd, od, ggd, gxd, gd, sd_ = t(G), t(X), t(out0.copy()), t(gg), t(gx), t(gate), t(shift)
    d = _lib.FlowWgradDesc(G=_lib.ptr(Gd), gather_g=_lib.ptr(ggd), item=_lib.ptr(gd), X=_lib.ptr(Xd), gather_x=_lib.ptr(gxd), x_shift=_lib.ptr(sd_),
                           out=od.data_ptr() + 4 * col0, R=G.shape[0], Cg=Cg, Ca=Ca, S=S_, ldg=G.shape[1], ldx=X.shape[1],
                           ld_item=0 if gate is None else gate.shape[1], ld_out=out0.shape[1], act=int(relu), alpha=alpha, beta=beta)
    _lib.api().ehm_flow_wgrad(C.byref(d), _lib.stream_ptr())
    torch.cuda.synchronize()
    return od.cpu().numpy()


@pytest.mark.parametrize("case", list(WGRAD_CASES))
def test_wgrad_matches_float64(dev, case):
    Cg, Ca, use_gg, use_gx, use_gate, relu, use_shift, alpha, front, behind = WGRAD_CASES[case]
    g = np.random.Generator(np.random.PCG64(sum(map(ord, case))))
    worst = 0.0
    for R, S_ in ((1, 1), (33, 1), (33, 5), (70, 5), (70, 1)):
        G = _f32(g.normal(size=(R, 144 if use_gg else Cg + 4)))
        X = _f32(g.normal(size=(R, 144 if use_gx else Ca + 4)))
        gate = _f32(g.normal(size=(-(-R // S_), Cg + 8))) if use_gate else None
        shift = _f32(g.normal(size=Ca)) if use_shift else None
        gg, gx = (ODD if use_gg else None), (EVEN if use_gx else None)
        out0 = np.full((Cg, front + Ca + behind), SENTINEL, np.float32)
        got = _run_wgrad(dev, G, X, out0, front, Cg, Ca, S_, gg, gx, gate, relu, shift, alpha)
        kw = dict(gg=gg, gx=gx, gate=None if gate is None else gate[:, :Cg], S=S_, relu=relu, shift=shift, alpha=alpha)
        Gl, Xl = (G if use_gg else G[:, :Cg]), (X if use_gx else X[:, :Ca])
        want = _wgrad_ref(Gl, Xl, np.float64, **kw)
        bar = gr.bar_of(_wgrad_ref(Gl, Xl, np.float32, **kw), want)
        worst = max(worst, _check(f"wgrad {case} R = {R} S = {S_}", got[:, front:front + Ca], want, bar))
        assert (got[:, :front] == SENTINEL).all() and (got[:, front + Ca:] == SENTINEL).all(), "columns outside the window were written"
    print(f"wgrad {case}: largest error / bar {worst:.3f}")


@pytest.mark.parametrize("beta", [1.0, -0.5])
def test_wgrad_adds_to_a_gradient_buffer_with_beta(dev, beta):
    """out <- alpha G^T X + beta out, into a column window of a wider matrix whose other columns are sentinels (R = 33: a partial 16-row step)."""
    g = np.random.Generator(np.random.PCG64(61))
    R, Cg, Ca, front, behind, alpha = 33, 144, 72, 3, 6, -1.0
    G, X = _f32(g.normal(size=(R, Cg))), _f32(g.normal(size=(R, Ca + 4)))
    out0 = np.full((Cg, front + Ca + behind), SENTINEL, np.float32)
    out0[:, front:front + Ca] = g.normal(scale=3.0, size=(Cg, Ca))
    got = _run_wgrad(dev, G, X, out0, front, Cg, Ca, 1, alpha=alpha, beta=beta)
    ref = lambda dt: dt(alpha) * (G.astype(dt).T @ X[:, :Ca].astype(dt)) + dt(beta) * out0[:, front:front + Ca].astype(dt)
    _check(f"wgrad beta = {beta}", got[:, front:front + Ca], ref(np.float64), gr.bar_of(ref(np.float32), ref(np.float64)))
    assert (got[:, :front] == SENTINEL).all() and (got[:, front + Ca:] == SENTINEL).all(), "columns outside the window were written"


@pytest.mark.parametrize("Bn", [1, 3])
def test_context_weight_gradient_matches_float64(dev, Bn):
    """dWctx = dP^T ctx_pad, [12 * 1024, ctx_pad] over the B items, in one call."""
    g = np.random.Generator(np.random.PCG64(20 + Bn))
    dP, cp = _f32(g.normal(size=(Bn, 12 * H))), _f32(g.normal(size=(Bn, 2592)))
    out0 = np.full((12 * H, 2592 + 2), SENTINEL, np.float32)
    got = _run_wgrad(dev, dP, cp, out0, 0, 12 * H, 2592, 1)
    want = dP.astype(np.float64).T @ cp.astype(np.float64)
    _check(f"wgrad context B = {Bn}", got[:, :2592], want, gr.bar_of(dP.T @ cp, want))
    assert (got[:, 2592:] == SENTINEL).all()


def _run_reduce(dev, mode, G, out0, N, S_, gather=None, U2=None, item=None, scale=1.0):
    from egohmr_amd import _lib
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    Gd, od, gd, ud, itd = t(G), t(out0.copy()), t(gather), t(U2), t(item)
    d = _lib.FlowReduceDesc(G=_lib.ptr(Gd), gather=_lib.ptr(gd), U2=_lib.ptr(ud), item=_lib.ptr(itd), out=_lib.ptr(od), R=G.shape[0], N=N, S=S_,
                            ldg=G.shape[1], ldu=0 if U2 is None else U2.shape[1], ld_item=0 if item is None else item.shape[1],
                            ld_out=out0.shape[-1], mode=mode, scale=scale)
    _lib.api().ehm_flow_reduce(C.byref(d), _lib.stream_ptr())
    torch.cuda.synchronize()
    return od.cpu().numpy()


def test_reductions_match_float64(dev):
    g = np.random.Generator(np.random.PCG64(31))
    worst = 0.0
    for R, S_ in ((1, 1), (33, 1), (33, 5), (70, 5)):
        items = -(-R // S_)
        it_of = np.arange(R) // S_
        G, U2, item = _f32(g.normal(size=(R, H + 4))), _f32(g.normal(size=(R, H + 8))), _f32(g.normal(size=(items, H + 12)))
        ds = _f32(g.normal(size=(R, 144)))
        for dt in (np.float64, np.float32):
            f = lambda a: np.asarray(a, dt)
            sg = _sig(f(item[:, :H]))
            ref = dict(cols=f(G[:, :H]).sum(0), cols_gather=-f(ds)[:, ODD].sum(0), cols_gate=(f(G[:, :H]) * sg[it_of]).sum(0),
                       item=np.stack([f(G[it_of == i, :H]).sum(0) for i in range(items)]),
                       gate=-np.stack([(f(G[it_of == i, :H]) * f(U2[it_of == i, :H])).sum(0) * (sg[i] * (1 - sg[i])) for i in range(items)]))
            if dt == np.float64:
                want = ref
        flat, wide = np.full(H + 3, SENTINEL, np.float32), np.full((items + 1, H + 5), SENTINEL, np.float32)
        got = dict(cols=_run_reduce(dev, 0, G, flat, H, S_), cols_gather=_run_reduce(dev, 0, ds, flat, HALF, 1, gather=ODD, scale=-1.0),
                   cols_gate=_run_reduce(dev, 0, G, flat, H, S_, item=item), item=_run_reduce(dev, 1, G, wide, H, S_),
                   gate=_run_reduce(dev, 2, G, wide, H, S_, U2=U2, item=item, scale=-1.0))
        for name in want:
            n = HALF if name == "cols_gather" else H
            live = got[name][:n] if got[name].ndim == 1 else got[name][:items, :n]
            worst = max(worst, _check(f"reduce {name} R = {R} S = {S_}", live, want[name], gr.bar_of(ref[name], want[name])))
            rest = got[name][n:] if got[name].ndim == 1 else np.concatenate([got[name][items:].ravel(), got[name][:items, n:].ravel()])
            assert (rest == SENTINEL).all(), f"{name}: written outside its output"
    print(f"reductions: largest error / bar {worst:.3f}")


# --------------------------------------------------------------------------------------------- 3. ehm_flow_finish_backward
def test_finish_backward_matches_float64(dev, setup):
    from egohmr_amd import _lib
    g = np.random.Generator(np.random.PCG64(41))
    x64 = setup[True]["r64"]["out"][0]                                # the float64 reference's samples of the end-to-end case: [R,144]
    assert gr.sines(x64).min() >= MIN_SINE
    R = x64.shape[0]
    pose, g6, ggo, gbp, glp, z, gz = (_f32(a) for a in (x64, g.normal(size=(R, 144)), g.normal(size=(R, 9)), g.normal(size=(R, 23 * 9)),
                                                        g.normal(size=R), g.normal(size=(R, 144)), g.normal(size=(R, 144))))
    t = lambda a: torch.from_numpy(a).to(dev)
    dpose, dz, ssum = torch.empty(R, 144, device=dev), torch.empty(R, 144, device=dev), torch.empty(1, device=dev)
    _lib.api().ehm_flow_finish_backward(t(glp), t(z), t(gz), dz, ssum, t(pose), t(g6), t(ggo), t(gbp), dpose, R, _lib.stream_ptr())
    dz_only = torch.empty(R, 144, device=dev)
    _lib.api().ehm_flow_finish_backward(t(glp), t(z), None, dz_only, None, None, None, None, None, None, R, _lib.stream_ptr())
    torch.cuda.synchronize()
    gR = np.concatenate([ggo.reshape(R, 1, 3, 3), gbp.reshape(R, 23, 3, 3)], 1)
    ref = {}
    for dt in (torch.float64, torch.float32):
        p = torch.tensor(pose, dtype=dt, requires_grad=True)
        (gr.rot6d_prohmr(p).reshape(R, 24, 3, 3) * torch.tensor(gR, dtype=dt)).sum().backward()
        ref[dt] = p.grad.numpy() + g6.astype(np.float64 if dt == torch.float64 else np.float32)
    _check("finish backward: dpose", dpose.cpu().numpy(), ref[torch.float64], gr.bar_of(ref[torch.float32], ref[torch.float64]))
    # dz = -dlp z: exact to one rounding (alone), one fmaf with the incoming cotangent
    assert np.array_equal(dz_only.cpu().numpy(), -glp[:, None] * z)
    exact = gz.astype(np.float64) - glp[:, None].astype(np.float64) * z.astype(np.float64)
    assert np.array_equal(dz.cpu().numpy(), exact.astype(np.float32))
    _check("finish backward: sum of dlp", ssum.cpu().numpy(), glp.astype(np.float64).sum(), gr.bar_of(glp.sum(dtype=np.float32), glp.astype(np.float64).sum()))


# --------------------------------------------------------------------------------------------- 4. end to end
def _device_run(k, sampling, rows_grad=True, ctx_grad=True, params=True):
    flow, dev = k["flow"], k["dev"]
    e = k[sampling]
    t = lambda a: torch.from_numpy(a).to(dev)
    flow.grad_params = params
    flow.zero_grad(set_to_none=True)
    c, rows = t(e["c"]).requires_grad_(ctx_grad), t(e["rows"]).requires_grad_(rows_grad)
    if sampling:
        o = flow.sample_and_log_prob(c, z=rows)
        out = (o["pred_pose_6d"], o["log_prob"], o["global_orient"], o["body_pose"])
        rc = e["cots"][2].reshape(B, S, 24, 3, 3)
        cots = (e["cots"][0].reshape(B, S, 144), e["cots"][1].reshape(B, S), rc[:, :, :1], rc[:, :, 1:])
    else:
        out = flow.log_prob(rows, c)
        cots = (e["cots"][0].reshape(B, S), e["cots"][1].reshape(B, S, 144))
    torch.autograd.backward(out, [t(np.ascontiguousarray(a)) for a in cots])
    torch.cuda.synchronize()
    flow.grad_params = False
    grads = {"flow.flow." + n: (None if p.grad is None else p.grad.detach().clone()) for n, p in flow.named_parameters()}
    grads["rows"], grads["ctx"] = (None if rows.grad is None else rows.grad.reshape(-1, 144)), c.grad
    return out, grads


@pytest.mark.parametrize("sampling", [False, True], ids=["log_prob", "sampling"])
def test_end_to_end_gradients_match_float64(setup, sampling):
    e = setup[sampling]
    r64, r32 = e["r64"], e["r32"]
    margin = gr.relu_margin(r64, r32)
    print(f"kink condition: min |v| / bar = {margin:.2f}")
    assert margin > 1.0
    if sampling:
        assert gr.sines(r64["out"][0]).min() >= MIN_SINE
    out, grads = _device_run(setup, sampling)
    # the autograd route's forward: the no-graph route's bits, and a grad_fn
    before = e["before"]
    before = (before["pred_pose_6d"], before["log_prob"], before["global_orient"], before["body_pose"]) if sampling else before
    for a, b in zip(out, before):
        assert a.grad_fn is not None and b.grad_fn is None and torch.equal(a.detach(), b)
    assert type(out[0].grad_fn).__name__.startswith("FlowSampleFunction" if sampling else "FlowFunction")
    groups = {}
    for name, want in r64["grads"].items():
        assert want is not None and grads[name] is not None, name
        ratio = _check(f"d {name}", grads[name].cpu().numpy().reshape(want.shape), want, gr.bar_of(r32["grads"][name], want))
        kind = name if name in ("rows", "ctx") else ("affine" if ".transform_net." not in name else "net")
        groups[kind] = max(groups.get(kind, 0.0), ratio)
    print(f"{'sampling' if sampling else 'log_prob'}: largest error / bar per group: " + ", ".join(f"{a} {b:.3f}" for a, b in groups.items()))


# --------------------------------------------------------------------------------------------- 5. determinism, needs_input_grad
@pytest.mark.parametrize("sampling", [False, True], ids=["log_prob", "sampling"])
def test_backward_is_deterministic_and_computes_what_is_asked(setup, sampling):
    _, g1 = _device_run(setup, sampling)
    _, g2 = _device_run(setup, sampling)
    for name in g1:
        assert torch.equal(g1[name], g2[name]), name
    _, gp = _device_run(setup, sampling, rows_grad=False, ctx_grad=False, params=True)           # parameters only
    assert gp["ctx"] is None and gp["rows"] is None
    for name in g1:
        if name not in ("rows", "ctx"):
            assert torch.equal(gp[name], g1[name]), name
    _, gc = _device_run(setup, sampling, rows_grad=False, ctx_grad=True, params=False)           # the context only
    assert torch.equal(gc["ctx"], g1["ctx"]) and gc["rows"] is None
    assert all(v is None for n, v in gc.items() if n not in ("rows", "ctx"))


@pytest.mark.parametrize("sampling", [False, True], ids=["log_prob", "sampling"])
def test_launches_follow_what_is_asked(setup, sampling, monkeypatch):
    """Counted launches: frozen parameters (requires_grad False under grad_params = True, and grad_params = False) launch no weight-gradient
    product and no reduction for a bias; a context that does not require grad launches no dP Wctx^T (the twelve N = ctx products)."""
    from egohmr_amd import flow_grad as fg
    flow = setup["flow"]
    calls = {"wgrad": 0, "cols": 0, "ctx_gemm": 0}
    wgrad, reduce_, gemm = fg._wgrad, fg._reduce, flow._gemm

    def count_wgrad(*a, **k):
        calls["wgrad"] += 1
        return wgrad(*a, **k)

    def count_reduce(st, mode, *a, **k):
        calls["cols"] += mode == 0
        return reduce_(st, mode, *a, **k)

    def count_gemm(st, X, W, Y, R, K, N, *a, **k):
        calls["ctx_gemm"] += N == CTX
        return gemm(st, X, W, Y, R, K, N, *a, **k)

    monkeypatch.setattr(fg, "_wgrad", count_wgrad)
    monkeypatch.setattr(fg, "_reduce", count_reduce)
    monkeypatch.setattr(flow, "_gemm", count_gemm)
    zero = lambda: calls.update(wgrad=0, cols=0, ctx_gemm=0)
    _, full = _device_run(setup, sampling)                                                       # everything asked for
    assert calls == {"wgrad": 4 * (6 + 1) + 12, "cols": 4 * (5 + 1) + 1, "ctx_gemm": 12}
    zero()
    _device_run(setup, sampling, rows_grad=True, ctx_grad=True, params=False)                    # grad_params = False
    assert calls == {"wgrad": 0, "cols": 0, "ctx_gemm": 12}
    zero()
    flow.requires_grad_(False)                                                                   # frozen parameters, grad_params = True
    try:
        _, frozen = _device_run(setup, sampling, rows_grad=True, ctx_grad=True, params=True)
    finally:
        flow.requires_grad_(True)
    assert calls == {"wgrad": 0, "cols": 0, "ctx_gemm": 12}
    assert torch.equal(frozen["rows"], full["rows"]) and torch.equal(frozen["ctx"], full["ctx"])
    assert all(v is None for n, v in frozen.items() if n not in ("rows", "ctx"))
    zero()
    _, gp = _device_run(setup, sampling, rows_grad=True, ctx_grad=False, params=True)            # the context does not require grad
    assert calls["ctx_gemm"] == 0 and calls["wgrad"] == 4 * (6 + 1) + 12 and gp["ctx"] is None
    zero()
    _device_run(setup, sampling, rows_grad=True, ctx_grad=False, params=False)                   # the rows alone: no per-item term at all
    assert calls == {"wgrad": 0, "cols": 0, "ctx_gemm": 0}


def test_a_parameter_changed_between_forward_and_backward_raises(setup):
    from egohmr_amd import _lib
    dev, e = setup["dev"], setup[False]
    flow = _flow_on_device(setup["sd"], setup["ctx"], dev)
    flow.grad_params = True
    lp, _ = flow.log_prob(torch.from_numpy(e["rows"]).to(dev), torch.from_numpy(e["c"]).to(dev))
    with torch.no_grad():
        next(flow.parameters()).mul_(1.0)                          # (an in-place update: the values stay, the version moves)
    with pytest.raises(_lib.EgoHMRHipError, match="modified .* between a forward and its backward"):
        lp.sum().backward()


# --------------------------------------------------------------------------------------------- 6. an optimizer's steps
def test_adamw_steps_lower_the_nll_and_the_weight_cache_follows(setup):
    dev, sd, ctx = setup["dev"], setup["sd"], setup["ctx"]
    flow = _flow_on_device(sd, ctx, dev)
    flow.grad_params = True
    e = setup[False]
    c, x = torch.from_numpy(e["c"]).to(dev), torch.from_numpy(e["rows"]).to(dev)
    opt = torch.optim.AdamW(flow.parameters(), lr=1e-4)
    fresh = _flow_on_device(sd, ctx, dev)
    losses = []
    for step in range(10):
        opt.zero_grad(set_to_none=True)
        loss = -flow.log_prob(x, c)[0].mean()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
        with torch.no_grad():                                        # the cache saw the in-place update: a fresh module on the new weights agrees
            lp = flow.log_prob(x, c)[0]
        fresh.load_state_dict(flow.state_dict(), strict=True)        # (copy_ into the fresh module's own tensors: ITS cache has to follow too)
        assert torch.equal(lp, fresh.log_prob(x, c)[0]), step
        if step in (0, 9):                                           # and a module built from scratch on the updated state dict
            scratch = _flow_on_device({"flow.flow." + k: v.detach().cpu().numpy() for k, v in flow.state_dict().items()}, ctx, dev)
            assert torch.equal(lp, scratch.log_prob(x, c)[0]), step
    with torch.no_grad():
        losses.append(float(-flow.log_prob(x, c)[0].mean()))
    print("NLL over ten AdamW steps: " + " ".join(f"{v:.4f}" for v in losses))
    assert losses[-1] < losses[0] and all(np.isfinite(losses))


# --------------------------------------------------------------------------------------------- 7. refusals, unchanged routes
def test_refusals_and_the_no_graph_routes(setup):
    from egohmr_amd import _lib
    dev, flow = setup["dev"], setup["flow"]
    t = lambda a: torch.from_numpy(a).to(dev)
    for sampling in (False, True):
        e = setup[sampling]
        c, rows = t(e["c"]).requires_grad_(True), t(e["rows"]).requires_grad_(True)
        with torch.no_grad():                                        # after the autograd calls of the tests above: the bits of the call before them
            now = flow.sample_and_log_prob(c, z=rows) if sampling else flow.log_prob(rows, c)
        pairs = [(now[n], e["before"][n]) for n in ("pred_pose_6d", "log_prob", "global_orient", "body_pose")] if sampling else list(zip(now, e["before"]))
        for a, b in pairs:
            assert a.grad_fn is None and not a.requires_grad and torch.equal(a, b)
        out = flow.log_prob(t(e["rows"]), t(e["c"]))                 # grad mode on, nothing requires grad, grad_params = False
        assert out[0].grad_fn is None
    bn = _flow_on_device(syn.make_stage1_flow_state_dict(10, batch_norm=True, **FLAGS), setup["ctx"], dev, bn=True)
    e = setup[False]
    with pytest.raises(_lib.EgoHMRHipError, match="BatchNorm of the flow's ResidualNet is not differentiated"):
        bn.log_prob(t(e["rows"]).requires_grad_(True), t(e["c"]))
    assert bn.log_prob(t(e["rows"]), t(e["c"]))[0].grad_fn is None     # (its no-graph route is untouched)
    with pytest.raises(_lib.EgoHMRHipError, match="CPU tensor"):
        flow.log_prob(torch.from_numpy(e["rows"]).requires_grad_(True), t(e["c"]))
    with pytest.raises(_lib.EgoHMRHipError, match="CPU tensor"):
        flow.sample_and_log_prob(t(e["c"]), z=torch.from_numpy(e["rows"]).requires_grad_(True))
