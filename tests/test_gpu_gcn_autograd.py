"""GPU (MI355X): the backward of the Modulated-GCN denoiser's graph convs (csrc/gcn_bwd.hip through egohmr_amd/gcn_grad.py, the three GEMMs on
ehm_conv_nhwc_split) and the autograd route of ModulatedGCN.forward, against float64 autograd through the oracle on the device.

Per conv the gate source handed to the kernels is the float32 rounding of the float64 forward's activation, so both sides share every ReLU gate by
construction and no case is left out.  End to end the forward is the module's own float32 one: the seed is chosen (on the CPU, see E2E_SEED) such that
every float64 pre-activation of every conv has |v| >= 1e-4 max|v| of that conv - twice the forward's bar of 5e-5 max - and the test asserts that
condition on the reference alone.

Bar: the project's bar for VJP kernels (tests/test_gpu_guidance.py, tests/test_gpu_smpl_autograd.py): atol = 2e-4 max|ref|, rtol = 2e-3 - a ceiling.
Every case prints the measured max|err| / max|ref| of every gradient."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VJP_ATOL_REL, VJP_RTOL = 2e-4, 2e-3
CANARY = 12345.0
PARAMS = ("W", "M", "adj2", "bias", "bn_weight", "bn_bias")
E2E_SEED = 52           # searched on the CPU with gate_margin() below over seeds 0..63: 12, 48 and 52 meet GATE_MARGIN (1.1e-4, 1.3e-4, 1.6e-4); the widest
GATE_MARGIN = 1e-4


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


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _syn_layer(g, K, N, dev, bn=True):
    """tests/test_gpu_gcn.py's synthetic layer."""
    ly = {"W": _t(g.normal(scale=0.55 / math.sqrt(K), size=(2, K, N)), dev), "M": _t(1 + g.normal(scale=0.15, size=(24, N)), dev),
          "adj2": _t(g.normal(scale=0.02, size=(24, 24)), dev), "bias": _t(g.normal(scale=0.05, size=N), dev)}
    if bn:
        ly.update(bn_weight=_t(g.uniform(0.8, 1.2, size=N), dev), bn_bias=_t(g.normal(scale=0.05, size=N), dev),
                  bn_mean=_t(g.normal(scale=0.1, size=N), dev), bn_var=_t(g.uniform(0.6, 1.4, size=N), dev))
    return ly


def _regime_layer(regime, g, K, N, dev, X, adj, bn=True):
    """The weight regimes of tests/test_gpu_gcn.py that matter to a backward: 'syn'; 'bn' = trained-like statistics (mean = the data's, var ~ 1e-3)
    with negative gammas; 'adj' = asymmetric adj2 of O(0.3); 'zero' = all-zero W."""
    from oracle import gcn as og
    ly = _syn_layer(g, K, N, dev, bn)
    if regime == "bn" and bn:
        ly["bn_var"] = _t(g.uniform(0.5e-3, 2e-3, size=N), dev)
        ly["bn_weight"] = _t(g.uniform(0.5, 1.5, size=N) * g.choice([-1.0, 1.0], size=N), dev)
        W = ly["W"].double()
        ly["bn_mean"] = og.mix(X @ W[0], X @ W[1], ly, adj).reshape(-1, N).mean(0).float()
    elif regime == "bn":                              # the output conv has no BatchNorm: modulation of both signs instead
        ly["M"] = _t(g.normal(scale=1.0, size=(24, N)), dev)
    elif regime == "adj":
        ly["adj2"] = _t(g.normal(scale=0.3, size=(24, 24)), dev)
    elif regime == "zero":
        ly["W"] = torch.zeros_like(ly["W"])
    return ly


def _create(dev, adj, inp, hidden, out, hid):
    from egohmr_amd import _lib
    keep = [adj]

    def params(ly, cin, cout):
        p = _lib.GConvParams()
        t = lambda v: keep.append(v.contiguous()) or keep[-1].data_ptr()
        p.W, p.M, p.adj2, p.bias = t(ly["W"]), t(ly["M"]), t(ly["adj2"]), t(ly["bias"])
        if ly.get("bn_weight") is not None:
            p.bn_weight, p.bn_bias, p.bn_mean, p.bn_var = t(ly["bn_weight"]), t(ly["bn_bias"]), t(ly["bn_mean"]), t(ly["bn_var"])
        p.in_dim, p.out_dim = cin, cout
        return p

    pin = params(inp, inp["W"].shape[1], hid)
    arr = (_lib.GConvParams * max(1, len(hidden)))(*[params(ly, hid, hid) for ly in hidden])
    pout = params(out, hid, 6)
    h = C.c_void_p()
    _lib.api().ehm_gcn_create(C.byref(h), adj, C.byref(pin), arr, len(hidden), C.byref(pout), hid, None)
    return _lib.Handle(h, _lib.api().ehm_gcn_destroy, keep)


def _check(tag, got, ref):
    """got / ref: dicts of tensors.  Prints max|err| / max|ref| of every gradient, then holds each to the bar."""
    line = []
    for k, r in ref.items():
        e = float((got[k].double() - r).abs().max())
        line.append(f"{k} {e / max(float(r.abs().max()), 1e-300):.1e}")
    print(f"{tag}: max|err|/max|ref|  " + "  ".join(line))
    for k, r in ref.items():
        np.testing.assert_allclose(got[k].double().cpu().numpy(), r.cpu().numpy(), atol=VJP_ATOL_REL * float(r.abs().max()), rtol=VJP_RTOL,
                                   err_msg=f"{tag}: {k}")


def _run_conv(dev, adj, kind, K, hid, bodies, regime, res, seed):
    """One conv of a handle, input-only and full, against float64 autograd through oracle.gcn.hidden_conv on the device."""
    from egohmr_amd import gcn_grad
    from oracle import gcn as og
    g = _rng(seed)
    N = 6 if kind == "output" else hid
    bn = kind != "output"
    rows = bodies * 24
    X = _t(g.normal(scale=0.7, size=(rows, K)), dev)
    X64 = X.double().view(bodies, 24, K)
    ly = _regime_layer(regime, g, K, N, dev, X64, adj, bn)
    other = lambda k, n, b: _syn_layer(g, k, n, dev, b)
    if kind == "input":
        h, conv = _create(dev, adj, ly, [], other(hid, 6, False), hid), gcn_grad.INPUT
    elif kind == "hidden":
        h, conv = _create(dev, adj, other(hid, hid, True), [other(hid, hid, True), ly], other(hid, 6, False), hid), 1
    else:
        h, conv = _create(dev, adj, other(hid, hid, True), [], ly, hid), gcn_grad.OUTPUT
    gout = _t(g.normal(size=(rows, N)), dev)
    R = _t(g.normal(scale=30.0, size=(rows, N)), dev) if res else None        # large against y: out - res would lose small gates
    # ---- float64 reference
    names = [k for k in PARAMS if k in ly]
    leaves = [X64.clone().requires_grad_()] + [ly[k].double().requires_grad_() for k in names]
    if res:
        leaves.append(R.double().view(bodies, 24, N).requires_grad_())
    ly64 = {**{k: v.double() for k, v in ly.items()}, **dict(zip(names, leaves[1:1 + len(names)]))}
    y = og.bn_relu(og.mix(leaves[0] @ ly64["W"][0], leaves[0] @ ly64["W"][1], ly64, adj), ly64)
    out = y + leaves[-1] if res else y
    grads = torch.autograd.grad(out, leaves, gout.double().view(bodies, 24, N))
    ref = dict(zip(["x"] + names, grads))
    ref["x"] = ref["x"].reshape(rows, K)
    if res:
        assert torch.equal(grads[-1].reshape(rows, N), gout.double())            # the residual's gradient is the cotangent itself
    gate = y.detach().float().reshape(rows, N).contiguous() if bn else None      # the float32 rounding of the float64 forward
    if bn:
        frac = float((gate > 0).float().mean())
        assert 0.02 < frac < 0.98, frac                                          # both gate values occur
    # ---- the kernels
    cw = gcn_grad.ConvWeights(ly["W"])
    Kp = (K + 31) // 32 * 32
    Xp = torch.zeros(rows, Kp, device=dev)
    Xp[:, :K] = X
    shapes = dict(W=(2, K, N), M=(24, N), adj2=(24, 24), bias=(N,), bn_weight=(N,), bn_bias=(N,))
    tag = f"{kind}[K={K} N={N} bodies={bodies} {regime} res={int(res)}]"

    def buffers():
        flat = {k: torch.full((int(np.prod(shapes[k])) + 64,), CANARY, device=dev) for k in names}
        return flat, {k: flat[k][:int(np.prod(shapes[k]))].view(shapes[k]) for k in names}

    # input only: nothing else is computed or written
    flat, outs = buffers()
    r = gcn_grad.conv_backward(h, conv, cw, Xp, gate, gout, bodies, need_x=True, need_w=False, need_params=False, has_bn=bn, out=outs)
    assert set(r) == {"x"}
    for k in names:
        assert bool((flat[k] == CANARY).all()), f"{tag}: {k} was written by an input-only backward"
    _check(tag + " input-only", r, {"x": ref["x"]})
    # full, twice: bit-equal parameter reductions, the canaries behind every output intact
    runs = []
    for _ in range(2):
        flat, outs = buffers()
        r = gcn_grad.conv_backward(h, conv, cw, Xp, gate, gout, bodies, need_x=True, need_w=True, need_params=True, has_bn=bn, out=outs)
        for k in names:
            n = int(np.prod(shapes[k]))
            assert bool((flat[k][n:] == CANARY).all()), f"{tag}: wrote behind {k}"
            assert r[k].data_ptr() == outs[k].data_ptr()
        runs.append({k: v.clone() for k, v in r.items()})
    for k in names:
        if k != "W":
            assert torch.equal(runs[0][k], runs[1][k]), f"{tag}: {k} differs between two calls"
    _check(tag + " full", runs[0], ref)
    torch.cuda.synchronize()
    h.close()


REGIMES = ("syn", "bn", "adj", "zero")


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("hid,bodies", [(64, 1), (192, 9), (320, 33), (1024, 9)])
def test_hidden_conv_backward_vs_fp64(dev, adj, hid, bodies, regime, res):
    _run_conv(dev, adj, "hidden", hid, hid, bodies, regime, res, seed=hid + bodies)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("hid,bodies", [(64, 1), (192, 9)])
def test_input_conv_backward_vs_fp64(dev, adj, hid, bodies, regime):
    """in_dim = 70: no multiple of the engine's 32-wide K tile nor of its 8-column output granule."""
    _run_conv(dev, adj, "input", 70, hid, bodies, regime, False, seed=7 + hid)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("hid,bodies", [(64, 1), (320, 33)])
def test_output_conv_backward_vs_fp64(dev, adj, hid, bodies, regime):
    """N = 6, no BatchNorm, no gate."""
    _run_conv(dev, adj, "output", hid, hid, bodies, regime, False, seed=3 + hid)


def test_entries_refuse_bad_arguments(dev, adj):
    from egohmr_amd import _lib, gcn_grad
    g = _rng(0)
    hid, bodies = 64, 2
    h = _create(dev, adj, _syn_layer(g, hid, hid, dev), [_syn_layer(g, hid, hid, dev)], _syn_layer(g, hid, 6, dev, False), hid)
    A = _lib.api()
    t = torch.zeros(bodies * 24, 2 * hid, device=dev)
    bad = [lambda: A.ehm_gcn_bwd_epilogue(h, 1, t, t, t, 2 * hid, bodies, None),                  # no such hidden conv
           lambda: A.ehm_gcn_bwd_epilogue(h, 0, t, None, t, 2 * hid, bodies, None),               # a conv with ReLU needs its gate
           lambda: A.ehm_gcn_bwd_epilogue(h, gcn_grad.OUTPUT, t, t, t, 32, bodies, None),         # the output conv has none
           lambda: A.ehm_gcn_bwd_epilogue(h, 0, t, t, torch.zeros_like(t), 2 * hid - 1, bodies, None),
           lambda: A.ehm_gcn_bwd_epilogue(h, 0, t, t, torch.zeros_like(t), 2 * hid, 0, None),
           lambda: A.ehm_gcn_bwd_params(h, 0, t, t, t, 2 * hid, bodies, t, t, t, t, t, t, 16, None)]   # workspace too small
    for f in bad:
        with pytest.raises(_lib.EgoHMRHipError) as e:
            f()
        assert e.value.rc == -22
    h.close()


# ---------------------------------------------------------------------------------------------- the module, end to end
def _module_state(seed, in_dim=70, hid=64, blocks=1):
    """A ModulatedGCN state dict with _syn_layer-like weights and the input x [2, 24, in_dim], as float64 CPU tensors."""
    g = _rng(seed)
    sd = {}

    def conv(p, K, N, bn):
        q = p + ".gconv" if bn else p
        sd[q + ".W"] = g.normal(scale=0.55 / math.sqrt(K), size=(2, K, N))
        sd[q + ".M"] = 1 + g.normal(scale=0.15, size=(24, N))
        sd[q + ".adj2"] = g.normal(scale=0.02, size=(24, 24))
        sd[q + ".bias"] = g.normal(scale=0.05, size=N)
        if bn:
            sd[p + ".bn.weight"] = g.uniform(0.8, 1.2, size=N) * g.choice([-1.0, 1.0], size=N)
            sd[p + ".bn.bias"] = g.normal(scale=0.05, size=N)
            sd[p + ".bn.running_mean"] = g.normal(scale=0.1, size=N)
            sd[p + ".bn.running_var"] = g.uniform(0.6, 1.4, size=N)

    conv("gconv_input.0", in_dim, hid, True)
    for b in range(blocks):
        conv(f"gconv_layers.{b}.gconv1", hid, hid, True)
        conv(f"gconv_layers.{b}.gconv2", hid, hid, True)
    conv("gconv_output", hid, 6, False)
    x = g.normal(scale=0.7, size=(2, 24, in_dim))
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).double()            # the float32 values the module holds, as float64
    return {k: f(v) for k, v in sd.items()}, f(x)


def _preactivations(sd, x, adj, blocks=1):
    """The float64 pre-activation (BatchNorm output in front of the ReLU; the output conv's result) of every conv."""
    from oracle import model as om
    vs = []

    def gc(p, t):
        v = om._bn(om.modulated_graph_conv(sd, p + ".gconv", t, adj).transpose(1, 2), sd, p + ".bn").transpose(1, 2)
        vs.append(v)
        return torch.relu(v)

    out = gc("gconv_input.0", x)
    for b in range(blocks):
        out = out + gc(f"gconv_layers.{b}.gconv2", gc(f"gconv_layers.{b}.gconv1", out))
    vs.append(om.modulated_graph_conv(sd, "gconv_output", out, adj))
    return vs


def gate_margin(seed):
    """min over the convs of min|v| / max|v| (float64, CPU): what the seed search maximises."""
    from oracle import model as om
    sd, x = _module_state(seed)
    return min(float(v.abs().min() / v.abs().max()) for v in _preactivations(sd, x, om.smpl_adjacency(torch.float64)))


@pytest.fixture(scope="module")
def module_case(dev):
    """The module with E2E_SEED's weights and the float64 reference gradients (computed once, shared, left unchanged)."""
    from egohmr_amd.model import ModulatedGCN, smpl_tree_adjacency
    from oracle import model as om
    sd, x = _module_state(E2E_SEED)
    adj64 = om.smpl_adjacency(torch.float64)
    margin = min(float(v.abs().min() / v.abs().max()) for v in _preactivations(sd, x, adj64))
    m = ModulatedGCN(smpl_tree_adjacency(), in_dim=70, hid_dim=64, num_layers=1)
    missing = m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    assert not missing.unexpected_keys and all("num_batches_tracked" in k for k in missing.missing_keys), missing
    m = m.to(dev).eval()
    cot = torch.from_numpy(_rng(99).normal(size=(2, 24, 6))).float().double()
    names = [k for k in sd if "running_" not in k]
    leaves = {k: sd[k].clone().requires_grad_() for k in names}
    xl = x.clone().requires_grad_()
    out = om.modulated_gcn({**sd, **leaves}, xl, adj64, p="", num_blocks=1)
    grads = torch.autograd.grad(out, [xl] + [leaves[k] for k in names], cot)
    ref = dict(zip(["x"] + names, grads))
    return dict(m=m, sd=sd, x=x, cot=cot, ref=ref, out=out.detach(), margin=margin, names=names)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_module_gradients_vs_fp64(dev, module_case, precision):
    c = module_case
    m = c["m"]
    print(f"gate margin of seed {E2E_SEED}: min|v|/max|v| = {c['margin']:.2e}")
    assert c["margin"] >= GATE_MARGIN
    m.precision, m.grad_params = precision, True
    try:
        m.zero_grad(set_to_none=True)
        x = c["x"].float().to(dev).requires_grad_()
        out = m(x)
        assert out.grad_fn is not None and out.shape == (2, 24, 6)
        scale = float(c["out"].abs().max())
        err = float((out.detach().double().cpu() - c["out"]).abs().max())
        print(f"autograd-route forward[{precision}] max|err| vs fp64 = {err:.2e} (|y|max {scale:.2f})")
        assert err < 5e-5 * max(1.0, scale)
        out.backward(c["cot"].float().to(dev))
        got = {"x": x.grad.cpu()}
        params = dict(m.named_parameters())
        for k in c["names"]:
            assert params[k].grad is not None, k
            got[k] = params[k].grad.cpu()
        _check(f"ModulatedGCN[{precision}]", got, c["ref"])
    finally:
        m.grad_params, m.precision = False, "f16x3"
        m.zero_grad(set_to_none=True)


def test_module_behaviour(dev, module_case):
    from egohmr_amd import _lib
    from egohmr_amd.model import ModulatedGCN, smpl_tree_adjacency
    m = module_case["m"]
    xs = module_case["x"].float().to(dev)
    m.zero_grad(set_to_none=True)
    before = m(xs)
    assert before.grad_fn is None and not before.requires_grad              # parameters require grad, grad mode is on: still today's route
    x = xs.clone().requires_grad_()
    m(x).sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    assert all(p.grad is None for p in m.parameters())
    after = m(xs)
    assert after.grad_fn is None and torch.equal(before, after)
    with torch.no_grad():
        assert m(x).grad_fn is None and torch.equal(m(x), before)
    # grad_params: every listed parameter, nothing else
    m.grad_params = True
    try:
        m(xs).sum().backward()                                              # x does not require grad: the parameters alone select the route
        listed = {id(p) for p in m.grad_parameters()}
        for n, p in m.named_parameters():
            assert (p.grad is not None) == (id(p) in listed), n
            assert p.grad is None or (p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all())), n
        # needs_input_grad decides: a frozen parameter gets nothing
        m.zero_grad(set_to_none=True)
        m.gconv_output.W.requires_grad_(False)
        m.gconv_layers[0].gconv1.bn.weight.requires_grad_(False)
        m(xs).sum().backward()
        assert m.gconv_output.W.grad is None and m.gconv_layers[0].gconv1.bn.weight.grad is None and m.gconv_output.M.grad is not None
        m.gconv_output.W.requires_grad_(True)
        m.gconv_layers[0].gconv1.bn.weight.requires_grad_(True)
        # the refusals
        m.precision = "f16"
        with pytest.raises(_lib.EgoHMRHipError, match="f16x3"):
            m(x)
        m.precision = "f16x3"
        m.train()
        with pytest.raises(NotImplementedError, match="inference only"):
            m(x)
        m.eval()
    finally:
        m.grad_params, m.precision = False, "f16x3"
        m.eval()
        m.zero_grad(set_to_none=True)
    assert torch.equal(m(xs), before)
    nl = ModulatedGCN(smpl_tree_adjacency(), in_dim=70, hid_dim=64, num_layers=1, nonlocal_layer=True).to(dev).eval()
    with pytest.raises(NotImplementedError, match="non-local"):
        nl(x)
    assert nl(xs).grad_fn is None


def test_in_place_update_rebuilds_the_packed_operands(dev, module_case):
    """Parameters updated in place between two calls: the one cached (handle, packed GEMM operands) pair is rebuilt - output and every gradient equal, bit
    for bit, those of a fresh module that loaded the updated weights, and so does the no-grad forward (its input GEMM reads the same packed operand)."""
    from egohmr_amd.model import ModulatedGCN, smpl_tree_adjacency
    xs, cot = module_case["x"].float().to(dev), module_case["cot"].float().to(dev)

    def make(sd):
        m = ModulatedGCN(smpl_tree_adjacency(), in_dim=70, hid_dim=64, num_layers=1)
        m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
        m.grad_params = True
        return m.to(dev).eval()

    def run(m):
        m.zero_grad(set_to_none=True)
        x = xs.clone().requires_grad_()
        out = m(x)
        out.backward(cot)
        return [out.detach(), x.grad] + [p.grad for p in m.grad_parameters()]

    old = make(module_case["sd"])
    before = run(old)
    with torch.no_grad():
        old.gconv_layers[0].gconv1.gconv.W.mul_(0.5)
        old.gconv_input[0].gconv.W.add_(0.01)
    got = run(old)
    assert not torch.equal(got[0], before[0])
    fresh = make(old.state_dict())
    want = run(fresh)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a is not None and torch.equal(a, b), i
    with torch.no_grad():
        assert torch.equal(fresh(xs), old(xs))
