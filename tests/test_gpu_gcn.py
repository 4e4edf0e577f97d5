"""GPU (MI355X): the Modulated-GCN denoiser's kernels (csrc/gcn.hip, csrc/gcn_tile.hip, csrc/gcn_dev.h and their copies inside the fused step
launches) against the float64 references of oracle.gcn, computed on the device from the values the kernels actually see: activations are the
packed operands unpacked with ehm_gcn_unpack_activations (exact), weights are the float32 parameters promoted to float64.

Error model.  It extends the one of tests/test_gpu_linear.py; every bound below is derived from it, none is fitted to an observed error.
Let u = 2^-24, X the conv's input [rows, K], W_k its two branch weights (k = 0 diagonal, 1 neighbour), h_k = X W_k, s the layer's power-of-two
weight scale (csrc/gcn.hip pack_layer: |W| s < 4096 from the layer's absmax; 1 for an all-zero layer), R_k = sqrt((X^2) (W_k^2)^T) the random-walk
scale of the K products and |X|_1 the row's absolute sum.

GEMM part, per tier (bound E_k on |h_k - X W_k|):
  * f32: the f32-input MFMA is a k-ordered fma chain (exact products, K roundings of partial sums of scale R_k + |h_k|):
        E = 4 sqrt(K) u (R + |h|)
  * f16x3 (split-f16): the activation operand is exact (X2 rows are hi + lo); W s is split into hi + lo: 2^-22 |w| per weight plus the
    subnormal floor 2^-25 / s of the lo half (an outlier weight makes s small enough to push every other weight's lo half there); the dropped
    al.wl term and both splits as in test_gpu_linear, 3 roundings per product in f32 accumulation:
        E = 8 2^-20 R + 2^-22 sqrt(3K) (R + |h|) + 2^-25 |X|_1 / s
  * f16: activations exact f16, W s rounded once to f16 (2^-11 |w| + 2^-25 / s):
        E = 4 2^-11 R + 2^-22 sqrt(K) (R + |h|) + 2^-25 |X|_1 / s
Epilogue, per output (joint j, channel n) with the BatchNorm factor c_n = gamma_n / sqrt(var_n + eps) (1 without BatchNorm), A the symmetrised
adjacency and the magnitude of the mix  mag = |c_n| (|A_jj M_jn h0_jn| + sum_{j' != j} |A_jj' M_j'n h1_j'n|):
  * the GEMM errors through modulation and the 24-term mix:  |c_n| (|A_jj M_jn| E0_jn + sum_{j' != j} |A_jj' M_j'n| E1_j'n)
  * the f32 epilogue: the folded coefficients D = A_jj M c, M1 = M c (at most 7 roundings each), the folded shift (bias - mean) c + beta
    (6 roundings through c), the fma(D, h0, shift), the product M1 h1 and the 23-step fma chain of the mix: at most 40 roundings, each of a
    quantity bounded by the BatchNorm cancellation scale, 40 u (mag + |c_n| (|bias_n| + |mean_n|) + |beta_n|)
  * the f16 tier runs the mix on the f16 matrix cores ([Aoff | I] x [h1; h0] in f16): d0, g1 and Aoff each rounded once to f16,
    3 2^-11 (mag + |shift_n|), plus the f16 subnormal floor of the 49 operands, 2^-25 (1 + sum_j' |A_jj'| + sum_j' |g1_j'|)
  * ReLU is 1-Lipschitz; the residual add: 2 u (|y| + |res|) (the split tier adds hi and lo separately)
  * the output format: X2 2^-22 |y| + 2^-25, f16 2^-11 |y| + 2^-25, float32 0
The hoisted input conv has no GEMM: its pre-activations are 8 f32 operations (h_oth + tvec, the vis-gated image slice, six fmas of x @ Wx), at
most 8 u (|h_img| + |h_oth| + |tvec| + sum_c |x_c Wx_c|) each, then the same epilogue.  The output conv's responses are an exact-f32 MFMA chain
over K plus three partial-sum adds, 4 sqrt(K) u (R + |h|) + 3 u |X| |W|, and its mix 30 u (mag + |bias|).  A bound is multiplied by (1 + 2^-10)
for the second-order terms (a rounding of an already perturbed value).

The sampling-loop test composes these: the per-layer bounds of the network are propagated as a random walk, i.e. the squared bound of a conv's
input goes through the same conv with squared coefficients (|c A M|^2 over W^2) and adds to the squared local bound of that conv.

Every test prints its largest error / bound ratio."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

from egohmr_amd import synthetic as syn

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PREC = {"f32": 0, "f16x3": 1, "f16": 2}
TILE = 192


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


@pytest.fixture(scope="module")
def sens_sd():
    return syn.make_sensitive_state_dict(0, with_backbone=False)


def _ck(rc, L):
    assert rc == 0, (rc, L.ehm_last_error())


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


# ------------------------------------------------------------------------------------------------ layers and weight regimes
REGIMES = ("syn", "sens", "outlier", "bn", "adj", "M", "zero")


def _syn_layer(g, K, N, dev, bn=True):
    ly = {"W": _t(g.normal(scale=0.55 / math.sqrt(K), size=(2, K, N)), dev), "M": _t(1 + g.normal(scale=0.15, size=(24, N)), dev),
          "adj2": _t(g.normal(scale=0.02, size=(24, 24)), dev), "bias": _t(g.normal(scale=0.05, size=N), dev)}
    if bn:
        ly.update(bn_weight=_t(g.uniform(0.8, 1.2, size=N), dev), bn_bias=_t(g.normal(scale=0.05, size=N), dev),
                  bn_mean=_t(g.normal(scale=0.1, size=N), dev), bn_var=_t(g.uniform(0.6, 1.4, size=N), dev))
    return ly


def _sd_layer(sd, p, dev, bn=True):
    c = p + ".gconv" if bn else p
    ly = {"W": _t(sd[c + ".W"], dev), "M": _t(sd[c + ".M"], dev), "adj2": _t(sd[c + ".adj2"], dev), "bias": _t(sd[c + ".bias"], dev)}
    if bn:
        ly.update(bn_weight=_t(sd[p + ".bn.weight"], dev), bn_bias=_t(sd[p + ".bn.bias"], dev), bn_mean=_t(sd[p + ".bn.running_mean"], dev),
                  bn_var=_t(sd[p + ".bn.running_var"], dev))
    return ly


def _sens_hidden(sd, dev):
    return [_sd_layer(sd, f"diffusion_model.gconv_layers.{b}.gconv{i}", dev) for b in range(4) for i in (1, 2)]


def _regime_layer(regime, g, K, dev, sens=None, X=None, adj=None):
    """One hid -> hid conv in a weight regime.  'bn' needs the conv's float64 input X to place running_mean at the channel's mean."""
    from oracle import gcn as og
    if regime == "sens":
        return sens
    ly = _syn_layer(g, K, K, dev)
    if regime == "outlier":                       # one weight 2^15 x the layer's absmax: the others' lo halves become f16 subnormals
        ly["W"][1, 3, 5] = float(ly["W"].abs().max()) * 2.0 ** 15
    elif regime == "bn":                          # trained-like statistics: mean = the data's, var ~ 1e-3, negative gammas
        ly["bn_var"] = _t(g.uniform(0.5e-3, 2e-3, size=K), dev)
        ly["bn_weight"] = _t(g.uniform(0.5, 1.5, size=K) * g.choice([-1.0, 1.0], size=K), dev)
        W = ly["W"].double()
        y = og.mix(X @ W[0], X @ W[1], ly, adj)
        ly["bn_mean"] = y.reshape(-1, K).mean(0).float()
    elif regime == "adj":                         # asymmetric adj2 of O(0.3)
        ly["adj2"] = _t(g.normal(scale=0.3, size=(24, 24)), dev)
    elif regime == "M":                           # modulation far from 1 (both signs, near zero, large)
        ly["M"] = _t(g.normal(scale=4.0, size=(24, K)), dev)
    elif regime == "zero":                        # wmax = 0: weight scale 1
        ly["W"] = torch.zeros_like(ly["W"])
    return ly


def _w_scale(W):
    """csrc/gcn.hip pack_layer: 2^(12 - e) for absmax = m 2^e, clamped to 2^+-24; 1 for an all-zero layer."""
    wmax = float(W.abs().max())
    if not (0.0 < wmax < 3.0e38):
        return 1.0
    e = 12 - math.frexp(wmax)[1]
    return 2.0 ** max(-24, min(24, e))


def _create(L, dev, adj, inp, hidden, out, hid):
    from egohmr_amd import _lib
    keep = []

    def params(ly, cin, cout):
        p = _lib.GConvParams()
        t = lambda v: keep.append(v.contiguous()) or keep[-1].data_ptr()
        p.W = t(ly["W"]) if ly.get("W") is not None else None
        p.M, p.adj2, p.bias = t(ly["M"]), t(ly["adj2"]), t(ly["bias"])
        if ly.get("bn_weight") is not None:
            p.bn_weight, p.bn_bias, p.bn_mean, p.bn_var = t(ly["bn_weight"]), t(ly["bn_bias"]), t(ly["bn_mean"]), t(ly["bn_var"])
        p.in_dim, p.out_dim = cin, cout
        return p

    keep.append(adj)
    pin = params(inp, hid, hid)
    arr = (_lib.GConvParams * max(1, len(hidden)))(*[params(ly, hid, hid) for ly in hidden]) if hidden else (_lib.GConvParams * 1)()
    pout = params(out, hid, 6)
    h = C.c_void_p()
    _ck(L.ehm_gcn_create(C.byref(h), adj.data_ptr(), C.byref(pin), arr, len(hidden), C.byref(pout), hid, None), L)
    return h, keep


# ------------------------------------------------------------------------------------------------ formats
def _pack(L, X, fmt):
    """float32 [rows, K] -> the format's bytes in a float32-sized buffer (f16 rows use its first half)"""
    if fmt == "f32":
        return X.clone()
    out = torch.zeros_like(X)
    _ck(L.ehm_gcn_pack_activations(X.data_ptr(), out.data_ptr(), X.shape[0], X.shape[1], 32 if fmt == "x2" else 0, None), L)
    return out


def _unpack(L, Y, fmt, rows, K):
    if fmt == "f32":
        return Y.view(-1)[: rows * K].view(rows, K).clone()
    out = torch.empty(rows, K, device=Y.device)
    _ck(L.ehm_gcn_unpack_activations(Y.data_ptr(), out.data_ptr(), rows, K, 32 if fmt == "x2" else 0, None), L)
    return out


def _act_fmt(tier):
    return {"f32": "f32", "f16x3": "x2", "f16": "f16"}[tier]


def _bytes(fmt, rows, K):
    return rows * K * (2 if fmt == "f16" else 4)


# ------------------------------------------------------------------------------------------------ bounds
def _gemm_tol(X, W, tier, s):
    """E_k for both branches: X [..., K] float64, W [2, K, N] float64"""
    K = X.shape[-1]
    X2, A1 = X * X, X.abs().sum(-1, keepdim=True)
    out = []
    for k in range(2):
        h = torch.matmul(X, W[k]).abs()
        R = torch.sqrt(torch.matmul(X2, W[k] * W[k]))
        if tier == "f32":
            e = 4 * math.sqrt(K) * U * (R + h)
        elif tier == "f16x3":
            e = 8 * 2.0 ** -20 * R + 2.0 ** -22 * math.sqrt(3 * K) * (R + h) + 2.0 ** -25 * A1 / s
        else:
            e = 4 * 2.0 ** -11 * R + 2.0 ** -22 * math.sqrt(K) * (R + h) + 2.0 ** -25 * A1 / s
        out.append(e)
    return out


def _coefs(ly, adj, dev):
    from oracle import gcn as og
    A = og.sym_adjacency(adj.double(), ly["adj2"].double())
    Ad = torch.diagonal(A)
    Ao = A * (1 - torch.eye(24, dtype=A.dtype, device=dev))
    M = ly["M"].double()
    if ly.get("bn_weight") is not None:
        c = ly["bn_weight"].double() / torch.sqrt(ly["bn_var"].double() + 1e-5)
        shift = (ly["bias"].double() - ly["bn_mean"].double()) * c + ly["bn_bias"].double()
        cancel = c.abs() * (ly["bias"].double().abs() + ly["bn_mean"].double().abs()) + ly["bn_bias"].double().abs()
    else:
        c = torch.ones_like(ly["bias"].double())
        shift, cancel = ly["bias"].double(), ly["bias"].double().abs()
    return Ad, Ao, M, c, shift, cancel


def _epi_tol(h0, h1, E0, E1, ly, adj, epi, y, res=None, store="f32"):
    """per-output bound of the epilogue on pre-activations h0, h1 [b, 24, N] with their bounds E0, E1; y = the float64 output"""
    Ad, Ao, M, c, shift, cancel = _coefs(ly, adj, h0.device)
    ac = c.abs()
    mag = ac * ((Ad[:, None] * M * h0).abs() + torch.matmul(Ao.abs(), (M * h1).abs()))
    g = ac * ((Ad[:, None] * M).abs() * E0 + torch.matmul(Ao.abs(), M.abs() * E1))
    t = g + 40 * U * (mag + cancel)
    if epi == "f16":
        g1 = (M * c * h1).abs()
        t = t + 3 * 2.0 ** -11 * (mag + shift.abs()) + 2.0 ** -25 * (1 + Ao.abs().sum(1)[:, None] + g1.sum(-2, keepdim=True))
    ya = y.abs()
    if res is not None:
        t = t + 2 * U * (ya + res.abs())
    if store == "x2":
        t = t + 2.0 ** -22 * ya + 2.0 ** -25
    elif store == "f16":
        t = t + 2.0 ** -11 * ya + 2.0 ** -25
    return t * (1 + 2.0 ** -10)


def _hidden_tol(X, ly, adj, tier, s, res=None, store="f32", y=None):
    """(float64 output, bound) of a hidden conv on X [b, 24, K] float64"""
    from oracle import gcn as og
    W = ly["W"].double()
    h0, h1 = torch.matmul(X, W[0]), torch.matmul(X, W[1])
    E0, E1 = _gemm_tol(X, W, tier, s)
    y = og.epilogue(h0, h1, ly, adj, res) if y is None else y
    return y, _epi_tol(h0, h1, E0, E1, ly, adj, "f16" if tier == "f16" else "f32", y, res, store)


def _ratio(got, ref, tol):
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all()
    return float(torch.where(err == 0, torch.zeros_like(err), err / tol).max()), float(err.max())


# ------------------------------------------------------------------------------------------------ 1. hidden conv
# (tier, residual, layer of an 8-conv handle, hid, bodies, weight regime): a pairwise cover, not the product
HIDDEN_CASES = [
    ("f32", 0, 0, 64, 1, "syn"), ("f32", 1, 7, 192, 9, "outlier"), ("f32", 0, 3, 320, 257, "bn"), ("f32", 1, 5, 1024, 33, "sens"),
    ("f32", 1, 2, 512, 8, "adj"), ("f32", 0, 6, 1024, 7, "M"), ("f32", 0, 4, 192, 257, "zero"),
    ("f16x3", 1, 7, 64, 33, "bn"), ("f16x3", 0, 7, 1024, 257, "sens"), ("f16x3", 1, 0, 192, 8, "M"), ("f16x3", 0, 1, 320, 1, "outlier"),
    ("f16x3", 1, 4, 512, 9, "syn"), ("f16x3", 0, 2, 1024, 7, "adj"), ("f16x3", 1, 6, 64, 257, "zero"), ("f16x3", 1, 3, 1024, 1, "sens"),
    ("f16", 0, 7, 512, 33, "outlier"), ("f16", 1, 0, 1024, 9, "bn"), ("f16", 0, 3, 192, 8, "adj"), ("f16", 1, 5, 1024, 7, "sens"),
    ("f16", 0, 6, 320, 1, "M"), ("f16", 1, 1, 1024, 257, "syn"), ("f16", 1, 7, 320, 9, "zero"), ("f16", 0, 2, 512, 257, "bn"),
]


@pytest.mark.parametrize("tier,res,layer,hid,bodies,regime", HIDDEN_CASES)
def test_hidden_layer_vs_fp64(L, dev, adj, sens_sd, tier, res, layer, hid, bodies, regime):
    """ehm_gcn_hidden_layer on layer `layer` of an 8-conv handle (the last one writes float32 in the split tier), with one spare all-padding
    row tile and a canary behind the output, against oracle.gcn.hidden_conv on the unpacked operands."""
    from egohmr_amd import _lib
    g = _rng(1000 + 7 * layer + hid + bodies)
    rows = bodies * 24
    rows_pad = (rows + TILE - 1) // TILE * TILE + TILE
    X = torch.zeros(rows_pad, hid, device=dev)
    X[:rows] = torch.relu(_t(g.normal(size=(rows, hid)), dev))
    R = torch.zeros(rows_pad, hid, device=dev)
    R[:rows] = torch.relu(_t(g.normal(size=(rows, hid)), dev))
    fmt = _act_fmt(tier)
    Xp, Rp = _pack(L, X, fmt), _pack(L, R, fmt)
    Xk, Rk = _unpack(L, Xp, fmt, rows, hid).double().view(bodies, 24, hid), _unpack(L, Rp, fmt, rows, hid).double().view(bodies, 24, hid)
    sens = _sens_hidden(sens_sd, dev)[layer] if regime == "sens" else None
    layers = [_syn_layer(g, hid, hid, dev) for _ in range(8)]
    layers[layer] = _regime_layer(regime, g, hid, dev, sens, Xk, adj)
    h, keep = _create(L, dev, adj, _syn_layer(g, hid, hid, dev), layers, _syn_layer(g, hid, 6, dev, bn=False), hid)
    try:
        _ck(L.ehm_gcn_set_precision(h, PREC[tier]), L)
        out_fmt = "f32" if (tier == "f32" or (tier == "f16x3" and layer == 7)) else fmt
        Y = torch.full((rows_pad + TILE, hid), float("nan"), device=dev)
        canary = Y.clone()
        _ck(L.ehm_gcn_hidden_layer(h, layer, Xp.data_ptr(), Rp.data_ptr() if res else None, Y.data_ptr(), rows_pad, None), L)
        _ck(L.ehm_gcn_stack_status(h, None), L)
        nb = _bytes(out_fmt, rows_pad, hid)
        assert torch.equal(Y.view(torch.uint8).view(-1)[nb:], canary.view(torch.uint8).view(-1)[nb:]), "write past rows_pad"
        got = _unpack(L, Y, out_fmt, rows, hid).view(bodies, 24, hid)
        ly = layers[layer]
        ref, tol = _hidden_tol(Xk, ly, adj, tier, _w_scale(ly["W"]), Rk if res else None, out_fmt)
        r, e = _ratio(got, ref, tol)
        print(f"[hidden {tier} res={res} layer={layer} hid={hid} B={bodies} {regime}] max|err| {e:.3e}  max err/bound {r:.3f}")
        assert r <= 1.0, r
    finally:
        L.ehm_gcn_destroy(h)


# ------------------------------------------------------------------------------------------------ 2. the benchmark's shape, layer by layer, and the chain
@pytest.mark.parametrize("tier", ["f16x3", "f16"])
def test_headline_shape_layers_and_chain(L, dev, adj, sens_sd, tier):
    """hid 1024, 8 convs (the benchmark's weights), B = 256 x 2 passes with half of the items (every other one) in the pass map: every
    per-conv launch against float64 from the device's own input to it, then the chained launch (4-wave split tile / 8-wave f16 tile) equal
    to the per-conv launches bit for bit."""
    hid, B = 1024, 256
    vb = B + B // 2
    rows = vb * 24
    rows_pad = (rows + TILE - 1) // TILE * TILE
    g = _rng(77)
    layers = _sens_hidden(sens_sd, dev)
    h, keep = _create(L, dev, adj, _sd_layer(sens_sd, "diffusion_model.gconv_input.0", dev), layers,
                      _sd_layer(sens_sd, "diffusion_model.gconv_output", dev, bn=False), hid)
    try:
        _ck(L.ehm_gcn_set_precision(h, PREC[tier]), L)
        fmt = _act_fmt(tier)
        X0 = torch.zeros(rows_pad, hid, device=dev)
        X0[:rows] = torch.relu(_t(g.normal(size=(rows, hid)), dev))
        X0p = _pack(L, X0, fmt)
        ref = [X0p.clone(), torch.zeros_like(X0p), torch.zeros_like(X0p)]
        worst, cur = 0.0, 0
        for blk in range(4):
            y2 = 2 if cur == 0 else 0
            for i, (src, res, dst) in enumerate(((cur, None, 1), (1, cur, y2))):
                layer = 2 * blk + i
                out_fmt = "f32" if (tier == "f16x3" and layer == 7) else fmt
                _ck(L.ehm_gcn_hidden_layer(h, layer, ref[src].data_ptr(), ref[res].data_ptr() if res is not None else None,
                                           ref[dst].data_ptr(), rows_pad, None), L)
                Xk = _unpack(L, ref[src], fmt, rows, hid).double().view(vb, 24, hid)
                Rk = _unpack(L, ref[res], fmt, rows, hid).double().view(vb, 24, hid) if res is not None else None
                got = _unpack(L, ref[dst], out_fmt, rows, hid).view(vb, 24, hid)
                ly = layers[layer]
                r_, tol = _hidden_tol(Xk, ly, adj, tier, _w_scale(ly["W"]), Rk, out_fmt)
                r, e = _ratio(got, r_, tol)
                worst = max(worst, r)
                print(f"[headline {tier} layer {layer}] max|err| {e:.3e}  max err/bound {r:.3f}")
                assert r <= 1.0, (layer, r)
            cur = y2
        _ck(L.ehm_gcn_stack_status(h, None), L)
        bufs_t = [X0p.clone(), torch.full_like(X0p, float("nan")), torch.full_like(X0p, float("nan"))]
        bufs = (C.c_void_p * 3)(*[t.data_ptr() for t in bufs_t])
        resi = C.c_int(-1)
        _ck(L.ehm_gcn_hidden_stack(h, bufs, rows_pad, C.byref(resi), None), L)
        _ck(L.ehm_gcn_stack_status(h, None), L)
        assert resi.value == cur
        assert torch.equal(bufs_t[cur][:rows].view(torch.int32), ref[cur][:rows].view(torch.int32))
        print(f"[headline {tier}] chained launch == per-conv launches bit for bit; max err/bound {worst:.3f}")
    finally:
        L.ehm_gcn_destroy(h)


# ------------------------------------------------------------------------------------------------ 3. input conv
def _pass_map(kind, B, dev):
    """(vis [B,24] uint8, mask_items or None, mask_slot or None, num_masked): 'none' = no map, 'empty' / 'partial' / 'full'.  Items that
    keep no second pass have every joint visible; the others a visibility pattern (none visible, one hidden joint, random)."""
    g = _rng(300 + B)
    vis = np.ones((B, 24), np.uint8)
    need = {"none": np.arange(B) % 2 == 0, "empty": np.zeros(B, bool), "partial": (np.arange(B) % 3) != 1, "full": np.ones(B, bool)}[kind]
    for b in np.nonzero(need)[0]:
        vis[b] = (0 if b % 4 == 0 else 1) if b % 4 in (0, 1) else g.integers(0, 2, 24)
        if b % 4 == 1:
            vis[b, b % 24] = 0
    if kind == "none":
        return torch.from_numpy(vis).to(dev), None, None, -1
    items = np.nonzero(need)[0].astype(np.int32)
    slot = -np.ones(B, np.int32)
    slot[items] = np.arange(len(items), dtype=np.int32)
    return torch.from_numpy(vis).to(dev), torch.from_numpy(items).to(dev), torch.from_numpy(slot).to(dev), len(items)


def _input_tol(ins, ly, adj, tier, passes, items, whole, store):
    from oracle import gcn as og
    h_img, h_oth, vis, x, Wx, tvec = ins
    p0, p1 = og.input_pre(h_img, h_oth, vis, x, Wx, tvec, passes, items, whole)
    a0, a1 = og.input_pre(h_img.abs(), h_oth.abs(), vis, x.abs(), Wx.abs(), tvec.abs(), passes, items, whole)   # magnitudes of the operands
    y = og.epilogue(p0, p1, ly, adj)
    return y, _epi_tol(p0, p1, 8 * U * a0, 8 * U * a1, ly, adj, "f16" if tier == "f16" else "f32", y, None, store)


INPUT_CASES = [   # (tier, passes, uncond mode, pass map, B)
    ("f32", 1, 0, "none", 1), ("f32", 2, 1, "partial", 9), ("f32", 2, 0, "full", 257), ("f32", 2, 1, "empty", 9),
    ("f16x3", 2, 0, "partial", 257), ("f16x3", 1, 1, "none", 9), ("f16x3", 2, 1, "none", 1), ("f16x3", 2, 0, "empty", 257),
    ("f16", 2, 1, "full", 9), ("f16", 2, 0, "none", 257), ("f16", 1, 0, "partial", 1), ("f16", 2, 1, "partial", 257),
]


@pytest.mark.parametrize("tier,passes,whole,kind,B", INPUT_CASES)
def test_input_layer_vs_fp64(L, dev, adj, sens_sd, tier, passes, whole, kind, B):
    """ehm_gcn_input_layer (f32 / X2 / f16 rows) against oracle.gcn.input_conv: vis-gated h_img, h_oth, tvec, x @ Wx, pass map, uncond mode."""
    hid = 1024
    g = _rng(500 + B + 3 * passes)
    inp = _sd_layer(sens_sd, "diffusion_model.gconv_input.0", dev)
    h, keep = _create(L, dev, adj, inp, _sens_hidden(sens_sd, dev), _sd_layer(sens_sd, "diffusion_model.gconv_output", dev, bn=False), hid)
    try:
        vis, items, slot, nm = _pass_map(kind, B, dev)
        _ck(L.ehm_gcn_set_precision(h, PREC[tier]), L)
        _ck(L.ehm_gcn_set_uncond_mode(h, whole), L)
        _ck(L.ehm_gcn_set_pass_map(h, items.data_ptr() if nm > 0 else None, slot.data_ptr() if nm >= 0 else None, nm), L)
        h_img, h_oth = _t(g.normal(scale=0.5, size=(B, 2, hid)), dev), _t(g.normal(scale=0.5, size=(B, 2, hid)), dev)
        x, Wx, tvec = _t(g.normal(size=(B, 144)), dev), _t(g.normal(scale=0.3, size=(2, 6, hid)), dev), _t(g.normal(scale=0.5, size=(2, hid)), dev)
        vb = B + (B if nm < 0 else nm) if passes == 2 else B
        rows = vb * 24
        rows_pad = (rows + TILE - 1) // TILE * TILE
        fmt = _act_fmt(tier)
        Y = torch.full((rows_pad + TILE, hid), float("nan"), device=dev)
        canary = Y.clone()
        _ck(L.ehm_gcn_input_layer(h, h_img.data_ptr(), h_oth.data_ptr(), vis.data_ptr(), x.data_ptr(), Wx.data_ptr(), tvec.data_ptr(),
                                  Y.data_ptr(), B, passes, None), L)
        _ck(L.ehm_gcn_stack_status(h, None), L)
        nb = _bytes(fmt, rows, hid)
        assert torch.equal(Y.view(torch.uint8).view(-1)[nb:], canary.view(torch.uint8).view(-1)[nb:]), "write past the valid rows"
        got = _unpack(L, Y, fmt, rows, hid).view(vb, 24, hid)
        ins = tuple(t.double() for t in (h_img, h_oth, vis, x, Wx, tvec))
        ref, tol = _input_tol(ins, inp, adj, tier, passes, items if (passes == 2 and nm >= 0) else None, bool(whole), fmt)
        assert ref.shape == got.shape
        r, e = _ratio(got, ref, tol)
        print(f"[input {tier} passes={passes} uncond={whole} map={kind} B={B}] max|err| {e:.3e}  max err/bound {r:.3f}")
        assert r <= 1.0, r
    finally:
        L.ehm_gcn_destroy(h)


@pytest.mark.parametrize("tier", ["f32", "f16x3", "f16"])
def test_input_layer_rows_vs_fp64(L, dev, adj, tier):
    """ehm_gcn_input_layer_rows on ragged body counts against oracle.gcn.input_rows."""
    from oracle import gcn as og
    hid = 320
    g = _rng(600 + PREC[tier])
    inp = _syn_layer(g, hid, hid, dev)
    h, keep = _create(L, dev, adj, inp, [_syn_layer(g, hid, hid, dev) for _ in range(2)], _syn_layer(g, hid, 6, dev, bn=False), hid)
    worst = 0.0
    try:
        _ck(L.ehm_gcn_set_precision(h, PREC[tier]), L)
        fmt = _act_fmt(tier)
        for bodies in (1, 7, 9, 33):
            pre = _t(g.normal(size=(bodies * 24, 2, hid)), dev)
            rows_pad = (bodies * 24 + TILE - 1) // TILE * TILE
            Y = torch.full((rows_pad, hid), float("nan"), device=dev)
            _ck(L.ehm_gcn_input_layer_rows(h, pre.data_ptr(), Y.data_ptr(), bodies, None), L)
            got = _unpack(L, Y, fmt, bodies * 24, hid).view(bodies, 24, hid)
            p = pre.double().view(bodies, 24, 2, hid)
            y = og.input_rows(pre.double(), inp, adj)
            z = torch.zeros_like(p[:, :, 0])
            tol = _epi_tol(p[:, :, 0], p[:, :, 1], z, z, inp, adj, "f16" if tier == "f16" else "f32", y, None, fmt)
            r, e = _ratio(got, y, tol)
            worst = max(worst, r)
            assert r <= 1.0, (bodies, r)
        print(f"[input rows {tier}] max err/bound {worst:.3f}")
    finally:
        L.ehm_gcn_destroy(h)


# ------------------------------------------------------------------------------------------------ 4. output conv
OUTPUT_CASES = [   # (tier, passes, pass map, hid)
    ("f32", 1, "none", 192), ("f32", 2, "partial", 320), ("f32", 2, "full", 1024),
    ("f16x3", 2, "none", 1024), ("f16x3", 2, "partial", 192), ("f16x3", 1, "none", 320),
    ("f16", 2, "empty", 320), ("f16", 2, "partial", 1024), ("f16", 1, "none", 192), ("f16", 2, "full", 192),
]


@pytest.mark.parametrize("tier,passes,kind,hid", OUTPUT_CASES)
def test_output_layer_vs_fp64(L, dev, adj, tier, passes, kind, hid):
    """ehm_gcn_output_layer: f32 rows, the split tier's float32 last conv, f16 rows; the visibility fuse of the two passes and the pass-map
    slots (visibility none / one joint / random per item), against oracle.gcn.output_conv."""
    from oracle import gcn as og
    B = 21
    g = _rng(700 + hid + passes)
    out = _syn_layer(g, hid, 6, dev, bn=False)
    h, keep = _create(L, dev, adj, _syn_layer(g, hid, hid, dev), [_syn_layer(g, hid, hid, dev) for _ in range(2)], out, hid)
    try:
        vis, items, slot, nm = _pass_map(kind, B, dev)
        _ck(L.ehm_gcn_set_precision(h, PREC[tier]), L)
        _ck(L.ehm_gcn_set_pass_map(h, items.data_ptr() if nm > 0 else None, slot.data_ptr() if nm >= 0 else None, nm), L)
        vb = B + (B if nm < 0 else nm) if passes == 2 else B
        rows = vb * 24
        rows_pad = (rows + TILE - 1) // TILE * TILE
        X = torch.zeros(rows_pad, hid, device=dev)
        X[:rows] = torch.relu(_t(g.normal(size=(rows, hid)), dev))
        fmt = "f16" if tier == "f16" else "f32"
        Xp = _pack(L, X, fmt)
        Xk = _unpack(L, Xp, fmt, rows, hid).double().view(vb, 24, hid)
        x0 = torch.full((B, 144), float("nan"), device=dev)
        _ck(L.ehm_gcn_output_layer(h, Xp.data_ptr(), vis.data_ptr(), x0.data_ptr(), B, passes, None), L)
        torch.cuda.synchronize()
        W = out["W"].double()
        hs0, hs1 = torch.matmul(Xk, W[0]), torch.matmul(Xk, W[1])
        S = [torch.matmul(Xk.abs(), W[k].abs()) for k in range(2)]
        E0, E1 = (4 * math.sqrt(hid) * U * (torch.sqrt(torch.matmul(Xk * Xk, W[k] * W[k])) + hh.abs()) + 3 * U * S[k] for k, hh in ((0, hs0), (1, hs1)))
        y = og.mix(hs0, hs1, out, adj)
        Ad, Ao, M, c, shift, cancel = _coefs(out, adj, dev)
        mag = (Ad[:, None] * M * hs0).abs() + torch.matmul(Ao.abs(), (M * hs1).abs())
        tol = ((Ad[:, None] * M).abs() * E0 + torch.matmul(Ao.abs(), M.abs() * E1) + 30 * U * (mag + out["bias"].double().abs())) * (1 + 2.0 ** -10)
        sl = slot if (passes == 2 and nm >= 0) else None
        ref = og.fuse(y, vis, B, passes, sl)
        tol = og.fuse(tol, vis, B, passes, sl)
        r, e = _ratio(x0, ref, tol)
        print(f"[output {tier} passes={passes} map={kind} hid={hid}] max|err| {e:.3e}  max err/bound {r:.3f}")
        assert r <= 1.0, r
    finally:
        L.ehm_gcn_destroy(h)


# ------------------------------------------------------------------------------------------------ 5. pack / unpack
def _np_split(v):
    """gcn_dev.h split_store in numpy: hi = f16(clamp(v)), lo = f16(clamp(v - hi)), the difference in float32"""
    v = v.astype(np.float32)
    hi = np.clip(v, -65504, 65504).astype(np.float16)
    lo = np.clip((v - hi.astype(np.float32)).astype(np.float32), -65504, 65504).astype(np.float16)
    return hi, lo


def test_pack_unpack_bitwise(L, dev):
    """ehm_gcn_pack_activations (groups 32 and 0) bit for bit against a numpy restatement of split_store / the f16 pack: subnormals, halfway
    ties, +-65504, 65520, values past 131008; unpack is exact."""
    g = _rng(800)
    K, rows = 96, 5
    special = np.array([0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -14, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2049.0, 2051.0,
                        65504.0, -65504.0, 65520.0, -65520.0, 131008.0, 140000.0, -2.0e5, 1e-30, 1 / 3, -2 / 3, 5.960464477539063e-08,
                        6.103515625e-05, 1 + 2.0 ** -22, 1 + 2.0 ** -23], np.float32)
    X = g.normal(scale=3.0, size=(rows, K)).astype(np.float32)
    X.reshape(-1)[: special.size] = special
    X[2] *= 1e-5                                      # subnormal lo halves
    X[3] = (np.round(X[3] * 2048) + 0.5) / 2048        # ties of the hi rounding
    Xd = torch.from_numpy(X).to(dev)
    P = torch.zeros(rows, K, device=dev)
    _ck(L.ehm_gcn_pack_activations(Xd.data_ptr(), P.data_ptr(), rows, K, 32, None), L)
    hi, lo = _np_split(X)
    want = np.empty((rows, K // 32, 2, 32), np.float16)
    want[:, :, 0] = hi.reshape(rows, K // 32, 32)
    want[:, :, 1] = lo.reshape(rows, K // 32, 32)
    got = P.cpu().numpy().view(np.uint16).reshape(rows, K // 32, 2, 32)
    assert np.array_equal(got, want.view(np.uint16))
    back = _unpack(L, P, "x2", rows, K).cpu().numpy()
    assert np.array_equal(back, hi.astype(np.float32) + lo.astype(np.float32))
    P0 = torch.zeros(rows, K, device=dev)
    _ck(L.ehm_gcn_pack_activations(Xd.data_ptr(), P0.data_ptr(), rows, K, 0, None), L)
    got0 = P0.cpu().numpy().view(np.uint16).reshape(-1)[: rows * K]
    assert np.array_equal(got0, np.clip(X, -65504, 65504).astype(np.float16).view(np.uint16).reshape(-1))
    assert np.array_equal(_unpack(L, P0, "f16", rows, K).cpu().numpy(), np.clip(X, -65504, 65504).astype(np.float16).astype(np.float32))


# ------------------------------------------------------------------------------------------------ 6. range guard
def test_range_guard_looks_at_valid_rows_only(L, dev, adj):
    """After an input conv for B = 9 (216 valid rows of 384), values in the padding rows that drive the next conv past 65504 leave
    ehm_gcn_stack_status at 0; the same values in valid rows give -34 (ERANGE)."""
    from oracle import gcn as og
    hid, B = 64, 9
    g = _rng(900)
    layers = [_syn_layer(g, hid, hid, dev) for _ in range(2)]
    h, keep = _create(L, dev, adj, _syn_layer(g, hid, hid, dev), layers, _syn_layer(g, hid, 6, dev, bn=False), hid)
    try:
        _ck(L.ehm_gcn_set_precision(h, PREC["f16x3"]), L)
        rows, rows_pad = B * 24, 384
        h_img, h_oth = _t(g.normal(scale=0.5, size=(B, 2, hid)), dev), _t(g.normal(scale=0.5, size=(B, 2, hid)), dev)
        x, Wx, tvec = _t(g.normal(size=(B, 144)), dev), _t(g.normal(scale=0.3, size=(2, 6, hid)), dev), _t(g.normal(scale=0.5, size=(2, hid)), dev)
        vis = torch.ones(B, 24, dtype=torch.uint8, device=dev)
        X = torch.zeros(rows_pad, hid, device=dev)
        _ck(L.ehm_gcn_input_layer(h, h_img.data_ptr(), h_oth.data_ptr(), vis.data_ptr(), x.data_ptr(), Wx.data_ptr(), tvec.data_ptr(),
                                  X.data_ptr(), B, 1, None), L)
        assert L.ehm_gcn_stack_status(h, None) == 0
        big = torch.full((rows_pad - rows, hid), 65000.0, device=dev)
        bigp = _pack(L, big, "x2")
        yref = og.hidden_conv(_unpack(L, bigp, "x2", rows_pad - rows, hid).double()[:144].view(6, 24, hid), layers[0], adj)
        assert float(yref.abs().max()) > 65504                  # the precondition: these rows do drive the conv past the f16 range
        X.view(torch.int32)[rows:] = bigp.view(torch.int32)
        Y = torch.zeros_like(X)
        _ck(L.ehm_gcn_hidden_layer(h, 0, X.data_ptr(), None, Y.data_ptr(), rows_pad, None), L)
        assert L.ehm_gcn_stack_status(h, None) == 0
        X.view(torch.int32)[rows - 144: rows] = bigp.view(torch.int32)[:144]
        _ck(L.ehm_gcn_hidden_layer(h, 0, X.data_ptr(), None, Y.data_ptr(), rows_pad, None), L)
        assert L.ehm_gcn_stack_status(h, None) == -34
        assert L.ehm_gcn_stack_status(h, None) == 0
    finally:
        L.ehm_gcn_destroy(h)


# ------------------------------------------------------------------------------------------------ 7. zero hidden convs
@pytest.mark.parametrize("tier", ["f32", "f16x3", "f16"])
def test_zero_hidden_convs_denoise_vs_fp64(L, dev, adj, tier):
    """A handle with no hidden conv (ModulatedGCN(num_layers=0)): the input conv feeds the output conv directly, so in the split tier it has to
    write float32 rows (the output conv reads float32 there).  Input conv -> (empty) hidden stack -> output conv against float64."""
    from oracle import gcn as og
    hid, B = 128, 7
    g = _rng(950)
    inp, out = _syn_layer(g, hid, hid, dev), _syn_layer(g, hid, 6, dev, bn=False)
    h, keep = _create(L, dev, adj, inp, [], out, hid)
    try:
        _ck(L.ehm_gcn_set_precision(h, PREC[tier]), L)
        h_img, h_oth = _t(g.normal(scale=0.5, size=(B, 2, hid)), dev), _t(g.normal(scale=0.5, size=(B, 2, hid)), dev)
        x, Wx, tvec = _t(g.normal(size=(B, 144)), dev), _t(g.normal(scale=0.3, size=(2, 6, hid)), dev), _t(g.normal(scale=0.5, size=(2, hid)), dev)
        vis = torch.from_numpy(g.integers(0, 2, size=(B, 24)).astype(np.uint8)).to(dev)
        rows = 2 * B * 24
        rows_pad = (rows + TILE - 1) // TILE * TILE
        bufs_t = [torch.zeros(rows_pad, hid, device=dev) for _ in range(3)]
        _ck(L.ehm_gcn_input_layer(h, h_img.data_ptr(), h_oth.data_ptr(), vis.data_ptr(), x.data_ptr(), Wx.data_ptr(), tvec.data_ptr(),
                                  bufs_t[0].data_ptr(), B, 2, None), L)
        bufs = (C.c_void_p * 3)(*[t.data_ptr() for t in bufs_t])
        resi = C.c_int(-1)
        _ck(L.ehm_gcn_hidden_stack(h, bufs, rows_pad, C.byref(resi), None), L)
        x0 = torch.full((B, 144), float("nan"), device=dev)
        _ck(L.ehm_gcn_output_layer(h, bufs_t[resi.value].data_ptr(), vis.data_ptr(), x0.data_ptr(), B, 2, None), L)
        _ck(L.ehm_gcn_stack_status(h, None), L)
        ins = tuple(t.double() for t in (h_img, h_oth, vis, x, Wx, tvec))
        ref, _ = og.denoiser(*ins, [inp, out], adj, passes=2)
        # bound: the input conv's (f16 rows in the f16 tier), composed through the output conv as in the sampling-loop test
        store = "f16" if tier == "f16" else "f32"
        y, tin = _input_tol(ins, inp, adj, tier, 2, None, False, store)
        x0_tol = _out_tol(y, tin, out, adj, vis, B, 2, None)
        r, e = _ratio(x0, ref, x0_tol)
        print(f"[zero hidden convs {tier}] max|err| {e:.3e}  max err/bound {r:.3f}")
        assert r <= 1.0, r
    finally:
        L.ehm_gcn_destroy(h)


def _conv_sq(v2, ly, adj):
    """a squared bound of a conv's input [b,24,K] through the conv with squared coefficients (random walk)"""
    W = ly["W"].double()
    Ad, Ao, M, c, _, _ = _coefs(ly, adj, v2.device)
    h0, h1 = torch.matmul(v2, W[0] ** 2), torch.matmul(v2, W[1] ** 2)
    return (c ** 2) * ((Ad[:, None] * M) ** 2 * h0 + torch.matmul(Ao ** 2, M ** 2 * h1))


def _out_tol(X, tin, out, adj, vis, B, passes, slot):
    """bound of x0 from the output conv's float64 input X with bound tin: local (exact-f32 responses + mix) and propagated"""
    from oracle import gcn as og
    K = X.shape[-1]
    W = out["W"].double()
    hs = [torch.matmul(X, W[k]) for k in range(2)]
    E = [4 * math.sqrt(K) * U * (torch.sqrt(torch.matmul(X * X, W[k] ** 2)) + hs[k].abs()) + 3 * U * torch.matmul(X.abs(), W[k].abs())
         for k in range(2)]
    Ad, Ao, M, _, _, _ = _coefs(out, adj, X.device)
    mag = (Ad[:, None] * M * hs[0]).abs() + torch.matmul(Ao.abs(), (M * hs[1]).abs())
    loc = ((Ad[:, None] * M).abs() * E[0] + torch.matmul(Ao.abs(), M.abs() * E[1]) + 30 * U * (mag + out["bias"].double().abs())) * (1 + 2.0 ** -10)
    tol = torch.sqrt(_conv_sq(tin ** 2, out, adj)) + loc
    return og.fuse(tol, vis, B, passes, slot)


# ------------------------------------------------------------------------------------------------ 8. inside ehm_sample_loop
def _x0_table():
    """Two ehm_step_coefs rows: step 0 x1 = x_T (coef2 = 1), step 1 x2 = x0(x1) (coef1 = 1): the sample is the denoiser's x0 at x_T bit for bit,
    and step 1's input conv runs inside step 0's fused launch."""
    from egohmr_amd import _lib
    r0, r1 = _lib.StepCoefs(), _lib.StepCoefs()
    r0.coef2 = 1.0
    r1.coef1 = 1.0
    return (_lib.StepCoefs * 2)(r0, r1), 2


@pytest.fixture(scope="module")
def sens_model(dev):
    from egohmr_amd.factory import build_synthetic_model
    return build_synthetic_model(dev, 0, diffuse_fuse=True, sensitive=True)


@pytest.mark.parametrize("passes", [1, 2])
def test_denoiser_inside_the_sample_loop(dev, adj, sens_model, monkeypatch, passes):
    """x0 out of ehm_sample_loop (fused step launch and per-step launches; every tier) is (i) bit-equal to FusedSampler.denoise_once on the
    same prepared state and tvec, and (ii) within the composed float64 bound of the whole network from the prepared float32 inputs."""
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device
    from egohmr_amd.fused import FusedSampler
    from oracle import gcn as og
    m = sens_model
    fs = m.fused_sampler
    monkeypatch.setattr(FusedSampler, "step_table", staticmethod(lambda *a, **k: _x0_table()))
    m.diffuse_fuse = passes == 2
    m.prune_passes = True
    d = create_gaussian_diffusion(num_diffusion_timesteps=2, timestep_respacing="")
    B = 40
    batch = batch_to_device(syn.make_batch(B, 512, seed=1500 + passes), dev)
    st = fs.prepare(batch)
    noise = torch.from_numpy(syn.make_noise_stack(2, B, seed=1600 + passes)).to(dev)
    x = noise[0].contiguous()
    dm = m.diffusion_model
    sd = {k: v.detach() for k, v in dm.state_dict().items()}
    sdp = {("diffusion_model." + k): v.cpu().numpy() for k, v in sd.items()}
    inp = _sd_layer(sdp, "diffusion_model.gconv_input.0", dev)
    hidden = _sens_hidden(sdp, dev)
    out = _sd_layer(sdp, "diffusion_model.gconv_output", dev, bn=False)
    t0 = time.time()
    worst = {}
    try:
        for tier in ("f32", "f16x3", "f16"):
            m.gcn_precision = tier
            tv = fs.timestep_vectors([d.timestep_map[i] for i in range(1, -1, -1)])
            generic = fs.denoise_once(st, x, tv[1].contiguous(), passes)
            for psl in (False, True):
                m.per_step_launches = psl
                res = fs.run(d, dict(batch), noise, ddim=False, guided=False, prepared=st, lowprec=0)
                got = res["sample"]
                assert torch.equal(got, generic), (tier, psl, float((got - generic).abs().max()))
            # (ii) the composed bound from the prepared float32 inputs
            items = st.mask_items[: st.num_masked] if (passes == 2 and st.num_masked >= 0) else None
            slot = st.mask_slot if (passes == 2 and st.num_masked >= 0) else None
            ins = tuple(t.double() for t in (st.h_img, st.h_oth, st.vis, x, fs._folded.Wx, tv[1]))
            fmt = _act_fmt(tier)
            y, tol = _input_tol(ins, inp, adj, tier, passes, items, False, fmt)
            for b in range(4):
                r = (y, tol)
                y1, t1 = _hidden_tol(y, hidden[2 * b], adj, tier, _w_scale(hidden[2 * b]["W"]), None, fmt)
                tol = torch.sqrt(_conv_sq(tol ** 2, hidden[2 * b], adj) + t1 ** 2)
                last = b == 3
                y2, t2 = _hidden_tol(y1, hidden[2 * b + 1], adj, tier, _w_scale(hidden[2 * b + 1]["W"]), r[0],
                                     "f32" if (last and tier == "f16x3") else fmt)
                tol = torch.sqrt(_conv_sq(tol ** 2, hidden[2 * b + 1], adj) + t2 ** 2) + r[1]
                y = y2
            x0_ref = og.fuse(og.hidden_conv(y, out, adj), st.vis, B, passes, slot)
            x0_tol = _out_tol(y, tol, out, adj, st.vis, B, passes, slot)
            ref_all, _ = og.denoiser(*ins, [inp] + hidden + [out], adj, passes, items, slot)
            assert torch.allclose(ref_all, x0_ref, rtol=0, atol=1e-12)
            r_, e = _ratio(generic, x0_ref, x0_tol)
            worst[tier] = r_
            print(f"[sample loop passes={passes} {tier}] x0 bit-equal to denoise_once (fused and per-step launches); max|err| vs fp64 {e:.3e}, "
                  f"max err/bound {r_:.3f}")
            assert r_ <= 1.0, (tier, r_)
    finally:
        m.gcn_precision, m.per_step_launches, m.diffuse_fuse = "f16x3", False, True
    print(f"[sample loop passes={passes}] {time.time() - t0:.1f} s")
