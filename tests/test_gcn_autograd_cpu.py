"""CPU: the closed-form vector-Jacobian product of one Modulated-GCN graph conv that csrc/gcn_bwd.hip and egohmr_amd/gcn_grad.py implement
(ModulatedGraphConv + BatchNorm1d(eval) + ReLU + residual: modulated_gcn_conv.py:39-50, modulated_gcn.py:21-28, :38-42), written once in float64
torch, equals autograd through oracle.gcn.hidden_conv; the new entry points are exported, prototyped and refuse bad arguments before any device call;
the route selection of ModulatedGCN.forward."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import gcn as og

NEW = ("ehm_gcn_bwd_epilogue", "ehm_gcn_bwd_params", "ehm_gcn_bwd_params_workspace_bytes")
PARAMS = ("W", "M", "adj2", "bias", "bn_weight", "bn_bias")


def closed_form_vjp(x, ly, adj, g, eps=og.BN_EPS):
    """x [b,24,K], layer dict (float64), g = dL/dout [b,24,N] -> dict of gradients (x, residual and every parameter the layer has)."""
    W, M, bias = ly["W"], ly["M"], ly["bias"]
    A = og.sym_adjacency(adj, ly["adj2"])
    E = torch.eye(24, dtype=A.dtype)
    Ad, Ao = A * E, A * (1 - E)
    h0, h1 = x @ W[0], x @ W[1]
    u0, u1 = M * h0, M * h1
    z = Ad @ u0 + Ao @ u1 + bias
    bn = ly.get("bn_weight") is not None
    out = {"residual": g}
    if bn:
        rstd = 1.0 / torch.sqrt(ly["bn_var"] + eps)
        c = ly["bn_weight"] * rstd
        v = c * (z - ly["bn_mean"]) + ly["bn_bias"]
        vbar = g * (torch.relu(v) > 0)
        out["bn_bias"] = vbar.sum((0, 1))
        out["bn_weight"] = (vbar * (z - ly["bn_mean"]) * rstd).sum((0, 1))
        zbar = c * vbar
    else:
        zbar = g
    out["bias"] = zbar.sum((0, 1))
    u0bar = Ad.T @ zbar                                   # u0bar[j] = A_jj zbar[j]
    u1bar = Ao.T @ zbar                                   # u1bar[i] = sum_{j != i} A_ji zbar[j]
    Abar = torch.einsum("bjn,bin->ji", zbar, u0) * E + torch.einsum("bjn,bin->ji", zbar, u1) * (1 - E)
    out["adj2"] = (Abar + Abar.T) / 2
    out["M"] = (u0bar * h0 + u1bar * h1).sum(0)
    h0bar, h1bar = M * u0bar, M * u1bar
    out["W"] = torch.stack([torch.einsum("bjk,bjn->kn", x, h0bar), torch.einsum("bjk,bjn->kn", x, h1bar)])
    out["x"] = h0bar @ W[0].T + h1bar @ W[1].T
    return out


def _layer(g, K, N, bn, neg_gamma, adj_scale):
    ly = {"W": g.normal(scale=0.55 / math.sqrt(K), size=(2, K, N)), "M": 1 + g.normal(scale=0.15, size=(24, N)),
          "adj2": g.normal(scale=adj_scale, size=(24, 24)), "bias": g.normal(scale=0.05, size=N)}
    if bn:
        gam = g.uniform(0.5, 1.5, size=N) * (g.choice([-1.0, 1.0], size=N) if neg_gamma else 1.0)
        ly.update(bn_weight=gam, bn_bias=g.normal(scale=0.05, size=N), bn_mean=g.normal(scale=0.1, size=N), bn_var=g.uniform(0.6, 1.4, size=N))
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in ly.items()}


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("bn,neg_gamma", [(True, False), (True, True), (False, False)])
@pytest.mark.parametrize("adj_scale", [0.02, 0.3])
def test_closed_form_vjp_equals_autograd_through_the_oracle(res, bn, neg_gamma, adj_scale):
    from egohmr_amd.model import smpl_tree_adjacency
    g = np.random.Generator(np.random.PCG64(11))
    b, K, N = 3, 40, 6 if not bn else 24
    adj = smpl_tree_adjacency().double()
    ly = _layer(g, K, N, bn, neg_gamma, adj_scale)
    assert not torch.equal(ly["adj2"], ly["adj2"].T)                                       # asymmetric
    if neg_gamma:
        assert (ly["bn_weight"] < 0).any() and (ly["bn_weight"] > 0).any()
    x = torch.from_numpy(g.normal(size=(b, 24, K)))
    r = torch.from_numpy(g.normal(scale=3.0, size=(b, 24, N))) if res else None
    gout = torch.from_numpy(g.normal(size=(b, 24, N)))
    names = [k for k in PARAMS if k in ly]
    leaves = [x.clone().requires_grad_()] + [ly[k].clone().requires_grad_() for k in names] + ([r.clone().requires_grad_()] if res else [])
    lyg = {**ly, **dict(zip(names, leaves[1:1 + len(names)]))}
    out = og.hidden_conv(leaves[0], lyg, adj, residual=leaves[-1] if res else None)
    ref = dict(zip(["x"] + names + (["residual"] if res else []), torch.autograd.grad(out, leaves, gout)))
    got = closed_form_vjp(x, ly, adj, gout)
    for k, v in ref.items():
        err = float((got[k] - v).abs().max()) / max(float(v.abs().max()), 1e-300)
        assert err < 1e-12, (k, err)
    if bn:                                                                                  # both signs of the gate occur
        z = og.mix(x @ ly["W"][0], x @ ly["W"][1], ly, adj)
        y = og.bn_relu(z, ly)
        assert 0.1 < float((y > 0).double().mean()) < 0.9


def test_gate_of_a_small_activation_is_not_recoverable_from_out_minus_residual():
    """Why the forward keeps the gate source: in float32, res + y == res for a small positive y, so (out - res > 0) loses the gate."""
    y, res = torch.tensor(1e-6, dtype=torch.float32), torch.tensor(100.0, dtype=torch.float32)
    assert y > 0 and not ((res + y) - res > 0)


# ---------------------------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def L():
    from egohmr_amd import _lib
    _lib.build()
    return _lib.lib()


def test_symbols_are_exported_and_prototyped(L):
    from egohmr_amd import _lib
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.PROTOTYPES and name not in _lib.VALUE_FUNCTIONS
        assert _lib.PROTOTYPES[name][0] is ctypes.c_int
        assert callable(getattr(_lib.api(), name))
    assert len(_lib.PROTOTYPES["ehm_gcn_bwd_epilogue"][1]) == 8
    assert len(_lib.PROTOTYPES["ehm_gcn_bwd_params"][1]) == 15
    assert len(_lib.PROTOTYPES["ehm_gcn_bwd_params_workspace_bytes"][1]) == 4
    assert "gcn_bwd.hip" in _lib.SOURCES
    assert (_lib.GCN_CONV_INPUT, _lib.GCN_CONV_OUTPUT) == (-1, -2)


def test_entries_refuse_a_null_handle_before_any_device_call(L):
    from egohmr_amd import _lib
    nb = ctypes.c_int64(-1)
    assert L.ehm_gcn_bwd_params_workspace_bytes(None, 0, 4, ctypes.byref(nb)) == -22 and b"bad argument" in L.ehm_last_error()
    assert nb.value == -1
    p = 0x10000                                                                            # never dereferenced on the host
    assert L.ehm_gcn_bwd_epilogue(None, 0, p, p, p, 128, 4, None) == -22
    assert L.ehm_gcn_bwd_params(None, 0, p, p, p, 128, 4, p, p, p, p, p, p, 1 << 20, None) == -22
    with pytest.raises(_lib.EgoHMRHipError) as e:
        _lib.api().ehm_gcn_bwd_epilogue(None, 0, None, None, None, 0, 0, None)
    assert e.value.rc == -22 and e.value.function == "ehm_gcn_bwd_epilogue"


# ---------------------------------------------------------------------------------------------- route selection (no device needed)
def test_route_selection():
    from egohmr_amd.model import ModulatedGCN, smpl_tree_adjacency
    m = ModulatedGCN(smpl_tree_adjacency(), in_dim=70, hid_dim=64, num_layers=1).eval()
    assert m.grad_params is False
    x = torch.zeros(2, 24, 70)
    assert not m._wants_grad(x)                                         # parameters require grad by default: still today's route
    assert m._wants_grad(x.clone().requires_grad_())
    with torch.no_grad():
        assert not m._wants_grad(x.clone().requires_grad_())
    m.grad_params = True
    assert m._wants_grad(x)
    for p in m.parameters():
        p.requires_grad_(False)
    assert not m._wants_grad(x)
    names = [n for n, _ in m.named_parameters()]
    gp = m.grad_parameters()
    assert len(gp) == 6 * 3 + 4 and {id(p) for p in gp} == {id(p) for p in m.parameters()}, names
    m.train()
    with pytest.raises(NotImplementedError, match="inference only"):
        m(x.clone().requires_grad_())
