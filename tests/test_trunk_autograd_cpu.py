"""No GPU: the call surface of the ResNet-50 trunk's backward (csrc/conv_bwd.hip, egohmr_amd/trunk_grad.py, ResNet50Features.grad_params,
EgoHMR.trunk_grad) - exported symbols, argument refusals, route refusals, the BatchNorm unfold formulas, the float64 reference of
tests/trunk_grad_ref.py against torch autograd, init_optimizers' list - and the seed of the end-to-end GPU test."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import trunk_grad_ref as R

ATOL, RTOL = 2e-4, 2e-3                   # the project's VJP bar (tests/test_gpu_gcn_autograd.py, tests/test_gpu_pointnet_autograd.py)
# The end-to-end seed (weights, image, cotangent; B = 2, 64 x 64): searched on the CPU over seeds 0..23 with trunk_grad_ref.float32_error - a float32
# run of the reference against its float64 run, max over the 159 parameter tensors of max|g32 - g64| / max|g64|.  Seeds 7, 13, 14, 18 and 22 have a ReLU
# gate or a pool arg-max that float32 flips (4.6e-4 .. 1.1e-1); the others lie between 1.4e-6 and 4.1e-6; 3 is the lowest (1.40e-6).
E2E_SEED = 3
E2E_F32_ERROR = 1.403e-6                  # measured; the GPU test needs it within a quarter of the bar
E2E_SHAPE = (2, 64, 64)

NEW = {"ehm_conv_bwd_gate": 12, "ehm_conv_bwd_wgrad_workspace_bytes": 9, "ehm_conv_bwd_wgrad": 16, "ehm_resnet_stem_backward_workspace_bytes": 4,
       "ehm_resnet_stem_backward": 14, "ehm_smpl_backward_ordered": 11, "ehm_smpl_backward_ordered_workspace_bytes": 3}


def test_symbols_exported_and_bound():
    from egohmr_amd import _lib
    handle = C.CDLL(_lib.build())
    header = open(os.path.join(_lib.INCLUDE, "egohmr_hip.h")).read()
    for name, nargs in NEW.items():
        assert getattr(handle, name) is not None and name in _lib.PROTOTYPES and name in header
        assert len(_lib.PROTOTYPES[name][1]) == nargs and _lib.PROTOTYPES[name][0] is C.c_int
        assert name not in _lib.VALUE_FUNCTIONS                       # sizes come back through an out-pointer
    assert "conv_bwd.hip" in _lib.SOURCES
    # the ordered SMPL backward is a twin beside the entry point that exists, with its prototype
    assert _lib.PROTOTYPES["ehm_smpl_backward_ordered"] == _lib.PROTOTYPES["ehm_smpl_backward"]
    assert _lib.PROTOTYPES["ehm_smpl_backward_ordered_workspace_bytes"] == _lib.PROTOTYPES["ehm_smpl_backward_workspace_bytes"]


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """Every refusal runs before a launch: dummy addresses are never dereferenced."""
    from egohmr_amd import _lib
    L = _lib.lib()
    a, b, c, d = 0x10000, 0x20000, 0x30000, 0x40000
    gate_ok = dict(g=a, per=0, y=b, scale=None, out=c, N=1, Ho=4, Wo=4, C=64, H=4, W=4)
    for bad in (dict(g=None), dict(y=None), dict(out=None), dict(C=48), dict(C=0), dict(N=0), dict(per=2), dict(H=9, W=9), dict(H=8, W=5), dict(g=a + 4),
                dict(out=a)):
        k = {**gate_ok, **bad}
        assert L.ehm_conv_bwd_gate(k["g"], k["per"], k["y"], k["scale"], k["out"], k["N"], k["Ho"], k["Wo"], k["C"], k["H"], k["W"], None) == -22, bad
        assert b"bad argument" in L.ehm_last_error()
    nb = C.c_int64(-1)
    assert L.ehm_conv_bwd_wgrad_workspace_bytes(2, 7, 7, 64, 128, 3, 1, 1, None) == -22
    for shape in ((2, 7, 7, 96, 64, 3, 1, 1), (2, 7, 7, 64, 32, 3, 1, 1), (2, 7, 7, 64, 64, 5, 1, 2), (2, 7, 7, 64, 64, 3, 3, 1), (0, 7, 7, 64, 64, 1, 1, 0),
                  (1, 1, 1, 64, 64, 3, 1, 0), (1, 7, 7, 64, 64, 3, 1, -1)):
        assert L.ehm_conv_bwd_wgrad_workspace_bytes(*shape, C.byref(nb)) == -22, shape
        assert L.ehm_conv_bwd_wgrad(a, b, 1 << 20, c, d, *shape, 0x50000, 1 << 40, None) == -22, shape
    shape = (2, 7, 7, 64, 128, 3, 1, 1)
    assert L.ehm_conv_bwd_wgrad_workspace_bytes(*shape, C.byref(nb)) == 0 and nb.value >= 4 * 128 * 9 * 64
    for args in ((None, b, 98, c, d, *shape, 0x50000, nb.value), (a, None, 98, c, d, *shape, 0x50000, nb.value), (a, b, 97, c, d, *shape, 0x50000, nb.value),
                 (a, b, 98, None, None, *shape, 0x50000, nb.value), (a, b, 98, c, d, *shape, None, nb.value), (a, b, 98, c, d, *shape, 0x50000, nb.value - 1),
                 (a, b, 98, c, d, *shape, 0x50004, nb.value)):
        assert L.ehm_conv_bwd_wgrad(*args, None) == -22, args
        assert b"bad argument" in L.ehm_last_error()
    assert L.ehm_resnet_stem_backward_workspace_bytes(1, 32, 32, None) == -22
    for n, h, w in ((0, 32, 32), (1, 30, 32), (1, 32, 48), (1, 0, 32)):
        assert L.ehm_resnet_stem_backward_workspace_bytes(n, h, w, C.byref(nb)) == -22
        assert L.ehm_resnet_stem_backward(a, b, c, d, 0x50000, 0x60000, None, None, n, h, w, 0x70000, 1 << 40, None) == -22
    assert L.ehm_resnet_stem_backward_workspace_bytes(1, 32, 32, C.byref(nb)) == 0 and nb.value > 0
    for args in ((None, b, c, d, 0x50000, 0x60000), (a, None, c, d, 0x50000, 0x60000), (a, b, None, d, 0x50000, 0x60000), (a, b, c, None, 0x50000, 0x60000),
                 (a, b, c, d, None, None)):
        assert L.ehm_resnet_stem_backward(*args, None, None, 1, 32, 32, 0x70000, nb.value, None) == -22, args
    assert L.ehm_resnet_stem_backward(a, b, c, d, 0x50000, 0x60000, None, None, 1, 32, 32, 0x70000, nb.value - 1, None) == -22
    assert L.ehm_resnet_stem_backward(a, b, c, d, 0x50000, 0x60000, None, None, 1, 32, 32, None, nb.value, None) == -22


def test_ordered_smpl_backward_is_opt_in_and_rejects_bad_arguments():
    from egohmr_amd import _lib
    from egohmr_amd.smpl import SMPL
    assert SMPL.ordered_backward is False
    L = _lib.lib()
    nb = C.c_int64(-1)
    assert L.ehm_smpl_backward_ordered_workspace_bytes(None, 4, C.byref(nb)) == -22 and b"bad argument" in L.ehm_last_error()
    assert L.ehm_smpl_backward_ordered(None, None, None, None, None, None, None, 0, None, 0, None) == -22 and b"bad argument" in L.ehm_last_error()
    assert L.ehm_smpl_backward(None, None, None, None, None, None, None, 0, None, 0, None) == -22


def test_route_refusals_come_before_any_device_call():
    from egohmr_amd import _lib
    from egohmr_amd.encoders import ResNet50Features
    assert ResNet50Features.grad_params is False
    m = ResNet50Features().eval()
    x = torch.zeros(1, 3, 32, 32)
    m.grad_params, m.hi_only = True, True
    with pytest.raises(_lib.EgoHMRHipError) as e:
        m(x)
    assert str(e.value) == ResNet50Features.GRAD_HI_ONLY
    m.hi_only = False
    with pytest.raises(NotImplementedError) as e:
        m(x.clone().requires_grad_())
    assert str(e.value) == ResNet50Features.GRAD_IMAGE and "image gradient" in str(e.value)
    # the other cases take the route that exists today: a CPU tensor is refused by the package's error, never an autograd route
    with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):
        m(x)
    m.grad_params = False
    with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):
        m(x.clone().requires_grad_())
    m.grad_params = True
    for p in m.parameters():
        p.requires_grad_(False)
    m.hi_only = True                                      # nothing requires grad: no autograd route, so no refusal of its own
    with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):
        m(x)
    with torch.no_grad():
        for p in m.parameters():
            p.requires_grad_(True)
        with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):
            m(x)


@pytest.mark.parametrize("K", [1, 3])
def test_unfold_formulas_match_autograd_through_fold(K):
    from egohmr_amd import trunk_grad
    g = torch.Generator().manual_seed(11 + K)
    conv = torch.nn.Conv2d(6, 10, K, bias=False).double()
    bn = torch.nn.BatchNorm2d(10).double().eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(10, generator=g, dtype=torch.float64) + 0.5)
        bn.bias.copy_(torch.randn(10, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(10, generator=g, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(10, generator=g, dtype=torch.float64) + 0.5)
    gw, gb = torch.randn(10, 6, K, K, generator=g, dtype=torch.float64), torch.randn(10, generator=g, dtype=torch.float64)
    wf, bf = trunk_grad.fold(conv, bn)
    want = torch.autograd.grad((wf * gw).sum() + (bf * gb).sum(), [conv.weight, bn.weight, bn.bias])
    stats = (bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone())
    for got in (trunk_grad.unfold(conv, bn, gw, gb), trunk_grad.unfold(conv, bn, gw.float(), gb.float()),
                R.unfold(conv.weight.detach(), bn.weight.detach(), bn.running_mean, bn.running_var, gw, gb, bn.eps)):
        for a, b in zip(got, want):
            assert a.dtype == torch.float64 and torch.allclose(a, b, rtol=1e-6, atol=1e-7)
    # what is not given is not invented
    assert trunk_grad.unfold(conv, bn, gw, None)[1:] == (None, None) and trunk_grad.unfold(conv, bn, None, gb)[:2] == (None, None)
    assert all(torch.equal(a, b) for a, b in zip(stats, (bn.running_mean, bn.running_var, bn.num_batches_tracked)))
    # the reference's fold is the module's
    wr, br = R.fold(conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    assert torch.equal(wr, wf) and torch.equal(br, bf)


@pytest.mark.parametrize("N,H,W,Ci,Co,K,stride,pad", [(1, 1, 1, 4, 3, 1, 1, 0), (1, 1, 1, 4, 3, 3, 1, 1), (2, 7, 7, 4, 6, 3, 1, 1), (3, 5, 3, 4, 4, 3, 1, 1),
                                                      (2, 8, 8, 4, 4, 3, 2, 1), (1, 7, 7, 4, 4, 3, 2, 1), (2, 8, 8, 4, 6, 1, 2, 0), (1, 7, 7, 4, 6, 1, 2, 0)])
def test_reference_conv_vjp_matches_autograd(N, H, W, Ci, Co, K, stride, pad):
    g = torch.Generator().manual_seed(N * 100 + H * 10 + K + stride)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    w, b, x = r(Co, Ci, K, K).requires_grad_(), r(Co).requires_grad_(), r(N, Ci, H, W).requires_grad_()
    pre = F.conv2d(x, w, b, stride, pad)
    res = r(*pre.shape).requires_grad_()
    y = F.relu(pre + res)
    cot = r(*y.shape)
    want = torch.autograd.grad(y, [w, b, x, res], cot)
    G, gw, gb, gx = R.conv_vjp(w.detach(), x.detach(), y.detach(), cot, stride, pad)
    for a, bb in zip((gw, gb, gx, G), want):
        assert a.shape == bb.shape and torch.allclose(a, bb, rtol=1e-12, atol=1e-12)


def test_reference_pool_route_and_stem_vjp():
    g = torch.Generator().manual_seed(5)
    z = torch.randn(2, 3, 8, 6, generator=g, dtype=torch.float64).requires_grad_()
    gp = torch.randn(2, 3, 4, 3, generator=g, dtype=torch.float64)
    want, = torch.autograd.grad(F.max_pool2d(z, 3, 2, 1), z, gp)
    assert torch.equal(R.pool_route(z.detach(), gp), want)
    # ties: the lowest row-major index of a window wins, in every window that holds the patch; a NaN is the maximum
    zt = torch.zeros(1, 1, 4, 4, dtype=torch.float64)
    zt[0, 0, 1:3, 1:3] = 2.0
    routed = R.pool_route(zt, torch.tensor([[[[1.0, 10.0], [100.0, 1000.0]]]], dtype=torch.float64))
    expect = torch.zeros(4, 4, dtype=torch.float64)
    expect[1, 1] = 1111.0                         # (1,1) is the first maximiser of all four windows
    assert torch.equal(routed[0, 0], expect)
    zt[0, 0, 3, 3] = float("nan")
    routed = R.pool_route(zt, torch.tensor([[[[1.0, 10.0], [100.0, 1000.0]]]], dtype=torch.float64))
    assert float(routed[0, 0, 3, 3]) == 1000.0 and float(routed[0, 0, 1, 1]) == 111.0
    # the stem by hand against autograd
    w, b, img = (torch.randn(64, 3, 7, 7, generator=g, dtype=torch.float64) * 0.1).requires_grad_(), torch.randn(64, generator=g, dtype=torch.float64).requires_grad_(), \
        torch.randn(2, 3, 32, 32, generator=g, dtype=torch.float64)
    zz = F.conv2d(img, w, b, 2, 3)
    pooled = F.max_pool2d(F.relu(zz), 3, 2, 1)
    cot = torch.randn(*pooled.shape, generator=g, dtype=torch.float64)
    want = torch.autograd.grad(pooled, [w, b], cot)
    gw, gb, _ = R.stem_vjp(img, torch.where(pooled.detach() > 0, cot, torch.zeros_like(cot)), zz.detach())
    assert torch.allclose(gw, want[0], rtol=1e-12, atol=1e-12) and torch.allclose(gb, want[1], rtol=1e-12, atol=1e-12)


def test_reference_chain_matches_autograd_and_names_match_the_module():
    from egohmr_amd.encoders import ResNet50Features
    from egohmr_amd import trunk_grad
    m = ResNet50Features()
    assert [n for n, _ in m.named_parameters()] == R.param_names()
    U, Um = R.unit_names(), trunk_grad.units(m)
    assert len(U) == len(Um) == 65 and [u is None for u in U] == [u is None for u in Um]
    for u, um in zip(U, Um):
        if u is not None:
            assert um[0] is m.get_submodule(u[0]) and um[1] is m.get_submodule(u[1]) and um[0].stride[0] == u[2] and um[0].padding[0] == u[3]
    sd, img, gout = R.make_state(1), R.make_image(1, 32, 32, 1), R.make_cotangent(1, 1)
    want, _ = R.autograd_grads(sd, img, gout)
    acts = []
    R.trunk(sd, img, acts)
    got = R.unfold_all(sd, R.trunk_vjp_chain(R.fold_state(sd), img, acts[1:], acts[0], gout))
    assert sorted(got) == sorted(want) and len(got) == 159
    for n in want:
        assert torch.allclose(got[n], want[n], rtol=1e-9, atol=1e-12 * float(want[n].abs().max())), n
    # x2_decode: hi + lo of the split rows
    v = torch.randn(3, 64, dtype=torch.float64) * 5
    hi = v.half()
    lo = (v - hi.double()).half()
    buf = torch.stack([hi.view(3, 2, 32), lo.view(3, 2, 32)], dim=2).reshape(3, 128).view(torch.float32)
    assert buf.shape == (3, 64) and torch.equal(R.x2_decode(buf, 2, 64), (hi.double() + lo.double())[:2])


def test_init_optimizers_with_trunk_grad_is_the_references_list():
    from tests.test_train_step_cpu import _cpu_model
    from egohmr_amd.model import EgoHMR
    assert EgoHMR.trunk_grad is False
    m = _cpu_model()
    ref = (list(m.backbone.parameters()) + list(m.scene_enc.parameters()) + list(m.transl_enc.parameters()) + list(m.beta_layer.parameters()) +
           list(m.diffusion_model.parameters()) + list(m.embed_timestep.parameters()) + list(m.input_process.parameters()))       # egohmr.py:141-144
    nb = len(list(m.backbone.parameters()))
    m.init_optimizers()
    assert len(m.opt_params) == len(ref) - nb and all(a is b for a, b in zip(m.opt_params, ref[nb:]))
    m.trunk_grad = True
    m.init_optimizers()
    assert len(m.opt_params) == len(ref) and all(a is b for a, b in zip(m.opt_params, ref))
    assert all(a is b for a, b in zip(m.optimizer.param_groups[0]["params"], ref)) and isinstance(m.optimizer, torch.optim.AdamW)
    m._set_train_modes()
    assert m.training and not m.backbone.training and all(not mod.training for mod in m.backbone.modules())
    for phrase in ("compute_loss has a backward", "ResNet-50 trunk", "non-local block", "EgoHMR.forward", "frozen_trunk_training", "trunk_grad", "image gradient"):
        assert phrase in EgoHMR.NOT_BUILT


def test_the_committed_seed_keeps_float32_within_a_quarter_of_the_bar():
    e = R.float32_error(E2E_SEED, *E2E_SHAPE)
    print(f"seed {E2E_SEED}: max over the parameter tensors of max|g32 - g64| / max|g64| = {e:.3e} (committed {E2E_F32_ERROR:.3e}; a quarter of the bar {ATOL / 4:.1e})")
    assert e <= ATOL / 4 and E2E_F32_ERROR <= ATOL / 4            # (the float32 run's rounding may differ a little between machines: the bound is what counts)
