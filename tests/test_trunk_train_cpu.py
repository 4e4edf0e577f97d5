"""No GPU: the call surface of the ResNet-50 trunk's train-mode BatchNorm2d route (csrc/bn2d_train.hip, egohmr_amd/trunk_grad.py TrunkTrainFunction,
ResNet50Features.train_batchnorm, EgoHMR._set_train_modes) - exported symbols, argument refusals, route refusals before any device call, the mode rule -
and the hand-written unit VJP of tests/trunk_train_ref.py against torch autograd in float64 (1e-10)."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from tests import trunk_grad_ref as R
from tests import trunk_train_ref as T

NEW = {"ehm_bn2d_train_workspace_bytes": 3, "ehm_bn2d_train_stats": 16, "ehm_bn2d_train_bwd_sums": 13, "ehm_bn2d_train_bwd_zbar": 18,
       "ehm_resnet_stem_preact": 8, "ehm_resnet_stem_route": 7, "ehm_resnet_stem_wgrad": 10}
TOL = 1e-10


def close(a, b):
    return a.shape == b.shape and float((a - b).abs().max()) <= TOL * max(1.0, float(b.abs().max()))


def test_symbols_exported_and_bound():
    from egohmr_amd import _lib
    handle = C.CDLL(_lib.build())
    header = open(os.path.join(_lib.INCLUDE, "egohmr_hip.h")).read()
    for name, nargs in NEW.items():
        assert getattr(handle, name) is not None and name in _lib.PROTOTYPES and name in header
        assert len(_lib.PROTOTYPES[name][1]) == nargs and _lib.PROTOTYPES[name][0] is C.c_int
        assert name not in _lib.VALUE_FUNCTIONS
    assert "bn2d_train.hip" in _lib.SOURCES


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """Every refusal runs before a launch: dummy addresses are never dereferenced."""
    from egohmr_amd import _lib
    L = _lib.lib()
    a, b, c, d, e, f, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
    nb = C.c_int64(-1)
    assert L.ehm_bn2d_train_workspace_bytes(98, 64, None) == -22
    for pixels, Cn in ((1, 64), (0, 64), (98, 48), (98, 0)):                   # fewer than two rows per channel; channels not a multiple of 32
        assert L.ehm_bn2d_train_workspace_bytes(pixels, Cn, C.byref(nb)) == -22
        assert L.ehm_bn2d_train_stats(a, 1, 1 << 20, pixels, Cn, 1e-5, 0.1, b, c, d, None, None, None, ws, 1 << 40, None) == -22
        assert L.ehm_bn2d_train_bwd_sums(a, b, 1, 1 << 20, pixels, Cn, c, d, e, f, ws, 1 << 40, None) == -22
        assert b"bad argument" in L.ehm_last_error()
    assert L.ehm_bn2d_train_workspace_bytes(98, 64, C.byref(nb)) == 0 and nb.value >= 8 * 3 * 64
    ok = (a, 1, 193, 98, 64, 1e-5, 0.1, b, c, d, None, None, None, ws, nb.value)
    for i, bad in ((0, None), (0, a + 4), (1, 2), (2, 97), (5, -1.0), (6, 1.5), (7, None), (8, None), (9, None), (13, None), (13, ws + 8), (14, nb.value - 1)):
        args = list(ok)
        args[i] = bad
        assert L.ehm_bn2d_train_stats(*args, None) == -22, (i, bad)
    ok = (a, b, 1, 193, 98, 64, c, d, e, f, ws, nb.value)
    for i, bad in ((0, None), (1, None), (2, 3), (3, 97), (6, None), (7, None), (8, None), (9, None), (10, None), (11, nb.value - 1)):
        args = list(ok)
        args[i] = bad
        assert L.ehm_bn2d_train_bwd_sums(*args, None) == -22, (i, bad)
    g = 0x80000
    ok = dict(G=a, z=b, x2=1, rows=193, mean=c, invstd=d, gamma=e, gbeta=f, ggamma=ws, scale=None, out=g, N=2, Ho=7, Wo=7, C=64, H=7, W=7)
    for bad in (dict(G=None), dict(z=None), dict(out=None), dict(gamma=None), dict(C=48), dict(N=0), dict(H=15, W=15), dict(H=14, W=9), dict(rows=97), dict(out=a),
                dict(x2=2), dict(N=1, Ho=1, Wo=1, H=1, W=1)):
        k = {**ok, **bad}
        assert L.ehm_bn2d_train_bwd_zbar(k["G"], k["z"], k["x2"], k["rows"], k["mean"], k["invstd"], k["gamma"], k["gbeta"], k["ggamma"], k["scale"], k["out"],
                                         k["N"], k["Ho"], k["Wo"], k["C"], k["H"], k["W"], None) == -22, bad
    for n, h, w in ((0, 32, 32), (1, 30, 32), (1, 32, 48)):
        assert L.ehm_resnet_stem_preact(a, b, c, d, n, h, w, None) == -22
        assert L.ehm_resnet_stem_route(a, b, c, n, h, w, None) == -22
        assert L.ehm_resnet_stem_wgrad(a, b, c, d, n, h, w, ws, 1 << 40, None) == -22
    assert L.ehm_resnet_stem_preact(a, b, c, None, 1, 32, 32, None) == -22 and L.ehm_resnet_stem_route(a, b, a, 1, 32, 32, None) == -22
    assert L.ehm_resnet_stem_wgrad(a, b, None, None, 1, 32, 32, ws, 1 << 40, None) == -22
    assert L.ehm_resnet_stem_wgrad(a, b, c, d, 1, 32, 32, ws, 256 * 148 * 64 * 4 - 1, None) == -22


def test_the_switch_defaults_to_off_and_the_refusals_come_before_any_device_call():
    from egohmr_amd import _lib
    from egohmr_amd.encoders import ResNet50Features
    assert ResNet50Features.train_batchnorm is False
    m = ResNet50Features()
    m.train()
    x = torch.zeros(2, 3, 64, 64)
    # the switch off: .train() is ignored - the route of today, which refuses a CPU tensor with the package's error
    with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):
        m(x)
    m.train_batchnorm = True
    for graph in (False, True):                                               # the no-graph route and the autograd route refuse alike
        m.grad_params = graph
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            m(torch.zeros(1, 3, 32, 32))                                      # layer4 is 1 x 1: one value per channel (torch raises ValueError too)
        m.bn1.momentum = None
        with pytest.raises(NotImplementedError, match="momentum=None"):
            m(x)
        m.bn1.momentum = 0.1
        m.layer3[1].bn2.track_running_stats = False
        with pytest.raises(NotImplementedError, match="track_running_stats=False"):
            m(x)
        m.layer3[1].bn2.track_running_stats = True
        with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):          # nothing left to refuse: the device route, which a CPU tensor cannot take
            m(x)
    m.hi_only = True
    with pytest.raises(_lib.EgoHMRHipError) as e:
        m(x)
    assert str(e.value) == ResNet50Features.GRAD_HI_ONLY
    m.hi_only = False
    with pytest.raises(NotImplementedError) as e:
        m(x.clone().requires_grad_())
    assert str(e.value) == ResNet50Features.GRAD_IMAGE
    m.eval()                                                                  # eval mode: the switch is not consulted
    with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError):
        from egohmr_amd import trunk_grad
        trunk_grad.bn_stats(torch.zeros(1, 64), 1, 64)


def test_set_train_modes_puts_the_backbone_in_train_mode_only_with_both_switches():
    from tests.test_train_step_cpu import _cpu_model
    m = _cpu_model()
    for trunk_grad, train_bn in ((False, False), (True, False), (False, True), (True, True)):
        m.trunk_grad, m.backbone.train_batchnorm = trunk_grad, train_bn
        m._set_train_modes()
        want = trunk_grad and train_bn
        assert m.training and m.backbone.training is want and all(mod.training is want for mod in m.backbone.modules()), (trunk_grad, train_bn)
        m.validation_setup()
        assert not m.training and not m.backbone.training and all(not mod.training for mod in m.backbone.modules())


# ---------------------------------------------------------------------------------------------- the hand-written unit VJP against autograd, float64
def _r(g, *s):
    return torch.randn(*s, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("N,H,W,Ci,Co,K,stride,pad", [(2, 5, 4, 6, 8, 1, 1, 0), (2, 8, 8, 4, 6, 3, 2, 1), (1, 7, 7, 4, 4, 3, 2, 1), (3, 5, 3, 4, 4, 3, 1, 1)])
def test_unit_vjp_matches_autograd(N, H, W, Ci, Co, K, stride, pad):
    g = torch.Generator().manual_seed(N * 100 + H * 10 + K + stride)
    w, gamma, beta, x = _r(g, Co, Ci, K, K).requires_grad_(), (_r(g, Co) * 0.3 + 1).requires_grad_(), _r(g, Co).requires_grad_(), _r(g, N, Ci, H, W).requires_grad_()
    z = F.conv2d(x, w, None, stride, pad)
    res = _r(g, *z.shape)
    y = F.relu(F.batch_norm(z, None, None, gamma, beta, True, 0.0, T.EPS) + res)
    cot = _r(g, *y.shape)
    want = torch.autograd.grad(y, [w, gamma, beta, x, z], cot)
    got = T.unit_vjp(w.detach(), gamma.detach(), x.detach(), z.detach(), y.detach(), cot, stride, pad)
    for a, b in zip((got["wbar"], got["gammabar"], got["betabar"], got["xbar"], got["zbar"]), want):
        assert close(a, b)
    # the running-statistics rule against nn.BatchNorm2d
    bn = torch.nn.BatchNorm2d(Co).double().train()
    bn(z.detach())
    bn(z.detach())
    mean, var, _ = T.batch_stats(z.detach())
    rm, rv = torch.zeros(Co, dtype=torch.float64), torch.ones(Co, dtype=torch.float64)
    for _ in range(2):
        rm, rv = T.running_update(rm, rv, mean, var, N * z.shape[2] * z.shape[3])
    assert close(rm, bn.running_mean) and close(rv, bn.running_var) and int(bn.num_batches_tracked) == 2
    m2, v2, _ = T.row_stats(z.detach().permute(0, 2, 3, 1).reshape(-1, Co))
    assert close(m2, mean) and close(v2, var)


@pytest.mark.parametrize("stride", [1, 2])
def test_projection_pair_vjp_matches_autograd(stride):
    """y = relu(BN3(conv3(a)) + BNd(convd(x))): one gated cotangent goes to both units, each with its own sums."""
    g = torch.Generator().manual_seed(40 + stride)
    N, H, W, Ca, Cx, Co = 2, 6, 6, 4, 6, 8
    Ho = (H - 1) // stride + 1
    a, x = _r(g, N, Ca, Ho, Ho).requires_grad_(), _r(g, N, Cx, H, W).requires_grad_()
    w3, wd = _r(g, Co, Ca, 1, 1).requires_grad_(), _r(g, Co, Cx, 1, 1).requires_grad_()
    g3, b3, gd, bd = [(_r(g, Co) * 0.3 + 1).requires_grad_() for _ in range(4)]
    z3, zd = F.conv2d(a, w3), F.conv2d(x, wd, None, stride)
    y = F.relu(F.batch_norm(z3, None, None, g3, b3, True, 0.0, T.EPS) + F.batch_norm(zd, None, None, gd, bd, True, 0.0, T.EPS))
    cot = _r(g, *y.shape)
    want = torch.autograd.grad(y, [w3, g3, b3, a, wd, gd, bd, x], cot)
    u3 = T.unit_vjp(w3.detach(), g3.detach(), a.detach(), z3.detach(), y.detach(), cot, 1, 0)
    ud = T.unit_vjp(wd.detach(), gd.detach(), x.detach(), zd.detach(), y.detach(), cot, stride, 0)
    got = (u3["wbar"], u3["gammabar"], u3["betabar"], u3["xbar"], ud["wbar"], ud["gammabar"], ud["betabar"], ud["xbar"])
    for p, q in zip(got, want):
        assert close(p, q)
    assert torch.equal(u3["G"], ud["G"])


def test_stem_unit_vjp_matches_autograd():
    g = torch.Generator().manual_seed(9)
    w, gamma, beta = (_r(g, 64, 3, 7, 7) * 0.1).requires_grad_(), (_r(g, 64) * 0.3 + 1).requires_grad_(), _r(g, 64).requires_grad_()
    with torch.no_grad():
        gamma[3] = -0.7                                                       # a negative scale: the arg-max of BN(z) is not that of z
    img = _r(g, 2, 3, 32, 32)
    z = F.conv2d(img, w, None, 2, 3)
    zn = F.batch_norm(z, None, None, gamma, beta, True, 0.0, T.EPS)
    pooled = F.max_pool2d(F.relu(zn), 3, 2, 1)
    cot = _r(g, *pooled.shape)
    want = torch.autograd.grad(pooled, [w, gamma, beta], cot)
    got = T.stem_unit_vjp(w.detach(), gamma.detach(), img, z.detach(), zn.detach(), torch.where(pooled.detach() > 0, cot, torch.zeros_like(cot)))
    for a, b in zip((got["wbar"], got["gammabar"], got["betabar"]), want):
        assert close(a, b)


def test_train_mode_reference_trunk_matches_a_module_of_torch_layers():
    """T.trunk's statistics list and output against the same arithmetic spelled with nn.BatchNorm2d modules in .train() on the stem + first block."""
    sd, img = R.make_state(2), R.make_image(2, 64, 64, 2)
    stats = []
    out = T.trunk(sd, img, stats)
    assert out.shape == (2, 2048) and len(stats) == 53 and stats[0][3] == 2 * 32 * 32 and stats[-1][3] == 2 * 2 * 2
    bn = torch.nn.BatchNorm2d(64).double().train()
    with torch.no_grad():
        bn.weight.copy_(sd["bn1.weight"])
        bn.bias.copy_(sd["bn1.bias"])
        bn.running_mean.copy_(sd["bn1.running_mean"])
        bn.running_var.copy_(sd["bn1.running_var"])
    z = F.conv2d(img, sd["conv1.weight"], None, 2, 3)
    bn(z)
    rm, rv = T.running_update(sd["bn1.running_mean"], sd["bn1.running_var"], stats[0][0], stats[0][1], stats[0][3])
    assert close(rm, bn.running_mean) and close(rv, bn.running_var)
    grads, out2 = T.autograd_grads(sd, img, R.make_cotangent(2, 2))
    assert torch.equal(out2, out.detach()) and len(grads) == 159 and all(bool(torch.isfinite(v).all()) for v in grads.values())
