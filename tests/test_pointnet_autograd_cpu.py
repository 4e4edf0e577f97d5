"""CPU: the float64 restatement of the scene PointNet (tests/pointnet_grad_ref.py) equals oracle.model.resnet_pointnet; the backward that
csrc/pointnet_bwd.hip and egohmr_amd/pointnet_grad.py implement, written out by hand in float64, equals autograd through it - ties resolved to the
lowest row; margin() and the end-to-end seeds; the new entry points are exported, declared and prototyped; the route selection of
ResnetPointnet.forward and the two 'not built' messages."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import model as om
from tests import pointnet_grad_ref as R

H, OUT = 128, 64
# (B, N) -> seed of weights and points with the widest margin() among seeds 0..255 (searched on the CPU: 2.78e-4 at (1, 5), 1.97e-4 at (2, 3))
E2E_SEED = {(1, 5): 34, (2, 3): 55}
E2E_MARGIN = 1e-4                       # about 400 x the forward's 2^-22 store rounding

NEW = {"ehm_pointnet_bwd_workspace_bytes": 4, "ehm_pointnet_pool_argmax": 10, "ehm_pointnet_bwd_scatter": 13, "ehm_pointnet_bwd_gate": 16,
       "ehm_pointnet_bwd_net0": 10, "ehm_pointnet_bwd_lift": 13, "ehm_pointnet_bwd_wgrad_workspace_bytes": 5, "ehm_pointnet_bwd_wgrad": 14}


# ---------------------------------------------------------------------------------------------- 6. the reference itself
def test_restatement_equals_the_oracle():
    for B, N, seed in ((3, 7, 0), (1, 1, 1), (2, 193, 2)):
        sd, p = R.make_weights(H, OUT, seed), R.make_points(B, N, seed)
        out, it = R.forward(sd, p)
        ref = om.resnet_pointnet(sd, p)
        assert float((out - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
        assert len(it["net"]) == 4 and it["net"][0].shape == (B, N, H) and it["x"][1].shape == (B, N, 2 * H) and it["arg"][3].shape == (B, H)
        for net, pooled in zip(it["net"], it["pooled"]):
            assert torch.equal(pooled, net.max(dim=1)[0])


def test_argmax_rule():
    nan = float("nan")
    net = torch.tensor([[[1.0, -3.0, 0.0, nan], [2.0, -1.0, 0.0, 5.0], [2.0, -1.0, 0.0, nan], [2.0, -2.0, -1.0, 7.0]]], dtype=torch.float64)   # [1,4,4]
    assert R.argmax_lowest(net).tolist() == [[1, 1, 0, 0]]


def test_margin_definition_and_the_chosen_seeds():
    for (B, N), seed in E2E_SEED.items():
        sd, p = R.make_weights(H, OUT, seed), R.make_points(B, N, seed)
        m = R.margin(sd, p)
        print(f"margin(B={B}, N={N}, seed={seed}) = {m:.3e}")
        assert m >= E2E_MARGIN
    # by hand on a case small enough to read: a ReLU input 1e-3 of its tensor's maximum, or a pool gap of 1e-3, bounds the margin
    sd, p = R.make_weights(H, OUT, 3), R.make_points(1, 4, 3)
    _, it = R.forward(sd, p)
    m = R.margin(sd, p)
    expect = min(float(v.abs().min() / v.abs().max()) for v in [it["net0"]] + it["x"] + it["h"] + [it["pooled"][3]])
    for net in it["net"]:
        s = net.sort(dim=1, descending=True)[0]
        expect = min(expect, float((s[:, 0] - s[:, 1]).min() / net.abs().max()))
    assert m == pytest.approx(expect, rel=1e-12) and 0 < m < 1
    assert R.margin(sd, R.make_points(1, 1, 3)) > 0                      # N = 1: no pool gap to take


@pytest.mark.parametrize("zero_fc1", [False, True])
def test_backward_by_hand_equals_autograd_with_a_tie(zero_fc1):
    B, N = 3, 7
    sd, p = R.make_weights(H, OUT, 5, zero_fc1=zero_fc1), R.make_points(B, N, 5)
    p[1, 4] = p[1, 2]                                                     # two identical points: every column of body 1 that peaks there is a tie
    gout = torch.from_numpy(np.random.Generator(np.random.PCG64(9)).normal(size=(B, OUT)))
    out, it, pbar, g = R.autograd_reference(sd, p, gout)
    tied = sum(int(((a[1] == 2)).sum()) for a in it["arg"])
    assert tied > 0 and all(int((a[1] == 4).sum()) == 0 for a in it["arg"])        # resolved to the lowest row
    pb2, g2 = R.backward_by_hand(sd, p, it, gout)
    assert float((pbar - pb2).abs().max()) <= 1e-10 * float(pbar.abs().max())
    assert float(pbar[1, 4].abs().max()) == 0 and float(pbar[1, 2].abs().max()) > 0      # a point reaches the output through the pools alone: the tie's loser gets nothing
    for k in R.PARAM_NAMES:
        assert float((g[k] - g2[k]).abs().max()) <= 1e-10 * max(float(g[k].abs().max()), 1e-300), k


# ---------------------------------------------------------------------------------------------- 7. surface and messages
@pytest.fixture(scope="module")
def L():
    from egohmr_amd import _lib
    _lib.build()
    return _lib.lib()


def test_symbols_are_exported_declared_and_prototyped(L):
    from egohmr_amd import _lib
    hdr = open(os.path.join(_lib.INCLUDE, "egohmr_hip.h")).read()
    for name, arity in NEW.items():
        assert hasattr(L, name), name
        assert name in _lib.PROTOTYPES and name not in _lib.VALUE_FUNCTIONS
        assert _lib.PROTOTYPES[name][0] is ctypes.c_int
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared in include/egohmr_hip.h"
        assert len(m.group(1).split(",")) == arity == len(_lib.PROTOTYPES[name][1]), name
        assert callable(getattr(_lib.api(), name))
    assert "pointnet_bwd.hip" in _lib.SOURCES


def test_entries_refuse_bad_arguments_before_any_device_call(L):
    p = 0x10000                                                           # never dereferenced on the host
    nb = ctypes.c_int64(-1)
    assert L.ehm_pointnet_bwd_workspace_bytes(2, 192, 128, None) == -22 and b"bad argument" in L.ehm_last_error()
    assert L.ehm_pointnet_bwd_workspace_bytes(2, 191, 128, ctypes.byref(nb)) == -22 and nb.value == -1      # rows: whole 192-row tiles
    assert L.ehm_pointnet_bwd_workspace_bytes(2, 192, 96, ctypes.byref(nb)) == -22                          # columns: multiples of 128
    assert L.ehm_pointnet_bwd_workspace_bytes(2, 384, 256, ctypes.byref(nb)) == 0 and nb.value >= (2 * 2 + 2) * 256 * 4 * 4
    assert L.ehm_pointnet_pool_argmax(None, 1, p, 1, 5, 192, 128, p, 1 << 30, None) == -22
    assert L.ehm_pointnet_pool_argmax(p, 1, p, 1, 193, 192, 128, p, 1 << 30, None) == -22                   # N > N_padded
    assert L.ehm_pointnet_pool_argmax(p, 1, p, 1, 5, 192, 128, p, 16, None) == -22                          # workspace too small
    assert L.ehm_pointnet_bwd_scatter(None, None, p, p, p, p, 1, 5, 192, 128, p, 1 << 30, None) == -22
    assert L.ehm_pointnet_bwd_gate(None, p, 1, None, None, None, p, None, None, 1, 5, 192, 128, None, 0, None) == -22
    assert L.ehm_pointnet_bwd_gate(p, p, 1, None, None, None, p + 2, None, None, 1, 5, 192, 128, None, 0, None) == -22   # 16-byte alignment
    assert L.ehm_pointnet_bwd_wgrad_workspace_bytes(300, 192, 128, 256, ctypes.byref(nb)) == 0 and nb.value == 150 * 128 * 256 * 4     # at most 256 runs
    assert L.ehm_pointnet_bwd_wgrad(p, p, 1, 0, p, 64, 1, 5, 192, 128, 128, p, 1 << 30, None) == -22         # ld_out < Ca
    assert L.ehm_pointnet_bwd_wgrad(p, p, 1, 0, p, 128, 1, 5, 192, 128, 128, p, 16, None) == -22             # workspace too small
    assert L.ehm_pointnet_bwd_net0(p, p, p, None, None, 1, 5, 192, 128, None) == -22
    assert L.ehm_pointnet_bwd_lift(p, p, None, None, None, p, 1, 5, 192, 128, p, 1 << 30, None) == -22      # pbar needs the weights


def _net():
    from egohmr_amd.encoders import ResnetPointnet
    return ResnetPointnet(out_dim=OUT, hidden_dim=H)


def test_route_selection_and_cpu_refusal():
    from egohmr_amd import _lib
    from egohmr_amd.encoders import ResnetPointnet
    from egohmr_amd.pointnet_grad import PARAM_NAMES
    assert ResnetPointnet.grad_params is False
    m = _net()
    assert PARAM_NAMES == R.PARAM_NAMES
    gp = m.grad_parameters()
    assert len(gp) == 24 and {id(q) for q in gp} == {id(q) for q in m.parameters()}
    assert [id(q) for q in gp] == [id(m.get_parameter(n)) for n in R.PARAM_NAMES]
    p = torch.zeros(2, 5, 3)
    assert not m._wants_grad(p)                                           # parameters require grad by default: still today's route
    assert m._wants_grad(p.clone().requires_grad_())
    with torch.no_grad():
        assert not m._wants_grad(p.clone().requires_grad_())
    m.grad_params = True
    assert m._wants_grad(p)
    with torch.no_grad():
        assert not m._wants_grad(p)
    for q in m.parameters():
        q.requires_grad_(False)
    assert not m._wants_grad(p) and m._wants_grad(p.clone().requires_grad_())
    # a CPU tensor is refused first, whatever the flags
    for gpar, hi, rg in ((False, False, False), (True, False, True), (True, True, True), (False, True, True)):
        m.grad_params, m.hi_only = gpar, hi
        with pytest.raises(_lib.EgoHMRHipError, match="ResnetPointnet runs on the HIP kernels only \\(got a CPU tensor\\); there is no CPU path"):
            m(p.clone().requires_grad_(rg))
    assert "hi_only" in ResnetPointnet.GRAD_HI_ONLY


def test_not_built_messages_name_what_is_left():
    from egohmr_amd.diffusion import GaussianDiffusion
    from egohmr_amd.model import EgoHMR
    msgs = []
    for call in (lambda: EgoHMR.training_step(None), lambda: GaussianDiffusion.training_losses(None, None, None, None)):
        with pytest.raises(NotImplementedError, match="compute_loss has a backward") as e:
            call()
        msgs.append(str(e.value))
    for s in msgs:
        assert "ResNet-50 trunk" in s and "non-local block" in s and "EgoHMR.forward" in s
        assert "conditioning encoders" not in s and "encoders' backward" not in s
