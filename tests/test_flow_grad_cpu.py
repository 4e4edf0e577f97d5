"""CPU: the references of the flow's backward (tests/flow_grad_ref.py) are right - the torch restatement equals flow_ref, its gradients equal finite
differences, the differentiable fold equals the numpy fold - and the parts of the autograd route that need no GPU: the C entries, the route
selection, and the seed conditions test_gpu_flow_grad.py relies on (asserted on the references alone)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from egohmr_amd import synthetic as syn
from tests import flow_grad_ref as gr
from tests import flow_ref as fr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = dict(with_focal_length=True, with_bbox_info=True, with_cam_center=True)
B, S = 2, 2
# PCG64(seed) inputs (flow_grad_ref.inputs), chosen among seeds 0 .. 15 for the widest margin of the float64 run's ReLU inputs over their own error
# bars (and, sampling, a smallest sine >= 0.1): forward seed 0 has min |v| / bar = 6.1; sampling seed 8 has 4.9 at a smallest sine of 0.12
SEEDS = {False: 0, True: 8}
MIN_SINE = 0.1


@pytest.fixture(scope="module")
def case():
    sd = syn.make_stage1_flow_state_dict(10, **FLAGS)
    return sd, syn.stage1_context_dim(**FLAGS)


@pytest.mark.parametrize("sampling", [False, True])
def test_restatement_equals_flow_ref(case, sampling):
    sd, ctx = case
    c, rows = gr.inputs(SEEDS[sampling], B, S, ctx)
    r = gr.run(sd, c, rows, S, sampling, torch.float64)
    cr, rr = np.repeat(c, S, 0), rows.reshape(-1, 144)
    if sampling:
        x, lp = fr.sample_and_log_prob(sd, rr, cr)
        want = (x, lp, fr.rot6d_prohmr(x).reshape(-1, 24, 3, 3))
    else:
        want = fr.log_prob(sd, rr, cr)
    for got, w in zip(r["out"], want):
        assert np.abs(got - w).max() <= 1e-12 * max(1.0, np.abs(w).max())


@pytest.mark.parametrize("sampling", [False, True])
def test_seed_conditions_hold_on_the_references(case, sampling):
    """Every ReLU input of the float64 run lies farther from zero than its tensor's own error bar, so a device forward inside its bar takes the
    reference's masks; the sampled joints are well conditioned."""
    sd, ctx = case
    c, rows = gr.inputs(SEEDS[sampling], B, S, ctx)
    r64, r32 = gr.run(sd, c, rows, S, sampling, torch.float64), gr.run(sd, c, rows, S, sampling, torch.float32)
    assert len(r64["relu"]) == 16
    margin = gr.relu_margin(r64, r32)
    print(f"sampling = {sampling}: min |v| / bar = {margin:.2f}")
    assert margin > 1.0
    if sampling:
        assert gr.sines(r64["out"][0]).min() >= MIN_SINE


@pytest.mark.parametrize("sampling", [False, True])
def test_reference_gradients_equal_finite_differences(case, sampling):
    sd, ctx = case
    c, rows = gr.inputs(SEEDS[sampling], B, S, ctx)
    g = np.random.Generator(np.random.PCG64(5))
    shapes = [(B * S, 144), (B * S,), (B * S, 24, 3, 3)] if sampling else [(B * S,), (B * S, 144)]
    cots = [g.normal(size=s) for s in shapes]
    grads = gr.run(sd, c, rows, S, sampling, torch.float64, cots)["grads"]
    p = gr.tensors(sd, torch.float64)
    ct, rt = torch.tensor(c, dtype=torch.float64), torch.tensor(rows.reshape(-1, 144), dtype=torch.float64)
    tc = [torch.tensor(a) for a in cots]

    def value():
        if sampling:
            x, lp = gr.sample_and_log_prob(p, rt, ct, S)
            out = (x, lp, gr.rot6d_prohmr(x).reshape(-1, 24, 3, 3))
        else:
            out = gr.log_prob(p, rt, ct, S)
        return float(sum((o * a).sum() for o, a in zip(out, tc)))

    kinds = {}                                                     # one tensor of each parameter kind (block 1), and the three inputs
    for k in p:
        if p[k].dtype == torch.float64 and re.match(re.escape(gr.PREFIX) + r"[345]\.", k):
            kinds.setdefault(re.sub(r"\d+", "#", k), k)
    assert len(kinds) == 6 + 8
    targets = [(k, p[k]) for k in kinds.values()] + [("rows", rt), ("ctx", ct)]
    for name, t in targets:
        flat, gflat = t.reshape(-1), grads[name].reshape(-1)
        for i in g.choice(flat.numel(), size=3, replace=False):
            v0, h = float(flat[i]), 1e-5
            flat[i] = v0 + h
            up = value()
            flat[i] = v0 - h
            dn = value()
            flat[i] = v0
            fd = (up - dn) / (2 * h)
            assert abs(fd - gflat[i]) <= 1e-6 * max(1.0, abs(fd)), (name, int(i), fd, float(gflat[i]))


def test_torch_fold_equals_the_numpy_fold_and_its_gradients_equal_finite_differences(case):
    from egohmr_amd import flow_grad as fg
    from egohmr_amd.stage1 import GlowFlow
    sd, ctx = case
    f = GlowFlow(ctx)
    f.load_state_dict({k[len("flow.flow."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    tr = f._transform._transforms
    total = 0.0
    for l in range(4):
        a = gr.affine_of(sd, l)
        module = GlowFlow.fold(tr[3 * l], tr[3 * l + 1])           # what GlowFlow._weights folds with (numpy)
        plain = gr.fold_numpy(*a)
        t = fg.fold(*[torch.tensor(v, dtype=torch.float64) for v in a])
        for m, q, u in zip(module[:3], plain[:3], t[:3]):
            assert np.abs(m - q).max() <= 1e-12 and np.abs(m - u.numpy()).max() <= 1e-12
        assert module[3] == plain[3] == float(t[3])                # log|det|: bit-identical
        total += module[3]
    assert abs(total - fr.logdet(sd)) <= 1e-12 * abs(total)
    # gradients of a random functional of (A, c, Ainv, logdet), block 2
    g = np.random.Generator(np.random.PCG64(9))
    leaves = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in gr.affine_of(sd, 2)]
    cots = [torch.tensor(g.normal(size=s)) for s in ((144, 144), (144,), (144, 144), ())]
    value = lambda: sum((o * q).sum() for o, q in zip(fg.fold(*leaves), cots))
    grads = torch.autograd.grad(value(), leaves)
    with torch.no_grad():
        for leaf, gl in zip(leaves, grads):
            for i in g.choice(leaf.numel(), size=3, replace=False):
                v0, h = float(leaf[i]), 1e-6
                leaf[i] = v0 + h
                up = float(value())
                leaf[i] = v0 - h
                dn = float(value())
                leaf[i] = v0
                fd = (up - dn) / (2 * h)
                assert abs(fd - float(gl[i])) <= 1e-6 * max(1.0, abs(fd)), (int(i), fd, float(gl[i]))


def test_new_entries_are_declared_exported_and_bound():
    from egohmr_amd import _lib
    _lib.build()
    L = _lib.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "egohmr_hip.h")).read(), flags=re.S)
    for name in ("ehm_flow_wgrad", "ehm_flow_reduce", "ehm_flow_finish_backward"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name) and name in _lib.PROTOTYPES and hasattr(_lib.api(), name)
    assert (_lib.FLOW_PRO_GATE, _lib.FLOW_EPI_MASK, _lib.FLOW_EPI_MASK_ADD, _lib.FLOW_EPI_ADD) == (4, 5, 6, 7)
    for k, v in (("EHM_FLOW_PRO_GATE", 4), ("EHM_FLOW_EPI_MASK", 5), ("EHM_FLOW_EPI_MASK_ADD", 6), ("EHM_FLOW_EPI_ADD", 7)):
        assert re.search(rf"\b{k} = {v}\b", text), k
    # the refusals run before anything is launched (dummy addresses)
    wg = dict(G=0x10000, gather_g=None, item=None, X=0x20000, gather_x=None, x_shift=None, out=0x30000, R=4, Cg=72, Ca=1024, S=1, ldg=72, ldx=1024,
              ld_item=0, ld_out=1024, act=0, alpha=1.0, beta=0.0)
    assert L.ehm_flow_wgrad(None, None) == -22
    for bad in (dict(G=None), dict(X=None), dict(out=None), dict(R=0), dict(S=0), dict(ld_out=512), dict(ldg=64), dict(ldx=512), dict(act=2),
                dict(out=0x10000), dict(item=0x40000, ld_item=64)):
        assert L.ehm_flow_wgrad(C.byref(_lib.FlowWgradDesc(**{**wg, **bad})), None) == -22, bad
    rd = dict(G=0x10000, gather=None, U2=None, item=None, out=0x30000, R=4, N=1024, S=2, ldg=1024, ldu=0, ld_item=0, ld_out=1024, mode=0, scale=1.0)
    assert L.ehm_flow_reduce(None, None) == -22
    for bad in (dict(G=None), dict(out=None), dict(R=0), dict(mode=3), dict(ldg=512), dict(mode=1, ld_out=512), dict(mode=2),
                dict(mode=2, U2=0x20000, ldu=1024), dict(mode=1, gather=0x50000)):
        assert L.ehm_flow_reduce(C.byref(_lib.FlowReduceDesc(**{**rd, **bad})), None) == -22, bad
    fb = L.ehm_flow_finish_backward
    assert fb(None, None, None, None, None, None, None, None, None, None, 4, None) == -22        # nothing asked for
    assert fb(0x10000, None, None, 0x20000, None, None, None, None, None, None, 4, None) == -22   # dz without z
    assert fb(None, None, None, None, 0x20000, None, None, None, None, None, 4, None) == -22      # the sum without the cotangent
    assert fb(None, None, None, None, None, None, 0x10000, None, None, 0x20000, 4, None) == -22   # dpose without the pose
    assert fb(0x10000, 0x20000, None, 0x30000, None, None, None, None, None, None, 0, None) == -22
    # the new operands of ehm_flow_gemm
    gm = dict(X=0x10000, gather=None, W=0x20000, bias=None, pro_scale=None, pro_shift=None, item=None, scatter=None, Y=0x30000, R=5, K=1024, N=1024, S=1,
              ldx=1024, ldw=1024, ldy=1024, ld_item=0, prologue=0, epilogue=0)
    for bad in (dict(prologue=4), dict(prologue=4, item=0x40000, ld_item=512), dict(epilogue=5), dict(epilogue=5, mask=0x30000, ld_mask=1024),
                dict(epilogue=6, mask=0x40000, ld_mask=1024), dict(epilogue=7), dict(epilogue=7, add=0x40000, ld_add=512), dict(epilogue=8),
                dict(add=0x40000, ld_add=1024), dict(aux=0x40000), dict(N=72, ldw=72), dict(N=72, ldw=64, w_window=1)):
        assert L.ehm_flow_gemm(C.byref(_lib.FlowGemmDesc(**{**gm, **bad})), None) == -22, bad


def test_route_selection_without_a_gpu(case):
    from egohmr_amd import flow_grad as fg
    from egohmr_amd.stage1 import GlowFlow
    f = GlowFlow(case[1])
    assert GlowFlow.grad_params is False and all(p.requires_grad for p in f.parameters())
    x, xg = torch.zeros(1, 1, 144), torch.zeros(1, 1, 144, requires_grad=True)
    assert not fg.wants_grad(f, x, None)                           # nothing requires grad
    assert not fg.wants_grad(f, x)                                 # grad_params = False and only parameters require grad
    assert fg.wants_grad(f, x, xg) and fg.wants_grad(f, None, xg)
    with torch.no_grad():
        assert not fg.wants_grad(f, xg)
    f.grad_params = True
    assert fg.wants_grad(f, x)
    with torch.no_grad():
        assert not fg.wants_grad(f, x)
    f.requires_grad_(False)
    assert not fg.wants_grad(f, x) and fg.wants_grad(f, xg)
    # the refusals of the autograd route that need no device: BatchNorm, CPU tensors
    from egohmr_amd import _lib
    with pytest.raises(_lib.EgoHMRHipError, match="BatchNorm of the flow's ResidualNet is not differentiated"):
        GlowFlow(case[1], batch_norm=True).log_prob(xg, torch.zeros(1, case[1]))
    with pytest.raises(_lib.EgoHMRHipError, match="CPU tensor"):
        GlowFlow(case[1]).log_prob(xg, torch.zeros(1, case[1]))
    # no parameter of the flow is left without a gradient slot, and the buffers get none
    names = [n for n, _ in GlowFlow(case[1]).named_parameters()]
    assert len(names) == 4 * (6 + 16) and not any("_features" in n for n in names)
