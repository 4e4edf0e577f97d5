"""GPU (MI355X): ModulatedGCN(nonlocal_layer=True) with nonlocal_grad end to end - in_dim 70, hid 64, one block, grad_params - in eval and train mode against
the float64 restatement of tests/nonlocal_ref.py (pinned to the reference's own module by tests/test_nonlocal_grad_cpu.py), at the bars of
tests/test_gpu_gcn_train.py: the forward at 5e-5 max(1, max|ref|), gradients at the VJP bar (atol = 2e-4 max|ref|, rtol = 2e-3; the gradients that are zero
in exact arithmetic as tests/test_gpu_nonlocal_grad.py holds them), W.1's running statistics at rtol 1e-5 + atol 1e-6 sqrt(var).  The forward is the
module's own float32 one, so the seeds are chosen on the CPU such that every ReLU pre-activation of the float64 reference has |v| >= GATE_MARGIN max|v| of
its conv (asserted on the reference alone): no gate flips.  Then what is computed when (needs_input_grad, frozen parameters, the no-grad forward), and
data parallel: a world of one bit-equal to no sync, two gloo ranks on ragged shards against one process on the whole batch."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nonlocal_dp_rank as RK  # noqa: E402
import nonlocal_ref as NR  # noqa: E402
from test_gpu_nonlocal_grad import VJP_ATOL_REL, check_forward, vjp_ratio  # noqa: E402

pytestmark = pytest.mark.gpu

GATE_MARGIN = 1e-4
# searched on the CPU over seeds 0..255 of NR.module_state(seed, bodies=2) with NR.modulated_gcn's BatchNorm outputs: eval mode 12, 48, 52, 87, 117, 148,
# 217, 222 meet GATE_MARGIN (52 the widest, 1.6e-4); train mode 31, 68, 93, 145, 156, 193, 197, 207, 218, 228, 240 (68 and 156 the widest, 1.5e-4)
E2E_SEED = {"eval": 52, "train": 68}
DP_COUNTS = [2, 1]
DP_SEED = 68                  # (three bodies: the data-parallel case compares two float32 routes with each other, no gate margin is needed)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def adj64():
    from oracle import model as om
    return om.smpl_adjacency(torch.float64)


@pytest.fixture(scope="module")
def refs(adj64):
    """Per mode: E2E_SEED's state, input, cotangent and the float64 reference run (computed once on the CPU, shared, left unchanged)."""
    out = {}
    for mode, seed in E2E_SEED.items():
        sd, x = NR.module_state(seed, bodies=2)
        cot = RK.cotangent(2).double()
        out[mode] = dict(sd=sd, x=x, cot=cot, ref=NR.run(sd, x, cot, adj64, 1, train=mode == "train"))
    return out


def check_module_grads(tag, got, ref, train):
    """got / ref: {state-dict name: gradient} + 'x'.  The VJP bar per tensor; zero-in-exact-arithmetic gradients on the scale of their un-cancelled partner."""
    partner = {NR.NL + "phi.bias": NR.NL + "theta.bias"}
    if train:
        partner.update({NR.NL + "W.0.bias": NR.NL + "W.1.bias", NR.NL + "g.bias": NR.NL + "W.1.bias"})
        partner.update({k: k.replace("gconv.bias", "bn.bias") for k in ref if k.endswith("gconv.bias") and not k.startswith("gconv_output")})
    worst = {}
    for k, r in ref.items():
        if k in partner:
            scale = float(ref[partner[k]].abs().max())
            assert float(r.abs().max()) <= 1e-9 * scale, (k, "the reference's own is not zero to rounding")
            worst[k] = float(got[k].double().abs().max()) / (VJP_ATOL_REL * scale)
        else:
            worst[k] = vjp_ratio(got[k].cpu(), r)
    print(f"{tag}: err / VJP bar " + ", ".join(f"{k.replace('non_local.', 'nl.')} {v:.1e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_module_vs_fp64(dev, refs, mode, precision):
    c = refs[mode]
    ref = c["ref"]
    margin = NR.gate_margin(ref)
    print(f"gate margin of seed {E2E_SEED[mode]} ({mode}): min|v|/max|v| = {margin:.2e}")
    assert margin >= GATE_MARGIN
    train = mode == "train"
    m = RK.build(c["sd"], dev, precision, train)
    tag = f"[ModulatedGCN + non-local {mode} {precision}]"
    runs = [RK.step(m, c["x"].float().to(dev), c["cot"].float().to(dev)) for _ in range(2)]
    for k in runs[0]["grads"]:
        assert torch.equal(runs[0]["grads"][k], runs[1]["grads"][k]), f"{k} differs between two identical calls"
    assert torch.equal(runs[0]["gx"], runs[1]["gx"]) and torch.equal(runs[0]["out"], runs[1]["out"])
    got = runs[0]
    assert sorted(got["grads"]) == sorted(ref["grads"]) and len(got["grads"]) == 32
    check_forward(tag, got["out"], ref["out"])
    check_module_grads(tag, dict(got["grads"], x=got["gx"]), dict(ref["grads"], x=ref["gx"]), train)
    bn = m.non_local.W[1]
    if train:
        # the reference ran once; the module twice on the same input: the second update from the first one's result, in float64
        assert int(bn.num_batches_tracked) == 2
        r1m, r1v = ref["sd"][NR.NL + "W.1.running_mean"], ref["sd"][NR.NL + "W.1.running_var"]
        bm, bv = (r1m - 0.9 * c["sd"][NR.NL + "W.1.running_mean"]) / 0.1, (r1v - 0.9 * c["sd"][NR.NL + "W.1.running_var"]) / 0.1
        want_m, want_v = 0.9 * r1m + 0.1 * bm, 0.9 * r1v + 0.1 * bv
        atol = 1e-6 * want_v.sqrt()
        for have, want, name in ((bn.running_mean, want_m, "running_mean"), (bn.running_var, want_v, "running_var")):
            err = (have.double().cpu() - want).abs()
            print(f"{tag} W.1.{name}: max err / (atol + rtol |ref|) = {float((err / (atol + 1e-5 * want.abs())).max()):.2e}")
            assert bool((err <= atol + 1e-5 * want.abs()).all()), name
    else:
        assert int(bn.num_batches_tracked) == 0 and torch.equal(bn.running_var.double().cpu(), c["sd"][NR.NL + "W.1.running_var"])


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_what_is_computed_when(dev, refs, mode):
    c = refs[mode]
    train = mode == "train"
    m = RK.build(c["sd"], dev, "f16x3", train)
    x, cot = c["x"].float().to(dev), c["cot"].float().to(dev)
    m.eval()
    with torch.no_grad():
        before = m(x).clone()
    m.train(train)
    # only x.requires_grad: every parameter's .grad stays None
    m.grad_params = False
    xg = x.clone().requires_grad_(True)
    m(xg).backward(cot)
    assert xg.grad is not None and all(p.grad is None for p in m.parameters())
    gx_only = xg.grad.clone()
    # a frozen block parameter (and a frozen conv parameter) receives none; the others do, and x's gradient has the same bits
    m.grad_params = True
    frozen = (m.non_local.theta.weight, m.non_local.W[1].bias, m.gconv_output.M)
    for p in frozen:
        p.requires_grad_(False)
    xg = x.clone().requires_grad_(True)
    m(xg).backward(cot)
    assert all(p.grad is None for p in frozen)
    assert all(p.grad is not None for p in m.grad_parameters() if p.requires_grad)
    assert torch.equal(xg.grad, gx_only)
    full = RK.step(RK.build(c["sd"], dev, "f16x3", train), x, cot)
    names = {id(p): n for n, p in m.named_parameters()}
    for p in m.grad_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad.cpu(), full["grads"][names[id(p)]]), names[id(p)]
    # parameters alone (x does not require grad)
    for p in m.parameters():
        p.grad = None
    m(x).backward(cot)
    assert m.non_local.g.weight.grad is not None and torch.equal(m.non_local.g.weight.grad.cpu(), full["grads"]["non_local.g.weight"])
    # the no-grad eval forward after all that: the parameters did not move; under train mode the running statistics did
    m.eval()
    with torch.no_grad():
        after = m(x)
    if train:
        assert not torch.equal(before, after)
        m2 = RK.build(c["sd"], dev, "f16x3", False)
        with torch.no_grad():
            assert torch.equal(m2(x), before)
    else:
        assert torch.equal(before, after)
    assert before.grad_fn is None and after.grad_fn is None


def test_eval_forward_of_both_routes_agrees(dev, refs):
    """The autograd route's forward (unfolded BatchNorm, one launch per conv) against the inference route (folded GEMM, chained convs): the same function, two
    float32 roundings of it - both within the forward bar of the float64 reference."""
    c = refs["eval"]
    m = RK.build(c["sd"], dev, "f16x3", False)
    x = c["x"].float().to(dev)
    with torch.no_grad():
        plain = m(x)
    with_grad = m(x.clone().requires_grad_(True))
    assert plain.grad_fn is None and with_grad.grad_fn is not None
    check_forward("[inference route]", plain.cpu(), c["ref"]["out"])
    check_forward("[autograd route]", with_grad.detach().cpu(), c["ref"]["out"])


# ---------------------------------------------------------------------------------------------- data parallel
def test_world_of_one_is_bit_equal_to_no_sync(dev, refs):
    from egohmr_amd import dist as edist
    c = refs["train"]
    x, cot = c["x"].float().to(dev), c["cot"].float().to(dev)
    a = RK.step(RK.build(c["sd"], dev), x, cot)
    m = RK.build(c["sd"], dev)
    m.stat_sync = edist.StatSync([2], 0)
    b = RK.step(m, x, cot)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["gx"], b["gx"])
    for what in ("grads", "buffers"):
        differ = sorted(k for k in a[what] if not torch.equal(a[what][k], b[what][k]))
        assert not differ, (what, differ)
    m.stat_sync = edist.StatSync([3], 0)                      # counts that do not match the input are refused
    with pytest.raises(ValueError, match="stat_sync counts"):
        m(x)


def run_ranks(tmp_path, seed, counts, precision="f16x3", limit=120):
    """One fresh process per rank, each under its own time limit; the parent checks every exit status.  -> what the ranks saved, in rank order."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(len(counts)):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(len(counts)),
                   EGOHMR_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable, RK.__file__, str(seed), json.dumps(counts), precision,
                                       str(tmp_path / f"rank{r}.pt")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = [p.communicate()[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, (p.returncode, log.decode()[-3000:])
    return [torch.load(tmp_path / f"rank{r}.pt") for r in range(len(counts))]


def test_two_ranks_on_ragged_shards_equal_one_process(dev, tmp_path):
    """Ragged counts [2, 1] on the bare ModulatedGCN: the ranks' output rows put together, W.1's (and every conv's) running statistics and the rank-summed
    gradients against ONE process on the whole batch - two float32 routes of the same sums, at the VJP bar, the forward bar and the running statistics'
    bar; the running statistics bit-equal between the ranks (every rank merges the same gathered moments in the same order)."""
    res = run_ranks(tmp_path, DP_SEED, DP_COUNTS)
    B = sum(DP_COUNTS)
    sd, x = NR.module_state(DP_SEED, bodies=B)
    whole = RK.step(RK.build(sd, dev), x.float().to(dev), RK.cotangent(B).to(dev))
    tag = f"[non-local data parallel {DP_COUNTS[0]}+{DP_COUNTS[1]}]"
    check_forward(tag, torch.cat([r["out"] for r in res]), whole["out"].double())
    summed = {k: sum(r["grads"][k].double() for r in res) for k in whole["grads"]}
    ref = {k: v.double() for k, v in whole["grads"].items()}
    worst = {}
    for k, r in ref.items():
        if float(r.abs().max()) == 0.0:                       # the exact zeros of a bias in front of a train-mode BatchNorm: on every rank too
            assert all(float(q["grads"][k].abs().max()) == 0.0 for q in res), k
            continue
        zero_partner = {NR.NL + "phi.bias": NR.NL + "theta.bias", NR.NL + "g.bias": NR.NL + "W.1.bias", NR.NL + "W.0.bias": NR.NL + "W.1.bias"}.get(k)
        if zero_partner is not None:                          # zero to rounding on both sides: against the scale of the un-cancelled partner
            scale = float(ref[zero_partner].abs().max())
            worst[k] = max(float(summed[k].abs().max()), float(r.abs().max())) / (VJP_ATOL_REL * scale)
        else:
            worst[k] = vjp_ratio(summed[k], r)
    worst["x"] = vjp_ratio(torch.cat([r["gx"] for r in res]), whole["gx"].double())
    print(f"{tag}: rank-summed gradients, err / VJP bar " + ", ".join(f"{k.replace('non_local.', 'nl.')} {v:.1e}" for k, v in worst.items()))
    assert not {k: v for k, v in worst.items() if not v <= 1.0}
    stats = [k for k in whole["buffers"] if "running_" in k]
    assert len(stats) == 8 and NR.NL + "W.1.running_mean" in stats
    for k in stats:
        want = whole["buffers"][k].double()
        var = whole["buffers"][k.replace("running_mean", "running_var")].double()
        for r in res:
            err = (r["buffers"][k].double() - want).abs()
            assert bool((err <= 1e-6 * var.sqrt() + 1e-5 * want.abs()).all()), (k, r["rank"], float(err.max()))
        assert torch.equal(res[0]["buffers"][k], res[1]["buffers"][k]), k
        assert not torch.equal(want.float(), sd[k].float()), k
    print(f"{tag}: {len(stats)} running statistics within rtol 1e-5 + atol 1e-6 sqrt(var) of one process, bit-equal between the ranks")
    for r in res:
        assert all(int(v) == 1 for k, v in r["buffers"].items() if "num_batches" in k)
