"""GPU (MI355X): EgoHMR.data_parallel - two ranks (gloo, a fresh process each, sharing the one GPU: three processes with the GPU open) take the optimizer
step of one process on the whole batch.  The model and batch are those of tests/test_gpu_train_step.py (tests/dp_common.py); the rank processes run
tests/dp_common.py as a script and leave what they computed in a file.

E1  frozen trunk, the denoiser on batch statistics, shards 2 + 2 and 3 + 1: every rank's reduced gradients against the float64 reference of the WHOLE batch
    (train_step_ref.train_forward on the ranks' own img_feats put together) at the VJP bar of tests/test_gpu_train_step.py with its exact-zero rule for
    gconv.bias; sum (B_r / B) loss_r at FWD_REL; the nine running means / variances at rtol 1e-5 + atol 1e-6 sqrt(running_var); num_batches_tracked + 1;
    gradients, running statistics and stepped parameters bit-identical on the two ranks.
E2  frozen statistics: the reduced gradients are, bit for bit, this process's two shards one after the other, each backpropagating loss B_r / B, added.
E3  trunk_grad + backbone.train_batchnorm, 2 + 2 images of 64 x 64: the fold invariant on every rank, the stem's merged statistics against float64 ones of
    the whole batch's pre-pool activation, running buffers and reduced gradients bit-identical on the two ranks and finite.
E4  data_parallel = True without a process group: a step bit-equal to data_parallel = False.
RCCL: E1 over nccl with one device per rank where the box has two; skipped on a one-GPU box.  Every figure is printed before it is asserted."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_step_ref as TR  # noqa: E402
from egohmr_amd import synthetic as syn  # noqa: E402
from tests import dp_common as DP  # noqa: E402
from tests.test_gpu_train_step import FWD_REL, _check_grads  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def run_ranks(tmp_path, case, counts, backend="gloo"):
    """One fresh process per rank, a time limit on each; -> what every rank saved, in rank order."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(len(counts)):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(len(counts)),
                   EGOHMR_DIST_BACKEND=backend, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, DP.__file__, case, json.dumps(counts), str(tmp_path / f"rank{r}.pt")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0, log.decode()[-3000:]
    return [torch.load(tmp_path / f"rank{r}.pt") for r in range(len(counts))]


@pytest.fixture(scope="module")
def world(dev, golden_dir, synth_weights, smpl_asset):
    """This process's model (as the ranks build theirs), the whole batch on the CPU and the reference's constants."""
    m = DP.build(dev, synth_weights, smpl_asset)
    m.init_optimizers()
    b_np, flags, d, t, x_t = DP.whole_batch(golden_dir)
    mean, std = syn.make_body_rep_stats(0)
    ref = dict(weights=m.loss_weights(), smpl_asset=smpl_asset, gt=TR.gt_inputs(b_np, (syn.make_smpl_asset(1), syn.make_smpl_asset(2))), mean=mean, std=std)
    return dict(model=m, b_np=b_np, flags=flags, t=t, x_t=x_t, ref=ref, names=TR.opt_names(m), sd=TR.state64(synth_weights))


def reset(m, synth_weights, case):
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth_weights.items()}, strict=False)
    for p in m.parameters():
        p.grad = None
    m.validation_setup()
    DP.configure(m, case)
    m.init_optimizers()


def same_bits(a, b):
    return sorted(k for k in a if not torch.equal(a[k], b[k]))


def check_e1(tag, res, w, counts):
    names = w["names"]
    img_feats = torch.cat([r["img_feats"] for r in res])
    sd, leaves = TR.leaves(w["sd"], names)
    sd = {k: (v if k in names else v.clone()) for k, v in sd.items()}                       # (its running statistics are updated in place)
    ref = TR.train_forward(sd, w["b_np"], img_feats, w["x_t"], w["t"], train_bn=True, **w["ref"])
    grads = torch.autograd.grad(ref["loss"], leaves, allow_unused=True)
    ref_g = {n: (torch.zeros_like(p) if g is None else g) for n, p, g in zip(names, leaves, grads)}
    print(f"[{tag}] gate margin of the reference on the ranks' img_feats: {ref['margin']:.2e}")
    for r in res:
        _check_grads(f"{tag} rank {r['rank']}", dict(got_g={n: g.to("cpu") for n, g in r["grads"].items()}, ref_g=ref_g), names, True)
    B = sum(counts)
    loss = sum(c / B * r["loss"] for c, r in zip(counts, res))
    want = float(ref["loss"].detach())
    print(f"[{tag}] sum (B_r / B) loss_r = {loss:.6f}, the reference's {want:.6f}: |err| {abs(loss - want):.3e}, bar {FWD_REL * max(1.0, abs(want)):.3e}")
    assert abs(loss - want) <= FWD_REL * max(1.0, abs(want))
    bns = [k[:-len(".running_mean")] for k in res[0]["buffers"] if k.startswith("diffusion_model.") and k.endswith(".running_mean")]
    assert len(bns) == 9
    worst = 0.0
    for p in bns:
        want_v = sd[p + ".running_var"]
        atol = 1e-6 * want_v.sqrt()
        for r in res:
            for key in (".running_mean", ".running_var"):
                want_t = sd[p + key]
                err = (r["buffers"][p + key].double() - want_t).abs()
                worst = max(worst, float((err / (atol + 1e-5 * want_t.abs())).max()))
                assert bool((err <= atol + 1e-5 * want_t.abs()).all()), (p, key, r["rank"])
                assert not torch.equal(r["buffers"][p + key], r["buffers_before"][p + key])
            assert int(r["buffers"][p + ".num_batches_tracked"]) == int(r["buffers_before"][p + ".num_batches_tracked"]) + 1
    print(f"[{tag}] nine running means / variances: worst err / (atol + rtol |ref|) = {worst:.2e}")
    for what in ("grads", "buffers", "params"):
        assert not same_bits(res[0][what], res[1][what]), (what, same_bits(res[0][what], res[1][what]))
    assert same_bits(res[0]["params"], {n: w["sd"][n].float() for n in names})             # the step did move the parameters


@pytest.mark.parametrize("counts", [[2, 2], [3, 1]])
def test_e1_batch_statistics_two_ranks_equal_the_whole_batch(dev, world, tmp_path, counts):
    check_e1(f"E1 gloo {counts[0]}+{counts[1]}", run_ranks(tmp_path, "e1", counts), world, counts)


def test_e1_over_rccl_with_one_device_per_rank(dev, world, tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip("the RCCL variant needs two devices; on a one-GPU box the nccl path of dist.StatSync / all_reduce_sum_ stays unverified")
    check_e1("E1 nccl 2+2", run_ranks(tmp_path, "e1", [2, 2], backend="nccl"), world, [2, 2])


@pytest.mark.parametrize("counts", [[2, 2], [3, 1]])
def test_e2_frozen_statistics_two_ranks_are_the_two_shards_added(dev, world, synth_weights, tmp_path, counts):
    res = run_ranks(tmp_path, "e2", counts)
    m, B = world["model"], sum(counts)
    parts = []
    for r in range(2):
        reset(m, synth_weights, "e2")
        batch, ts = DP.shard(world["b_np"], world["flags"], world["x_t"], world["t"], DP.items_of(counts, r), dev)
        g, loss = DP.scaled_step_gradients(m, batch, ts, counts[r] / B)
        print(f"[E2 {counts[0]}+{counts[1]}] shard {r}: loss {float(loss):.6f} here, {res[r]['loss']:.6f} on the rank")
        parts.append(g)
    torch.cuda.synchronize()
    m.validation_setup()
    want = {n: (parts[0][n] + parts[1][n]).cpu() for n in world["names"]}
    differ = same_bits(want, res[0]["grads"])
    print(f"[E2 {counts[0]}+{counts[1]}] {len(want)} reduced gradients, {len(differ)} differ from the two shards added in this process")
    assert not differ, differ
    assert not same_bits(res[0]["grads"], res[1]["grads"]) and not same_bits(res[0]["params"], res[1]["params"])
    for r in res:                                                                            # frozen statistics stay as they were
        assert not same_bits(r["buffers"], r["buffers_before"])


def test_e3_trunk_on_all_ranks_statistics(dev, golden_dir, synth_weights, tmp_path):
    res = run_ranks(tmp_path, "e3", [2, 2])
    assert all(r["fold_invariant"] for r in res)
    # the stem is row-independent: its raw pre-pool activation of the whole batch in float64 (teacher forced on the weights and the images)
    b_np = DP.whole_batch(golden_dir, small_images=True)[0]
    w = torch.from_numpy(np.asarray(synth_weights["backbone.conv1.weight"])).double()
    z = torch.nn.functional.conv2d(torch.from_numpy(b_np["img"]).double(), w, None, 2, 3)
    z = z.permute(0, 2, 3, 1).reshape(-1, 64)
    mean64, var64 = z.mean(0), z.var(0, unbiased=False)
    for r in res:
        e_m = float(((r["stem_mean"].double() - mean64).abs() / var64.sqrt()).max())
        e_v = float(((r["stem_var"].double() - var64).abs() / var64).max())
        print(f"[E3 rank {r['rank']}] stem: max |mean err| / std {e_m:.2e}, max rel err of var {e_v:.2e}; |mean| / std up to {float((mean64.abs() / var64.sqrt()).max()):.2f}")
        np.testing.assert_allclose(r["stem_var"].double().numpy(), var64.numpy(), rtol=1e-5, atol=0)
        assert bool(((r["stem_mean"].double() - mean64).abs() <= 1e-6 * var64.sqrt()).all())
    assert torch.equal(res[0]["stem_mean"], res[1]["stem_mean"]) and torch.equal(res[0]["stem_var"], res[1]["stem_var"])
    for what in ("grads", "buffers", "params"):
        assert not same_bits(res[0][what], res[1][what]), (what, same_bits(res[0][what], res[1][what]))
    moved = [k for k in res[0]["buffers"] if k.startswith("backbone.") and k.endswith("running_mean")
             and not torch.equal(res[0]["buffers"][k], res[0]["buffers_before"][k])]
    n_bb = len([n for n in res[0]["grads"] if n.startswith("backbone.")])
    print(f"[E3] {len(res[0]['grads'])} reduced gradients ({n_bb} of the backbone), {len(moved)} backbone running means moved")
    assert len(moved) == 53 and n_bb == 159
    assert all(bool(torch.isfinite(v).all()) for r in res for what in ("grads", "buffers", "params") for v in r[what].values())


def test_e4_without_a_process_group_the_switch_changes_nothing(dev, world, synth_weights):
    m = world["model"]
    batch, ts = DP.shard(world["b_np"], world["flags"], world["x_t"], world["t"], list(range(DP.B_E2E)), dev)
    runs = []
    try:
        for flag in (False, True):
            reset(m, synth_weights, "e1")
            m.data_parallel = flag
            torch.manual_seed(0)
            out = m.training_step(batch, ts, 0)
            torch.cuda.synchronize()
            runs.append(dict(loss=out["losses"]["loss"], grads={n: p.grad.clone() for n, p in zip(world["names"], m.opt_params)},
                             state={k: v.detach().clone() for k, v in m.state_dict().items()}))
    finally:
        m.data_parallel = False
        m.validation_setup()
    assert float(runs[0]["loss"]) == float(runs[1]["loss"])
    assert not same_bits(runs[0]["grads"], runs[1]["grads"]) and not same_bits(runs[0]["state"], runs[1]["state"])
