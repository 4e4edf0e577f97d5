"""GPU (MI355X): one EgoHMR.training_step of a model with gcn_nonlocal_layer=True behind diffusion_model.nonlocal_grad - frozen trunk, the denoiser on
batch statistics, the batch and model of tests/test_gpu_train_step.py (B = 4, N = 512, its NOISE_SEED and TIMESTEPS).

1  forward + compute_loss + backward against the float64 route (train_step_ref.train_forward with the denoiser of tests/nonlocal_ref.py in place of
   gcn_train_ref's, fed the device's own img_feats) at that file's bars: pred_x_start and the loss at FWD_REL, every gradient of init_optimizers' list at the
   VJP bar - the block's ten among them; the gradients that are zero in exact arithmetic as tests/test_gpu_nonlocal_grad.py holds them.
   The gate margin: every ReLU of the denoiser sits in FRONT of the block, so the reference's BatchNorm outputs - and NOISE_SEED's search - are those of
   the model without it; asserted by running the float64 forward of that model on the same inputs.
2  training_step: every tensor of the optimizer's list gets a finite gradient, the block's ten parameters move, W.1's running statistics move, and an
   eval-mode val_losses call after the step runs on the updated block (ModulatedGCN.nonlocal_packed keys on the parameter versions) and differs from the one
   before it."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nonlocal_ref as NR  # noqa: E402
import train_step_ref as TR  # noqa: E402
import val_losses_ref as R  # noqa: E402
from egohmr_amd import synthetic as syn  # noqa: E402
from tests.test_gpu_train_step import (B_E2E, FWD_REL, N_SCENE, NOISE_SEED, T_STEPS, TIMESTEPS, VJP_ATOL_REL, _build, _check_forward,  # noqa: E402
                                       _check_grads)

pytestmark = pytest.mark.gpu

NLP = "diffusion_model.non_local."
# zero in exact arithmetic under batch statistics (tests/test_nonlocal_grad_cpu.py says why) -> the gradient whose scale they are held against
ZERO_PARTNER = {NLP + "phi.bias": NLP + "theta.bias", NLP + "W.0.bias": NLP + "W.1.bias", NLP + "g.bias": NLP + "W.1.bias"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights():
    return syn.make_state_dict(0, nonlocal_layer=True)


@pytest.fixture(scope="module")
def setup(dev, golden_dir, weights, smpl_asset):
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device
    g = np.load(os.path.join(golden_dir, "g21_val_losses_a.npz"))
    assert int(g["N"]) == N_SCENE
    b_np, flags = R.golden_batch(g)
    cut = lambda d: {k: (cut(v) if isinstance(v, dict) else v[:B_E2E]) for k, v in d.items()}
    b_np = cut(b_np)
    batch = batch_to_device(b_np, dev)
    batch["smpl_params_is_axis_angle"] = {k: v[:B_E2E] for k, v in flags.items()}
    mean, std = syn.make_body_rep_stats(0)
    d = create_gaussian_diffusion(num_diffusion_timesteps=T_STEPS, timestep_respacing="", body_rep_mean=mean, body_rep_std=std)
    t = torch.tensor(TIMESTEPS)
    noise = torch.from_numpy(np.random.default_rng(NOISE_SEED).normal(size=(B_E2E, 144)).astype(np.float32))
    x_t = d.q_sample(TR.x_start_of(b_np, mean, std).float(), t, noise=noise)
    m = _build(dev, weights, smpl_asset, gcn_nonlocal_layer=True)
    m.diffusion_model.nonlocal_grad = True
    m.diffusion_model.train_batchnorm = True
    m.init_optimizers()
    ref = dict(weights=m.loss_weights(), smpl_asset=smpl_asset, gt=TR.gt_inputs(b_np, (syn.make_smpl_asset(1), syn.make_smpl_asset(2))), mean=mean, std=std)
    return dict(model=m, batch=batch, b_np=b_np, d=d, t=t, noise=noise, x_t=x_t, ref=ref, names=TR.opt_names(m), sd=TR.state64(weights), mean=mean, std=std)


def _reset(m, weights):
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()}, strict=False)
    for p in m.parameters():
        p.grad = None
    m.validation_setup()
    m.init_optimizers()


def test_step_gradients_vs_fp64(dev, setup, weights, synth_weights, monkeypatch):
    s = setup
    m, batch = s["model"], s["batch"]
    _reset(m, weights)
    assert len([n for n in s["names"] if n.startswith(NLP)]) == 10
    batch["x_t"] = s["x_t"].to(dev)
    img_feats = m.fused_sampler.prepare(batch, _constants_only=True).img_feats.clone()
    m._set_train_modes()
    assert m.training and m.diffusion_model.training and m.diffusion_model.non_local.W[1].training
    out = m(batch, s["t"].to(dev), eval_with_uncond=False)
    loss = m.compute_loss(batch, out)
    loss.backward()
    torch.cuda.synchronize()
    # the float64 route: train_step_ref's, with the denoiser that has the block
    plain = TR.train_forward(dict(TR.state64(synth_weights)), s["b_np"], img_feats.cpu(), s["x_t"], s["t"], train_bn=True, update_running=False, **s["ref"])
    monkeypatch.setattr(TR, "T", SimpleNamespace(
        modulated_gcn_train=lambda gsd, X, adj, blocks=4, update_running=True: NR.modulated_gcn(gsd, X, adj, blocks, True, update_running=update_running),
        eval_forward=lambda gsd, X, adj, blocks=4: NR.modulated_gcn(gsd, X, adj, blocks, False)[0]))
    sd, leaves = TR.leaves(s["sd"], s["names"])
    sd = {k: (v if k in s["names"] else v.clone()) for k, v in sd.items()}
    r = TR.train_forward(sd, s["b_np"], img_feats.cpu(), s["x_t"], s["t"], train_bn=True, **s["ref"])
    print(f"[non-local step] gate margin of the reference on the device's img_feats: {r['margin']:.2e} (seed {NOISE_SEED}); without the block {plain['margin']:.2e}")
    assert abs(r["margin"] - plain["margin"]) <= 1e-6 * plain["margin"] and r["margin"] > 0        # the block sits behind every gate (two float64 runs)
    assert not torch.equal(r["x0"].detach(), plain["x0"].detach())              # and it does something
    grads = torch.autograd.grad(r["loss"], leaves, allow_unused=True)
    ref_g = {n: (torch.zeros_like(p) if g is None else g) for n, p, g in zip(s["names"], leaves, grads)}
    got_g = {n: p.grad for n, p in m.named_parameters()}
    c = dict(out=out, loss=loss.detach(), ref=r, ref_g=ref_g, got_g=got_g)
    _check_forward("non-local step", c)
    _check_grads("non-local step", c, [n for n in s["names"] if n not in ZERO_PARTNER], True)
    for n, partner in ZERO_PARTNER.items():
        scale = float(ref_g[partner].abs().max())
        got = float(got_g[n].double().abs().max())
        print(f"[non-local step] {n}: max|got| / (VJP atol on {partner}) = {got / (VJP_ATOL_REL * scale):.2e}; the reference's own / scale {float(ref_g[n].abs().max()) / scale:.1e}")
        assert float(ref_g[n].abs().max()) <= 1e-9 * scale and got <= VJP_ATOL_REL * scale, n
    bn = m.diffusion_model.non_local.W[1]
    # W.1's running statistics.  The statistics kernels' own bar (rtol 1e-5 + atol 1e-6 sqrt(var)) is for a GIVEN u and is held in
    # tests/test_gpu_nonlocal_grad.py and tests/test_gpu_nonlocal_module.py; here u comes out of thirteen float32 layers, which the forward bar holds to
    # FWD_REL max(1, max|.|): the batch mean moves by at most that, the variance by twice that relative to itself, and the running update takes
    # `momentum` of either.  The batch's own mean / variance from the reference's update: b = (r1 - 0.9 r0) / 0.1
    for name, factor in (("running_mean", 1.0), ("running_var", 2.0)):
        want, r0 = sd[NLP + "W.1." + name], s["sd"][NLP + "W.1." + name]
        b = (want - 0.9 * r0) / 0.1
        bar = 0.1 * factor * FWD_REL * max(1.0, float(b.abs().max()))
        err = float((getattr(bn, name).double().cpu() - want).abs().max())
        print(f"[non-local step] W.1.{name}: max|err| {err:.3e}, bar {bar:.3e} (momentum x {factor:g} x FWD_REL x max(1, max|batch value| = {float(b.abs().max()):.3g}))")
        assert err <= bar, name
        assert not torch.equal(getattr(bn, name).double().cpu(), r0)
    assert int(bn.num_batches_tracked) == int(s["sd"][NLP + "W.1.num_batches_tracked"]) + 1
    m.validation_setup()


def test_training_step_moves_the_block_and_sampling_sees_it(dev, setup, weights):
    from egohmr_amd.diffusion import create_gaussian_diffusion
    s = setup
    m, batch = s["model"], s["batch"]
    _reset(m, weights)
    d5 = create_gaussian_diffusion(num_diffusion_timesteps=T_STEPS, timestep_respacing="ddim5", body_rep_mean=s["mean"], body_rep_std=s["std"])

    def sample():
        torch.manual_seed(3)
        out = d5.val_losses(m, batch, [B_E2E, 144], timestep_respacing="ddim5")
        torch.cuda.synchronize()
        return out["pred_vertices"].clone(), float(out["losses"]["loss"])
    v0, l0 = sample()
    v0b, l0b = sample()
    assert torch.equal(v0, v0b) and l0 == l0b                                   # the same seed samples the same bodies: what differs below is the weights
    block = {n: p for n, p in m.named_parameters() if n.startswith(NLP)}
    assert len(block) == 10
    before = {n: p.detach().clone() for n, p in block.items()}
    stats = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith(NLP + "W.1.running")}
    out = s["d"].training_losses(m, batch, s["t"].to(dev), noise=s["noise"].to(dev))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["losses"]["loss"]))
    names = TR.opt_names(m)
    missing = [n for n, p in zip(names, m.opt_params) if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not missing, missing
    still = [n for n, p in block.items() if torch.equal(p.detach(), before[n])]
    print(f"[non-local step] block parameters that did not move: {still}")
    assert not still, still
    after = m.state_dict()
    assert all(not torch.equal(after[k], v) for k, v in stats.items()) and len(stats) == 2
    v1, l1 = sample()
    assert not m.training and bool(torch.isfinite(v1).all())
    print(f"[non-local step] val_losses loss before the step {l0:.6f}, after {l1:.6f}; max vertex move {float((v1 - v0).abs().max()):.3e} m")
    assert not torch.equal(v1, v0) and l1 != l0
    # with the flag off again the step is refused as ever
    m.diffusion_model.nonlocal_grad = False
    try:
        with pytest.raises(NotImplementedError, match="non-local block has no backward"):
            m.training_step(batch, s["t"].to(dev), 0)
    finally:
        m.diffusion_model.nonlocal_grad = True
        m.validation_setup()
