"""What the data-parallel training tests share between the parent test process (tests/test_gpu_data_parallel.py) and the rank processes it starts (this
file run as a script): the model and batch of tests/test_gpu_train_step.py (B = 4, N = 512, its NOISE_SEED and TIMESTEPS), the sharding, and one step.

As a script:  python tests/dp_common.py CASE COUNTS_JSON OUT.pt   with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT / EGOHMR_DIST_BACKEND in the environment.
CASE: e1 (frozen trunk, denoiser on batch statistics), e2 (frozen statistics), e3 (trunk_grad + backbone.train_batchnorm, 64 x 64 images)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import train_step_ref as TR  # noqa: E402
import val_losses_ref as R  # noqa: E402
from egohmr_amd import synthetic as syn  # noqa: E402

B_E2E, N_SCENE, T_STEPS = 4, 512, 1000
TIMESTEPS = [0, T_STEPS - 1, 500, 37]
NOISE_SEED = 165                       # tests/test_gpu_train_step.py: its gate-margin search is for this batch
E3_IMG_SEED, E3_HW = 3, 64


def build(dev, synth_weights, smpl_asset, **kw):
    from egohmr_amd.factory import build_synthetic_model
    m = build_synthetic_model(dev, 0, diffuse_fuse=True, state_dict=synth_weights, smpl_asset=smpl_asset, smpl_asset_male=syn.make_smpl_asset(1),
                              smpl_asset_female=syn.make_smpl_asset(2), start_coap_epoch=R.START_COAP_EPOCH, **{**R.CASE_WEIGHTS, **kw})
    m.frozen_trunk_training = True
    return m


def whole_batch(golden_dir, small_images=False):
    """(b_np, flags, diffusion, t, x_t) of the whole batch on the CPU; small_images: E3's 64 x 64 images in place of the golden ones."""
    from egohmr_amd.diffusion import create_gaussian_diffusion
    g = np.load(os.path.join(golden_dir, "g21_val_losses_a.npz"))
    assert int(g["N"]) == N_SCENE
    b_np, flags = R.golden_batch(g)
    cut = lambda d: {k: (cut(v) if isinstance(v, dict) else v[:B_E2E]) for k, v in d.items()}
    b_np, flags = cut(b_np), {k: v[:B_E2E] for k, v in flags.items()}
    if small_images:
        b_np["img"] = np.random.default_rng(E3_IMG_SEED).normal(size=(B_E2E, 3, E3_HW, E3_HW)).astype(np.float32)
    mean, std = syn.make_body_rep_stats(0)
    d = create_gaussian_diffusion(num_diffusion_timesteps=T_STEPS, timestep_respacing="", body_rep_mean=mean, body_rep_std=std)
    t = torch.tensor(TIMESTEPS)
    noise = torch.from_numpy(np.random.default_rng(NOISE_SEED).normal(size=(B_E2E, 144)).astype(np.float32))
    x_t = d.q_sample(TR.x_start_of(b_np, mean, std).float(), t, noise=noise)
    return b_np, flags, d, t, x_t


def shard(b_np, flags, x_t, t, items, dev):
    """The items' part of the batch on the device, with its x_t; and their timesteps."""
    from egohmr_amd.factory import batch_to_device
    sub = lambda d: {k: (sub(v) if isinstance(v, dict) else v[items]) for k, v in d.items()}
    batch = batch_to_device(sub(b_np), dev)
    batch["smpl_params_is_axis_angle"] = {k: v[items] for k, v in flags.items()}
    batch["x_t"] = x_t[items].to(dev)
    return batch, t[items].to(dev)


def items_of(counts, rank):
    start = sum(counts[:rank])
    return list(range(start, start + counts[rank]))


def configure(m, case):
    m.diffusion_model.train_batchnorm = case in ("e1", "e3")
    m.trunk_grad = case == "e3"
    m.backbone.train_batchnorm = case == "e3"


def scaled_step_gradients(m, batch, t, weight):
    """forward + compute_loss + (loss * weight).backward() with no optimizer step: (float32 gradients by name, the loss)."""
    m._set_train_modes()
    out = m(batch, t, eval_with_uncond=False)
    loss = m.compute_loss(batch, out)
    m.optimizer.zero_grad()
    (loss * weight).backward()
    return {n: p.grad.detach().clone() for n, p in zip(TR.opt_names(m), m.opt_params)}, loss.detach()


def rank_main(case, counts, out_path):
    from egohmr_amd import dist as edist
    from egohmr_amd import trunk_grad
    rank, world, local = edist.init_from_env()
    assert world == len(counts)
    import torch.distributed as td
    dev = torch.device("cuda", local if td.get_backend() == "nccl" else 0)         # gloo: the ranks share the one GPU of the box
    if dev.index:
        torch.cuda.set_device(dev)
    golden = os.path.join(HERE, "golden")
    sw, asset = syn.make_state_dict(0), syn.make_smpl_asset(0)
    m = build(dev, sw, asset)
    configure(m, case)
    m.data_parallel = True
    if rank == 1:                                                                   # init_optimizers must bring rank 0's values back
        with torch.no_grad():
            next(m.beta_layer.parameters()).add_(1.0)
    m.init_optimizers()
    b_np, flags, d, t, x_t = whole_batch(golden, small_images=case == "e3")
    batch, ts = shard(b_np, flags, x_t, t, items_of(counts, rank), dev)
    res = dict(rank=rank, counts=counts)
    names = TR.opt_names(m)
    if case == "e3":
        # the fold invariant, on all ranks' statistics: the backbone's own call with the step's sync object
        import copy
        sync = edist.StatSync.exchange(len(items_of(counts, rank)), dev)
        bb = m.backbone
        bb.train()
        bb.stat_sync = sync
        try:
            img = batch["img"].float()
            out, rec = trunk_grad.train_forward(bb, img)
        finally:
            bb.stat_sync = None
        twin = copy.deepcopy(bb)
        twin._fold_key_fn = twin._fold_key = twin._fold_fn = None
        twin.eval()
        with torch.no_grad():
            for u, e in zip(trunk_grad.units(twin), rec.bn):
                if u is not None:
                    u[1].running_mean.copy_(e[2]), u[1].running_var.copy_(e[3])
        res["fold_invariant"] = bool(torch.equal(twin(img), out))
        res["stem_mean"], res["stem_var"] = rec.bn[0][2].cpu(), rec.bn[0][3].cpu()
        del twin, rec, out
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sw.items()}, strict=False)       # the statistics as before that call
        m.init_optimizers()
    else:
        res["img_feats"] = m.fused_sampler.prepare(batch, _constants_only=True).img_feats.detach().clone().cpu()
    before = {k: v.detach().clone().cpu() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    torch.manual_seed(rank)
    out = m.training_step(batch, ts, 0)
    torch.cuda.synchronize()
    res["loss"] = float(out["losses"]["loss"])
    res["grads"] = {n: p.grad.detach().cpu() for n, p in zip(names, m.opt_params)}
    res["params"] = {n: p.detach().cpu() for n, p in zip(names, m.opt_params)}
    res["buffers"] = {k: v.detach().cpu() for k, v in m.state_dict().items() if k in before}
    res["buffers_before"] = before
    edist.barrier()
    torch.save(res, out_path)
    td.destroy_process_group()


if __name__ == "__main__":
    rank_main(sys.argv[1], json.loads(sys.argv[2]), sys.argv[3])
