"""One rank of tests/test_gpu_nonlocal_module.py's data-parallel case, run as a script in a fresh process (gloo, the ranks share the one GPU): the bare
ModulatedGCN(nonlocal_layer=True) with nonlocal_grad under .train() + train_batchnorm on this rank's items of the batch, its BatchNorms (W.1 among them)
on all ranks' rows through ModulatedGCN.stat_sync.  Leaves the output rows, the rank's own gradients and the running statistics in a file.

    python tests/nonlocal_dp_rank.py SEED COUNTS_JSON PRECISION OUT.pt      with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import nonlocal_ref as NR  # noqa: E402

COT_SEED = 99


def build(sd, dev, precision="f16x3", train=True):
    from egohmr_amd.model import ModulatedGCN, smpl_tree_adjacency
    m = ModulatedGCN(smpl_tree_adjacency(), in_dim=70, hid_dim=64, num_layers=1, nonlocal_layer=True)
    missing = m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    assert not missing.unexpected_keys and all("num_batches_tracked" in k for k in missing.missing_keys), missing
    m = m.to(dev).train(train)
    m.nonlocal_grad, m.grad_params, m.train_batchnorm, m.precision = True, True, bool(train), precision
    return m


def cotangent(bodies):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(COT_SEED)).normal(size=(bodies, 24, 6)).astype(np.float32))


def step(m, x, cot):
    """forward + backward -> dict(out, gx, grads by state-dict name, the running statistics)"""
    for p in m.parameters():
        p.grad = None
    x = x.clone().requires_grad_(True)
    out = m(x)
    out.backward(cot)
    torch.cuda.synchronize()
    names = {id(p): n for n, p in m.named_parameters()}
    return dict(out=out.detach().cpu(), gx=x.grad.cpu(), grads={names[id(p)]: p.grad.detach().cpu() for p in m.grad_parameters()},
                buffers={k: v.detach().cpu() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k})


def main(seed, counts, precision, out_path):
    import torch.distributed as td
    from egohmr_amd import dist as edist
    rank, world, _ = edist.init_from_env("gloo")
    assert world == len(counts)
    dev = torch.device("cuda", 0)
    sd, x = NR.module_state(seed, bodies=sum(counts))
    m = build(sd, dev, precision)
    lo = sum(counts[:rank])
    items = slice(lo, lo + counts[rank])
    m.stat_sync = edist.StatSync.exchange(counts[rank], dev)
    assert m.stat_sync.counts == counts and m.stat_sync.rank == rank
    res = step(m, x[items].float().to(dev), cotangent(sum(counts))[items].to(dev))
    m.stat_sync = None
    edist.barrier()
    torch.save(dict(res, rank=rank), out_path)
    td.destroy_process_group()


if __name__ == "__main__":
    main(int(sys.argv[1]), json.loads(sys.argv[2]), sys.argv[3], sys.argv[4])
