#!/usr/bin/env python3
"""Write tests/golden/g22_nonlocal_train.npz by running the REFERENCE's own ModulatedGCN(nonlocal_layer=True) (models/egohmr/modulated_gcn/modulated_gcn.py:
60-116 with nets/non_local_embedded_gaussian.py) in .double() on the CPU, forward and backward, in .train() and in .eval().  Test infrastructure, run by
hand where the reference tree is present; not collected by pytest.

    python tests/make_nonlocal_golden.py <path of the reference tree>           # from the repository root

The file holds data only: the seed and the sizes, x, the cotangent, and per mode the output, the gradient of x and of every parameter, and the block's
W.1 running statistics after the call.  The weights are tests/nonlocal_ref.module_state(SEED), pushed in through load_state_dict."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import nonlocal_ref as NR  # noqa: E402
from oracle import model as om  # noqa: E402

SEED, IN_DIM, HID, BLOCKS, B = 22, 70, 64, 1, 3


def fd_check(net, x, cot, mode, h=1e-6):
    """autograd against central differences of <net(x), cot> in one entry of every parameter of the block and of the convs in front of it (float64: 1e-6
    relative to the gradient's largest entry).  Train mode: on a copy, so that the running statistics of `net` see one call only."""
    import copy
    probe = copy.deepcopy(net)
    grads = {n: p.grad for n, p in net.named_parameters()}
    with torch.no_grad():
        for n, p in probe.named_parameters():
            if n.startswith("gconv_output") or (mode == "train" and (n.endswith("gconv.bias") or n.endswith("W.0.bias"))):
                continue
            i = int(grads[n].abs().argmax())
            flat = p.view(-1)
            old = float(flat[i])
            flat[i] = old + h
            up = float((probe(x) * cot).sum())
            flat[i] = old - h
            dn = float((probe(x) * cot).sum())
            flat[i] = old
            fd, ag = (up - dn) / (2 * h), float(grads[n].view(-1)[i])
            assert abs(fd - ag) <= 1e-6 * abs(ag) + 1e-9, (mode, n, fd, ag)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from models.egohmr.modulated_gcn.modulated_gcn import ModulatedGCN
    sd, x = NR.module_state(SEED, in_dim=IN_DIM, hid=HID, blocks=BLOCKS, bodies=B)
    cot = torch.from_numpy(np.random.Generator(np.random.PCG64(SEED + 1)).normal(size=(B, 24, 6)).astype(np.float32)).double()
    out = dict(seed=SEED, in_dim=IN_DIM, hid=HID, blocks=BLOCKS, x=x.numpy(), cot=cot.numpy())
    for mode in ("train", "eval"):
        net = ModulatedGCN(om.smpl_adjacency(torch.float64), in_dim=IN_DIM, out_dim=6, hid_dim=HID, num_layers=BLOCKS, nonlocal_layer=True).double()
        missing, unexpected = net.load_state_dict(sd, strict=False)
        assert not unexpected and all("adj" in k or "num_batches_tracked" in k for k in missing), (missing, unexpected)
        net.train(mode == "train")
        # torch's CPU batch_norm backward (seen on 2.10) mis-reads a cotangent whose strides are channels-last while the BatchNorm's input is contiguous -
        # exactly what modulated_gcn.py:109's permute hands W.1 - and returns wrong gradients for everything upstream.  The hook makes that cotangent
        # contiguous before the block's backward sees it; the reference's code is untouched, and fd_check below holds the result against central differences
        net.non_local.register_forward_hook(lambda m, i, o: (o.register_hook(lambda g: g.contiguous()) and None) if o.requires_grad else None)
        xl = x.clone().requires_grad_(True)
        y = net(xl)
        y.backward(cot)
        fd_check(net, x, cot, mode)
        out[mode + ".out"] = y.detach().numpy()
        out[mode + ".gx"] = xl.grad.numpy()
        for n, p in net.named_parameters():
            out[f"{mode}.grad.{n}"] = p.grad.numpy()
        for n in ("running_mean", "running_var", "num_batches_tracked"):
            out[f"{mode}.non_local.W.1.{n}"] = getattr(net.non_local.W[1], n).numpy()
    path = os.path.join(HERE, "golden", "g22_nonlocal_train.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
