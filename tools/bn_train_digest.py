#!/usr/bin/env python3
"""SHA-256 of everything the 17 train-mode BatchNorm entries write (csrc/gcn_train.hip: ehm_gcn_train_adjacency / _preact / _stats / _normalize /
_bn_backward / _stats_local / _stats_merge / _bwd_local / _bwd_merge; csrc/bn2d_train.hip: ehm_bn2d_train_stats / _bwd_sums / _bwd_zbar / _stats_local /
_stats_merge / _bwd_local / _bwd_merge / _bwd_zbar_rows) on fixed seeded inputs: one line `<entry> <case> <digest>` per call, over the raw bytes of all
its outputs (the running statistics and num_batches_tracked count), and a last line with the number of lines and the digest of all of them.
    python tools/bn_train_digest.py [--out FILE]
The tool goes through the C ABI alone (egohmr_amd._lib), so two builds of the library compare with it: EHM_LIB_PATH=<other build> selects the second.
Equal last lines = the two builds write the same bits in every case.  A refactor of the two files is checked this way (docs/EXPERIMENTS.md).

Cases, the smallest that reach every branch.  gcn: N = 64 and 320 (a second, partly filled 256-channel chunk), bodies 1, 3 and 130 (more than the 128
body groups: a lane adds two bodies), have_sums 0 and 1, with and without running buffers / parameter gradients, world 1 and world 3 with uneven rows
(one z cut into three).  bn2d: X2 buffers of 32 and 160 channels, float32 rows of 8, 136 and 160, pixels 1 (local entries only), 2, 17 and 4097 (runs longer
than one 16-row group, the last one partial), world 1 and 3, zbar dense and zero-dilated (5 x 5 -> 3 x 3), with and without scale, zbar_rows with
total_rows equal to and larger than N Ho Wo.  'big' cases hold channels with |mean| / std = 1e3."""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from egohmr_amd import _lib  # noqa: E402

EPS, MOMENTUM, INPUT = 1e-5, 0.1, -1
LINES = []


def rng(*key):
    return np.random.Generator(np.random.PCG64(list(key)))


def emit(entry, case, *outs):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in outs:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    LINES.append(f"{entry} {case} {h.hexdigest()}")
    print(LINES[-1], flush=True)


def rows_of(v):
    return (C.c_int64 * len(v))(*v)


def values(g, rows, Cn, big):
    """float32 [rows, Cn]: O(1) means and spreads per channel, or (big) |mean| = 1e3 spreads"""
    z = g.uniform(0.5, 2.0, size=Cn) * g.normal(size=(rows, Cn))
    z += 1e3 * g.uniform(0.5, 2.0, size=Cn) * g.choice([-1.0, 1.0], size=Cn) if big else g.normal(size=Cn)
    return torch.from_numpy(z.astype(np.float32))


# ---------------------------------------------------------------------------------------------- csrc/gcn_train.hip
class GCN:
    def __init__(self, dev, N):
        g = rng(1, N)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        self.dev, self.N, self.A = dev, N, _lib.api()
        adj = t(np.abs(g.normal(scale=0.2, size=(24, 24))))
        self.keep = [adj]

        def params(K, Nout, bn):
            p = _lib.GConvParams()
            put = lambda a: self.keep.append(t(a)) or self.keep[-1].data_ptr()
            p.W, p.M = put(g.normal(scale=0.1, size=(2, K, Nout))), put(1 + g.normal(scale=0.15, size=(24, Nout)))
            p.adj2, p.bias = put(g.normal(scale=0.3, size=(24, 24))), put(g.normal(scale=0.05, size=Nout))
            if bn:
                p.bn_weight, p.bn_bias = put(g.uniform(0.5, 1.5, size=Nout) * g.choice([-1.0, 1.0], size=Nout)), put(g.normal(scale=0.05, size=Nout))
                p.bn_mean, p.bn_var = put(g.normal(scale=0.1, size=Nout)), put(g.uniform(0.6, 1.4, size=Nout))
            p.in_dim, p.out_dim = K, Nout
            return p

        pin, hidden, pout = params(64, N, True), (_lib.GConvParams * 1)(), params(N, 6, False)
        h = C.c_void_p()
        self.A.ehm_gcn_create(C.byref(h), adj, C.byref(pin), hidden, 0, C.byref(pout), N, None)
        self.h = _lib.Handle(h, self.A.ehm_gcn_destroy, self.keep)

    def ws(self, bodies):
        nb = C.c_int64(0)
        self.A.ehm_gcn_train_workspace_bytes(self.h, INPUT, bodies, C.byref(nb))
        return torch.zeros(nb.value // 8, device=self.dev, dtype=torch.float64), nb.value

    def new(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, device=self.dev, dtype=dtype)

    def running(self):
        return torch.full((self.N,), 0.25, device=self.dev), torch.full((self.N,), 1.5, device=self.dev)

    def case(self, bodies, big):
        A, h, N, dev, rows = self.A, self.h, self.N, self.dev, bodies * 24
        g = rng(2, N, bodies, int(big))
        tag = f"gcn_N{N}_b{bodies}" + ("_big" if big else "")
        ws, nb = self.ws(bodies)
        adjA = self.new(24, 24)
        A.ehm_gcn_train_adjacency(h, INPUT, adjA, None)
        emit("ehm_gcn_train_adjacency", tag, adjA)
        z = self.new(rows, N)
        if big:                                             # a z that no preact wrote: have_sums = 0 only
            z.copy_(values(g, rows, N, True))
        else:
            pre = torch.from_numpy(g.normal(size=(rows, 2 * N)).astype(np.float32)).to(dev)
            A.ehm_gcn_train_preact(h, INPUT, pre, 2 * N, bodies, adjA, z, ws, nb, None)
            emit("ehm_gcn_train_preact", tag, z)
            mean, invstd, (rm, rv) = self.new(N), self.new(N), self.running()
            A.ehm_gcn_train_stats(h, INPUT, z, bodies, 1, EPS, MOMENTUM, mean, invstd, rm, rv, ws, nb, None)
            emit("ehm_gcn_train_stats", tag + "_sums1_run", mean, invstd, rm, rv)
            A.ehm_gcn_train_preact(h, INPUT, pre, 2 * N, bodies, adjA, z, ws, nb, None)
            local = self.new(2, N, dtype=torch.float64)
            A.ehm_gcn_train_stats_local(h, INPUT, z, bodies, 1, local, ws, nb, None)
            emit("ehm_gcn_train_stats_local", tag + "_sums1", local)
        mean, invstd, (rm, rv) = self.new(N), self.new(N), self.running()
        A.ehm_gcn_train_stats(h, INPUT, z, bodies, 0, EPS, MOMENTUM, mean, invstd, rm, rv, ws, nb, None)
        emit("ehm_gcn_train_stats", tag + "_sums0_run", mean, invstd, rm, rv)
        mean, invstd = self.new(N), self.new(N)
        A.ehm_gcn_train_stats(h, INPUT, z, bodies, 0, EPS, MOMENTUM, mean, invstd, None, None, ws, nb, None)
        emit("ehm_gcn_train_stats", tag + "_sums0", mean, invstd)
        res = torch.from_numpy(g.normal(size=(rows, N)).astype(np.float32)).to(dev)
        y, out = self.new(rows, N), self.new(rows, N)
        A.ehm_gcn_train_normalize(h, INPUT, z, mean, invstd, None, y, None, bodies, None)
        emit("ehm_gcn_train_normalize", tag + "_y", y)
        A.ehm_gcn_train_normalize(h, INPUT, z, mean, invstd, res, y, out, bodies, None)
        emit("ehm_gcn_train_normalize", tag + "_y_out_res", y, out)
        gout = torch.from_numpy(g.normal(size=(rows, N)).astype(np.float32)).to(dev)
        gate = torch.from_numpy(g.normal(size=(rows, N)).astype(np.float32)).to(dev)
        for grads in (True, False):
            zbar, gw, gb = self.new(rows, N), self.new(N), self.new(N)
            A.ehm_gcn_train_bn_backward(h, INPUT, gout, gate, z, mean, invstd, bodies, zbar, gw if grads else None, gb if grads else None, ws, nb, None)
            emit("ehm_gcn_train_bn_backward", tag + ("_grads" if grads else ""), zbar, gw, gb)
        splits = [(bodies,)] + ([(1, 1, 1)] if bodies == 3 else [(100, 29, 1)] if bodies == 130 else [])
        for split in splits:
            wtag = f"{tag}_w{len(split)}"
            cuts = np.cumsum((0,) + split) * 24
            shard = lambda t, r: t[cuts[r]:cuts[r + 1]].contiguous()
            gathered = self.new(len(split), 2, N, dtype=torch.float64)
            for r, b in enumerate(split):
                wsr, nbr = self.ws(b)
                A.ehm_gcn_train_stats_local(h, INPUT, shard(z, r), b, 0, gathered[r], wsr, nbr, None)
            emit("ehm_gcn_train_stats_local", wtag + "_sums0", gathered)
            rws = rows_of([24 * b for b in split])
            mean, invstd, (rm, rv) = self.new(N), self.new(N), self.running()
            A.ehm_gcn_train_stats_merge(h, INPUT, gathered, rws, len(split), EPS, MOMENTUM, mean, invstd, rm, rv, None)
            emit("ehm_gcn_train_stats_merge", wtag + "_run", mean, invstd, rm, rv)
            mean, invstd = self.new(N), self.new(N)
            A.ehm_gcn_train_stats_merge(h, INPUT, gathered, rws, len(split), EPS, MOMENTUM, mean, invstd, None, None, None)
            emit("ehm_gcn_train_stats_merge", wtag, mean, invstd)
            sums = self.new(len(split), 2, N, dtype=torch.float64)
            for r, b in enumerate(split):
                wsr, nbr = self.ws(b)
                A.ehm_gcn_train_bwd_local(h, INPUT, shard(gout, r), shard(gate, r), shard(z, r), mean, invstd, b, sums[r], wsr, nbr, None)
            emit("ehm_gcn_train_bwd_local", wtag, sums)
            for r, b in enumerate(split):
                for grads in (True, False):
                    wsr, nbr = self.ws(b)
                    zbar, gw, gb = self.new(b * 24, N), self.new(N), self.new(N)
                    A.ehm_gcn_train_bwd_merge(h, INPUT, sums, rws, len(split), r, shard(gout, r), shard(gate, r), shard(z, r), mean, invstd, b, zbar,
                                              gw if grads else None, gb if grads else None, wsr, nbr, None)
                    emit("ehm_gcn_train_bwd_merge", f"{wtag}_rank{r}" + ("_grads" if grads else ""), zbar, gw, gb)

    def close(self):
        torch.cuda.synchronize()
        self.h.close()


# ---------------------------------------------------------------------------------------------- csrc/bn2d_train.hip
def pack_x2(x):
    """float32 [rows, C] (C % 32 == 0) -> the X2 form as float32 [rows, C]: per 32 channels 32 f16 hi halves, then the 32 f16 lo halves (value = hi + lo)"""
    rows, Cn = x.shape
    hi = x.half()
    lo = (x - hi.float()).half()
    both = torch.stack([hi.view(rows, Cn // 32, 32), lo.view(rows, Cn // 32, 32)], dim=2)
    return both.reshape(rows, 2 * Cn).contiguous().view(torch.float32)


class BN2D:
    def __init__(self, dev, Cn, x2):
        self.dev, self.C, self.x2, self.A = dev, Cn, x2, _lib.api()
        self.tag = f"bn2d_{'x2' if x2 else 'f32'}_C{Cn}"
        self.one_call = Cn % 32 == 0

    def ws(self, pixels):
        nb = C.c_int64(0)
        self.A.ehm_bn2d_train_workspace_bytes(max(pixels, 2), (self.C + 31) // 32 * 32, C.byref(nb))
        return torch.zeros(nb.value // 8, device=self.dev, dtype=torch.float64), nb.value

    def new(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, device=self.dev, dtype=dtype)

    def put(self, x):
        return (pack_x2(x) if self.x2 else x).to(self.dev).contiguous()

    def running(self):
        return torch.full((self.C,), 0.25, device=self.dev), torch.full((self.C,), 1.5, device=self.dev), torch.full((), 5, dtype=torch.int64, device=self.dev)

    def rows_case(self, pixels, big):
        A, Cn, x2 = self.A, self.C, int(self.x2)
        g = rng(3, Cn, x2, pixels, int(big))
        tag = f"{self.tag}_p{pixels}" + ("_big" if big else "")
        x = values(g, pixels, Cn, big)
        G = torch.from_numpy(g.normal(scale=100.0, size=(pixels, Cn)).astype(np.float32))
        G[torch.from_numpy(g.random((pixels, Cn)) < 0.4)] = 0.0
        z, G = self.put(x), G.to(self.dev)
        ws, nb = self.ws(pixels)
        # statistics for the backward entries where the forward ones refuse the shape (one row in all): seeded ones
        mean = torch.from_numpy(g.normal(size=Cn).astype(np.float32)).to(self.dev)
        invstd = torch.from_numpy(g.uniform(0.5, 2.0, size=Cn).astype(np.float32)).to(self.dev)
        if self.one_call and pixels >= 2:
            mean, var, invstd, (rm, rv, nbt) = self.new(Cn), self.new(Cn), self.new(Cn), self.running()
            A.ehm_bn2d_train_stats(z, x2, pixels, pixels, Cn, EPS, MOMENTUM, mean, var, invstd, rm, rv, nbt, ws, nb, None)
            emit("ehm_bn2d_train_stats", tag + "_run", mean, var, invstd, rm, rv, nbt)
            mean, var, invstd = self.new(Cn), self.new(Cn), self.new(Cn)
            A.ehm_bn2d_train_stats(z, x2, pixels, pixels, Cn, EPS, MOMENTUM, mean, var, invstd, None, None, None, ws, nb, None)
            emit("ehm_bn2d_train_stats", tag, mean, var, invstd)
            gbeta, ggamma = self.new(Cn), self.new(Cn)
            A.ehm_bn2d_train_bwd_sums(G, z, x2, pixels, pixels, Cn, mean, invstd, gbeta, ggamma, ws, nb, None)
            emit("ehm_bn2d_train_bwd_sums", tag, gbeta, ggamma)
        splits = [(pixels,)] + ([(9, 7, 1)] if pixels == 17 else [(3000, 1096, 1)] if pixels == 4097 else [])
        for split in splits:
            wtag = f"{tag}_w{len(split)}"
            cuts = np.cumsum((0,) + split)
            zs = [self.put(x[cuts[r]:cuts[r + 1]]) for r in range(len(split))]
            Gs = [G[cuts[r]:cuts[r + 1]].contiguous() for r in range(len(split))]
            gathered = self.new(len(split), 2, Cn, dtype=torch.float64)
            for r, p in enumerate(split):
                wsr, nbr = self.ws(p)
                A.ehm_bn2d_train_stats_local(zs[r], x2, p, p, Cn, gathered[r], wsr, nbr, None)
            emit("ehm_bn2d_train_stats_local", wtag, gathered)
            if pixels >= 2:
                mean, var, invstd, (rm, rv, nbt) = self.new(Cn), self.new(Cn), self.new(Cn), self.running()
                A.ehm_bn2d_train_stats_merge(gathered, rows_of(split), len(split), Cn, EPS, MOMENTUM, mean, var, invstd, rm, rv, nbt, None)
                emit("ehm_bn2d_train_stats_merge", wtag + "_run", mean, var, invstd, rm, rv, nbt)
                mean, var, invstd = self.new(Cn), self.new(Cn), self.new(Cn)
                A.ehm_bn2d_train_stats_merge(gathered, rows_of(split), len(split), Cn, EPS, MOMENTUM, mean, var, invstd, None, None, None, None)
                emit("ehm_bn2d_train_stats_merge", wtag, mean, var, invstd)
            sums = self.new(len(split), 2, Cn, dtype=torch.float64)
            for r, p in enumerate(split):
                wsr, nbr = self.ws(p)
                A.ehm_bn2d_train_bwd_local(Gs[r], zs[r], x2, p, p, Cn, mean, invstd, sums[r], wsr, nbr, None)
            emit("ehm_bn2d_train_bwd_local", wtag, sums)
            for r in range(len(split)):
                for own in (True, False):
                    o = [self.new(Cn) for _ in range(4)]
                    A.ehm_bn2d_train_bwd_merge(sums, len(split), r, Cn, o[0], o[1], o[2] if own else None, o[3] if own else None, None)
                    emit("ehm_bn2d_train_bwd_merge", f"{wtag}_rank{r}" + ("_own" if own else ""), *o)

    def zbar_case(self):
        A, Cn, x2 = self.A, self.C, int(self.x2)
        g = rng(4, Cn, x2)
        N, Ho, Wo = 2, 3, 3
        R = N * Ho * Wo
        f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(self.dev)
        z = self.put(values(g, R, Cn, False))
        G = f(g.normal(scale=100.0, size=(R, Cn)))
        mean, invstd, gamma = f(g.normal(size=Cn)), f(g.uniform(0.5, 2.0, size=Cn)), f(g.normal(size=Cn) * 0.3 + 1.0)
        gbeta, ggamma = f(g.normal(scale=30.0, size=Cn)), f(g.normal(scale=30.0, size=Cn))
        scale = f(0.25).reshape(())
        for H, W, name in ((3, 3, "dense"), (5, 5, "dilated")):
            for s, sname in ((None, ""), (scale, "_scale")):
                tag = f"{self.tag}_{name}{sname}"
                if self.one_call:
                    out = self.new(N, H, W, Cn)
                    A.ehm_bn2d_train_bwd_zbar(G, z, x2, R, mean, invstd, gamma, gbeta, ggamma, s, out, N, Ho, Wo, Cn, H, W, None)
                    emit("ehm_bn2d_train_bwd_zbar", tag, out)
                for total in (R, R + 7):
                    out = self.new(N, H, W, Cn)
                    A.ehm_bn2d_train_bwd_zbar_rows(G, z, x2, R, mean, invstd, gamma, gbeta, ggamma, s, out, N, Ho, Wo, Cn, H, W, total, None)
                    emit("ehm_bn2d_train_bwd_zbar_rows", f"{tag}_total{total}", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    for N in (64, 320):
        net = GCN(dev, N)
        for bodies in (1, 3, 130):
            net.case(bodies, False)
        if N == 64:
            net.case(3, True)
        net.close()
    for Cn, x2 in ((32, True), (160, True), (8, False), (136, False), (160, False)):
        b = BN2D(dev, Cn, x2)
        for pixels in (1, 2, 17, 4097):
            b.rows_case(pixels, False)
        if Cn in (32, 160):
            b.rows_case(17, True)
        b.zbar_case()
    LINES.append(f"cases {len(LINES)} sha256 {hashlib.sha256(chr(10).join(LINES).encode()).hexdigest()}")
    print(LINES[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
