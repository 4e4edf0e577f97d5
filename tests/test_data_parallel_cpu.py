"""No GPU: the data-parallel training step's call surface - the merge of the ranks' BatchNorm statistics restated in float64 numpy against the statistics
of the concatenated rows, the exported symbols and their refusals before any launch, dist.StatSync over a gloo world of two, and the switch's default."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import bn_sync_ref as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ehm_gcn_train_stats_local": 9, "ehm_gcn_train_stats_merge": 12, "ehm_gcn_train_bwd_local": 12, "ehm_gcn_train_bwd_merge": 18,
       "ehm_bn2d_train_stats_local": 9, "ehm_bn2d_train_stats_merge": 13, "ehm_bn2d_train_bwd_local": 12, "ehm_bn2d_train_bwd_merge": 9,
       "ehm_bn2d_train_bwd_zbar_rows": 19}


# ---------------------------------------------------------------------------------------------- the merge formula
def _shards(seed, sizes, C_, offsets=None, ratio=0.0):
    g = np.random.default_rng(seed)
    out = []
    for k, n in enumerate(sizes):
        z = g.normal(size=(n, C_)) + ratio
        if offsets is not None:
            z = z + offsets[k]
        out.append(z.astype(np.float32).astype(np.float64))         # what a rank holds are float32 values
    return out


@pytest.mark.parametrize("sizes,offsets,ratio", [((48, 48), None, 0.0), ((72, 24), None, 0.0), ((5, 1, 9), None, 0.0), ((72, 24), None, 1000.0),
                                                 ((48, 48), (30.0, -30.0), 0.0), ((72, 24), (30.0, -30.0), 0.0), ((1, 1), (30.0, -30.0), 0.0)])
def test_merge_restatement_matches_the_concatenated_rows(sizes, offsets, ratio):
    """Equal and ragged shards, |mean| / sigma = 1e3, shards whose means sit at +30 sigma and -30 sigma, one row per rank: the merged (mean, var) against
    numpy's float64 two-pass statistics of all rows.  The bar is float64 rounding of well-conditioned sums: 1e-12 relative (var), 1e-12 sigma (mean)."""
    zs = _shards(len(sizes) * 7 + int(ratio), sizes, 6, offsets, ratio)
    allz = np.concatenate(zs)
    mu, var, R = S.merge_stats(np.stack([S.local_stats(z) for z in zs]), sizes)
    want_mu, want_var = allz.mean(0), allz.var(0)
    assert R == allz.shape[0]
    print(f"sizes {sizes} offsets {offsets} ratio {ratio}: max|dmean|/sigma {np.max(np.abs(mu - want_mu) / np.sqrt(want_var)):.1e}, "
          f"max rel dvar {np.max(np.abs(var - want_var) / want_var):.1e}")
    np.testing.assert_allclose(var, want_var, rtol=1e-12, atol=0)
    assert np.all(np.abs(mu - want_mu) <= 1e-12 * np.sqrt(want_var))
    rm, rv = S.running_update(np.zeros(6), np.ones(6), mu, var, R, 0.1)
    bn = torch.nn.BatchNorm1d(6).double().train()
    bn(torch.from_numpy(allz))
    np.testing.assert_allclose(rm, bn.running_mean.numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(rv, bn.running_var.numpy(), rtol=1e-12)


def test_a_world_of_one_gets_its_own_statistics_back_bit_for_bit():
    z = _shards(3, (31,), 8, ratio=50.0)[0]
    local = S.local_stats(z)
    mu, var, R = S.merge_stats(local[None], [31])
    assert np.array_equal(mu, local[0]) and np.array_equal(var, local[1] / 31.0) and R == 31


def test_scaled_shard_losses_add_up_to_the_batch_mean():
    """Why the ranks backpropagate loss_r B_r / B: every term of the loss is a mean over the items."""
    per_item = np.random.default_rng(0).normal(size=4)
    for counts in ((2, 2), (3, 1)):
        parts, at = [], 0
        for c in counts:
            parts.append(per_item[at:at + c].mean() * c / 4)
            at += c
        assert abs(sum(parts) - per_item.mean()) < 1e-15


# ---------------------------------------------------------------------------------------------- the library
def test_symbols_exported_and_bound():
    from egohmr_amd import _lib
    handle = C.CDLL(_lib.build())
    header = open(os.path.join(_lib.INCLUDE, "egohmr_hip.h")).read()
    for name, nargs in NEW.items():
        assert getattr(handle, name) is not None and name in _lib.PROTOTYPES and name in header, name
        assert len(_lib.PROTOTYPES[name][1]) == nargs and _lib.PROTOTYPES[name][0] is C.c_int, name
        assert name not in _lib.VALUE_FUNCTIONS


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """Every refusal runs before a launch: dummy addresses are never dereferenced."""
    from egohmr_amd import _lib
    L = _lib.lib()
    a, b, c, d, e, f, g, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x80000, 0x70000
    rows = lambda *v: (C.c_int64 * len(v))(*v)
    big = 1 << 40
    # a NULL handle first, as every ehm_gcn_train_* entry
    assert L.ehm_gcn_train_stats_local(None, 0, a, 4, 1, b, ws, big, None) == -22
    assert L.ehm_gcn_train_stats_merge(None, 0, a, rows(48, 48), 2, 1e-5, 0.1, b, c, None, None, None) == -22
    assert L.ehm_gcn_train_bwd_local(None, 0, a, b, c, d, e, 4, f, ws, big, None) == -22
    assert L.ehm_gcn_train_bwd_merge(None, 0, a, rows(48, 48), 2, 0, b, c, d, e, f, 2, g, None, None, ws, big, None) == -22
    # bn2d: local
    ok = (a, 1, 193, 98, 64, b, ws, big)
    assert L.ehm_bn2d_train_workspace_bytes(98, 64, C.byref(C.c_int64())) == 0
    for i, bad in ((0, None), (0, a + 4), (1, 2), (2, 97), (3, 0), (4, 48), (4, 0), (5, None), (5, b + 4), (6, None), (6, ws + 8), (7, 8)):
        args = list(ok)
        args[i] = bad
        assert L.ehm_bn2d_train_stats_local(*args, None) == -22, (i, bad)
    assert L.ehm_bn2d_train_stats_local(a, 1, 193, 98, 136, b, ws, big, None) == -22          # an X2 buffer's granule is 32 channels
    ok = (a, b, 0, 98, 98, 136, c, d, e, ws, big)
    for i, bad in ((0, None), (1, None), (2, 3), (3, 97), (4, 0), (5, 132), (6, None), (7, None), (8, None), (9, None), (10, 8)):
        args = list(ok)
        args[i] = bad
        assert L.ehm_bn2d_train_bwd_local(*args, None) == -22, (i, bad)
    # bn2d: merge - world >= 1, every rank has rows, together at least two
    ok = dict(g=a, rows=rows(98, 49), world=2, C=64, eps=1e-5, mom=0.1, mean=b, var=c, invstd=d)
    for bad in (dict(g=None), dict(g=a + 4), dict(rows=None), dict(world=0), dict(world=65), dict(rows=rows(98, 0)), dict(rows=rows(1), world=1), dict(C=0),
                dict(C=12), dict(eps=-1.0), dict(mom=1.5), dict(mean=None), dict(var=None), dict(invstd=None)):
        k = {**ok, **bad}
        assert L.ehm_bn2d_train_stats_merge(k["g"], k["rows"], k["world"], k["C"], k["eps"], k["mom"], k["mean"], k["var"], k["invstd"], None, None, None,
                                            None) == -22, bad
        assert b"bad argument" in L.ehm_last_error()
    for bad in ((None, 2, 0, 64, b, c), (a, 0, 0, 64, b, c), (a, 2, 2, 64, b, c), (a, 2, -1, 64, b, c), (a, 2, 0, 12, b, c), (a, 2, 0, 64, None, c),
                (a, 2, 0, 64, b, None)):
        assert L.ehm_bn2d_train_bwd_merge(*bad, None, None, None) == -22, bad
    ok = dict(G=a, z=b, x2=1, rows=193, mean=c, invstd=d, gamma=e, gbeta=f, ggamma=ws, scale=None, out=g, N=2, Ho=7, Wo=7, C=64, H=7, W=7, R=147)
    for bad in (dict(G=None), dict(out=None), dict(C=48), dict(N=0), dict(H=15, W=15), dict(rows=97), dict(out=a), dict(x2=2), dict(R=97), dict(R=1, N=1, Ho=1, Wo=1,
                H=1, W=1), dict(x2=1, C=136)):
        k = {**ok, **bad}
        assert L.ehm_bn2d_train_bwd_zbar_rows(k["G"], k["z"], k["x2"], k["rows"], k["mean"], k["invstd"], k["gamma"], k["gbeta"], k["ggamma"], k["scale"],
                                              k["out"], k["N"], k["Ho"], k["Wo"], k["C"], k["H"], k["W"], k["R"], None) == -22, bad


# ---------------------------------------------------------------------------------------------- the switch and StatSync
def test_the_switch_defaults_to_off_and_a_world_of_one_is_todays_route():
    from egohmr_amd import dist as edist
    from egohmr_amd.encoders import ResNet50Features
    from egohmr_amd.model import EgoHMR, ModulatedGCN
    assert EgoHMR.data_parallel is False and ModulatedGCN.stat_sync is None and ResNet50Features.stat_sync is None
    from tests.test_train_step_cpu import _cpu_model
    m = _cpu_model()
    m.data_parallel = True
    assert m._data_parallel_world() == 1                               # no process group
    s = edist.StatSync.exchange(3)
    assert s.counts == [3] and s.world == 1 and s.rank == 0 and s.loss_weight == 1.0 and list(s.rows(24)) == [72]
    loc = torch.arange(8, dtype=torch.float64).reshape(2, 4)
    assert torch.equal(s.gather(loc), loc[None])
    with pytest.raises(ValueError, match="at least one item"):
        edist.StatSync([2, 0], 0)
    with pytest.raises(ValueError, match="rank"):
        edist.StatSync([2, 2], 2)
    # the "fewer than two values per channel" refusal looks at all ranks' rows
    bb = ResNet50Features().train()
    bb.train_batchnorm = True
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        bb(torch.zeros(1, 3, 32, 32))
    bb.stat_sync = edist.StatSync([1, 1], 0)
    from egohmr_amd import _lib
    with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):        # two rows in all: nothing left to refuse but the CPU tensor
        bb(torch.zeros(1, 3, 32, 32))


_RANK = r"""
import json, sys, torch, torch.distributed as td
sys.path.insert(0, {repo!r})
from egohmr_amd import dist as edist
rank, counts = int(sys.argv[1]), json.loads(sys.argv[3])
td.init_process_group("gloo", init_method="file://" + sys.argv[2], rank=rank, world_size=len(counts))
res = dict()
s = edist.StatSync.exchange(counts[rank])
res["counts"], res["rank"], res["weight"], res["rows"] = s.counts, s.rank, s.loss_weight, list(s.rows(24))
local = torch.full((2, 5), float(rank + 1), dtype=torch.float64) * torch.arange(1, 6, dtype=torch.float64)
res["gathered"] = s.gather(local).tolist()
flat = torch.arange(4, dtype=torch.float32) + rank
res["reduced"] = edist.all_reduce_sum_(flat).tolist()
try:
    edist.StatSync.exchange(0 if rank == 1 else 2)
    res["refused"] = False
except ValueError as e:
    res["refused"] = str(e)
td.barrier()
td.destroy_process_group()
json.dump(res, open(sys.argv[4], "w"))
"""


@pytest.mark.parametrize("counts", [[2, 2], [3, 1]])
def test_statsync_over_a_gloo_world_of_two(tmp_path, counts):
    """4 items as 2 + 2 and 3 + 1: the count exchange, the loss weights B_r / B, gather in rank order, the flat SUM, and a rank without items refused on BOTH
    ranks after the exchange."""
    script = tmp_path / "rank.py"
    script.write_text(_RANK.format(repo=REPO))
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(tmp_path / "rendezvous"), json.dumps(counts), str(tmp_path / f"out{r}.json")],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    for p in procs:
        log, _ = p.communicate(timeout=120)
        assert p.returncode == 0, log.decode()[-2000:]
    for r in range(2):
        res = json.load(open(tmp_path / f"out{r}.json"))
        assert res["counts"] == counts and res["rank"] == r and res["weight"] == counts[r] / 4 and res["rows"] == [24 * c for c in counts]
        want = [[[float(k + 1) * j for j in range(1, 6)]] * 2 for k in range(2)]
        assert res["gathered"] == want
        assert res["reduced"] == [1.0, 3.0, 5.0, 7.0]
        assert res["refused"] and "at least one item" in res["refused"]
    assert sum(counts[r] / 4 for r in range(2)) == 1.0
