"""CPU: the prepared batch of the sampling engine (egohmr_amd/fused.py): the one function that builds the second-pass map from a per-item
`need` mask, and the two operations on a prepared batch - `take` (some items) and `tile` (the batch S times, sample-major).  `tile` builds
its map by offset arithmetic (no host read-back); this file ties it to the function.  Plain torch on CPU tensors, no library load."""
import dataclasses

import pytest
import torch

from egohmr_amd.fused import _Prepared, pass_map

SIZES, RATES = (1, 3, 11, 64, 257), (0.0, 0.3, 1.0)


def _need(B, rate, seed=0):
    g = torch.Generator().manual_seed(1000 * B + int(10 * rate) + seed)
    return torch.rand(B, generator=g) < rate            # rate 0 -> none, rate 1 -> all (rand is in [0, 1))


@dataclasses.dataclass
class _WithTable(_Prepared):
    table: torch.Tensor = None                          # NOT per item, though it will have B rows


def _prepared(B, rate, cls=_Prepared, **extra):
    """A prepared batch of distinguishable CPU tensors whose pass map is the function's on `vis`."""
    g = torch.Generator().manual_seed(7 * B + int(10 * rate))
    need = _need(B, rate)
    vis = torch.ones(B, 24, dtype=torch.uint8)
    vis[need, torch.randint(0, 24, (int(need.sum()),), generator=g)] = 0       # items with `need` have one invisible joint
    r = lambda *shape: torch.randn(B, *shape, generator=g)
    items, slot, n = pass_map(need)
    return cls(B=B, h_img=r(2, 8), h_oth=r(2, 8), vis=vis, vis_bool=vis.view(torch.bool), betas=r(10), scene=r(5, 3), transl=r(3), fx=r(), cam_cx=r(),
               cam_cy=r(), img_feats=r(16), scene_feats=r(4), finite=torch.rand(B, generator=g) < 0.9, mask_items=items, mask_slot=slot, num_masked=n,
               inputs=[vis], **extra), need


def _assert_map(got, need):
    """`got` = (mask_items, mask_slot, num_masked) is the pass map of `need` by its definition, spelled out item by item."""
    items, slot, n = got
    want_items = [b for b in range(need.numel()) if need[b]]
    want_slot = [want_items.index(b) if need[b] else -1 for b in range(need.numel())]
    assert n == len(want_items) and isinstance(n, int)
    assert items.tolist() == want_items and slot.tolist() == want_slot
    assert items.dtype == torch.int32 and slot.dtype == torch.int32 and items.is_contiguous() and slot.is_contiguous()
    assert items.shape == (n,) and slot.shape == (need.numel(),)


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("rate", RATES)
def test_pass_map_is_ascending_items_rank_or_minus_one_and_count(B, rate):
    need = _need(B, rate)
    assert int(need.sum()) == (0 if rate == 0.0 else B if rate == 1.0 else int(need.sum()))
    _assert_map(pass_map(need), need)


def test_per_item_fields_are_declared_and_are_fields():
    names = {f.name for f in dataclasses.fields(_Prepared)}
    assert set(_Prepared.PER_ITEM) <= names
    assert names - set(_Prepared.PER_ITEM) == {"B", "inputs", "mask_items", "mask_slot", "num_masked"}


@pytest.mark.parametrize("S", (1, 2, 5))
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("rate", RATES)
def test_tile_is_the_pass_map_of_the_repeated_need_and_replicates_sample_major(B, rate, S):
    st, need = _prepared(B, rate)
    t = st.tile(S)
    assert t.B == S * B and type(t) is _Prepared
    items, slot, n = pass_map(need.repeat(S))
    assert t.num_masked == n and torch.equal(t.mask_items, items) and torch.equal(t.mask_slot, slot)
    _assert_map((t.mask_items, t.mask_slot, t.num_masked), need.repeat(S))
    for k in _Prepared.PER_ITEM:
        v, w = getattr(st, k), getattr(t, k)
        assert w.shape == (S * B, *v.shape[1:]) and w.dtype == v.dtype and w.is_contiguous(), k
        for s in range(S):
            assert torch.equal(w[s * B:(s + 1) * B], v), (k, s)                # body s * B + b is item b
    assert t.inputs is st.inputs


def test_tile_keeps_no_map_as_no_map():
    st, _ = _prepared(11, 0.3)
    st = dataclasses.replace(st, num_masked=-1)
    assert st.tile(1).num_masked == -1 and st.tile(3).num_masked == -1 and st.tile(3).B == 33


def _indices(B):
    g = torch.Generator().manual_seed(B)
    n, k = 2 * B + 1, max(B // 2, 1)
    yield "permuted", torch.randperm(B, generator=g)
    yield "repeated", torch.arange(n) % k                                      # as calibrate_schedule replicates the finite items
    yield "int32", torch.randperm(B, generator=g)[: max(B // 3, 1)].to(torch.int32)


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("rate", RATES)
def test_take_selects_the_declared_fields_and_rebuilds_the_pass_map(B, rate):
    st, need = _prepared(B, rate)
    for name, idx in _indices(B):
        t = st.take(idx)
        sel = idx.long()
        assert t.B == sel.numel() and type(t) is _Prepared, name
        for k in _Prepared.PER_ITEM:
            assert torch.equal(getattr(t, k), getattr(st, k).index_select(0, sel)) and getattr(t, k).is_contiguous(), (name, k)
        want = ~t.vis_bool.all(dim=1)
        assert torch.equal(want, need[sel]), name
        items, slot, n = pass_map(want)
        assert t.num_masked == n and torch.equal(t.mask_items, items) and torch.equal(t.mask_slot, slot), name
        _assert_map((t.mask_items, t.mask_slot, t.num_masked), need[sel])
        assert t.inputs is st.inputs


def test_take_of_items_that_all_see_every_joint_has_an_empty_map():
    st, need = _prepared(64, 0.3)
    idx = torch.nonzero(~need).reshape(-1).flip(0)
    t = st.take(idx)
    assert t.num_masked == 0 and t.mask_items.numel() == 0 and t.mask_slot.tolist() == [-1] * idx.numel()
    assert t.mask_items.dtype == torch.int32 and t.mask_slot.dtype == torch.int32


def test_take_int_is_the_first_n_and_the_whole_batch_is_itself():
    st, need = _prepared(11, 0.3)
    assert st.take(11) is st and st.take(400) is st
    t = st.take(4)
    assert t.B == 4 and torch.equal(t.h_img, st.h_img[:4]) and torch.equal(t.vis, st.vis[:4])
    _assert_map((t.mask_items, t.mask_slot, t.num_masked), need[:4])


@pytest.mark.parametrize("B", (3, 11))
def test_a_field_with_B_rows_that_is_not_per_item_is_left_alone(B):
    """What a `shape[0] == B` rule gets wrong: a table that happens to have B rows is neither re-indexed nor replicated."""
    table = torch.arange(B * 2.0).reshape(B, 2)
    st, _ = _prepared(B, 0.3, cls=_WithTable, table=table)
    for r in (st.take(torch.arange(B).flip(0)), st.take(B - 1), st.take(torch.arange(2 * B) % B), st.tile(2), st.tile(5)):
        assert type(r) is _WithTable and r.table is table and r.inputs is st.inputs
        assert r.h_img.shape[0] == r.B and r is not st
    assert torch.equal(st.take(torch.arange(B).flip(0)).h_img, st.h_img.flip(0))      # (the per-item fields did move)
