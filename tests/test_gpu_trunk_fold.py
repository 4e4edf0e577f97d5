"""GPU (MI355X): the host side of the folded trunk (egohmr_amd/encoders.py FoldedTrunk) - what it packs and what it keeps between calls, the state it
declares, the record argument of the train route - and the path of split_gemm.pack_weight that packs an already padded matrix without a copy.  The
values the trunk computes are pinned by the other trunk tests; the C entry points are counted with the recorder of test_gpu_trunk_walk."""
import pytest
import torch

from tests import trunk_grad_ref as R
from tests import trunk_train_ref as T
from tests.test_gpu_trunk_walk import calls  # noqa: F401  (the recorder fixture)

pytestmark = pytest.mark.gpu

SEED = 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return R.make_state(SEED)


def packs(seen):
    """the ehm_split_pack calls recorded since the last look"""
    n = sum(1 for name, _ in seen if name == "ehm_split_pack")
    del seen[:]
    return n


# ehm_split_pack calls of a forward, counted once on the closure this class replaced.  Eval: 16 blocks x 3 convs, the four projections inside the
# dual packs of their conv3 (apart with fuse_shortcut=False).  Train: 52 raw units, then 32 folded conv1 / conv2 and 16 folded conv3 (+ projection)
@pytest.mark.parametrize("kw, want", [({}, 48), (dict(fuse_shortcut=False), 52)])
def test_eval_runner_packs_on_its_first_call_only(dev, sd, calls, kw, want):  # noqa: F811
    fn = R.load_module(sd, dev).folded(**kw)
    img = R.make_image(1, 32, 32, SEED).float().to(dev)
    assert packs(calls) == 0                               # (folding packs nothing)
    first = fn(img)
    assert packs(calls) == want
    second = fn(img)
    assert packs(calls) == 0
    assert torch.equal(first, second)


def test_train_route_keeps_no_pack(dev, sd, calls):  # noqa: F811
    m = T.load_module(sd, dev)
    img = R.make_image(2, 64, 64, SEED).float().to(dev)
    with torch.no_grad():
        m(img)
        assert packs(calls) == 100
        m(img)
        assert packs(calls) == 100


@pytest.mark.parametrize("Co, K", [(128, 64), (72, 40)])
def test_pack_weight_equals_a_direct_pack_of_the_padded_matrix(dev, Co, K):
    """[128, 64] has the padded shape already (packed as it is), [72, 40] is padded both ways: buffer and scale byte for byte."""
    from egohmr_amd import _lib
    from egohmr_amd.split_gemm import pack_weight, round_up, weight_scale
    w = torch.randn(Co, K, generator=torch.Generator().manual_seed(Co)).to(dev)
    before = w.clone()
    packed = pack_weight(w)
    Cp, Kp = round_up(Co, 128), round_up(K, 32)
    wp = torch.zeros(Cp, Kp, device=dev)
    wp[:Co, :K] = w
    scale = weight_scale(float(wp.abs().max()))
    buf = torch.full((Cp, Kp), float("nan"), device=dev)
    _lib.api().ehm_split_pack(wp, buf, Cp, Kp, Kp, scale, _lib.stream_ptr())
    assert packed.scale == scale and packed.cols == round_up(Co, 8) and packed.bias is None
    assert packed.buf.shape == buf.shape and packed.buf.dtype == buf.dtype
    assert torch.equal(packed.buf.view(torch.int32), buf.view(torch.int32))
    assert torch.equal(w, before)                          # (the unpadded path reads the caller's matrix in place)


def test_state_is_declared_and_goes_with_the_weights(dev, sd):
    m = R.load_module(sd, dev)
    fn = m.folded()
    for name in ("stem", "blocks", "stem_wt", "stem_b", "dgrad"):
        assert hasattr(fn, name), name
    assert len(fn.stem) == 4 and len(fn.blocks) == 16 and all(len(b) == 4 for b in fn.blocks)
    assert fn.stem_wt.shape == (147, 64) and fn.stem_b.shape == (64,)
    assert fn.dgrad == {}
    img, gout = R.make_image(1, 32, 32, SEED).float().to(dev), R.make_cotangent(1, SEED).float().to(dev)
    m.grad_params = True
    cur = m.current()
    with torch.no_grad():
        m(img)
    assert cur.dgrad == {}                                 # a forward packs no data-gradient weight
    m(img).backward(gout)
    assert m.current() is cur and sorted(cur.dgrad) == [i for i, u in enumerate(R.unit_names()) if u is not None and i > 0]
    m.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in R.make_state(SEED + 1).items()})
    new = m.current()
    assert new is not cur and new.dgrad == {}


def test_record_goes_in_as_rec(dev, sd, calls):  # noqa: F811
    from egohmr_amd import trunk_grad
    m = T.load_module(sd, dev)
    img = R.make_image(2, 64, 64, SEED).float().to(dev)
    units = R.unit_names()
    rec = trunk_grad.TrainRecord()
    out = m.folded(train=True)(img, rec=rec)
    assert out.shape == (2, 2048) and bool(torch.isfinite(out).all())
    assert len(rec.acts) == 1 + 3 * 16 and len(rec.bn) == len(units)
    assert all((e is None) == (u is None) for e, u in zip(rec.bn, units))
    assert rec.stem_wt.shape == (147, 64) and rec.stem_b.shape == (64,)
    torch.cuda.synchronize()
    del calls[:]
    with pytest.raises(TypeError):
        m.folded(train=True)(img, trunk_grad.TrainRecord())
    assert calls == []                                     # refused before any device call
