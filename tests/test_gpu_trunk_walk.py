"""GPU (MI355X): WHICH launches the backward of ResNet50Features makes (egohmr_amd/trunk_grad.py `_walk`), on the eval-mode route and on the train-mode
BatchNorm route.  The other trunk tests pin the values; here the C entry points a backward calls are recorded - the attributes of the namespace
`_lib.api()` returns are wrapped for the test's duration - and counted: no data gradient (ehm_conv_nhwc_split) below the lowest unit that wants
something, the projection blocks' shared column sum taken once, and the same sequence on every call.

One module per route from trunk_grad_ref.make_state at (2, 64, 64): the smallest shape at which layer 4 has more than two rows per channel."""
import pytest
import torch

from tests import trunk_grad_ref as R
from tests import trunk_train_ref as T

pytestmark = pytest.mark.gpu

SHAPE, SEED = (2, 64, 64), 2
TOP = "layer4.2.bn3.bias"
# need pattern -> (the parameters that train, ehm_conv_nhwc_split calls of one backward on either route)
PATTERNS = {
    "all": (lambda n: True, 52),                                                # 16 blocks x 3 convs + the 4 projections
    "top-bias": (lambda n: n == TOP, 0),
    "top-bias+layer2-projection": (lambda n: n in (TOP, "layer2.0.downsample.0.weight"), 38),   # 12 whole blocks above block 3, two of them projections
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def case(dev):
    B, H, W = SHAPE
    sd = R.make_state(SEED)
    mods = dict(eval=R.load_module(sd, dev), train=T.load_module(sd, dev))
    img, gout = R.make_image(B, H, W, SEED).float().to(dev), R.make_cotangent(B, SEED).float().to(dev)
    for m in mods.values():
        m.grad_params = True
        m(img).backward(gout)                  # the eval route packs its 52 data-gradient weights on first use: done here, so two later calls are alike
        m.zero_grad(set_to_none=True)
    return dict(mods=mods, img=img, gout=gout)


@pytest.fixture
def calls(monkeypatch):
    """Every call through `_lib.api()` while the test runs, as (entry-point name, its scalar arguments; "ptr" for whatever else is not None)."""
    from egohmr_amd import _lib
    A, seen = _lib.api(), []
    for name, fn in list(vars(A).items()):
        def call(*args, _fn=fn, _name=name):
            seen.append((_name, tuple(a if a is None or isinstance(a, (int, float)) else "ptr" for a in args)))
            return _fn(*args)
        monkeypatch.setattr(A, name, call)
    return seen


def backward_calls(m, case, calls, trains):
    """The calls of one backward with the parameters `trains` selects trainable; the parameters are left trainable."""
    try:
        for n, p in m.named_parameters():
            p.requires_grad_(bool(trains(n)))
        m.zero_grad(set_to_none=True)
        out = m(case["img"])
        del calls[:]
        out.backward(case["gout"])
        torch.cuda.synchronize()
        got = {n for n, p in m.named_parameters() if p.grad is not None}
        assert got == {n for n, _ in m.named_parameters() if trains(n)}
        return list(calls)
    finally:
        for p in m.parameters():
            p.requires_grad_(True)
        m.zero_grad(set_to_none=True)


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("route", ["eval", "train"])
def test_data_gradients_stop_at_the_lowest_unit(dev, case, calls, route, pattern):
    trains, want = PATTERNS[pattern]
    m = case["mods"][route]
    first = backward_calls(m, case, calls, trains)
    second = backward_calls(m, case, calls, trains)
    dgrads = sum(1 for name, _ in first if name == "ehm_conv_nhwc_split")
    print(f"[{route}, {pattern}] {len(first)} calls in one backward, {dgrads} data gradients")
    assert dgrads == want
    assert [name for name, _ in first] == [name for name, _ in second]


def test_bias_only_takes_the_shared_column_sum_once(dev, case, calls):
    """Eval route, only the 53 BatchNorm biases trainable: a projection block's downsample unit wants nothing but the column sum its conv3 already
    produced, so no weight-gradient launch runs for it - 16 x 3 launches in all, none with a weight-gradient output, none with a projection's geometry."""
    seq = backward_calls(case["mods"]["eval"], case, calls, lambda n: n.endswith(".bias"))
    wgrads = [args for name, args in seq if name == "ehm_conv_bwd_wgrad"]
    # ehm_conv_bwd_wgrad(G, x, x_rows, gW, gb, N, H, W, Ci, Co, K, stride, pad, ...)
    assert all(a[3] is None and a[4] is not None for a in wgrads)
    assert not [a for a in wgrads if a[10] == 1 and a[11] == 2]                  # (1 x 1, stride 2: the projections of layers 2 - 4)
    assert len(wgrads) == 48                                                     # ... and layer 1's: one launch per conv1 / conv2 / conv3 only
