"""CPU: the train-mode BatchNorm entries of csrc/gcn_train.hip (and their backward companions in csrc/gcn_bwd.hip) are exported, prototyped and refuse a
NULL handle before any device call; ModulatedGCN.train_batchnorm is opt-in and every configuration the train-mode route cannot run is refused before any
device call."""
import ctypes

import pytest
import torch

NEW = {"ehm_gcn_train_workspace_bytes": 4, "ehm_gcn_train_adjacency": 4, "ehm_gcn_train_preact": 10, "ehm_gcn_train_stats": 14, "ehm_gcn_train_normalize": 10,
       "ehm_gcn_train_bn_backward": 14, "ehm_gcn_train_bwd_epilogue": 8, "ehm_gcn_train_bwd_params_workspace_bytes": 4, "ehm_gcn_train_bwd_params": 12}


@pytest.fixture(scope="module")
def L():
    from egohmr_amd import _lib
    _lib.build()
    return _lib.lib()


def test_symbols_are_exported_and_prototyped(L):
    from egohmr_amd import _lib
    for name, nargs in NEW.items():
        assert hasattr(L, name), name
        assert name in _lib.PROTOTYPES and name not in _lib.VALUE_FUNCTIONS
        assert _lib.PROTOTYPES[name][0] is ctypes.c_int and len(_lib.PROTOTYPES[name][1]) == nargs, name
        assert callable(getattr(_lib.api(), name))
    assert "gcn_train.hip" in _lib.SOURCES
    header = open(_lib.INCLUDE + "/egohmr_hip.h").read()
    for name in NEW:
        assert f"int {name}(" in header, name


def test_entries_refuse_a_null_handle_before_any_device_call(L):
    from egohmr_amd import _lib
    p = 0x10000                                                                            # never dereferenced on the host
    nb = ctypes.c_int64(-1)
    calls = {"ehm_gcn_train_workspace_bytes": (None, 0, 4, ctypes.byref(nb)),
             "ehm_gcn_train_adjacency": (None, 0, p, None),
             "ehm_gcn_train_preact": (None, 0, p, 128, 4, p, p, p, 1 << 20, None),
             "ehm_gcn_train_stats": (None, 0, p, 4, 1, 1e-5, 0.1, p, p, p, p, p, 1 << 20, None),
             "ehm_gcn_train_normalize": (None, 0, p, p, p, p, p, p, 4, None),
             "ehm_gcn_train_bn_backward": (None, 0, p, p, p, p, p, 4, p, p, p, p, 1 << 20, None),
             "ehm_gcn_train_bwd_epilogue": (None, 0, p, p, p, 128, 4, None),
             "ehm_gcn_train_bwd_params_workspace_bytes": (None, 0, 4, ctypes.byref(nb)),
             "ehm_gcn_train_bwd_params": (None, 0, p, p, p, 128, 4, p, p, p, 1 << 20, None)}
    assert set(calls) == set(NEW)
    for name, args in calls.items():
        assert getattr(L, name)(*args) == -22, name
        assert b"bad argument" in L.ehm_last_error(), name
    assert nb.value == -1
    with pytest.raises(_lib.EgoHMRHipError) as e:
        _lib.api().ehm_gcn_train_stats(None, 0, None, 0, 0, 0.0, 0.0, None, None, None, None, None, 0, None)
    assert e.value.rc == -22 and e.value.function == "ehm_gcn_train_stats"


def _module(**kw):
    from egohmr_amd.model import ModulatedGCN, smpl_tree_adjacency
    return ModulatedGCN(smpl_tree_adjacency(), in_dim=70, hid_dim=64, num_layers=1, **kw)


def test_train_batchnorm_is_opt_in():
    from egohmr_amd.model import ModulatedGCN
    assert ModulatedGCN.train_batchnorm is False
    m = _module()
    assert m.train_batchnorm is False and m.p_dropout == 0.0
    assert _module(p_dropout=None).p_dropout is None and _module(p_dropout=0.25).p_dropout == 0.25
    m.train()
    with pytest.raises(NotImplementedError, match="inference only"):
        m(torch.zeros(2, 24, 70))
    m.grad_params = True
    with pytest.raises(NotImplementedError, match="inference only"):
        m(torch.zeros(2, 24, 70).requires_grad_())


def test_train_route_refusals_come_before_any_device_call():
    """CPU tensors throughout: each refusal is raised before the device check ('needs its input on a HIP device'), which is what an accepted
    configuration then meets on this machine."""
    from egohmr_amd import _lib
    x = torch.zeros(2, 24, 70)

    def on(**kw):
        m = _module(**kw).train()
        m.train_batchnorm = True
        return m

    with pytest.raises(NotImplementedError, match="dropout"):
        on(p_dropout=0.25)(x)
    with pytest.raises(NotImplementedError, match="non-local"):
        on(nonlocal_layer=True)(x)
    m = on()
    m.precision = "f16"
    with pytest.raises(_lib.EgoHMRHipError, match="f16x3") as e:
        m(x)
    assert str(e.value) == m.GRAD_F16
    m = on()
    m.gconv_layers[0].gconv2.bn.momentum = None
    with pytest.raises(NotImplementedError, match="momentum"):
        m(x)
    m = on()
    m.gconv_input[0].bn.track_running_stats = False
    with pytest.raises(NotImplementedError, match="track_running_stats"):
        m(x)
    m = on()
    m.gconv_layers[0].gconv1.bn.eval()
    with pytest.raises(ValueError, match="eval mode"):
        m(x)
    for p_dropout in (None, 0, 0.0):                                     # accepted: the next check is the device's
        with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):
            on(p_dropout=p_dropout)(x)
    # eval() is not touched by the flag
    m = on().eval()
    with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):
        m(x)


def test_not_built_messages_keep_their_phrase():
    from egohmr_amd import diffusion, model
    with pytest.raises(NotImplementedError, match="compute_loss has a backward"):
        model.EgoHMR.training_step(None)
    with pytest.raises(NotImplementedError, match="compute_loss has a backward"):
        diffusion.GaussianDiffusion.training_losses(None, None, None, None)
