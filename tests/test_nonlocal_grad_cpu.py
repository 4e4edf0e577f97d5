"""No GPU: the call surface of the non-local block's backward behind ModulatedGCN.nonlocal_grad - the flag and its default, what is refused with it off and
what no longer is with it on, grad_parameters' list, the exported entry and its argument checks - and the float64 restatement of tests/nonlocal_ref.py
pinned to the reference's own ModulatedGCN(nonlocal_layer=True) in .train() and .eval() (tests/golden/g22_nonlocal_train.npz, written by
tests/make_nonlocal_golden.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nonlocal_ref as NR  # noqa: E402
import val_losses_ref as R  # noqa: E402

OLD = "non-local block has no backward"


def _gcn(**kw):
    from egohmr_amd.model import ModulatedGCN, smpl_tree_adjacency
    return ModulatedGCN(smpl_tree_adjacency(), in_dim=70, hid_dim=64, num_layers=1, **kw)


def _cpu_model(**kw):
    from egohmr_amd.factory import build_synthetic_model
    return build_synthetic_model("cpu", 0, **R.CASE_WEIGHTS, start_coap_epoch=R.START_COAP_EPOCH, **kw)


def _cpu_batch(golden_dir, B=2):
    from egohmr_amd.factory import batch_to_device
    g = np.load(os.path.join(golden_dir, "g21_val_losses_a.npz"))
    b_np, flags = R.golden_batch(g)
    cut = lambda d: {k: (cut(v) if isinstance(v, dict) else v[:B]) for k, v in d.items()}
    batch = batch_to_device(cut(b_np), "cpu")
    batch["smpl_params_is_axis_angle"] = {k: v[:B] for k, v in flags.items()}
    return batch


def test_flag_exists_and_is_off():
    from egohmr_amd.model import ModulatedGCN
    assert ModulatedGCN.nonlocal_grad is False
    assert _gcn(nonlocal_layer=True).nonlocal_grad is False


def test_grad_parameters_appends_the_blocks_ten():
    m = _gcn(nonlocal_layer=True)
    off = m.grad_parameters()
    plain = _gcn().grad_parameters()
    assert len(off) == len(plain) == 6 * 3 + 4
    m.nonlocal_grad = True
    on = m.grad_parameters()
    assert len(on) == len(off) + 10 and all(a is b for a, b in zip(on, off))
    names = {id(p): n for n, p in m.named_parameters()}
    assert [names[id(p)] for p in on[len(off):]] == ["non_local." + k for k in NR.BLOCK_PARAMS]
    assert [names[id(p)] for p in on] == NR.grad_names(1)
    m.nonlocal_grad = False
    assert all(a is b for a, b in zip(m.grad_parameters(), off)) and len(m.grad_parameters()) == len(off)
    p = _gcn()
    p.nonlocal_grad = True                                   # without the block the flag changes nothing
    assert len(p.grad_parameters()) == len(plain)


def test_module_refusals_with_the_flag_off_and_the_device_check_with_it_on():
    from egohmr_amd import _lib
    x = torch.zeros(2, 24, 70)
    m = _gcn(nonlocal_layer=True).train()
    m.train_batchnorm = True
    with pytest.raises(NotImplementedError, match=OLD):
        m(x)
    m.nonlocal_grad = True
    with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):
        m(x)
    m.precision = "f16"                                      # plain f16 stays refused
    with pytest.raises(_lib.EgoHMRHipError) as e:
        m(x)
    assert str(e.value) == m.GRAD_F16
    m.precision = "f16x3"
    m.non_local.W[1].eval()                                  # W.1 takes part in the mode check
    with pytest.raises(ValueError, match="BatchNorm2d is in eval mode"):
        m(x)
    m.train()
    m.non_local.W[1].momentum = None
    with pytest.raises(NotImplementedError, match="momentum"):
        m(x)


def test_forward_saving_refusal(monkeypatch):
    from egohmr_amd import gcn_grad
    m = _gcn(nonlocal_layer=True).eval()

    def no_device_call(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(m, "_native", no_device_call)
    with pytest.raises(NotImplementedError, match=OLD):
        gcn_grad.forward_saving(m, torch.zeros(1, 24, 70))
    m.nonlocal_grad = True
    with pytest.raises(AssertionError, match="a device call was made"):
        gcn_grad.forward_saving(m, torch.zeros(1, 24, 70))


def test_egohmr_refusals_with_the_flag_off_and_the_device_check_with_it_on(golden_dir):
    from egohmr_amd import _lib
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.model import EgoHMR
    _lib.build()
    d = create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="")
    t = torch.tensor([0, 49])
    batch = _cpu_batch(golden_dir)
    batch["x_t"] = torch.zeros(2, 144)                       # (training_losses draws its own; training_step reads the caller's)
    m = _cpu_model(gcn_nonlocal_layer=True)
    m.frozen_trunk_training = True
    m.init_optimizers()
    assert all(any(p is q for q in m.opt_params) for p in m.diffusion_model.non_local.parameters())
    for call in (lambda: m.training_step(batch, t, 0), lambda: d.training_losses(m, batch, t, noise=torch.zeros(2, 144))):
        with pytest.raises(NotImplementedError, match=OLD):
            call()
    m.diffusion_model.nonlocal_grad = True
    for call in (lambda: m.training_step(batch, t, 0), lambda: d.training_losses(m, batch, t, noise=torch.zeros(2, 144))):
        with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):
            call()
    assert "the non-local block's backward" in EgoHMR.NOT_BUILT
    m.validation_setup()
    assert not m.training and not m.diffusion_model.training


def test_entry_declared_exported_and_bound():
    from egohmr_amd import _lib
    handle = C.CDLL(_lib.build())
    hdr = open(os.path.join(_lib.INCLUDE, "egohmr_hip.h")).read()
    for name, nargs in (("ehm_nonlocal_attention_backward", 6), ("ehm_nonlocal_bn_residual", 10)):
        assert getattr(handle, name) is not None and name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs
        assert f"int {name}(" in hdr
    assert "nonlocal_bwd.hip" in _lib.SOURCES


def test_entry_refuses_bad_arguments_without_a_gpu():
    """EHM_CHECK_ARG runs before any launch: null pointers, bodies <= 0 or past the grid limit, Ci <= 0."""
    from egohmr_amd import _lib
    L = C.CDLL(_lib.build())
    f = L.ehm_nonlocal_attention_backward
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.ehm_last_error.restype = C.c_char_p
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    for args in ((None, p, p, 1, 32), (p, None, p, 1, 32), (p, p, None, 1, 32), (p, p, p, 0, 32), (p, p, p, -3, 32), (p, p, p, 1 << 31, 32),
                 (p, p, p, 1, 0), (p, p, p, 1, -64)):
        assert f(*args, None) == -22, args
        assert b"bad argument" in L.ehm_last_error() and b"ehm_nonlocal_attention_backward" in L.ehm_last_error()
    with pytest.raises(_lib.EgoHMRHipError, match="bad argument"):
        _lib.api().ehm_nonlocal_attention_backward(None, None, None, 1, 32, None)


# ---------------------------------------------------------------------------------------------- the restatement against the reference's own module
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "g22_nonlocal_train.npz"))


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_restatement_matches_the_reference_module(golden, mode):
    """Both sides float64: rtol 1e-9, atol 1e-12 max|ref| - about 1e3 operations with about 1e3 of cancellation on 2^-52."""
    from oracle import model as om
    g = golden
    sd, x = NR.module_state(int(g["seed"]), in_dim=int(g["in_dim"]), hid=int(g["hid"]), blocks=int(g["blocks"]), bodies=g["x"].shape[0])
    assert np.array_equal(x.numpy(), g["x"])
    res = NR.run(sd, x, torch.from_numpy(g["cot"]), om.smpl_adjacency(torch.float64), int(g["blocks"]), train=mode == "train")

    def check(tag, got, want):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-9, atol=1e-12 * float(np.abs(want).max()), err_msg=tag)
    check("out", res["out"], g[mode + ".out"])
    check("gx", res["gx"], g[mode + ".gx"])
    names = NR.grad_names(int(g["blocks"]))
    assert sorted(k[len(mode) + 6:] for k in g.files if k.startswith(mode + ".grad.")) == sorted(names)
    for n in names:
        want = g[f"{mode}.grad.{n}"]
        if mode == "train" and (n.endswith("gconv.bias") and not n.startswith("gconv_output") or n.endswith("W.0.bias") or n.endswith(".g.bias")):
            # a bias in front of a train-mode BatchNorm (g's reaches W.1 as a constant per channel: the rows of P sum to one): zero, to rounding on both
            # sides - against the scale of that BatchNorm's beta gradient
            beta = n.replace("gconv.bias", "bn.bias").replace("W.0.bias", "W.1.bias").replace(".g.bias", ".W.1.bias")
            scale = float(np.abs(g[f"{mode}.grad.{beta}"]).max())
            assert float(np.abs(want).max()) <= 1e-9 * scale and float(res["grads"][n].abs().max()) <= 1e-9 * scale, n
            continue
        if n.endswith("phi.bias"):
            # phi's bias adds theta_a . b to every logit of row a, which the softmax does not see: zero in both modes, to rounding on both sides - against
            # the scale of theta's bias gradient, a sum of the same terms that does not cancel
            scale = float(np.abs(g[f"{mode}.grad.{NR.NL}theta.bias"]).max())
            assert float(np.abs(want).max()) <= 1e-9 * scale and float(res["grads"][n].abs().max()) <= 1e-9 * scale, n
            continue
        check(n, res["grads"][n], want)
    for k in ("running_mean", "running_var"):
        check(k, res["sd"][f"non_local.W.1.{k}"], g[f"{mode}.non_local.W.1.{k}"])
    assert int(g[f"{mode}.non_local.W.1.num_batches_tracked"]) == (1 if mode == "train" else 0)
    if mode == "eval":
        assert np.array_equal(res["sd"]["non_local.W.1.running_mean"].numpy(), sd["non_local.W.1.running_mean"].numpy())
