"""CPU: the general SMPL VJP (ehm_smpl_backward) is exported, prototyped and refuses bad arguments before any device call; the pluggable
collision model defaults to the build's proxy; a CPU-tensor SMPL.forward with requires_grad inputs still raises the package's error."""
import ctypes

import pytest
import torch

NEW = ("ehm_smpl_backward", "ehm_smpl_backward_workspace_bytes")


@pytest.fixture(scope="module")
def L():
    from egohmr_amd import _lib
    _lib.build()
    return _lib.lib()


def _fake_handle(V=6890, n_extra=21):
    """Host memory laid out like the head of an ehm_smpl (SmplDev: int V, int n_extra, ...): enough for the size arithmetic, which is all an entry point
    may read before it has accepted its arguments.  Nothing here is ever handed to a device."""
    buf = (ctypes.c_int32 * 256)()
    buf[0], buf[1] = V, n_extra
    return buf


def test_symbols_are_exported_and_prototyped(L):
    from egohmr_amd import _lib
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.PROTOTYPES and name not in _lib.VALUE_FUNCTIONS          # status returns: the size comes back through a pointer
        assert _lib.PROTOTYPES[name][0] is ctypes.c_int
        assert callable(getattr(_lib.api(), name))
    assert len(_lib.PROTOTYPES["ehm_smpl_backward"][1]) == 11
    assert len(_lib.PROTOTYPES["ehm_smpl_backward_workspace_bytes"][1]) == 3


def test_workspace_bytes_argument_checks_and_size(L):
    nb = ctypes.c_int64(-1)
    h = _fake_handle()
    assert L.ehm_smpl_backward_workspace_bytes(None, 4, ctypes.byref(nb)) == -22 and b"bad argument" in L.ehm_last_error()
    assert L.ehm_smpl_backward_workspace_bytes(h, 0, ctypes.byref(nb)) == -22
    assert L.ehm_smpl_backward_workspace_bytes(h, 4, None) == -22
    assert nb.value == -1
    assert L.ehm_smpl_backward_workspace_bytes(h, 4, ctypes.byref(nb)) == 0
    small = nb.value
    assert small >= 4 * 6890 * 3 * 4 + 4 * 24 * (9 + 12 + 12) * 4                  # at least the private vertex cotangent + R, A, gA
    assert L.ehm_smpl_backward_workspace_bytes(h, 257, ctypes.byref(nb)) == 0 and nb.value > small


def test_backward_refuses_bad_arguments_without_a_gpu(L):
    """EINVAL before any device call: there is no GPU here, so anything that reached the runtime would not come back as -22."""
    h = _fake_handle()
    nb = ctypes.c_int64()
    B = 4
    assert L.ehm_smpl_backward_workspace_bytes(h, B, ctypes.byref(nb)) == 0
    betas, rot, gv, gj, gb, gr, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000      # never dereferenced on the host
    ok = dict(h=h, betas=betas, rotmats=rot, gverts=gv, gjoints=gj, gbetas=gb, grotmats=gr, B=B, ws=ws, nbytes=nb.value)

    def call(**kw):
        a = {**ok, **kw}
        return L.ehm_smpl_backward(a["h"], a["betas"], a["rotmats"], a["gverts"], a["gjoints"], a["gbetas"], a["grotmats"], a["B"], a["ws"], a["nbytes"], None)

    bad = [dict(h=None),                                   # null handle
           dict(gverts=None, gjoints=None),                # no gradient input
           dict(gbetas=None, grotmats=None),               # no gradient output
           dict(nbytes=nb.value - 1), dict(nbytes=0),      # a workspace that is too small
           dict(ws=None), dict(ws=ws + 4),                 # no / a misaligned workspace
           dict(betas=None), dict(rotmats=None), dict(B=0), dict(B=-3)]
    for kw in bad:
        assert call(**kw) == -22, kw
        assert b"bad argument" in L.ehm_last_error()


def test_checked_view_raises_on_bad_arguments(L):
    from egohmr_amd import _lib
    with pytest.raises(_lib.EgoHMRHipError) as e:
        _lib.api().ehm_smpl_backward(None, None, None, None, None, None, None, 0, None, 0, None)
    assert e.value.rc == -22 and e.value.function == "ehm_smpl_backward"
    with pytest.raises(_lib.EgoHMRHipError) as e:
        _lib.api().ehm_smpl_backward_workspace_bytes(None, 1, None)
    assert e.value.rc == -22 and e.value.function == "ehm_smpl_backward_workspace_bytes"


def test_collision_model_defaults_to_none(synth_weights, smpl_asset):
    from egohmr_amd import _lib
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import build_synthetic_model
    m = build_synthetic_model(torch.device("cpu"), 0, diffuse_fuse=True, state_dict=synth_weights, smpl_asset=smpl_asset)
    assert m.collision_model is None
    assert "collision_model" not in "".join(m.state_dict().keys())
    # attached: the one-call loop refuses a guided run before it looks at anything else (no silent use of the proxy) ...
    m.collision_model = object()
    d = create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="")
    with pytest.raises(_lib.EgoHMRHipError, match="collision_model"):
        m.fused_sampler.run(d, {}, torch.zeros(51, 1, 144), ddim=False, guided=True)
    # ... and the samplers route such a loop step by step
    assert not d._fused_ok(m, 0, None, None, False, 0.0, guided=True) and d._fused_ok(m, 0, None, None, False, 0.0, guided=False)
    m.collision_model = None
    assert d._fused_ok(m, 0, None, None, False, 0.0, guided=True)


def test_guided_loop_with_a_collision_model_is_not_fused():
    """The routing rule, on stand-ins: guided + collision_model -> generic route; everything else as before."""
    from types import SimpleNamespace
    from egohmr_amd.diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="")
    plain = SimpleNamespace(fused_sampler=object(), collision_model=None)
    plugged = SimpleNamespace(fused_sampler=object(), collision_model=object())
    assert d._fused_ok(plain, 0, None, None, False, 0.0) and d._fused_ok(plain, 0, None, None, False, 0.0, guided=True)
    assert d._fused_ok(plugged, 0, None, None, False, 0.0) and d._fused_ok(plugged, 0, None, None, False, 0.0, guided=False)
    assert not d._fused_ok(plugged, 0, None, None, False, 0.0, guided=True)


def test_cpu_forward_with_requires_grad_raises_the_hip_device_error(smpl_asset):
    from egohmr_amd import _lib
    from egohmr_amd.smpl import SMPL
    smpl = SMPL(smpl_asset)
    betas = torch.zeros(2, 10, requires_grad=True)
    R = torch.eye(3).expand(2, 24, 3, 3).clone().requires_grad_()
    with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):
        smpl(betas=betas, body_pose=R[:, 1:], global_orient=R[:, [0]], pose2rot=False)
    with pytest.raises(_lib.EgoHMRHipError, match="HIP device"):
        smpl(betas=betas, body_pose=torch.zeros(2, 69, requires_grad=True), global_orient=torch.zeros(2, 3, requires_grad=True))
