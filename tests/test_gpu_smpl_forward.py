"""GPU (MI355X): the forward entries of csrc/smpl.hip - ehm_smpl_forward, ehm_smpl_forward_rot6d, ehm_rot6d_to_rotmat, the refusals of
ehm_smpl_create - through the C ABI, against the float64 oracle (oracle.smpl.SMPLOracle) under the derived bound of tests/smpl_ref.py (its module
docstring counts every constant; tests/test_smpl_ref_cpu.py shows on the CPU that the bound tells a broken hi / lo split of the blend from the faithful
one).  No comparison against float64 here uses a bare number: every one is error <= bound / bound_valu, and the largest error / bound is printed.

Every output (verts, joints, A_out, R_out, pose6d_out) sits between canary guards and is pre-filled with a sentinel pattern: after each call the guards
are intact and no sentinel is left inside.  The float64 reference is computed once per case on the CPU.

Shapes - the smallest that reach each path of the two skinning kernels (smpl_ref.cases()):
  V = 1     one lane, one vertex (a vertex tile with a single vertex; the 12-byte store at the last vertex of the buffer)
  V = 33    2 matrix-core tiles of 32 in one group of four waves: two surplus waves (`if (!live) return`), the second tile holds one vertex
  V = 129   5 tiles: a second group with three surplus waves
  V = 257   the VALU kernel's 256-vertex tile edge
  V = 1157  37 tiles -> 10 groups > 8 XCD slots: the second round of `(kk / b_tiles) * 8 + xcd`, 6 dead groups
  V = 2305  10 VALU tiles > 8 slots (`round_up(v_tiles, 8)`)
  B = 1, 16, 17, 23   the VALU path and its 16-body groups;   B = 24, 32, 33, 65   the matrix-core path: its minimum, tile edges, three tiles

Measured on an MI355X (largest error / bound per group; a figure above 1 would be a finding):
  forward matrix, 6 V x 8 B, N(0, 1) inputs      VALU: vertices 0.072, joints 0.080, extra joints 0.034, A 0.511;  matrix cores: 0.061, 0.098, 0.030, 0.635
  input families at V {33, 1157}, B {17, 33}     vertices, VALU / matrix cores: betas x 5  0.045 / 0.044, leaf rotations 0.036 / 0.045,
                                                 near-identity 1e-3  0.070 / 0.164, 1e-6  0.044 / 0.123, identity 0.012 / 0.052 (the same against v_shaped);
                                                 joints <= 0.071, A <= 0.587
  dense weights (24-joint loop), n_extra = 0     vertices 0.048, joints 0.132, A 0.696;  n_extra = 0: 0.027 (VALU), 0.033 (matrix cores)
  ehm_smpl_forward_rot6d                         pose6d_out bit-equal;  R_out 0.668 (V 33, B 7), 0.718 (V 129, B 33);  vertices 0.063, joints 0.107, A 0.606
  ehm_rot6d_to_rotmat, both modes                0.465 (n = 168), 0.607 (n = 792)
  bit-equal: A_out = NULL against given, the rot6d entry without its three optional outputs, a reused handle (B = 65, 24, 33, 7, 40) against fresh ones,
  every body beside a poisoned one; the poisoned body: all vertices NaN, under a NaN rotation of joint 9 its 12 descendants NaN, the other 12 joints unmoved.
The matrix-core figures equal tests/smpl_ref.py's emulation of the faithful order to the digits shown (near1e-6: 0.123 on both) - the subnormal lo halves of
the near-identity coefficients behave on the matrix cores as in numpy.  An engine without the coefficients' lo halves, the basis's lo halves or both cross
products is 15 to 79 times over the vertex bound on the `blend` cases (CPU emulation, tests/test_smpl_ref_cpu.py).  Nothing was found: no guard written,
no element left unwritten, no ratio above 1, every refusal EHM_EINVAL with its message.  88 tests, 4.5 s."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import smpl_ref as R
from tests.test_gpu_linear import SENTINEL
from tests.test_gpu_trunk_autograd import guarded, guards_intact

pytestmark = pytest.mark.gpu

SENTINEL32 = SENTINEL * 0x10001                 # two sentinel halves: the float32 1.5e16
CASES = R.cases()
EINVAL = -22


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _api():
    from egohmr_amd import _lib
    return _lib.api(), _lib


def new_model(asset, dev):
    from egohmr_amd.smpl import SMPL
    return SMPL(asset).to(dev)


@functools.lru_cache(maxsize=None)
def _model(V, seed, n_extra, weights):
    return new_model(R.cached_asset(V, seed, n_extra, weights), torch.device("cuda:0"))


class Out:
    """an output between guards, pre-filled with the sentinel"""

    def __init__(self, dev, *shape):
        self.full, self.t = guarded(dev, *shape)
        self.t.view(torch.int32).fill_(SENTINEL32)

    def check(self, name):
        assert guards_intact(self.full), f"{name}: a guard band was written"
        assert not bool((self.t.view(torch.int32) == SENTINEL32).any()), f"{name}: an element was not written"
        return self.t

    def numpy(self):
        return self.t.cpu().numpy()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def forward(model, dev, betas, rotmats, with_A=True):
    """ehm_smpl_forward on guarded outputs -> SimpleNamespace(vertices, joints, A) of device tensors (A None without A_out)"""
    A, L = _api()
    B, V, nj = betas.shape[0], model.num_verts, model.num_joints_out
    be = torch.as_tensor(betas).to(dev).contiguous()
    rot = torch.as_tensor(rotmats).to(dev).contiguous()
    v, j, a = Out(dev, B, V, 3), Out(dev, B, nj, 3), (Out(dev, B, 24, 3, 4) if with_A else None)
    A.ehm_smpl_forward(model.handle(), be, rot, v.t, j.t, a.t if with_A else None, B, L.stream_ptr())
    torch.cuda.synchronize()
    return SimpleNamespace(vertices=v.check("verts"), joints=j.check("joints"), A=a.check("A_out") if with_A else None)


def to_numpy(out):
    return SimpleNamespace(vertices=out.vertices.cpu().numpy(), joints=out.joints.cpu().numpy(), A=None if out.A is None else out.A.cpu().numpy())


def report(name, r):
    print(f"{name}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, (name, r)


# ------------------------------------------------------------------------------------------------ 1. forward against float64
FORWARD = [c for c in CASES if c.group in ("matrix", "family")]


@pytest.mark.parametrize("case", FORWARD, ids=[c.id for c in FORWARD])
def test_forward_against_float64(dev, case):
    asset, x = case.asset(), case.inputs()
    model = _model(case.V, case.asset_seed, case.n_extra, case.weights)
    path = R.path_of(asset, case.B)
    out = to_numpy(forward(model, dev, x.betas, x.rotmats))
    assert out.joints.shape == (case.B, 24 + case.n_extra, 3)
    bnd = (R.bound if path == "mfma" else R.bound_valu)(asset, x.betas, x.rotmats)
    report(f"{case.id} [{path}]", R.ratios(out, bnd))
    if case.family == "identity":           # the posed body IS the shaped body: vertices = v_shaped, joints = J, under the same bound
        ref = bnd.ref
        report(f"{case.id} [{path}] against v_shaped / J",
               {"vertices": R.ratio(out.vertices, ref.v_shaped.numpy(), bnd.vertices), "joints": R.ratio(out.joints[:, :24], ref.J.numpy(), bnd.joints)})


@pytest.mark.parametrize("B", (17, 33))
def test_forward_without_A_out_gives_the_same_bits(dev, B):
    case = next(c for c in CASES if c.group == "matrix" and c.V == 129 and c.B == B)
    x, model = case.inputs(), _model(case.V, case.asset_seed, case.n_extra, case.weights)
    with_A = forward(model, dev, x.betas, x.rotmats)
    without = forward(model, dev, x.betas, x.rotmats, with_A=False)
    assert same_bits(with_A.vertices, without.vertices) and same_bits(with_A.joints, without.joints)


# ------------------------------------------------------------------------------------------------ 2. dense weights, no extra joints
DENSE = [c for c in CASES if c.group == "dense"]


@pytest.mark.parametrize("case", DENSE, ids=[c.id for c in DENSE])
def test_dense_weights_and_no_extra_joints(dev, case):
    asset, x = case.asset(), case.inputs()
    model = _model(case.V, case.asset_seed, case.n_extra, case.weights)
    path = R.path_of(asset, case.B)
    assert path == "valu" or case.weights == "sparse"
    out = to_numpy(forward(model, dev, x.betas, x.rotmats))
    assert out.joints.shape == (case.B, 24 + case.n_extra, 3)
    report(f"{case.id} [{path}]", R.ratios(out, (R.bound if path == "mfma" else R.bound_valu)(asset, x.betas, x.rotmats)))


# ------------------------------------------------------------------------------------------------ 3. the rot6d entries
def forward_rot6d(model, dev, betas, x, mean, std, outputs=True):
    A, L = _api()
    B, V, nj = betas.shape[0], model.num_verts, model.num_joints_out
    t = lambda a: torch.as_tensor(a).to(dev).contiguous()
    v, j = Out(dev, B, V, 3), Out(dev, B, nj, 3)
    r, p, a = (Out(dev, B, 24, 3, 3), Out(dev, B, 144), Out(dev, B, 24, 3, 4)) if outputs else (None, None, None)
    A.ehm_smpl_forward_rot6d(model.handle(), t(betas), t(x), t(mean), t(std), v.t, j.t, r.t if outputs else None, p.t if outputs else None,
                             a.t if outputs else None, B, L.stream_ptr())
    torch.cuda.synchronize()
    out = SimpleNamespace(vertices=v.check("verts"), joints=j.check("joints"), A=None, R=None, pose6d=None)
    if outputs:
        out.A, out.R, out.pose6d = a.check("A_out"), r.check("R_out"), p.check("pose6d_out")
    return out


@pytest.mark.parametrize("V,B", ((33, 7), (129, 33)))
def test_forward_rot6d(dev, V, B):
    asset, model = R.cached_asset(V, 0, R.N_EXTRA, "sparse"), _model(V, 0, R.N_EXTRA, "sparse")
    x, mean, std = R.rot6d_inputs(B, 0)
    betas = R.inputs("normal", B, 6).betas
    ref6 = R.rot6d64(x, mean, std)
    out = forward_rot6d(model, dev, betas, x, mean, std)
    pose6d = out.pose6d.cpu().numpy()
    assert np.array_equal(pose6d.view(np.int32), ref6.pose6d.view(np.int32)), "pose6d_out is not the float32 x * std + mean rounded once"
    Rg = out.R.cpu().numpy().astype(np.float64)
    r_R = R.ratio(Rg, ref6.R, ref6.E_R)
    # the skinning under its own bound, at the rotations the device returned: Gram-Schmidt's conditioning stays out of it
    path = R.path_of(asset, B)
    bnd = (R.bound if path == "mfma" else R.bound_valu)(asset, betas, Rg)
    r = R.ratios(to_numpy(out), bnd)
    r["R_out"] = r_R
    report(f"rot6d V = {V}, B = {B} [{path}], conditioning {ref6.cond.max():.2f}", r)
    bare = forward_rot6d(model, dev, betas, x, mean, std, outputs=False)
    assert same_bits(out.vertices, bare.vertices) and same_bits(out.joints, bare.joints)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("B", (7, 33))
def test_rot6d_to_rotmat(dev, mode, B):
    A, L = _api()
    x, mean, std = R.rot6d_inputs(B, 0)
    p = R.rot6d64(x, mean, std).pose6d.reshape(B * 24, 6)                # well-conditioned 6-vectors in the 'diffusion' layout ...
    x6 = p.astype(np.float64).reshape(-1, 3, 2)
    a1, a2 = x6[..., 0], x6[..., 1]
    feed = p if mode == 1 else np.concatenate([a1, a2], 1).astype(np.float32)          # ... and the same vectors in the 'prohmr' layout
    ref, E, cond = R.gram_schmidt64(a1, a2)
    out = Out(dev, B * 24, 3, 3)
    A.ehm_rot6d_to_rotmat(torch.from_numpy(np.ascontiguousarray(feed)).to(dev), out.t, B * 24, mode, L.stream_ptr())
    torch.cuda.synchronize()
    report(f"ehm_rot6d_to_rotmat mode {mode}, n = {B * 24}, conditioning {cond.max():.2f}", {"R": R.ratio(out.check("R").cpu().numpy(), ref, E)})
    assert A.ehm_rot6d_to_rotmat(None, None, 0, mode, L.stream_ptr()) == 0          # an empty batch: nothing to do, null pointers allowed


# ------------------------------------------------------------------------------------------------ 4. handle reuse
def test_handle_reuse_across_batch_sizes(dev):
    """pf_cap and ws_cap only grow: a smaller later batch reads buffers that hold an earlier, larger batch's fragments and transforms"""
    asset = R.cached_asset(129, 0, R.N_EXTRA, "sparse")
    used = new_model(asset, dev)
    for B in (65, 24, 33, 7, 40):
        x = R.inputs("normal", B, 7)
        got = forward(used, dev, x.betas, x.rotmats, with_A=False)
        fresh = new_model(asset, dev)
        want = forward(fresh, dev, x.betas, x.rotmats, with_A=False)
        assert same_bits(got.vertices, want.vertices) and same_bits(got.joints, want.joints), B
        fresh.handle().close()
    used.handle().close()


# ------------------------------------------------------------------------------------------------ 5. non-finite containment
def _ancestors(j):
    out = []
    while R.PARENTS[j] >= 0:
        j = R.PARENTS[j]
        out.append(j)
    return out


DESCENDANTS_OF_9 = [j for j in range(24) if 9 in _ancestors(j)]


@pytest.mark.parametrize("B,body", ((40, 13), (20, 9)))           # the middle of a 32-body matrix-core tile / of a 16-body VALU group
@pytest.mark.parametrize("what", ("beta", "rotation"))
def test_one_poisoned_body_stays_alone(dev, B, body, what):
    """input data only: a NaN in one beta, or in one rotation entry of the mid-chain joint 9, of ONE body"""
    assert DESCENDANTS_OF_9 == [12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23]
    model = _model(129, 0, R.N_EXTRA, "sparse")
    x = R.inputs("normal", B, 8)
    clean = forward(model, dev, x.betas, x.rotmats)
    betas, rot = x.betas.copy(), x.rotmats.copy()
    if what == "beta":
        betas[body, 3] = np.nan
    else:
        rot[body, 9, 1, 2] = np.nan
    bad = forward(model, dev, betas, rot)
    others = [b for b in range(B) if b != body]
    for name in ("vertices", "joints", "A"):
        assert same_bits(getattr(bad, name)[others], getattr(clean, name)[others]), name
    assert bool(torch.isnan(bad.vertices[body]).all()), "a vertex of the poisoned body is not NaN"
    assert bool(torch.isnan(bad.joints[body, 24:]).all())                      # (the extra joints are vertices)
    if what == "rotation":
        keep = [j for j in range(24) if j not in DESCENDANTS_OF_9]
        assert same_bits(bad.joints[body, keep], clean.joints[body, keep]), "a joint above or beside joint 9 moved"
        assert bool(torch.isnan(bad.joints[body, DESCENDANTS_OF_9]).all()), "a descendant of joint 9 is not NaN"
    else:
        assert bool(torch.isnan(bad.joints[body, :24]).all())                  # every rest joint is regressed from the betas


# ------------------------------------------------------------------------------------------------ 6. refusals
def _create(dev, asset, parents=None, extra=None, n_extra=None):
    A, L = _api()
    t = lambda k: torch.as_tensor(np.asarray(asset[k], np.float32)).to(dev).contiguous()
    bufs = [t("v_template"), t("shapedirs"), t("posedirs"), t("J_regressor"), t("lbs_weights")]
    par = ([-1] + R.PARENTS[1:]) if parents is None else parents
    ext = [int(i) for i in (asset["extra_joints_idxs"] if extra is None else extra)]
    n_extra = len(ext) if n_extra is None else n_extra
    h = C.c_void_p()
    A.ehm_smpl_create(C.byref(h), *bufs, (C.c_int32 * 24)(*par), (C.c_int32 * max(len(ext), 1))(*ext), asset["v_template"].shape[0], n_extra,
                      L.stream_ptr())
    return L.Handle(h, A.ehm_smpl_destroy, keep=bufs)


def test_create_and_forward_refuse_bad_arguments(dev):
    A, L = _api()
    V = 33
    asset = R.cached_asset(V, 0, R.N_EXTRA, "sparse")
    good = [-1] + R.PARENTS[1:]
    bad_parent, bad_root = list(good), list(good)
    bad_parent[5], bad_root[0] = 7, 0
    refusals = (
        (dict(parents=bad_parent), "parents[5]=7 must satisfy 0 <= parent < child"),
        (dict(parents=bad_root), "bad argument: parents[0] < 0"),
        (dict(extra=[0] * 65), "n_extra <= 64"),
        (dict(extra=[0, V, 1]), "setup failed (rc=-22)"),
    )
    for kw, message in refusals:
        with pytest.raises(L.EgoHMRHipError) as e:
            _create(dev, asset, **kw)
        assert e.value.rc == EINVAL and "ehm_smpl_create" in str(e.value) and message in str(e.value), str(e.value)
    # the process is still usable: a valid create and a forward under the bound
    h = _create(dev, asset)
    x = R.inputs("normal", 5, 9)
    be, rot = torch.from_numpy(x.betas).to(dev), torch.from_numpy(x.rotmats).to(dev)
    v, j = Out(dev, 5, V, 3), Out(dev, 5, 24 + R.N_EXTRA, 3)
    with pytest.raises(L.EgoHMRHipError) as e:
        A.ehm_smpl_forward(h, be, rot, v.t, j.t, None, 0, L.stream_ptr())
    assert e.value.rc == EINVAL and "B > 0" in str(e.value)
    torch.cuda.synchronize()
    assert guards_intact(v.full) and bool((v.t.view(torch.int32) == SENTINEL32).all())          # a refused call writes nothing
    A.ehm_smpl_forward(h, be, rot, v.t, j.t, None, 5, L.stream_ptr())
    torch.cuda.synchronize()
    out = SimpleNamespace(vertices=v.check("verts").cpu().numpy(), joints=j.check("joints").cpu().numpy(), A=None)
    report("after the refusals, V = 33, B = 5 [valu]", R.ratios(out, R.bound_valu(asset, x.betas, x.rotmats)))
    h.close()
