"""Host-side reference, error bound and emulation of the SMPL forward entries (ehm_smpl_forward, ehm_smpl_forward_rot6d, ehm_rot6d_to_rotmat;
csrc/smpl.hip, csrc/step_dev.h: pose_chain_body, csrc/smpl_dev.h: rot6d_to_R), for tests/test_smpl_ref_cpu.py and tests/test_gpu_smpl_forward.py
(numpy / torch float64, no GPU, no native library):

  make_asset    a small SMPL-shaped body for any V >= 1 (sub-sampled rows of synthetic.make_smpl_asset, own regressor, weights, extra ids)
  inputs        betas / rotation matrices of an input family (and the 6-D vectors they came from, for the conditioning check)
  forward64     oracle.smpl.SMPLOracle in float64 - the one reference
  rot6d64       the de-normalised 6-vector as the kernel forms it (one float32 rounding) and float64 Gram-Schmidt with its bound
  bound / bound_valu   per-element first-order error bounds of A, the 24 posed joints, the vertices and the extra joints
  emulate       the device's order of operations in numpy float32 / float16, both skinning paths, with the broken split variants
  cases         the one list of cases both test files iterate

Error model.  u = 2^-24 (half an ulp of float32).  The inputs (asset, betas, rotation matrices) are float32 and enter the float64 reference
exactly, so no representation error of an input is in the bound.  Every constant below is a count of float32 roundings that a term passes
through in the source line named next to it; magnitudes are those of the float64 reference (first order: products of two errors are dropped).
A compiler that contracts a product and an add into one fma only removes roundings.

Joints (smpl.hip joint_basis_kernel, step_dev.h pose_chain_body):
  * J_template[j][c] and J_shape[j][c][l] are sums over the V vertices: thread t of 256 runs `s = fmaf(Jr, x, s)` over v = t, t + 256, ... -
    n_v = ceil(V / 256) roundings - and `red[t] += red[t + o]` for o = 128 ... 1 adds 8 more:  E_Jt = (n_v + 8) u sum_v |Jr||v_template|, E_Js alike.
  * `s = fmaf(J_shape, beta, s)` ten times, then `J_template + s`:  E_J = E_Jt + sum_l (E_Js + 10 u |J_shape|) |beta_l| + u |J|.
  * `Jx[c] - pj` (rel_joints):  E_t = E_J(child) + E_J(parent) + u |t|;  the root keeps E_J.
Chain (pose_chain_body, level by level; the rotations R are inputs, E_R = 0):
  * `p0 * R[0] + p1 * R[3] + p2 * R[6]`: the first product is rounded, then two adds - 3 roundings:
        E_Grot(child) = E_Grot(parent) |R| + 3 u |Grot(parent)| |R|
  * `p0 * t[0] + p1 * t[1] + p2 * t[2] + p3`: 4 roundings:
        E_Gt(child) = E_Grot(parent) |t| + |Grot(parent)| E_t + E_Gt(parent) + 4 u (|Grot(parent)| |t| + |Gt(parent)|)
    (the issue's E_G(child) = E_G(parent) |T| + |G_parent| E_T + k u |G_parent||T| with k = 3 for the rotation block, 4 for the translation).
    The posed joints are Gt.
  * `gj = G[r][0] * Jx[0] + G[r][1] * Jx[1] + G[r][2] * Jx[2]` (3 roundings) and `G[r][3] - gj` (1):
        E_At = E_Gt + E_Grot |J| + |Grot| E_J + 3 u |Grot| |J| + u |At|;   E_Arot = E_Grot.
Blend on the matrix cores (pf_pack_kernel, pd_pack_kernel, skin_mfma_body), p = v_template + (1 / s) sum_k c_k (s D_k), c = [R[1:] - I | betas],
D = [posedirs; shapedirs], s = pd_scale (a power of two: it adds no rounding):
  * `Rws[...] - 1.f` in float32: 1 u |c| (exact between 0.5 and 2 - counted anyway).
  * split of a coefficient, `hi = (_Float16)x; lo = (_Float16)(x - (float)hi)`: x - hi is exact, |x - hi| <= 2^-11 |x|, and lo is rounded once:
    |x - hi - lo| <= 2^-22 |x| = 4 u |x| while lo is a normal f16 - and <= 2^-25 (half the f16 subnormal spacing) when it is not.  The coefficients are not
    scaled, so every |c_k| below about 2^-3 has a subnormal lo: the floor 2^-25 sum_k |D_k|.  The basis IS scaled (1024 <= s max|D| < 2048), its lo halves
    are normal down to 2^-14 of the largest entry:  4 u |D_k|, with the floor (2^-25 / s) sum_k |c_k| for the entries below that.
  * the product c_lo . D_lo is left out (three MFMAs per product, not four): |c_lo||D_lo| <= 2^-11 |c| 2^-11 |D| = 4 u |c||D|.
  * accumulation - the f16-MFMA model of tests/conv_x2_ref.py: the products of f16 halves are exact in float32 and the matrix cores add the 16 of
    one instruction into the float32 accumulator with at most one rounding per instruction.  14 k-steps x 3 chained instructions per accumulator =
    42 roundings of partial sums, each at most sum_k |c_k||D_k| in magnitude (worst case, no random-walk argument).
        k_blend = 1 + 4 + 4 + 4 + 42 = 55
  * `fmaf(acc[c][r], inv, t0)`: acc / s is exact, one rounding of the sum: u |p|.
        E_p = 55 u sum_k |c_k||D_k| + 2^-25 sum_k |D_k| + (2^-25 / s) sum_k |c_k| + u |p|
Blend on the VALU (skin_kernel; bound_valu): `po = fmaf(be, s0, po)` ten times from zero, `po += t0`, then `po = fmaf(f, d0, po)` 207 times - every term
passes at most 218 roundings of partial sums no larger than |v_template| + sum_k |c_k||D_k|, and `Rws[...] - 1` adds 1 u |c| as above:
        E_p = 218 u (|v_template| + sum_k |c_k||D_k|) + u sum_k |c_k||D_k|
Weighted transform: `T2[e] = wj * q[e]` then three `fma(wj, q[e], T2[e])` (matrix-core path), four `fmaf(wj, r0[e], T[e])` from zero (VALU, sparse):
k_w = 4 roundings;  24 for an asset with more than four weights per vertex (`for (int j = 0; j < kJ; ++j)`):
        E_T = sum_j w_j E_A(j) + k_w u sum_j w_j |A(j)|
Apply, `T[0] * px + T[1] * py + T[2] * pz + T[3]`: 4 roundings:
        E_v = sum_c (E_T[r][c] |p_c| + |T[r][c]| E_p[c]) + E_T[r][3] + 4 u (sum_c |T[r][c]||p_c| + |T[r][3]|)
An extra joint is a copy of its vertex and takes its bound.

rot6d (rot6d_to_R: every product, sum, quotient and root rounded separately; the input 6-vector is the float32 the kernel formed, so it is exact):
  n1 = sqrt(x^2 + y^2 + z^2): 3 roundings under the root, the root halves them and adds one - 2.5 u; b1 = a1 / n1: E_b1 = 3.5 u |b1|
  d = b1 . a2:  E_d = sum E_b1 |a2| + 3 u sum |b1||a2|;   w = a2 - d b1:  E_w = E_d |b1| + |d| E_b1 + u |d b1| + u |w|
  n2 = |w|:  E_n2 = sum |w| E_w / n2 + 2.5 u n2;   b2 = w / n2:  E_b2 = E_w / n2 + |b2| E_n2 / n2 + u |b2|
  b3 = b1 x b2:  E_b3x = E_b1y |b2z| + |b1y| E_b2z + E_b1z |b2y| + |b1z| E_b2y + 2 u (|b1y b2z| + |b1z b2y|), cyclic.
The division by n2 is where the conditioning |a2| / |a2 - (b1 . a2) b1| enters (E_w is of the order u |a2|); 1 / |a1| enters where an ABSOLUTE
error of the 6-vector is carried in (a caller's tolerance on pose6d).  `conditioning` returns max(1 / |a1|, |a2| / |w|); every input family
keeps it <= 4 (tests/test_smpl_ref_cpu.py).

What the bound can tell apart (tests/test_smpl_ref_cpu.py, figures in docs/EXPERIMENTS.md R33.1): an engine that drops c_lo or D_lo is off by about
2^-12 of a term, 55 u is 2^-18.2 of the sum of |terms| - with few dominant terms (large betas, rotations on leaf joints only, near-identity
poses, where the ten shape terms carry the blend) such an engine misses the bound several times over on some vertex."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from egohmr_amd import synthetic as syn
from oracle.smpl import SMPLOracle

U = 2.0 ** -24
F16_FLOOR = 2.0 ** -25               # half the spacing of the f16 subnormals
KJ, POSE_BASIS, BLEND_K, BLEND_STEPS = 24, 207, 224, 14
K_BLEND = 1 + 4 + 4 + 4 + 3 * BLEND_STEPS
K_VALU = 10 + 1 + POSE_BASIS
MFMA_MIN_BODIES = 24                 # kSkinMfmaMinBodies
BODY_GROUP, VALU_TILE, MFMA_TILE = 16, 256, 32        # kBGF, kVT, vertices per wave of skin_mfma_body
LEAF_JOINTS = (10, 11, 15, 22, 23)   # joints of SMPL_PARENTS without a child
PARENTS = [int(p) for p in syn.SMPL_PARENTS]


def _rng(*key):
    return np.random.Generator(np.random.PCG64([abs(hash_int(k)) for k in key]))


def hash_int(k):
    """a stable integer of a str / int key (python's hash() of a str changes between processes)"""
    if isinstance(k, (int, np.integer)):
        return int(k)
    return int.from_bytes(str(k).encode(), "little") % (2 ** 61 - 1)


# ------------------------------------------------------------------------------------------------ assets
@functools.lru_cache(maxsize=4)
def _base(seed):
    return syn.make_smpl_asset(seed)


def sparse_slots(lbs_weights):
    """ehm_smpl_create's compressed copy: (w_idx [4, V], w_val [4, V]) - the non-zeros of a row in ascending joint order, padding slots
    "joint 0, weight 0" - or None when some row has more than four."""
    W = np.asarray(lbs_weights, np.float32)
    V = W.shape[0]
    idx, val = np.zeros((4, V), np.int64), np.zeros((4, V), np.float32)
    for v in range(V):
        nz = np.flatnonzero(W[v])
        if len(nz) > 4:
            return None
        idx[:len(nz), v], val[:len(nz), v] = nz, W[v, nz]
    return idx, val


def make_asset(V, seed, n_extra, weights="sparse"):
    """A small SMPL-shaped asset (float32 arrays, int64 ids; deterministic): rows of synthetic.make_smpl_asset(seed) sub-sampled for v_template,
    shapedirs and posedirs; J_regressor rows convex over up to 8 of the V vertices; parents = SMPL_PARENTS; a few faces (egohmr_amd.smpl.SMPL asks for
    them).  extra_joints_idxs has n_extra ids: vertex V - 1 first, vertex 0, vertex V - 1 AGAIN, then random ones.
    weights = "sparse": row v has 1 + v % 4 non-zeros, except the first four rows:
        row 0: joint 23 alone;  row 1: joints 0 and 23;  row 2: joint 0 alone;  row 3: joints 0, 5 and 23
    (V >= 8 gives rows with exactly 1, 2, 3 and 4 non-zeros).  ehm_smpl_create fills the slots in ascending joint order, so a non-zero on joint 0 always
    sits in the FIRST slot; what rows 1 and 3 give is joint 0 as a live slot and as the "joint 0, weight 0" padding slots of the same row.
    weights = "dense": as sparse, but every third row (v % 3 == 0, from row 6 on) has 6 non-zeros: the VALU kernel's 24-joint loop at every B."""
    assert V >= 1 and 0 <= n_extra <= 64 and weights in ("sparse", "dense")
    base = _base(seed)
    g = _rng("asset", V, seed, n_extra, weights)
    rows = np.sort(g.choice(syn.NUM_VERTS, size=V, replace=False))
    posedirs = base["posedirs"].reshape(POSE_BASIS, syn.NUM_VERTS, 3)[:, rows].reshape(POSE_BASIS, V * 3)
    Jr = np.zeros((KJ, V))
    for j in range(KJ):
        pick = g.choice(V, size=min(V, 8), replace=False)
        w = g.random(len(pick)) + 0.1
        Jr[j, pick] = w / w.sum()
    W = np.zeros((V, KJ))
    fixed = {0: [23], 1: [0, 23], 2: [0], 3: [0, 5, 23]}
    for v in range(V):
        if v in fixed:
            js = fixed[v]
        else:
            n = 6 if (weights == "dense" and v % 3 == 0 and v >= 6) else 1 + v % 4
            js = g.choice(KJ, size=n, replace=False)
        w = g.random(len(js)) + 0.05
        W[v, js] = w / w.sum()
    extra = np.array(([V - 1, 0, V - 1] + [int(i) for i in g.integers(0, V, size=max(n_extra - 3, 0))])[:n_extra], dtype=np.int64)
    return {
        "v_template": np.ascontiguousarray(base["v_template"][rows]),
        "shapedirs": np.ascontiguousarray(base["shapedirs"][rows]),
        "posedirs": np.ascontiguousarray(posedirs),
        "J_regressor": Jr.astype(np.float32),
        "lbs_weights": W.astype(np.float32),
        "parents": syn.SMPL_PARENTS.copy(),
        "faces": g.integers(0, V, size=(4, 3)).astype(np.int64),
        "extra_joints_idxs": extra,
    }


def pd_scale(asset):
    """ehm_smpl_create: the power of two s with 1024 <= s max|D| < 2048 (frexpf(2048 / amax))"""
    amax = np.float32(max(np.abs(asset["posedirs"]).max(), np.abs(asset["shapedirs"]).max()))
    if not (0 < amax < 1e30):
        return 1.0
    _, e = np.frexp(np.float32(2048.0) / amax)
    return float(np.ldexp(1.0, int(e) - 1))


# ------------------------------------------------------------------------------------------------ rot6d
def gram_schmidt64(a1, a2):
    """float64 [..., 3] x 2 -> (R [..., 3, 3] with columns b1, b2, b3, its bound E_R, the conditioning factor [...]) - utils/geometry.py:61-66 and
    the rot6d part of the module docstring"""
    a1, a2 = np.asarray(a1, np.float64), np.asarray(a2, np.float64)
    dot = lambda x, y: (x * y).sum(-1, keepdims=True)
    n1 = np.sqrt(dot(a1, a1))
    b1 = a1 / n1
    d = dot(b1, a2)
    w = a2 - d * b1
    n2 = np.sqrt(dot(w, w))
    b2 = w / n2
    b3 = np.cross(b1, b2)
    assert n1.min() > 1e-6 and n2.min() > 1e-6                    # (far from F.normalize's 1e-12 clamp)
    E1 = 3.5 * U * np.abs(b1)
    Ed = dot(E1, np.abs(a2)) + 3 * U * dot(np.abs(b1), np.abs(a2))
    Ew = Ed * np.abs(b1) + np.abs(d) * E1 + U * np.abs(d * b1) + U * np.abs(w)
    En2 = dot(np.abs(w), Ew) / n2 + 2.5 * U * n2
    E2 = Ew / n2 + np.abs(b2) * En2 / n2 + U * np.abs(b2)
    r1, r2 = lambda x: np.roll(x, -1, -1), lambda x: np.roll(x, -2, -1)         # b3 = r1(b1) r2(b2) - r2(b1) r1(b2)
    ab1, ab2 = np.abs(b1), np.abs(b2)
    E3 = (r1(E1) * r2(ab2) + r1(ab1) * r2(E2) + r2(E1) * r1(ab2) + r2(ab1) * r1(E2) + 2 * U * (r1(ab1) * r2(ab2) + r2(ab1) * r1(ab2)))
    cond = np.maximum(1.0 / n1, np.sqrt(dot(a2, a2)) / n2)[..., 0]
    return np.stack([b1, b2, b3], -1), np.stack([E1, E2, E3], -1), cond


def conditioning(x6):
    """max(1 / |a1|, |a2| / |a2 - (b1 . a2) b1|) of 6-vectors [..., 3, 2] in the 'diffusion' layout (a1 = x[0::2], a2 = x[1::2])"""
    return gram_schmidt64(x6[..., 0], x6[..., 1])[2]


def round_once(x, std, mean):
    """float32 arrays -> x * std + mean rounded ONCE to float32 (the fma the kernel's `rot_or_x[e] * std_[e] + mean[e]` contracts to).  The product is exact
    in float64; the float64 sum is rounded, so its error (TwoSum) decides the rare case in which that sum lands on a float32 tie."""
    prod = x.astype(np.float64) * std.astype(np.float64)
    m = np.broadcast_to(mean.astype(np.float64), prod.shape)
    s = prod + m
    bb = s - prod
    err = (prod - (s - bb)) + (m - bb)
    r = s.astype(np.float32)
    dlt = s - r.astype(np.float64)
    other = np.nextafter(r, np.where(dlt > 0, np.inf, -np.inf).astype(np.float32))
    half = (other.astype(np.float64) - r.astype(np.float64)) / 2
    flip = (dlt != 0) & (dlt == half) & (np.sign(err) == np.sign(dlt))
    return np.where(flip, other, r).astype(np.float32)


def rot6d64(x, mean, std):
    """x [B, 144], mean / std [144] float32 -> SimpleNamespace(pose6d float32 [B, 144]: what pose6d_out must hold bit for bit; R float64 [B, 24, 3, 3];
    E_R its bound; cond [B, 24])"""
    p = round_once(np.asarray(x, np.float32), np.asarray(std, np.float32), np.asarray(mean, np.float32))
    x6 = p.astype(np.float64).reshape(-1, KJ, 3, 2)
    R, E, cond = gram_schmidt64(x6[..., 0], x6[..., 1])
    return SimpleNamespace(pose6d=p, R=R, E_R=E, cond=cond)


def rot6d_inputs(B, seed):
    """(x [B, 144], mean [144], std [144]) float32 with a non-trivial mean and std: the de-normalised vectors are the identity's 6-D form plus
    noise of 0.1 (mean) and about 0.1 (x * std, x clipped at three standard deviations)"""
    g = _rng("rot6d", B, seed)
    ident = np.tile(np.array([1, 0, 0, 1, 0, 0], np.float64), KJ)           # (a1, a2) interleaved: a1 = e1, a2 = e2
    mean = (ident + 0.1 * g.normal(size=144)).astype(np.float32)
    std = (0.05 + 0.1 * g.random(144)).astype(np.float32)
    x = np.clip(g.normal(size=(B, 144)), -3.0, 3.0).astype(np.float32)
    return x, mean, std


# ------------------------------------------------------------------------------------------------ input families
FAMILIES = ("normal", "betas5", "leaf", "near1e-3", "near1e-6", "identity")


def _well_conditioned(g, shape):
    """N(0, 1) 6-vectors [*shape, 3, 2], those with a conditioning factor above 4 drawn again"""
    x6 = g.normal(size=shape + (3, 2))
    for _ in range(64):
        bad = conditioning(x6) > 4.0
        if not bad.any():
            return x6
        x6[bad] = g.normal(size=(int(bad.sum()), 3, 2))
    raise AssertionError("no well-conditioned draw")


def inputs(family, B, seed):
    """SimpleNamespace(betas float32 [B, 10], rotmats float32 [B, 24, 3, 3], x6 float64 [B, 24, 3, 2]: the 6-vectors the rotations came from)
      normal     N(0, 1) 6-vectors on every joint, betas N(0, 1)
      betas5     the same with betas x 5
      leaf       identity everywhere but the five leaf joints (N(0, 1) there), betas N(0, 1): the chain above them stays exact
      near1e-3   identity 6-vectors + 1e-3 N(0, 1), betas N(0, 1);   near1e-6 alike: every |R - I| entry has a subnormal (or zero) f16 lo half
      identity   the exact identity pose, betas N(0, 1)"""
    assert family in FAMILIES
    g = _rng("inputs", family, B, seed)
    ident = np.zeros((B, KJ, 3, 2))
    ident[..., 0, 0] = 1.0
    ident[..., 1, 1] = 1.0
    betas = g.normal(size=(B, 10))
    if family in ("normal", "betas5"):
        x6 = _well_conditioned(g, (B, KJ))
        if family == "betas5":
            betas = betas * 5.0
    elif family == "leaf":
        x6 = ident.copy()
        x6[:, list(LEAF_JOINTS)] = _well_conditioned(g, (B, len(LEAF_JOINTS)))
    elif family.startswith("near"):
        x6 = ident + float(family[4:]) * g.normal(size=ident.shape)
    else:
        x6 = ident
    R = gram_schmidt64(x6[..., 0], x6[..., 1])[0]
    return SimpleNamespace(betas=betas.astype(np.float32), rotmats=R.astype(np.float32), x6=x6)


# ------------------------------------------------------------------------------------------------ reference and bound
def forward64(asset, betas, rotmats):
    """oracle.smpl.SMPLOracle(asset, dtype=torch.float64) on float32 / float64 inputs: .vertices, .joints [B, 24 + n_extra, 3], .A, .J, .v_shaped"""
    rot = torch.as_tensor(np.asarray(rotmats, np.float64)).reshape(-1, KJ, 3, 3)
    be = torch.as_tensor(np.asarray(betas, np.float64))
    return SMPLOracle(asset, dtype=torch.float64)(be, rot[:, 1:], rot[:, :1])


def blend_operands(asset, betas, rotmats):
    """float64: c [B, 217] = [R[1:] - I | betas], D [217, V * 3] = [posedirs; shapedirs]"""
    R = np.asarray(rotmats, np.float64).reshape(-1, KJ, 3, 3)
    V = asset["v_template"].shape[0]
    c = np.concatenate([(R[:, 1:] - np.eye(3)).reshape(-1, POSE_BASIS), np.asarray(betas, np.float64)], 1)
    D = np.concatenate([np.asarray(asset["posedirs"], np.float64), np.asarray(asset["shapedirs"], np.float64).reshape(V * 3, 10).T], 0)
    return c, D


def _bound(asset, betas, rotmats, valu, ref=None, E_R=None):
    ref = forward64(asset, betas, rotmats) if ref is None else ref
    f64 = lambda k: np.asarray(asset[k], np.float64)
    vt, sd, Jr, W = f64("v_template"), f64("shapedirs"), f64("J_regressor"), f64("lbs_weights")
    V = vt.shape[0]
    be = np.asarray(betas, np.float64)
    R = np.asarray(rotmats, np.float64).reshape(-1, KJ, 3, 3)
    B = R.shape[0]
    J, A = ref.J.numpy(), ref.A.numpy()
    Grot, Gt = A[..., :3], ref.joints[:, :KJ].numpy()
    par = PARENTS
    # joints
    n_jb = math.ceil(V / 256) + 8
    E_Jt = n_jb * U * (np.abs(Jr) @ np.abs(vt))                                                     # [24, 3]
    Js = np.einsum("jv,vcl->jcl", Jr, sd)
    E_Js = n_jb * U * np.einsum("jv,vcl->jcl", np.abs(Jr), np.abs(sd))
    E_J = E_Jt[None] + np.einsum("jcl,bl->bjc", E_Js + 10 * U * np.abs(Js), np.abs(be)) + U * np.abs(J)
    t = J.copy()
    t[:, 1:] -= J[:, par[1:]]
    E_t = E_J.copy()
    E_t[:, 1:] = E_J[:, 1:] + E_J[:, par[1:]] + U * np.abs(t[:, 1:])
    # chain
    E_Grot, E_Gt = np.zeros((B, KJ, 3, 3)), np.zeros((B, KJ, 3))
    E_Gt[:, 0] = E_t[:, 0]
    E_R = np.zeros((B, KJ, 3, 3)) if E_R is None else np.asarray(E_R, np.float64)      # (rotations that the device formed itself: bound_valu's E_R)
    E_Grot[:, 0] = E_R[:, 0]
    mv = lambda M, v: np.einsum("brc,bc->br", M, v)
    for j in range(1, KJ):
        p = par[j]
        aP, aR, at = np.abs(Grot[:, p]), np.abs(R[:, j]), np.abs(t[:, j])
        E_Grot[:, j] = E_Grot[:, p] @ aR + aP @ E_R[:, j] + 3 * U * (aP @ aR)
        E_Gt[:, j] = mv(E_Grot[:, p], at) + mv(aP, E_t[:, j]) + E_Gt[:, p] + 4 * U * (mv(aP, at) + np.abs(Gt[:, p]))
    E_A = np.zeros((B, KJ, 3, 4))
    E_A[..., :3] = E_Grot
    aG, aJ = np.abs(Grot), np.abs(J)
    E_A[..., 3] = (E_Gt + np.einsum("bjrc,bjc->bjr", E_Grot, aJ) + np.einsum("bjrc,bjc->bjr", aG, E_J)
                   + 3 * U * np.einsum("bjrc,bjc->bjr", aG, aJ) + U * np.abs(A[..., 3]))
    # blend
    c, D = blend_operands(asset, betas, R)
    S = (np.abs(c) @ np.abs(D)).reshape(B, V, 3)
    p = vt[None] + (c @ D).reshape(B, V, 3)
    if valu:
        E_p = K_VALU * U * (np.abs(vt)[None] + S) + U * S + (E_R[:, 1:].reshape(B, POSE_BASIS) @ np.abs(D[:POSE_BASIS])).reshape(B, V, 3)
    else:
        assert not E_R.any(), "a rotation error is carried through the VALU blend only"
        s = pd_scale(asset)
        E_p = (K_BLEND * U * S + F16_FLOOR * np.abs(D).sum(0).reshape(1, V, 3) + (F16_FLOOR / s) * np.abs(c).sum(1)[:, None, None] + U * np.abs(p))
    # weighted transform and apply
    k_w = 4 if (sparse_slots(asset["lbs_weights"]) is not None) else KJ
    assert valu or k_w == 4, "the matrix-core path needs <= 4 weights per vertex"
    T = np.einsum("vj,bje->bve", W, A.reshape(B, KJ, 12)).reshape(B, V, 3, 4)
    E_T = (np.einsum("vj,bje->bve", W, E_A.reshape(B, KJ, 12)) + k_w * U * np.einsum("vj,bje->bve", W, np.abs(A).reshape(B, KJ, 12))).reshape(B, V, 3, 4)
    ap = np.abs(p)
    E_v = (np.einsum("bvrc,bvc->bvr", E_T[..., :3], ap) + np.einsum("bvrc,bvc->bvr", np.abs(T[..., :3]), E_p) + E_T[..., 3]
           + 4 * U * (np.einsum("bvrc,bvc->bvr", np.abs(T[..., :3]), ap) + np.abs(T[..., 3])))
    extra = E_v[:, np.asarray(asset["extra_joints_idxs"], np.int64)]
    return SimpleNamespace(A=E_A, joints=E_Gt, vertices=E_v, extra=extra, all_joints=np.concatenate([E_Gt, extra], 1), ref=ref,
                           p=E_p, J=E_J, t=E_t, J_shape=E_Js, rest=SimpleNamespace(p=p, J=J, t=t, J_shape=Js))


def bound(asset, betas, rotmats, ref=None):
    """Per-element bounds of the matrix-core path (B >= 24, <= 4 weights per vertex): .A [B, 24, 3, 4], .joints [B, 24, 3], .vertices [B, V, 3],
    .extra [B, n_extra, 3], .all_joints [B, 24 + n_extra, 3]; .ref = the float64 reference they were taken at"""
    return _bound(asset, betas, rotmats, False, ref)


def bound_valu(asset, betas, rotmats, ref=None, E_R=None):
    """The same for the VALU skinning kernel (B < 24, or an asset with more than four weights in a row).  Beside the outputs' bounds: .p, .J, .t, .J_shape -
    the bounds of the blended rest vertex, the rest joints, the joint offsets and the regressed shape basis (tests/smpl_vjp_ref.py: the backward recomputes
    them) - and .rest, their float64 values.  E_R [B, 24, 3, 3]: an error bound of the rotations themselves, for an entry that forms them on the device
    (first order: `aP @ E_R` in the chain, `E_R |posedirs|` in the blend); None = the rotations are exact inputs."""
    return _bound(asset, betas, rotmats, True, ref, E_R)


def path_of(asset, B):
    return "mfma" if (B >= MFMA_MIN_BODIES and sparse_slots(asset["lbs_weights"]) is not None) else "valu"


def ratio(got, ref, bnd):
    """Largest |got - ref| / bound; a non-finite `got` gives inf, an empty array 0"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - ref)
        e = np.where(d == 0, 0.0, d / bnd)                    # (a zero bound - an exact element, such as the root's rotation block - admits no error)
    e = np.where(np.isfinite(got), e, np.inf)
    return float(e.max())


def ratios(out, bnd):
    """{group: largest error / bound} of an output (.A, .joints [B, 24 + n_extra, 3], .vertices; .A may be None) against bnd.ref"""
    ref = bnd.ref
    r = {"vertices": ratio(out.vertices, ref.vertices.numpy(), bnd.vertices),
         "joints": ratio(out.joints[:, :KJ], ref.joints[:, :KJ].numpy(), bnd.joints),
         "extra": ratio(out.joints[:, KJ:], ref.joints[:, KJ:].numpy(), bnd.extra)}
    if getattr(out, "A", None) is not None:
        r["A"] = ratio(out.A, ref.A.numpy(), bnd.A)
    return r


# ------------------------------------------------------------------------------------------------ the device's order of operations
def _fma(a, b, c):
    """float32 fma (the float64 product of two float32 is exact; the double rounding of the sum does not matter to an emulation)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def split16(x):
    """float32 -> (hi, lo) float16 as pd_pack_kernel / pf_pack_kernel split a value"""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    return hi, (x - hi.astype(np.float32)).astype(np.float16)


def _dot3(P, M):
    """[B, 3, 3] x [B, 3, k] float32 in the kernel's order: p0 * m0 rounded, then two fmas"""
    acc = (P[:, :, 0, None] * M[:, None, 0, :]).astype(np.float32)
    acc = _fma(P[:, :, 1, None], M[:, None, 1, :], acc)
    return _fma(P[:, :, 2, None], M[:, None, 2, :], acc)


def emulate(asset, betas, rotmats, path, drop=None):
    """The forward in numpy float32 / float16 in the device's order -> SimpleNamespace(vertices [B, V, 3], joints [B, 24 + n_extra, 3], A [B, 24, 3, 4];
    and what the backward recomputes, for tests/smpl_vjp_ref.py: p [B, V, 3] the blended rest vertex, J [B, 24, 3], J_template, J_shape [24, 3, 10]).
    path = "mfma": skin_mfma_body (pd_scale, hi / lo split of both operands, per k-step of 16 the products c_lo . D_hi, c_hi . D_lo, c_hi . D_hi added
    to the float32 accumulator in that order, one rounding each);  path = "valu": skin_kernel's fmaf chains (sparse-4 or 24-joint transform as the
    asset's weights decide).  Sums of products are taken as the compiler contracts them (a * b + c -> fma).
    drop (mfma only): "a_lo" zeroes the coefficients' lo halves, "b_lo" the basis's, "cross" leaves both cross products out."""
    assert path in ("mfma", "valu") and drop in (None, "a_lo", "b_lo", "cross") and not (drop and path == "valu")
    f = np.float32
    vt, sd = np.asarray(asset["v_template"], f), np.asarray(asset["shapedirs"], f)
    pdirs, Jr, W = np.asarray(asset["posedirs"], f), np.asarray(asset["J_regressor"], f), np.asarray(asset["lbs_weights"], f)
    V = vt.shape[0]
    be = np.asarray(betas, f)
    R = np.asarray(rotmats, f).reshape(-1, KJ, 3, 3)
    B = R.shape[0]
    par = PARENTS
    # joint_basis_kernel: 256 strided fmaf chains, then the LDS tree
    n = math.ceil(V / 256)
    X = np.zeros((n * 256, 33), f)
    X[:V] = np.concatenate([vt, sd.reshape(V, 30)], 1)
    Jp = np.zeros((KJ, n * 256), f)
    Jp[:, :V] = Jr
    s = np.zeros((KJ, 33, 256), f)
    for i in range(n):
        s = _fma(Jp[:, None, i * 256:(i + 1) * 256], X[i * 256:(i + 1) * 256].T[None], s)
    o = 128
    while o > 0:
        s[..., :o] = s[..., :o] + s[..., o:2 * o]
        o >>= 1
    Jt, Js = s[:, :3, 0], s[:, 3:, 0].reshape(KJ, 3, 10)
    # pose_chain_body
    acc = np.zeros((B, KJ, 3), f)
    for l in range(10):
        acc = _fma(Js[None, :, :, l], be[:, None, None, l], acc)
    J = (Jt[None] + acc).astype(f)
    t = J.copy()
    t[:, 1:] = J[:, 1:] - J[:, par[1:]]
    Grot, Gt = np.zeros((B, KJ, 3, 3), f), np.zeros((B, KJ, 3), f)
    Grot[:, 0], Gt[:, 0] = R[:, 0], t[:, 0]
    for j in range(1, KJ):
        p = par[j]
        Grot[:, j] = _dot3(Grot[:, p], R[:, j])
        Gt[:, j] = (_dot3(Grot[:, p], t[:, j, :, None])[..., 0] + Gt[:, p]).astype(f)
    A = np.zeros((B, KJ, 3, 4), f)
    A[..., :3] = Grot
    gj = _dot3(Grot.reshape(B * KJ, 3, 3), J.reshape(B * KJ, 3, 1)).reshape(B, KJ, 3)
    A[..., 3] = Gt - gj
    # blend
    c = np.concatenate([(R[:, 1:] - np.eye(3, dtype=f)).astype(f).reshape(B, POSE_BASIS), be], 1)           # [B, 217]
    D = np.concatenate([pdirs, sd.reshape(V * 3, 10).T], 0)                                                    # [217, V * 3]
    if path == "valu":
        po = np.zeros((B, V * 3), f)
        for l in range(10):
            po = _fma(be[:, l, None], D[POSE_BASIS + l][None], po)
        po = (po + vt.reshape(1, V * 3)).astype(f)
        for k in range(POSE_BASIS):
            po = _fma(c[:, k, None], D[k][None], po)
        p = po.reshape(B, V, 3)
    else:
        scale = f(pd_scale(asset))
        cp, Dp = np.zeros((B, BLEND_K), f), np.zeros((BLEND_K, V * 3), f)
        cp[:, :c.shape[1]], Dp[:D.shape[0]] = c, D * scale
        (a_hi, a_lo), (b_hi, b_lo) = split16(cp), split16(Dp)
        if drop == "a_lo":
            a_lo = np.zeros_like(a_lo)
        if drop == "b_lo":
            b_lo = np.zeros_like(b_lo)
        products = [(a_hi, b_hi)] if drop == "cross" else [(a_lo, b_hi), (a_hi, b_lo), (a_hi, b_hi)]
        acc = np.zeros((B, V * 3), f)
        for st in range(BLEND_STEPS):
            k = slice(16 * st, 16 * st + 16)
            for a, b in products:
                acc = (acc.astype(np.float64) + a[:, k].astype(np.float64) @ b[k].astype(np.float64)).astype(f)
        p = _fma(acc, f(1.0) / scale, vt.reshape(1, V * 3)).reshape(B, V, 3)
    # weighted transform
    slots = sparse_slots(W)
    Af = A.reshape(B, KJ, 12)
    if slots is not None:
        idx, val = slots
        if path == "mfma":
            T = (val[0][None, :, None] * Af[:, idx[0]]).astype(f)
            first = 1
        else:
            T, first = np.zeros((B, V, 12), f), 0
        for s4 in range(first, 4):
            T = _fma(val[s4][None, :, None], Af[:, idx[s4]], T)
    else:
        assert path == "valu"
        T = np.zeros((B, V, 12), f)
        for j in range(KJ):
            T = _fma(W[None, :, j, None], Af[:, j, None, :], T)
    T = T.reshape(B, V, 3, 4)
    # apply: ((T0 px + T1 py) + T2 pz) + T3
    v = (T[..., 0] * p[:, :, None, 0]).astype(f)
    v = _fma(T[..., 1], p[:, :, None, 1], v)
    v = _fma(T[..., 2], p[:, :, None, 2], v)
    v = (v + T[..., 3]).astype(f)
    joints = np.concatenate([Gt, v[:, np.asarray(asset["extra_joints_idxs"], np.int64)]], 1)
    return SimpleNamespace(vertices=v, joints=joints, A=A, p=p, J=J, J_template=Jt, J_shape=Js)


# ------------------------------------------------------------------------------------------------ cases
V_MATRIX = (1, 33, 129, 257, 1157, 2305)         # what each reaches: the module docstring of tests/test_gpu_smpl_forward.py
B_MATRIX = (1, 16, 17, 23, 24, 32, 33, 65)
N_EXTRA = 5


class Case(SimpleNamespace):
    """V, n_extra, weights, asset_seed, B, family, seed, group ("matrix", "family", "dense"), blend (a broken split must show)"""

    @property
    def id(self):
        return f"{self.group}-V{self.V}-B{self.B}-{self.weights}-x{self.n_extra}-{self.family}"

    def asset(self):
        return cached_asset(self.V, self.asset_seed, self.n_extra, self.weights)

    def inputs(self):
        return inputs(self.family, self.B, self.seed)


@functools.lru_cache(maxsize=None)
def cached_asset(V, seed, n_extra, weights):
    return make_asset(V, seed, n_extra, weights)


def cases():
    """The one list both test files iterate.  matrix: V_MATRIX x B_MATRIX on sparse assets, N(0, 1) inputs (48).  family: the other input families at
    V in {33, 1157}, B in {17, 33}; those on the matrix-core path (B = 33) are tagged `blend` - the ten shape terms (and on `leaf` the 45
    leaf-rotation terms) dominate the blend in every one of them.  dense: more than four weights per row at B in {3, 40}, V in {33, 257}, and a sparse asset
    without extra joints at the same B."""
    out = []
    for V in V_MATRIX:
        for B in B_MATRIX:
            out.append(Case(V=V, n_extra=N_EXTRA, weights="sparse", asset_seed=0, B=B, family="normal", seed=1, group="matrix", blend=False))
    for V in (33, 1157):
        for B in (17, 33):
            for fam in FAMILIES[1:]:
                out.append(Case(V=V, n_extra=N_EXTRA, weights="sparse", asset_seed=0, B=B, family=fam, seed=2, group="family", blend=B >= MFMA_MIN_BODIES))
    for V in (33, 257):
        for B in (3, 40):
            out.append(Case(V=V, n_extra=N_EXTRA, weights="dense", asset_seed=1, B=B, family="normal", seed=3, group="dense", blend=False))
    for B in (3, 40):
        out.append(Case(V=33, n_extra=0, weights="sparse", asset_seed=1, B=B, family="normal", seed=3, group="dense", blend=False))
    return out
