"""Host-side reference, error bound and emulation of the SMPL VJP entries (ehm_smpl_backward, ehm_smpl_backward_ordered, ehm_smpl_backward_rot6d;
csrc/guidance.hip), for tests/test_smpl_vjp_ref_cpu.py and tests/test_gpu_smpl_vjp.py (numpy / torch float64, no GPU, no native library):

  backward64         the staged float64 restatement of what the seven kernels compute (NOT autograd; the CPU test shows it equals autograd)
  backward_rot6d64   the same for the 6-D entry: the de-normalised 6-vector as smpl_ref.round_once forms it, the Gram-Schmidt VJP on top
  bound, bound_rot6d per-element error bounds of grotmats / gbetas / gpose6d (below)
  emulate            the device's order of operations in numpy float32, both gA routes, with the `drop` variants - each a plausible kernel bug
  cases, cotangents  the one list of cases both test files iterate, and the cotangent families

Error model (as in tests/smpl_ref.py).  u = 2^-24.  The VJP is linear in the cotangents and multilinear in its coefficients (w, A.R, vp, R, t, J, the
basis rows), so the bound is a RUNNING one: every stage is run once more on absolute values with every subtraction an addition - the majorant M, the sum
of |terms| of that stage's output - and carries an error E beside it:
    E_out = stage(|coefficients|, E_in)  +  stage(E_coefficient, M_in)  +  k u M_out
the incoming error through the stage, the float32 error of a coefficient the backward recomputes (smpl_ref.bound_valu's E_p for the blended rest
vertex, E_Grot = E_A[..., :3], E_J, E_t, E_J_shape), and k roundings of the stage's own arithmetic, each at most u times a partial sum that M bounds.
The inputs (asset, betas, rotations, cotangents) are float32 and exact.  fma contraction only removes roundings.  The counts k, line by line:

extra_joints_bwd_kernel   `gv[idx[e]] += gjoints[...]`: one rounding per pick of that vertex:  k = the number of times the vertex is picked.
skin_bwd_kernel (atomic route), per entry of gA:
  * `w0 = wj * g0`, `w0 * vp`: 2 roundings of a term;
  * `atomicAdd(g + e, ...)` into LDS: at most min(V, 256) additions, in any order;  `atomicAdd(gA + ..., s)`: one addition per vertex tile, any order:
        k_gA = 2 + min(V, 256) + v_tiles
skin_gA_ordered_kernel / skin_gA_sum_kernel (ordered route):
  * the same 2 roundings of a term;  wave_sum: row16_sum's four `v +=` and the three additions of the four row sums, 7;  `sG[bb][j][e] += t` once per
    wave, 4;  `s += part[t]`, v_tiles:
        k_gA = 2 + 7 + 4 + v_tiles
skin_bwd_kernel, the transformed cotangent:
  * `T[e] = fmaf(wj, a[..], T[e])` once per non-zero weight of the row: n_w = the largest number of non-zeros in a row of lbs_weights;  the
    transform's rotation block carries E_Grot:  E_T = sum_j w_j E_Grot(j) + n_w u sum_j w_j |A.R(j)|
  * `o[0] = T[0] * g0 + T[3] * g1 + T[6] * g2`: 3 roundings.
posefeat_bwd_mfma_kernel / posefeat_sum_kernel: v_mfma_f32_32x32x2_f32 contracts two k per instruction - `acc[t] = mfma(a[i], b[i], acc[t])` forms
  a0 b0 + a1 b1 + acc - with one rounding per instruction, the accumulation model of tests/conv_x2_ref.py (a model of the matrix cores, not a source
  line: were each of the two products added with a rounding of its own, the 4 below would be an 8).  A chain (one accumulator of one wave) runs over
  n_g = the largest number of 8-k groups that any of the 32 K-chunks holds, 4 instructions per group;  `((acc + red[0]) + red[1]) + red[2]` adds 3;
  `s += part[q]` 7:
        k_pf = 4 n_g + 3 + 7
shape_bwd_kernel: `acc = fmaf(sv, g, acc)` over k = tid, tid + 256, ...: ceil(3 V / 256);  `v += __shfl_xor(v, o)` 6;  `((red[0] + red[1]) + red[2]) +
  red[3]` 3:
        k_sb = ceil(3 V / 256) + 9
chain_bwd_rotmat_kernel (chain_bwd_kernel alike):
  * `gA[...] - gt * Jx[c]`: the product and the difference, 2;  `gt + gjoints[...]`: 1.
  * `sC[j][r * 4 + c] = dG[0] * R[c * 3] + dG[1] * R[..] + dG[2] * R[..] + dG[3] * t[c]`: 4;  `dG[e] += sC[c][e]`: one per child (at most 3: the root, joint 9).
  * `s = GP[r] * dG[c] + GP[..] * dG[..] + GP[..] * dG[..]`: 3;  `s += gpf[...]`: 1.
  * `dt = GP[c] * dG[3] + ...`: 3;  `G[c] * gAt[0] + ...`: 3;  `dt - (...)`: 1;  `dJ[c] -= sT[child][c]`: one per child.
  * `s = fmaf(J_shape[...], sJ[jj][c], s)` over 24 joints x 3: 72;  `gbetas_v[...] + s`: 1.
rot6d_bwd (bound_rot6d): the rotations are the device's own, E_R = smpl_ref.gram_schmidt64's bound - it enters the forward quantities (bound_valu's
  E_R) and the `dG . R^T` product of the reverse chain; then, with M and E carried through the same lines:
  * `g1[0] += b2[1] * g3[2] - b2[2] * g3[1]`: 2 products, the difference, the addition - a term passes 3;  g2 alike.
  * `t = b2 . g2` 3, `b2[c] * t` 1, `g2[c] - ..` 1, `/ n2` 1: 6;  n2 carries E_n2 (the division is where the conditioning enters).
  * `gub1 = gu . b1`: 3;  `gu[c] - gub1 * b1[c]`: 2;  `g1[c] += -d * gu[c] - gub1 * a2[c]`: 4.
  * `t = b1 . g1` ... `/ n1`: 6, E_n1 = 2.5 u n1.
  Inputs keep smpl_ref.conditioning <= 4 (rot6d_inputs).

What the bound can tell apart: every `drop` variant of `emulate` loses or misplaces whole terms - an error of the order of M, against k u M with k at
most a few hundred - so each is over the bound by orders of magnitude on its designated case (tests/test_smpl_vjp_ref_cpu.py prints by how much)."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle.smpl import SMPLOracle
from tests import smpl_ref as R

U, KJ, PARENTS, POSE_BASIS = R.U, R.KJ, R.PARENTS, R.POSE_BASIS
VT, BG, PF_TILE, PF_CHUNKS, SB_BODIES = 256, 8, 32, 32, 4          # kVT, kBG, the pose-feature body tile, 4 waves x kPfSplit, kSbB
CHILDREN = [[c for c in range(KJ) if PARENTS[c] == j] for j in range(KJ)]
N_CHILD = np.array([len(c) for c in CHILDREN], np.float64)
DEPTH = [0] * KJ
for _j in range(1, KJ):
    DEPTH[_j] = DEPTH[PARENTS[_j]] + 1
DROPS = ("pf_tail", "tiles8", "dAt_J", "extra", "extra_once", "gbetas_v", "gpf_in", "last8", "last32")


def _f64(a):
    return np.asarray(a, np.float64)


def _scatter(gverts, gjoints, idx, B, V):
    """the vertex cotangent with the extra joints' rows added (every pick of a vertex counts), float64"""
    gv = np.zeros((B, V, 3)) if gverts is None else _f64(gverts).copy()
    if gjoints is not None:
        for e, i in enumerate(idx):
            gv[:, i] += _f64(gjoints)[:, KJ + e]
    return gv


def _gp(Grot):
    GP = np.empty_like(Grot)
    GP[:, 0] = np.eye(3)
    GP[:, 1:] = Grot[:, PARENTS[1:]]
    return GP


def _bases(asset):
    V = asset["v_template"].shape[0]
    return _f64(asset["posedirs"]), _f64(asset["shapedirs"]).reshape(V * 3, 10).T.copy()         # [207, 3 V], [10, 3 V]


# ------------------------------------------------------------------------------------------------ the float64 restatement
def backward64(asset, betas, rotmats, gverts, gjoints):
    """(grotmats [B, 24, 3, 3], gbetas [B, 10]) float64: the VJP of (vertices, joints) = SMPL(betas, rotmats) against the cotangents gverts [B, V, 3]
    and gjoints [B, 24 + n_extra, 3] (either may be None), stage by stage as csrc/guidance.hip computes it."""
    out = _backward64(asset, betas, rotmats, gverts, gjoints)
    return out.grotmats, out.gbetas


def _backward64(asset, betas, rotmats, gverts, gjoints):
    ref = R.forward64(asset, betas, rotmats)
    W = _f64(asset["lbs_weights"])
    V = W.shape[0]
    Rm = _f64(rotmats).reshape(-1, KJ, 3, 3)
    B = Rm.shape[0]
    J, Grot = ref.J.numpy(), ref.A.numpy()[..., :3]
    t = J.copy()
    t[:, 1:] -= J[:, PARENTS[1:]]
    c, D = R.blend_operands(asset, betas, Rm)
    vp = _f64(asset["v_template"])[None] + (c @ D).reshape(B, V, 3)
    PD, SD = _bases(asset)
    Js = np.einsum("jv,vcl->jcl", _f64(asset["J_regressor"]), _f64(asset["shapedirs"]))
    # 1. the extra joints are vertex picks
    gv = _scatter(gverts, gjoints, asset["extra_joints_idxs"], B, V)
    # 2. skinning: gA[j] = sum_v w[v, j] [gv (x) vp | gv],  gvp = (sum_j w A_j.R)^T gv
    gA_R = np.einsum("vj,bve->bje", W, (gv[..., :, None] * vp[..., None, :]).reshape(B, V, 9)).reshape(B, KJ, 3, 3)
    gA_t = np.einsum("vj,bvr->bjr", W, gv)
    T = np.einsum("vj,bje->bve", W, Grot.reshape(B, KJ, 9)).reshape(B, V, 3, 3)
    gvp = np.einsum("bvrc,bvr->bvc", T, gv)
    # 3. / 4. the two contractions of the blend
    gpf = gvp.reshape(B, V * 3) @ PD.T
    gbv = gvp.reshape(B, V * 3) @ SD.T
    # 5. reverse chain: A.R = G.R, A.t = G.t - G.R J, joint = G.t
    dG_R = gA_R - gA_t[..., :, None] * J[:, :, None, :]
    dG_t = gA_t + (0.0 if gjoints is None else _f64(gjoints)[:, :KJ])
    for j in range(KJ - 1, 0, -1):                          # (a child's index is above its parent's: every dG is complete when it is passed on)
        p = PARENTS[j]
        dG_R[:, p] += dG_R[:, j] @ Rm[:, j].transpose(0, 2, 1) + dG_t[:, j, :, None] * t[:, j, None, :]
        dG_t[:, p] += dG_t[:, j]
    GP = _gp(Grot)
    grot = np.einsum("bjkr,bjkc->bjrc", GP, dG_R)
    grot[:, 1:] += gpf.reshape(B, KJ - 1, 3, 3)
    # 6. rest joints: t_j = J_j - J_parent, A_j.t = G_j.t - G_j.R J_j;  into gbetas through J_shape, beside the blend's share
    dt = np.einsum("bjkc,bjk->bjc", GP, dG_t)
    dJ = dt - np.einsum("bjkc,bjk->bjc", Grot, gA_t)
    for j in range(1, KJ):
        dJ[:, PARENTS[j]] -= dt[:, j]
    gbetas = gbv + np.einsum("jcl,bjc->bl", Js, dJ)
    return SimpleNamespace(grotmats=grot, gbetas=gbetas, gvp=gvp, gA_R=gA_R, gA_t=gA_t, gpf=gpf, gbetas_v=gbv, dJ=dJ)


def autograd64(asset, betas, rotmats, gverts, gjoints):
    """the same by torch float64 autograd through oracle.smpl.SMPLOracle (what backward64 is checked against)"""
    be = torch.tensor(_f64(betas), requires_grad=True)
    rot = torch.tensor(_f64(rotmats).reshape(-1, KJ, 3, 3), requires_grad=True)
    out = SMPLOracle(asset, dtype=torch.float64)(be, rot[:, 1:], rot[:, :1])
    s = 0.0
    if gverts is not None:
        s = s + (out.vertices * torch.as_tensor(_f64(gverts))).sum()
    if gjoints is not None:
        s = s + (out.joints * torch.as_tensor(_f64(gjoints))).sum()
    gb, gr = torch.autograd.grad(s, (be, rot))
    return gr.numpy(), gb.numpy()


# ------------------------------------------------------------------------------------------------ rot6d
def _gs_vjp(a1, a2, gR):
    """float64: VJP of R = [b1 b2 b3] (columns; smpl_ref.gram_schmidt64) -> (ga1, ga2) [..., 3], the lines of rot6d_bwd"""
    dot = lambda x, y: (x * y).sum(-1, keepdims=True)
    n1 = np.sqrt(dot(a1, a1))
    b1 = a1 / n1
    d = dot(b1, a2)
    w = a2 - d * b1
    n2 = np.sqrt(dot(w, w))
    b2 = w / n2
    g1, g2, g3 = gR[..., 0].copy(), gR[..., 1].copy(), gR[..., 2]
    g1 += np.cross(b2, g3)
    g2 += np.cross(g3, b1)
    gu = (g2 - b2 * dot(b2, g2)) / n2
    gub1 = dot(gu, b1)
    ga2 = gu - gub1 * b1
    g1 += -d * gu - gub1 * a2
    ga1 = (g1 - b1 * dot(b1, g1)) / n1
    return ga1, ga2


def backward_rot6d64(asset, betas, x, mean, std, gverts):
    """gpose6d [B, 144] float64 of ehm_smpl_backward_rot6d: pose6d = x * std + mean rounded once to float32 (smpl_ref.round_once), R = Gram-Schmidt in
    float64, grotmats by backward64, then the Gram-Schmidt VJP in the 'diffusion' layout (a1 = pose6d[0::2], a2 = pose6d[1::2] of a joint)"""
    r6 = R.rot6d64(x, mean, std)
    grot, _ = backward64(asset, betas, r6.R, gverts, None)
    x6 = r6.pose6d.astype(np.float64).reshape(-1, KJ, 3, 2)
    ga1, ga2 = _gs_vjp(x6[..., 0], x6[..., 1], grot)
    return np.stack([ga1, ga2], -1).reshape(-1, 144)


def autograd_rot6d64(asset, betas, x, mean, std, gverts):
    p = torch.tensor(R.rot6d64(x, mean, std).pose6d.astype(np.float64), requires_grad=True)
    x6 = p.reshape(-1, KJ, 3, 2)
    a1, a2 = x6[..., 0], x6[..., 1]
    b1 = a1 / a1.norm(dim=-1, keepdim=True)
    w = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = w / w.norm(dim=-1, keepdim=True)
    rot = torch.stack([b1, b2, torch.cross(b1, b2, dim=-1)], -1)
    out = SMPLOracle(asset, dtype=torch.float64)(torch.as_tensor(_f64(betas)), rot[:, 1:], rot[:, :1])
    return torch.autograd.grad((out.vertices * torch.as_tensor(_f64(gverts))).sum(), p)[0].numpy()


# ------------------------------------------------------------------------------------------------ the bound
def pf_groups(V):
    """the K split of posefeat_bwd_mfma_kernel: (G, Gfull, [(g0, g1)] of the 32 chunks)"""
    V3 = 3 * V
    G, Gfull = (V3 + 7) // 8, V3 // 8
    return G, Gfull, [(c * G // PF_CHUNKS, (c + 1) * G // PF_CHUNKS) for c in range(PF_CHUNKS)]


def counts(asset, route):
    """the rounding counts of the module docstring for an asset and a gA route ("atomic", "ordered")"""
    assert route in ("atomic", "ordered")
    W = np.asarray(asset["lbs_weights"])
    V = W.shape[0]
    v_tiles = math.ceil(V / VT)
    n_g = max(g1 - g0 for g0, g1 in pf_groups(V)[2])
    return SimpleNamespace(gA=(2 + min(V, VT) + v_tiles) if route == "atomic" else (2 + 7 + 4 + v_tiles), n_w=int((W != 0).sum(1).max()),
                           pf=4 * n_g + 3 + 7, sb=math.ceil(3 * V / 256) + 9)


def _bound(asset, betas, rotmats, gverts, gjoints, route, E_R=None):
    """the running majorant / error pass of the module docstring -> (grotmats, gbetas) bounds and majorants"""
    k = counts(asset, route)
    fb = R.bound_valu(asset, betas, rotmats, E_R=E_R)
    W = _f64(asset["lbs_weights"])
    V = W.shape[0]
    Rm = _f64(rotmats).reshape(-1, KJ, 3, 3)
    B = Rm.shape[0]
    aR = np.abs(Rm)
    E_R = np.zeros_like(aR) if E_R is None else _f64(E_R)
    aGrot, E_Grot = np.abs(fb.ref.A.numpy()[..., :3]), fb.A[..., :3]
    avp, E_p = np.abs(fb.rest.p), fb.p
    aJ, E_J, at, E_t = np.abs(fb.rest.J), fb.J, np.abs(fb.rest.t), fb.t
    aJs, E_Js = np.abs(fb.rest.J_shape), fb.J_shape
    PD, SD = (np.abs(m) for m in _bases(asset))
    idx = np.asarray(asset["extra_joints_idxs"], np.int64)
    # extra_joints_bwd_kernel
    M_gv = _scatter(None if gverts is None else np.abs(_f64(gverts)), None if gjoints is None else np.abs(_f64(gjoints)), idx, B, V)
    picks = np.bincount(idx, minlength=V).astype(np.float64) if gjoints is not None else np.zeros(V)
    E_gv = picks[None, :, None] * U * M_gv
    # skin_bwd_kernel / skin_gA_ordered_kernel: gA
    outer = lambda a, b: (a[..., :, None] * b[..., None, :]).reshape(B, V, 9)
    wsum = lambda X: np.einsum("vj,bve->bje", W, X)
    M_gA_R = wsum(outer(M_gv, avp)).reshape(B, KJ, 3, 3)
    E_gA_R = wsum(outer(E_gv, avp) + outer(M_gv, E_p)).reshape(B, KJ, 3, 3) + k.gA * U * M_gA_R
    M_gA_t = wsum(M_gv)
    E_gA_t = wsum(E_gv) + k.gA * U * M_gA_t
    # skin_bwd_kernel: the transformed cotangent
    M_T = np.einsum("vj,bje->bve", W, aGrot.reshape(B, KJ, 9)).reshape(B, V, 3, 3)
    E_T = np.einsum("vj,bje->bve", W, E_Grot.reshape(B, KJ, 9)).reshape(B, V, 3, 3) + k.n_w * U * M_T
    M_gvp = np.einsum("bvrc,bvr->bvc", M_T, M_gv)
    E_gvp = np.einsum("bvrc,bvr->bvc", E_T, M_gv) + np.einsum("bvrc,bvr->bvc", M_T, E_gv) + 3 * U * M_gvp
    # posefeat_bwd_mfma_kernel, shape_bwd_kernel
    M_gpf = M_gvp.reshape(B, V * 3) @ PD.T
    E_gpf = E_gvp.reshape(B, V * 3) @ PD.T + k.pf * U * M_gpf
    M_gbv = M_gvp.reshape(B, V * 3) @ SD.T
    E_gbv = E_gvp.reshape(B, V * 3) @ SD.T + k.sb * U * M_gbv
    # chain_bwd_rotmat_kernel: dG
    M_dR = M_gA_R + M_gA_t[..., :, None] * aJ[:, :, None, :]
    E_dR = E_gA_R + E_gA_t[..., :, None] * aJ[:, :, None, :] + M_gA_t[..., :, None] * E_J[:, :, None, :] + 2 * U * M_dR
    M_dt = M_gA_t + (0.0 if gjoints is None else np.abs(_f64(gjoints)[:, :KJ]))
    E_dt = E_gA_t + U * M_dt
    for j in range(KJ - 1, 0, -1):
        p = PARENTS[j]
        E_dR[:, j] += N_CHILD[j] * U * M_dR[:, j]                     # (its own children are all in)
        E_dt[:, j] += N_CHILD[j] * U * M_dt[:, j]
        tr = lambda X: X.transpose(0, 2, 1)
        M_sC = M_dR[:, j] @ tr(aR[:, j]) + M_dt[:, j, :, None] * at[:, j, None, :]
        E_sC = (E_dR[:, j] @ tr(aR[:, j]) + M_dR[:, j] @ tr(E_R[:, j]) + E_dt[:, j, :, None] * at[:, j, None, :]
                + M_dt[:, j, :, None] * E_t[:, j, None, :] + 4 * U * M_sC)
        M_dR[:, p] += M_sC
        E_dR[:, p] += E_sC
        M_dt[:, p] += M_dt[:, j]
        E_dt[:, p] += E_dt[:, j]
    E_dR[:, 0] += N_CHILD[0] * U * M_dR[:, 0]
    E_dt[:, 0] += N_CHILD[0] * U * M_dt[:, 0]
    aGP, E_GP = _gp(aGrot), _gp(E_Grot)
    E_GP[:, 0] = 0.0                                                  # (the root's "parent rotation" is the exact identity)
    mm = lambda P, X: np.einsum("bjkr,bjkc->bjrc", P, X)
    mv = lambda P, x: np.einsum("bjkc,bjk->bjc", P, x)
    M_grot = mm(aGP, M_dR)
    E_grot = mm(E_GP, M_dR) + mm(aGP, E_dR) + 3 * U * M_grot
    M_grot[:, 1:] += M_gpf.reshape(B, KJ - 1, 3, 3)
    E_grot[:, 1:] += E_gpf.reshape(B, KJ - 1, 3, 3)
    E_grot += U * M_grot
    # rest joints and gbetas
    M_t = mv(aGP, M_dt)
    E_tt = mv(E_GP, M_dt) + mv(aGP, E_dt) + 3 * U * M_t
    M_a = mv(aGrot, M_gA_t)
    M_dJ = M_t + M_a
    E_dJ = E_tt + mv(E_Grot, M_gA_t) + mv(aGrot, E_gA_t) + 3 * U * M_a
    for j in range(1, KJ):
        M_dJ[:, PARENTS[j]] += M_t[:, j]
        E_dJ[:, PARENTS[j]] += E_tt[:, j]
    E_dJ += (1 + N_CHILD)[None, :, None] * U * M_dJ
    M_gb = M_gbv + np.einsum("jcl,bjc->bl", aJs, M_dJ)
    E_gb = E_gbv + np.einsum("jcl,bjc->bl", E_Js, M_dJ) + np.einsum("jcl,bjc->bl", aJs, E_dJ) + (3 * KJ + 1) * U * M_gb
    return SimpleNamespace(grotmats=E_grot, gbetas=E_gb, M_grotmats=M_grot, M_gbetas=M_gb)


def bound(asset, betas, rotmats, gverts, gjoints, route):
    """Per-element bounds .grotmats [B, 24, 3, 3], .gbetas [B, 10] of ehm_smpl_backward (route "atomic") / ehm_smpl_backward_ordered ("ordered"), and the
    majorants .M_grotmats, .M_gbetas they scale with.  An element whose majorant is zero has a zero bound: it must come out an exact zero."""
    return _bound(asset, betas, rotmats, gverts, gjoints, route)


def bound_rot6d(asset, betas, x, mean, std, gverts):
    """Per-element bound [B, 144] of ehm_smpl_backward_rot6d's gpose6d (the atomic gA route; module docstring, rot6d_bwd)"""
    r6 = R.rot6d64(x, mean, std)
    assert r6.cond.max() <= 4.0
    g = _bound(asset, betas, r6.R, gverts, None, "atomic", E_R=r6.E_R)
    x6 = r6.pose6d.astype(np.float64).reshape(-1, KJ, 3, 2)
    a1, a2 = x6[..., 0], x6[..., 1]
    dot = lambda p, q: (p * q).sum(-1, keepdims=True)
    n1 = np.sqrt(dot(a1, a1))
    b1 = a1 / n1
    d = dot(b1, a2)
    w = a2 - d * b1
    n2 = np.sqrt(dot(w, w))
    b2 = w / n2
    ab1, ab2, aa2 = np.abs(b1), np.abs(b2), np.abs(a2)
    E_b1, E_b2 = r6.E_R[..., 0], r6.E_R[..., 1]
    E_n1 = 2.5 * U * n1
    E_d = dot(E_b1, aa2) + 3 * U * dot(ab1, aa2)
    E_w = E_d * ab1 + np.abs(d) * E_b1 + U * np.abs(d * b1) + U * np.abs(w)
    E_n2 = dot(np.abs(w), E_w) / n2 + 2.5 * U * n2
    r1, r2 = lambda v: np.roll(v, -1, -1), lambda v: np.roll(v, -2, -1)
    acr = lambda p, q: r1(p) * r2(q) + r2(p) * r1(q)                   # the majorant of a cross product
    M, E = g.M_grotmats, g.grotmats
    M1, M2, M3, E1, E2, E3 = M[..., 0].copy(), M[..., 1].copy(), M[..., 2], E[..., 0].copy(), E[..., 1].copy(), E[..., 2]
    M1 += acr(ab2, M3)
    E1 += acr(E_b2, M3) + acr(ab2, E3) + 3 * U * M1
    M2 += acr(M3, ab1)
    E2 += acr(M3, E_b1) + acr(E3, ab1) + 3 * U * M2
    Mt = dot(ab2, M2)
    Mu = (M2 + ab2 * Mt) / n2
    Eu = (E2 + E_b2 * Mt + ab2 * (dot(E_b2, M2) + dot(ab2, E2))) / n2 + Mu * E_n2 / n2 + 6 * U * Mu
    Mub = dot(Mu, ab1)
    Eub = dot(Eu, ab1) + dot(Mu, E_b1) + 3 * U * Mub
    Ma2 = Mu + Mub * ab1
    Ea2 = Eu + Eub * ab1 + Mub * E_b1 + 2 * U * Ma2
    M1 += np.abs(d) * Mu + Mub * aa2
    E1 += E_d * Mu + np.abs(d) * Eu + Eub * aa2 + 4 * U * M1
    Mt1 = dot(ab1, M1)
    Ma1 = (M1 + ab1 * Mt1) / n1
    Ea1 = (E1 + E_b1 * Mt1 + ab1 * (dot(E_b1, M1) + dot(ab1, E1))) / n1 + Ma1 * E_n1 / n1 + 6 * U * Ma1
    return np.stack([Ea1, Ea2], -1).reshape(-1, 144)


def ratios(got_rot, got_betas, ref_rot, ref_betas, bnd):
    """{group: largest error / bound}; an output that was not asked for (None) is left out"""
    r = {}
    if got_rot is not None:
        r["grotmats"] = R.ratio(np.asarray(got_rot).reshape(ref_rot.shape), ref_rot, bnd.grotmats)
    if got_betas is not None:
        r["gbetas"] = R.ratio(got_betas, ref_betas, bnd.gbetas)
    return r


# ------------------------------------------------------------------------------------------------ the device's order of operations
_fma = R._fma


def _chain3(a, b):
    """sum_k a[k] * b[k] over three operand pairs in the kernels' order: the first product rounded, then two fmas (float32)"""
    acc = (a[0] * b[0]).astype(np.float32)
    return _fma(a[2], b[2], _fma(a[1], b[1], acc))


def _tree(x, far):
    """float32 pairwise tree over the last axis (a power of two): neighbours first (row16_sum's DPP steps) or far halves first (xor shuffles 32 ... 1)"""
    while x.shape[-1] > 1:
        n = x.shape[-1] // 2
        x = (x[..., :n] + x[..., n:]) if far else (x[..., 0::2] + x[..., 1::2])
    return x[..., 0]


def emulate(asset, betas, rotmats, gverts, gjoints, route, drop=None):
    """ehm_smpl_backward (route "atomic": the LDS and global float atomics taken in ONE order, vertices then tiles ascending) or ehm_smpl_backward_ordered
    ("ordered": exactly) in numpy float32 -> (grotmats [B, 24, 3, 3], gbetas [B, 10]).  drop = one of DROPS, a broken kernel:
      pf_tail     the partial last 8-k group of the pose-feature contraction left out
      tiles8      vertex tiles >= 8 left out of both skinning kernels (the second XCD round)
      dAt_J       `- dA.t (x) J` missing from dG.R
      extra       the extra joints' cotangent not scattered;   extra_once: scattered once for a repeated index
      gbetas_v    the blend's share left out of gbetas
      gpf_in      the pose-feature contraction taken with the incoming cotangent, not the in-place transformed one
      last8       the last body of a partial 8-body skinning group left zero;   last32: of a partial 32-body pose-feature tile"""
    assert route in ("atomic", "ordered") and (drop is None or drop in DROPS)
    f = np.float32
    fw = R.emulate(asset, betas, rotmats, "valu")               # pose_chain_body and the VALU blend: what both skinning kernels recompute
    W = np.asarray(asset["lbs_weights"], f)
    V = W.shape[0]
    Rm = np.asarray(rotmats, f).reshape(-1, KJ, 3, 3)
    B = Rm.shape[0]
    idx = np.asarray(asset["extra_joints_idxs"], np.int64)
    vp, J, A = fw.p, fw.J, fw.A
    Grot = A[..., :3]
    t = J.copy()
    t[:, 1:] = J[:, 1:] - J[:, PARENTS[1:]]
    # extra_joints_bwd_kernel: the picks in index order
    gv = np.zeros((B, V, 3), f) if gverts is None else np.asarray(gverts, f).copy()
    if gjoints is not None and drop != "extra":
        seen = set()
        for e, i in enumerate(idx):
            if drop == "extra_once" and int(i) in seen:
                continue
            seen.add(int(i))
            gv[:, i] = gv[:, i] + np.asarray(gjoints, f)[:, KJ + e]
    # gA
    v_tiles = math.ceil(V / VT)
    live_tiles = min(v_tiles, 8) if drop == "tiles8" else v_tiles
    pad = v_tiles * VT - V
    gA = np.zeros((B, KJ, 12), f)
    Wp = np.concatenate([W, np.zeros((pad, KJ), f)], 0)
    for b in range(B):
        g4 = np.concatenate([gv[b], np.zeros((pad, 3), f)], 0)
        p4 = np.concatenate([np.concatenate([vp[b], np.ones((V, 1), f)], 1), np.zeros((pad, 4), f)], 0)         # [vp | 1]: w * 1 is exact
        wg = (Wp[:, :, None] * g4[:, None, :]).astype(f)                                                         # w0, w1, w2
        c = (wg[:, :, :, None] * p4[:, None, None, :]).astype(f).reshape(v_tiles, VT, KJ, 12)[:live_tiles]
        if route == "ordered":
            waves = c.reshape(live_tiles, 4, 64, KJ, 12).transpose(0, 1, 3, 4, 2)                                # lanes last
            rows = _tree(waves.reshape(live_tiles, 4, KJ, 12, 4, 16), far=False)                                 # row16_sum
            ws = ((rows[..., 0] + rows[..., 1]) + rows[..., 2]) + rows[..., 3]                                    # wave_sum
            tile = np.zeros((live_tiles, KJ, 12), f)
            for w_ in range(4):
                tile = tile + ws[:, w_]
        else:
            tile = np.zeros((live_tiles, KJ, 12), f)
            for i in range(VT):
                tile = tile + c[:, i]
        s = np.zeros((KJ, 12), f)
        for tl in range(live_tiles):
            s = s + tile[tl]
        gA[b] = s
    if drop == "last8" and B % BG:
        gA[B - 1] = 0
    # skin_bwd_kernel: gvp in place
    T = np.zeros((B, V, 9), f)
    for j in range(KJ):
        T = _fma(W[None, :, j, None], Grot[:, j].reshape(B, 1, 9), T)
    T = T.reshape(B, V, 3, 3)
    gvp = _chain3([T[:, :, 0], T[:, :, 1], T[:, :, 2]], [gv[..., 0, None], gv[..., 1, None], gv[..., 2, None]])
    if drop == "tiles8":
        gvp[:, 8 * VT:] = gv[:, 8 * VT:]
    if drop == "last8" and B % BG:
        gvp[B - 1] = gv[B - 1]
    # posefeat_bwd_mfma_kernel: 32 chunks of 8-k groups, four instructions a group, each contracting k + i and k + 4 + i with one rounding
    V3 = V * 3
    G, Gfull, chunks = pf_groups(V)
    PD = np.zeros((POSE_BASIS, G * 8), np.float64)
    PD[:, :V3] = asset["posedirs"]
    X = np.zeros((B, G * 8), np.float64)
    X[:, :V3] = (gv if drop == "gpf_in" else gvp).reshape(B, V3)
    part = np.zeros((PF_CHUNKS, B, POSE_BASIS), f)
    for ci, (g0, g1) in enumerate(chunks):
        acc = np.zeros((B, POSE_BASIS), f)
        for g in range(g0, g1):
            if g >= Gfull and drop == "pf_tail":
                continue
            for i in range(4):
                ks = [8 * g + i, 8 * g + 4 + i]
                acc = (acc.astype(np.float64) + X[:, ks] @ PD[:, ks].T).astype(f)
        part[ci] = acc
    part = part.reshape(8, 4, B, POSE_BASIS)
    blk = ((part[:, 0] + part[:, 1]) + part[:, 2]) + part[:, 3]
    gpf = blk[0]
    for q in range(1, 8):
        gpf = gpf + blk[q]
    if drop == "last32" and B % PF_TILE:
        gpf[B - 1] = 0
    # shape_bwd_kernel
    n = math.ceil(V3 / 256)
    SD = np.zeros((10, n * 256), f)
    SD[:, :V3] = np.asarray(asset["shapedirs"], f).reshape(V3, 10).T
    Xs = np.zeros((B, n * 256), f)
    Xs[:, :V3] = gvp.reshape(B, V3)
    acc = np.zeros((B, 10, 256), f)
    for i in range(n):
        acc = _fma(SD[None, :, i * 256:(i + 1) * 256], Xs[:, None, i * 256:(i + 1) * 256], acc)
    wv = _tree(acc.reshape(B, 10, 4, 64), far=True)
    gbv = ((wv[..., 0] + wv[..., 1]) + wv[..., 2]) + wv[..., 3]
    if drop == "gbetas_v":
        gbv = np.zeros_like(gbv)
    # chain_bwd_rotmat_kernel
    gA = gA.reshape(B, KJ, 3, 4)
    gAt = gA[..., 3]
    dG = np.zeros((B, KJ, 3, 4), f)
    dG[..., :3] = gA[..., :3] if drop == "dAt_J" else _fma(-gAt[..., :, None], J[:, :, None, :], gA[..., :3])
    dG[..., 3] = gAt if gjoints is None else gAt + np.asarray(gjoints, f)[:, :KJ]
    for d in range(max(DEPTH), 0, -1):
        level = [j for j in range(KJ) if DEPTH[j] == d]
        sC = {}
        for j in level:
            Rt = Rm[:, j].transpose(0, 2, 1)                                                                      # [k, c] = R[c][k]
            acc = _chain3([dG[:, j, :, 0, None], dG[:, j, :, 1, None], dG[:, j, :, 2, None]], [Rt[:, None, 0], Rt[:, None, 1], Rt[:, None, 2]])
            sC[j] = np.concatenate([_fma(dG[:, j, :, 3, None], t[:, j, None, :], acc), dG[:, j, :, 3, None]], 2)
        for j in level:
            dG[:, PARENTS[j]] = dG[:, PARENTS[j]] + sC[j]
    GP = _gp(Grot)
    col = lambda M, c: [M[..., 0, c], M[..., 1, c], M[..., 2, c]]
    grot = np.zeros((B, KJ, 3, 3), f)
    for r in range(3):
        for c in range(3):
            grot[..., r, c] = _chain3(col(GP, r), col(dG, c))
    grot[:, 1:] = grot[:, 1:] + gpf.reshape(B, KJ - 1, 3, 3)
    dt = np.stack([_chain3(col(GP, c), col(dG, 3)) for c in range(3)], -1)
    dJ = np.stack([dt[..., c] - _chain3(col(Grot, c), [gAt[..., 0], gAt[..., 1], gAt[..., 2]]) for c in range(3)], -1).astype(f)
    for j in range(1, KJ):                                            # (ascending children per parent)
        dJ[:, PARENTS[j]] = dJ[:, PARENTS[j]] - dt[:, j]
    s = np.zeros((B, 10), f)
    for jj in range(KJ):
        for c in range(3):
            s = _fma(fw.J_shape[None, jj, c, :], dJ[:, jj, c, None], s)
    return grot, (gbv + s).astype(f)


# ------------------------------------------------------------------------------------------------ cases
V_SMALL = (1, 3, 4, 7, 8, 13, 86, 255, 256, 257)            # what each reaches: the module docstring of tests/test_gpu_smpl_vjp.py
V_LARGE = 2305
B_ALL = (1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 65)
COTANGENTS = ("dense", "verts", "joints", "one_vertex", "zero_bodies", "posed24", "extra")
N_EXTRA = R.N_EXTRA


class Case(SimpleNamespace):
    """V, B, n_extra, weights, asset_seed, family, seed, cot (a cotangent family), group ("shape", "cotangent", "asset", "family")"""

    @property
    def id(self):
        return f"{self.group}-V{self.V}-B{self.B}-{self.weights}-x{self.n_extra}-{self.family}-{self.cot}"

    def asset(self):
        return R.cached_asset(self.V, self.asset_seed, self.n_extra, self.weights)

    def inputs(self):
        return R.inputs(self.family, self.B, self.seed)

    def cotangents(self):
        return cotangents(self.cot, self.B, self.V, self.n_extra, self.seed)


ZERO_BODY, NEG_ZERO_BODY = 0, -1             # of zero_bodies: the first body all +0.0, the last all -0.0 (both in a group with live bodies when B > 2)


def cotangents(cot, B, V, n_extra, seed):
    """(gverts [B, V, 3] or None, gjoints [B, 24 + n_extra, 3] or None) float32:
      dense        N(0, 1) on vertices and joints             verts / joints   one of the two, the other None
      one_vertex   a single non-zero vertex (the last one of the body) in the middle body, no joints: every other block takes the early exit
      zero_bodies  dense vertices, no joints; body 0 all +0.0 and body B - 1 all -0.0
      posed24      joints only, zero on the extra joints      extra            joints only, zero on the 24 posed joints"""
    assert cot in COTANGENTS
    g = R._rng("cotangent", cot, B, V, seed)
    gv = g.normal(size=(B, V, 3)).astype(np.float32)
    gj = g.normal(size=(B, KJ + n_extra, 3)).astype(np.float32)
    if cot == "verts":
        return gv, None
    if cot == "joints":
        return None, gj
    if cot == "one_vertex":
        one = np.zeros_like(gv)
        one[B // 2, V - 1] = gv[B // 2, V - 1]
        return one, None
    if cot == "zero_bodies":
        gv[ZERO_BODY] = 0.0
        gv[NEG_ZERO_BODY] = -0.0
        return gv, None
    if cot == "posed24":
        gj[:, KJ:] = 0.0
        return None, gj
    if cot == "extra":
        gj[:, :KJ] = 0.0
        return None, gj
    return gv, gj


def cases():
    """The one list both test files iterate.
    shape: dense cotangents, sparse asset with five extra joints (ids V - 1, 0, V - 1 again, two random), N(0, 1) inputs: every V_SMALL at B in {1, 9, 33},
        every B_ALL at V in {7, 257}, V = 2305 at B in {9, 65}.
    cotangent: the other families at (V, B) = (13, 9) and (257, 9); one_vertex also at (2305, 9).
    asset: dense weights (six non-zeros in a row) and n_extra = 0 (dense cotangents, and joints only: jstride 72) at (13, 9) and (257, 33).
    family: betas x 5 and the identity pose at (13, 9) and (257, 33)."""
    mk = lambda **kw: Case(**{**dict(n_extra=N_EXTRA, weights="sparse", asset_seed=0, family="normal", seed=11, cot="dense"), **kw})
    shapes = [(V, B) for V in V_SMALL for B in (1, 9, 33)]
    shapes += [(V, B) for V in (7, 257) for B in B_ALL if (V, B) not in shapes]
    shapes += [(V_LARGE, 9), (V_LARGE, 65)]
    out = [mk(V=V, B=B, group="shape") for V, B in shapes]
    for V, B in ((13, 9), (257, 9)):
        out += [mk(V=V, B=B, cot=cot, seed=12, group="cotangent") for cot in COTANGENTS[1:]]
    out.append(mk(V=V_LARGE, B=9, cot="one_vertex", seed=12, group="cotangent"))
    for V, B in ((13, 9), (257, 33)):
        out.append(mk(V=V, B=B, weights="dense", asset_seed=1, seed=13, group="asset"))
        out.append(mk(V=V, B=B, n_extra=0, asset_seed=1, seed=13, group="asset"))
        out.append(mk(V=V, B=B, n_extra=0, asset_seed=1, seed=13, cot="joints", group="asset"))
        out += [mk(V=V, B=B, family=fam, seed=14, group="family") for fam in ("betas5", "identity")]
    return out


ROT6D_SHAPES = tuple((V, B) for V in (1, 257, V_LARGE) for B in (1, 9, 33))


def rot6d_case(V, B):
    """(asset, betas, x, mean, std, gverts) of a rot6d case: smpl_ref.rot6d_inputs (conditioning <= 4), N(0, 1) betas and vertex cotangents"""
    x, mean, std = R.rot6d_inputs(B, 3)
    return (R.cached_asset(V, 0, N_EXTRA, "sparse"), R.inputs("normal", B, 15).betas, x, mean, std, cotangents("verts", B, V, N_EXTRA, 15)[0])


# (drop variant, the case on which it must show: V, B, cotangent family) - tests/test_smpl_vjp_ref_cpu.py
DESIGNATED = (("pf_tail", 13, 9, "dense"), ("tiles8", V_LARGE, 9, "dense"), ("dAt_J", 13, 9, "dense"), ("extra", 13, 9, "extra"),
              ("extra_once", 13, 9, "extra"), ("gbetas_v", 13, 9, "dense"), ("gpf_in", 13, 9, "dense"), ("last8", 13, 9, "dense"),
              ("last32", 13, 33, "dense"))


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """the float64 reference of a case, computed once: SimpleNamespace(grotmats, gbetas)"""
    case = next(c for c in cases() if c.id == case_id)
    x = case.inputs()
    gv, gj = case.cotangents()
    grot, gb = backward64(case.asset(), x.betas, x.rotmats, gv, gj)
    return SimpleNamespace(grotmats=grot, gbetas=gb)
