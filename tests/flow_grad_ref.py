"""tests/flow_ref.py restated in torch, so that autograd differentiates it: both directions of the stage-1 flow, log_prob and the 'prohmr' rot6d
rule.  Every function runs in the dtype of the tensors it is given: float64 autograd is the reference of the flow's backward tests, float32 autograd
the measure of what a float32 chain may lose (the tests' error bars are multiples of the float32 run's distance from the float64 run).

Parameters are a {checkpoint name: tensor} dict (``tensors``), names as in flow_ref (``flow.flow._transform._transforms.{i}.*``).  Rows: R = B * S, row
r belongs to item r // S; the functions take the context per ITEM [B,ctx] and repeat it, so its gradient comes back per item.
"""
import numpy as np
import torch

from tests import flow_ref as fr

D, HIDDEN, PREFIX = fr.D, fr.HIDDEN, fr.PREFIX
AFFINE = ("log_scale", "shift", "lower_entries", "upper_entries", "unconstrained_upper_diag", "bias")


def tensors(sd, dtype, requires_grad=False):
    """The floating-point entries of a numpy state dict as leaf tensors of `dtype`; the index lists as int64 tensors; flags are left out."""
    out = {}
    for k, v in sd.items():
        v = np.asarray(v)
        if v.dtype.kind == "f":
            out[k] = torch.tensor(v, dtype=dtype, requires_grad=requires_grad)
        elif k.endswith("_features"):
            out[k] = torch.tensor(v.astype(np.int64))
    return out


def _lu(p, i):
    g = lambda n: p[f"{PREFIX}{i}.{n}"]
    dt = g("lower_entries").dtype
    il, iu = torch.tril_indices(D, D, -1), torch.triu_indices(D, D, 1)
    diag = torch.log1p(torch.exp(g("unconstrained_upper_diag"))) + 1e-3
    Lm = torch.eye(D, dtype=dt).index_put((il[0], il[1]), g("lower_entries"))
    U = torch.zeros(D, D, dtype=dt).index_put((iu[0], iu[1]), g("upper_entries")) + torch.diag(diag)
    return Lm, U


def residual_net(p, i, x_id, c, relu_inputs=None):
    """transform_net of coupling i (flow_ref.residual_net without BatchNorm); relu_inputs: a list that receives every ReLU input, in order."""
    g = lambda n: p[f"{PREFIX}{i}.transform_net.{n}"]
    lin = lambda n, x: x @ g(n + ".weight").T + g(n + ".bias")
    t = lin("initial_layer", torch.cat([x_id, c], 1))
    for k in range(2):
        u = t
        for j in range(2):
            if relu_inputs is not None:
                relu_inputs.append(u)
            u = lin(f"blocks.{k}.linear_layers.{j}", torch.relu(u))
        t = t + u * torch.sigmoid(lin(f"blocks.{k}.context_layer", c))
    return lin("final_layer", t)


def _coupling(p, i, x, c, sign, relu_inputs):
    idf, trf = p[f"{PREFIX}{i}.identity_features"], p[f"{PREFIX}{i}.transform_features"]
    v = residual_net(p, i, x[:, idf], c, relu_inputs)
    return x.index_add(1, trf, sign * v)


def forward(p, x, ctx, S, relu_inputs=None):
    """x [R,144] -> z [R,144] given the per-item context ctx [B,ctx_dim], R = B * S."""
    c = ctx.repeat_interleave(S, 0)
    for l in range(4):
        a, lu, cp = 3 * l, 3 * l + 1, 3 * l + 2
        x = torch.exp(p[f"{PREFIX}{a}.log_scale"]) * x + p[f"{PREFIX}{a}.shift"]
        Lm, U = _lu(p, lu)
        x = (x @ U.T) @ Lm.T + p[f"{PREFIX}{lu}.bias"]
        x = _coupling(p, cp, x, c, 1.0, relu_inputs)
    return x


def inverse(p, z, ctx, S, relu_inputs=None):
    """z [R,144] -> x [R,144]: the transforms inverted, in reverse order."""
    c = ctx.repeat_interleave(S, 0)
    x = z
    for l in reversed(range(4)):
        a, lu, cp = 3 * l, 3 * l + 1, 3 * l + 2
        x = _coupling(p, cp, x, c, -1.0, relu_inputs)
        Lm, U = _lu(p, lu)
        y = torch.linalg.solve_triangular(Lm, (x - p[f"{PREFIX}{lu}.bias"]).T, upper=False)
        x = torch.linalg.solve_triangular(U, y, upper=True).T
        x = (x - p[f"{PREFIX}{a}.shift"]) * torch.exp(-p[f"{PREFIX}{a}.log_scale"])
    return x


def logdet(p):
    total = 0.0
    for l in range(4):
        total = total + p[f"{PREFIX}{3 * l}.log_scale"].sum()
        total = total + torch.log(torch.log1p(torch.exp(p[f"{PREFIX}{3 * l + 1}.unconstrained_upper_diag"])) + 1e-3).sum()
    return total


def log_prob(p, x, ctx, S, relu_inputs=None):
    """(log_prob [R], z [R,144])."""
    z = forward(p, x, ctx, S, relu_inputs)
    return -0.5 * (z * z).sum(1) - fr.LOG_2PI_HALF_D + logdet(p), z


def sample_and_log_prob(p, z, ctx, S, relu_inputs=None):
    """(x [R,144], log_prob [R])."""
    return inverse(p, z, ctx, S, relu_inputs), -0.5 * (z * z).sum(1) - fr.LOG_2PI_HALF_D + logdet(p)


def rot6d_prohmr(x):
    """flow_ref.rot6d_prohmr in torch: x [..., 144] -> R [n,3,3]."""
    x = x.reshape(-1, 6)
    a1, a2 = x[:, 0:3], x[:, 3:6]
    b1 = a1 / torch.clamp_min(torch.linalg.norm(a1, dim=1, keepdim=True), 1e-12)
    u = a2 - (b1 * a2).sum(1, keepdim=True) * b1
    b2 = u / torch.clamp_min(torch.linalg.norm(u, dim=1, keepdim=True), 1e-12)
    return torch.stack([b1, b2, torch.linalg.cross(b1, b2)], -1)


def sines(x):
    """flow_ref's conditioning measure of the Gram-Schmidt step: the sine between the two 3-vectors of every joint of x [..., 144]."""
    p = np.asarray(x, np.float64).reshape(-1, 6)
    c = np.cross(p[:, :3], p[:, 3:])
    return np.linalg.norm(c, axis=1) / np.linalg.norm(p[:, :3], axis=1) / np.linalg.norm(p[:, 3:], axis=1)


# --------------------------------------------------------------------------------------------- the fold
def fold_numpy(log_scale, shift, lower_entries, upper_entries, unconstrained_upper_diag, bias):
    """ActNorm + LULinear as one affine map s <- s A^T + c, float64 numpy: (A, c, Ainv, logdet) - the statement GlowFlow.fold is held to."""
    f = lambda a: np.asarray(a, np.float64)
    Lm, U = fr.lu_matrices(dict(lower_entries=lower_entries, upper_entries=upper_entries, unconstrained_upper_diag=unconstrained_upper_diag))
    LU = Lm @ U
    A, c = LU * np.exp(f(log_scale))[None, :], LU @ f(shift) + f(bias)
    Ainv = np.exp(-f(log_scale))[:, None] * np.linalg.solve(U, np.linalg.solve(Lm, np.eye(D)))
    return A, c, Ainv, float(f(log_scale).sum() + np.log(np.diag(U)).sum())


def affine_of(sd, l):
    """The six affine parameters of block l of a numpy state dict, in the order of AFFINE."""
    return [np.asarray(sd[f"{PREFIX}{3 * l if n in AFFINE[:2] else 3 * l + 1}.{n}"]) for n in AFFINE]


# --------------------------------------------------------------------------------------------- error bars and seeded inputs
def context_rows(g, B, ctx):
    """The context rows of test_gpu_flow._context_rows: the leading camera features, post-ReLU image features, scene features."""
    return np.concatenate([g.normal(scale=0.3, size=(B, ctx - 2560)), g.uniform(0, 2, size=(B, 2048)), g.normal(size=(B, 512))], 1).astype(np.float32)


def bar_of(v32, v64):
    """The project's rule for free-running float32 chains: 8 x the float32 reference's distance from the float64 one, floored at one float32 ulp of
    the tensor's largest magnitude (the rounding of the result itself)."""
    v64 = np.asarray(v64, np.float64)
    return max(8.0 * float(np.abs(np.asarray(v32, np.float64) - v64).max()), float(np.spacing(np.float32(np.abs(v64).max()))))


def inputs(seed, B, S, ctx):
    g = np.random.Generator(np.random.PCG64(seed))
    c = context_rows(g, B, ctx)
    rows = g.normal(size=(B, S, 144)).astype(np.float32)
    rows[:, 0] = 0.0
    return c, rows


def run(sd, c, rows, S, sampling, dtype, cots=None):
    """One direction in `dtype` with autograd.  Returns dict(out = the outputs, relu = every ReLU input, grads = {name | 'rows' | 'ctx': gradient}
    when the cotangents `cots` (numpy, one per output) are given).  Outputs: (log_prob, z), or (x, log_prob, rotations [R,24,3,3])."""
    p = tensors(sd, dtype, requires_grad=cots is not None)
    ct = torch.tensor(c, dtype=dtype, requires_grad=cots is not None)
    rt = torch.tensor(rows.reshape(-1, 144), dtype=dtype, requires_grad=cots is not None)
    relu = []
    if sampling:
        x, lp = sample_and_log_prob(p, rt, ct, S, relu)
        out = (x, lp, rot6d_prohmr(x).reshape(-1, 24, 3, 3))
    else:
        out = log_prob(p, rt, ct, S, relu)
    res = dict(out=[o.detach().numpy() for o in out], relu=[u.detach().numpy() for u in relu])
    if cots is not None:
        names = [k for k, v in p.items() if v.requires_grad]
        total = sum((o * torch.tensor(np.asarray(g).reshape(o.shape), dtype=dtype)).sum() for o, g in zip(out, cots) if g is not None)
        gr = torch.autograd.grad(total, [p[k] for k in names] + [rt, ct], allow_unused=True)
        res["grads"] = {k: (None if g is None else g.numpy()) for k, g in zip(names + ["rows", "ctx"], gr)}
    return res


def relu_margin(r64, r32):
    """min over the ReLU-input tensors of (smallest |v| of the float64 run) / (that tensor's own bar); the kink condition needs it above 1."""
    return min(float(np.abs(a).min()) / bar_of(b, a) for a, b in zip(r64["relu"], r32["relu"]))
