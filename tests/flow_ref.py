"""The stage-1 pose flow restated in numpy: nflows' ConditionalGlow(144, 1024, 4, 2, context_features=ctx) as models/prohmr/smpl_flow.py builds it,
inference only, both directions.  nflows (ProHMR's fork) is not a dependency and its source is not at hand: this file restates ProHMR section 3.2
(each block f_AC . f_LT . f_IN) with the layers of published nflows (ActNorm, LULinear, AdditiveCouplingTransform, nn.nets.ResidualNet) and is the
reference of every flow test.  Every function runs in the dtype it is given: float64 is the reference, float32 the measure of what a float32 chain
may lose (the tests' error bars are multiples of the float32 run's distance from the float64 run on the same inputs).

A state dict here is a plain {name: numpy array} with the checkpoint's names, ``flow.flow._transform._transforms.{i}.*``; the transforms are
applied in index order x -> z ("forward", what log_prob uses) and in reverse order, inverted, z -> x (sampling).  Rows: R = B * S, row r belongs
to item r // S (nflows repeats each context row S times consecutively).
"""
import re

import numpy as np

D, HIDDEN = 144, 1024
PREFIX = "flow.flow._transform._transforms."
LOG_2PI_HALF_D = 72.0 * np.log(2.0 * np.pi)            # D / 2 * log(2 pi)
BN_EPS = 1e-3                                          # nflows' ResidualBlock: BatchNorm1d(features, eps=1e-3)


# --------------------------------------------------------------------------------------------- the checkpoint's structure
def transform_keys(sd, prefix=PREFIX):
    """{index: {name below the transform: array}} of the keys under `prefix`."""
    out = {}
    for k, v in sd.items():
        if k.startswith(prefix):
            m = re.match(r"(\d+)\.(.+)$", k[len(prefix):])
            if m is None:
                raise KeyError(f"flow checkpoint: {k} is not <index>.<name> below {prefix}")
            out.setdefault(int(m.group(1)), {})[m.group(2)] = v
    return out


def infer_kinds(sd, prefix=PREFIX):
    """The kind of each transform from its key set, in index order: 'actnorm' (log_scale), 'lulinear' (lower_entries), 'coupling'
    (transform_net.*).  Anything else, a gap in the indices, an affine coupling (final_layer with 144 rows) and an ActNorm whose `initialized` is
    False are refused, naming what was found."""
    tk = transform_keys(sd, prefix)
    if sorted(tk) != list(range(len(tk))):
        raise KeyError(f"flow checkpoint: transform indices {sorted(tk)} are not 0 .. n-1")
    kinds = []
    for i in range(len(tk)):
        names = set(tk[i])
        if "log_scale" in names:
            if "initialized" in names and not bool(np.asarray(tk[i]["initialized"])):
                raise ValueError(f"flow checkpoint: ActNorm {prefix}{i} has initialized == False (data-dependent initialisation belongs to training)")
            kinds.append("actnorm")
        elif "lower_entries" in names:
            kinds.append("lulinear")
        elif any(n.startswith("transform_net.") for n in names):
            rows = np.asarray(tk[i]["transform_net.final_layer.weight"]).shape[0]
            if rows != D // 2:
                raise ValueError(f"flow checkpoint: coupling {prefix}{i} has a final_layer of {rows} rows (affine coupling has {D}); only the additive "
                                 f"coupling ({D // 2} rows) is built")
            kinds.append("coupling")
        else:
            raise KeyError(f"flow checkpoint: unknown transform {prefix}{i} with keys {sorted(names)}")
    return kinds


# --------------------------------------------------------------------------------------------- the layers
def softplus(x):
    return np.log1p(np.exp(x))


def lu_matrices(p, dtype=np.float64):
    """(L unit lower triangular, U = strict upper + diag(softplus(unconstrained_upper_diag) + 1e-3)); the entries fill tril / triu indices row-major."""
    Lm, U = np.eye(D, dtype=dtype), np.zeros((D, D), dtype=dtype)
    Lm[np.tril_indices(D, -1)] = np.asarray(p["lower_entries"], dtype)
    U[np.triu_indices(D, 1)] = np.asarray(p["upper_entries"], dtype)
    U[np.diag_indices(D)] = softplus(np.asarray(p["unconstrained_upper_diag"], dtype)) + dtype(1e-3)
    return Lm, U


def has_batch_norm(p):
    return any(".batch_norm_layers." in n for n in p)


def _bn(p, name, x, dtype):
    g = lambda leaf: np.asarray(p[f"{name}.{leaf}"], dtype)
    return (x - g("running_mean")) / np.sqrt(g("running_var") + dtype(BN_EPS)) * g("weight") + g("bias")


def residual_net(p, x_id, c, dtype=np.float64):
    """transform_net of a coupling (nflows.nn.nets.ResidualNet, two blocks, eval mode) on x_id [R,72] and the context c [R,ctx]."""
    g = lambda name: np.asarray(p["transform_net." + name], dtype)
    lin = lambda name, x: x @ g(name + ".weight").T + g(name + ".bias")
    bn = has_batch_norm(p)
    t = lin("initial_layer", np.concatenate([x_id, c], 1))
    for k in range(2):
        u = t
        for j in range(2):
            if bn:
                u = _bn(p, f"transform_net.blocks.{k}.batch_norm_layers.{j}", u, dtype)
            u = lin(f"blocks.{k}.linear_layers.{j}", np.maximum(u, 0))
        gate = lin(f"blocks.{k}.context_layer", c)
        t = t + u * (1 / (1 + np.exp(-gate)))                    # F.glu(cat[u, context]) + the residual
    return lin("final_layer", t)


def _coupling(p, x, c, sign, dtype):
    idf, trf = np.asarray(p["identity_features"]).astype(np.int64), np.asarray(p["transform_features"]).astype(np.int64)
    y = x.copy()
    y[:, trf] = x[:, trf] + sign * residual_net(p, x[:, idf], c, dtype)
    return y


def forward(sd, x, c, dtype=np.float64):
    """x [R,144] -> z [R,144] given the context rows c [R,ctx]."""
    x, c = np.asarray(x, dtype), np.asarray(c, dtype)
    tk = transform_keys(sd)
    for i, kind in enumerate(infer_kinds(sd)):
        p = tk[i]
        if kind == "actnorm":
            x = np.exp(np.asarray(p["log_scale"], dtype)) * x + np.asarray(p["shift"], dtype)
        elif kind == "lulinear":
            Lm, U = lu_matrices(p, dtype)
            x = (x @ U.T) @ Lm.T + np.asarray(p["bias"], dtype)
        else:
            x = _coupling(p, x, c, 1, dtype)
    return x


def inverse(sd, z, c, dtype=np.float64):
    """z [R,144] -> x [R,144]: the transforms inverted, in reverse order."""
    x, c = np.asarray(z, dtype), np.asarray(c, dtype)
    tk = transform_keys(sd)
    kinds = infer_kinds(sd)
    for i in reversed(range(len(kinds))):
        p = tk[i]
        if kinds[i] == "actnorm":
            x = (x - np.asarray(p["shift"], dtype)) * np.exp(-np.asarray(p["log_scale"], dtype))
        elif kinds[i] == "lulinear":
            Lm, U = lu_matrices(p, dtype)
            x = np.linalg.solve(U, np.linalg.solve(Lm, (x - np.asarray(p["bias"], dtype)).T)).T
        else:
            x = _coupling(p, x, c, -1, dtype)
    return x


def logdet(sd):
    """log |det dz/dx| of the forward direction: data independent, float64."""
    tk = transform_keys(sd)
    total = 0.0
    for i, kind in enumerate(infer_kinds(sd)):
        if kind == "actnorm":
            total += float(np.asarray(tk[i]["log_scale"], np.float64).sum())
        elif kind == "lulinear":
            total += float(np.log(softplus(np.asarray(tk[i]["unconstrained_upper_diag"], np.float64)) + 1e-3).sum())
    return total


def _base_log_prob(z, dtype):
    if dtype == np.float32:                   # the squares added in index order by float32 fmaf (a float32 product is exact in float64)
        ss = np.zeros(z.shape[0], np.float32)
        for i in range(z.shape[1]):
            ss = (z[:, i].astype(np.float64) * z[:, i].astype(np.float64) + ss.astype(np.float64)).astype(np.float32)
        return np.float32(-0.5) * ss - np.float32(LOG_2PI_HALF_D)
    return -0.5 * (z * z).sum(1) - LOG_2PI_HALF_D


def log_prob(sd, x, c, dtype=np.float64):
    """(log_prob [R], z [R,144]) of x given c: -1/2 ||z||^2 - 72 log 2 pi + the forward log|det|."""
    z = forward(sd, x, c, dtype)
    return _base_log_prob(z, dtype) + dtype(logdet(sd)), z


def sample_and_log_prob(sd, z, c, dtype=np.float64):
    """(x [R,144], log_prob [R]) of the noise z: x = inverse(z), log_prob = (-1/2 ||z||^2 - 72 log 2 pi) - log|det| of the inverse."""
    z = np.asarray(z, dtype)
    return inverse(sd, z, c, dtype), _base_log_prob(z, dtype) - dtype(-logdet(sd))


def rot6d_prohmr(x6d):
    """utils/geometry.py:56-66 with rot6d_mode='prohmr' in float64: x [n,6] -> R [n,3,3], a1 = x[0:3], a2 = x[3:6]."""
    x = np.asarray(x6d, np.float64).reshape(-1, 6)
    a1, a2 = x[:, 0:3], x[:, 3:6]
    b1 = a1 / np.maximum(np.linalg.norm(a1, axis=1, keepdims=True), 1e-12)
    u = a2 - (b1 * a2).sum(1, keepdims=True) * b1
    b2 = u / np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-12)
    return np.stack([b1, b2, np.cross(b1, b2)], -1)


# --------------------------------------------------------------------------------------------- one GEMM of the chain (ehm_flow_gemm)
def flow_gemm(X, W, bias=None, gather=None, prologue="none", pro_scale=None, pro_shift=None, epilogue="bias", item=None, scatter=None, Y=None, S=1,
              dtype=np.float64):
    """ehm_flow_gemm restated on the R rows of X, in `dtype`: returns the new Y.  W [K,N]; S rows per item."""
    f = lambda a: np.asarray(a, dtype)
    X = f(X)
    A = X[:, np.asarray(gather)] if gather is not None else X[:, :W.shape[0]]
    if prologue == "relu":
        A = np.maximum(A, 0)
    elif prologue == "bn_relu":
        A = np.maximum(f(pro_scale) * A + f(pro_shift), 0)
    elif prologue == "shift":
        A = A - f(pro_shift)
    v = A @ f(W)
    if bias is not None:
        v = v + f(bias)
    it = np.arange(X.shape[0]) // S
    if epilogue == "bias":
        return v
    if epilogue == "item_add":
        return v + f(item)[it]
    Y = np.array(Y, dtype)
    if epilogue == "glu_res":
        return Y + v * (1 / (1 + np.exp(-f(item)[it])))
    Y[:, np.asarray(scatter)] += v if epilogue == "scatter_add" else -v
    return Y
