"""float64 numpy restatement of the data-parallel BatchNorm merge (csrc/common.h merge_moments; the *_stats_merge / *_bwd_merge entries of
csrc/gcn_train.hip and csrc/bn2d_train.hip), shared by tests/test_data_parallel_cpu.py and tests/test_gpu_bn_sync.py."""
import numpy as np


def local_stats(z):
    """A rank's own (mean, M2 = sum of squares centred on that mean) of its rows z [R_r, C], two-pass in float64: [2, C]."""
    z = np.asarray(z, dtype=np.float64)
    mu = z.sum(0) / z.shape[0]
    return np.stack([mu, ((z - mu) ** 2).sum(0)])


def merge_stats(gathered, rows):
    """gathered [world, 2, C], rows [world] -> (mean, biased var, R) of all rows, in rank order as the kernel adds them:
    R = sum R_r,  mu = mu_0 + sum R_r (mu_r - mu_0) / R,  M2 = sum M2_r + sum R_r (mu_r - mu)^2,  var = M2 / R."""
    g, rows = np.asarray(gathered, dtype=np.float64), [float(r) for r in rows]
    R = sum(rows)
    d = np.zeros(g.shape[2])
    for k in range(1, len(rows)):
        d = d + rows[k] * (g[k, 0] - g[0, 0])
    mu = g[0, 0] + d / R
    s, c = np.zeros(g.shape[2]), np.zeros(g.shape[2])
    for k in range(len(rows)):
        s = s + g[k, 1]
        c = c + rows[k] * (g[k, 0] - mu) ** 2
    return mu, (s + c) / R, R


def running_update(rm, rv, mean, var, R, momentum):
    """nn.BatchNorm's update with the GLOBAL row count: the variance unbiased by R / (R - 1)."""
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * var * R / (R - 1)


def bn_backward(G, z, gamma, eps):
    """float64 whole-batch BatchNorm backward on rows: G, z [R, C] -> (zbar, betabar, gammabar)."""
    G, z, gamma = (np.asarray(a, dtype=np.float64) for a in (G, z, gamma))
    R = z.shape[0]
    mu = z.mean(0)
    invstd = 1.0 / np.sqrt(z.var(0) + eps)
    xh = (z - mu) * invstd
    gb, gg = G.sum(0), (G * xh).sum(0)
    return gamma * invstd * (G - gb / R - xh * gg / R), gb, gg
