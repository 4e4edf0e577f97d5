"""Oracle: the build-defined collision proxy (CPU, autograd).  Test infrastructure only.

NOT a restatement of reference code.  The reference calls ``smpl.coap.collision_loss`` (COAP,
models/egohmr/egohmr.py:555) or ``smpl.volume.collision_loss`` (VolumetricSMPL,
models/egohmr/egohmr_volsmpl.py:612): learned occupancy / SDF networks whose code and weights are
not in /root/reference and cannot be fetched offline - PARITY UNPINNED at that boundary.  The
north-star names a "scene-point Chamfer/SDF guidance reduction"; this proxy is its definition here:

    d_p   = min_v || p - v ||           (scene point p already bbox-selected; v body vertices)
    loss  = sum_p  relu(tau - d_p)^2    (tau = 5 cm: scene points nearer than tau count as contact)

The gradient flows to the arg-min vertex only, like ``torch.min``.
"""
from __future__ import annotations

import torch

TAU = 0.05


def proxy_collision_loss(points, verts, joints=None, full_pose_aa=None, tau: float = TAU):
    """points [1,n,3], verts [1,V,3] -> scalar."""
    p = points[0]
    v = verts[0]
    total = torch.zeros((), dtype=v.dtype)
    for s in range(0, p.shape[0], 1024):
        diff = p[s:s + 1024, None, :] - v[None, :, :]
        d2 = (diff * diff).sum(-1)
        d2min, _ = d2.min(dim=1)
        d = torch.sqrt(d2min + 1e-12)
        total = total + (torch.relu(tau - d) ** 2).sum()
    return total


def proxy_min_dist(points, verts):
    """points [n,3], verts [V,3] -> distance of every point to its nearest vertex (same epsilon as the loss)."""
    out = []
    for s in range(0, points.shape[0], 1024):
        diff = points[s:s + 1024, None, :] - verts[None, :, :]
        out.append(torch.sqrt((diff * diff).sum(-1).min(dim=1).values + 1e-12))
    return torch.cat(out) if out else points.new_zeros(0)


def proxy_collision_loss_batched(points, verts, tau: float = TAU):
    """The VolSMPL-shaped call `volume.collision_loss(points [B,N,3], smpl_output) -> [B]` (models/egohmr/egohmr_volsmpl.py:609-612):
    every scene point of every item, no bounding-box selection."""
    return torch.stack([proxy_collision_loss(points[[b]], verts[[b]], tau=tau) for b in range(points.shape[0])])


def proxy_occupancy(points, verts, tau: float = TAU):
    """Stand-in for `coap.query(points [1,n,3], smpl_output) -> occupancy [1,n]` (egohmr.py:509, `> 0.5` = inside):
    1 where the point is closer than tau to the surface, else 0."""
    return (proxy_min_dist(points[0], verts[0]) < tau).to(verts.dtype).unsqueeze(0)


def proxy_sdf(points, verts, tau: float = TAU):
    """Stand-in for `volume.query_fast(points [1,n,3], smpl_output) -> sdf [1,n]` (egohmr_volsmpl.py:574, `< 0` = inside)."""
    return (proxy_min_dist(points[0], verts[0]) - tau).unsqueeze(0)


def exact_proxy(verts, scene, tau: float = TAU, all_points: bool = False, chunk: int | None = None):
    """The proxy of a batch in float64, by brute force over every vertex, on whatever device the inputs are: the reference for the
    native search (ehm_collision_query).  verts [B,V,3], scene [B,N,3] (float32 or float64; computed in float64 from exactly these values).

    all_points=False selects the scene points inside the vertex bounding box, faces included (egohmr.py:550-552); True takes every point
    (egohmr_volsmpl.py:609-612).  The nearest vertex of a point is the lowest-index one among equally near vertices, like torch.min.
    Returns a dict of float64 / int64 tensors:
      loss [B], gverts [B,V,3] (d loss / d verts), hits [B] (selected points with d < tau),
      selected [B,N] bool, d [B,N] (sqrt(min d2 + 1e-12)), nearest [B,N] (vertex index), gap [B,N] (second-nearest minus nearest
      squared distance, where vertices at the very position of the nearest one do not count as second: exact duplicates tie on purpose),
      ncontrib [B,V] (hit points whose nearest vertex is v), gabs [B,V,3] (sum of |d loss_p / d v| over those points)."""
    v64, p64 = verts.double(), scene.double()
    B, V, N = v64.shape[0], v64.shape[1], p64.shape[1]
    tau = float(tau)
    chunk = chunk or max(1, (1 << 24) // (B * V))                            # ~0.4 GB of float64 differences per step
    if all_points:
        selected = torch.ones(B, N, dtype=torch.bool, device=p64.device)
    else:
        lo, hi = v64.min(1, keepdim=True).values, v64.max(1, keepdim=True).values
        selected = ((p64 >= lo) & (p64 <= hi)).all(-1)
    d = torch.empty(B, N, dtype=torch.float64, device=p64.device)
    nearest = torch.empty(B, N, dtype=torch.long, device=p64.device)
    gap = torch.empty(B, N, dtype=torch.float64, device=p64.device)
    for s in range(0, N, chunk):
        diff = p64[:, s:s + chunk, None, :] - v64[:, None, :, :]
        d2 = (diff * diff).sum(-1)                                             # [B,c,V]
        bi = torch.argmin(d2, -1)                                              # the first minimum (documented for argmin)
        best = torch.gather(d2, -1, bi.unsqueeze(-1)).squeeze(-1)
        bv = torch.gather(v64, 1, bi.unsqueeze(-1).expand(-1, -1, 3))          # [B,c,3]
        same = (v64[:, None, :, :] == bv[:, :, None, :]).all(-1)               # exact duplicates of the nearest vertex
        second = torch.where(same, torch.full_like(d2, float("inf")), d2).min(-1).values
        d[:, s:s + chunk] = torch.sqrt(best + 1e-12)
        nearest[:, s:s + chunk] = bi
        gap[:, s:s + chunk] = second - best
    h = torch.where(selected, tau - d, torch.zeros_like(d))
    hit = h > 0
    hz = torch.where(hit, h, torch.zeros_like(h))
    loss = (hz * hz).sum(1)
    bv = torch.gather(v64, 1, nearest.unsqueeze(-1).expand(-1, -1, 3))
    c = (2.0 * hz / d).unsqueeze(-1) * (p64 - bv)                              # d (tau - d)^2 / d v = 2 h (p - v) / d
    gverts = torch.zeros(B, V, 3, dtype=torch.float64, device=p64.device)
    gabs = torch.zeros_like(gverts)
    idx = nearest.unsqueeze(-1).expand(-1, -1, 3)
    gverts.scatter_add_(1, idx, c)
    gabs.scatter_add_(1, idx, c.abs())
    ncontrib = torch.zeros(B, V, dtype=torch.float64, device=p64.device).scatter_add_(1, nearest, hit.double())
    return dict(loss=loss, gverts=gverts, hits=hit.sum(1), selected=selected, d=d, nearest=nearest, gap=gap, ncontrib=ncontrib, gabs=gabs)
