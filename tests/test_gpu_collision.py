"""GPU (MI355X): the collision-guidance kernels of csrc/guidance.hip against float64 references computed on the device (or, for the body
model, on the CPU) from exactly the float32 inputs the kernels received.

  1. the nearest-vertex search (ehm_collision_query: bbox_kernel, select_kernel, nearest_grid_kernel / nearest_kernel) against
     oracle.collision.exact_proxy, a float64 brute force over every vertex;
  2. the skinning / rot6d VJP (ehm_smpl_backward_rot6d) against float64 autograd through oracle.smpl.SMPLOracle;
  3. the guidance gradient as ehm_sample_loop computes it (ehm_guidance_impl, matrix-core vposed route from B = 24 on) against float64
     autograd of oracle.model.EgoHMROracle.guide_coll's restatement, and against the generic route's four calls;
  4. the rot6d VJP at its clamp threshold |a1| = eps or |u| = eps, eps = float32(1e-12), against float32 CPU autograd (F.normalize,
     the reference's semantics) and float64 autograd with the float32 threshold.  (float32(1e-12) < 1e-12: a float64 restatement with a
     Python-float threshold would take the clamped branch at the tie and hide the difference.)

Error model (u = 2^-24):
  * search.  A float32 squared distance is off by at most 6u d2 (three rounded differences, three squares, two sums), so d by at most
    about 5u d after the sqrt.  Two vertices can therefore swap their order only when their squared distances lie within 6u of each
    other, and a point can flip between hit and miss only when |d - tau| is a few u tau.  The fixtures move every point that the float64
    reference finds within 2^-16 (relative) of such an edge far away from the body (2^-16 is ~40 times the 6u above), assert that
    enough points are left, and then require hits to match exactly and every vertex that no hit point chose to keep an exact zero
    gradient.  Exact ties (bit-identical duplicate vertices) are kept on purpose: the float32 distances tie exactly too, and the gradient
    must go to the lower index.
      loss: per hit point h = tau - d is off by at most 7u tau, h^2 by 14u tau h + u h^2; the float sums (lane, wave, block, atomics)
            chain at most L = ceil(count / 16) + 32 + ceil(N / 1024) additions:   bound = 16u tau sum(h) + (L + 1) u sum(h^2).
      gverts: one contribution 2h (p - v) / d is off by at most 28u tau (|p - v| <= d, h < tau); m contributions meet in atomics:
            bound = 32u tau m + m u sum|contribution|  per vertex and component.
  * skinning / rot6d VJP.  The chain VJP runs through 24 joints, a 20670-term pose-blend contraction and Gram-Schmidt with cancellation
    in every stage; a rigorous element-wise bound is not practical.  The bound is relative to a named float64 scale, the largest
    |d/dpose6d| of the body: |err| <= 2^-12 max_b|ref|.  (test_gpu_guidance.py keeps its looser 2e-4 of the batch maximum plus 2e-3 relative.)
    Bodies without an incoming gradient must come out exactly zero, whatever else shares their tile.
  * guidance gradient.  Here the kernels pose the body themselves: their float32 vertices differ from the float64 body by dv ~ 1e-6 m,
    so the scene is filtered against the float64 body with an absolute slack of SLACK = 1e-4 m on the tie, hinge and bounding-box
    edges instead (the test asserts dv < SLACK / 8).  The hinge term of every hit point then moves by about 2 dv through h = tau - d
    alone, whatever its size, so the gradient carries an error of order dv / h relative to the point's share - ~1e-4 of the body's
    largest entry for ~1000 hit points, close to 2^-12 without any kernel error.  Bound: |err| <= 2^-10 max_b|ref| per item, for
    both routes; items with a zero loss and the zeroed joints must be exactly zero.  The two float32 routes share that vertex error
    and differ only in the skinning VJP's vposed source and the atomics' order: |loop - generic| <= 2^-16 max_b|generic|.
Every test prints its largest error / bound ratio and how many points its filters moved."""
import math
import time

import numpy as np
import pytest
import torch

from egohmr_amd import synthetic as syn

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TAU = float(np.float32(0.05))             # the kernels' float32 tau
EPS32 = float(np.float32(1e-12))          # float32 F.normalize / clamp_min threshold
EDGE = 2.0 ** -16                         # relative width of the tie / hinge edges the fixtures stay away from
SLACK = 1e-4                              # absolute edge width (m) when the body is float64-posed (part 3)
GUIDE_REL = 2.0 ** -10                    # part 3: the same, with the float32 body's own vertex error inside (see the error model)
ROUTES_REL = 2.0 ** -16                   # part 3: sample loop against the generic route (both float32: same body, other vposed / atomics)
VJP_REL = 2.0 ** -12                      # chain-VJP bound relative to the body's largest float64 gradient entry
MAX_CELLS, LDS = 4096, 160 * 1024         # csrc/guidance.hip: kMaxCells, LDS per CU


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def model(dev, synth_weights, smpl_asset):
    from egohmr_amd.factory import build_synthetic_model
    return build_synthetic_model(dev, 0, diffuse_fuse=True, state_dict=synth_weights, smpl_asset=smpl_asset)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ------------------------------------------------------------------------------------------------ part 1: the search
def _uses_grid(V):
    """collision_impl's choice: the in-LDS cell grid (nearest_grid_kernel) or the brute force (nearest_kernel)."""
    Vp = (V + 3) // 4 * 4
    return V <= 8192 and 16 * Vp + (2 * MAX_CELLS + 1) * 4 + 16 <= LDS - 4608


def _slices(cus, B, N):
    """collision_impl: blocks per body of nearest_grid_kernel."""
    return min(max(cus // B, 1), 4, (N + 1023) // 1024)


def _grid(verts_b):
    """nearest_grid_kernel's cell edge h, cell counts and growth iterations for one body (float32, as the kernel)."""
    v = verts_b.numpy().astype(np.float32)
    lo, hi = v.min(0), v.max(0)
    ext = np.maximum(hi - lo, np.float32(1e-6)).astype(np.float32)
    h = np.float32(max(np.float32(TAU), np.cbrt(np.float32(ext[0] * ext[1] * ext[2]) / np.float32(3000.0))))
    it = 0
    while True:
        n = (ext / h).astype(np.int64) + 1
        if int(np.prod(n)) <= MAX_CELLS:
            return float(h), n, it
        h = np.float32(h * np.float32(1.1))
        it += 1


def _smpl_verts(smpl_asset, B, seed, offset=(0.0, 0.0, 0.0)):
    from oracle import geometry as ogeo
    from oracle.smpl import SMPLOracle
    g = _rng(seed)
    x = torch.from_numpy(g.normal(size=(B, 144)).astype(np.float32))
    betas = torch.from_numpy(g.normal(size=(B, 10)).astype(np.float32))
    R = ogeo.rot6d_to_rotmat(x, "diffusion").view(B, 24, 3, 3)
    v = SMPLOracle(smpl_asset)(betas=betas, body_pose=R[:, 1:], global_orient=R[:, [0]]).vertices
    return (v + torch.tensor(offset, dtype=torch.float32)).contiguous()


def _cloud(B, V, ext, seed, flat_axis=None, offset=(0.0, 0.0, 0.0)):
    g = _rng(seed)
    v = g.uniform(-0.5, 0.5, size=(B, V, 3)) * np.asarray(ext) + np.asarray(offset)
    if flat_axis is not None:
        v[..., flat_axis] = offset[flat_axis]
    return torch.from_numpy(v.astype(np.float32))


def _scene(verts, N, seed, near=0.6, noise=0.025, pad=0.15):
    """[B,N,3] float32: a fraction of points around random vertices, the rest uniform in the padded bounding box."""
    g = _rng(seed)
    B, V = verts.shape[:2]
    nn = int(N * near)
    pts = verts[:, g.integers(0, V, size=nn)].double() + torch.from_numpy(g.normal(scale=noise, size=(B, nn, 3)))
    lo, hi = verts.min(1).values.double() - pad, verts.max(1).values.double() + pad
    uni = lo[:, None] + (hi - lo)[:, None] * torch.from_numpy(g.uniform(size=(B, N - nn, 3)))
    return torch.cat([pts, uni], 1).float().contiguous()


def _edges(r, tau, slack=0.0):
    """[B,N] bool: points the float64 reference puts within the float32 error edge (plus an absolute slack) of a nearest-vertex swap or of
    the hinge."""
    d = r["d"]
    best = d * d - 1e-12
    second = best + r["gap"]
    dist_gap = torch.sqrt(second.clamp_min(0)) - torch.sqrt(best.clamp_min(0))
    tie = (r["gap"] <= EDGE * (2 * best + r["gap"])) | (dist_gap <= slack)
    relevant = r["selected"] & (d < tau * (1 + EDGE) + slack)            # a point beyond tau contributes nothing whichever vertex is nearest
    hinge = r["selected"] & ((d - tau).abs() <= EDGE * (tau + d) + slack)
    return (relevant & tie) | hinge


def _filtered(verts, scene, all_points, dev, slack=0.0, ref_verts=None):
    """Move the edge points of `scene` far away (50 m beyond the body's box corner, where they contribute nothing) and return
    (scene, reference on the moved scene, number moved).  With slack > 0 (a float64-posed body: ref_verts) points within slack of a
    bounding-box face move too."""
    from oracle.collision import exact_proxy
    rv = (verts if ref_verts is None else ref_verts).to(dev)
    s = scene.to(dev).clone()
    r = exact_proxy(rv, s, TAU, all_points)
    bad = _edges(r, TAU, slack)
    if slack > 0 and not all_points:
        lo, hi = rv.min(1, keepdim=True).values, rv.max(1, keepdim=True).values
        bad |= (((s.double() - lo).abs() <= slack) | ((s.double() - hi).abs() <= slack)).any(-1)
    far = (rv.max(1).values + 50.0).float()
    s = torch.where(bad.unsqueeze(-1), far.unsqueeze(1).expand_as(s), s).contiguous()
    moved = int(bad.sum())
    if moved:
        r = exact_proxy(rv, s, TAU, all_points)
    return s, r, moved


def _query(verts, scene, all_points):
    from egohmr_amd import _lib
    B, V, N = verts.shape[0], verts.shape[1], scene.shape[1]
    loss = torch.full((B,), 7.0, device=verts.device)
    gverts = torch.full_like(verts, 7.0)
    hits = torch.full((B,), 7, device=verts.device, dtype=torch.int32)
    _lib.api().ehm_collision_query(verts, scene, loss, gverts, hits, B, V, N, TAU, int(all_points), None)
    torch.cuda.synchronize()
    return loss, gverts, hits


def _check_search(tag, verts, scene, r, all_points, moved, min_hits=1):
    dev = verts.device
    loss, gverts, hits = _query(verts.contiguous(), scene.contiguous(), all_points)
    B, N = scene.shape[:2]
    assert int(r["hits"].sum()) >= min_hits, (tag, "too few hit points left after filtering")
    assert torch.equal(hits.long(), r["hits"].to(dev)), (tag, hits.tolist(), r["hits"].tolist())
    h = torch.where(r["selected"] & (r["d"] < TAU), TAU - r["d"], torch.zeros_like(r["d"]))
    cnt = r["selected"].sum(1).double()
    L = torch.ceil(cnt / 16) + 32 + math.ceil(N / 1024)
    lb = 16 * U * TAU * h.sum(1) + (L + 1) * U * (h * h).sum(1) + 1e-30
    el = (loss.double() - r["loss"]).abs()
    m = r["ncontrib"].unsqueeze(-1)
    gb = 32 * U * TAU * m + m * U * r["gabs"] + 1e-30
    eg = (gverts.double() - r["gverts"]).abs()
    assert bool(torch.isfinite(gverts).all())
    zero = (m == 0).expand_as(gverts)
    assert bool((gverts[zero] == 0).all()), (tag, "gradient on a vertex that no hit point chose")
    assert bool((loss[r["loss"] == 0] == 0).all()), (tag, "loss of an item without a hit")
    ratio = max(float((el / lb).max()), float((eg / gb).max()))
    print(f"[search] {tag}: hits {int(r['hits'].sum())}, moved {moved}, max err/bound {ratio:.3g}")
    assert ratio <= 1.0, (tag, ratio)
    return ratio


@pytest.mark.parametrize("all_points", [False, True])
@pytest.mark.parametrize("B,N,want", [(2, 700, 1), (2, 1500, 2), (2, 2500, 3), (2, 4096, 4), (3, 5000, 4), (70, 3000, None)])
def test_search_slices_and_point_counts(dev, cus, smpl_asset, B, N, want, all_points):
    """SMPL bodies (V = 6890, not a multiple of 4: padding vertices), 1 to 4 slices of nearest_grid_kernel, N below / not a multiple of 1024;
    the last item has no scene point anywhere near its body (all_points) or inside its box (bbox): zero loss, hits and gradient."""
    s = _slices(cus, B, N)
    if want is not None:
        assert s == want, (cus, B, N, s)
    else:                                  # the slice count from the CU side: CUs / B
        assert s == min(max(cus // B, 1), 4)
    verts = _smpl_verts(smpl_asset, B, 100 + B)
    scene = _scene(verts, N, 200 + N)
    scene[-1] = verts[-1].max(0).values + 3.0
    scene, r, moved = _filtered(verts, scene, all_points, dev)
    assert float(r["loss"][-1]) == 0.0 and float(r["loss"][:-1].min()) > 0
    _check_search(f"B={B} N={N} slices={s} all_points={all_points}", verts.to(dev), scene, r, all_points, moved, min_hits=100 * (B - 1))


def test_search_selected_count_at_slice_edges(dev, cus, smpl_asset):
    """Exactly 16 * slices selected points (each block of a body gets one point per wave), one fewer and one more, and one item with none."""
    B, N = 4, 2500
    s = _slices(cus, B, N)
    assert s == 3
    verts = _smpl_verts(smpl_asset, B, 31)
    g = _rng(32)
    scene = (verts.max(1).values + 2.0)[:, None].expand(B, N, 3).clone()          # outside every box
    for b, cnt in enumerate((16 * s, 16 * s - 1, 16 * s + 1, 0)):
        if cnt:
            pos = g.choice(N, size=cnt, replace=False)
            pts = verts[b, g.integers(0, 6890, size=cnt)].double() + torch.from_numpy(g.normal(scale=0.01, size=(cnt, 3)))
            lo, hi = verts[b].min(0).values.double(), verts[b].max(0).values.double()
            scene[b, pos] = torch.maximum(torch.minimum(pts, hi), lo).float()
    scene, r, moved = _filtered(verts, scene, False, dev)
    assert moved == 0
    assert r["selected"].sum(1).tolist() == [48, 47, 49, 0]
    _check_search("selected 16*slices, -1, +1, 0", verts.to(dev), scene, r, False, moved, min_hits=100)


@pytest.mark.parametrize("all_points", [False, True])
@pytest.mark.parametrize("V", [6890, 7899, 7900, 7901, 7903])
def test_search_both_kernels_around_the_lds_switch(dev, V, all_points):
    """nearest_grid_kernel up to V = 7900, nearest_kernel (brute force) from 7901 on (collision_impl's LDS formula); V % 4 != 0 puts
    padding vertices in play on both sides."""
    assert _uses_grid(7900) and not _uses_grid(7901)
    verts = _cloud(2, V, (0.5, 1.7, 0.3), seed=V)
    scene = _scene(verts, 3000, seed=V + 1)
    scene, r, moved = _filtered(verts, scene, all_points, dev)
    _check_search(f"V={V} ({'grid' if _uses_grid(V) else 'brute force'}) all_points={all_points}", verts.to(dev), scene, r, all_points, moved,
                  min_hits=500)


@pytest.mark.parametrize("all_points", [False, True])
@pytest.mark.parametrize("shape", ["small", "large", "flat", "flat_large"])
def test_search_grid_shapes(dev, shape, all_points):
    """A body small enough that h = tau, large ones that make the h *= 1.1 growth loop run, and flat ones (zero extent: ext clamped to 1e-6)."""
    ext, flat, off = {"small": ((0.3, 0.25, 0.2), None, (0.4, -0.2, 1.0)), "large": ((6.0, 6.0, 0.15), None, (2.0, 0.0, -1.0)),
                      "flat": ((0.8, 1.0, 0.0), 2, (0.0, 0.0, 0.75)), "flat_large": ((4.0, 4.0, 0.0), 2, (0.0, 1.0, -0.5))}[shape]
    verts = _cloud(2, 5000, ext, seed=7, flat_axis=flat, offset=off)
    h, n, it = _grid(verts[0])
    if shape in ("small", "flat"):
        assert h == TAU and it == 0, (h, it)
    else:
        assert it >= 1, (h, n, it)
    if flat is not None:
        assert float(verts[..., flat].max() - verts[..., flat].min()) == 0.0
    scene = _scene(verts, 4000, seed=8, noise=0.03)
    if flat is not None:                   # two fifths of the points (the ones near vertices) on the plane itself: inside the flat box
        scene[:, : scene.shape[1] * 2 // 5, flat] = verts[0, 0, flat]
    scene, r, moved = _filtered(verts, scene, all_points, dev)
    _check_search(f"{shape} h={h:.4f} cells={n.tolist()} growth={it} all_points={all_points}", verts.to(dev), scene, r, all_points, moved,
                  min_hits=500)


def test_search_points_on_the_selection_boundary(dev, smpl_asset):
    """bbox mode: points exactly on each face of the box (inclusive test); all_points mode (margin tau): points just inside and just
    outside tau beyond each face and each corner.  Both must agree with the reference's selection."""
    B, delta = 2, 1e-3 * TAU
    verts = _smpl_verts(smpl_asset, B, 41)
    g = _rng(42)
    base = _scene(verts, 1200, seed=43)
    extra = []
    for b in range(B):
        v = verts[b].double()
        lo, hi = v.min(0).values, v.max(0).values
        pts = []
        for c in range(3):
            for side, val in ((0, lo[c]), (1, hi[c])):
                e = v[int(v[:, c].argmax() if side else v[:, c].argmin())]          # a vertex on this face
                sign = 1.0 if side else -1.0
                for t in (0.004, 0.012, 0.03):                                      # on the face, off the vertex along the face
                    p = e.clone()
                    p[(c + 1) % 3] += t * (1 if g.uniform() < 0.5 else -1)
                    p = torch.maximum(torch.minimum(p, hi), lo)
                    p[c] = val
                    pts.append(p)
                for dd in (TAU - delta, TAU + delta):                              # beyond the face by tau -+ delta, straight out of the vertex
                    p = e.clone()
                    p[c] = val + sign * dd
                    pts.append(p)
        for corner in range(8):
            sgn = torch.tensor([1.0 if corner >> k & 1 else -1.0 for k in range(3)], dtype=torch.float64)
            cp = torch.where(sgn > 0, hi, lo)
            for dd in (TAU - delta, TAU + delta):
                pts.append(cp + sgn * dd / math.sqrt(3.0))
        extra.append(torch.stack(pts))
    extra = torch.stack(extra).float()
    scene = torch.cat([base, extra], 1)
    ne = extra.shape[1]
    for all_points in (False, True):
        s, r, moved = _filtered(verts, scene, all_points, dev)
        sel = r["selected"][:, -ne:].cpu()
        if not all_points:                 # the face points (three per face) are selected, the ones beyond the faces are not
            face = torch.tensor(([True] * 3 + [False] * 2) * 6 + [False] * 16)
            assert torch.equal(sel, face.expand_as(sel))
            assert int((r["selected"][:, -ne:] & (r["d"][:, -ne:] < TAU)).sum()) >= 12
        else:
            assert bool(sel.all())
            inside = r["d"][:, -ne:][:, torch.tensor(([False] * 3 + [True, False]) * 6 + [False] * 16)]
            assert bool((inside < TAU).all())   # tau - delta out of an extreme vertex: a hit that only the margin-tau selection admits
        _check_search(f"boundary points all_points={all_points}", verts.to(dev), s, r, all_points, moved, min_hits=200)


@pytest.mark.parametrize("V", [2630, 7901])
def test_search_exact_ties_cell_boundaries_and_points_on_vertices(dev, V):
    """Duplicate vertices (exact ties: the gradient goes to the lower index, like torch.min), a cluster of 130 copies of one vertex (every
    lane of a wave sees more than one copy), scene points on cell boundaries (lo + k h) and points equal to a vertex (finite, no gradient
    for that pair).  V = 2630 runs the grid, 7901 the brute force."""
    g = _rng(V)
    n0 = V - 630
    base = _cloud(1, n0, (0.35, 0.3, 0.25), seed=V + 3, offset=(0.1, 0.2, 0.3))[0]
    verts = torch.cat([base, base[7:8].expand(130, 3), base[:500]], 0).unsqueeze(0).contiguous()   # 130 copies of vertex 7, copies of 0..499
    assert verts.shape[1] == V
    h, n, it = _grid(verts[0])
    lo = verts[0].min(0).values
    pts = [verts[0, 7].double() + torch.from_numpy(g.normal(scale=0.003, size=(200, 3))),           # mostly nearest: the 131 copies of vertex 7
           verts[0, g.integers(0, 500, size=400)].double() + torch.from_numpy(g.normal(scale=0.01, size=(400, 3))),
           verts[0, g.integers(0, V, size=50)].double()]                                           # on vertices
    cb = verts[0, g.integers(0, n0, size=300)].double() + torch.from_numpy(g.normal(scale=0.01, size=(300, 3)))
    k = torch.from_numpy(g.integers(1, int(n[0]), size=300))
    cb[:, 0] = (lo[0] + (k.float() * np.float32(h))).double()                                        # x on a cell boundary
    pts.append(cb)
    scene = torch.cat(pts, 0).float().unsqueeze(0)
    scene, r, moved = _filtered(verts, scene, False, dev)
    dup_hits = int(((r["nearest"][0] < 500) & (r["d"][0] < TAU)).sum())
    assert dup_hits >= 200 and int(((r["nearest"][0] == 7) & (r["d"][0] < TAU)).sum()) >= 100
    assert float(r["gverts"][0, n0:].abs().max()) == 0.0        # no gradient on the higher-index copies
    for all_points in (False, True):
        s, rr, mv = _filtered(verts, scene.cpu(), all_points, dev)
        _check_search(f"ties / cell boundaries / on-vertex V={V} ({'grid' if _uses_grid(V) else 'brute force'}) all_points={all_points}",
                      verts.to(dev), s, rr, all_points, moved + mv, min_hits=500)


# ------------------------------------------------------------------------------------------------ part 2: the skinning / rot6d VJP
def _rot6d64(x, mode):
    """rot6d_to_rotmat (utils/geometry.py:59-66) with F.normalize's float32 threshold, for float64 inputs."""
    x = x.reshape(-1, 2, 3).permute(0, 2, 1) if mode == "prohmr" else x.reshape(-1, 3, 2)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    b1 = a1 / a1.norm(dim=1, keepdim=True).clamp_min(EPS32)
    u = a2 - (b1 * a2).sum(dim=1, keepdim=True) * b1
    b2 = u / u.norm(dim=1, keepdim=True).clamp_min(EPS32)
    return torch.stack((b1, b2, torch.linalg.cross(b1, b2, dim=1)), dim=-1)


def _smpl_vjp(dev, handle, asset, x, betas, mean, std, gv):
    """(native ehm_smpl_backward_rot6d [B,144], float64 autograd [B,144]) of sum(gv * verts) w.r.t. the de-normalised 6-D pose."""
    from egohmr_amd import _lib
    from oracle.smpl import SMPLOracle
    B = x.shape[0]
    out = torch.full((B, 144), 7.0, device=dev)
    d = [t.to(dev).contiguous() for t in (betas, x, mean, std, gv)]
    _lib.api().ehm_smpl_backward_rot6d(handle, d[0], d[1], d[2], d[3], d[4], out, B, None)
    torch.cuda.synchronize()
    p6 = (x.double() * std.double() + mean.double()).requires_grad_()
    R = _rot6d64(p6, "diffusion").view(B, 24, 3, 3)
    v = SMPLOracle(asset, torch.float64)(betas=betas.double(), body_pose=R[:, 1:], global_orient=R[:, [0]]).vertices
    (v * gv.double()).sum().backward()
    return out.cpu().double(), p6.grad


def _vjp_ratio(out, ref, skip=None, rel=VJP_REL):
    """max over bodies of max|out - ref| / (rel max|ref|) (entries in `skip` [B,144] bool excluded); bodies with ref == 0 must be exactly 0."""
    err = (out - ref).abs()
    ok = torch.ones_like(ref, dtype=torch.bool) if skip is None else ~skip
    worst = 0.0
    for b in range(ref.shape[0]):
        S = float(ref[b][ok[b]].abs().max())
        if S == 0.0:
            assert float(out[b].abs().max()) == 0.0, b
            continue
        worst = max(worst, float(err[b][ok[b]].max()) / (rel * S))
    return worst


def _hot_gverts(B, seed, V=6890, bodies=None):
    """incoming d loss / d verts: 300 random vertices, every multiple of kVT = 256 and the last three vertices (the partial last 8-k group of the
    pose-blend contraction: 3 V % 8 = 6) hot, in the given bodies (default all)."""
    g = _rng(seed)
    hot = np.unique(np.concatenate([g.integers(0, V, size=300), np.arange(0, V, 256), [V - 3, V - 2, V - 1]]))
    gv = torch.zeros(B, V, 3)
    bodies = range(B) if bodies is None else bodies
    for b in bodies:
        gv[b, hot] = torch.from_numpy(g.normal(size=(len(hot), 3)).astype(np.float32))
    return gv


@pytest.mark.parametrize("B", [1, 8, 9, 31, 32, 33, 65, 257])
def test_smpl_backward_rot6d_vs_fp64(dev, model, smpl_asset, B):
    """One to many 8-body skin_bwd groups and 32-body posefeat_bwd_mfma tiles, ragged ones included."""
    g = _rng(500 + B)
    x = torch.from_numpy(g.normal(size=(B, 144)).astype(np.float32))
    betas = torch.from_numpy(g.normal(size=(B, 10)).astype(np.float32))
    mean, std = (torch.from_numpy(a) for a in syn.make_body_rep_stats(0))
    out, ref = _smpl_vjp(dev, model.smpl.handle(), smpl_asset, x, betas, mean, std, _hot_gverts(B, 600 + B))
    ratio = _vjp_ratio(out, ref)
    print(f"[vjp] B={B}: max err/bound {ratio:.3g}")
    assert ratio <= 1.0


@pytest.mark.parametrize("B,body", [(33, 17), (65, 64), (40, 0)])
def test_smpl_backward_rot6d_no_leak_between_bodies(dev, model, smpl_asset, B, body):
    """Only one body of its skin_bwd group / MFMA tile has an incoming gradient: every other body's gradient is exactly zero."""
    g = _rng(700 + B)
    x = torch.from_numpy(g.normal(size=(B, 144)).astype(np.float32))
    betas = torch.from_numpy(g.normal(size=(B, 10)).astype(np.float32))
    mean, std = (torch.from_numpy(a) for a in syn.make_body_rep_stats(0))
    out, ref = _smpl_vjp(dev, model.smpl.handle(), smpl_asset, x, betas, mean, std, _hot_gverts(B, 800 + B, bodies=[body]))
    others = torch.arange(B) != body
    assert float(out[others].abs().max()) == 0.0
    assert float(out[body].abs().max()) > 0
    ratio = _vjp_ratio(out, ref)
    print(f"[vjp] leak B={B} body={body}: max err/bound {ratio:.3g}")
    assert ratio <= 1.0


def _dense_asset(smpl_asset):
    """tests/test_gpu_edges.py's body model: a third of the vertices carry six skinning weights (no matrix-core skinning fragments)."""
    asset = dict(smpl_asset)
    g = _rng(77)
    w = np.array(asset["lbs_weights"], dtype=np.float64).copy()
    for v in g.choice(w.shape[0], size=w.shape[0] // 3, replace=False):
        js = g.choice(w.shape[1], size=6, replace=False)
        w[v] = 0.0
        w[v, js] = g.uniform(0.05, 1.0, size=6)
        w[v] /= w[v].sum()
    asset["lbs_weights"] = w.astype(np.float32)
    return asset


@pytest.fixture(scope="module")
def dense_model(dev, synth_weights, smpl_asset):
    from egohmr_amd.factory import build_synthetic_model
    asset = _dense_asset(smpl_asset)
    return build_synthetic_model(dev, 0, diffuse_fuse=True, state_dict=synth_weights, smpl_asset=asset), asset


@pytest.mark.parametrize("B", [9, 33])
def test_smpl_backward_rot6d_dense_skinning_weights(dev, dense_model, B):
    m, asset = dense_model
    g = _rng(900 + B)
    x = torch.from_numpy(g.normal(size=(B, 144)).astype(np.float32))
    betas = torch.from_numpy(g.normal(size=(B, 10)).astype(np.float32))
    mean, std = (torch.from_numpy(a) for a in syn.make_body_rep_stats(0))
    out, ref = _smpl_vjp(dev, m.smpl.handle(), asset, x, betas, mean, std, _hot_gverts(B, 910 + B))
    ratio = _vjp_ratio(out, ref)
    print(f"[vjp] dense weights B={B}: max err/bound {ratio:.3g}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ part 4: the rot6d clamp threshold
def _rot6d_rows():
    """(a1, a2) pairs at and around the clamp threshold, exact zeros and exactly parallel pairs.  The kernel's sqrtf is the correctly rounded
    expansion (v_sqrt_f32 plus a one-ulp correction from fma residuals), so sqrtf(e * e) == e for these e, and |a1| or |u| lands exactly on
    the threshold."""
    e = np.float32(1e-12)
    below, above = np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(1))
    a2 = (0.3, -0.8, 0.2)
    rows = []
    for t in (e, below, above):
        rows += [((t, 0, 0), a2), ((0, t, 0), a2), ((0, 0, -t), (0.1, 0.9, -0.4))]    # |a1| at / one ulp below / one ulp above eps
        rows += [((1, 0, 0), (5, t, 0)), ((0, 1, 0), (0, -2, t)), ((0, 0, 2), (-t, 0, 3))]   # |u| = t exactly (u = a2 - (b1.a2) b1)
    rows += [((0, 0, 0), a2), ((0, 0, 0), (0, 0, 0)), ((0.3, 0.4, 0.5), (0, 0, 0)),        # exact zeros
             ((1, 0, 0), (3, 0, 0)), ((0, 2, 0), (0, -1, 0)), ((0, 0, 4), (0, 0, 4))]       # exactly parallel: u == 0
    return np.array([[*a, *b] for a, b in rows], dtype=np.float32)


def _pack6(a, mode):
    """[n,6] (a1 | a2) -> the 6-D layout of `mode` (prohmr: a1 then a2; diffusion: interleaved)."""
    if mode == "prohmr":
        return a.copy()
    return np.stack([a[:, 0], a[:, 3], a[:, 1], a[:, 4], a[:, 2], a[:, 5]], 1)


def test_rot6d_backward_at_the_clamp_threshold(dev):
    from egohmr_amd import _lib
    from oracle import geometry as ogeo
    a = _rot6d_rows()
    e = np.float32(1e-12)
    assert float(torch.tensor([float(e), 0.0, 0.0]).norm()) == float(e)           # float32 CPU torch sees |a1| == eps too
    g = _rng(5)
    gR = g.normal(size=(2 * len(a), 3, 3)).astype(np.float32)
    gR[: len(a)] = 0.0
    gR[: len(a), :, 0] = (0.3, 0.5, 0.7)                                           # gradient on b1 alone
    a = np.concatenate([a, a])
    worst = 0.0
    for mode in ("prohmr", "diffusion"):
        x = torch.from_numpy(_pack6(a, mode))
        gx = torch.full_like(x, 7.0).to(dev)
        _lib.api().ehm_rot6d_to_rotmat_bwd(x.to(dev), torch.from_numpy(gR).to(dev).contiguous(), gx, x.shape[0], {"prohmr": 0, "diffusion": 1}[mode], None)
        torch.cuda.synchronize()
        gx = gx.cpu().double()
        x32 = x.clone().requires_grad_()
        (ogeo.rot6d_to_rotmat(x32, mode) * torch.from_numpy(gR)).sum().backward()
        x64 = x.double().requires_grad_()
        (_rot6d64(x64, mode) * torch.from_numpy(gR).double()).sum().backward()
        for name, ref in (("float32 autograd", x32.grad.double()), ("float64 autograd", x64.grad)):
            scale = ref.abs().amax(1, keepdim=True)
            assert bool(torch.isfinite(gx).all())
            r = float(((gx - ref).abs() / (2.0 ** -16 * scale + 1e-30)).max())
            worst = max(worst, r)
            assert r <= 1.0, (mode, name, r)
        # the case of the issue: a1 = (eps, 0, 0), gradient (0.3, 0.5, 0.7) on b1 -> (0, 5e11, 7e11) on a1 (the clamped branch gave 3e11 first)
        ga1 = gx[0, [0, 1, 2]] if mode == "prohmr" else gx[0, [0, 2, 4]]
        assert abs(float(ga1[0])) <= 1e-6 * float(ga1.abs().max()) and abs(float(ga1[1]) / 5e11 - 1) < 1e-5
    print(f"[rot6d] threshold rows: max err/bound {worst:.3g}")


def test_smpl_backward_rot6d_at_the_clamp_threshold(dev, model, smpl_asset):
    """The same tie through the whole VJP (chain_bwd_kernel): mean 0 and std 1, so the kernel's 6-D pose is x itself; body 1 has
    |a1| = eps on joint 5 and |u| = eps on joint 8."""
    B = 2
    g = _rng(1000)
    x = torch.from_numpy(g.normal(size=(B, 144)).astype(np.float32))
    e = float(np.float32(1e-12))
    j5, j8 = x[1, 30:36].view(3, 2), x[1, 48:54].view(3, 2)                      # diffusion layout: a1 = column 0, a2 = column 1
    j5[:, 0] = torch.tensor([e, 0.0, 0.0])
    j8[:, 0] = torch.tensor([1.0, 0.0, 0.0])
    j8[:, 1] = torch.tensor([5.0, e, 0.0])
    betas = torch.from_numpy(g.normal(size=(B, 10)).astype(np.float32))
    mean, std = torch.zeros(144), torch.ones(144)
    out, ref = _smpl_vjp(dev, model.smpl.handle(), smpl_asset, x, betas, mean, std, _hot_gverts(B, 1001))
    special = torch.zeros(B, 144, dtype=torch.bool)
    special[1, 30:36] = special[1, 48:54] = True
    ratio = _vjp_ratio(out, ref, skip=special)
    for sl in (slice(30, 36), slice(48, 54)):
        S = float(ref[1, sl].abs().max())
        assert S > 1e6                                                              # the 1/eps scale of the tie
        ratio = max(ratio, float((out[1, sl] - ref[1, sl]).abs().max()) / (VJP_REL * S))
    print(f"[vjp] clamp threshold through the chain: max err/bound {ratio:.3g}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ part 3: the gradient inside ehm_sample_loop
def _gradient_table():
    """Two ehm_step_coefs rows: step 0 x1 = grad(x_T) (coef1 = coef2 = nonzero = 0, grad_scale = 1), step 1 x2 = x1 (coef2 = 1, grad_scale 0):
    x_final is bit for bit the guidance gradient at x_T (csrc/step_dev.h, the DDPM update)."""
    from egohmr_amd import _lib
    r0, r1 = _lib.StepCoefs(), _lib.StepCoefs()
    r0.grad_scale = 1.0
    r1.coef2 = 1.0
    return (_lib.StepCoefs * 2)(r0, r1), 0


def _guide_ref(x, st, mean, std, asset, scene, reduction, all_points):
    """float64 autograd of EgoHMROracle.guide_coll's restatement with the proxy, at the nearest vertices and selection of the float64 body."""
    from oracle.collision import exact_proxy
    from oracle.model import EgoHMROracle
    from oracle.smpl import SMPLOracle
    B = x.shape[0]
    p6 = (x.double().cpu() * std.double().cpu() + mean.double().cpu()).requires_grad_()
    R = _rot6d64(p6, "diffusion").view(B, 24, 3, 3)
    v = SMPLOracle(asset, torch.float64)(betas=st.betas.double().cpu(), body_pose=R[:, 1:], global_orient=R[:, [0]]).vertices
    r = {k: t.cpu() for k, t in exact_proxy(v.detach().to(x.device), scene.to(x.device), TAU, all_points).items()}
    hit = r["selected"] & (r["d"] < TAU)
    nv = torch.gather(v, 1, r["nearest"].unsqueeze(-1).expand(-1, -1, 3))
    d = torch.sqrt(((scene.cpu().double() - nv) ** 2).sum(-1) + 1e-12)
    loss = torch.where(hit, (TAU - d) ** 2, torch.zeros_like(d)).sum(1)
    red = loss.mean() if reduction == "mean" else loss.sum()
    gr = torch.autograd.grad([-red], [p6])[0].reshape(B, 24, 6).clone()
    gr[:, 3:] *= 2
    gr[:, EgoHMROracle.GRAD_ZERO_JOINTS] = 0
    return gr.reshape(B, 144), loss.detach(), v.detach()


@pytest.mark.parametrize("B", [23, 24, 33, 128])
def test_guidance_gradient_inside_the_sample_loop_vs_fp64(dev, model, smpl_asset, monkeypatch, B):
    """ehm_sample_loop's guidance gradient (B < 24: VALU skinning, recomputed blend; B >= 24: the matrix-core forward's vposed) for both
    reductions and both selections, against float64 autograd and against the generic route (FusedSampler.guidance_gradient)."""
    from egohmr_amd import _lib
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import batch_to_device
    from egohmr_amd.fused import FusedSampler
    fs, N = model.fused_sampler, 2048
    monkeypatch.setattr(FusedSampler, "step_table", staticmethod(lambda *a, **k: _gradient_table()))
    d = create_gaussian_diffusion(num_diffusion_timesteps=2, timestep_respacing="")
    assert d.num_timesteps == 2
    batch = batch_to_device(syn.make_batch(B, N, seed=1100 + B), dev)
    st = fs.prepare(batch)
    noise = torch.from_numpy(syn.make_noise_stack(2, B, seed=1200 + B)).to(dev) * 0.5
    x = noise[0].contiguous()
    mean, std = model._std_mean()
    # the scene: points around the float64-posed body at x_T, filtered against it with SLACK, float32 vertices checked against it
    _, _, v64 = _guide_ref(x, st, mean, std, smpl_asset, torch.zeros(B, 1, 3), "mean", False)
    v32 = torch.empty(B, 6890, 3, device=dev)
    j32 = torch.empty(B, model.smpl.num_joints_out, 3, device=dev)
    _lib.api().ehm_smpl_forward_rot6d(model.smpl.handle(), st.betas, x, mean, std, v32, j32, None, None, None, B, None)
    torch.cuda.synchronize()
    dv = float((v32.cpu().double() - v64).abs().max())
    assert dv < SLACK / 8, dv
    scene0 = _scene(v64.float(), N, seed=1300 + B, near=0.5, noise=0.02)
    scene0[-1] = v64[-1].float().max(0).values + 3.0                    # one item without a collision: zero gradient
    results = []
    t0 = time.time()
    for all_points in (False, True):
        scene, _, moved = _filtered(v64.float(), scene0, all_points, dev, slack=SLACK, ref_verts=v64)
        st.scene = scene.contiguous()
        for reduction in ("mean", "sum"):
            model.guide_all_points, model.guide_reduction = all_points, reduction
            try:
                res = fs.run(d, dict(batch), noise, ddim=False, guided=True, cond_grad_weight=1.0, prepared=st, lowprec=0, trace=True)
                assert torch.equal(fs.last_trace[0], x)
                grad = res["sample"].cpu().double()
                generic = fs.guidance_gradient(st, x, st.betas).cpu().double()
            finally:
                model.guide_all_points, model.guide_reduction = False, "mean"
            ref, loss, _ = _guide_ref(x, st, mean, std, smpl_asset, scene, reduction, all_points)
            assert float(loss[-1]) == 0.0 and int((loss[:-1] > 0).sum()) == B - 1
            zero = torch.zeros(B, 24, dtype=torch.bool)
            zero[:, [0, 3, 6, 9] + list(range(12, 24))] = True
            zero = zero.repeat_interleave(6, 1)
            assert float(grad[zero].abs().max()) == 0.0 and float(grad[-1].abs().max()) == 0.0
            r, rg = _vjp_ratio(grad, ref, rel=GUIDE_REL), _vjp_ratio(generic, ref, rel=GUIDE_REL)
            rr = _vjp_ratio(grad, generic, rel=ROUTES_REL)
            results.append((f"B={B} {reduction} all_points={all_points}", r, rg, rr))
            print(f"[loop] B={B} {reduction} all_points={all_points}: err/bound sample loop {r:.3g}, generic route {rg:.3g}, "
                  f"loop vs generic {rr:.3g}; moved {moved}")
    print(f"[loop] B={B}: {time.time() - t0:.1f} s")
    for tag, r, rg, rr in results:
        assert r <= 1.0 and rg <= 1.0 and rr <= 1.0, (tag, r, rg, rr)
