"""The rendering rule of include/egohmr_hip.h (ehm_render) restated in numpy: a loop over the faces, vectorised over the pixels of each face's padded
bounding box.  float64 is the reference of tests/test_render_cpu.py and tests/test_gpu_render.py; the same code in float32 (`dtype=np.float32`) is
the yardstick of what float32 arithmetic loses against it.  Beside the three outputs it returns two per-pixel ambiguity margins:

  edge_margin   the smallest |edge function| / edge length, in px, over the faces whose padded bounding box contains the sample: how far the
                sample is from an edge line that decides coverage
  depth_gap     (second nearest - nearest) / nearest covering depth (inf with fewer than two covering faces)

A pixel is AMBIGUOUS when edge_margin < EDGE_TOL (1e-3 px) or depth_gap < DEPTH_TOL (1e-4): float32 may then legitimately choose another face.  The
exact comparisons leave such pixels out, and test_render_cpu.py asserts on this reference alone that they are at most MAX_AMBIGUOUS (6 %) of the
covered pixels of every case, so no case can hide a failure behind them.

The module also builds the meshes and cameras of the cases both test files use.  Pure numpy, no GPU, no package import."""
import math

import numpy as np

EDGE_TOL, DEPTH_TOL, MAX_AMBIGUOUS = 1e-3, 1e-4, 0.06
BASE_COLOR = (1.0, 193.0 / 255.0, 193.0 / 255.0)
DEFAULTS = dict(z_near=0.05, smooth=True, two_sided=False, cull_backface=False, base_color=BASE_COLOR, vertex_colors=None, ambient=0.3,
                diffuse=4.0 / math.pi, light_dir=(0.0, 0.0, -1.0))


def _edges(u, v, px, py):
    """u, v: three arrays (the projected vertices, broadcastable against px, py) -> e0, e1, e2 as the header writes them."""
    e0 = (u[1] - u[0]) * (py - v[0]) - (v[1] - v[0]) * (px - u[0])
    e1 = (u[2] - u[1]) * (py - v[1]) - (v[2] - v[1]) * (px - u[1])
    e2 = (u[0] - u[2]) * (py - v[2]) - (v[0] - v[2]) * (px - u[2])
    return e0, e1, e2


def vertex_normals(verts, faces):
    """Sum of the un-normalised face cross products per vertex (faces with a non-finite cross product add nothing)."""
    p0, p1, p2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.cross(p1 - p0, p2 - p0).astype(verts.dtype)
    c[~np.isfinite(c).all(1)] = 0
    vn = np.zeros_like(verts)
    for k in range(3):
        np.add.at(vn, faces[:, k], c)
    return vn


def render_ref(vertices, faces, fx, fy, cx, cy, H, W, background=None, bg_color=(0, 0, 0), dtype=np.float64, **opt):
    """One item.  vertices [V,3] (camera frame), faces int [F,3]; background uint8 [H,W,3] or None (bg_color).
    -> dict(color uint8 [H,W,3], depth [H,W] (0 on background), face_index int32 [H,W] (-1), edge_margin, depth_gap, ambiguous bool [H,W])."""
    o = dict(DEFAULTS)
    o.update(opt)
    T = dtype
    verts = np.asarray(vertices).astype(T)
    faces = np.asarray(faces).astype(np.int64)
    fx, fy, cx, cy, z_near = T(fx), T(fy), T(cx), T(cy), T(o["z_near"])
    half = T(0.5)
    with np.errstate(all="ignore"):
        x, y, z = verts[:, 0], verts[:, 1], verts[:, 2]
        U = fx * x / z + cx
        Vv = fy * y / z + cy
        ok = np.isfinite(verts).all(1) & (z > z_near) & np.isfinite(U) & np.isfinite(Vv)
    best_z = np.full((H, W), np.inf, T)
    second_z = np.full((H, W), np.inf, T)
    best_i = np.full((H, W), -1, np.int32)
    margin = np.full((H, W), np.inf, T)
    for f, (i0, i1, i2) in enumerate(faces):
        if not (ok[i0] and ok[i1] and ok[i2]):
            continue
        u, v = (U[i0], U[i1], U[i2]), (Vv[i0], Vv[i1], Vv[i2])
        area = (u[1] - u[0]) * (v[2] - v[0]) - (v[1] - v[0]) * (u[2] - u[0])
        if not np.isfinite(area) or area == 0 or (o["cull_backface"] and area > 0):
            continue
        # the samples (j + 0.5, i + 0.5) inside the bounding box padded by a pixel
        j0, j1 = max(int(math.floor(min(u) - 0.5)) - 1, 0), min(int(math.ceil(max(u) - 0.5)) + 1, W - 1)
        r0, r1 = max(int(math.floor(min(v) - 0.5)) - 1, 0), min(int(math.ceil(max(v) - 0.5)) + 1, H - 1)
        if j0 > j1 or r0 > r1:
            continue
        px = (np.arange(j0, j1 + 1).astype(T) + half)[None, :]
        py = (np.arange(r0, r1 + 1).astype(T) + half)[:, None]
        e0, e1, e2 = _edges(u, v, px, py)
        lens = [T(math.hypot(float(u[(k + 1) % 3] - u[k]), float(v[(k + 1) % 3] - v[k]))) for k in range(3)]
        win = (slice(r0, r1 + 1), slice(j0, j1 + 1))
        with np.errstate(all="ignore"):
            m = np.minimum(np.minimum(np.abs(e0) / lens[0], np.abs(e1) / lens[1]), np.abs(e2) / lens[2])
        margin[win] = np.fmin(margin[win], m)
        s = e0 + e1 + e2
        cov = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) if area > 0 else ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
        cov &= s != 0
        if not cov.any():
            continue
        with np.errstate(all="ignore"):
            iz = e1 / s / verts[i0, 2] + e2 / s / verts[i1, 2] + e0 / s / verts[i2, 2]
            zz = np.where(cov, 1 / iz, np.inf).astype(T)
        bz, sz, bi = best_z[win], second_z[win], best_i[win]
        nearer = zz < bz                                   # faces come in index order: a tie keeps the lower index
        sz_new = np.where(nearer, bz, np.minimum(sz, zz))
        second_z[win] = sz_new
        best_i[win] = np.where(nearer, f, bi)
        best_z[win] = np.where(nearer, zz, bz)
    covered = best_i >= 0
    with np.errstate(all="ignore"):
        gap = np.where(np.isfinite(second_z), (second_z - best_z) / best_z, np.inf)
    gap = np.where(covered, gap, np.inf)
    ambiguous = (margin < EDGE_TOL) | (gap < DEPTH_TOL)
    # ---- the winners' colours
    color = np.empty((H, W, 3), np.uint8)
    color[:] = np.asarray(bg_color, np.uint8) if background is None else background
    if covered.any():
        ii, jj = np.nonzero(covered)
        fw = faces[best_i[ii, jj]]
        u = [U[fw[:, k]] for k in range(3)]
        v = [Vv[fw[:, k]] for k in range(3)]
        e0, e1, e2 = _edges(u, v, jj.astype(T) + half, ii.astype(T) + half)
        s = e0 + e1 + e2
        w = [e1 / s / verts[fw[:, 0], 2], e2 / s / verts[fw[:, 1], 2], e0 / s / verts[fw[:, 2], 2]]      # b_k / z_k
        if o["smooth"]:
            vn = vertex_normals(verts, faces)
            n = sum(w[k][:, None] * vn[fw[:, k]] for k in range(3))
        else:
            p0, p1, p2 = verts[fw[:, 0]], verts[fw[:, 1]], verts[fw[:, 2]]
            n = np.cross(p1 - p0, p2 - p0).astype(T)
        ln = np.sqrt((n * n).sum(1))
        l = np.asarray(o["light_dir"], T)
        with np.errstate(all="ignore"):
            ndl = np.where((ln > 0) & np.isfinite(ln), (n * l).sum(1) / ln, 0)
        ndl = np.abs(ndl) if o["two_sided"] else np.maximum(ndl, 0)
        light = T(o["ambient"]) + T(o["diffuse"]) * ndl
        if o["vertex_colors"] is not None:
            vc = np.asarray(o["vertex_colors"]).astype(T)
            base = sum(w[k][:, None] * vc[fw[:, k]] for k in range(3)) / (w[0] + w[1] + w[2])[:, None]
        else:
            base = np.asarray(o["base_color"], T)[None, :]
        c = np.clip(base * light[:, None], 0, 1)
        color[ii, jj] = np.floor(T(255) * c + half).astype(np.uint8)
    return dict(color=color, depth=np.where(covered, best_z, 0).astype(T), face_index=best_i, edge_margin=margin, depth_gap=gap,
                ambiguous=ambiguous, covered=covered)


# ------------------------------------------------------------------------------------------------------------------------ meshes
def rotation(ax, ay):
    """Rotation about x by ax, then about y by ay (radians)."""
    ca, sa, cb, sb = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay)
    rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    return ry @ rx


def uv_sphere(stacks, slices, radius=1.0, tilt=(0.4, 0.3)):
    """A closed UV sphere about the origin, its poles single vertices: 2 * slices * (stacks - 1) faces, wound so that the cross product
    (p1 - p0) x (p2 - p0) points outwards; tilted so that no edge is axis-aligned.  -> (float32 [V,3], int32 [F,3])."""
    verts = [(0.0, 0.0, 1.0)]
    for i in range(1, stacks):
        th = math.pi * i / stacks
        for j in range(slices):
            ph = 2 * math.pi * j / slices
            verts.append((math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)))
    verts.append((0.0, 0.0, -1.0))
    ring = lambda i, j: 1 + (i - 1) * slices + j % slices
    faces = []
    for j in range(slices):
        faces.append((0, ring(1, j), ring(1, j + 1)))
        faces.append((len(verts) - 1, ring(stacks - 1, j + 1), ring(stacks - 1, j)))
    for i in range(1, stacks - 1):
        for j in range(slices):
            faces.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            faces.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    v = np.asarray(verts) @ rotation(*tilt).T * radius
    f = np.asarray(faces, np.int32)
    vol = np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum()
    if vol < 0:
        f = f[:, ::-1].copy()
    return v.astype(np.float32), f


def triangle_soup(n, seed, extent=(1.6, 1.1), depth=(1.5, 4.0), size=0.35):
    """n random triangles in front of the camera, overlapping in the image and in depth, of either orientation.  -> (float32 [3n,3], int32 [n,3])."""
    g = np.random.Generator(np.random.PCG64(seed))
    c = np.stack([g.uniform(-extent[0], extent[0], n), g.uniform(-extent[1], extent[1], n), g.uniform(depth[0], depth[1], n)], 1)
    v = c[:, None, :] + g.uniform(-size, size, (n, 3, 3))
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def _case(vertices, faces, fx, fy, cx, cy, H, W):
    f32 = lambda a: np.asarray(a, np.float32)
    return dict(vertices=f32(vertices), faces=np.asarray(faces, np.int32), fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy), H=H, W=W)


def case_sphere168():
    """Sphere, 168 faces, 64 x 48, three items with their own cameras: centred; partly outside the image; wholly behind the near plane."""
    v, f = uv_sphere(8, 12, radius=0.6)
    t = np.array([[0.05, -0.03, 2.5], [0.95, 0.4, 2.2], [0.0, 0.0, -1.0]])
    return _case(v[None] + t[:, None, :], f, [60.0, 66.5, 60.0], [60.0, 63.25, 60.0], [31.7, 30.2, 32.0], [24.3, 22.9, 24.0], 48, 64)


def case_sphere1472():
    """Sphere, 1472 faces, 160 x 120 (many tiles), plus a copy pushed far away whose faces are smaller than a pixel."""
    v, f = uv_sphere(24, 32, radius=0.9)
    far = v * 0.5 + np.array([28.0, -20.0, 60.0], np.float32)
    verts = np.concatenate([v + np.array([0.1, 0.05, 2.6], np.float32), far], 0)
    return _case(verts[None], np.concatenate([f, f + len(v)], 0), [150.0], [150.0], [80.3], [60.6], 120, 160)


def case_soup(n=2000, seed=5):
    """Triangle soup, 96 x 64: long lists per tile, several LDS chunks, high depth complexity."""
    v, f = triangle_soup(n, seed)
    return _case(v[None], f, [40.0], [40.0], [48.2], [31.6], 64, 96)


def render_case(case, dtype=np.float64, **opt):
    """render_ref of every item of a case -> list of its dicts."""
    return [render_ref(case["vertices"][b], case["faces"], case["fx"][b], case["fy"][b], case["cx"][b], case["cy"][b], case["H"], case["W"],
                       dtype=dtype, **opt) for b in range(case["vertices"].shape[0])]


def ambiguous_share(results):
    """Ambiguous pixels as a share of the pixels the reference covers, over the items of a case."""
    amb = sum(int(r["ambiguous"].sum()) for r in results)
    return amb / max(sum(int(r["covered"].sum()) for r in results), 1)
