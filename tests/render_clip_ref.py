"""The near-plane rule of include/egohmr_hip.h (ehm_render with clip_near = 1) restated in numpy, on top of tests/render_ref.py: the faces wholly in
front of the plane are render_ref's (that function is called, not copied), and every CROSSING face - three finite vertices, at least one at
z > z_near and at least one at z <= z_near - is evaluated by the header's homogeneous rule over the whole image, so the reference does not depend
on any binning box.  float64 is the reference; `dtype=np.float32` is the same code in float32, the yardstick of what float32 loses.

render_clip_ref returns what render_ref returns.  Its `ambiguous` mask also marks a pixel where a crossing face that covers it or nearly covers it
(every E_k within EDGE_TOL px of the covered side, z within DEPTH_TOL of the clipped side) has either of
  |z - z_near| / z_near < DEPTH_TOL
  |E_k| / hypot(dE_k/du, dE_k/dv) < EDGE_TOL px for one k
and the depth gap is taken over both kinds of face.  Two more masks say where the rule can change a picture: `crossing_covered` (some crossing face
covers the pixel) and `crossing_near` (covers or nearly covers).

`all_homogeneous=True` applies the homogeneous rule to every face with a vertex in front (the faces wholly in front too) and render_ref to none:
the check of the rule's mathematics against the existing one.

The module also builds the meshes and cameras of the cases tests/test_render_clip_cpu.py and tests/test_gpu_render_clip.py share.  Pure numpy."""
import numpy as np

from tests import render_ref as R

EDGE_TOL, DEPTH_TOL, MAX_AMBIGUOUS = R.EDGE_TOL, R.DEPTH_TOL, R.MAX_AMBIGUOUS


def crossing_faces(vertices, faces, z_near, all_homogeneous=False):
    """-> the indices of the faces the homogeneous rule takes."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    fin = np.isfinite(v).all(1)[f].all(1)
    with np.errstate(invalid="ignore"):
        front = (v[:, 2] > z_near)[f].sum(1)
    take = fin & (front >= 1) & ((front <= 2) | bool(all_homogeneous))
    return np.nonzero(take)[0]


def render_clip_ref(vertices, faces, fx, fy, cx, cy, H, W, background=None, bg_color=(0, 0, 0), dtype=np.float64, all_homogeneous=False, **opt):
    """One item, as render_ref: -> dict(color, depth, face_index, edge_margin, depth_gap, ambiguous, covered, crossing_covered, crossing_near)."""
    o = dict(R.DEFAULTS)
    o.update(opt)
    T = dtype
    verts = np.asarray(vertices).astype(T)
    faces = np.asarray(faces).astype(np.int64)
    fx, fy, cx, cy, z_near = T(fx), T(fy), T(cx), T(cy), T(o["z_near"])
    half = T(0.5)
    if all_homogeneous:
        best_z = np.full((H, W), np.inf, T)
        second_z = np.full((H, W), np.inf, T)
        best_i = np.full((H, W), -1, np.int32)
        margin = np.full((H, W), np.inf, T)
        color = np.empty((H, W, 3), np.uint8)
        color[:] = np.asarray(bg_color, np.uint8) if background is None else background
    else:
        base = R.render_ref(vertices, faces, fx, fy, cx, cy, H, W, background=background, bg_color=bg_color, dtype=dtype, **opt)
        best_z = np.where(base["covered"], base["depth"], np.inf).astype(T)
        with np.errstate(all="ignore"):
            second_z = np.where(np.isfinite(base["depth_gap"]), best_z * (1 + base["depth_gap"]), np.inf).astype(T)
        best_i = base["face_index"].copy()
        margin = base["edge_margin"].copy()
        color = base["color"].copy()
    rx = (np.arange(W).astype(T) + half - cx)[None, :]
    ry = (np.arange(H).astype(T) + half - cy)[:, None]
    coef = {}
    from_cross = np.zeros((H, W), bool)
    cross_cov = np.zeros((H, W), bool)
    cross_near = np.zeros((H, W), bool)
    cross_amb = np.zeros((H, W), bool)
    for f in crossing_faces(verts, faces, float(o["z_near"]), all_homogeneous):
        p = verts[faces[f]]
        with np.errstate(all="ignore"):
            g = [(fx * p[k, 0], fy * p[k, 1], p[k, 2]) for k in range(3)]
            c = []
            for k in range(3):
                a, b = g[(k + 1) % 3], g[(k + 2) % 3]
                c.append((a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]))
            D = (g[0][0] * c[0][0] + g[0][1] * c[0][1]) + g[0][2] * c[0][2]
        if not np.isfinite(D) or D == 0 or (o["cull_backface"] and D > 0):
            continue
        coef[f] = c
        sgn = T(1) if D > 0 else T(-1)
        with np.errstate(all="ignore"):
            E = [(c[k][0] * rx + c[k][1] * ry) + c[k][2] for k in range(3)]
            S = (E[0] + E[1]) + E[2]
            z = (D / S).astype(T)
            cov = (sgn * E[0] >= 0) & (sgn * E[1] >= 0) & (sgn * E[2] >= 0) & (S != 0) & (z > z_near)
            grad = [float(np.hypot(np.float64(c[k][0]), np.float64(c[k][1]))) for k in range(3)]
            m = [np.broadcast_to(sgn * E[k].astype(np.float64) / grad[k] if grad[k] > 0 else np.where(sgn * E[k] >= 0, np.inf, -np.inf), (H, W))
                 for k in range(3)]                                              # signed distance to the edge line, px, positive inside
            mmin = np.minimum(np.minimum(m[0], m[1]), m[2])
            mabs = np.minimum(np.minimum(np.abs(m[0]), np.abs(m[1])), np.abs(m[2]))
            near = (mmin > -EDGE_TOL) & (sgn * S > 0) & (z > z_near * (1 - DEPTH_TOL))
            amb = near & ((mabs < EDGE_TOL) | (np.abs(z - z_near) / z_near < DEPTH_TOL))
        cross_cov |= cov
        cross_near |= near | cov
        cross_amb |= amb
        margin = np.where(near, np.fmin(margin, mabs.astype(T)), margin)
        zz = np.where(cov, z, np.inf).astype(T)
        nearer = (zz < best_z) | ((zz == best_z) & cov & (f < best_i))          # the lexicographic minimum of (z, face index)
        second_z = np.where(nearer, best_z, np.minimum(second_z, zz))
        best_i = np.where(nearer, f, best_i).astype(np.int32)
        best_z = np.where(nearer, zz, best_z)
        from_cross = np.where(nearer, True, from_cross)
    covered = best_i >= 0
    with np.errstate(all="ignore"):
        gap = np.where(np.isfinite(second_z), (second_z - best_z) / best_z, np.inf)
    gap = np.where(covered, gap, np.inf)
    ambiguous = (margin < EDGE_TOL) | (gap < DEPTH_TOL) | cross_amb
    # ---- the colours of the pixels a crossing face wins: the header's weights beta_k = E_k / S, then render_ref's Lambert term
    sel = from_cross & covered
    if sel.any():
        ii, jj = np.nonzero(sel)
        fi = best_i[ii, jj]
        fw = faces[fi]
        C = np.array([coef[f] for f in fi], T)                                   # [n, 3, 3]
        px, py = jj.astype(T) + half - cx, ii.astype(T) + half - cy
        E = [(C[:, k, 0] * px + C[:, k, 1] * py) + C[:, k, 2] for k in range(3)]
        S = (E[0] + E[1]) + E[2]
        w = [E[k] / S for k in range(3)]
        if o["smooth"]:
            vn = R.vertex_normals(verts, faces)
            n = (w[0][:, None] * vn[fw[:, 0]] + w[1][:, None] * vn[fw[:, 1]]) + w[2][:, None] * vn[fw[:, 2]]
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
            basec = (w[0][:, None] * vc[fw[:, 0]] + w[1][:, None] * vc[fw[:, 1]]) + w[2][:, None] * vc[fw[:, 2]]
        else:
            basec = np.asarray(o["base_color"], T)[None, :]
        col = np.clip(basec * light[:, None], 0, 1)
        color[ii, jj] = np.floor(T(255) * col + half).astype(np.uint8)
    return dict(color=color, depth=np.where(covered, best_z, 0).astype(T), face_index=best_i, edge_margin=margin, depth_gap=gap, ambiguous=ambiguous,
                covered=covered, crossing_covered=cross_cov, crossing_near=cross_near)


def render_clip_case(case, dtype=np.float64, **opt):
    """render_clip_ref of every item of a case -> list of its dicts."""
    return [render_clip_ref(case["vertices"][b], case["faces"], case["fx"][b], case["fy"][b], case["cx"][b], case["cy"][b], case["H"], case["W"],
                            dtype=dtype, **opt) for b in range(case["vertices"].shape[0])]


# ------------------------------------------------------------------------------------------------------------------------ cases
FLOOR_Y = 1.2
FLOOR = np.float32([[-4, FLOOR_Y, -2], [4, FLOOR_Y, -2], [4, FLOOR_Y, 8], [-4, FLOOR_Y, 8]])
FLOOR_FACES = np.int32([[0, 1, 2], [0, 2, 3]])               # both triangles reach from z = -2 to z = 8: both cross


def case_floor(H=48, W=64):
    """The floor quad y = 1.2, x in [-4, 4], z in [-2, 8], fx = fy = 60, B = 2 with their own cameras: item 0 stands on it (both faces cross), item 1
    sees it from 2.5 m further back and 0.3 m higher up, wholly in front."""
    v = np.stack([FLOOR, FLOOR + np.float32([0, 0.3, 2.5])], 0)
    return R._case(v, FLOOR_FACES, [60.0, 60.0], [60.0, 60.0], [W / 2 - 0.3, W / 2 + 1.2], [H / 2 - 3.7, H / 2 - 5.1], H, W)


def case_cut_sphere():
    """uv_sphere(168 faces), radius 0.6, about (0.7, 0.2, 0.3): z from -0.3 to 0.9, so the near plane cuts through it; the camera (the origin, 0.79
    from the centre) is outside.  64 x 48."""
    v, f = R.uv_sphere(8, 12, radius=0.6)
    return R._case((v + np.float32([0.7, 0.2, 0.3]))[None], f, [30.0], [30.5], [20.3], [22.6], 48, 64)


def case_inside_sphere():
    """The same sphere about (0.4, 0.05, 0.1): the camera is inside it, close to the wall on its left, where the near plane cuts the faces in view.  A
    ray of slope s = |(x, y)| / z leaves the sphere at z > z_near while s stays under about 2.9 (the cut circle's nearest point, 0.147 away in the
    plane z = 0.05, for the facets' inradius 0.55); fx = 16 keeps the image's corners under 2.5, so every pixel is covered."""
    v, f = R.uv_sphere(8, 12, radius=0.6)
    return R._case((v + np.float32([0.4, 0.05, 0.1]))[None], f, [16.0], [16.5], [31.7], [24.3], 48, 64)


def case_cut_soup(n=300, seed=17):
    """Triangle soup with depths drawn from (-1, 3) and corners up to 1.2 m from the centre: about a third of the faces cross (101 of 300), nearly
    all of those have a vertex at z < 0.  96 x 64."""
    v, f = R.triangle_soup(n, seed, depth=(-1.0, 3.0), size=1.2)
    return R._case(v[None], f, [40.0], [40.0], [48.2], [31.6], 64, 96)


def room_mesh():
    """A closed box of 12 faces around the camera, x in [-2, 2.3], y in [-1.4, 1.2], z in [-1.5, 4], slightly turned so that no edge is axis-aligned.
    -> (float32 [8,3], int32 [12,3], float32 colours [8,3])."""
    lo, hi = np.array([-2.0, -1.4, -1.5]), np.array([2.3, 1.2, 4.0])
    v = np.array([[(lo, hi)[(i >> k) & 1][k] for k in range(3)] for i in range(8)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.int32([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])
    v = v @ R.rotation(0.05, 0.12).T
    g = np.random.Generator(np.random.PCG64(29))
    return v.astype(np.float32), f, g.uniform(0.2, 1.0, size=(8, 3)).astype(np.float32)


def case_room():
    """The room plus a 168-face sphere as the body (radius 0.5 about (0.1, 0.3, 2.4)), as render_in_scene concatenates them: the body first.
    -> (case, number of body vertices, number of body faces, float32 colours [V,3]); 96 x 64."""
    body, bf = R.uv_sphere(8, 12, radius=0.5)
    body = body + np.float32([0.1, 0.3, 2.4])
    room, rf, rc = room_mesh()
    colors = np.concatenate([np.tile(np.float32(R.BASE_COLOR), (len(body), 1)), rc], 0)
    case = R._case(np.concatenate([body, room], 0)[None], np.concatenate([bf, rf + len(body)], 0), [40.0], [41.0], [48.3], [31.2], 64, 96)
    return case, len(body), len(bf), colors
