"""The mesh collision term (include/egohmr_hip.h, "mesh collision term") in NumPy, brute force over (point, face) pairs, for the tests of
csrc/mesh_collision.hip.  dtype = float64 is the reference; dtype = float32 runs the SAME statements in single precision and is the yardstick for
what rounding alone does to the outputs (the kernel's error bar is a multiple of its error, never of the kernel's own).

    selection   bbox of the body's vertices, both ends inclusive, or every point (all_points)
    occupancy   w(p) = sum_f 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) / 4 pi,  inside <=> w > 0.5
    depth       d(p) = min_f dist(p, triangle f) at the closest point c = sum_k beta_k v_k; lowest face index among equally near ones
    degenerate  a face that repeats a vertex index: 0 in w, left out of the minimum
    outputs     loss = sum_{selected, inside} d^2, hits = their number, gverts[f_k] += 2 beta_k (c - p)
"""
import numpy as np

from tests.render_ref import uv_sphere

# The medial-axis test of filter_cloud: `gap` = the second-best squared distance among the faces whose closest point differs from the best face's, minus
# the best; a point is dropped when gap < GAP_REL d_max^2, d_max the larger (second-best) of the two distances.  A RELATIVE gap: the float32 rounding of
# a squared distance is a few 2^-24 of d^2 itself, so 1e-6 d^2 is about ten times the difference below which single precision may name the other face.
# "Differs": across an edge shared by two faces the closest point moves continuously from one face onto the edge; for the foot c1 of the perpendicular
# on face A and the closest point c2 on its neighbour B, d2^2 - d1^2 ~ |c2 - c1|^2.  Every point whose foot lies within sqrt(GAP_REL) d of an edge
# would so have a gap below the bar without being anywhere near the medial axis (a band around every edge: 0.7 % of a cloud at 168 faces, 2.7 % at
# 1472, over 5 % at 13 776), and the outputs are continuous there.  Two closest points therefore count as different when they lie farther apart than
# sqrt(GAP_REL) d = SAME_REL d: exactly the pairs whose small gap adjacency does NOT explain - two separate nearest spots of the surface.
GAP_REL = 1e-6
SAME_REL = 1e-3


def peanut(stacks, slices, radius=0.5):
    """The concave test body: uv_sphere with every vertex scaled by 1 + 0.45 (2 z^2 - 1), z the unit-sphere height.  Closed, wound outwards."""
    v, f = uv_sphere(stacks, slices, radius=1.0)
    v = np.asarray(v, np.float64)
    z = v[:, 2:3] / np.linalg.norm(v, axis=1, keepdims=True)
    return radius * v * (1.0 + 0.45 * (2.0 * z * z - 1.0)), np.asarray(f, np.int64)


def _dot(x, y):
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]


def closest_bary(ab, ac, ap, bp, cp):
    """Barycentric weights (v, w) [the point is (1 - v - w) A + v B + w C] of the closest point of a triangle, from its edges ab, ac and the vectors from
    its corners to the point; every argument a triple of component arrays that broadcast.  Vertex A, vertex B, edge AB, vertex C, edge AC, edge BC,
    interior - the first region that applies.  The arithmetic stays in the inputs' dtype."""
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    dt = d1.dtype
    one, zero = dt.type(1), dt.type(0)

    def div(n, d):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(d > 0, n / np.where(d > 0, d, one), zero)
    inv = div(one, va + vb + vc)
    v, w = vb * inv, vc * inv                                                                          # interior
    t = div(d4 - d3, (d4 - d3) + (d5 - d6))
    cases = [((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), one - t, t),                                # edge BC
             ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, div(d2, d2 - d6)),                              # edge AC
             ((d6 >= 0) & (d5 <= d6), zero, one),                                                      # vertex C
             ((vc <= 0) & (d1 >= 0) & (d3 <= 0), div(d1, d1 - d3), zero),                              # edge AB
             ((d3 >= 0) & (d4 <= d3), one, zero),                                                      # vertex B
             ((d1 <= 0) & (d2 <= 0), zero, zero)]                                                      # vertex A
    for cond, vv, ww in cases:                       # later entries are the EARLIER regions: they have the last word
        v, w = np.where(cond, vv, v), np.where(cond, ww, w)
    return v.astype(dt, copy=False), w.astype(dt, copy=False)


def body_points(verts, faces, pts, dtype=np.float64, want_gap=False):
    """One body, points pts [n,3] (no selection here): w [n], d [n], face [n], beta [n,3], q = c - p [n,3] and (want_gap) gap [n]."""
    dtype = np.dtype(dtype).type
    verts, pts = np.asarray(verts, dtype), np.asarray(pts, dtype)
    faces = np.asarray(faces, np.int64)
    n, F = len(pts), len(faces)
    ok = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    V0, V1, V2 = (tuple(verts[faces[:, k], c][None, :] for c in range(3)) for k in range(3))
    ab, ac = tuple(V1[c] - V0[c] for c in range(3)), tuple(V2[c] - V0[c] for c in range(3))
    w, d2 = np.zeros(n, dtype), np.full(n, np.inf, dtype)
    face, beta, q, gap = np.full(n, -1, np.int64), np.zeros((n, 3), dtype), np.zeros((n, 3), dtype), np.full(n, np.inf)
    step = max(1, 1_500_000 // max(F, 1))
    for s in range(0, n, step):
        P = tuple(pts[s:s + step, c][:, None] for c in range(3))
        a, b, c = (tuple(Vk[i] - P[i] for i in range(3)) for Vk in (V0, V1, V2))
        la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
        bxc = (b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0])
        den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
        omega = np.where(ok[None], dtype(2) * np.arctan2(_dot(a, bxc), den), dtype(0))
        w[s:s + step] = omega.sum(1, dtype=dtype) / dtype(4 * np.pi)
        neg = lambda x: tuple(-x[i] for i in range(3))
        v, ww = closest_bary(ab, ac, neg(a), neg(b), neg(c))
        u = dtype(1) - v - ww
        qq = tuple(u * a[i] + v * b[i] + ww * c[i] for i in range(3))                                   # closest point - p
        dd = np.where(ok[None], _dot(qq, qq), np.inf)
        best = np.argmin(dd, axis=1)                                                                   # the first minimum: the lowest face index
        rows = np.arange(len(best))
        d2[s:s + step], face[s:s + step] = dd[rows, best], (best if ok.any() else -1)
        beta[s:s + step] = np.stack([u[rows, best], v[rows, best], ww[rows, best]], -1)
        qb = np.stack([qq[i][rows, best] for i in range(3)], -1)
        q[s:s + step] = qb
        if want_gap:
            apart = np.sqrt(sum((qq[i] - qb[:, i:i + 1]) ** 2 for i in range(3)))
            other = apart > SAME_REL * np.sqrt(dd[rows, best])[:, None]
            gap[s:s + step] = np.where(other & ok[None], dd, np.inf).min(1) - dd[rows, best]
    return dict(w=w, d=np.sqrt(d2), face=face, beta=beta, q=q, gap=gap)


def per_body(verts, faces, scene, dtype=np.float64, want_gap=False):
    """body_points of EVERY point of every body: what mesh_collision_ref(..., per=) assembles for either selection without computing it again."""
    return [body_points(v, faces, s, dtype, want_gap) for v, s in zip(verts, scene)]


def mesh_collision_ref(verts, faces, scene, all_points=False, dtype=np.float64, per=None):
    """verts [B,V,3], faces [F,3], scene [B,N,3] -> loss [B], gverts [B,V,3], hits [B] and per point [B,N]: selected, w, d, face (w = 0, d = inf,
    face = -1 where the point is not selected).  per: per_body(verts, faces, scene, dtype), if the caller has it."""
    dtype = np.dtype(dtype).type
    verts, scene = np.asarray(verts, dtype), np.asarray(scene, dtype)
    faces = np.asarray(faces, np.int64)
    B, V, N = verts.shape[0], verts.shape[1], scene.shape[1]
    out = dict(loss=np.zeros(B, dtype), gverts=np.zeros((B, V, 3), dtype), hits=np.zeros(B, np.int64), selected=np.zeros((B, N), bool),
               w=np.zeros((B, N), dtype), d=np.full((B, N), np.inf, dtype), face=np.full((B, N), -1, np.int64))
    for b in range(B):
        lo, hi = verts[b].min(0), verts[b].max(0)
        sel = np.ones(N, bool) if all_points else ((scene[b] >= lo).all(-1) & (scene[b] <= hi).all(-1))
        out["selected"][b] = sel
        if not sel.any():
            continue
        r = {k: x[sel] for k, x in per[b].items()} if per is not None else body_points(verts[b], faces, scene[b][sel], dtype)
        for k in ("w", "d", "face"):
            out[k][b, sel] = r[k]
        inside = (r["w"] > dtype(0.5)) & (r["face"] >= 0)
        out["hits"][b] = int(inside.sum())
        out["loss"][b] = (r["d"][inside] ** 2).sum(dtype=dtype)
        for k in range(3):
            np.add.at(out["gverts"][b], faces[r["face"][inside], k], dtype(2) * r["beta"][inside, k:k + 1] * r["q"][inside])
    return out


def filter_cloud(verts, faces, pts, n_want):
    """Filter the INPUTS: of the candidate cloud pts [M,3], drop every point that for ANY of the bodies verts [B,V,3] (float64) lies nearer than 1e-4 m to
    the surface, has |w - 0.5| < 1e-3, or sits on the medial axis (gap < 1e-6 d_max^2: two different nearest faces); keep the first n_want of the rest.
    Returns (kept [n_want,3], the dropped share among the candidates looked at, the bodies' float64 body_points of the kept points)."""
    pts = np.asarray(pts, np.float64)
    bad = np.zeros(len(pts), bool)
    per = []
    for vb in np.asarray(verts, np.float64):
        r = body_points(vb, faces, pts, np.float64, want_gap=True)
        bad |= (r["d"] < 1e-4) | (np.abs(r["w"] - 0.5) < 1e-3) | (r["gap"] < GAP_REL * (r["d"] ** 2 + r["gap"]))
        per.append(r)
    keep = np.nonzero(~bad)[0]
    assert len(keep) >= n_want, (len(keep), n_want)
    last = keep[n_want - 1] + 1                      # the candidates looked at to find n_want good ones
    keep = keep[:n_want]
    return pts[keep], float(bad[:last].mean()), [{k: x[keep] for k, x in r.items()} for r in per]


def rel_err(x, ref):
    """Max-norm error relative to the tensor's largest magnitude (0 for an all-zero reference that is matched exactly)."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    m = np.abs(ref).max() if ref.size else 0.0
    e = np.abs(x - ref).max() if ref.size else 0.0
    return e / m if m > 0 else e
