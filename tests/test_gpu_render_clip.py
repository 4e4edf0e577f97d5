"""GPU: ehm_render with clip_near = 1 (csrc/render.hip, egohmr_amd.render) against the float64 restatement of the near-plane rule,
tests/render_clip_ref.py, at the smallest shapes at which a face can straddle the plane in every way.  Every case is compared by
tests/test_gpu_render.py's `check`, with its bars: face_index equal on every pixel that is not ambiguous, depth within 4 x the error of the float32
run of the reference, colour within 1 level there, differing pixels at most 5 % of the covered.  The share of ambiguous pixels is bounded in
tests/test_render_clip_cpu.py, on the reference alone."""
import numpy as np
import pytest
import torch

from tests import render_clip_ref as K
from tests import render_ref as R
from tests.test_gpu_render import check, gpu_render, raw_render

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_REF = {}


def reference(name, case, **opt):
    """(float64 results, float32 results) of a case of render_clip_ref, computed once per name."""
    if name not in _REF:
        _REF[name] = (K.render_clip_case(case, **opt), K.render_clip_case(case, dtype=np.float32, **opt))
    return _REF[name]


def only_under_crossing_faces(on, off, r64):
    """Invariant 3: the two flag values differ only where some crossing face covers or nearly covers the pixel."""
    for b, a in enumerate(r64):
        away = ~a["crossing_near"]
        for k in on:
            np.testing.assert_array_equal(on[k][b][away], off[k][b][away], err_msg=f"{k} item {b}")


@pytest.mark.parametrize("H,W", [(48, 64), (45, 67)], ids=["64x48", "67x45-bytewise"])
def test_floor_under_the_camera_and_a_floor_wholly_in_front(dev, H, W):
    """B = 2 with their own cameras: item 0's two faces both cross (without the flag the item is pure background), item 1's are wholly in front and
    bit-equal with the flag on and off."""
    case = K.case_floor(H, W)
    r64, r32 = reference(f"floor {H}x{W}", case, two_sided=True)
    got, _ = gpu_render(case, dev, two_sided=True, clip_near=True)
    check(f"floor {W}x{H}", r64, r32, got)
    off, _ = gpu_render(case, dev, two_sided=True)
    assert (off["face_index"][0] == -1).all() and (got["face_index"][0] >= 0).sum() > 0.3 * H * W
    for k in got:
        np.testing.assert_array_equal(got[k][1], off[k][1])
    only_under_crossing_faces(got, off, r64)
    again, _ = gpu_render(case, dev, two_sided=True, clip_near=True)                 # two calls, the same bits
    for k in got:
        np.testing.assert_array_equal(again[k], got[k])


@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("two_sided", [0, 1])
@pytest.mark.parametrize("smooth", [0, 1])
def test_sphere_cut_by_the_near_plane_camera_outside(dev, smooth, two_sided, cull):
    case = K.case_cut_sphere()
    opt = dict(smooth=bool(smooth), two_sided=bool(two_sided), cull_backface=bool(cull))
    r64, r32 = reference(f"cut sphere {opt}", case, **opt)
    got, _ = gpu_render(case, dev, clip_near=True, **opt)
    check(f"cut sphere {opt}", r64, r32, got)
    off, _ = gpu_render(case, dev, **opt)
    only_under_crossing_faces(got, off, r64)
    crossing = K.crossing_faces(case["vertices"][0], case["faces"], 0.05)
    assert np.isin(got["face_index"], crossing).sum() > 800 and not np.isin(off["face_index"], crossing).any()      # (937 pixels in the reference)


def test_sphere_seen_from_inside_covers_every_pixel(dev):
    case = K.case_inside_sphere()
    r64, r32 = reference("inside sphere", case, smooth=True, two_sided=True)
    got, _ = gpu_render(case, dev, smooth=True, two_sided=True, clip_near=True)
    check("inside sphere", r64, r32, got)
    keep = ~r64[0]["ambiguous"]
    assert (got["face_index"][0][keep] >= 0).all() and (got["depth"][0][keep] > 0.05).all()
    off, _ = gpu_render(case, dev, smooth=True, two_sided=True)
    assert (off["face_index"] == -1).sum() > 300


def test_soup_through_the_plane_default_capacity_and_one_rerun(dev):
    """300 triangles, a third of them crossing, many with a vertex behind the camera (z < 0).  A bin capacity too small makes MeshRenderer run once
    more with the needed one: a crossing face counts like any other, and the result is the same."""
    case = K.case_cut_soup()
    r64, r32 = reference("cut soup", case, smooth=False, two_sided=True)
    got, r = gpu_render(case, dev, smooth=False, two_sided=True, clip_near=True)
    check("cut soup", r64, r32, got)
    off, roff = gpu_render(case, dev, smooth=False, two_sided=True)
    only_under_crossing_faces(got, off, r64)
    small, rs = gpu_render(case, dev, smooth=False, two_sided=True, clip_near=True, bin_capacity=50)
    assert rs.reruns == 1 and 50 < rs.bin_capacity <= r.bin_capacity
    for k in got:
        np.testing.assert_array_equal(small[k], got[k])
    raw, needed = raw_render(rs, case, dev, 50)                                       # the raw entry: flagged, pure background
    assert needed[0] == rs.bin_capacity and (raw["face_index"] == -1).all() and (raw["depth"] == 0).all() and (raw["color"] == [9, 8, 7]).all()
    _, needed_off = raw_render(roff, case, dev, roff.bin_capacity)
    assert needed[0] > needed_off[0]                                                  # the crossing faces are in the lists
    exact, needed = raw_render(rs, case, dev, rs.bin_capacity)
    assert needed[0] == rs.bin_capacity
    np.testing.assert_array_equal(exact["face_index"], got["face_index"])
    np.testing.assert_array_equal(exact["depth"], got["depth"])


def test_render_in_scene_draws_a_closed_room_closed(dev):
    """A box of 12 faces around the camera and a sphere as the body, through render_in_scene with per-vertex colours.  With the flag no pixel is
    background; without it the walls beside, above and below the camera are missing (the defect); the body's pixels do not change."""
    from egohmr_amd.render import render_in_scene
    case, nbv, nbf, colors = K.case_room()
    H, W = case["H"], case["W"]
    cam = tuple(float(case[k][0]) for k in ("fx", "fy", "cx", "cy"))
    verts, faces = case["vertices"][0], case["faces"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = (*cam, t(verts[:nbv]), t(verts[nbv:]), t(faces[nbf:] - nbv), t(colors[nbv:]))
    on = render_in_scene(*args, body_faces=faces[:nbf], size=(H, W), two_sided=True, clip_near=True).cpu().numpy()
    off = render_in_scene(*args, body_faces=faces[:nbf], size=(H, W), two_sided=True, clip_near=False).cpu().numpy()
    assert on.shape == (H, W, 3) and on.dtype == np.uint8
    r64, r32 = reference("room", case, two_sided=True, vertex_colors=colors, ambient=0.0)
    ref = r64[0]
    keep = ~ref["ambiguous"]
    d = np.abs(on[..., ::-1].astype(int) - ref["color"].astype(int)).max(-1)         # (the output is BGR)
    print(f"room: {int((d > 0).sum())} of {int(ref['covered'].sum())} covered pixels differ, max {d[keep].max()} levels")
    assert d[keep].max() <= 1 and (d > 0).sum() <= 0.05 * ref["covered"].sum()
    # the room's colours are in [0.2, 1] and two-sided lit, but a level 255 in all three channels is not excluded by that: use the face index
    from egohmr_amd.render import scene_renderer
    r = scene_renderer(faces[:nbf], nbv, faces[nbf:] - nbv, colors[nbv:], dev, two_sided=True, clip_near=True)
    out = r.render(t(case["vertices"]), *cam, size=(H, W), bg_color=(255, 255, 255), want=("color", "depth", "face_index"), bgr=True)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    np.testing.assert_array_equal(got["color"][0], on)
    assert (got["face_index"][0][keep] >= 0).all(), "a closed room has no background pixel"
    got["color"] = got["color"][..., ::-1]
    check("room", r64, r32, got)
    roff = scene_renderer(faces[:nbf], nbv, faces[nbf:] - nbv, colors[nbv:], dev, two_sided=True)
    fo = roff.render(t(case["vertices"]), *cam, size=(H, W), bg_color=(255, 255, 255), want=("color", "face_index"), bgr=True)
    holes = (fo["face_index"][0] == -1).cpu().numpy()
    assert holes.sum() > 0 and (off[holes] == 255).all(), "without the flag the room has holes"
    print(f"room: {int(holes.sum())} of {H * W} pixels are background without clip_near, 0 with it")
    body = (ref["face_index"] >= 0) & (ref["face_index"] < nbf) & keep
    assert body.sum() > 200
    np.testing.assert_array_equal(on[body], off[body])


@pytest.mark.parametrize("name,items", [("case_sphere168", (0, 1)), ("case_soup", (0,))])
def test_without_a_crossing_face_the_flag_changes_no_bit(dev, name, items):
    case = dict(getattr(R, name)())
    for k in ("vertices", "fx", "fy", "cx", "cy"):
        case[k] = case[k][list(items)]
    assert all(len(K.crossing_faces(v, case["faces"], 0.05)) == 0 for v in case["vertices"])
    for opt in (dict(smooth=True), dict(smooth=False, two_sided=True)):
        r = {}
        for flag in (False, True):
            from egohmr_amd.render import MeshRenderer
            m = MeshRenderer(case["faces"], dev, num_vertices=case["vertices"].shape[1], clip_near=flag, **opt)
            r[flag] = raw_render(m, case, dev, m.bin_capacity)
        for k in ("color", "depth", "face_index"):
            np.testing.assert_array_equal(r[True][0][k], r[False][0][k])
        np.testing.assert_array_equal(r[True][1], r[False][1])
        assert (r[True][0]["face_index"] >= 0).sum() > 400


def test_drop_rules_with_the_flag_on(dev):
    """A crossing face with a NaN vertex is dropped and its neighbours stay; a vertex at exactly z == z_near makes its face crossing, not in front; a
    face wholly behind is still dropped; a NULL output is not computed."""
    z_near = np.float32(0.05)
    zn = float(z_near)                                     # the float32 value itself, for the float64 reference too: the vertex IS on the plane
    # three separate triangles: 0 crosses, 1 crosses with a NaN vertex, 2 is wholly behind; and 3, in front except for one vertex exactly on the plane
    tri = np.float32([[-0.6, 0.3, -0.4], [0.1, 0.25, 1.5], [-0.5, -0.3, 1.2],
                      [0.2, 0.3, -0.4], [0.9, 0.25, 1.5], [np.nan, -0.3, 1.2],
                      [-0.3, -0.2, -1.0], [0.3, -0.2, -2.0], [0.0, 0.3, -1.5],
                      [0.02, -0.01, z_near], [0.6, -0.5, 1.0], [0.1, -0.6, 1.1]])
    faces = np.arange(12, dtype=np.int32).reshape(4, 3)
    case = R._case(tri[None], faces, [30.0], [30.0], [31.7], [24.3], 48, 64)
    assert list(K.crossing_faces(tri, faces, float(z_near))) == [0, 3]
    r64, r32 = K.render_clip_case(case, smooth=False, two_sided=True, z_near=zn), K.render_clip_case(case, dtype=np.float32, smooth=False, two_sided=True, z_near=zn)
    assert R.ambiguous_share(r64) <= K.MAX_AMBIGUOUS
    got, r = gpu_render(case, dev, smooth=False, two_sided=True, z_near=zn, clip_near=True)
    check("drop rules", r64, r32, got)
    seen = set(np.unique(got["face_index"]))
    assert seen == {-1, 0, 3}, seen
    off, _ = gpu_render(case, dev, smooth=False, two_sided=True, z_near=zn)
    assert (off["face_index"] == -1).all()                 # face 3 is not "in front": without the flag the vertex on the plane drops it
    # the same face 3 moved one float32 above the plane is wholly in front, and takes the existing rule with the flag on and off
    up = tri.copy()
    up[9, 2] = np.nextafter(z_near, np.float32(1))
    case_up = R._case(up[None], faces, [30.0], [30.0], [31.7], [24.3], 48, 64)
    a, _ = gpu_render(case_up, dev, smooth=False, two_sided=True, z_near=zn, clip_near=True)
    b, _ = gpu_render(case_up, dev, smooth=False, two_sided=True, z_near=zn)
    assert (b["face_index"] == 3).sum() > 50 and np.array_equal(np.where(a["face_index"] == 3, a["depth"], 0), np.where(b["face_index"] == 3, b["depth"], 0))
    # only the requested buffer is written
    raw, _ = raw_render(r, case, dev, r.bin_capacity, want=("depth",), fill=0xAB)
    np.testing.assert_array_equal(raw["depth"], got["depth"])
    assert (raw["color"] == 0xAB).all() and (raw["face_index"].view(np.uint8) == 0xAB).all()
