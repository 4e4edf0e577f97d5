"""CPU: the near-plane rule's restatement (tests/render_clip_ref.py) against a closed form and against the existing rule (tests/render_ref.py), the
share of ambiguous pixels of every case tests/test_gpu_render_clip.py uses (asserted here, on the reference alone), and the GPU-free part of the
C ABI: the clip_near field's values, its place in the descriptor, and the workspace it does not change."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import render_clip_ref as K
from tests import render_ref as R


@pytest.mark.parametrize("H,W", [(48, 64), (45, 67)])
def test_floor_depth_is_the_ray_plane_value_below_the_horizon(H, W):
    """A ray through (u, v) below the horizon meets the plane y = 1.2 at z = 1.2 fy / (v - cy) and x = (u - cx) z / fx; the quad holds the points
    with |x| <= 4 and z <= 8 (z >= -2 is no bound in front of the camera, and z > z_near holds for every row of the image).  Both faces cross, so the
    existing rule draws nothing."""
    case = K.case_floor(H, W)
    v, f = case["vertices"][0], case["faces"]
    fx, fy, cx, cy = (float(case[k][0]) for k in ("fx", "fy", "cx", "cy"))
    assert len(K.crossing_faces(v, f, 0.05)) == 2
    r = K.render_clip_ref(v, f, fx, fy, cx, cy, H, W, two_sided=True)
    uu, vv = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    with np.errstate(divide="ignore"):
        z = float(v[0, 1]) * fy / (vv - cy)                   # (the float32 vertex's own y: the float32 nearest to 1.2)
    x = (uu - cx) * z / fx
    inside = (vv > cy) & (z <= 8) & (np.abs(x) <= 4)
    keep = ~r["ambiguous"]
    np.testing.assert_array_equal(r["covered"][keep], inside[keep])
    assert inside.sum() > 0.3 * H * W and r["ambiguous"].sum() <= 0.06 * inside.sum()
    sel = keep & inside
    np.testing.assert_allclose(r["depth"][sel], z[sel], rtol=1e-12)
    assert not r["covered"][vv < cy].any() and (r["depth"][vv < cy] == 0).all() and (r["color"][vv < cy] == 0).all()
    assert not R.render_ref(v, f, fx, fy, cx, cy, H, W, two_sided=True)["covered"].any()
    # item 1 is wholly in front: no crossing face, and the clipped reference is the existing one
    v1 = case["vertices"][1]
    cam = [float(case[k][1]) for k in ("fx", "fy", "cx", "cy")]
    assert len(K.crossing_faces(v1, f, 0.05)) == 0
    a, b = K.render_clip_ref(v1, f, *cam, H, W, two_sided=True), R.render_ref(v1, f, *cam, H, W, two_sided=True)
    assert a["covered"].sum() > 200
    for k in ("color", "depth", "face_index", "ambiguous"):
        np.testing.assert_array_equal(a[k], b[k])


@pytest.mark.parametrize("opt", [dict(smooth=False), dict(smooth=True), dict(smooth=True, two_sided=True, cull_backface=True)], ids=["flat", "smooth", "culled"])
def test_homogeneous_rule_on_faces_in_front_agrees_with_the_existing_rule(opt):
    """case_sphere168 item 0 is wholly in front.  The homogeneous rule applied to every one of its faces, in float64, gives render_ref's coverage,
    winners, depth and colour off the ambiguous pixels: D has the sign of area, E_k / S are the perspective-correct weights, D / S is the depth."""
    case = R.case_sphere168()
    g = np.random.Generator(np.random.PCG64(31))
    colors = g.uniform(0, 1, size=(case["vertices"].shape[1], 3))
    args = (case["vertices"][0], case["faces"], case["fx"][0], case["fy"][0], case["cx"][0], case["cy"][0], case["H"], case["W"])
    for extra in (dict(), dict(vertex_colors=colors)):
        a = R.render_ref(*args, **opt, **extra)
        b = K.render_clip_ref(*args, all_homogeneous=True, **opt, **extra)
        keep = ~(a["ambiguous"] | b["ambiguous"])
        assert a["covered"].sum() > 400 and keep.sum() > 0.9 * keep.size
        np.testing.assert_array_equal(a["face_index"][keep], b["face_index"][keep])
        np.testing.assert_allclose(b["depth"][keep], a["depth"][keep], rtol=1e-12, atol=0)
        np.testing.assert_array_equal(a["color"][keep], b["color"][keep])


def gpu_cases():
    """name -> (case, options): every case of tests/test_gpu_render_clip.py that is compared with the reference."""
    out = {"floor 64x48": (K.case_floor(), dict(two_sided=True)), "floor 67x45": (K.case_floor(45, 67), dict(two_sided=True))}
    for smooth in (0, 1):
        for two_sided in (0, 1):
            for cull in (0, 1):
                out[f"cut sphere s{smooth} t{two_sided} c{cull}"] = (K.case_cut_sphere(), dict(smooth=bool(smooth), two_sided=bool(two_sided), cull_backface=bool(cull)))
    out["inside sphere"] = (K.case_inside_sphere(), dict(smooth=True, two_sided=True))
    out["cut soup"] = (K.case_cut_soup(), dict(smooth=False, two_sided=True))
    room, _, _, colors = K.case_room()
    out["room"] = (room, dict(two_sided=True, vertex_colors=colors, ambient=0.0))
    return out


CASES = gpu_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_ambiguous_pixels_are_a_small_share_of_every_clip_case(name):
    case, opt = CASES[name]
    res = K.render_clip_case(case, **opt)
    share = R.ambiguous_share(res)
    covered = sum(int(r["covered"].sum()) for r in res)
    crossing = sum(int(r["crossing_covered"].sum()) for r in res)
    print(f"{name}: {covered} covered pixels, {crossing} under a crossing face, ambiguous share {share:.4f}")
    assert covered > 300 and crossing > 100 and share <= K.MAX_AMBIGUOUS
    for a, b in zip(res, K.render_clip_case(case, dtype=np.float32, **opt)):      # float32 on the same formulas chooses the same faces
        keep = ~a["ambiguous"]
        np.testing.assert_array_equal(a["face_index"][keep], b["face_index"][keep])


def test_clip_cases_are_what_the_gpu_tests_need():
    soup = K.case_cut_soup()
    z = soup["vertices"][0][:, 2].reshape(-1, 3)
    front = (z > 0.05).sum(1)
    crossing = ((front > 0) & (front < 3)).sum()
    assert 70 <= crossing <= 130 and (z[(front > 0) & (front < 3)].min(1) < 0).sum() > 20 and len(K.crossing_faces(soup["vertices"][0], soup["faces"], 0.05)) == crossing
    sph = K.case_cut_sphere()
    assert np.linalg.norm(sph["vertices"][0].mean(0)) > 0.6 and 20 < len(K.crossing_faces(sph["vertices"][0], sph["faces"], 0.05)) < 100
    inside = K.render_clip_case(K.case_inside_sphere(), smooth=True, two_sided=True)[0]
    assert (inside["covered"] | inside["ambiguous"]).all()
    room, nbv, nbf, colors = K.case_room()
    on = K.render_clip_case(room, two_sided=True, vertex_colors=colors, ambient=0.0)[0]
    off = R.render_case(room, two_sided=True, vertex_colors=colors, ambient=0.0)[0]
    assert (on["covered"] | on["ambiguous"]).all() and (~off["covered"]).sum() > 500
    body = off["face_index"] >= 0
    body &= off["face_index"] < nbf
    assert body.sum() > 200 and np.array_equal(on["face_index"][body], off["face_index"][body]) and len(room["faces"]) == nbf + 12


def _desc(**kw):
    from egohmr_amd import _lib
    f = dict(vertices=0x10000, faces=0x20000, vf_offsets=0x30000, vf_faces=0x40000, fx=0x50000, fy=0x60000, cx=0x70000, cy=0x80000, B=2, V=100, F=196,
             H=48, W=64, smooth=1, z_near=0.05, bin_capacity=1024, needed_capacity=0x90000, color=0xa0000)
    f.update(kw)
    return _lib.RenderDesc(**f)


def test_clip_near_takes_0_or_1_and_needs_no_workspace():
    from egohmr_amd import _lib
    L = _lib.lib()
    n0, n1 = C.c_int64(-1), C.c_int64(-2)
    assert L.ehm_render_workspace_bytes(C.byref(_desc(clip_near=0)), C.byref(n0)) == 0
    assert L.ehm_render_workspace_bytes(C.byref(_desc(clip_near=1)), C.byref(n1)) == 0
    assert n0.value == n1.value > 0
    for bad in (2, -1, 256):
        assert L.ehm_render_workspace_bytes(C.byref(_desc(clip_near=bad)), C.byref(n0)) == -22, bad
        assert L.ehm_render(C.byref(_desc(clip_near=bad, workspace=0x100000, workspace_bytes=n1.value)), None) == -22, bad
        assert b"bad argument" in L.ehm_last_error()


def test_clip_near_is_the_last_field_of_the_c_descriptor(tmp_path):
    from egohmr_amd import _lib
    assert _lib.RenderDesc._fields_[-1][0] == "clip_near"
    src = tmp_path / "clip.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "egohmr_hip.h"\nint main(void) {\n'
                   '  printf("%d %d %d\\n", (int)sizeof(ehm_render_desc), (int)offsetof(ehm_render_desc, clip_near), (int)sizeof(((ehm_render_desc*)0)->clip_near));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "clip"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", _lib.INCLUDE, str(src), "-o", str(exe)], check=True)
    size, off, width = (int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == C.sizeof(_lib.RenderDesc) and off == _lib.RenderDesc.clip_near.offset and width == C.sizeof(C.c_int)
    assert off == _lib.RenderDesc.workspace_bytes.offset + 8


def test_mesh_renderer_takes_the_flag_and_defaults_to_off():
    from egohmr_amd.render import MeshRenderer, scene_renderer
    f = np.array([[0, 1, 2]])
    assert MeshRenderer(f, "cpu").clip_near is False and MeshRenderer(f, "cpu", clip_near=True).clip_near is True
    assert scene_renderer(f, 3, f, None, "cpu").clip_near is False and scene_renderer(f, 3, f, None, "cpu", clip_near=True).clip_near is True
