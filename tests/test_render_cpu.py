"""CPU: the rendering rule's float64 restatement (tests/render_ref.py) against closed forms, the share of ambiguous pixels of every case the GPU
tests use (asserted here, on the reference alone), the host side of egohmr_amd.render (the vertex -> face CSR, the OBJ mesh reader) and the
GPU-free part of the C ABI (bad descriptors, the descriptor's ctypes mirror)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import render_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_square_is_an_exact_rectangle_with_the_lambert_colour():
    """A fronto-parallel square at z = 2 facing the camera, projected onto [10.25, 30.25] x [8.75, 20.75] px: the samples inside are columns 10 .. 29
    and rows 9 .. 20; depth is 2 everywhere; n.l = 1, so the colour is base * (ambient + k), clamped."""
    fx = fy = 100.0
    cx, cy, z = 20.25, 14.75, 2.0
    x0, x1, y0, y1 = (10.25 - cx) * z / fx, (30.25 - cx) * z / fx, (8.75 - cy) * z / fy, (20.75 - cy) * z / fy
    v = np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]])
    f = np.array([[0, 2, 1], [0, 3, 2]])                     # counter-clockwise for an OpenGL viewer: the normal points at the camera
    for smooth in (False, True):
        r = R.render_ref(v, f, fx, fy, cx, cy, 32, 40, smooth=smooth, base_color=(0.5, 0.25, 0.125), ambient=0.3, diffuse=1.0)
        want = np.zeros((32, 40), bool)
        want[9:21, 10:30] = True
        np.testing.assert_array_equal(r["covered"], want)
        np.testing.assert_allclose(r["depth"][want], 2.0, rtol=1e-13)
        assert (r["depth"][~want] == 0).all() and (r["face_index"][~want] == -1).all()
        levels = [math.floor(255 * c * 1.3 + 0.5) for c in (0.5, 0.25, 0.125)]
        assert (r["color"][want] == levels).all() and (r["color"][~want] == 0).all()
    r = R.render_ref(v, f, fx, fy, cx, cy, 32, 40)            # the defaults: 1.0 * (0.3 + 4/pi) clamps
    assert (r["color"][want] == 255).all() and (r["color"][~want] == 0).all()
    # seen from behind (the winding reversed): ambient only, |n.l| with two_sided, nothing with cull_backface
    back = f[:, ::-1]
    assert tuple(R.render_ref(v, back, fx, fy, cx, cy, 32, 40, base_color=(0.5, 0.5, 0.5))["color"][15, 20]) == (38, 38, 38)      # floor(255 * 0.15 + 0.5)
    assert tuple(R.render_ref(v, back, fx, fy, cx, cy, 32, 40, base_color=(0.5, 0.5, 0.5), diffuse=1.0, two_sided=True)["color"][15, 20]) == (166,) * 3
    assert not R.render_ref(v, back, fx, fy, cx, cy, 32, 40, cull_backface=True)["covered"].any()
    assert R.render_ref(v, f, fx, fy, cx, cy, 32, 40, cull_backface=True)["covered"].sum() == 240
    # the diagonal is shared by the two faces: the lower index wins there, and the far copy of the square loses everywhere
    two = np.concatenate([v, v * [1, 1, 1] + [0, 0, 0.5]], 0)
    r = R.render_ref(two, np.concatenate([f + 4, f], 0), fx, fy, cx, cy, 32, 40)
    assert set(np.unique(r["face_index"])) == {-1, 2, 3} and np.allclose(r["depth"][want], 2.0)


def test_reference_sphere_centre_depth_is_the_ray_sphere_value_within_the_sagitta():
    """The pixel on the optical axis of a sphere of radius r centred on it at distance d sees depth d - r, up to the facets' sagitta
    r (1 - cos(half the longest edge's angle))."""
    r, d = 0.9, 2.6
    v, f = R.uv_sphere(24, 32, radius=r)
    res = R.render_ref(v + [0, 0, d], f, 150.0, 150.0, 80.5, 60.5, 120, 160)
    step = math.hypot(math.pi / 24, 2 * math.pi / 32)       # a facet's longest edge is at most the diagonal of one (stack, slice) cell
    sagitta = r * (1 - math.cos(step / 2))
    z = res["depth"][60, 80]                                # the sample (80.5, 60.5) is the principal point: the ray is the optical axis
    assert d - r <= z + 1e-12 and z <= d - r + sagitta, (z, d - r, sagitta)
    # the silhouette: a sphere's outline has radius f r / sqrt(d^2 - r^2) px about the principal point; the facetted one lies inside it
    rad = 150.0 * r / math.sqrt(d * d - r * r)
    ii, jj = np.nonzero(res["covered"])
    dist = np.hypot(jj + 0.5 - 80.5, ii + 0.5 - 60.5)
    assert dist.max() <= rad + 1e-9 and dist.max() >= rad * math.cos(step / 2) - 1.0


@pytest.mark.parametrize("name", ["case_sphere168", "case_sphere1472", "case_soup"])
def test_ambiguous_pixels_are_a_small_share_of_every_case(name):
    case = getattr(R, name)()
    res = R.render_case(case)
    share = R.ambiguous_share(res)
    covered = sum(int(r["covered"].sum()) for r in res)
    print(f"{name}: {covered} covered pixels, ambiguous share {share:.4f}")
    assert covered > 500 and share <= R.MAX_AMBIGUOUS
    # float32 against float64 on the same formulas: outside the ambiguous set both choose the same face
    for a, b in zip(res, R.render_case(case, dtype=np.float32)):
        keep = ~a["ambiguous"]
        np.testing.assert_array_equal(a["face_index"][keep], b["face_index"][keep])


def test_case_sphere168_items_are_what_the_gpu_test_needs():
    case = R.case_sphere168()
    res = R.render_case(case)
    assert res[0]["covered"].sum() > 400 and not res[0]["covered"][[0, -1]].any() and not res[0]["covered"][:, [0, -1]].any()     # inside
    assert res[1]["covered"][:, -1].any() and res[1]["covered"][-1].any()                                                        # cut by the border
    assert not res[2]["covered"].any()                                                                                             # behind z_near
    assert len(case["faces"]) == 168 and len(R.case_sphere1472()["faces"]) == 2 * 1472


def test_vertex_face_csr_against_brute_force():
    from egohmr_amd.render import build_vertex_face_csr
    g = np.random.Generator(np.random.PCG64(3))
    for V, F in ((7, 1), (50, 200), (98, 168)):
        faces = g.integers(0, V, size=(F, 3)) if F != 168 else R.uv_sphere(8, 12)[1]
        off, vf = build_vertex_face_csr(faces, V)
        assert off.dtype == np.int32 and vf.dtype == np.int32 and off.shape == (V + 1,) and vf.shape == (3 * F,) and off[0] == 0 and off[-1] == 3 * F
        for v in range(V):
            want = [f for f in range(F) for k in range(3) if faces[f, k] == v]       # face-index order, a face once per corner
            assert list(vf[off[v]:off[v + 1]]) == want, v


def test_read_obj_mesh_reads_every_token_form(tmp_path):
    from egohmr_amd.io import read_obj_mesh, read_obj_vertices
    p = tmp_path / "m.obj"
    p.write_text("# a comment\nmtllib x.mtl\nv 0 0 0 1 0 0\nv 1 0 0 0 1 0\nv 1 1 0 0 0 1\nv 0 1 0 0.5 0.5 0.5\nvn 0 0 1\nvt 0 0\n"
                 "f 1 2 3\nf 1/1 3/1 4/1\nf 1/1/1 2/1/1 3/1/1 4/1/1\nf -4//1 -3//1 -1//1\n"
                 "v 0.5 0.5 1.25 1 1 1\nf 1 2 -1\n\ng grp\nf 5 4 3 2 1\n")
    v, f, c = read_obj_mesh(str(p))
    assert v.dtype == np.float32 and f.dtype == np.int32 and c.dtype == np.float32
    np.testing.assert_array_equal(v, np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.25]]))
    np.testing.assert_array_equal(c, np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0.5], [1, 1, 1]]))
    np.testing.assert_array_equal(f, [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 1, 3], [0, 1, 4], [4, 3, 2], [4, 2, 1], [4, 1, 0]])
    np.testing.assert_array_equal(read_obj_vertices(str(p)), v.astype(np.float64))
    q = tmp_path / "plain.obj"                               # no colours on one vertex: none are returned
    q.write_text("v 0 0 0 1 0 0\nv 1 0 0\nv 0 1 0 1 1 1\nf 1 2 3\n")
    assert read_obj_mesh(str(q))[2] is None
    for bad in ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n",
                "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -4 1 2\n"):
        q.write_text(bad)
        with pytest.raises(ValueError):
            read_obj_mesh(str(q))


def _desc(**kw):
    """An ehm_render_desc every check accepts, on dummy (never dereferenced) addresses; each use breaks one rule."""
    from egohmr_amd import _lib
    f = dict(vertices=0x10000, faces=0x20000, vf_offsets=0x30000, vf_faces=0x40000, fx=0x50000, fy=0x60000, cx=0x70000, cy=0x80000, B=2, V=100, F=196,
             H=48, W=64, smooth=1, z_near=0.05, bin_capacity=1024, needed_capacity=0x90000, color=0xa0000)
    f.update(kw)
    return _lib.RenderDesc(**f)


def test_render_entries_reject_bad_descriptors_without_a_gpu():
    from egohmr_amd import _lib
    L = _lib.lib()
    n = C.c_int64(-1)
    assert L.ehm_render_workspace_bytes(C.byref(_desc()), C.byref(n)) == 0 and n.value > 2 * 196 * 64
    small = n.value
    assert L.ehm_render_workspace_bytes(C.byref(_desc(bin_capacity=4096)), C.byref(n)) == 0 and n.value - small == 2 * 3072 * 4
    for bad in (dict(vertices=None), dict(faces=None), dict(H=0), dict(W=0), dict(H=-3), dict(W=40000), dict(frames=0xb0000, Fr=1),
                dict(color=None), dict(B=0), dict(B=65536), dict(fx=None), dict(vf_offsets=None), dict(bin_capacity=0), dict(V=0), dict(F=0)):
        assert L.ehm_render(C.byref(_desc(**bad)), None) == -22, bad
        assert b"bad argument" in L.ehm_last_error(), bad
        assert L.ehm_render_workspace_bytes(C.byref(_desc(**bad)), C.byref(n)) == -22, bad
    assert L.ehm_render(None, None) == -22 and L.ehm_render_workspace_bytes(C.byref(_desc()), None) == -22
    # a good descriptor without a workspace, with too small a one, without the capacity array: refused before any device call
    assert L.ehm_render(C.byref(_desc()), None) == -22
    assert L.ehm_render(C.byref(_desc(workspace=0x100000, workspace_bytes=small - 1)), None) == -22
    assert L.ehm_render(C.byref(_desc(workspace=0x100000, workspace_bytes=small, needed_capacity=None)), None) == -22
    assert L.ehm_render(C.byref(_desc(workspace=0x100004, workspace_bytes=small)), None) == -22
    with pytest.raises(_lib.EgoHMRHipError, match="ehm_render"):
        _lib.api().ehm_render(C.byref(_desc(color=None)), None)
    assert "ehm_render" not in _lib.VALUE_FUNCTIONS and "ehm_render_workspace_bytes" not in _lib.VALUE_FUNCTIONS


def test_render_desc_mirror_has_the_c_layout(tmp_path):
    """sizeof and every field offset of ehm_render_desc from a compiled C program (the header is plain C99) against _lib.RenderDesc."""
    from egohmr_amd import _lib
    names = [n for n, _ in _lib.RenderDesc._fields_]
    body = ['  printf("%d", (int)sizeof(ehm_render_desc));'] + [f'  printf(" %d", (int)offsetof(ehm_render_desc, {n}));' for n in names]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "egohmr_hip.h"\nint main(void) {\n' + "\n".join(body) + '\n  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", _lib.INCLUDE, str(src), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert nums[0] == C.sizeof(_lib.RenderDesc)
    assert nums[1:] == [getattr(_lib.RenderDesc, n).offset for n in names]


def test_renderer_refuses_cpu_tensors_and_bad_faces():
    import torch
    from egohmr_amd import EgoHMRHipError, MeshRenderer, render_in_scene, render_on_img       # the package exports
    from egohmr_amd import render as rmod
    assert rmod.MeshRenderer is MeshRenderer and callable(render_on_img) and callable(render_in_scene)
    for faces in ([[0, 1, 7]], [[0, -1, 2]], np.zeros((0, 3), np.int64), [[0.0, 1.0, 2.0]]):
        with pytest.raises(ValueError):
            MeshRenderer(np.asarray(faces), "cpu", num_vertices=7)
    r = MeshRenderer(np.array([[0, 1, 2]]), "cpu")
    with pytest.raises(EgoHMRHipError):
        r.render(torch.zeros(1, 3, 3), 10.0, 10.0, 4.0, 4.0, size=(8, 8))
    with pytest.raises(EgoHMRHipError):
        render_on_img(10.0, 10.0, 4.0, 4.0, torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(3, 3), r)
    with pytest.raises(ValueError):
        r.render(torch.zeros(1, 3, 3), 10.0, 10.0, 4.0, 4.0, size=(8, 8), want=())
