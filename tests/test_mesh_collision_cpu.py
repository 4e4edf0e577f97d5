"""CPU: the mesh collision term's float64 restatement (tests/mesh_collision_ref.py) against what must hold of it on a closed concave body, the
exports and ctypes prototypes of its two entry points, and the Python switch EgoHMR.collision_proxy - no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import mesh_collision_ref as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cloud(n, seed, verts, faces):
    g = np.random.Generator(np.random.PCG64(seed))
    return M.filter_cloud(verts[None] if verts.ndim == 2 else verts, faces, g.uniform(-0.8, 0.8, size=(n + n // 20, 3)), n)[:2]


def test_winding_number_of_the_peanut_is_zero_or_one():
    for stacks, slices in ((8, 12), (24, 32)):
        v, f = M.peanut(stacks, slices)
        pts = np.random.Generator(np.random.PCG64(1)).uniform(-0.8, 0.8, size=(600, 3))
        r = M.body_points(v, f, pts)
        assert np.abs(r["w"] - np.round(r["w"])).max() < 1e-12
        assert set(np.unique(np.round(r["w"]).astype(int))) == {0, 1}
        # the concavity is there: the waist is thinner than the lobes
        assert np.round(M.body_points(v, f, np.array([[0.0, 0.0, 0.6], [0.4, 0.0, 0.0], [0.2, 0.0, 0.0]]))["w"]).tolist() == [1, 0, 1]


def test_filter_drops_at_most_one_percent_of_the_gpu_clouds():
    """The clouds of tests/test_gpu_mesh_collision.py (seed 3, the three bodies of its case 1) on the reference alone."""
    for stacks, slices in ((8, 12), (24, 32)):
        v, f = M.peanut(stacks, slices)
        bodies = np.stack([v, 0.7 * v + [0.05, -0.03, 0.02]])
        pts, dropped = _cloud(3000, 3, bodies, f)
        print(f"peanut {len(f)} faces: dropped share {dropped:.4f}")
        assert pts.shape == (3000, 3) and dropped <= 0.01


def test_gverts_is_the_finite_difference_of_the_loss():
    v, f = M.peanut(8, 12)
    pts, _ = _cloud(400, 5, v, f)
    ref = M.mesh_collision_ref(v[None], f, pts[None])
    assert ref["hits"][0] > 20 and ref["selected"][0].sum() > ref["hits"][0]
    g, h = ref["gverts"][0], 1e-6
    touched = np.nonzero(np.abs(g).sum(1) > 0)[0]
    assert len(touched) > 10
    fd = np.zeros_like(g)
    for i in touched:
        for c in range(3):
            vp, vm = v.copy(), v.copy()
            vp[i, c] += h
            vm[i, c] -= h
            # all_points: the bounding box moves with a vertex, the selected set must not (every inside point is selected either way)
            fd[i, c] = (M.mesh_collision_ref(vp[None], f, pts[None], all_points=True)["loss"][0] -
                        M.mesh_collision_ref(vm[None], f, pts[None], all_points=True)["loss"][0]) / (2 * h)
    assert np.abs(fd - g).max() <= 1e-6 * np.abs(g).max(), (np.abs(fd - g).max(), np.abs(g).max())
    assert (g[np.setdiff1d(np.arange(len(v)), touched)] == 0).all()


def test_translation_changes_nothing_and_far_bodies_are_exact_zeros():
    v, f = M.peanut(8, 12)
    pts, _ = _cloud(300, 7, v, f)
    t = np.array([2.0, -1.0, 0.5])                         # exactly representable sums at these magnitudes are not needed: float64 has the room
    a, b = M.mesh_collision_ref(v[None], f, pts[None]), M.mesh_collision_ref((v + t)[None], f, (pts + t)[None])
    np.testing.assert_array_equal(a["hits"], b["hits"])
    np.testing.assert_array_equal(a["selected"], b["selected"])
    # (a point whose foot lies on an edge up to rounding may name either face of that edge: d^2 moves by the rounding, ~1e-16, the closest point and
    # with it the gradient by its square root, ~1e-8 - the outputs are continuous there, which is what the two bounds say)
    assert (a["face"] == b["face"]).mean() > 0.98
    np.testing.assert_allclose(a["loss"], b["loss"], rtol=1e-12)
    np.testing.assert_allclose(a["gverts"], b["gverts"], rtol=0, atol=1e-7 * np.abs(a["gverts"]).max())
    far = M.mesh_collision_ref((v + 10.0)[None], f, pts[None])
    assert far["hits"][0] == 0 and far["loss"][0] == 0 and not far["gverts"].any() and not far["selected"].any()
    # a single triangle and a face list with repeated indices: no NaN, no hit
    one = M.mesh_collision_ref(v[None], f[:1], pts[None], all_points=True)
    assert one["hits"][0] == 0 and one["loss"][0] == 0 and np.isfinite(one["w"]).all() and np.abs(one["w"]).max() < 0.5
    soup = np.concatenate([f, [[3, 3, 7], [5, 9, 5], [2, 2, 2]]])
    s = M.mesh_collision_ref(v[None], soup, pts[None])
    np.testing.assert_array_equal(s["hits"], a["hits"])
    np.testing.assert_array_equal(s["gverts"], a["gverts"])


def test_float32_restatement_is_close_to_float64():
    v, f = M.peanut(8, 12)
    pts, _ = _cloud(500, 9, v, f)
    v32, p32 = v.astype(np.float32), pts.astype(np.float32)
    a = M.mesh_collision_ref(v32[None], f, p32[None])
    b = M.mesh_collision_ref(v32[None], f, p32[None], dtype=np.float32)
    assert b["loss"].dtype == np.float32 and b["gverts"].dtype == np.float32
    np.testing.assert_array_equal(a["hits"], b["hits"])
    sel = a["selected"][0]
    assert np.abs(a["w"][0, sel] - b["w"][0, sel]).max() < 5e-6
    assert M.rel_err(b["loss"], a["loss"]) < 1e-5 and M.rel_err(b["gverts"], a["gverts"]) < 1e-4


def test_library_exports_and_binds_the_mesh_collision_entries():
    """The two entry points are exported, and _lib binds them with the header's argument lists (this is the test that fails without the feature)."""
    from egohmr_amd import _lib
    _lib.build()
    L = _lib.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "egohmr_hip.h")).read(), flags=re.S)
    ctype = {"const float*": C.c_void_p, "float*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t*": C.c_void_p, "void*": C.c_void_p,
             "ehm_smpl*": C.c_void_p, "int": C.c_int}
    for name in ("ehm_mesh_collision_query", "ehm_smpl_set_collision_mesh"):
        assert hasattr(L, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in the header"
        args = [re.sub(r"\s*\b\w+$", "", a.strip()).replace(" *", "*") for a in m.group(1).split(",")]      # drop the parameter names
        res, proto = _lib.PROTOTYPES[name]
        assert res is C.c_int and proto == [ctype[a] for a in args], (name, args)
        assert name not in _lib.VALUE_FUNCTIONS
    assert [a.strip().split()[-1] for a in re.search(r"ehm_mesh_collision_query\s*\(([^)]*)\)", text).group(1).split(",")] == \
        ["verts", "faces", "scene", "loss", "gverts", "hits", "B", "V", "F", "N", "all_points", "stream"]
    for macro, val in (("EHM_MESH_COLLISION_FACE_CHUNK", _lib.MESH_COLLISION_FACE_CHUNK), ("EHM_MESH_COLLISION_POINT_BLOCK", _lib.MESH_COLLISION_POINT_BLOCK)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", text).group(1)) == val
    # argument checks run before any device call (dummy addresses: nothing is dereferenced)
    ok = dict(verts=0x10000, faces=0x20000, scene=0x30000, loss=0x40000, gverts=None, hits=None, B=2, V=86, F=168, N=64, all_points=0, stream=None)
    for bad in (dict(verts=None), dict(faces=None), dict(scene=None), dict(loss=None), dict(B=0), dict(B=65536), dict(V=0), dict(F=0), dict(N=0)):
        assert L.ehm_mesh_collision_query(*dict(ok, **bad).values()) == -22, bad
        assert b"bad argument" in L.ehm_last_error()
    faces = (C.c_int32 * 3)(0, 1, 2)
    assert L.ehm_smpl_set_collision_mesh(None, faces, 1) == -22
    with pytest.raises(_lib.EgoHMRHipError, match="ehm_smpl_set_collision_mesh"):
        _lib.api().ehm_smpl_set_collision_mesh(None, faces, 1)
    # a host stand-in for a handle (V leads it, tests/test_smpl_autograd_cpu.py): a negative count and an index that is no vertex are refused
    # before anything is allocated
    fake = (C.c_int * 2)(86, 0)
    assert L.ehm_smpl_set_collision_mesh(fake, faces, -1) == -22
    assert L.ehm_smpl_set_collision_mesh(fake, None, 1) == -22
    for bad in ((0, 1, 86), (0, -1, 2)):
        assert L.ehm_smpl_set_collision_mesh(fake, (C.c_int32 * 3)(*bad), 1) == -22
        assert b"is not a vertex" in L.ehm_last_error()


def test_collision_proxy_switch_rejects_unknown_values():
    import torch
    from egohmr_amd.factory import build_synthetic_model
    m = build_synthetic_model("cpu", 0)
    assert m.collision_proxy == "vertex" and not m.mesh_collision()
    for bad in ("faces", "Mesh", "", None, 1):
        with pytest.raises(ValueError, match="collision_proxy"):
            m.collision_proxy = bad
        assert m.collision_proxy == "vertex"
    m.collision_proxy = "mesh"
    assert m.mesh_collision()
    m.collision_model = object()                           # an attached model takes precedence
    assert not m.mesh_collision()
    m.collision_model = None
    # the calibrated precision schedule is kept per collision mode for guided loops, and shared for unguided ones
    from egohmr_amd.diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion(num_diffusion_timesteps=50, timestep_respacing="ddim5")
    fs = m.fused_sampler
    k_mesh, u_mesh = fs.schedule_key(d, True, 4, 1.0), fs.schedule_key(d, True, 0)
    m.collision_proxy = "vertex"
    assert fs.schedule_key(d, True, 4, 1.0) != k_mesh and fs.schedule_key(d, True, 0) == u_mesh
    # faces are validated once, on the host, before any device call
    m.collision_proxy = "mesh"
    assert m.smpl.collision_faces_host().dtype == np.int32 and m.smpl.collision_faces_host().shape == tuple(m.smpl.faces_tensor.shape)
    m.smpl.faces_tensor = torch.tensor([[0, 1, m.smpl.num_verts]])
    with pytest.raises(ValueError, match="vertices"):
        m.smpl.collision_faces_host()
