"""GPU: csrc/render.hip (ehm_render) and egohmr_amd.render against the float64 restatement of the rule, tests/render_ref.py, at the smallest shapes
that still break things.  The bars, per case:
  face_index  equal on every pixel that is not ambiguous (render_ref: within 1e-3 px of an edge line, or two covering depths within 1e-4), the
              background included
  depth       within 4 x the error a float32 numpy evaluation of render_ref's formulas makes against float64 on the same case (both printed): the
              kernel evaluates those formulas in float32 too, in another operation order and with 1/z_k rounded once more
  color       within 1 level on every non-ambiguous pixel; the pixels that differ at all, ambiguous ones included, are at most 5 % of the covered
The share of ambiguous pixels is bounded in tests/test_render_cpu.py, on the reference alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import render_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_REF = {}


def reference(name, **opt):
    """(case, float64 results, float32 results) of a case of render_ref, computed once per option set."""
    key = (name, tuple(sorted(opt.items())))
    if key not in _REF:
        case = getattr(R, name)()
        _REF[key] = (case, R.render_case(case, **opt), R.render_case(case, dtype=np.float32, **opt))
    return _REF[key]


def gpu_render(case, dev, want=("color", "depth", "face_index"), bin_capacity=None, frames=None, frame_index=None, bg_color=(0, 0, 0), **opt):
    from egohmr_amd.render import MeshRenderer
    r = MeshRenderer(case["faces"], dev, num_vertices=case["vertices"].shape[1], bin_capacity=bin_capacity, **opt)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = r.render(t(case["vertices"]), t(case["fx"]), t(case["fy"]), t(case["cx"]), t(case["cy"]), frames=frames, frame_index=frame_index,
                   size=None if frames is not None else (case["H"], case["W"]), bg_color=bg_color, want=want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, r


def check(label, ref64, ref32, got, color=True):
    """The module docstring's bars for one case (lists over its items)."""
    err_gpu = err_32 = 0.0
    covered = differing = 0
    for b, (a, s) in enumerate(zip(ref64, ref32)):
        keep = ~a["ambiguous"]
        np.testing.assert_array_equal(got["face_index"][b][keep], a["face_index"][keep], err_msg=f"{label} item {b}: face_index")
        assert (got["depth"][b][~a["covered"] & keep] == 0).all()
        sel = keep & a["covered"]
        if sel.any():
            err_gpu = max(err_gpu, float(np.abs(got["depth"][b][sel] - a["depth"][sel]).max()))
            err_32 = max(err_32, float(np.abs(s["depth"][sel].astype(np.float64) - a["depth"][sel]).max()))
        if color:
            d = np.abs(got["color"][b].astype(int) - a["color"].astype(int)).max(-1)
            assert d[keep].max() <= 1, f"{label} item {b}: colour off by {d[keep].max()} levels"
            differing += int((d > 0).sum())
        covered += int(a["covered"].sum())
    print(f"{label}: depth error kernel {err_gpu:.3e} m, float32 numpy {err_32:.3e} m, ratio {err_gpu / err_32 if err_32 else float('nan'):.2f}; "
          f"{differing} of {covered} covered pixels differ in colour")
    assert err_gpu <= 4 * err_32, (label, err_gpu, err_32)
    assert differing <= 0.05 * covered, (label, differing, covered)


MODES = [dict(smooth=False), dict(smooth=True), dict(smooth=True, two_sided=True), dict(smooth=False, two_sided=True, cull_backface=True)]


@pytest.mark.parametrize("opt", MODES, ids=["flat", "smooth", "smooth-two-sided", "flat-two-sided-culled"])
def test_sphere_three_items_own_cameras(dev, opt):
    """168 faces, 64 x 48, B = 3: centred; partly outside the image; wholly behind z_near (all background)."""
    case, r64, r32 = reference("case_sphere168", **opt)
    got, _ = gpu_render(case, dev, **opt)
    check(f"sphere168 {opt}", r64, r32, got)
    assert (got["face_index"][2] == -1).all() and (got["depth"][2] == 0).all() and (got["color"][2] == 0).all()
    assert got["color"].dtype == np.uint8 and got["depth"].dtype == np.float32 and got["face_index"].dtype == np.int32


@pytest.mark.parametrize("opt", MODES[:3], ids=["flat", "smooth", "smooth-two-sided"])
def test_sphere_many_tiles_and_subpixel_faces(dev, opt):
    """1472 faces over 160 x 120 (3 x 8 tiles) plus a copy at z = 60 whose faces are smaller than a pixel."""
    case, r64, r32 = reference("case_sphere1472", **opt)
    far = r64[0]["face_index"] >= 1472
    assert 1 <= far.sum() <= 12
    got, _ = gpu_render(case, dev, **opt)
    check(f"sphere1472 {opt}", r64, r32, got)


def raw_render(r, case, dev, capacity, want=("color", "depth", "face_index"), color_offset=0, fill=None):
    """The entry itself, once, with `capacity` list entries per item -> (outputs, needed_capacity).  color_offset: the colour buffer starts that many
    bytes into a 16-byte aligned allocation.  fill: the outputs' initial byte."""
    from egohmr_amd import _lib
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    B, H, W = case["vertices"].shape[0], case["H"], case["W"]
    verts, cams = t(case["vertices"]), [t(case[k]) for k in ("fx", "fy", "cx", "cy")]
    raw = torch.full((B * H * W * 3 + color_offset,), fill if fill is not None else 0, dtype=torch.uint8, device=dev)
    outs = {"color": raw[color_offset:].view(B, H, W, 3), "depth": torch.zeros(B, H, W, device=dev), "face_index": torch.zeros(B, H, W, dtype=torch.int32, device=dev)}
    if fill is not None:
        outs["depth"].view(torch.uint8).fill_(fill)
        outs["face_index"].view(torch.uint8).fill_(fill)
    needed = torch.full((B,), -7, dtype=torch.int32, device=dev)
    d = r._desc(verts, *cams, None, None, H, W, (9, 8, 7), False, {k: outs[k] for k in want}, needed, capacity)
    if color_offset and "color" in want:
        d.color = raw.data_ptr() + color_offset
    n = C.c_int64(0)
    _lib.api().ehm_render_workspace_bytes(C.byref(d), C.byref(n))
    ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n.value
    _lib.api().ehm_render(C.byref(d), _lib.stream_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}, needed.cpu().numpy()


def test_triangle_soup_long_lists_and_a_small_bin_capacity(dev):
    """2000 overlapping triangles on 96 x 64 (two tile columns, the second half a tile; lists of many 128-record chunks).  With a bin capacity far too
    small MeshRenderer runs again with the needed one and matches; the raw entry flags the item and leaves it pure background."""
    case, r64, r32 = reference("case_soup", smooth=False, two_sided=True)
    got, r = gpu_render(case, dev, smooth=False, two_sided=True)
    check("soup", r64, r32, got)
    assert r.reruns == 0 and r.bin_capacity == 4 * 2000 + 64
    small, rs = gpu_render(case, dev, smooth=False, two_sided=True, bin_capacity=100)
    assert rs.reruns == 1 and 100 < rs.bin_capacity <= r.bin_capacity
    for k in got:
        np.testing.assert_array_equal(small[k], got[k])
    raw, needed = raw_render(rs, case, dev, 100)
    assert needed[0] == rs.bin_capacity
    assert (raw["color"] == [9, 8, 7]).all() and (raw["depth"] == 0).all() and (raw["face_index"] == -1).all()
    exact, needed = raw_render(rs, case, dev, rs.bin_capacity, color_offset=4)            # exactly enough, and a colour buffer off the 16-byte grid
    assert needed[0] == rs.bin_capacity
    cov = got["face_index"] >= 0
    np.testing.assert_array_equal(exact["face_index"], got["face_index"])
    np.testing.assert_array_equal(exact["depth"], got["depth"])
    np.testing.assert_array_equal(exact["color"][cov], got["color"][cov])
    assert (exact["color"][~cov] == [9, 8, 7]).all()


def _one(vertices, faces, fx, fy, cx, cy, H, W):
    return R._case(np.asarray(vertices, np.float32)[None], faces, [fx], [fy], [cx], [cy], H, W)


def test_shape_edges(dev):
    """W and H no multiples of the tile (67 x 45: two tile columns, three tile rows, the byte-wise colour path); a 1 x 1 image; F = 1; one triangle
    larger than the image; a mesh wholly off-screen; B = 1 throughout."""
    v, f = R.uv_sphere(8, 12, radius=0.6)
    big = np.float32([[-40, -30, 3], [50, -28, 2], [3, 60, 4]])
    cases = {
        "67x45 sphere": _one(v + np.float32([0.3, 0.1, 2.0]), f, 44.0, 45.5, 40.2, 21.7, 45, 67),
        "1x1 sphere": _one(v + np.float32([0, 0, 2.0]), f, 6.0, 6.0, 0.4, 0.6, 1, 1),
        "1x1 big triangle": _one(big, [[0, 1, 2]], 10.0, 10.0, 0.5, 0.5, 1, 1),
        "67x45 big triangle": _one(big, [[0, 2, 1]], 30.0, 30.0, 33.0, 22.0, 45, 67),
        "130x20 one small face": _one(np.float32([[0.1, 0.0, 2], [0.4, 0.05, 2.1], [0.2, 0.3, 1.9]]), [[0, 1, 2]], 90.0, 90.0, 100.0, 4.0, 20, 130),
        "off-screen sphere": _one(v + np.float32([30.0, 0, 2.0]), f, 44.0, 44.0, 33.0, 22.0, 45, 67),
    }
    for label, case in cases.items():
        opt = dict(smooth=label.endswith("sphere"), two_sided=True)
        r64, r32 = R.render_case(case, **opt), R.render_case(case, dtype=np.float32, **opt)
        got, _ = gpu_render(case, dev, **opt)
        assert got["color"].shape == (1, case["H"], case["W"], 3)
        n = int(r64[0]["covered"].sum())
        assert (n == 0) == (label == "off-screen sphere") and (label != "67x45 big triangle" or n == 45 * 67)
        if n:
            check(label, r64, r32, got)
        else:
            assert (got["face_index"] == -1).all() and (got["depth"] == 0).all() and (got["color"] == 0).all()


def test_non_finite_vertex_drops_its_faces_only(dev):
    """One vertex of item 1 is NaN and one of its neighbours infinite: the faces that use them are absent, the rest of the item is the reference's, and
    items 0 and 2 are bit-equal to a run without item 1."""
    case = dict(R.case_sphere168())
    case["vertices"] = case["vertices"].copy()
    front = int(np.argmin(case["vertices"][1, :, 2]))
    other = [int(i) for i in case["faces"][np.nonzero((case["faces"] == front).any(1))[0][0]] if i != front][0]
    case["vertices"][1, front, 1] = np.nan
    case["vertices"][1, other, 0] = np.inf
    for opt in (dict(smooth=False), dict(smooth=True)):
        r64, r32 = R.render_case(case, **opt), R.render_case(case, dtype=np.float32, **opt)
        got, _ = gpu_render(case, dev, **opt)
        check(f"non-finite {opt}", r64, r32, got)
        bad = np.nonzero(~np.isfinite(case["vertices"][1]).all(1))[0]
        gone = np.nonzero(np.isin(case["faces"], bad).any(1))[0]
        assert len(bad) == 2 and len(gone) >= 6 and not np.isin(got["face_index"][1], gone).any()
        clean = {k: (v[[0, 2]] if k != "faces" and isinstance(v, np.ndarray) else v) for k, v in case.items()}
        two, _ = gpu_render(clean, dev, **opt)
        for k in got:
            np.testing.assert_array_equal(got[k][[0, 2]], two[k])


def test_composite_over_shared_frames_and_null_outputs(dev):
    case, r64, _ = reference("case_sphere168", smooth=True)
    H, W = case["H"], case["W"]
    g = np.random.Generator(np.random.PCG64(11))
    frames = g.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)
    fidx = np.int32([1, 1, 0])
    got, r = gpu_render(case, dev, frames=torch.from_numpy(frames).to(dev), frame_index=torch.from_numpy(fidx).to(dev), smooth=True)
    plain, _ = gpu_render(case, dev, bg_color=(3, 250, 77), smooth=True)
    for b in range(3):
        cov = got["face_index"][b] >= 0
        np.testing.assert_array_equal(got["color"][b][~cov], frames[fidx[b]][~cov])           # bit-equal to the frame
        np.testing.assert_array_equal(got["color"][b][cov], plain["color"][b][cov])           # the body does not depend on the background
        assert (plain["color"][b][~cov] == [3, 250, 77]).all()
        want = R.render_ref(case["vertices"][b], case["faces"], case["fx"][b], case["fy"][b], case["cx"][b], case["cy"][b], H, W, background=frames[fidx[b]])
        keep = ~r64[b]["ambiguous"]
        assert np.abs(got["color"][b].astype(int) - want["color"].astype(int)).max(-1)[keep].max() <= 1
    for k in ("depth", "face_index"):
        np.testing.assert_array_equal(got[k], plain[k])
    # a NULL output is not computed: only the requested buffers change
    for want in (("depth",), ("color",), ("face_index", "color")):
        raw, _ = raw_render(r, case, dev, r.bin_capacity, want=want, fill=0xAB)
        for k in ("color", "depth", "face_index"):
            if k in want:
                sel = got["face_index"] >= 0 if k == "color" else np.ones_like(got["face_index"], bool)      # (the raw call's background colour is its own)
                np.testing.assert_array_equal(raw[k][sel], plain[k][sel])
            else:
                assert (raw[k].view(np.uint8) == 0xAB).all(), (want, k)
    only = r.render(torch.from_numpy(case["vertices"]).to(dev), *[torch.from_numpy(case[k]).to(dev) for k in ("fx", "fy", "cx", "cy")], size=(H, W), want=("depth",))
    assert set(only) == {"depth"} and np.array_equal(only["depth"].cpu().numpy(), got["depth"])


def test_render_in_scene_interpolates_vertex_colours(dev):
    """Two meshes through render_in_scene (a sphere as the body, moved by a 4 x 4, and a coloured triangle soup as the scene) against the reference on
    the concatenation with per-vertex colours; the output is BGR as the reference's."""
    from egohmr_amd.render import render_in_scene, scene_renderer
    body, bf = R.uv_sphere(8, 12, radius=0.5)
    scene, sf = R.triangle_soup(300, 9, extent=(1.4, 1.0), depth=(2.0, 4.0))
    g = np.random.Generator(np.random.PCG64(13))
    sc = g.uniform(0, 1, size=(len(scene), 3)).astype(np.float32)
    T = np.eye(4)
    T[:3, :3] = R.rotation(0.2, -0.5)
    T[:3, 3] = [0.1, 0.05, 2.4]
    H, W, cam = 64, 96, (42.0, 41.0, 48.3, 31.2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    img = render_in_scene(*cam, t(body), t(scene), t(sf), t(sc), body_faces=bf, size=(H, W), body_transform=T, two_sided=True)
    assert img.shape == (H, W, 3) and img.dtype == torch.uint8
    moved = (body.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    verts = np.concatenate([moved, scene], 0)
    colors = np.concatenate([np.tile(np.float32(R.BASE_COLOR), (len(body), 1)), sc], 0)
    ref = R.render_ref(verts, np.concatenate([bf, sf + len(body)], 0), *cam, H, W, bg_color=(255, 255, 255), vertex_colors=colors, ambient=0.0,
                       two_sided=True)
    assert R.ambiguous_share([ref]) <= R.MAX_AMBIGUOUS and (ref["face_index"] < len(bf))[ref["covered"]].sum() > 100
    d = np.abs(img.cpu().numpy()[..., ::-1].astype(int) - ref["color"].astype(int)).max(-1)
    print(f"render_in_scene: {int((d > 0).sum())} of {int(ref['covered'].sum())} covered pixels differ, max {d[~ref['ambiguous']].max()} levels")
    assert d[~ref["ambiguous"]].max() <= 1 and (d > 0).sum() <= 0.05 * ref["covered"].sum()
    kept = scene_renderer(bf, len(body), sf, sc, dev, two_sided=True)
    again = render_in_scene(*cam, t(body)[None], t(scene), size=(H, W), body_transform=T, renderer=kept)
    assert again.shape == (1, H, W, 3) and torch.equal(again[0], img)


def test_render_on_img_of_smpl_vertices_equals_the_raw_entry(dev, smpl_asset):
    from egohmr_amd import MeshRenderer, render_on_img, smpl as smpl_mod
    body = smpl_mod.create(asset=smpl_asset, gender="neutral").to(dev)
    g = np.random.Generator(np.random.PCG64(21))
    B, H, W = 2, 90, 160
    with torch.no_grad():
        out = body(betas=torch.from_numpy(g.normal(size=(B, 10)).astype(np.float32)).to(dev),
                   body_pose=torch.from_numpy(g.normal(scale=0.2, size=(B, 69)).astype(np.float32)).to(dev),
                   global_orient=torch.zeros(B, 3, device=dev), transl=torch.tensor([[0.0, 0.1, 3.0], [0.3, -0.1, 2.5]], device=dev))
    verts = out.vertices.contiguous()
    frames = torch.from_numpy(g.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)).to(dev)
    r = MeshRenderer(body.faces, dev, num_vertices=verts.shape[1])
    img = render_on_img(120.0, 120.0, 80.0, 45.0, frames, verts, r)
    assert img.shape == (B, H, W, 3) and img.dtype == torch.uint8 and (img != frames).any(dim=-1).sum() > 200
    one = render_on_img(120.0, 120.0, 80.0, 45.0, frames[1], verts[1], r)
    assert one.shape == (H, W, 3) and torch.equal(one, img[1])
    case = dict(vertices=verts.cpu().numpy(), fx=np.float32([120, 120]), fy=np.float32([120, 120]), cx=np.float32([80, 80]), cy=np.float32([45, 45]), H=H, W=W)
    raw, needed = raw_render(r, case, dev, r.bin_capacity, want=("face_index",))
    rgb = MeshRenderer(body.faces, dev, num_vertices=verts.shape[1], base_color=R.BASE_COLOR[::-1])      # what bgr=True turns the material into
    direct = rgb.render(verts, 120.0, 120.0, 80.0, 45.0, frames=frames, want=("color", "face_index"))
    assert torch.equal(direct["color"], img) and np.array_equal(direct["face_index"].cpu().numpy(), raw["face_index"]) and (needed <= r.bin_capacity).all()
    assert torch.equal(render_on_img(120.0, 120.0, 80.0, 45.0, frames, verts, r), img)                   # two calls, the same bits


def test_stage2_driver_render_overlays_the_decoded_samples(dev, synth_weights, smpl_asset):
    from egohmr_amd import synthetic as syn, smpl as smpl_mod
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.driver import Stage2Driver
    from egohmr_amd.factory import batch_to_device, build_synthetic_model
    from egohmr_amd.render import MeshRenderer
    B, N, S, n, rs = 2, 1024, 2, 50, "ddim5"
    model = build_synthetic_model(dev, 0, diffuse_fuse=True, state_dict=synth_weights, smpl_asset=smpl_asset)
    bnp = syn.make_batch(B, N, seed=23)
    gt = syn.make_gt_annotations(B, seed=23)
    bnp["smpl_params"].update({k: gt[k] for k in ("global_orient", "body_pose", "betas")})
    bnp["gender"] = gt["gender"]
    bnp["cam_cx"] = bnp["cam_cx"] + np.float32([0.75, -3.5])                      # the script truncates the principal point: int(cam_cx)
    smpls = {k: smpl_mod.create(asset=syn.make_smpl_asset(i) if i else smpl_asset, gender=k).to(dev) for i, k in enumerate(("neutral", "male", "female"))}
    d = create_gaussian_diffusion(num_diffusion_timesteps=n, timestep_respacing=rs)
    drv = Stage2Driver(model, d, smpls["neutral"], smpls["male"], smpls["female"], num_samples=S, timestep_respacing=rs, eval_contact_score=False)
    batch = batch_to_device(bnp, dev)
    step = drv.step(batch, [torch.from_numpy(syn.make_noise_stack(d.num_timesteps, B, seed=23 + 10 * s)).to(dev) for s in range(S)])
    H, W = 1080, 1920
    frames = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)).to(dev)
    fidx = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    img = drv.render(step, batch, frames, fidx, items=(1, 0))
    assert img.shape == (2, S, H, W, 3) and img.dtype == torch.uint8
    assert drv.render(step, batch, frames, fidx).shape == (1, S, H, W, 3) and drv.render(step, batch, frames, fidx, items=(0, 1), samples=(1,)).shape == (2, 1, H, W, 3)
    r = MeshRenderer(smpls["neutral"].faces, dev, num_vertices=step["decoded"]["vertices_full"].shape[2])
    for i, item in enumerate((1, 0)):
        f = float(bnp["fx"][item]) * drv.fx_norm_coeff
        want = r.render(step["decoded"]["vertices_full"][item].contiguous(), f, f, float(int(bnp["cam_cx"][item])), float(int(bnp["cam_cy"][item])),
                        frames=frames[int(fidx[item])][None], bgr=True)["color"]
        assert torch.equal(img[i], want) and (want != frames[int(fidx[item])]).any(dim=-1).sum() > 1000
    assert torch.equal(drv.render(step, batch, frames, fidx, items=(1, 0)), img)
