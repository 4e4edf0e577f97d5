"""GPU: ehm_scene_select (egohmr_amd.scene.SceneClouds) against the float64 numpy restatements of tests/test_scene_cpu.py: the selected vertices
and n_selected equal, the points bit-equal to the restatement's T_out v in float32 and within one float32 ulp of the loader's form; constructed
ties on every bound; the k = 1 / 2 edges; failures; determinism; and stage 1 -> cube -> Stage2Driver(two_stage=True) end to end."""
import math
import random

import numpy as np
import pytest
import torch

from egohmr_amd import scene as es
from egohmr_amd._lib import EgoHMRHipError
from tests.test_scene_cpu import cube_center_ref, cube_ref, loader_rows, out_rows, whole_scene_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _mesh(g, n, half=3.0):
    """a room-sized synthetic mesh: x, z in [-half, half], y in [0, 3] (sizes not a multiple of the 2048-vertex tile)"""
    return np.stack([g.uniform(-half, half, n), g.uniform(0, 3, n), g.uniform(-half, half, n)], -1)


def _affine(g, t=2.0):
    a, b = g.uniform(0, 2 * np.pi), g.uniform(-0.3, 0.3)
    R = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]]) @ \
        np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, g.uniform(-t, t, 3)
    return T


def _ulps(a, b):
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def _check_item(got_pts, got_idx, got_n, mesh, ref_idx, ref_n, T_out, stride):
    assert got_n == ref_n
    assert np.array_equal(got_idx, ref_idx[::stride])
    want = out_rows(mesh[ref_idx], T_out, stride)
    assert np.array_equal(got_pts, want)
    assert _ulps(got_pts, loader_rows(mesh[ref_idx], T_out, stride)) <= 1


SIZES = [2**21, 300001, 77777, 40961]


@pytest.fixture(scope="module")
def meshes():
    g = np.random.default_rng(11)
    return [_mesh(g, n) for n in SIZES]


@pytest.mark.parametrize("num_meshes", [1, 2, 4])
def test_cube_matches_restatement(dev, meshes, num_meshes):
    g = np.random.default_rng(100 + num_meshes)
    ms = meshes[:num_meshes] if num_meshes > 1 else [meshes[2]]
    sc = es.SceneClouds(ms, dev)
    B, target, stride = (256 if num_meshes == 4 else 40), 2000, (1 if num_meshes != 2 else 3)
    mi = g.integers(0, len(ms), B)
    crop = np.stack([_affine(g) for _ in range(B)])
    out = np.stack([_affine(g) for _ in range(B)])
    centres = g.uniform(-1.5, 1.5, (B, 3))                                  # in mesh coordinates, then to the PV frame as a float32 translation
    tp = np.stack([(crop[b, :3, :3] @ centres[b] + crop[b, :3, 3]) for b in range(B)]).astype(np.float32)
    ang = g.uniform(0, 2 * np.pi, B)
    pts, n, idx = sc.cube(torch.from_numpy(mi), torch.from_numpy(tp).to(dev), crop, out, angle=ang, target=target, stride=stride, return_index=True)
    assert pts.shape == (B, -(-target // stride), 3) and pts.dtype == torch.float32
    pts, n, idx = pts.cpu().numpy(), n.cpu().numpy(), idx.cpu().numpy()
    for b in range(B):
        c = cube_center_ref(tp[[b]], crop[b])
        ref_idx, ref_n = cube_ref(ms[mi[b]], c, ang[b], 2, target)
        _check_item(pts[b], idx[b], n[b], ms[mi[b]], ref_idx, ref_n, out[b], stride)


def test_cube_full_size_and_rng_draws(dev, meshes):
    g = np.random.default_rng(7)
    sc = es.SceneClouds([meshes[0]], dev)
    B = 24
    crop = np.stack([_affine(g) for _ in range(B)])
    out = np.stack([_affine(g) for _ in range(B)])
    tp = np.stack([(crop[b, :3, :3] @ g.uniform(-1.5, 1.5, 3) + crop[b, :3, 3]) for b in range(B)]).astype(np.float32)
    pts, n, idx = sc.cube([0] * B, tp, crop, out, rng=random.Random(5), return_index=True)
    r = random.Random(5)
    ang = [r.uniform(0, 2 * (math.pi)) for _ in range(B)]                   # the script draws once per frame, in frame order
    assert sc.last_angles == ang
    pts, n, idx = pts.cpu().numpy(), n.cpu().numpy(), idx.cpu().numpy()
    for b in range(B):
        ref_idx, ref_n = cube_ref(meshes[0], cube_center_ref(tp[[b]], crop[b]), ang[b], 2, 20000)
        _check_item(pts[b], idx[b], n[b], meshes[0], ref_idx, ref_n, out[b], 1)


@pytest.mark.parametrize("num_meshes", [1, 3])
def test_whole_scene_matches_restatement(dev, meshes, num_meshes):
    g = np.random.default_rng(200 + num_meshes)
    ms = [meshes[0]] if num_meshes == 1 else meshes[1:]
    sc = es.SceneClouds(ms, dev)
    B, target = (16, 20000) if num_meshes == 1 else (64, 2000)
    mi = g.integers(0, len(ms), B)
    K = 4
    chain = np.stack([np.stack([_affine(g, 0.3) for _ in range(K)]) for _ in range(B)])    # small shifts: z > 0 keeps a good share of the room
    out = np.stack([_affine(g) for _ in range(B)])
    pts, n, idx = sc.whole_scene(mi, chain, out, target=target, stride=2, return_index=True)
    pts, n, idx = pts.cpu().numpy(), n.cpu().numpy(), idx.cpu().numpy()
    for b in range(B):
        ref_idx, ref_n = whole_scene_ref(ms[mi[b]], chain[b], target)
        _check_item(pts[b], idx[b], n[b], ms[mi[b]], ref_idx, ref_n, out[b], 2)
    # K = 1 and 2: shorter chains
    for K in (1, 2):
        pts, n, idx = sc.whole_scene(mi[:8], chain[:8, :K], out[:8], target=target, return_index=True)
        for b in range(8):
            ref_idx, ref_n = whole_scene_ref(ms[mi[b]], chain[b, :K], target)
            _check_item(pts[b].cpu().numpy(), idx[b].cpu().numpy(), n[b].item(), ms[mi[b]], ref_idx, ref_n, out[b], 1)


def test_constructed_ties(dev):
    eps = np.nextafter
    # cube, a = 0, centre (0, *, 0): the rotated coordinates are the vertex's own; vertices exactly on the four faces are in, one ulp outside
    # are out; y == ymin + 2 is in, one ulp above is out
    c = np.array([0.0, 0.25, 0.0], np.float32)
    face = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 2.0, 1.0), (-1.0, 0.0, -1.0)]
    out_ = [(eps(1.0, 9), 0.0, 0.0), (eps(-1.0, -9), 0.0, 0.0), (0.0, 0.0, eps(1.0, 9)), (0.0, 0.0, eps(-1.0, -9)), (0.0, eps(2.0, 9), 0.0)]
    fill = [(0.1 * i - 0.3, 1.0, 0.05 * i - 0.5) for i in range(12)]
    v = np.array(face + out_ + fill, np.float64)
    I = np.eye(4)
    sc = es.SceneClouds([v], dev)
    target = len(face) + len(fill)
    pts, n, idx = sc.cube([0], c[None], I[None], I[None], angle=[0.0], target=target, return_index=True)
    ref_idx, ref_n = cube_ref(v, cube_center_ref(c[None], I), 0.0, 2, target)
    assert ref_n == target and n.item() == target
    assert np.array_equal(idx[0].cpu().numpy(), ref_idx) and set(ref_idx.tolist()) == set(range(len(face))) | set(range(11, 11 + len(fill)))
    # whole scene under identity transforms: z == 0 is out, the smallest positive z is in
    w = np.array([(0, 0, 0.0), (0, 0, 5e-324), (0, 0, -0.0), (1, 1, 1.0), (0, 0, -5e-324)], np.float64)
    sc = es.SceneClouds([w], dev)
    pts, n, idx = sc.whole_scene([0], np.stack([I] * 4)[None], I[None], target=2, return_index=True)
    assert n.item() == 2 and idx[0].cpu().tolist() == [1, 3]


@pytest.mark.parametrize("n_sel,target,stride", [(1000, 1000, 1), (1999, 1000, 1), (2000, 1000, 1), (2000, 1000, 7), (4099, 1000, 3)])
def test_counts(dev, n_sel, target, stride):
    g = np.random.default_rng(n_sel + stride)
    N = 3 * n_sel + 17
    v = _mesh(g, N)
    front = np.sort(g.choice(N, n_sel, replace=False))
    v[:, 2] = -np.abs(v[:, 2]) - 0.01
    v[front, 2] = np.abs(v[front, 2]) + 0.01
    I = np.eye(4)
    sc = es.SceneClouds([v], dev)
    pts, n, idx = sc.whole_scene([0], np.stack([I] * 4)[None], I[None], target=target, stride=stride, return_index=True)
    k = n_sel // target
    assert n.item() == n_sel
    assert np.array_equal(idx[0].cpu().numpy(), front[0::k][:target][::stride])


def test_key_frame_selects_with_one_chain_and_outputs_with_another(dev, meshes):
    g = np.random.default_rng(9)
    sc = es.SceneClouds([meshes[3]], dev)
    key = np.stack([_affine(g) for _ in range(4)])
    outs = np.stack([_affine(g) for _ in range(3)])                         # three frames after the key frame, each with its own loader matrix
    pts, n, idx = sc.whole_scene([0] * 3, np.stack([key] * 3), outs, target=3000, return_index=True)
    ref_idx, ref_n = whole_scene_ref(meshes[3], key, 3000)
    for b in range(3):
        _check_item(pts[b].cpu().numpy(), idx[b].cpu().numpy(), n[b].item(), meshes[3], ref_idx, ref_n, outs[b], 1)
    assert not np.array_equal(pts[0].cpu().numpy(), pts[1].cpu().numpy())


def test_failures_name_the_items(dev, meshes):
    sc = es.SceneClouds([meshes[3]], dev)
    I = np.eye(4)
    tp = np.array([[0, 0, 0], [100, 0, 100], [0, 0, 0]], np.float32)       # item 1: far outside the room, an empty crop
    with pytest.raises(EgoHMRHipError, match=r"item 1: empty xz crop, n_selected = 0") as e:
        sc.cube([0] * 3, tp, np.stack([I] * 3), np.stack([I] * 3), angle=[0.0, 0.0, 0.0], target=1000)
    assert "item 0" not in str(e.value) and "item 2" not in str(e.value)
    ref_n = cube_ref(meshes[3], np.zeros(3), 0.0, 2, 1)[1]
    with pytest.raises(EgoHMRHipError, match=rf"item 0: fewer than target vertices selected, n_selected = {ref_n}"):
        sc.cube([0], tp[:1], I[None], I[None], angle=[0.0], target=ref_n + 1)
    with pytest.raises(EgoHMRHipError, match=r"item 1: fewer than target"):
        sc.whole_scene([0, 0], np.stack([np.stack([I] * 4)] * 2), np.stack([I] * 2), target=len(meshes[3]))   # (item 0: the same)


def test_two_runs_are_bit_equal(dev, meshes):
    g = np.random.default_rng(13)
    sc = es.SceneClouds(meshes[1:3], dev)
    B = 48
    crop = np.stack([_affine(g) for _ in range(B)])
    tp = np.stack([(crop[b, :3, :3] @ g.uniform(-1, 1, 3) + crop[b, :3, 3]) for b in range(B)]).astype(np.float32)
    args = (np.arange(B) % 2, tp, crop, crop)
    a = sc.cube(*args, angle=g.uniform(0, 6, B), target=3000, return_index=True)
    b = sc.cube(*args, angle=sc.last_angles, target=3000, return_index=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_stage1_cube_stage2_end_to_end(dev, golden_dir, stage2_fixture):
    """stage 1 (synthetic ProHMRSceneTransl) -> its translations -> cube(...) -> Stage2Driver(two_stage=True).step, against feeding the driver the
    restatement's cloud: bit-equal outputs."""
    import os

    from egohmr_amd.driver import Stage2Driver
    from egohmr_amd.factory import batch_to_device
    from tests.test_gpu_stage1 import _g19_batch, _stage1_model
    st = stage2_fixture
    g19 = np.load(os.path.join(golden_dir, "g19_stage1_all_on.npz"))
    transl = _stage1_model("all_on", dev)(_g19_batch(g19, dev))["pred_cam_full"]          # [5, 3] float32 on the device
    B, N = transl.shape[0], st["bnp"]["scene_pcd_verts_full"].shape[1]
    g = np.random.default_rng(17)
    crop = np.stack([_affine(g) for _ in range(B)])
    loader = np.stack([_affine(g) for _ in range(B)])
    tp = transl.cpu().numpy()
    centres = np.stack([cube_center_ref(tp[[b]], crop[b]) for b in range(B)])
    lo, hi = centres.min(0) - 1.5, centres.max(0) + 1.5
    nv = max(400003, int(1000 * (hi[0] - lo[0]) * (hi[2] - lo[2])))       # ~1000 vertices per square metre: N of them in every crop
    mesh = np.stack([g.uniform(lo[0], hi[0], nv), g.uniform(0, 3, nv), g.uniform(lo[2], hi[2], nv)], -1)
    sc = es.SceneClouds([mesh], dev)
    ang = g.uniform(0, 2 * np.pi, B)
    pts, _ = sc.cube([0] * B, transl, crop, loader, angle=ang, target=N)
    ref = np.stack([out_rows(mesh[cube_ref(mesh, centres[b], ang[b], 2, N)[0]], loader[b]) for b in range(B)])
    assert np.array_equal(pts.cpu().numpy(), ref)
    sm, S, rs = st["smpls"], st["S"], st["rs"]
    outs = []
    for cloud in (pts, torch.from_numpy(ref).to(dev)):
        drv = Stage2Driver(st["model"], st["diffusion"], sm["neutral"], sm["male"], sm["female"], num_samples=S, timestep_respacing=rs,
                           eval_contact_score=False, two_stage=True)
        b = batch_to_device(st["bnp"], dev)
        b["scene_pcd_verts_full"] = cloud
        b["stage1_transl_full"] = transl
        outs.append(drv.step(b, [torch.from_numpy(z).to(dev) for z in st["noises"]]))
    a, c = outs
    for k in ("betas", "global_orient", "body_pose"):
        assert torch.equal(a["pred"][k], c["pred"][k]), k
    for k in ("g_mpjpe", "mpjpe", "pa_mpjpe", "v2v"):
        assert torch.equal(a[k], c[k]), k


@pytest.fixture(scope="module")
def stage2_fixture(dev, synth_weights, smpl_asset):
    """a synthetic stage-2 model and batch, as tests/test_gpu_stage1.py's `stage2` fixture"""
    from egohmr_amd import smpl as smpl_mod
    from egohmr_amd import synthetic as syn
    from egohmr_amd.diffusion import create_gaussian_diffusion
    from egohmr_amd.factory import build_synthetic_model
    B, N, S, n, rs = 5, 1024, 2, 50, "ddim5"
    model = build_synthetic_model(dev, 0, state_dict=synth_weights, smpl_asset=smpl_asset)
    bnp = syn.make_batch(B, N, seed=23, vis_prob=0.5)
    gt = syn.make_gt_annotations(B, seed=23)
    bnp["smpl_params"].update({k: gt[k] for k in ("global_orient", "body_pose", "betas")})
    bnp["gender"] = gt["gender"]
    assets = {gname: syn.make_smpl_asset(i) for i, gname in enumerate(("neutral", "male", "female"))}
    assets["neutral"] = smpl_asset
    smpls = {k: smpl_mod.create(asset=a, gender=k).to(dev) for k, a in assets.items()}
    d = create_gaussian_diffusion(num_diffusion_timesteps=n, timestep_respacing=rs)
    noises = [syn.make_noise_stack(d.num_timesteps, B, seed=23 + 10 * s) for s in range(S)]
    return dict(model=model, diffusion=d, smpls=smpls, bnp=bnp, noises=noises, S=S, rs=rs)
