"""CPU: float64 numpy restatements of the reference's scene-cloud preprocessing (preprocess_scene_s1.py, preprocess_scene_s2_for_test.py) and
its loader's transforms (dataloaders/egobody_dataset.py), checked on hand-built clouds whose selection is known by construction; the host half
of egohmr_amd.scene (egobody_transforms, the per-item parameters, the item groups, argument validation) and io.read_obj_vertices.
tests/test_gpu_scene.py checks ehm_scene_select against these restatements."""
import math

import numpy as np
import pytest

from egohmr_amd import scene as es

ADD_TRANS = np.array([[1.0, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]])   # preprocess_scene_s1.py:57-60


# ------------------------------------------------------------------------------------------------ restatements (also used by test_gpu_scene)
def o3d_transform(v, T):
    """open3d's mesh.transform / pcd.transform of [p, 1] (w = 1 for an affine T), elementwise in float64: ((T0 x + T1 y) + T2 z) + T3."""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], -1)


def uniform_down_sample(sel, k):
    """open3d's PointCloud.uniform_down_sample(every_k_points=k): the points of indices range(0, n, k); k = 0 raises, as open3d does."""
    if k < 1:
        raise ValueError("Illegal sample rate.")
    return sel[list(range(0, len(sel), k))]


def select(sel, target):
    """select(pred, target) of the reference scripts: sel = indices where pred holds in mesh order; k = int(n / target)
    (preprocess_scene_s1.py:118-124, preprocess_scene_s2_for_test.py:206-208)."""
    k = int(len(sel) / target)
    return uniform_down_sample(sel, k)[0:target]


def whole_scene_ref(verts, chain, target):
    """preprocess_scene_s1.py:102-118: the chain of mesh.transform (:104-107), z > 0 (:113), select (:118-124).  -> (indices, n)."""
    v = np.asarray(verts, np.float64)
    for T in chain:
        v = o3d_transform(v, np.asarray(T, np.float64))
    sel = np.nonzero(v[:, -1] > 0)[0]
    return select(sel, target), len(sel)


def cube_ref(verts, body_center, rot_angle, cube_size, target):
    """preprocess_scene_s2_for_test.py:176-208 with the script's own expressions.  -> (indices, n); raises as the script aborts."""
    scene_verts = np.asarray(verts, np.float64)
    scene_verts_aug = np.zeros(scene_verts.shape)
    scene_verts_aug[:, 0] = (scene_verts[:, 0] - body_center[0]) * math.cos(rot_angle) - (scene_verts[:, 2] - body_center[2]) * math.sin(rot_angle) + body_center[0]
    scene_verts_aug[:, 2] = (scene_verts[:, 0] - body_center[0]) * math.sin(rot_angle) + (scene_verts[:, 2] - body_center[2]) * math.cos(rot_angle) + body_center[2]
    scene_verts_aug[:, 1] = scene_verts[:, 1]
    min_x, max_x = body_center[0] - cube_size / 2, body_center[0] + cube_size / 2            # :191-194
    min_y, max_y = body_center[2] - cube_size / 2, body_center[2] + cube_size / 2
    xz = np.where((scene_verts_aug[:, 0] >= min_x) & (scene_verts_aug[:, 0] <= max_x) &
                  (scene_verts_aug[:, 2] >= min_y) & (scene_verts_aug[:, 2] <= max_y))[0]
    crop = scene_verts_aug[xz]
    keep = xz[crop[:, 1] <= np.min(crop[:, 1]) + cube_size]                                # :197 (np.min of an empty crop raises)
    if len(keep) < target:                                                                  # :203-205
        raise ValueError(f"scene vertex number {len(keep)} < scene_verts_num_target {target}")
    return select(keep, target), len(keep)


def cube_center_ref(transl_pv_row, trans_scene2pv):
    """:131 points_coord_trans(cur_stage1_transl_pv, np.linalg.inv(trans_scene2pv))[0] (utils/geometry.py:134-141)."""
    trans_mtx = np.linalg.inv(trans_scene2pv)
    return (transl_pv_row.dot(trans_mtx[:3, :3].transpose()) + trans_mtx[:3, 3].reshape((1, -1)))[0]


def out_rows(verts_sel, T_out, stride=1):
    """What the kernel writes: T_out v of the original vertices, elementwise float64 in o3d_transform's order, cast once to float32, [::stride]."""
    return o3d_transform(np.asarray(verts_sel, np.float64), T_out).astype(np.float32)[::stride]


def loader_rows(verts_sel, T_out, stride=1):
    """The loader's form: points_coord_trans(v, T) (egobody_dataset.py:212, :224) with numpy's dot, then .astype(float32)[::rate] (:272-273)."""
    v = np.asarray(verts_sel, np.float64)
    return (v.dot(T_out[:3, :3].transpose()) + T_out[:3, 3].reshape((1, -1))).astype(np.float32)[::stride]


# ------------------------------------------------------------------------------------------------ restatements on clouds of known selection
def test_whole_scene_restatement_on_a_constructed_cloud():
    n = 10000
    v = np.zeros((n, 3))
    v[:, 0] = np.arange(n) * 1e-3
    v[:, 2] = np.where(np.arange(n) % 3 == 1, 1.0, -1.0)                  # every third vertex (1, 4, 7, ...) in front
    v[5, 2] = 0.0                                                          # z == 0 is not in front
    chain = [np.eye(4)] * 4
    idx, cnt = whole_scene_ref(v, chain, 1000)
    sel = np.arange(1, n, 3)
    assert cnt == len(sel) == 3333
    assert np.array_equal(idx, sel[0::3][:1000])                           # k = int(3333 / 1000) = 3
    flip = np.diag([1.0, 1.0, -1.0, 1.0])                                  # applied twice: the identity
    idx2, _ = whole_scene_ref(v, [flip, np.eye(4), flip, np.eye(4)], 1000)
    assert np.array_equal(idx2, idx)
    with pytest.raises(ValueError):
        whole_scene_ref(v, chain, 4000)                                    # k = 0: open3d raises


def test_cube_restatement_on_a_constructed_cloud():
    g = np.arange(-40, 41) * 0.05                                          # a 4 m x 4 m grid in xz on two floors
    X, Z = np.meshgrid(g, g, indexing="ij")
    flat = np.stack([X.ravel(), np.zeros(X.size), Z.ravel()], -1)
    v = np.concatenate([flat, flat + [0, 1.5, 0], flat + [0, 2.5, 0]])    # y = 0, 1.5 kept; y = 2.5 > min + 2 dropped
    c = np.array([0.5, 0.0, -0.25])
    idx, cnt = cube_ref(v, c, 0.0, 2, 100)
    inside = (np.abs(v[:, 0] - 0.5) <= 1 + 1e-12) & (np.abs(v[:, 2] + 0.25) <= 1 + 1e-12) & (v[:, 1] <= 2.0)
    sel = np.nonzero(inside)[0]
    assert cnt == len(sel) == 2 * 41 * 41
    assert np.array_equal(idx, sel[0::int(len(sel) / 100)][:100])
    idx_q, cnt_q = cube_ref(v, c, math.pi / 2, 2, 100)                     # a quarter turn maps the grid's square onto itself
    assert cnt_q == cnt
    with pytest.raises(ValueError):
        cube_ref(v, np.array([50.0, 0, 50.0]), 0.0, 2, 100)               # empty crop
    with pytest.raises(ValueError):
        cube_ref(v, c, 0.0, 2, cnt + 1)


def test_out_rows_are_within_one_ulp_of_the_loader_form():
    g = np.random.default_rng(0)
    v = g.uniform(-5, 5, (5000, 3))
    T = _random_affine(g)
    a, b = out_rows(v, T), loader_rows(v, T)
    assert np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max() <= 1
    assert np.array_equal(out_rows(v, T, 3), a[::3])


# ------------------------------------------------------------------------------------------------ host half of egohmr_amd.scene
def _random_affine(g, y_only=False):
    a = g.uniform(0, 2 * np.pi)
    R = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])
    if not y_only:
        b = g.uniform(-0.3, 0.3)
        R = R @ np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, g.uniform(-2, 2, 3)
    return T


def test_egobody_transforms_bit_equal_to_the_reference_expressions():
    g = np.random.default_rng(1)
    k2h, h2p = _random_affine(g), _random_affine(g)                        # float64 in the pkl: cast to float32 by other_utils.py:42-46
    world = _random_affine(g)
    chain, crop, loader = es.egobody_transforms(k2h, h2p, world.tolist())
    trans_kinect2holo, trans_holo2pv = k2h.astype(np.float32), h2p.astype(np.float32)
    trans_scene_to_main = np.linalg.inv(np.array(world.tolist()))         # preprocess_scene_s2_for_test.py:119-122
    trans_scene2pv = np.matmul(trans_kinect2holo, trans_scene_to_main)     # :127-130
    trans_scene2pv = np.matmul(trans_holo2pv, trans_scene2pv)
    trans_scene2pv = np.matmul(ADD_TRANS, trans_scene2pv)
    pcd_trans_kinect2pv = np.matmul(trans_holo2pv, trans_kinect2holo)      # egobody_dataset.py:206-207
    pcd_trans_kinect2pv = np.matmul(ADD_TRANS, pcd_trans_kinect2pv)
    pcd_trans_scene2pv = np.matmul(pcd_trans_kinect2pv, trans_scene_to_main)   # :223
    assert crop.dtype == loader.dtype == chain.dtype == np.float64
    assert np.array_equal(crop, trans_scene2pv) and np.array_equal(loader, pcd_trans_scene2pv)
    for got, want in zip(chain, (trans_scene_to_main, trans_kinect2holo, trans_holo2pv, ADD_TRANS)):   # preprocess_scene_s1.py:104-107
        assert np.array_equal(got, want.astype(np.float64))
    assert not np.array_equal(crop, loader)                                # the two association orders round differently


def test_cube_params_are_the_scripts_scalars():
    g = np.random.default_rng(2)
    B = 5
    crop = np.stack([_random_affine(g) for _ in range(B)])
    out = np.stack([_random_affine(g) for _ in range(B)])
    tp = g.uniform(-1, 3, (B, 3)).astype(np.float32)
    ang = g.uniform(0, 2 * np.pi, B)
    p = es.cube_params(tp, crop, out, ang, 2, B)
    for b in range(B):
        c = cube_center_ref(tp[[b]], crop[b])
        want = [math.cos(ang[b]), math.sin(ang[b]), c[0], c[2], c[0] - 2 / 2, c[0] + 2 / 2, c[2] - 2 / 2, c[2] + 2 / 2, 2.0]
        assert np.array_equal(p[b, :9], np.array(want))
        assert np.array_equal(p[b, es.P_OUT:es.P_OUT + 12], out[b, :3].ravel()) and p[b, es.P_ANGLE] == ang[b]
    w, K = es.whole_scene_params(np.stack([crop[:, None]] * 3, 1)[:, :, 0], out, B)
    assert K == 3 and np.array_equal(w[:, 12:24], crop[:, :3].reshape(B, 12))


def test_group_items_by_mesh_in_item_order():
    idx = np.array([1, 0, 1, 1, 0] + [2] * 10)
    gr = es.group_items(idx)
    assert gr.shape == (4, 1 + es.GROUP)
    assert gr[0].tolist() == [0, 1, 4] + [-1] * 6
    assert gr[1].tolist() == [1, 0, 2, 3] + [-1] * 5
    assert gr[2].tolist() == [2] + list(range(5, 13)) and gr[3].tolist() == [2, 13, 14] + [-1] * 6


def test_argument_validation_without_a_device():
    from egohmr_amd._lib import EgoHMRHipError
    good = np.zeros((10, 3))
    with pytest.raises(EgoHMRHipError, match="no CPU path"):
        es.SceneClouds([good], "cpu")
    with pytest.raises(ValueError, match="mesh 1"):
        es.SceneClouds([good, np.zeros((10, 2))], "cpu")
    with pytest.raises(ValueError, match="non-finite"):
        es.SceneClouds([np.full((4, 3), np.nan)], "cpu")
    I = np.eye(4)
    with pytest.raises(ValueError, match="select_chain"):
        es.whole_scene_params(np.stack([I] * 5)[None].repeat(2, 0), np.stack([I] * 2), 2)      # K = 5 > 4
    bad = I.copy()
    bad[3, 2] = 1e-9
    with pytest.raises(ValueError, match="affine"):
        es.whole_scene_params(np.stack([I, bad])[None], I[None], 1)
    with pytest.raises(ValueError, match="out_transform"):
        es.whole_scene_params(I[None, None], np.stack([I] * 2), 1)
    with pytest.raises(ValueError, match="transl_pv"):
        es.cube_params(np.zeros((2, 2)), np.stack([I] * 2), np.stack([I] * 2), [0, 0], 2, 2)
    with pytest.raises(ValueError, match="angle"):
        es.cube_params(np.zeros((2, 3)), np.stack([I] * 2), np.stack([I] * 2), [0], 2, 2)
    with pytest.raises(ValueError, match="cube_size"):
        es.cube_params(np.zeros((2, 3)), np.stack([I] * 2), np.stack([I] * 2), [0, 0], 0, 2)


def test_read_obj_vertices_round_trip(tmp_path):
    from egohmr_amd.io import read_obj_vertices
    g = np.random.default_rng(3)
    v = g.uniform(-10, 10, (257, 3))
    p = tmp_path / "scene.obj"
    with open(p, "w") as f:
        f.write("# scene\nmtllib scene.mtl\n")
        for i, r in enumerate(v):
            f.write(f"v {float(r[0])!r} {float(r[1])!r} {float(r[2])!r}" + (" 0.5 0.5 0.5\n" if i % 2 else "\n"))   # trailing vertex colours on some lines
            f.write(f"vn 0 1 0\nvt 0.{i} 0.5\n")
        f.write("f 1 2 3\nf 4 5 6\n")
    got = read_obj_vertices(str(p))
    assert got.dtype == np.float64 and got.shape == v.shape
    assert np.array_equal(got, v.astype(np.float32).astype(np.float64))
    assert np.array_equal(read_obj_vertices(str(p)), got)
