"""The scene point clouds of the two-stage evaluation, made on the device from resident scene meshes.

The reference makes them offline, one ``.npy`` per frame, with open3d, and its loader maps them into the PV camera:

    stage 1  scene_type='whole_scene'  preprocess_scene_s1.py:94-118 + dataloaders/egobody_dataset.py:205-212     SceneClouds.whole_scene
    stage 2  scene_type='cube'         preprocess_scene_s2_for_test.py:124-208 + egobody_dataset.py:213-225       SceneClouds.cube

Both end in ``[::scene_downsample_rate]`` and a float32 cast (egobody_dataset.py:272-273): ``stride`` here.  The selection is the ordered
compaction of csrc/scene.hip (ehm_scene_select): float64 predicates rounded exactly as numpy evaluates the reference's expressions, open3d's
``uniform_down_sample(k)`` (indices 0, k, 2k, ... of the selected vertices, k = int(n / target)) and the first ``target`` rows.  The output
rows are ``T_out v`` of the original mesh vertices, rounded once to float32 - the reference's transform back and forth changes them by float64
ulps only.  Every scalar the host can derive (cos a, sin a, the centre, the bounds) is computed here, in numpy, as the reference writes it.
"""
from __future__ import annotations

import ctypes as C
import math
import random as _random

import numpy as np
import torch

from . import _lib

GROUP, PARAMS, MAX_CHAIN = 8, 64, 4           # EHM_SCENE_GROUP, EHM_SCENE_PARAMS, EHM_SCENE_MAX_CHAIN
P_OUT = 48                                    # EHM_SCENE_P_OUT
P_ANGLE = 63                                  # (an unused slot: the angle, for the caller)
WHOLE, CUBE = 0, 1
STATUS = {1: "fewer than target vertices selected", 2: "empty xz crop"}

# opengl -> opencv (preprocess_scene_s1.py:57-60, the loader's self.add_trans)
ADD_TRANS = np.array([[1.0, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]])


def egobody_transforms(kinect2holo, holo2pv, kinect12_to_world):
    """The matrices of one EgoBody frame, each in the reference's association order, from the sequence's ``trans_kinect2holo``, the frame's
    ``trans_world2pv`` (transf_matrices_all_seqs.pkl; cast to float32 as get_transf_matrices_per_frame does, utils/other_utils.py:42-46) and
    the recording's ``kinect12_to_world`` JSON ``trans`` (inverted in float64: preprocess_scene_s1.py:90-92).

    Returns ``(chain [4,4,4], crop [4,4], loader [4,4])``, float64:
      chain   scene_to_main, kinect2holo, holo2pv, add_trans: the mesh.transform calls of preprocess_scene_s1.py:104-107 (whole_scene's
              ``select_chain``)
      crop    add_trans @ (holo2pv @ (kinect2holo @ scene_to_main)) (preprocess_scene_s2_for_test.py:127-130; cube's ``scene2pv_crop``)
      loader  (add_trans @ (holo2pv @ kinect2holo)) @ scene_to_main (egobody_dataset.py:206-207, :223): mesh coordinates -> PV camera, the
              ``out_transform`` of both modes (stage 1's loader applies its first factor to points stored as scene_to_main v)."""
    k2h = np.asarray(kinect2holo).astype(np.float32)
    h2p = np.asarray(holo2pv).astype(np.float32)
    s2m = np.linalg.inv(np.array(kinect12_to_world))
    crop = np.matmul(k2h, s2m)
    crop = np.matmul(h2p, crop)
    crop = np.matmul(ADD_TRANS, crop)
    k2pv = np.matmul(h2p, k2h)
    k2pv = np.matmul(ADD_TRANS, k2pv)
    loader = np.matmul(k2pv, s2m)
    chain = np.stack([np.asarray(m, np.float64) for m in (s2m, k2h, h2p, ADD_TRANS)])
    return chain, np.asarray(crop, np.float64), np.asarray(loader, np.float64)


def _host(x, dtype):
    return np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x), dtype)


def _affine(x, shape, name):
    """float64 4x4 matrices of the given batch shape whose last row is exactly [0, 0, 0, 1]: open3d's transform divides by w, which is then 1
    exactly; anything else is not supported."""
    m = _host(x, np.float64)
    if m.ndim != len(shape) + 2 or m.shape[:len(shape)] != shape or m.shape[-2:] != (4, 4):
        raise ValueError(f"{name} has shape {m.shape}, expected {tuple(shape) + (4, 4)}")
    if not np.all(m[..., 3, :] == np.array([0.0, 0.0, 0.0, 1.0])):
        raise ValueError(f"{name}: every matrix must be affine (last row exactly [0, 0, 0, 1])")
    return m


def whole_scene_params(select_chain, out_transform, B):
    """The per-item float64 parameters of ehm_scene_select's EHM_SCENE_WHOLE mode: the chain's 3x4 rows, T_out.  -> (params [B, 64], K)."""
    chain = _host(select_chain, np.float64)
    if chain.ndim != 4 or chain.shape[0] != B or not 1 <= chain.shape[1] <= MAX_CHAIN:
        raise ValueError(f"select_chain has shape {chain.shape}, expected [{B}, K <= {MAX_CHAIN}, 4, 4]")
    chain = _affine(chain, chain.shape[:2], "select_chain")
    out = _affine(out_transform, (B,), "out_transform")
    K = chain.shape[1]
    params = np.zeros((B, PARAMS), np.float64)
    params[:, :12 * K] = chain[:, :, :3, :].reshape(B, 12 * K)
    params[:, P_OUT:P_OUT + 12] = out[:, :3, :].reshape(B, 12)
    return params, K


def cube_params(transl_pv, scene2pv_crop, out_transform, angle, cube_size, B):
    """The per-item float64 parameters of EHM_SCENE_CUBE, each as preprocess_scene_s2_for_test.py computes it: cos a, sin a (math, :185-187),
    the centre's x and z (:131), the bounds c -/+ cube_size / 2 (:191-194), cube_size (:197), then T_out.  The angle is kept at P_ANGLE."""
    tp = _host(transl_pv, np.float32)
    if tp.shape != (B, 3):
        raise ValueError(f"transl_pv has shape {tp.shape}, expected ({B}, 3)")
    crop = _affine(scene2pv_crop, (B,), "scene2pv_crop")
    out = _affine(out_transform, (B,), "out_transform")
    angles = _host(angle, np.float64).reshape(-1)
    if angles.shape != (B,):
        raise ValueError(f"angle has {angles.size} values, expected {B}")
    if not cube_size > 0:
        raise ValueError(f"cube_size must be a positive number, not {cube_size!r}")
    params = np.zeros((B, PARAMS), np.float64)
    half = cube_size / 2
    for b in range(B):
        c = cube_center(tp[[b]], crop[b])
        a = float(angles[b])
        params[b, :9] = [math.cos(a), math.sin(a), c[0], c[2], c[0] - half, c[0] + half, c[2] - half, c[2] + half, cube_size]
        params[b, P_ANGLE] = a
    params[:, P_OUT:P_OUT + 12] = out[:, :3, :].reshape(B, 12)
    return params


def group_items(mesh_index):
    """The item groups of ehm_scene_select: per mesh (ascending), its items in item order, GROUP at a time -> int32 [groups, 1 + GROUP]."""
    idx = np.asarray(mesh_index).reshape(-1)
    groups = []
    for m in np.unique(idx):
        its = np.nonzero(idx == m)[0]
        for s in range(0, len(its), GROUP):
            chunk = its[s:s + GROUP]
            groups.append([int(m)] + [int(i) for i in chunk] + [-1] * (GROUP - len(chunk)))
    return np.asarray(groups, np.int32)


class SceneClouds:
    """Scene meshes resident on one HIP device (their float64 vertices only, uploaded once) and the per-batch stage-1 / stage-2 clouds.

    ``meshes``: a sequence of [V_i, 3] vertex arrays (numpy or torch; float64 - read OBJ files with egohmr_amd.io.read_obj_vertices).  An
    item names its mesh by position in this sequence.  Vertices must be finite."""

    def __init__(self, meshes, device):
        device = torch.device(device)
        arrs = []
        for i, m in enumerate(meshes):
            a = m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
            a = np.asarray(a, np.float64)
            if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] == 0:
                raise ValueError(f"mesh {i} has shape {a.shape}, expected [V, 3] with V > 0")
            if not np.isfinite(a).all():
                raise ValueError(f"mesh {i} has non-finite vertices")
            arrs.append(a)
        if not arrs:
            raise ValueError("no meshes")
        self.num_verts = np.array([len(a) for a in arrs], np.int64)
        if self.num_verts.max() > 2**31 - 4096:
            raise ValueError(f"a mesh of {self.num_verts.max()} vertices: at most 2^31 - 4096 are supported")
        self.offsets = np.concatenate([[0], np.cumsum(self.num_verts)]).astype(np.int64)
        if device.type != "cuda":
            raise _lib.EgoHMRHipError("SceneClouds runs on the HIP kernels only (got a CPU device); there is no CPU path")
        self.device = device
        soa = np.concatenate(arrs, 0).T.copy()                         # [3, total]: x[], y[], z[]
        self.verts = torch.from_numpy(soa).to(device)
        self.offsets_dev = torch.from_numpy(self.offsets).to(device)
        self._ws = None

    @property
    def num_meshes(self) -> int:
        return len(self.num_verts)

    # ---------------------------------------------------------------------------------------------------------------- public modes
    def whole_scene(self, mesh_index, select_chain, out_transform, target: int = 20000, stride: int = 1, return_index: bool = False):
        """Stage 1 (scene_type='whole_scene').  Per item b: apply the matrices ``select_chain[b]`` [K <= 4, 4, 4] one after another to the mesh
        vertices (the mesh.transform calls of preprocess_scene_s1.py:104-107), keep ``z > 0`` (:113), select ``target`` of them (:118-124)
        and return ``out_transform[b]`` applied to the ORIGINAL vertices (egobody_dataset.py:210-212, composed with scene_to_main: the
        ``loader`` matrix of egobody_transforms), then ``[::stride]``.  The reference recomputes the cloud only every 15th frame (:76): a
        frame between two key frames selects with the key frame's chain and outputs with its own ``out_transform``.

        Returns ``(points f32 [B, ceil(target/stride), 3], n_selected int64 [B], index int64 [B, rows] if return_index)`` on the device;
        index is the source vertex within its mesh.  Raises EgoHMRHipError naming the items with fewer than ``target`` vertices selected."""
        idx = self._mesh_index(mesh_index)
        params, K = whole_scene_params(select_chain, out_transform, len(idx))
        return self._run(WHOLE, idx, params, K, target, stride, return_index)

    def cube(self, mesh_index, transl_pv, scene2pv_crop, out_transform, angle=None, rng: _random.Random | None = None, cube_size: float = 2.0,
             target: int = 20000, stride: int = 1, return_index: bool = False):
        """Stage 2 (scene_type='cube').  Per item b, as preprocess_scene_s2_for_test.py:124-208: the centre
        ``c = points_coord_trans(transl_pv[[b]], inv(scene2pv_crop[b]))[0]`` (transl_pv: the float32 stage-1 translation in the PV camera;
        the ground truth for the train-time variant), the mesh rotated about y through c by ``angle[b]`` (``rng.uniform(0, 2 pi)`` per item
        in item order when None, as the script draws once per frame; ``rng`` None: the ``random`` module, as the script), the inclusive
        ``cube_size`` square in xz, ``y <= min(y) + cube_size``, select ``target`` of them; the rows are ``out_transform[b]`` (the ``loader``
        matrix of egobody_transforms) applied to the original vertices (egobody_dataset.py:223-224), then ``[::stride]``.

        Returns as whole_scene.  Raises EgoHMRHipError naming the items whose crop is empty or holds fewer than ``target`` vertices
        (the script aborts, :203-205)."""
        idx = self._mesh_index(mesh_index)
        B = len(idx)
        if angle is None:
            r = rng if rng is not None else _random
            angle = [r.uniform(0, 2 * (math.pi)) for _ in range(B)]
        params = cube_params(transl_pv, scene2pv_crop, out_transform, angle, cube_size, B)
        self.last_angles = [float(a) for a in params[:, P_ANGLE]]
        return self._run(CUBE, idx, params, 0, target, stride, return_index)

    # ---------------------------------------------------------------------------------------------------------------- internals
    def _mesh_index(self, mesh_index):
        idx = mesh_index.detach().cpu().numpy() if isinstance(mesh_index, torch.Tensor) else np.asarray(mesh_index)
        idx = np.asarray(idx).reshape(-1)
        if idx.size == 0:
            raise ValueError("empty batch")
        if not np.issubdtype(idx.dtype, np.integer) or idx.min() < 0 or idx.max() >= self.num_meshes:
            raise ValueError(f"mesh_index must hold integers in [0, {self.num_meshes})")
        return idx.astype(np.int64)

    def _prepare(self, mode, idx, params, chain_len, target, stride, return_index):
        """The descriptor of one ehm_scene_select call and its output tensors (the parameters and groups uploaded; the workspace sized)."""
        target, stride = int(target), int(stride)
        if target < 1 or stride < 1:
            raise ValueError(f"target ({target}) and stride ({stride}) must be >= 1")
        B, dev = len(idx), self.device
        groups = group_items(idx)
        rows = -(-target // stride)
        params_d = torch.from_numpy(params).to(dev)
        groups_d = torch.from_numpy(groups).to(dev)
        out = dict(points=torch.empty(B, rows, 3, dtype=torch.float32, device=dev),
                   index=torch.empty(B, rows, dtype=torch.int64, device=dev) if return_index else None,
                   n_selected=torch.empty(B, dtype=torch.int64, device=dev), status=torch.empty(B, dtype=torch.int32, device=dev),
                   keep=(params_d, groups_d))
        P = _lib.ptr
        d = _lib.SceneDesc(verts=P(self.verts), total_verts=int(self.offsets[-1]), mesh_offsets=P(self.offsets_dev), num_meshes=self.num_meshes,
                           max_mesh_verts=int(self.num_verts.max()), groups=P(groups_d), num_groups=len(groups), params=P(params_d), mode=mode,
                           chain_len=int(chain_len), B=B, target=target, stride=stride, points=P(out["points"]), index=P(out["index"]),
                           n_selected=P(out["n_selected"]), status=P(out["status"]), workspace=None, workspace_bytes=0)
        nb = C.c_int64(0)
        _lib.api().ehm_scene_workspace_bytes(C.byref(d), C.byref(nb))
        if self._ws is None or self._ws.numel() < nb.value:
            self._ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        d.workspace, d.workspace_bytes = P(self._ws), self._ws.numel()
        return d, out

    def _run(self, mode, idx, params, chain_len, target, stride, return_index):
        with _lib.on_device(self.device):
            st = _lib.stream_ptr()
            d, out = self._prepare(mode, idx, params, chain_len, target, stride, return_index)
            _lib.api().ehm_scene_select(C.byref(d), st)
            stat, n = out["status"].cpu().numpy(), out["n_selected"].cpu().numpy()
        bad = np.nonzero(stat != 0)[0]
        if len(bad):
            what = ", ".join(f"item {b}: {STATUS.get(int(stat[b]), f'status {int(stat[b])}')}, n_selected = {int(n[b])}" for b in bad[:16])
            raise _lib.EgoHMRHipError(f"scene selection failed for {len(bad)} of {len(idx)} items (target {d.target}): {what}"
                                      f"{' ...' if len(bad) > 16 else ''}")
        return (out["points"], out["n_selected"], out["index"]) if return_index else (out["points"], out["n_selected"])


def cube_center(transl_pv_row, scene2pv):
    """preprocess_scene_s2_for_test.py:131: points_coord_trans(transl_pv[[i]], inv(T))[0] (utils/geometry.py:137-141), float32 row, float64 T."""
    inv = np.linalg.inv(scene2pv)
    return (transl_pv_row.dot(inv[:3, :3].transpose()) + inv[:3, 3].reshape(1, -1))[0]
