"""The reference's qualitative output on the device: sampled bodies drawn over the frame, or inside the scene mesh.

What it stands in for: ``utils/renderer.py:15-47`` (``render_on_img``, ``render_in_scene``) as ``test_egohmr.py:153-166, :555-619`` calls them with
``--render True``, where pyrender, EGL and trimesh draw the SMPL mesh.  Here ``csrc/render.hip`` (``ehm_render``) rasterises it: the rule is
written out in ``include/egohmr_hip.h``, restated in float64 by ``tests/render_ref.py``, and its pixels are that rule's, not pyrender's - a Lambert
term under one directional light, no PBR shader, no gamma, no anti-aliasing.  By default there is no near-plane clipping either: a face with a vertex
at ``z <= z_near`` is dropped whole, which shows in ``render_in_scene`` as holes where the scene mesh reaches behind the camera.  ``clip_near=True``
(``MeshRenderer``, and through ``**kw`` ``scene_renderer`` and ``render_in_scene``) draws such a face where it lies in front of the plane, by the
header's homogeneous rule on the face's own vertices; faces wholly in front keep their bits.

The camera frame is the package's: x right, y down, z forward - what ``Stage2Driver.step`` returns in ``decoded['vertices_full']`` and what the
reference's ``camera_pose = diag(1, -1, -1, 1)`` converts to OpenGL's.  The defaults are the reference's scene: ambient light 0.3, a directional light
of intensity 4 on the camera axis - on a metallic-0 Lambert term that is ``4 / pi`` per unit ``n.l``, Fresnel and roughness ignored - and the material
``baseColorFactor = (1.0, 193/255, 193/255)`` of test_egohmr.py:157-160.

``MeshRenderer.render`` reads one small array back per call (the list capacity every item needed) and runs again when an item's face lists did not
fit; rendering is not inside any timed loop.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import EgoHMRHipError

BASE_COLOR = (1.0, 193.0 / 255.0, 193.0 / 255.0)      # test_egohmr.py:157-160, RGB
DIFFUSE = 4.0 / math.pi                                # pyrender.DirectionalLight(intensity=4.0) on a Lambert term
AMBIENT = 0.3                                          # utils/renderer.py:19
Z_NEAR = 0.05                                          # pyrender's DEFAULT_Z_NEAR


def build_vertex_face_csr(faces: np.ndarray, num_vertices: int):
    """faces int [F,3] -> (offsets int32 [V+1], face ids int32 [3F]): the faces incident to every vertex, in face-index order."""
    flat = np.asarray(faces, np.int64).reshape(-1)
    order = np.argsort(flat, kind="stable")            # stable over a face-major array: face-index order inside a vertex
    offsets = np.zeros(num_vertices + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=num_vertices), out=offsets[1:])
    return offsets.astype(np.int32), (order // 3).astype(np.int32)


def _per_item(x, B, dev, what):
    t = torch.as_tensor(x, dtype=torch.float32).to(dev).reshape(-1)
    if t.numel() == 1:
        t = t.expand(B)
    if t.numel() != B:
        raise ValueError(f"{what} must be a scalar or hold one value per item ({B}), not {t.numel()}")
    return t.contiguous()


class MeshRenderer:
    """One mesh topology (``faces`` int [F,3], shared by every item of a call) with its material and light.  ``faces`` is validated on the host, once
    (``0 <= index < V``), and the vertex -> face lists of the smooth normals are built there.  ``vertex_colors`` float [V,3] in [0,1] replaces
    ``base_color``; both are RGB.  ``light_dir`` points from the surface towards the light.  ``clip_near``: a face that straddles ``z = z_near`` is
    drawn where it lies in front of the plane, not dropped (off by default; a mesh without such a face renders to the same bits either way)."""

    def __init__(self, faces, device, vertex_colors=None, base_color=BASE_COLOR, ambient=AMBIENT, light_dir=(0.0, 0.0, -1.0), diffuse=DIFFUSE,
                 smooth=True, two_sided=False, cull_backface=False, z_near=Z_NEAR, num_vertices=None, bin_capacity=None, clip_near=False):
        f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] == 0 or not np.issubdtype(f.dtype, np.integer):
            raise ValueError(f"faces must be an integer array [F,3] with F > 0, not {f.dtype} {f.shape}")
        colors = None
        if vertex_colors is not None:
            colors = vertex_colors.detach().cpu().numpy() if isinstance(vertex_colors, torch.Tensor) else np.asarray(vertex_colors)
            colors = np.ascontiguousarray(colors, np.float32)
            if colors.ndim != 2 or colors.shape[1] != 3:
                raise ValueError(f"vertex_colors must be [V,3], not {colors.shape}")
        V = int(num_vertices) if num_vertices is not None else (colors.shape[0] if colors is not None else int(f.max()) + 1)
        if f.min() < 0 or f.max() >= V:
            raise ValueError(f"faces index vertices {int(f.min())} .. {int(f.max())} of a mesh with {V}")
        if colors is not None and colors.shape[0] != V:
            raise ValueError(f"vertex_colors has {colors.shape[0]} rows for {V} vertices")
        self.device = torch.device(device)
        self.V, self.F = V, int(f.shape[0])
        self.faces = torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(self.device)
        off, vf = build_vertex_face_csr(f, V)
        self.vf_offsets, self.vf_faces = torch.from_numpy(off).to(self.device), torch.from_numpy(vf).to(self.device)
        self._colors = {False: None, True: None}
        if colors is not None:                          # RGB, and flipped for frames in BGR
            self._colors = {False: torch.from_numpy(colors).to(self.device),
                            True: torch.from_numpy(np.ascontiguousarray(colors[:, ::-1])).to(self.device)}
        self.base_color = tuple(float(c) for c in base_color)
        l = np.asarray(light_dir, np.float64)
        self.light_dir = tuple(float(c) for c in l / np.linalg.norm(l))
        self.ambient, self.diffuse, self.z_near = float(ambient), float(diffuse), float(z_near)
        self.smooth, self.two_sided, self.cull_backface = bool(smooth), bool(two_sided), bool(cull_backface)
        self.clip_near = bool(clip_near)
        self.bin_capacity = int(bin_capacity) if bin_capacity is not None else 4 * self.F + 64
        self.reruns = 0                                 # calls whose lists did not fit the capacity and ran twice

    def _desc(self, vertices, fx, fy, cx, cy, frames, frame_index, H, W, bg_color, bgr, outs, needed, capacity):
        P = _lib.ptr
        base = self.base_color[::-1] if bgr else self.base_color
        d = _lib.RenderDesc(vertices=P(vertices), faces=P(self.faces), vf_offsets=P(self.vf_offsets), vf_faces=P(self.vf_faces),
                            vertex_colors=P(self._colors[bool(bgr)]), fx=P(fx), fy=P(fy), cx=P(cx), cy=P(cy), frames=P(frames), frame_index=P(frame_index),
                            B=vertices.shape[0], V=self.V, F=self.F, Fr=0 if frames is None else frames.shape[0], H=H, W=W,
                            smooth=int(self.smooth), two_sided=int(self.two_sided), cull_backface=int(self.cull_backface), z_near=self.z_near,
                            base_color=(C.c_float * 3)(*base), light_dir=(C.c_float * 3)(*self.light_dir), ambient=self.ambient, diffuse=self.diffuse,
                            bg_color=(C.c_uint8 * 4)(*[int(c) for c in bg_color], 0), bin_capacity=int(capacity), needed_capacity=P(needed),
                            color=P(outs.get("color")), depth=P(outs.get("depth")), face_index=P(outs.get("face_index")),
                            clip_near=int(self.clip_near))
        return d

    @torch.no_grad()
    def render(self, vertices, fx, fy, cx, cy, frames=None, frame_index=None, size=None, bg_color=(0, 0, 0), want=("color",), bgr=False):
        """vertices float32 [B,V,3] (camera frame) on the renderer's device; fx, fy, cx, cy scalars or [B]; the background is frame
        ``frame_index[b]`` of ``frames`` uint8 [Fr,H,W,3] (``frame_index`` defaults to 0 .. B-1 when Fr == B, to 0 when Fr == 1), or ``bg_color``
        (three levels, in the output's channel order) at ``size = (H, W)``.  ``bgr``: the frames are BGR, so the RGB material is flipped.
        -> {'color': uint8 [B,H,W,3], 'depth': float32 [B,H,W] (0 on background), 'face_index': int32 [B,H,W] (-1)} for the names in ``want``."""
        want = tuple(want)
        if not want or any(w not in ("color", "depth", "face_index") for w in want):
            raise ValueError(f"want must name some of 'color', 'depth', 'face_index', not {want}")
        if not isinstance(vertices, torch.Tensor) or not vertices.is_cuda or (frames is not None and not frames.is_cuda):
            raise EgoHMRHipError("MeshRenderer.render needs its vertices and frames on a HIP device; there is no CPU path")
        dev = vertices.device
        vertices = _lib.f32(vertices)
        if vertices.dim() != 3 or vertices.shape[1] != self.V or vertices.shape[2] != 3:
            raise ValueError(f"vertices must be [B,{self.V},3], not {tuple(vertices.shape)}")
        B = int(vertices.shape[0])
        if frames is not None:
            if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError(f"frames must be uint8 [Fr,H,W,3], not {frames.dtype} {tuple(frames.shape)}")
            frames = frames.contiguous()
            H, W = int(frames.shape[1]), int(frames.shape[2])
            if size is not None and tuple(size) != (H, W):
                raise ValueError(f"size {tuple(size)} is not the frames' {(H, W)}")
            if frame_index is None:
                if frames.shape[0] not in (1, B):
                    raise ValueError(f"{frames.shape[0]} frames for {B} items need a frame_index")
                frame_index = torch.arange(B, dtype=torch.int32, device=dev) if frames.shape[0] == B else torch.zeros(B, dtype=torch.int32, device=dev)
            frame_index = torch.as_tensor(frame_index).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
            if frame_index.numel() != B:
                raise ValueError(f"frame_index holds {frame_index.numel()} values for {B} items")
        else:
            if size is None:
                raise ValueError("without frames, size = (H, W) is needed")
            H, W = int(size[0]), int(size[1])
            frame_index = None
        fx, fy, cx, cy = (_per_item(v, B, dev, n) for v, n in ((fx, "fx"), (fy, "fy"), (cx, "cx"), (cy, "cy")))
        shapes = {"color": ((B, H, W, 3), torch.uint8), "depth": ((B, H, W), torch.float32), "face_index": ((B, H, W), torch.int32)}
        outs = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in want}
        needed = torch.empty(B, dtype=torch.int32, device=dev)
        A = _lib.api()
        with _lib.on_device(dev):
            for attempt in range(2):
                d = self._desc(vertices, fx, fy, cx, cy, frames, frame_index, H, W, bg_color, bgr, outs, needed, self.bin_capacity)
                nbytes = C.c_int64(0)
                A.ehm_render_workspace_bytes(C.byref(d), C.byref(nbytes))
                ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
                d.workspace, d.workspace_bytes = _lib.ptr(ws), int(nbytes.value)
                A.ehm_render(C.byref(d), _lib.stream_ptr())
                need = int(needed.max())                # the one host read-back: did every item's face lists fit?
                if need <= self.bin_capacity:
                    break
                if attempt == 1 or need >= 1 << 30:
                    raise EgoHMRHipError(f"ehm_render: the face lists need {need} entries per item")
                self.bin_capacity, self.reruns = need, self.reruns + 1
        return outs


def render_on_img(fx, fy, cx, cy, input_img, body_vertices, renderer: MeshRenderer, frame_index=None, bgr=True):
    """utils/renderer.py:15-30: the body over the input image.  ``input_img`` uint8 [H,W,3] or [Fr,H,W,3] on the device, BGR as cv2 decodes it
    (``bgr=False``: RGB); ``body_vertices`` [V,3] or [B,V,3] in the camera frame; the reference's trimesh, material and light are the renderer's
    faces, colour and light, its ``camera_pose`` is the frame convention.  -> uint8 [H,W,3] for one [V,3] body, else [B,H,W,3]."""
    one = body_vertices.dim() == 2
    v = body_vertices.unsqueeze(0) if one else body_vertices
    frames = input_img.unsqueeze(0) if input_img.dim() == 3 else input_img
    img = renderer.render(v, fx, fy, cx, cy, frames=frames, frame_index=frame_index, bgr=bgr)["color"]
    return img[0] if one else img


def scene_renderer(body_faces, num_body_vertices, scene_faces, scene_colors, device, body_color=BASE_COLOR, ambient=0.0, **kw) -> MeshRenderer:
    """The renderer of a body placed in a scene mesh: the two meshes concatenated (the scene's faces offset by the body's vertex count), the body in
    ``body_color``, the scene in its per-vertex colours [Vs,3] (None: mid grey).  ``ambient`` defaults to 0, a bare ``pyrender.Scene()``'s."""
    bf = body_faces.detach().cpu().numpy() if isinstance(body_faces, torch.Tensor) else np.asarray(body_faces)
    sf = scene_faces.detach().cpu().numpy() if isinstance(scene_faces, torch.Tensor) else np.asarray(scene_faces)
    Vb = int(num_body_vertices)
    if scene_colors is None:
        Vs = int(sf.max()) + 1
        sc = np.full((Vs, 3), 0.5, np.float32)
    else:
        sc = scene_colors.detach().cpu().numpy() if isinstance(scene_colors, torch.Tensor) else np.asarray(scene_colors)
        sc = np.asarray(sc, np.float32)[:, :3]
    colors = np.concatenate([np.tile(np.asarray(body_color, np.float32), (Vb, 1)), sc], 0)
    faces = np.concatenate([bf.astype(np.int64), sf.astype(np.int64) + Vb], 0)
    return MeshRenderer(faces, device, vertex_colors=colors, ambient=ambient, **kw)


def render_in_scene(fx, fy, cx, cy, body_vertices, scene_vertices, scene_faces=None, scene_colors=None, body_faces=None, size=(1080, 1920),
                    body_transform=None, renderer: MeshRenderer = None, bg_color=(255, 255, 255), bgr=True, **kw):
    """utils/renderer.py:33-47: the body inside the static scene mesh, seen by the camera ``fx, fy, cx, cy`` whose frame ``scene_vertices`` [Vs,3]
    are in.  ``body_vertices`` [V,3] or [B,V,3]; ``body_transform`` 4 x 4 takes them into that frame - the reference's chain of ``add_trans``,
    ``inv(transf_holo2pv)`` and ``inv(transf_kinect2holo)`` (test_egohmr.py:607-611) multiplied out by the caller.  ``renderer``: a
    ``scene_renderer`` kept between calls (it is built from ``body_faces``, ``scene_faces``, ``scene_colors`` and ``kw`` otherwise, which sorts the
    faces on the host).  The background is white, a bare ``pyrender.Scene()``'s.  -> uint8 [H,W,3] for one [V,3] body, else [B,H,W,3]."""
    one = body_vertices.dim() == 2
    v = _lib.f32(body_vertices.unsqueeze(0) if one else body_vertices)
    dev = v.device
    if body_transform is not None:
        T = torch.as_tensor(body_transform, dtype=torch.float64).to(dev)
        v = (v.double() @ T[:3, :3].T + T[:3, 3]).float()
    s = _lib.f32(scene_vertices, dev)
    if renderer is None:
        if body_faces is None or scene_faces is None:
            raise ValueError("render_in_scene needs a scene_renderer, or body_faces and scene_faces to build one")
        renderer = scene_renderer(body_faces, v.shape[1], scene_faces, scene_colors, dev, **kw)
    both = torch.cat([v, s.unsqueeze(0).expand(v.shape[0], -1, -1)], 1).contiguous()
    img = renderer.render(both, fx, fy, cx, cy, size=size, bg_color=bg_color, bgr=bgr)["color"]
    return img[0] if one else img


def contact_sheet(input_frames, on_img, in_scene=None, halve=True):
    """test_egohmr.py:619-625: per sample the row [input | overlay | in-scene] (a column given as None is left out), the S rows stacked, the sheet
    halved.  ``input_frames`` uint8 [S,H,W,3] (or one [H,W,3] frame for every sample), ``on_img`` and ``in_scene`` uint8 [S,H,W,3], all on one
    device -> uint8 [S H // 2, n W // 2, 3] (``halve=False``: [S H, n W, 3]).  The halving is the 2 x 2 mean (a + b + c + d + 2) >> 2 on integer
    torch ops; an odd height or width drops its last row or column first, as ``dsize = shape // 2`` does.  It stands for the script's
    cv2.resize(.., INTER_AREA); cv2's rounding was NOT compared, because cv2 is not installed."""
    if input_frames is not None and input_frames.dim() == 3:
        input_frames = input_frames.unsqueeze(0).expand(on_img.shape[0], -1, -1, -1)
    parts = [p for p in (input_frames, on_img, in_scene) if p is not None]
    for p in parts:
        if p.dtype != torch.uint8 or p.dim() != 4 or p.shape[-1] != 3 or p.shape[:3] != on_img.shape[:3]:
            raise ValueError(f"contact_sheet takes uint8 [S,H,W,3] tensors of one size, got {p.dtype} {tuple(p.shape)}")
    sheet = torch.cat([p.to(on_img.device) for p in parts], 2)
    sheet = sheet.reshape(-1, sheet.shape[2], 3)
    if not halve:
        return sheet.contiguous()
    h, w = sheet.shape[0] // 2, sheet.shape[1] // 2
    q = sheet[:2 * h, :2 * w].to(torch.int32).reshape(h, 2, w, 2, 3)
    return ((q.sum((1, 3)) + 2) >> 2).to(torch.uint8)
