"""Files on either side of the sampling path.

* `save_results` / `load_results`: the `results_seed_{seed}.pkl` dictionary test_egohmr.py:672-695 writes (pickle protocol 2,
  numpy arrays, exactly these keys) - what downstream visualisation / evaluation scripts of the reference read.
* `load_stage1_cam`: `results.pkl['pred_cam_full_list']` written by the stage-1 script (test_prohmr_scene.py:417-426) and
  consumed by `--two_stage` runs; `save_stage1_results` writes that file from egohmr_amd.stage1's translations.
* `load_stage1_checkpoint`: a ProHMR-scene checkpoint into egohmr_amd.stage1.ProHMRSceneTransl, or with `flow=True` - the pose flow's
  `flow.flow.*` included - into egohmr_amd.stage1.ProHMRScene (test_prohmr_scene.py:81-85).
* `read_obj_vertices`: the vertex array of a scene mesh OBJ (scene_mesh/{scene}/{scene}.obj), for egohmr_amd.scene.SceneClouds.
* `read_obj_mesh`: the same file with its faces and vertex colours, for egohmr_amd.render (test_egohmr.py:595-597 loads it with trimesh).
* `load_preprocess_stats`, `load_smpl_mean_params`, `load_checkpoint`: test_egohmr.py:109-111, models/egohmr/egohmr.py:669-671,
  test_egohmr.py:125-127.

Pure host-side numpy / pickle code: nothing here is on the measured path."""
from __future__ import annotations

import os
import pickle
from typing import Mapping

import numpy as np
import torch

from .synthetic import FLOW_DIM, FLOW_PREFIX

RESULT_KEYS = ("pred_betas_list", "pred_global_orient_list", "pred_body_pose_list", "collision_ratio_list", "contact_ratio_list",
               "gt_cam_full_list")                  # + 'pred_cam_full_list' for --two_stage runs


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def results_dict(pred_betas, pred_global_orient, pred_body_pose, collision_ratio, contact_ratio, gt_cam_full, pred_cam_full=None):
    """Assemble the dictionary of test_egohmr.py:685-693.  Shapes as the reference concatenates them:
    pred_betas [n, S, 10], pred_global_orient [n, S, 1, 3, 3], pred_body_pose [n, S, 23, 3, 3], collision / contact ratio [n, S],
    gt_cam_full [n, 3] (pred_cam_full [n, 3] when stage 1 supplied the translation)."""
    d = {"pred_betas_list": _np(pred_betas), "pred_global_orient_list": _np(pred_global_orient),
         "pred_body_pose_list": _np(pred_body_pose), "collision_ratio_list": _np(collision_ratio),
         "contact_ratio_list": _np(contact_ratio)}
    if pred_cam_full is not None:
        d["pred_cam_full_list"] = _np(pred_cam_full)
    d["gt_cam_full_list"] = _np(gt_cam_full)
    return d


def save_results(save_root: str, model_id: str, seed: int, results: Mapping[str, np.ndarray]) -> str:
    """`{save_root}/output_egohmr_{model_id}/results_seed_{seed}.pkl`, pickle protocol 2 (test_egohmr.py:680-695)."""
    missing = [k for k in RESULT_KEYS if k not in results]
    if missing:
        raise KeyError(f"results are missing {missing}")
    folder = os.path.join(save_root, f"output_egohmr_{model_id}")
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, f"results_seed_{seed}.pkl")
    with open(path, "wb") as f:
        pickle.dump({k: _np(v) for k, v in results.items()}, f, protocol=2)
    return path


def load_results(path: str) -> dict:
    with open(path, "rb") as f:
        d = pickle.load(f, encoding="latin1")
    missing = [k for k in RESULT_KEYS if k not in d]
    if missing:
        raise KeyError(f"{path}: not a results_seed_*.pkl (missing {missing})")
    return d


def load_stage1_cam(path: str) -> np.ndarray:
    """`pred_cam_full_list` [n, 3] of the stage-1 `results.pkl` (test_prohmr_scene.py:417-426), the body translation a
    `--two_stage` stage-2 run conditions on (test_egohmr.py:100-104)."""
    with open(path, "rb") as f:
        d = pickle.load(f, encoding="latin1")
    if "pred_cam_full_list" not in d:
        raise KeyError(f"{path}: no 'pred_cam_full_list' (is this a stage-1 results.pkl?)")
    cam = np.asarray(d["pred_cam_full_list"], dtype=np.float32)
    if cam.ndim != 2 or cam.shape[1] != 3:
        raise ValueError(f"{path}: pred_cam_full_list has shape {cam.shape}, expected [n, 3]")
    return cam


def save_stage1_results(save_root: str, model_id: str, pred_cam_full) -> str:
    """`{save_root}/output_prohmr_scene_{model_id}/results.pkl` = {'pred_cam_full_list': float32 [n, 3]} (test_prohmr_scene.py:417-426)."""
    cam = np.asarray(_np(pred_cam_full), dtype=np.float32)
    if cam.ndim != 2 or cam.shape[1] != 3:
        raise ValueError(f"pred_cam_full has shape {cam.shape}, expected [n, 3]")
    folder = os.path.join(save_root, f"output_prohmr_scene_{model_id}")
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, "results.pkl")
    with open(path, "wb") as f:
        pickle.dump({"pred_cam_full_list": cam}, f, protocol=2)
    return path


STAGE1_IGNORED_PREFIXES = ("flow.flow.", "discriminator.", "smpl")      # the flow, the GAN discriminator, the body models (smpl, smpl_male, ...)


FLOW_TRANSFORM_PREFIX = FLOW_PREFIX
FLOW_IGNORED_KEYS = ("flow.flow._distribution._log_z",)                 # the base distribution's constant: the kernels carry 72 log 2 pi themselves


def _truth(v) -> bool:
    """A scalar flag of a state dict as a bool: a tensor on any device (read on the host), a numpy or a Python value."""
    return bool(v.detach().cpu()) if isinstance(v, torch.Tensor) else bool(np.asarray(v))


def _shape(v) -> tuple:
    return tuple(v.shape) if hasattr(v, "shape") else tuple(np.shape(v))


def flow_transform_kinds(sd, prefix: str = FLOW_TRANSFORM_PREFIX) -> list:
    """The kind of each transform of a checkpoint's pose flow, from its key set, in index order: 'actnorm' (``log_scale``), 'lulinear'
    (``lower_entries``) or 'coupling' (``transform_net.*``).  Refused, each naming what was found and before any device call: an index that is
    not a number or a gap in the indices, a key set of none of the three kinds, a coupling whose ``final_layer`` has 144 rows (the affine
    coupling, not built), an ActNorm whose ``initialized`` is False (data-dependent initialisation belongs to training)."""
    per = {}
    for k, v in sd.items():
        if k.startswith(prefix):
            idx, _, name = k[len(prefix):].partition(".")
            if not idx.isdigit() or not name:
                raise KeyError(f"stage-1 checkpoint: {k} is not <index>.<name> below {prefix}")
            per.setdefault(int(idx), {})[name] = v
    if sorted(per) != list(range(len(per))):
        raise KeyError(f"stage-1 checkpoint: the flow's transform indices {sorted(per)} are not 0 .. n-1")
    kinds = []
    for i in range(len(per)):
        names = per[i]
        if "log_scale" in names:
            if "initialized" in names and not _truth(names["initialized"]):
                raise ValueError(f"stage-1 checkpoint: ActNorm {prefix}{i} has initialized == False; its data-dependent initialisation belongs to "
                                 "training and is not built")
            kinds.append("actnorm")
        elif "lower_entries" in names:
            kinds.append("lulinear")
        elif any(n.startswith("transform_net.") for n in names):
            fw = names.get("transform_net.final_layer.weight")
            if fw is None:
                raise KeyError(f"stage-1 checkpoint: coupling {prefix}{i} has no transform_net.final_layer.weight (keys {sorted(names)[:6]} ...)")
            if _shape(fw)[0] != FLOW_DIM // 2:
                raise ValueError(f"stage-1 checkpoint: coupling {prefix}{i} has a final_layer of {_shape(fw)[0]} rows (an affine coupling has "
                                 f"{FLOW_DIM}); only the additive coupling ({FLOW_DIM // 2} rows) is built")
            kinds.append("coupling")
        else:
            raise KeyError(f"stage-1 checkpoint: unknown flow transform {prefix}{i} with keys {sorted(names)}")
    return kinds


def flow_has_batch_norm(sd) -> bool:
    return any(k.startswith(FLOW_TRANSFORM_PREFIX) and ".batch_norm_layers." in k for k in sd)


def load_stage1_checkpoint(model: torch.nn.Module, path_or_state, flow: bool = False):
    """A ProHMR-scene checkpoint (test_prohmr_scene.py:81-85) into egohmr_amd.stage1.ProHMRSceneTransl.  The keys the translation does not
    read - ``flow.flow.*`` (the normalizing flow), ``discriminator.*``, ``smpl*`` and ``initialized`` - are ignored; every other key must be one
    of the model's and every one of the model's must be present.  Stricter than the reference's ``strict=False`` on purpose: that would
    silently keep random weights for a missing key, or for a head whose width (the context flags) does not match.  Returns the loaded keys.

    ``flow=True``: into egohmr_amd.stage1.ProHMRScene, ``flow.flow.*`` loaded as well (``flow.flow._distribution._log_z`` aside).  The flow's
    names are those of published nflows; a checkpoint that differs - other names, another chain of transforms than the model's ActNorm, LULinear,
    coupling per block, BatchNorm keys the model was not built for (``flow_batch_norm``) - is refused with the keys named
    (:func:`flow_transform_kinds` lists the other refusals), never loaded in part."""
    w = torch.load(path_or_state, map_location="cpu") if isinstance(path_or_state, (str, os.PathLike)) else path_or_state
    sd = w["state_dict"] if isinstance(w, Mapping) and "state_dict" in w else w
    ignored = tuple(p for p in STAGE1_IGNORED_PREFIXES if not (flow and p == "flow.flow."))
    sd = {k: v for k, v in sd.items() if k != "initialized" and not k.startswith(ignored) and not (flow and k in FLOW_IGNORED_KEYS)}
    need = model.state_dict()
    if flow:
        kinds, want = flow_transform_kinds(sd), flow_transform_kinds(need)
        if kinds != want:
            raise KeyError(f"stage-1 checkpoint: the flow's transforms are {kinds}, the model's are {want}")
    missing, unexpected = sorted(set(need) - set(sd)), sorted(set(sd) - set(need))
    if missing or unexpected:
        raise KeyError(f"stage-1 checkpoint: missing {missing[:8]}{' ...' if len(missing) > 8 else ''} ({len(missing)}), "
                       f"unexpected {unexpected[:8]}{' ...' if len(unexpected) > 8 else ''} ({len(unexpected)})")
    k = "flow.fc_head.layers.0.weight"
    if tuple(sd[k].shape) != tuple(need[k].shape):
        raise ValueError(f"stage-1 checkpoint: {k} is {tuple(sd[k].shape)}, the model's context flags (with_focal_length, with_bbox_info, "
                         f"with_cam_center) need {tuple(need[k].shape)}")
    if flow:
        for k in sorted(sd):
            if k.startswith("flow.flow.") and _shape(sd[k]) != tuple(need[k].shape):
                raise ValueError(f"stage-1 checkpoint: {k} is {_shape(sd[k])}, the model needs {tuple(need[k].shape)}")
    model.load_state_dict({kk: torch.as_tensor(np.asarray(v)) if not isinstance(v, torch.Tensor) else v for kk, v in sd.items()}, strict=True)
    return sorted(sd)


def load_preprocess_stats(path: str):
    """`preprocess_stats.npz` -> (body_rep_mean [144], body_rep_std [144]) (test_egohmr.py:109-111: keys 'Xmean', 'Xstd')."""
    z = np.load(path)
    mean, std = np.asarray(z["Xmean"], np.float32).reshape(-1), np.asarray(z["Xstd"], np.float32).reshape(-1)
    if mean.shape != (144,) or std.shape != (144,):
        raise ValueError(f"{path}: Xmean/Xstd have shapes {mean.shape}/{std.shape}, expected 144 values each")
    return mean, std


def load_smpl_mean_params(path: str) -> np.ndarray:
    """`data/smpl_mean_params.npz['shape']` -> init betas [1, 10] (models/egohmr/egohmr.py:669-671)."""
    shape = np.asarray(np.load(path)["shape"], np.float32).reshape(1, -1)
    if shape.shape != (1, 10):
        raise ValueError(f"{path}: 'shape' has {shape.size} values, expected 10")
    return shape


def load_checkpoint(model: torch.nn.Module, path_or_state, strict: bool = False):
    """`weights = torch.load(ckpt); model.load_state_dict(weights['state_dict'], strict=False)` (test_egohmr.py:125-127).
    Returns torch's (missing_keys, unexpected_keys) so a caller can see what a checkpoint did not cover."""
    w = torch.load(path_or_state, map_location="cpu") if isinstance(path_or_state, (str, os.PathLike)) else path_or_state
    sd = w["state_dict"] if isinstance(w, Mapping) and "state_dict" in w else w
    return model.load_state_dict(sd, strict=strict)


def read_obj_vertices(path: str) -> np.ndarray:
    """The vertices of an OBJ file, [V, 3] float64 in file order: the ``v x y z`` lines (a fourth weight or trailing vertex colours are
    ignored), what ``np.asarray(o3d.io.read_triangle_mesh(path).vertices)`` holds in preprocess_scene_s1.py / preprocess_scene_s2_for_test.py.

    open3d reads OBJ files through tinyobjloader, whose default ``real_t`` is float: each coordinate is parsed, rounded to float32 and widened to
    float64 in open3d's vertex array.  So here: parsed as a double, rounded to float32, widened.  That is believed from the libraries' sources
    and defaults, not checked against open3d itself (not a dependency of this package).  Faces, normals and texture coordinates are not
    read."""
    rows = []
    with open(path, "r") as f:
        for line in f:
            if line.startswith("v ") or line.startswith("v\t"):
                tok = line.split()
                if len(tok) < 4:
                    raise ValueError(f"{path}: vertex line with fewer than 3 coordinates: {line.strip()!r}")
                rows.append((float(tok[1]), float(tok[2]), float(tok[3])))
    return np.asarray(rows, np.float64).reshape(-1, 3).astype(np.float32).astype(np.float64)


def read_obj_mesh(path: str):
    """An OBJ file as a triangle mesh -> (vertices float32 [V,3], faces int32 [F,3], colors float32 [V,3] or None), what egohmr_amd.render draws.

    ``v x y z [r g b]`` lines (the colours are kept when EVERY vertex has them; a lone fourth value is a weight and is ignored); ``f`` lines with
    tokens ``a``, ``a/b``, ``a/b/c`` or ``a//c``, of which the vertex index ``a`` is read: 1-based, or negative and then relative to the vertices
    read so far; polygons are fan-triangulated around their first corner.  Normals, texture coordinates, groups and materials are not read."""
    verts, cols, faces = [], [], []
    with open(path, "r") as f:
        for ln, line in enumerate(f, 1):
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                if len(tok) < 4:
                    raise ValueError(f"{path}:{ln}: vertex line with fewer than 3 coordinates: {line.strip()!r}")
                verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
                if len(tok) >= 7:
                    cols.append((float(tok[4]), float(tok[5]), float(tok[6])))
            elif tok[0] == "f":
                if len(tok) < 4:
                    raise ValueError(f"{path}:{ln}: face with fewer than 3 corners: {line.strip()!r}")
                idx = []
                for t in tok[1:]:
                    a = int(t.split("/")[0])
                    a = a - 1 if a > 0 else len(verts) + a
                    if a < 0 or a >= len(verts):
                        raise ValueError(f"{path}:{ln}: face corner {t!r} is outside the {len(verts)} vertices read so far")
                    idx.append(a)
                faces.extend((idx[0], idx[k], idx[k + 1]) for k in range(1, len(idx) - 1))
    v = np.asarray(verts, np.float64).reshape(-1, 3).astype(np.float32)
    c = np.asarray(cols, np.float64).reshape(-1, 3).astype(np.float32) if verts and len(cols) == len(verts) else None
    return v, np.asarray(faces, np.int64).reshape(-1, 3).astype(np.int32), c
