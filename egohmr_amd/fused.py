"""The native sampling engine behind `EgoHMR.fused_sampler`: step-invariant conditioning (`prepare`), the one-call sampling loop
(`run` / `run_samples` -> ehm_sample_loop), the granular denoiser evaluation of `EgoHMR.forward`, the collision-guidance pieces and
the per-checkpoint precision-schedule calibration (`calibrate_schedule`).

Reference code this replaces on the hot path: diffusion/gaussian_diffusion.py:391-508 / :618-718 (the loops) driving
models/egohmr/egohmr.py:173-303 (forward) and :517-570 (guide_coll); see DESIGN.md sections 2 and 4.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from functools import partial
from types import SimpleNamespace

import torch

from . import _lib
from . import smpl as smpl_mod

PRECISIONS = {"f32": 0, "f16x3": 1, "f16": 2, "f16x2": 3}   # EHM_PREC_* ("f16x2": a tier of the f16x3 schedule and of the kernel tests, not a value of EgoHMR.gcn_precision)

# ---------------------------------------------------------------------------------------------- native engine
def pass_map(need):
    """Per-item `need` [B] (True: an invisible joint, the item takes the image-masked pass too) -> (mask_items: ascending indices with need,
    mask_slot [B]: rank of b among them or -1, num_masked: their count), int32 - as pass_map_kernel (csrc/prep.hip) writes it.  One host read-back."""
    need = need.reshape(-1).bool()
    rank = torch.cumsum(need, 0, dtype=torch.int32) - 1
    mask_slot = torch.where(need, rank, torch.full_like(rank, -1)).contiguous()
    mask_items = torch.nonzero(need).reshape(-1).to(torch.int32).contiguous()
    return mask_items, mask_slot, int(mask_items.numel())


def need_all_items(scales) -> bool:
    """THE need rule, part 1 (per call): with guidance scales (s_vis, s_inv) on the fuse x0 = u + s (c - u), item b needs the masked second pass iff
    some joint of it has s != 1.  s_vis != 1: every joint does, so every item needs it and the pass map is the identity."""
    return float(scales[0]) != 1.0


def item_need(vis_bool, need_all):
    """THE need rule, part 2 (per item), for calls that run two passes at all (EgoHMR.fuse_passes: s_inv != 1 or s_vis != 1): [B] bool, every item
    under need_all, else the items with an invisible joint - what item_prep_kernel (csrc/prep.hip, ehm_item_prep_desc.need_all) computes."""
    if need_all:
        return torch.ones(vis_bool.shape[0], dtype=torch.bool, device=vis_bool.device)
    return ~vis_bool.all(dim=1)


@dataclasses.dataclass
class _Prepared:
    """The step-invariant conditioning of a batch (FusedSampler.prepare)."""
    B: int
    h_img: torch.Tensor                 # [B,2,hid] image slice of the input conv        } per item: PER_ITEM
    h_oth: torch.Tensor                 # [B,2,hid] scene + translation + camera slice
    vis: torch.Tensor                   # [B,24] uint8 joint visibility
    vis_bool: torch.Tensor              # the same as bool
    betas: torch.Tensor
    scene: torch.Tensor
    transl: torch.Tensor
    fx: torch.Tensor
    cam_cx: torch.Tensor
    cam_cy: torch.Tensor
    img_feats: torch.Tensor
    scene_feats: torch.Tensor
    finite: torch.Tensor                # [B] bool: the item's inputs are finite
    mask_items: torch.Tensor            # the pass map (pass_map above); num_masked = -1: no map
    mask_slot: torch.Tensor
    num_masked: int
    inputs: list = None                 # strong references to the batch tensors behind the cache key (prepare)

    # the pass map was made for scales with s_vis != 1 (need_all_items): every item has a second pass.  A plain attribute that the operations below
    # hand on, not a field: it describes the map, like num_masked, and is set by whoever makes one
    need_all = False

    PER_ITEM = ("h_img", "h_oth", "vis", "vis_bool", "betas", "scene", "transl", "fx", "cam_cx", "cam_cy", "img_feats", "scene_feats", "finite")

    def take(self, index):
        """Some items as a prepared batch of their own: index = n (the first n; n >= B: self) or an index tensor (repeats allowed)."""
        if isinstance(index, int):
            if index >= self.B:
                return self
            index = torch.arange(index, device=self.vis.device)
        index = index.to(self.vis.device, torch.long)
        picked = {k: getattr(self, k).index_select(0, index).contiguous() for k in self.PER_ITEM}
        mask_items, mask_slot, num_masked = pass_map(item_need(picked["vis_bool"], self.need_all))
        out = dataclasses.replace(self, B=int(index.numel()), mask_items=mask_items, mask_slot=mask_slot, num_masked=num_masked, **picked)
        out.need_all = self.need_all
        return out

    def with_need(self, need_all):
        """The same batch with the pass map of the other need rule (one host read-back; nothing is encoded again)."""
        if bool(need_all) == bool(self.need_all):
            return self
        mask_items, mask_slot, num_masked = pass_map(item_need(self.vis_bool, need_all))
        out = dataclasses.replace(self, mask_items=mask_items, mask_slot=mask_slot, num_masked=num_masked)
        out.need_all = bool(need_all)
        return out

    def tile(self, S):
        """The batch S times, sample-major (body s * B + b); its pass map by offset arithmetic on the device (= pass_map(need.repeat(S)),
        tests/test_prepared_cpu.py, without the host read-back; the arithmetic holds for any per-item need, so for either rule of item_need).
        num_masked = -1 (no map) stays -1."""
        B, nm = self.B, max(self.num_masked, 0)
        off = torch.arange(S, device=self.mask_slot.device, dtype=torch.int32).view(-1, 1)
        slot = self.mask_slot.view(1, -1)
        tiled = {k: getattr(self, k).repeat(S, *([1] * (getattr(self, k).dim() - 1))).contiguous() for k in self.PER_ITEM}
        out = dataclasses.replace(
            self, B=S * B, mask_items=(self.mask_items.view(1, -1) + off * B).reshape(-1).contiguous(),
            mask_slot=torch.where(slot >= 0, slot + off * nm, torch.full_like(slot, -1)).reshape(-1).contiguous(),
            num_masked=S * self.num_masked if self.num_masked >= 0 else self.num_masked, **tiled)
        out.need_all = self.need_all
        return out


@dataclasses.dataclass
class _PreparedConstants(_Prepared):
    """prepare(_constants_only=True): what the training route of EgoHMR.forward keeps constant.  h_img, h_oth, betas and scene_feats are None and there
    is no pass map, so take() / tile() do not apply."""
    other: torch.Tensor = None          # the padded [scene (unwritten) | transl | cam] operand ehm_item_prep filled


class FusedSampler:
    """Owns the native denoiser handle and runs sampling loops through ehm_sample_loop."""

    def __init__(self, model):
        self._model_ref = [model]
        self._gcn = self._gcn_key = self._folded = None        # native denoiser handle, its weight key, the folded input-conv slices (gcn)
        self._nl_set = None                                    # (non-local block's weight key, handle serial) the handle was last given
        self._pk = self._ck = None                             # TensorKeys behind _param_key / _cond_param_key (built on first use: invalidate)
        self._prep = self._prep_key = None                     # the cached conditioning (prepare)
        self._joint_map = self._count_host = None              # prepare: openpose_to_smpl on the device; pinned word for the second-pass count
        self._beta_key = self._beta_w = None                   # _project: the beta head's packed weights
        self._tv_cache = None                                  # timestep_vectors: (key, vectors) of the last timestep sequence
        self._ws, self._graphs = None, {}                      # eager workspace; hipGraph entries by shape / schedule key (_replay)
        self._status_host = self._status_event = None          # defer_status: pinned status word + the event behind its copy
        self._sched_cache = {}          # schedule_key -> calibration info (calibrate_schedule)
        self.schedule_info = None       # the calibration the most recent 'auto' run used (None: ran all-f16x3 / explicit k)
        self.last_lowprec = 0
        self.last_twoterm = 0           # two-term steps (behind the plain-f16 ones) of the last call
        self.last_fuse = (0, 1.0, 0.0)  # (cfg, s_vis, s_inv) the handle was given for the last loop (ehm_gcn_set_fuse_scales)
        self.last_trace = None

    @property
    def model(self):
        return self._model_ref[0]

    # ------------------------------------------------------------------ weights -> native handle
    def _param_key(self):
        self._pk = self._pk or _lib.TensorKey(self.model.diffusion_model, self.model.input_process)
        return self._pk()

    def gcn(self):
        key = self._param_key()
        if self._gcn is None or key != self._gcn_key:
            if self._gcn is not None:
                self._gcn.close()
            m = self.model
            dm = m.diffusion_model
            gi = dm.gconv_input[0]
            h, keep = dm.create_native_handle(m.device)                        # (ModulatedGCN owns the parameter marshalling: ehm_gcn_create)
            self._gcn, self._gcn_key = _lib.Handle(h, _lib.api().ehm_gcn_destroy, keep), key
            # fold InputProcess (Linear 6->512) into the x_t slice of the input conv: x @ (Wp^T W_k[2694:3206]) + bp W_k[...]
            W = gi.gconv.W.detach().double()                                            # [2, 3718, hid]
            Wp, bp = m.input_process.poseEmbedding.weight.detach().double(), m.input_process.poseEmbedding.bias.detach().double()
            a, b, c, d = m.cond_split
            Wx = torch.einsum("ec,kef->kcf", Wp, W[:, b:c, :])                          # [2,6,hid]
            bx = torch.einsum("e,kef->kf", bp, W[:, b:c, :])                            # [2,hid]
            # the image / scene+translation+camera slices as ONE [K, 2*hid] matrix each (both branches side by side, K padded to 32 with
            # zero rows): operands of ehm_skinny_gemm_f32 in prepare()
            hid = dm.hid_dim
            Wd = gi.gconv.W.detach().float()
            k_oth = (b - a + 31) // 32 * 32
            W_img_cat = Wd[:, :a, :].permute(1, 0, 2).reshape(a, 2 * hid).contiguous()
            W_oth_cat = torch.zeros(k_oth, 2 * hid, device=m.device)
            W_oth_cat[:b - a] = Wd[:, a:b, :].permute(1, 0, 2).reshape(b - a, 2 * hid)
            self._folded = SimpleNamespace(Wx=Wx.float().contiguous(), bx=bx, W_t=W[:, c:d, :], W_img_cat=W_img_cat, W_oth_cat=W_oth_cat, k_oth=k_oth)
        A = _lib.api()
        A.ehm_gcn_set_uncond_mode(self._gcn, 0 if self.model.only_mask_img_cond else 1)
        mode = PRECISIONS[self.model.gcn_precision]
        if A.ehm_gcn_get_precision(self._gcn) != mode:
            A.ehm_gcn_set_precision(self._gcn, mode)
        if self.model.diffusion_model.nonlocal_layer:       # the one-call loop runs the block natively (ehm_gcn_set_nonlocal)
            (q, o), nl_key = self.model.diffusion_model.nonlocal_packed()
            if self._nl_set != (nl_key, self._gcn.serial):
                p = _lib.NonlocalParams(_lib.ptr(q.buf), _lib.ptr(q.bias), q.scale, _lib.ptr(o.buf), _lib.ptr(o.bias), o.scale,
                                        self.model.diffusion_model.non_local.inter_channels)
                A.ehm_gcn_set_nonlocal(self._gcn, C.byref(p))
                self._nl_set = (nl_key, self._gcn.serial)
        return self._gcn

    def _backbone_fn(self):
        """ResNet-50 with BatchNorm folded into the convolutions, rebuilt when the backbone weights change."""
        return self.model.backbone.current()

    # ------------------------------------------------------------------ step-invariant conditioning
    @torch.no_grad()
    def prepare(self, batch, _constants_only=False, _no_trunk=False, scales=None) -> _Prepared:
        """Everything in EgoHMR.forward that does not depend on x_t / t (egohmr.py:182-223, :263-265).
        scales: the call's guidance scales (EgoHMR.fuse_scales; None = the model's for a default call) - they decide which items the pass map keeps
        (need_all_items).
        _constants_only (the training route of EgoHMR.forward): only what stays constant with the trunk frozen - trunk, visibility, camera columns, scene,
        translation; the PointNet, the projections, the beta head and the native handle are left out (h_img, h_oth, betas, scene_feats = None, no pass map,
        no host read-back; `other` holds ehm_item_prep's operand).  Such an entry is cached under a key of its own: no other caller ever sees it.
        _no_trunk (with _constants_only, behind EgoHMR.trunk_grad): the trunk is left out too - img_feats = None, the caller runs it with a graph -
        again under a key of its own."""
        with _lib.on_device(self.model.device):          # every native call below launches on the CURRENT device's stream
            need_all = False if _constants_only else need_all_items(self.model.sampling_scales() if scales is None else scales)
            return self._prepare_on_device(batch, _constants_only, _constants_only and _no_trunk, need_all)

    def _prepare_on_device(self, batch, constants_only=False, no_trunk=False, need_all=False) -> _Prepared:
        m = self.model
        # Cache key = identity AND version of every tensor the conditioning is computed from, and of every weight it passes
        # through.  The cached entry keeps strong references to those input tensors, so neither their id() nor their storage can be
        # recycled for a different batch while the entry is alive; in-place edits bump _version.
        ins = [batch["img"], batch["scene_pcd_verts_full"], batch["orig_keypoints_2d"], batch["fx"], batch["cam_cx"], batch["cam_cy"],
               batch["box_center"], batch["box_size"], batch["smpl_params"]["transl"]]
        if ins[0].shape[0] == 0:
            raise ValueError("empty batch (the reference fails on it too: egohmr.py:233 reshapes x_t [0, 144] to [0, 24, -1])")
        # ... and of the model switches that ehm_item_prep bakes into the cached state (the camera-feature columns, the scene frame, which
        # OpenPose joints feed the visibility mask)
        if m.encoder_precision not in ("f16x3", "f16"):
            raise ValueError(f"EgoHMR.encoder_precision must be 'f16x3' or 'f16', not {m.encoder_precision!r}")
        m.backbone.hi_only = m.scene_enc.hi_only = m.encoder_precision == "f16"
        switches = (bool(m.with_bbox_info), bool(m.with_cam_center), bool(m.scene_cano), tuple(m.openpose_to_smpl), m.encoder_precision)
        key = tuple((id(t), t._version, t.data_ptr()) for t in ins) + self._param_key() + self._cond_param_key() + (switches,)
        if constants_only:
            key += ("constants_only",)
        if no_trunk:
            key += ("no_trunk",)
        base_key, key = key, key + (("need_all", bool(need_all)),)
        if self._prep is not None and self._prep_key == key:
            return self._prep
        if self._prep is not None and not constants_only and self._prep_key[:-1] == base_key and isinstance(self._prep_key[-1], tuple):
            # the same batch under the other need rule: only the pass map differs, the conditioning is not encoded again
            self._prep, self._prep_key = self._prep.with_need(need_all), key
            return self._prep
        if not constants_only:
            self.gcn()
        dev = m.device
        g = lambda k: _lib.f32(batch[k], dev)
        transl = _lib.f32(batch["smpl_params"]["transl"], dev)
        scene = g("scene_pcd_verts_full")
        if m.scene_cano:
            scene = scene - transl.unsqueeze(1)                                        # :211
        scene = scene.contiguous()
        img = g("img")
        B, st = img.shape[0], _lib.stream_ptr()
        # ---- per-item scalars in two launches (csrc/prep.hip): joint visibility (:186-188), the pass-pruning map (ehm_gcn_set_pass_map: items
        # with an invisible joint need the second pass), TranslEnc (:217) and the camera features (:195-205) written straight into the padded
        # [scene | transl | cam] operand of the projections, and the per-item "inputs are finite" flag.  The reference's float32 graph carries a
        # NaN / Inf of an item's inputs into every output of THAT item (ReLU and max-pool propagate NaN in torch); the kernels' v_max /
        # saturating conversions would swallow it, so the flag travels beside the data (ehm_pack_outputs).  A row sum is non-finite exactly
        # when the row holds a NaN / Inf - or finite values whose float32 sum overflows, which no image or point cloud in metres does.
        # The count of second passes is the ONE host read-back of a batch.  It is REQUESTED here (an asynchronous copy into pinned memory +
        # an event) and LOOKED AT after the encoders have been enqueued: in a pipeline of batches the copy sits behind the previous batch's
        # sampling loop, the host spends that time enqueuing this batch's encoders, and the GPU never waits for Python.
        kp = g("orig_keypoints_2d")
        fx, cx, cy, bc, bs = g("fx"), g("cam_cx"), g("cam_cy"), g("box_center"), g("box_size")
        te = m.transl_enc.layers
        tw = [_lib.f32(te[0].weight, dev), _lib.f32(te[0].bias, dev), _lib.f32(te[2].weight, dev), _lib.f32(te[2].bias, dev)]
        n_scene, n_tr = m.scene_enc.fc_c.out_features, te[2].out_features
        n_other = n_scene + n_tr + 1 + (3 if m.with_bbox_info else 0) + (2 if m.with_cam_center else 0)
        k_oth = (n_other + 31) // 32 * 32                                              # (= _folded.k_oth: the projections' K granule)
        jm = self._joint_map
        if kp.dim() != 3 or kp.shape[2] != 3 or not all(0 <= int(k) < kp.shape[1] for k in m.openpose_to_smpl):
            # (item_prep_kernel indexes keypoints_2d[b, joint_map[t], 2]: checked here, once per batch, instead of on the device)
            raise ValueError(f"orig_keypoints_2d must be [B, NK, 3] with NK > max(openpose_to_smpl) = {max(m.openpose_to_smpl)}; got {tuple(kp.shape)}")
        if jm is None or jm[0] != (tuple(m.openpose_to_smpl), str(dev)):
            jm = self._joint_map = ((tuple(m.openpose_to_smpl), str(dev)), torch.tensor(m.openpose_to_smpl, dtype=torch.int32, device=dev))
        oth = torch.empty(B, k_oth, device=dev)
        vis = torch.empty(B, 24, dtype=torch.uint8, device=dev)
        flags = torch.empty(2, B, dtype=torch.uint8, device=dev)                       # finite | need (scratch)
        maps = torch.empty(2 * B + 1, dtype=torch.int32, device=dev)                   # mask_slot | mask_items | count
        sums = (img.reshape(B, -1).sum(dim=1), scene.reshape(B, -1).sum(dim=1))
        P = _lib.ptr
        d = _lib.ItemPrepDesc(keypoints_2d=P(kp), joint_map=P(jm[1]), NK=kp.shape[1], force_visible=8, fx=P(fx), cx=P(cx),
                              cy=P(cy), box_center=P(bc), box_size=P(bs), transl=P(transl), fx_norm=m.cfg.CAM.FX_NORM_COEFF,
                              with_bbox=int(m.with_bbox_info), with_cam_center=int(m.with_cam_center), tW1=P(tw[0]), tb1=P(tw[1]),
                              tW2=P(tw[2]), tb2=P(tw[3]), t_hidden=te[0].out_features, t_out=n_tr, img_rowsum=P(sums[0]),
                              scene_rowsum=P(sums[1]), other=P(oth), other_ld=k_oth, other_col0=n_scene, vis=P(vis),
                              mask_slot=P(maps), mask_items=P(maps[B:]), count=P(maps[2 * B:]), finite=P(flags),
                              need_scratch=P(flags[1]), pass_group=1, B=B, need_all=int(bool(need_all)))
        _lib.api().ehm_item_prep(C.byref(d), st)
        if self._count_host is None:
            self._count_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._count_host.copy_(maps[2 * B:], non_blocking=True)
        count_ready = torch.cuda.Event()
        count_ready.record(torch.cuda.current_stream(dev))
        # The two encoders are independent, but each fills the chip on its own: one after the other on ONE stream (two streams measured
        # slower, docs/EXPERIMENTS.md)
        img_feats = None if no_trunk else self._backbone_fn()(img)                     # :183 (BatchNorm folded into the convs)
        if constants_only:
            self._prep = _PreparedConstants(B=B, h_img=None, h_oth=None, vis=vis, vis_bool=vis.view(torch.bool), betas=None, scene=scene, transl=transl, fx=fx,
                                   cam_cx=cx, cam_cy=cy, img_feats=None if no_trunk else img_feats.contiguous(), scene_feats=None,
                                            finite=flags[0].view(torch.bool), mask_items=maps[B:B], mask_slot=maps[:B], num_masked=-1, inputs=ins, other=oth)
            self._prep_key = key
            return self._prep
        scene_feats = m.scene_enc(scene)                                               # :214
        oth[:, :n_scene].copy_(scene_feats)                                            # :220-221 [scene | transl | cam] (the rest was written by ehm_item_prep)
        h_img, h_oth, betas = self._project(img_feats.contiguous(), oth, n_other)
        # items with a non-finite input (flags[0] == 0: their outputs are NaN by the packer's rule) get ZERO conditioning: the encoders' saturating f16 stores
        # have turned their inf / NaN into large FINITE features, which would drive the denoiser's activations to the f16 range and raise its range guard
        # (status bit 2) for an item that is already accounted for
        bad = (flags[0] == 0).view(B, 1, 1)
        h_img.masked_fill_(bad, 0.0)
        h_oth.masked_fill_(bad, 0.0)
        count_ready.synchronize()
        num_masked = int(self._count_host[0])
        self._prep = _Prepared(B=B, h_img=h_img, h_oth=h_oth, vis=vis, vis_bool=vis.view(torch.bool),
                               betas=betas, scene=scene, transl=transl, fx=fx, cam_cx=cx, cam_cy=cy, img_feats=img_feats,
                               scene_feats=scene_feats, finite=flags[0].view(torch.bool), mask_items=maps[B:B + num_masked],
                               mask_slot=maps[:B], num_masked=num_masked, inputs=ins)      # (inputs: strong references, see the key above)
        self._prep.need_all = bool(need_all)
        self._prep_key = key
        return self._prep

    def _project(self, img_feats, oth, n_other):
        """The step-invariant slices of the input graph conv ([B,2,hid] each: image features, scene + translation + camera features)
        and the beta head (egohmr.py:263-265, Linear -> ReLU -> Linear + init_betas) as exact-float32 matrix-core GEMMs built for M = B
        rows (ehm_skinny_gemm_f32).  oth = [scene | transl | cam] zero-padded to a multiple of 32 columns, n_other of them live."""
        m, f, A = self.model, self._folded, _lib.api()
        B, dev, hid = img_feats.shape[0], img_feats.device, m.diffusion_model.hid_dim
        st = _lib.stream_ptr()
        a = img_feats.shape[1]
        l1, l2 = m.beta_layer.layers[0], m.beta_layer.layers[2]
        if a % 32 or l1.out_features % 32 or l1.in_features != a + n_other or l2.out_features > 32:
            raise _lib.EgoHMRHipError(f"conditioning widths the projection kernels are not built for: image features {a}, beta head "
                                      f"{l1.in_features} -> {l1.out_features} -> {l2.out_features}, other features {n_other}")
        h_img = torch.empty(B, 2, hid, device=dev)
        h_oth = torch.empty(B, 2, hid, device=dev)
        A.ehm_skinny_gemm_f32(img_feats, f.W_img_cat, None, h_img, B, a, 2 * hid, 0, st)
        A.ehm_skinny_gemm_f32(oth, f.W_oth_cat, None, h_oth, B, f.k_oth, 2 * hid, 0, st)
        # beta head: both layers on the same kernel (weights transposed and zero-padded once per weight version; init_betas folded into
        # the second bias)
        ib = m.beta_layer.init_betas
        key = tuple((t.data_ptr(), t._version) for t in (l1.weight, l1.bias, l2.weight, l2.bias, ib)) + (str(dev),)
        if self._beta_key != key:
            Wt = torch.zeros(a + f.k_oth, l1.out_features, device=dev)
            w = l1.weight.detach().float().to(dev)
            Wt[:a] = w[:, :a].t()
            Wt[a:a + n_other] = w[:, a:].t()
            W2 = torch.zeros(l1.out_features, 32, device=dev)
            W2[:, :l2.out_features] = l2.weight.detach().float().to(dev).t()
            b2 = torch.zeros(32, device=dev)
            b2[:l2.out_features] = (l2.bias.detach().float().to(dev) + ib.detach().float().to(dev).reshape(-1))
            self._beta_w = (Wt.contiguous(), l1.bias.detach().float().to(dev).contiguous(), W2.contiguous(), b2)
            self._beta_key = key
        W1, b1, W2, b2 = self._beta_w
        xb = torch.cat([img_feats, oth], dim=1)
        hb = torch.empty(B, l1.out_features, device=dev)
        A.ehm_skinny_gemm_f32(xb, W1, b1, hb, B, xb.shape[1], l1.out_features, 1, st)
        b32 = torch.empty(B, 32, device=dev)
        A.ehm_skinny_gemm_f32(hb, W2, b2, b32, B, l1.out_features, 32, 0, st)
        return h_img, h_oth, b32[:, :l2.out_features].contiguous()

    def _cond_param_key(self):
        m = self.model
        self._ck = self._ck or _lib.TensorKey(m.backbone, m.scene_enc, m.transl_enc, m.beta_layer, m.embed_timestep)
        return self._ck()

    def _apply_pass_map(self, st, passes):
        """(virtual bodies, num_masked for the descriptor) after telling the handle which items still need the second pass."""
        m, A = self.model, _lib.api()
        h = self.gcn()
        if passes == 2 and m.prune_passes:
            A.ehm_gcn_set_pass_map(h, st.mask_items if st.num_masked else None, st.mask_slot, st.num_masked)
            return st.B + st.num_masked, st.num_masked
        A.ehm_gcn_set_pass_map(h, None, None, -1)
        return passes * st.B, -1

    def invalidate(self, structure: bool = False):
        """Drop the cached conditioning (bench.py: the encoders are part of every timed call).  structure=True also re-collects the
        parameter slots behind the weight-version keys (needed only after sub-modules or parameters were ADDED to the model)."""
        self._prep, self._prep_key = None, None
        if structure:
            self._pk = self._ck = None

    @torch.no_grad()
    def timestep_vectors(self, t_orig) -> torch.Tensor:
        """[n] original timesteps -> [n,2,hid]: TimestepEmbedder (egohmr.py:642-643) pushed through the timestep
        slice of the input conv, plus the folded InputProcess bias.  A python sequence of ints (the sampler's timestep map) is cached per
        (weights, sequence): the embedding MLP and its float64 projection ran again on every sampling call."""
        m = self.model
        self.gcn()
        ckey = None
        if not torch.is_tensor(t_orig):
            ckey = (self._param_key(), self._cond_param_key(), tuple(int(t) for t in t_orig))
            if self._tv_cache is not None and self._tv_cache[0] == ckey:
                return self._tv_cache[1]
            t_orig = torch.tensor(ckey[2], device=m.device, dtype=torch.long)
        temb = m.embed_timestep.time_embed(m.sequence_pos_encoder.pe[t_orig][:, 0])    # [n,512]
        tv = torch.einsum("ne,kef->nkf", temb.double(), self._folded.W_t) + self._folded.bx[None]
        tv = tv.float().contiguous()
        if ckey is not None:
            self._tv_cache = (ckey, tv)
        return tv

    @staticmethod
    def step_table(diffusion, ddim, cond_grad_weight, guided):
        """The T ehm_step_coefs rows of a loop (newest first = execution order), cached on the diffusion object: every row costs a handful of
        float32 CPU tensor ops (GaussianDiffusion.step_coefs keeps torch's roundings), 100 rows ~ 3 ms of host time per call."""
        cache = diffusion.__dict__.setdefault("_ehm_step_tables", {})
        # (the fingerprint of the tables the rows are computed from: a diffusion object whose betas / timestep map were edited in place gets new rows)
        fp = hash((diffusion.betas.tobytes(), tuple(getattr(diffusion, "timestep_map", ()))))
        key = (bool(ddim), float(cond_grad_weight), bool(guided), fp)
        if key not in cache:
            T = diffusion.num_timesteps
            rows = [diffusion.step_coefs(i, ddim, 0.0, cond_grad_weight, guided) for i in range(T - 1, -1, -1)]
            first_guided = next((i for i, r in enumerate(rows) if r.grad_scale != 0.0), T)
            cache[key] = ((_lib.StepCoefs * T)(*rows), first_guided)
        return cache[key]

    @staticmethod
    def guided_steps(diffusion, ddim, cond_grad_weight, guided) -> int:
        """The guided steps of a loop (a contiguous tail, gaussian_diffusion.py:378-385): schedule_key's ONE count, for run, calibration and install."""
        return diffusion.num_timesteps - FusedSampler.step_table(diffusion, ddim, cond_grad_weight, guided)[1]

    # ------------------------------------------------------------------ granular denoiser (EgoHMR.forward)
    def _workspace(self, nbytes, device):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self._ws

    @torch.no_grad()
    def denoise_once(self, st, x_t, tvec, passes=None, scales=None):
        """x0 [B,144] of one denoiser evaluation with guidance scales `scales` on the two passes (None: the model's for a default call; passes follows
        from them, EgoHMR.fuse_passes).  Scales (1, 0) - the reference's fuse - and one-pass calls take the select of ehm_gcn_output_layer."""
        m, A = self.model, _lib.api()
        scales = m.sampling_scales() if scales is None else tuple(float(v) for v in scales)
        passes = m.fuse_passes(scales) if passes is None else passes
        if passes == 2:
            st = st.with_need(need_all_items(scales))
        rows = self._apply_pass_map(st, passes)[0] * 24
        h = self.gcn()
        fill = lambda X0: A.ehm_gcn_input_layer(h, st.h_img, st.h_oth, st.vis, x_t, self._folded.Wx, tvec, X0, st.B, passes, _lib.stream_ptr())
        return m.diffusion_model.denoiser_tail(h, fill, rows=rows, B=st.B, passes=passes, vis=st.vis, precision=m.gcn_precision, device=m.device,
                                               scales=scales if self._cfg_kernels(passes, scales) else None)

    def _cfg_kernels(self, passes, scales) -> bool:
        """Whether a call combines its passes with the guidance kernels (ehm_gcn_set_fuse_scales: cfg = 1, ehm_gcn_output_layer_cfg) or takes the select:
        the select computes exactly the scales (1, 0), and a one-pass call has nothing to combine."""
        return passes == 2 and (tuple(scales) != (1.0, 0.0) or bool(self.model.force_cfg_kernels))

    # ------------------------------------------------------------------ guidance pieces
    @torch.no_grad()
    def collision(self, verts, scene, want_grad=True, want_hits=False, all_points=None):
        """The collision proxy for a batch of bodies: (loss [B], d loss / d verts [B,V,3] or None, hits [B] int32 or None).  EgoHMR.collision_proxy:
        'vertex' = the nearest-vertex hinge (ehm_collision_query), 'mesh' = winding-number occupancy and penetration depth of the posed mesh
        `smpl.faces_tensor` (ehm_mesh_collision_query)."""
        m = self.model
        verts, scene = _lib.f32(verts, m.device), _lib.f32(scene, m.device)
        B, V, N = verts.shape[0], verts.shape[1], scene.shape[1]
        mesh = m.mesh_collision()
        if mesh and V != m.smpl.num_verts:
            raise ValueError(f"collision_proxy = 'mesh': {V} vertices per body, the model's mesh has {m.smpl.num_verts}")
        faces = m.smpl.collision_faces() if mesh else None      # (validated when uploaded: ValueError before any launch)
        loss = torch.empty(B, device=m.device)
        gverts = torch.empty_like(verts) if want_grad else None
        hits = torch.empty(B, device=m.device, dtype=torch.int32) if want_hits else None
        allp = m.guide_all_points if all_points is None else all_points
        with torch.cuda.device(m.device):
            if mesh:
                _lib.api().ehm_mesh_collision_query(verts, faces, scene, loss, gverts, hits, B, V, faces.shape[0], N, int(bool(allp)), _lib.stream_ptr())
            else:
                _lib.api().ehm_collision_query(verts, scene, loss, gverts, hits, B, V, N, m.collision_tau, int(bool(allp)), _lib.stream_ptr())
        return loss, gverts, hits

    @torch.no_grad()
    def guidance_gradient(self, st, x, betas):
        m, A = self.model, _lib.api()
        B = x.shape[0]
        mean, std = m._std_mean()
        verts = torch.empty(B, m.smpl.num_verts, 3, device=m.device)
        joints = torch.empty(B, m.smpl.num_joints_out, 3, device=m.device)
        s = _lib.stream_ptr()
        A.ehm_smpl_forward_rot6d(m.smpl.handle(), betas, x, mean, std, verts, joints, None, None, None, B, s)
        loss, gverts, _ = self.collision(verts, st.scene)
        gpose = torch.empty(B, 144, device=m.device)
        A.ehm_smpl_backward_rot6d(m.smpl.handle(), betas, x, mean, std, gverts, gpose, B, s)
        grad = torch.empty(B, 144, device=m.device)
        denom = self.guide_denom(B)
        A.ehm_guidance_grad_finish(gpose, loss, grad, B, denom, s)
        return grad

    def guide_denom(self, B: int) -> float:
        """Denominator of the guidance gradient: B for `-loss.mean()` (egohmr.py:562), 1 for `-loss.sum()` (egohmr_volsmpl.py:618)."""
        m = self.model
        if m.guide_reduction != "mean":
            return 1.0
        return float(m.guide_denom_override) if m.guide_denom_override else float(B)

    # ------------------------------------------------------------------ precision schedule: calibrated per checkpoint
    def schedule_key(self, diffusion, ddim: bool, n_guided: int, cond_grad_weight: float = 0.0, guide_denom: float = 1.0):
        """What a calibrated k is valid for: these denoiser / embedder weights (identity + version of every tensor), this sampler
        (original timesteps visited, ancestral or DDIM), this guidance window, weight and reduction, these classifier-free guidance scales
        (EgoHMR.sampling_scales), this tolerance.  The batch size behind a
        `-loss.mean()` (guide_denom) is NOT part of the key: a ragged last batch, or ranks with different shard sizes, must find the job's one
        calibration (the f16 steps end >= 8 steps before the guided window whatever its strength)."""
        m = self.model
        return (self._param_key(), self._cond_param_key(), tuple(diffusion.timestep_map), int(getattr(diffusion, "original_num_steps", diffusion.num_timesteps)),
                bool(ddim), int(n_guided), (float(cond_grad_weight), str(m.guide_reduction), "mesh" if m.mesh_collision() else "vertex") if n_guided else None,
                bool(m.guide_all_points) if n_guided else False,
                bool(m.diffuse_fuse), tuple(float(v) for v in m.sampling_scales()),   # (s multiplies the two passes' rounding errors: k is per scale pair)
                float(m.schedule_tol), str(getattr(m, "f16x2_steps", 0)))

    def lowprec_steps(self, T: int, guided=False, ddim: bool = True, key=None) -> int:
        """How many LEADING steps of a T-step fused loop run on plain f16 operands (EgoHMR.f16x3_last_steps): None -> 0 (every step
        f32-grade), an int k -> T - k (the caller vouches for it), 'auto' -> T - k for the k that `calibrate_schedule` measured for
        `key` (= schedule_key(...)) on the LOADED weights, and 0 when there is no calibration for it.  There is no constant policy
        any more: a k tuned on one network says nothing about another (docs/EXPERIMENTS.md 3.6)."""
        k = self.model.f16x3_last_steps
        if k is None or self.model.gcn_precision != "f16x3":
            return 0
        if k == "auto":
            info = self._sched_cache.get(key) if key is not None else None
            if info is None:
                return 0
            k = info["k"]
        return max(0, T - int(k))

    def twoterm_steps(self, T: int, lowprec: int, key=None) -> int:
        """How many steps BEHIND the `lowprec` plain-f16 ones run two-term split-f16 products (EgoHMR.f16x2_steps): 0 -> 0, an int j -> j (at most
        the T - lowprec split steps), 'auto' -> the j that `calibrate_schedule` measured for `key`, and 0 when there is no calibration for it or when
        f16x3_last_steps is not 'auto' itself (an explicit k, or None, runs exactly the arithmetic it names)."""
        m = self.model
        j = getattr(m, "f16x2_steps", 0)
        if not j or m.gcn_precision != "f16x3":
            return 0
        if j == "auto":
            info = self._sched_cache.get(key) if (key is not None and m.f16x3_last_steps == "auto") else None
            j = 0 if info is None else info.get("two_term_steps", 0)
        return max(0, min(int(j), T - int(lowprec)))

    @staticmethod
    def pick_two_term(ladder, k, err_a, err_b, bar):
        """The second search of `calibrate_schedule`: with the last k steps split-f16, how many of them must stay three-term?  Candidates = the
        entries of the same `ladder` below k, then k itself (= no two-term step: error 0 by definition); `err_a(m)` / `err_b(m)` = error of the
        schedule [f16 x (T - k)] [two-term x (k - m)] [three-term x m].  Returns j = k - m for the smallest passing m, found like k is (`pick_k`)."""
        sub = [m for m in ladder if m < k] + [k]
        return int(k - sub[FusedSampler.pick_k(sub, err_a, err_b, bar)])

    @staticmethod
    def _k_ladder(T: int, floor: int = 2):
        """Candidate values of k (last k steps in f16x3), ascending, roughly geometric (ratio 4/3), always ending at T."""
        ks, x = [], float(max(floor, 2))
        while x < T:
            if not ks or int(round(x)) > ks[-1]:
                ks.append(int(round(x)))
            x *= 4.0 / 3.0
        return [k for k in ks if k < T] + [T]

    @staticmethod
    def pick_k(ladder, err_a, err_b, bar):
        """Index into `ladder` (ascending k, last entry = T = every step f32-grade, error 0 by definition) of the smallest k whose error
        on draw A is <= bar AND, from there upwards, the first k that also passes on draw B.  Bisection on draw A (the error falls with
        k up to noise; a non-monotone blip can only make the answer more conservative because draw B re-checks it), then a linear climb."""
        lo, hi = 0, len(ladder) - 1
        while lo < hi:
            mid = (lo + hi) // 2
            if err_a(ladder[mid]) <= bar:
                hi = mid
            else:
                lo = mid + 1
        idx = lo
        while idx < len(ladder) - 1 and err_b(ladder[idx]) > bar:
            idx += 1
        return idx

    @torch.no_grad()
    def calibrate_schedule(self, diffusion, batch=None, ddim=False, guided=False, cond_grad_weight=1.0, tol=None, bodies=64, prepared=None,
                           seeds=(20260929, 20260930), force=False, denom_items=None, n_guided=None):
        """Measure, for the weights that are loaded NOW, the smallest k such that a sampling loop whose first T - k steps run the hidden
        convs on plain f16 operands ends within `tol` metres (max vertex / joint distance, every body) of the loop that runs every step in
        split-f16 (f32-grade) arithmetic on the same noise - and cache it under `schedule_key`.

        Why per checkpoint: x_{t-1} = c1 x0(x_t) + c2 x_t carries an early step's rounding error with gain c1 J + c2, J = d x0 / d x_t.
        A denoiser that ignores x_t (J ~ 0) contracts it away within a few steps; a trained START_X denoiser has J -> 1 / sqrt(abar_t)
        at low noise, where c1 J + c2 = 1 / sqrt(alpha_t) >= 1: the error is carried to the output (gaussian_diffusion.py:298-337 is exact
        for any weights, so must this be).  Procedure: the first `bodies` items of the batch (conditioning already encoded), two private noise
        draws; bisection over a geometric ladder of k with draw A against tol / 2, then draw B must pass too (k moves up the ladder until
        it does).  k = T (no f16 step at all) always passes, so the result is always safe; cost = ~6-10 small sampling loops, once per
        (weights, sampler).  With EgoHMR.f16x2_steps = 'auto' a second search on the same ladder, draws and criterion then finds the largest j such that the
        first j of those k steps may run two-term products, a_hi (w_hi + w_lo) (`pick_two_term`; info["two_term_steps"], info["two_term_trials"]; k itself is
        found first and does not depend on it).  Returns the info dict that `schedule_info` / bench.py report."""
        m = self.model
        if m.gcn_precision != "f16x3":
            raise _lib.EgoHMRHipError("calibrate_schedule: the precision schedule only exists for gcn_precision='f16x3'")
        tol = float(m.schedule_tol if tol is None else tol)
        st_full = prepared if prepared is not None else self.prepare(batch)
        T = diffusion.num_timesteps
        if n_guided is None:
            n_guided = self.guided_steps(diffusion, ddim, cond_grad_weight, guided)
        denom_items = int(denom_items or st_full.B)
        old_tol, m.schedule_tol = m.schedule_tol, tol
        try:
            key = self.schedule_key(diffusion, ddim, n_guided, cond_grad_weight, self.guide_denom(denom_items))
        finally:
            m.schedule_tol = old_tol
        if not force and key in self._sched_cache:
            return self._sched_cache[key]
        # always `bodies` bodies: the finite items of the batch, replicated by index when there are fewer (each copy gets its own noise), so
        # that a first call with B = 2 does not fix k from two bodies for every later batch; items with non-finite inputs are left out (they
        # would turn every trial distance into NaN and cache k = T)
        good = torch.nonzero(st_full.finite).reshape(-1)
        if good.numel() == 0:
            return {"k": int(T), "T": int(T), "f16_steps": 0, "tol_m": tol, "criterion": "no item with finite inputs in the batch: not calibrated, not cached",
                    "bodies": 0, "ddim": bool(ddim), "guided_steps": int(n_guided), "trials": []}
        st = st_full.take(good[torch.arange(int(bodies), device=good.device) % good.numel()])
        nb, dev = st.B, m.device
        sub_batch = dict(batch) if batch is not None else {}

        def loop(noise, lowprec, twoterm=0):
            r = self.run(diffusion, sub_batch, noise, ddim=ddim, guided=guided, cond_grad_weight=cond_grad_weight, prepared=st,
                         denom_items=denom_items, lowprec=lowprec, twoterm=twoterm)
            o = r["other_outputs"]
            return o["pred_vertices"].clone(), o["pred_keypoints_3d"].clone()

        def dist(a, b):
            return max(float((a[0] - b[0]).norm(dim=-1).max()), float((a[1] - b[1]).norm(dim=-1).max()))

        draws, refs, tried = [], [], {}
        for sd_ in seeds:
            g = torch.Generator(device=dev).manual_seed(int(sd_))
            draws.append(torch.randn(T + 1, nb, 144, device=dev, generator=g))
        refs.append(loop(draws[0], 0))
        # the f16 steps never reach into the guided window: the guidance feeds nearest-vertex switches back with gain
        ladder = self._k_ladder(T, floor=(n_guided + 8) if n_guided else 2)

        def err(k, d):
            if (k, d) not in tried:
                tried[(k, d)] = 0.0 if k >= T else dist(loop(draws[d], T - k), refs[d])
            return tried[(k, d)]

        def err1(k):
            if ladder[-1] > k and len(refs) < 2:          # draw B's reference loop only when a candidate below T reaches the second check
                refs.append(loop(draws[1], 0))
            return err(k, 1)

        idx = self.pick_k(ladder, lambda k: err(k, 0), err1, 0.5 * tol)
        k = ladder[idx]
        # ---- the middle tier: of the k split steps, the first j as two-term products.  Same ladder, same criterion, same draws and references; m = the
        # three-term steps that remain.  (m = k is j = 0, today's schedule: always passes, so the result is always safe.)
        tried2, j = {}, 0
        if getattr(m, "f16x2_steps", 0) == "auto" and k > ladder[0]:
            def err2(mm, d):
                if (mm, d) not in tried2:
                    if d == 1 and len(refs) < 2:
                        refs.append(loop(draws[1], 0))
                    tried2[(mm, d)] = 0.0 if mm >= k else dist(loop(draws[d], T - k, k - mm), refs[d])
                return tried2[(mm, d)]
            j = self.pick_two_term(ladder, k, lambda mm: err2(mm, 0), lambda mm: err2(mm, 1), 0.5 * tol)
        info = {"k": int(k), "T": int(T), "f16_steps": int(T - k), "two_term_steps": int(j), "tol_m": tol,
                "two_term_trials": sorted([{"three_term_steps": mm, "two_term_steps": k - mm, "draw": d, "max_dist_m": e} for (mm, d), e in tried2.items()],
                                          key=lambda r: (r["three_term_steps"], r["draw"])), "criterion": "max vertex/joint distance to the all-f16x3 loop <= tol/2 on two noise draws",
                "bodies": int(nb), "ddim": bool(ddim), "guided_steps": int(n_guided),
                "trials": sorted([{"k": kk, "draw": d, "max_dist_m": e} for (kk, d), e in tried.items()], key=lambda r: (r["k"], r["draw"]))}
        self._sched_cache[key] = info
        self.schedule_info = info
        return info

    def install_schedule(self, diffusion, info, ddim=False, guided=False, cond_grad_weight=1.0, denom_items=1):
        """Adopt a calibration result measured elsewhere (another rank's: egohmr_amd.dist.agree_schedule) for THIS process's weights."""
        T = diffusion.num_timesteps
        n_guided = self.guided_steps(diffusion, ddim, cond_grad_weight, guided)
        assert int(info["T"]) == T, (info["T"], T)
        self._sched_cache[self.schedule_key(diffusion, ddim, n_guided, cond_grad_weight, self.guide_denom(int(denom_items)))] = dict(info)
        self.schedule_info = dict(info)

    @torch.no_grad()
    def measure_gain(self, batch=None, timesteps=(0,), prepared=None, bodies=16, delta=1e-2, seed=7):
        """Directional sensitivity of the loaded denoiser, || x0(x_t + d) - x0(x_t) || / || d || for a random direction d at x_t ~ N(0, 1),
        averaged over `bodies` items, per ORIGINAL timestep - the J that decides whether early rounding errors are contracted
        (calibrate_schedule).  Evaluated through the product's own denoiser in its f32-grade arithmetic."""
        m = self.model
        st = (prepared if prepared is not None else self.prepare(batch)).take(bodies)
        g = torch.Generator(device=m.device).manual_seed(seed)
        x = torch.randn(st.B, 144, device=m.device, generator=g)
        d = torch.randn(st.B, 144, device=m.device, generator=g)
        d = d / d.norm(dim=1, keepdim=True) * delta
        out = {}
        for t in timesteps:
            tv = self.timestep_vectors(torch.tensor([int(t)], device=m.device))[0]
            a = self.denoise_once(st, x, tv).clone()
            b = self.denoise_once(st, (x + d).contiguous(), tv)
            out[int(t)] = float(((b - a).norm(dim=1) / delta).mean())
        return out

    # ------------------------------------------------------------------ S samples of one batch in ONE loop
    @torch.no_grad()
    def run_samples(self, diffusion, batch, noise_stacks, ddim=False, guided=False, cond_grad_weight=1.0, defer_status=False):
        """The reference draws S samples per item with S sequential sampling loops over the same batch (test_egohmr.py:251-266).  The
        samples are independent given the conditioning, so this runs them as loops over g*B bodies (sample-major: body s*B + b) with
        the conditioning replicated by index - the same arithmetic per body (the guidance denominator stays B), fewer launches and
        full-size conv tiles for small B.  g = EgoHMR.loop_bodies // B samples share a loop (at least one): about 256 bodies per loop keep the
        three activation matrices of the chained hidden convs (50 MB each) inside the 256 MB Infinity Cache and give every layer whole rounds
        of tiles - ONE loop over 1280 bodies ran the chain kernel at 0.173 of peak, loops of 256 at 0.188 (profiles/r06r_loop_bodies_ab.txt).
        noise_stacks: S tensors [T+1,B,144].  Returns a list of S result dicts like run()."""
        S = len(noise_stacks)
        st = self.prepare(batch)
        if S == 1:
            return [self.run(diffusion, batch, noise_stacks[0], ddim=ddim, guided=guided, cond_grad_weight=cond_grad_weight, prepared=st,
                             defer_status=defer_status)]
        B = st.B
        width = int(getattr(self.model, "loop_bodies", 0) or 0)
        g = S if width <= 0 else max(1, min(S, width // max(B, 1)))
        outs = []
        for s0 in range(0, S, g):
            outs += self._run_sample_group(diffusion, batch, st, noise_stacks[s0:s0 + g], ddim, guided, cond_grad_weight, defer_status)
        # leave the model's per-call attributes as S sequential calls would: un-replicated inputs, the last sample's bodies
        m = self.model
        m.scene_pcd_verts, m.input_transl = st.scene, st.transl
        m.focal_length, m.camera_center_full = m.focal_length[:B], m.camera_center_full[:B]
        last = outs[-1]["other_outputs"]
        m.smpl_output = smpl_mod.SMPLOutput(vertices=last["pred_vertices"], joints=last["pred_keypoints_3d"],
                                            full_pose=torch.cat([last["pred_smpl_params"]["global_orient"], last["pred_smpl_params"]["body_pose"]], dim=1))
        return outs

    def _run_sample_group(self, diffusion, batch, st, noise_stacks, ddim, guided, cond_grad_weight, defer_status):
        """S samples of the prepared batch `st` as ONE loop over S*B bodies -> S result dicts."""
        S, B, T = len(noise_stacks), st.B, diffusion.num_timesteps
        run = partial(self.run, diffusion, dict(batch), ddim=ddim, guided=guided, cond_grad_weight=cond_grad_weight, denom_items=B, defer_status=defer_status)
        if S == 1:
            return [run(noise_stack=noise_stacks[0], prepared=st)]
        res = run(noise_stack=torch.cat([_lib.f32(n, self.model.device)[: T + 1] for n in noise_stacks], dim=1), prepared=st.tile(S))

        def split(x):
            if torch.is_tensor(x):
                return list(x.reshape(S, B, *x.shape[1:]).unbind(0)) if x.dim() >= 1 and x.shape[0] == S * B else [x] * S
            if isinstance(x, dict):
                parts = {k: split(v) for k, v in x.items()}
                return [{k: parts[k][i] for k in x} for i in range(S)]
            return [x] * S
        return split(res)

    # ------------------------------------------------------------------ whole loop
    @torch.no_grad()
    def run(self, diffusion, batch, noise_stack, ddim=False, guided=False, cond_grad_weight=1.0, trace=False, prepared=None, denom_items=None,
            defer_status=False, lowprec=None, twoterm=None):
        """p_sample_loop / ddim_sample_loop (gaussian_diffusion.py:391-508 / :618-718) in one native call.
        Returns the reference's dict(sample, pred_xstart, other_outputs).  The in-loop guidance is the build's collision proxy: a guided call on a
        model with `collision_model` attached raises (the samplers of diffusion.py route such a loop step by step through model.guide_coll)."""
        m = self.model
        if guided and getattr(m, "collision_model", None) is not None:
            raise _lib.EgoHMRHipError("FusedSampler.run(guided=True): the one-call loop cannot call the attached collision_model between steps and will "
                                      "not fall back to the build's proxy; sample through diffusion.p_sample_loop / ddim_sample_loop / val_losses")
        call = dict(diffusion=diffusion, batch=batch, noise_stack=noise_stack, ddim=ddim, guided=guided, cond_grad_weight=cond_grad_weight, trace=trace,
                    prepared=prepared, denom_items=denom_items)
        with _lib.on_device(m.device):
            try:
                return self._run_on_device(**call, defer_status=defer_status, lowprec=lowprec, twoterm=twoterm)
            except _lib.EgoHMRRangeError:
                # an activation left the f16 range and was clamped (status bit 2 of the handle, raised by the conv kernels' stores): never silent.
                # on_saturation = 'f32': this checkpoint gets float32 activations from now on (exact-f32 MFMA path, ~3x slower) and the call runs again
                if m.on_saturation != "f32" or m.gcn_precision == "f32":
                    raise
                import warnings
                warnings.warn("egohmr_amd: a denoiser activation reached the f16 range (|x| >= 65504) and was clamped in the split-f16 / f16 path; "
                              "EgoHMR.on_saturation = 'f32': switching this model to gcn_precision = 'f32' and re-running the call", RuntimeWarning)
                m.gcn_precision = "f32"
                return self._run_on_device(**call, defer_status=False, lowprec=None, twoterm=None)

    def _run_on_device(self, *, diffusion, batch, noise_stack, ddim, guided, cond_grad_weight, trace, prepared, denom_items, defer_status, lowprec, twoterm):
        m = self.model
        nonlocal_ci = m.diffusion_model.non_local.inter_channels if m.diffusion_model.nonlocal_layer else 0
        if nonlocal_ci and m.gcn_precision == "f16":
            raise _lib.EgoHMRHipError(m.diffusion_model.NONLOCAL_F16)
        if self._status_event is not None and self._status_event.query():   # a deferred status word of an earlier call has arrived: look at it now
            self.check_status()
        scales = m.sampling_scales()                      # (raises on a non-finite scale before any device call)
        st = prepared if prepared is not None else self.prepare(batch, scales=scales)
        if m.fuse_passes(scales) == 2:
            st = st.with_need(need_all_items(scales))     # (a `prepared` batch made under the other need rule: its pass map again, nothing else)
        B, T = st.B, diffusion.num_timesteps
        noise = _lib.f32(noise_stack, m.device)
        assert noise.shape[0] >= T + 1 and noise.shape[1] == B and noise.shape[2] == 144, noise.shape
        steps, first_guided = self.step_table(diffusion, ddim, cond_grad_weight, guided)
        any_guided = first_guided < T
        tvecs = self.timestep_vectors([diffusion.timestep_map[i] for i in range(T - 1, -1, -1)])   # [T,2,hid]
        if nonlocal_ci:
            lowprec, twoterm = 0, 0                       # the block reads float32 features: no plain-f16 steps (and the loop keeps one arithmetic)
        elif lowprec is None:
            lowprec, twoterm = self._scheduled_lowprec(diffusion=diffusion, batch=batch, st=st, ddim=ddim, guided=guided, cond_grad_weight=cond_grad_weight,
                                                       n_guided=T - first_guided, denom_items=denom_items or B)
        twoterm = int(twoterm or 0) if m.gcn_precision == "f16x3" else 0   # (an explicit lowprec without twoterm: no two-term step)
        self.last_lowprec = int(lowprec)                  # leading steps of THIS call on plain f16 operands
        self.last_twoterm = twoterm                       # ... and behind them on two-term split-f16 products
        desc, nbytes = self._describe(st=st, T=T, ddim=ddim, any_guided=any_guided, denom_items=denom_items or B, lowprec=lowprec, nonlocal_ci=nonlocal_ci,
                                      twoterm=twoterm, scales=scales)
        gcn, smpl_h = self.gcn(), m.smpl.handle()
        launch = partial(self._launch, gcn=gcn, smpl_h=smpl_h, desc=desc, steps=steps, nbytes=nbytes, any_guided=any_guided)
        ins = dict(h_img=st.h_img, h_oth=st.h_oth, vis=st.vis, tvecs=tvecs, noise=noise[: T + 1].contiguous(), betas=st.betas, scene=st.scene)
        graph = m.use_hip_graph is True or (m.use_hip_graph == "auto" and desc.passes * B <= 64)
        tr = torch.empty(T, B, 144, device=m.device) if trace else None
        with torch.cuda.device(m.device):
            if graph and not any_guided and not trace:
                o = self._replay(launch=launch, gcn=gcn, smpl_h=smpl_h, desc=desc, steps=steps, nbytes=nbytes, st=st, ins=ins)
            else:
                o = SimpleNamespace(**ins, **self._out_bufs(B))
                launch(bufs=o, ws=self._workspace(nbytes, m.device), tr=tr)
        return self._finish(batch=batch, st=st, o=o, tr=tr, noise=noise, T=T, guided_ddim=ddim and any_guided, gcn=gcn, defer_status=defer_status)

    def _scheduled_lowprec(self, *, diffusion, batch, st, ddim, guided, cond_grad_weight, n_guided, denom_items):
        """(leading plain-f16 steps, two-term steps behind them) by EgoHMR.f16x3_last_steps / f16x2_steps; 'auto' = the k and j calibrated for THESE
        weights and THIS sampler, measured now if need be."""
        m, skey = self.model, None
        if m.f16x3_last_steps == "auto" and m.gcn_precision == "f16x3":
            skey = self.schedule_key(diffusion, ddim, n_guided, cond_grad_weight, self.guide_denom(denom_items))
            if skey not in self._sched_cache and m.auto_calibrate:
                self.calibrate_schedule(diffusion, batch, ddim=ddim, guided=guided, cond_grad_weight=cond_grad_weight, prepared=st,
                                        denom_items=denom_items, n_guided=n_guided)
            self.schedule_info = self._sched_cache.get(skey)
        lowprec = self.lowprec_steps(diffusion.num_timesteps, n_guided, ddim, key=skey)
        return lowprec, self.twoterm_steps(diffusion.num_timesteps, lowprec, key=skey)

    def _describe(self, *, st, T, ddim, any_guided, denom_items, lowprec, nonlocal_ci, twoterm=0, scales=None):
        """(the loop's descriptor, its workspace size) after giving the handle this batch's pass map.  scales: the call's guidance scales (None: the
        model's); passes = 2 unless both are 1 - also for a diffuse_fuse=False model under a wrapper's outer scale."""
        m = self.model
        scales = m.sampling_scales() if scales is None else scales
        passes = m.fuse_passes(scales)
        cfg = self._cfg_kernels(passes, scales)
        _, num_masked = self._apply_pass_map(st, passes)
        # ... and how the loop's steps combine the two passes (a setting of the handle, read by ehm_sample_loop at entry like the map)
        self.last_fuse = (int(cfg), float(scales[0]) if cfg else 1.0, float(scales[1]) if cfg else 0.0)
        _lib.api().ehm_gcn_set_fuse_scales(self.gcn(), *self.last_fuse)
        # ... and which collision term its guided steps run: the SMPL handle's mesh, set under collision_proxy = 'mesh' and cleared otherwise (an
        # upload only when that changes), so that a model switched back to 'vertex' runs the vertex proxy's bits again
        m.smpl.set_collision_mesh(m.mesh_collision())
        desc = _lib.SampleDesc(B=st.B, passes=passes, num_steps=T, ddim=int(ddim), per_step_launches=int(bool(m.per_step_launches)),
                               lbs_every_step=int(m.lbs_every_step), num_scene_points=st.scene.shape[1] if any_guided else 0,
                               guide_denom=self.guide_denom(denom_items), tau=m.collision_tau, num_masked=num_masked,
                               guide_all_points=int(bool(m.guide_all_points)), lowprec_steps=int(lowprec), nonlocal_ci=int(nonlocal_ci), twoterm_steps=int(twoterm))
        return desc, _lib.api().ehm_sample_workspace_bytes(C.byref(desc), m.diffusion_model.hid_dim, m.smpl.num_verts)

    def _out_bufs(self, B):
        smpl = self.model.smpl
        shapes = dict(x_final=(144,), x0=(144,), verts=(smpl.num_verts, 3), joints=(smpl.num_joints_out, 3), R=(24, 3, 3), pose6d=(144,))
        return {k: torch.empty(B, *shape, device=self.model.device) for k, shape in shapes.items()}

    def _launch(self, *, gcn, smpl_h, desc, steps, nbytes, any_guided, bufs, ws, tr):
        mean, std = self.model._std_mean()
        _lib.api().ehm_sample_loop(gcn, smpl_h, C.byref(desc), steps, bufs.h_img, bufs.h_oth, bufs.vis, self._folded.Wx, bufs.tvecs, bufs.noise,
                                   bufs.scene if any_guided else None, bufs.betas, mean, std, bufs.x_final, bufs.x0, bufs.verts, bufs.joints, bufs.R,
                                   bufs.pose6d, tr, ws, nbytes, _lib.stream_ptr())

    def _replay(self, *, launch, gcn, smpl_h, desc, steps, nbytes, st, ins):
        """hipGraph route: the loop's launches are captured once per (shape, schedule) with every pointer inside persistent buffers; a call
        copies its inputs in, replays, and copies the results out."""
        m, dev = self.model, self.model.device
        ins = dict(ins, mask_items=st.mask_items, mask_slot=st.mask_slot)      # (the captured kernels read the pass map through persistent arrays too)
        mean, std = m._std_mean()
        # (every pointer the captured launches bake in that is not inside `bufs`: the two native handles - by serial, a recreated handle
        # can reuse a destroyed one's address - and the mean / std buffers)
        key = (st.B, desc.num_steps, desc.ddim, desc.passes, desc.lbs_every_step, desc.lowprec_steps, desc.twoterm_steps, self.last_fuse, m.gcn_precision, gcn.serial,
               bytes(steps), st.scene.shape[1], desc.num_masked, smpl_h.serial,
               mean.data_ptr(), std.data_ptr(), self._folded.Wx.data_ptr(), self._nl_set)
        ent = self._graphs.get(key)
        if ent is None:
            if len(self._graphs) >= 8:
                self._graphs.clear()
            bufs = SimpleNamespace(**{k: torch.empty_like(v) for k, v in ins.items()}, **self._out_bufs(st.B))
            ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
            for k, v in ins.items():
                getattr(bufs, k).copy_(v)
            if desc.num_masked >= 0:
                _lib.api().ehm_gcn_set_pass_map(gcn, bufs.mask_items if desc.num_masked else None, bufs.mask_slot, desc.num_masked)
            launch(bufs=bufs, ws=ws, tr=None)                # eager once: every lazy allocation inside the library happens here
            torch.cuda.synchronize(dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                launch(bufs=bufs, ws=ws, tr=None)
            ent = self._graphs[key] = SimpleNamespace(graph=g, bufs=bufs, ws=ws)
        for k, v in ins.items():
            getattr(ent.bufs, k).copy_(v)
        ent.graph.replay()
        return SimpleNamespace(**{k: getattr(ent.bufs, k).clone() for k in ("x_final", "x0", "verts", "joints", "R", "pose6d")})

    def _finish(self, *, batch, st, o, tr, noise, T, guided_ddim, gcn, defer_status):
        """The call's result dict (ehm_pack_outputs) and its status read."""
        m, A = self.model, _lib.api()
        # non-finite noise: x_T or a step's draw poisons the item from the next denoiser evaluation on; the LAST step's draw is multiplied by
        # nonzero_mask = 0 (DDIM: by sigma = 0 too) and 0 * NaN = NaN lands in that element of `sample` only (gaussian_diffusion.py:357-359, :575-580)
        self.last_trace = tr
        if tr is not None:
            batch["x_t"] = tr[-1]
        batch["vis_mask_smpl"] = st.vis_bool
        out = m._pack_output(batch, st, o.x0, o.pose6d, o.R, o.verts, o.joints, chk=noise, chk_rows=T, last_noise=noise[T], x_final=o.x_final)
        # a chained launch that gave up on a producer wait (GPU shared / preempted) flags the handle instead of hanging: one read-back
        # per sampling call (the call's only host wait, after everything has been enqueued) turns that into an exception rather than
        # silently wrong bodies
        # defer_status (throughput pipelines that keep batches in flight): the word is copied to pinned memory in stream order and
        # looked at by the NEXT call / by check_status(); the host does not wait here.  The flag is sticky on the device.
        with torch.cuda.device(m.device):
            if defer_status:
                if self._status_host is None:
                    self._status_host = torch.zeros(1, dtype=torch.int32).pin_memory()
                A.ehm_gcn_stack_status_async(gcn, self._status_host.data_ptr(), _lib.stream_ptr())
                self._status_event = torch.cuda.Event()
                self._status_event.record()
            else:
                A.ehm_gcn_stack_status(gcn, _lib.stream_ptr())
                m.backbone.check_status()                 # (the stream has been waited for: the trunk's stream-K time-out word is there)
        # ddim_sample_with_grad hands out the GUIDED x0 of its last step as pred_xstart (gaussian_diffusion.py:587-592) while other_outputs keep the model's own;
        # that step has alpha_bar_prev = 1, so its sample IS the guided x0 (x0g * 1 + 0 * eps)
        return {"sample": o.x_final, "pred_xstart": o.x_final if guided_ddim else o.x0, "other_outputs": out}

    def check_status(self):
        """Raise if a sampling call issued with defer_status=True flagged its chained launches (see run()), or if a stream-K conv of the ResNet-50
        trunk timed out in a hand-off (ResNet50Features.check_status).  Waits for that call."""
        self.model.backbone.check_status()
        if self._status_event is None:
            return
        self._status_event.synchronize()
        self._status_event = None
        if int(self._status_host[0]) != 0:
            self._status_host.zero_()
            with torch.cuda.device(self.model.device):
                _lib.api().ehm_gcn_stack_status(self.gcn(), _lib.stream_ptr())
