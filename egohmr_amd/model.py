"""EgoHMR stage-2 model with the reference's constructor / call surface, executing on libegohmr_hip.

Reference seams honoured (models/egohmr/egohmr.py):
  EgoHMR(cfg, device, body_rep_mean, body_rep_std, with_focal_length, with_bbox_info, with_cam_center, ...)   :29-40
  .forward(batch, timesteps) -> dict(pred_x_start, pred_smpl_params, pred_pose_6d, pred_keypoints_3d,
                                     pred_vertices, pred_keypoints_3d_full, pred_keypoints_2d_full)          :173-303
  .validation_setup()  :475-484     .guide_coll(batch, output, t, compute_grad)  :517-605
  .eval_coll(output)   :487-514     .parameters() / load_state_dict(strict=False) with the reference's names
plus ``fused_sampler`` (build extension) which diffusion.py uses to run the whole sampling loop natively.

What is different by design: the encoders (ResNet-50, scene PointNet), the translation / beta heads and
the conditioning + timestep slices of the GCN input conv do not depend on x_t, so they are evaluated once
per batch (``prepare``) instead of once per denoising step (egohmr.py:183,:214 sit inside forward); the
denoiser, rot6d->rotmat, SMPL LBS and the sampler update are hand-written HIP kernels (csrc/*.hip).
"""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import _lib, gcn_grad, geometry, loss_grad, split_gemm, synthetic, train_grad
from . import smpl as smpl_mod
from .encoders import ResnetPointnet, ResNet50Features
from .fused import PRECISIONS, FusedSampler  # noqa: F401  (PRECISIONS re-exported)

OPENPOSE_TO_SMPL = [8, 12, 9, 8, 13, 10, 8, 14, 11, 8, 14, 11, 0, 5, 2, 0, 5, 2, 6, 3, 7, 4, 7, 4]           # egohmr.py:111
OPENPOSE_TO_SMPL_LOOSE = [8, 13, 10, 8, 13, 10, 8, 14, 11, 8, 14, 11, 1, 5, 2, 0, 5, 2, 6, 3, 7, 4, 7, 4]     # egohmr.py:114
IMG_DIM = 2048          # columns of the GCN input feature: img 2048 | scene + transl + cam | x_t embed 512 | timestep embed 512 (EgoHMR.cond_split)
GRAD_ZERO_JOINTS = [0, 3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23]                               # egohmr.py:567


def default_cfg():
    """The yacs keys the sampling path reads (configs/prohmr.yaml:41-56)."""
    return SimpleNamespace(MODEL=SimpleNamespace(BACKBONE=SimpleNamespace(NUM_LAYERS=50, OUT_CHANNELS=2048)),
                           CAM=SimpleNamespace(FX_NORM_COEFF=1500.0), EXTRA=SimpleNamespace(FOCAL_LENGTH=5000.0),
                           TRAIN=SimpleNamespace(LR=1e-4, WEIGHT_DECAY=1e-4))


def smpl_tree_adjacency() -> torch.Tensor:
    """egohmr.py:86-93: symmetric SMPL-tree adjacency, rows normalised, diagonal forced to one."""
    a = np.zeros((24, 24), dtype=np.float32)
    for p, c in synthetic.SMPL_EDGES:
        a[p, c] = a[c, p] = 1.0
    a = a / a.sum(1, keepdims=True)
    np.fill_diagonal(a, 1.0)
    return torch.from_numpy(a)


# ---------------------------------------------------------------------------------------------- parameter holders
class ModulatedGraphConv(nn.Module):
    """Parameters of modulated_gcn_conv.py:16-37 (the arithmetic lives in csrc/gcn.hip)."""

    def __init__(self, in_features, out_features, adj):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.W = nn.Parameter(torch.empty(2, in_features, out_features))
        self.M = nn.Parameter(torch.empty(adj.size(0), out_features))
        self.adj2 = nn.Parameter(torch.full_like(adj, 1e-6))
        self.bias = nn.Parameter(torch.empty(out_features))
        nn.init.xavier_uniform_(self.W.data, gain=1.414)
        nn.init.xavier_uniform_(self.M.data, gain=1.414)
        bound = 1.0 / np.sqrt(out_features)
        nn.init.uniform_(self.bias, -bound, bound)


class _GraphConv(nn.Module):
    def __init__(self, adj, cin, cout):
        super().__init__()
        self.gconv = ModulatedGraphConv(cin, cout, adj)
        self.bn = nn.BatchNorm1d(cout)


class _ResGraphConv(nn.Module):
    def __init__(self, adj, dim):
        super().__init__()
        self.gconv1 = _GraphConv(adj, dim, dim)
        self.gconv2 = _GraphConv(adj, dim, dim)


class _NonLocalBlock(nn.Module):
    """Parameter tree of NONLocalBlock2D(in_channels=hid, sub_sample=False, bn_layer=True)
    (nets/non_local_embedded_gaussian.py:6-58): g / theta / phi 1x1 convs hid -> hid/2, W = Sequential(conv hid/2 -> hid, BatchNorm2d)
    with the reference's zero-initialised BatchNorm affine (identity block until trained)."""

    def __init__(self, hid_dim):
        super().__init__()
        ci = max(hid_dim // 2, 1)
        self.inter_channels = ci
        self.g = nn.Conv2d(hid_dim, ci, 1)
        self.theta = nn.Conv2d(hid_dim, ci, 1)
        self.phi = nn.Conv2d(hid_dim, ci, 1)
        self.W = nn.Sequential(nn.Conv2d(ci, hid_dim, 1), nn.BatchNorm2d(hid_dim))
        nn.init.constant_(self.W[1].weight, 0)
        nn.init.constant_(self.W[1].bias, 0)


class ModulatedGCN(nn.Module):
    """modulated_gcn.py:60-97 parameter tree: gconv_input.0, gconv_layers.{b}.gconv{1,2}, gconv_output."""

    def __init__(self, adj, in_dim, out_dim=6, hid_dim=1024, num_layers=4, nonlocal_layer=False, p_dropout=0.0):
        super().__init__()
        self.register_buffer("adj", adj.clone(), persistent=False)
        self.in_dim, self.hid_dim, self.out_dim, self.num_layers = in_dim, hid_dim, out_dim, num_layers
        self.gconv_input = nn.Sequential(_GraphConv(adj, in_dim, hid_dim))
        self.gconv_layers = nn.Sequential(*[_ResGraphConv(adj, hid_dim) for _ in range(num_layers)])
        self.gconv_output = ModulatedGraphConv(hid_dim, out_dim, adj)
        self.nonlocal_layer = bool(nonlocal_layer)
        self.p_dropout = p_dropout                                  # modulated_gcn.py:68: read by the train-mode route only (it has no dropout)
        if self.nonlocal_layer:                                     # modulated_gcn.py:93-94, reference parameter names
            self.non_local = _NonLocalBlock(hid_dim)
        self._nl_packed = self._nl_key = None                       # nonlocal_packed()
        self._nat = self._nat_key = self._nat_keyfn = None          # _native()

    # ------------------------------------------------------------------ native handle (ehm_gcn_create) - shared with FusedSampler.gcn()
    def create_native_handle(self, device):
        """ehm_gcn_create on this module's parameters -> (handle, tensors that must stay alive while it lives).  The caller destroys it."""
        keep = []

        def params(gc, bn):
            def t(x):
                x = _lib.f32(x, device)
                keep.append(x)
                return _lib.ptr(x)
            p = _lib.GConvParams()
            p.W, p.M, p.adj2, p.bias = t(gc.W), t(gc.M), t(gc.adj2), t(gc.bias)
            if bn is not None:
                p.bn_weight, p.bn_bias, p.bn_mean, p.bn_var = t(bn.weight), t(bn.bias), t(bn.running_mean), t(bn.running_var)
            p.in_dim, p.out_dim = gc.in_features, gc.out_features
            return p

        gi = self.gconv_input[0]
        inp = params(gi.gconv, gi.bn)
        hidden = []
        for blk in self.gconv_layers:
            hidden += [params(blk.gconv1.gconv, blk.gconv1.bn), params(blk.gconv2.gconv, blk.gconv2.bn)]
        outp = params(self.gconv_output, None)
        arr = (_lib.GConvParams * len(hidden))(*hidden)
        adj = _lib.f32(self.adj, device)
        keep.append(adj)
        h = C.c_void_p()
        with torch.cuda.device(device):
            _lib.api().ehm_gcn_create(C.byref(h), adj, C.byref(inp), arr, len(hidden), C.byref(outp), self.hid_dim, _lib.stream_ptr())
        return h, keep

    # ------------------------------------------------------------------ the optional non-local block (modulated_gcn.py:93-94, :104-110)
    def nonlocal_packed(self):
        """The non-local block's two 1x1-conv GEMMs as split_gemm.Packed operands: [theta | phi | g], and W.0 with BatchNorm(eval) folded, each with its
        bias; and the weight key they were packed for: re-packed when a parameter of the block changes.  (pack_weight's K padding and column rounding
        change nothing here: a native handle needs hid_dim % 64 == 0, so K = hid or hid / 2 is a multiple of 32 and Co = 3 hid / 2 or hid one of 8.)"""
        nl = self.non_local
        key = tuple((p.data_ptr(), p._version) for p in list(nl.parameters()) + list(nl.buffers()))
        if self._nl_key != key:
            pack = lambda w2, bias: split_gemm.pack_weight(w2.detach(), bias.detach().float().contiguous())
            wqkv = torch.cat([nl.theta.weight, nl.phi.weight, nl.g.weight], 0).flatten(1).float()
            bqkv = torch.cat([nl.theta.bias, nl.phi.bias, nl.g.bias], 0)
            bn = nl.W[1]
            sc = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
            ww = (nl.W[0].weight.flatten(1).double() * sc[:, None]).float()
            bw = ((nl.W[0].bias.double() - bn.running_mean.double()) * sc + bn.bias.double()).float()
            with _lib.on_device(wqkv.device):
                self._nl_packed, self._nl_key = (pack(wqkv, bqkv), pack(ww, bw)), key
        return self._nl_packed, self._nl_key

    @torch.no_grad()
    def non_local_native(self, X, rows, rows_pad):
        """NONLocalBlock2D on the joint axis (modulated_gcn.py:104-110): [theta|phi|g] as ONE 1x1-conv GEMM and W + BatchNorm(eval,
        folded) + residual as another, both on ehm_conv_nhwc_split (rows = N, H = W = 1); the 24 x 24 softmax attention per body
        in ehm_nonlocal_attention.  X: float32 [rows_pad, hid] -> the same."""
        qkv_w, out_w = self.nonlocal_packed()[0]
        qkv = split_gemm.gemm_rows(X, qkv_w, rows)
        y = torch.empty(rows, self.non_local.inter_channels, device=X.device)
        _lib.api().ehm_nonlocal_attention(qkv, y, rows // 24, y.shape[1], _lib.stream_ptr())
        return split_gemm.gemm_rows(y, out_w, rows, res=X, out=torch.zeros(rows_pad, self.hid_dim, device=X.device))

    # ------------------------------------------------------------------ everything after the input conv (forward below, FusedSampler.denoise_once)
    NONLOCAL_F16 = "the optional non-local GCN block runs on float32 features; use precision 'f16x3' or 'f32' (EgoHMR.gcn_precision, ModulatedGCN.precision) with it"

    @torch.no_grad()
    def denoiser_tail(self, h, fill, *, rows, B, passes, vis, precision, device, scales=None):
        """x0 [B, 144] from the native handle `h`: fill(X0) writes the input conv's `rows` rows into a zeroed [rows_pad, hid] buffer, then the residual blocks as
        ONE chained launch, the optional non-local block and gconv_output (vis / passes: the image-masked second pass).  precision: its name, as set on `h`.
        scales = (s_vis, s_inv): the two passes are combined per joint as u + s (c - u) (ehm_gcn_output_layer_cfg); None = the visibility select."""
        A = _lib.api()
        tile = A.ehm_gcn_row_tile()
        rows_pad = (rows + tile - 1) // tile * tile
        X = [torch.zeros(rows_pad, self.hid_dim, device=device) for _ in range(3)]
        s = _lib.stream_ptr()
        fill(X[0])
        bufs = (C.c_void_p * 3)(*map(_lib.ptr, X))
        res = C.c_int(0)
        A.ehm_gcn_hidden_stack(h, bufs, rows_pad, C.byref(res), s)
        feat = X[res.value]
        if self.nonlocal_layer:
            if precision == "f16":
                raise _lib.EgoHMRHipError(self.NONLOCAL_F16)
            feat = self.non_local_native(feat, rows, rows_pad)
        x0 = torch.empty(B, 144, device=device)
        if scales is None:
            A.ehm_gcn_output_layer(h, feat, vis, x0, B, passes, s)
        else:
            A.ehm_gcn_output_layer_cfg(h, feat, vis, x0, B, passes, float(scales[0]), float(scales[1]), s)
        return x0

    # ------------------------------------------------------------------ ModulatedGCN.forward on its own (modulated_gcn.py:99-116)
    precision = "f16x3"      # arithmetic of the standalone call: 'f16x3' (f32-grade, default) | 'f32' | 'f16' (fused.PRECISIONS)

    def _native(self, device):
        """(handle set to `precision`, gcn_grad.ConvWeights of every conv in the handle's order: the packed GEMM operands, made on first use) for forward():
        rebuilt when a parameter changes; its own handle (EgoHMR.fused_sampler's carries the sampler's pass map / precision schedule)."""
        if self._nat_keyfn is None:
            self._nat_keyfn = _lib.TensorKey(self)
        key = (self._nat_keyfn(), str(device))
        if self._nat_key != key:
            if self._nat is not None:
                self._nat[0].close()
            h, keep = self.create_native_handle(device)
            h = _lib.Handle(h, _lib.api().ehm_gcn_destroy, keep)
            self._nat, self._nat_key = (h, [gcn_grad.ConvWeights(_lib.f32(gc.W, device)) for gc, _ in self._convs()]), key
        A, h = _lib.api(), self._nat[0]
        if A.ehm_gcn_get_precision(h) != PRECISIONS[self.precision]:
            A.ehm_gcn_set_precision(h, PRECISIONS[self.precision])
        return self._nat

    def _input_gemm(self, x, cw):
        """The input conv's GEMM: x [B, 24, in_dim] -> (x as float32 rows [24 B, in_dim padded to 32], pre = x @ [W[0] | W[1]] [24 B, 2 hid])."""
        xp = split_gemm.pad_cols(_lib.f32(x).reshape(-1, self.in_dim), cw.fwd.buf.shape[1])
        return xp, split_gemm.gemm_rows(xp, cw.fwd)

    # ------------------------------------------------------------------ the autograd route (gcn_grad.GCNFunction; csrc/gcn_bwd.hip)
    # False: a call under grad mode differentiates w.r.t. x only (x.requires_grad) and leaves the parameters' .grad alone; True: it also reaches W, M, adj2, bias of
    # every conv and bn.weight / bn.bias of the input and hidden convs (eval-mode BatchNorm: frozen statistics) - those of them that require grad
    grad_params = False

    def _convs(self):
        """(gconv, bn or None) of every conv in the order of the native handle: input conv, hidden convs, output conv."""
        gi = self.gconv_input[0]
        out = [(gi.gconv, gi.bn)]
        for blk in self.gconv_layers:
            out += [(blk.gconv1.gconv, blk.gconv1.bn), (blk.gconv2.gconv, blk.gconv2.bn)]
        return out + [(self.gconv_output, None)]

    def grad_parameters(self):
        """The parameters the autograd route differentiates, in GCNFunction's order."""
        out = []
        for gc, bn in self._convs():
            out += [gc.W, gc.M, gc.adj2, gc.bias] + ([bn.weight, bn.bias] if bn is not None else [])
        if self.nonlocal_layer and self.nonlocal_grad:          # appended (gcn_grad.NONLOCAL_PARAMS): the convs keep their 6 ci + k places
            nl = self.non_local
            out += [nl.theta.weight, nl.theta.bias, nl.phi.weight, nl.phi.bias, nl.g.weight, nl.g.bias, nl.W[0].weight, nl.W[0].bias, nl.W[1].weight, nl.W[1].bias]
        return out

    # False: every route that needs a backward refuses a module with the non-local block, as ever.  True: the block runs on those routes too, between the last
    # residual add and gconv_output, with its backward in HIP (gcn_grad.nonlocal_forward / nonlocal_backward; csrc/nonlocal_bwd.hip): grad_parameters() ends with
    # its ten parameters, under .train() + train_batchnorm its BatchNorm2d (W.1) runs on batch statistics - all ranks' behind stat_sync.  Inference does not
    # depend on it
    nonlocal_grad = False

    def nonlocal_weights(self, device):
        """gcn_grad.NonLocalWeights of the block for the eval-mode autograd route: re-made when one of its conv parameters changes."""
        nl = self.non_local
        key = (str(device),) + tuple((p.data_ptr(), p._version) for m in (nl.theta, nl.phi, nl.g, nl.W[0]) for p in m.parameters())
        if getattr(self, "_nlw_key", None) != key:
            self._nlw, self._nlw_key = gcn_grad.NonLocalWeights(nl, device), key
        return self._nlw

    def _wants_grad(self, x):
        return torch.is_grad_enabled() and (x.requires_grad or (self.grad_params and any(p.requires_grad for p in self.grad_parameters())))

    # False: a call under .train() is refused.  True: it runs BatchNorm1d as torch does in training mode - batch statistics over all 24 B rows, the running
    # statistics and num_batches_tracked updated in place, a backward through the mean and the variance (gcn_grad.GCNTrainFunction; csrc/gcn_train.hip).
    # eval() calls do not depend on it
    train_batchnorm = False
    # A dist.StatSync, set for a call by EgoHMR.training_step behind EgoHMR.data_parallel: the train-mode route's BatchNorm statistics and their backward
    # sums then run over ALL ranks' rows (one all-gather per BatchNorm each way, also under no_grad).  None: this process's rows, today's calls
    stat_sync = None

    def _check_train(self):
        """What the train-mode route cannot run, refused before any device call."""
        if self.p_dropout is not None and self.p_dropout != 0:
            raise NotImplementedError(f"ModulatedGCN.forward: the train-mode route has no dropout (p_dropout = {self.p_dropout}); use p_dropout = None or 0")
        if self.nonlocal_layer and not self.nonlocal_grad:
            raise NotImplementedError("ModulatedGCN.forward: the non-local block has no backward; the train-mode route needs nonlocal_layer=False"
                                      " (or ModulatedGCN.nonlocal_grad = True, which turns the block's backward on)")
        if self.precision == "f16":
            raise _lib.EgoHMRHipError(self.GRAD_F16)
        for _, bn in self._convs()[:-1]:
            if bn.momentum is None or not bn.track_running_stats:
                raise NotImplementedError("ModulatedGCN.forward: the train-mode route updates the running statistics with a fixed momentum; "
                                          "BatchNorm1d(momentum=None) and track_running_stats=False are not built")
            if bn.training != self.training:
                raise ValueError("ModulatedGCN.forward: a BatchNorm1d of the denoiser is in eval mode while the module is in training mode; "
                                 "call .train() / .eval() on the whole ModulatedGCN")
        if self.nonlocal_layer:
            bn = self.non_local.W[1]
            if bn.momentum is None or not bn.track_running_stats:
                raise NotImplementedError("ModulatedGCN.forward: the train-mode route updates the running statistics with a fixed momentum; "
                                          "the non-local block's BatchNorm2d(momentum=None) and track_running_stats=False are not built")
            if bn.training != self.training:
                raise ValueError("ModulatedGCN.forward: the non-local block's BatchNorm2d is in eval mode while the module is in training mode; "
                                 "call .train() / .eval() on the whole ModulatedGCN")

    def _check_input(self, x):
        if self.training:
            if not self.train_batchnorm:
                raise NotImplementedError("ModulatedGCN.forward: inference only (BatchNorm in eval mode, no dropout); training is out of scope (SURVEY.md section 2)")
            self._check_train()
        if not x.is_cuda:
            raise _lib.EgoHMRHipError("ModulatedGCN.forward needs its input on a HIP device; egohmr_amd has no CPU path")
        if x.dim() != 3 or x.shape[1] != 24 or x.shape[2] != self.in_dim:
            raise ValueError(f"ModulatedGCN.forward: expected [B, 24, {self.in_dim}], got {tuple(x.shape)}")
        if self.out_dim != 6:
            raise NotImplementedError("the output-conv kernels are built for out_dim = 6 (the 6-D rotation head, egohmr.py:132)")

    GRAD_F16 = "the autograd route of ModulatedGCN.forward keeps float32 activations for its backward; use precision 'f16x3' or 'f32' (ModulatedGCN.precision) with it"

    def forward(self, x):
        """modulated_gcn.py:99-116 in eval mode on the HIP kernels: x [B, 24, in_dim] -> [B, 24, out_dim=6].

        With grad mode on and x.requires_grad - or `grad_params` set and a parameter that requires grad - the result carries a grad_fn: the same convs one
        launch each with their backward in HIP (gcn_grad.GCNFunction: eval-mode BatchNorm, first derivatives, precision 'f16x3' or 'f32'; the non-local
        block only behind `nonlocal_grad`).  Every other call runs the route below and returns a tensor without grad_fn."""
        self._check_input(x)
        if self.training:                                    # train_batchnorm (_check_input)
            if self._wants_grad(x):
                return gcn_grad.GCNTrainFunction.apply(self, x, *(self.grad_parameters() if self.grad_params else ()))
            return gcn_grad.forward_train(self, x, save=False)[0]
        if self._wants_grad(x):
            return gcn_grad.GCNFunction.apply(self, x, *(self.grad_parameters() if self.grad_params else ()))
        return self._forward_nograd(x)

    @torch.no_grad()
    def _forward_nograd(self, x):
        """forward() without a backward:
        gconv_input as a split-f16 GEMM x @ [W[0] | W[1]] (ehm_conv_nhwc_split, H = W = 1) + ehm_gcn_input_layer_rows (modulation, adjacency mix, bias,
        BatchNorm, ReLU), the residual blocks as ONE chained launch (ehm_gcn_hidden_stack), the optional non-local block, gconv_output
        (ehm_gcn_output_layer).  EgoHMR.forward / the sampler do NOT come through here: they hoist the step-invariant slices of the input feature
        (FusedSampler.prepare) - this is the module's own call surface for a user who feeds it a full feature tensor, as the reference allows."""
        A = _lib.api()
        dev = x.device
        B = x.shape[0]
        with _lib.on_device(dev):
            h, cws = self._native(dev)
            pre = self._input_gemm(x, cws[0])[1]
            s = _lib.stream_ptr()
            out = self.denoiser_tail(h, lambda X0: A.ehm_gcn_input_layer_rows(h, pre, X0, B, s), rows=B * 24, B=B, passes=1, vis=None,
                                     precision=self.precision, device=dev)
            A.ehm_gcn_stack_status(h, s)
        return out.view(B, 24, 6)


class PositionalEncoding(nn.Module):
    def __init__(self, d_model, dropout=0.1, max_len=5000):
        super().__init__()
        self.register_buffer("pe", torch.from_numpy(synthetic.positional_table(max_len, d_model)))


class TimestepEmbedder(nn.Module):
    def __init__(self, latent_dim, sequence_pos_encoder):
        super().__init__()
        self.sequence_pos_encoder = sequence_pos_encoder
        self.time_embed = nn.Sequential(nn.Linear(latent_dim, latent_dim), nn.SiLU(), nn.Linear(latent_dim, latent_dim))

    def forward(self, timesteps):
        return self.time_embed(self.sequence_pos_encoder.pe[timesteps]).permute(1, 0, 2)   # egohmr.py:642-643


class InputProcess(nn.Module):
    def __init__(self, input_dim, latent_dim):
        super().__init__()
        self.poseEmbedding = nn.Linear(input_dim, latent_dim)


class FCHeadBeta(nn.Module):
    def __init__(self, in_dim):
        super().__init__()
        self.layers = nn.Sequential(nn.Linear(in_dim, 1024), nn.ReLU(), nn.Linear(1024, 10))
        self.register_buffer("init_betas", torch.zeros(1, 10))   # data/smpl_mean_params.npz['shape'] in the reference (:669-671)

    def forward(self, feats, pred_pose=None):
        return self.layers(feats) + self.init_betas


class TranslEnc(nn.Module):
    def __init__(self, in_dim=3, out_dim=128):
        super().__init__()
        self.layers = nn.Sequential(nn.Linear(in_dim, 64), nn.ReLU(), nn.Linear(64, out_dim))

    def forward(self, x):
        return self.layers(x)


def val_losses_native(t, weights, penetration=None) -> dict:
    """ehm_val_losses (csrc/loss.hip) on a dict of contiguous device tensors named like the fields of ehm_val_losses_desc (EgoHMR.loss_inputs builds it), the
    nine weights of egohmr.py:422-430 and the per-item penetration term [B] or None -> losses [11], joint_vis_num [1] int64, per_item [B,11],
    per_item_vis [B] int64, vis_mask [B,24] uint8 (columns: _lib.LOSS_KEYS).  No host synchronisation."""
    dev, P, A, n = t["pred_vertices"].device, _lib.ptr, _lib.api(), len(_lib.LOSS_KEYS)
    B, V = t["pred_vertices"].shape[0], t["pred_vertices"].shape[1]
    out = dict(losses=torch.empty(n, device=dev), joint_vis_num=torch.empty(1, device=dev, dtype=torch.int64), per_item=torch.empty(B, n, device=dev),
               per_item_vis=torch.empty(B, device=dev, dtype=torch.int64), vis_mask=torch.empty(B, 24, device=dev, dtype=torch.uint8))
    with _lib.on_device(dev):
        nb = C.c_int64(0)
        A.ehm_val_losses_workspace_bytes(B, V, C.byref(nb))
        nbytes = nb.value
        ws = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
        d = _lib.ValLossesDesc(B=B, V=V, pred_joints=t["pred_keypoints_3d"].shape[1], gt_joints=t["gt_joints_male"].shape[1],
                               kp3d_points=t["keypoints_3d"].shape[1], kp3d_full_points=t["keypoints_3d_full"].shape[1], kp2d_points=t["keypoints_2d"].shape[1],
                               penetration=P(penetration), weights=(C.c_double * 9)(*[float(w) for w in weights]), workspace=P(ws), workspace_bytes=nbytes,
                               **{k: P(v) for k, v in t.items()}, **{k: P(v) for k, v in out.items()})
        A.ehm_val_losses(C.byref(d), _lib.stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------- model
class EgoHMR(nn.Module):
    def __init__(self, cfg=None, device=None, body_rep_mean=None, body_rep_std=None,
                 with_focal_length=False, with_bbox_info=False, with_cam_center=False,
                 scene_feat_dim=512, scene_type="whole_scene", scene_cano=False,
                 weight_loss_v2v=0, weight_loss_keypoints_3d=0, weight_loss_keypoints_3d_full=0, weight_loss_keypoints_2d_full=0,
                 weight_loss_betas=0, weight_loss_body_pose=0, weight_loss_global_orient=0, weight_loss_pose_6d_ortho=0,
                 weight_coap_penetration=0, start_coap_epoch=0, cond_mask_prob=0, only_mask_img_cond=False,
                 diffusion_blk=4, gcn_dropout=0.0, gcn_nonlocal_layer=False, gcn_hid_dim=1024,
                 pelvis_vis_loosen=False, diffuse_fuse=False, smpl_asset=None, smpl_model_path="data/smpl", allow_synthetic_smpl=False,
                 smpl_asset_male=None, smpl_asset_female=None):
        super().__init__()
        self.cfg = cfg if cfg is not None else default_cfg()
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        if not with_focal_length:
            # the reference itself cannot be constructed this way: `if self.with_focal_length or self.with_vfov` (egohmr.py:77) reads an
            # attribute that is never set
            raise AttributeError("'EgoHMR' object has no attribute 'with_vfov' (the reference fails the same way for with_focal_length=False, "
                                 "models/egohmr/egohmr.py:77); pass with_focal_length=True")
        self.with_focal_length, self.with_bbox_info, self.with_cam_center = True, bool(with_bbox_info), bool(with_cam_center)
        self.scene_type, self.scene_cano = scene_type, scene_cano
        self.only_mask_img_cond, self.diffuse_fuse = only_mask_img_cond, diffuse_fuse
        # cond_mask_prob only acts under self.training (mask_cond, egohmr.py:159-168): the sampling path ignores it; the training route of forward
        # (frozen_trunk_training) draws the reference's per-item mask from it (cond_drop_mask) and applies it inside ehm_cond_assemble
        self.cond_mask_prob = float(cond_mask_prob)
        # egohmr.py:121-122, :130-137: read by compute_loss only
        self.weight_loss_v2v, self.weight_loss_keypoints_3d = weight_loss_v2v, weight_loss_keypoints_3d
        self.weight_loss_keypoints_3d_full, self.weight_loss_keypoints_2d_full = weight_loss_keypoints_3d_full, weight_loss_keypoints_2d_full
        self.weight_loss_betas, self.weight_loss_body_pose = weight_loss_betas, weight_loss_body_pose
        self.weight_loss_global_orient, self.weight_loss_pose_6d_ortho = weight_loss_global_orient, weight_loss_pose_6d_ortho
        self.weight_coap_penetration, self.start_coap_epoch = weight_coap_penetration, start_coap_epoch
        # the ground-truth bodies of compute_loss (egohmr.py:106-107), created on first use and kept OUT of the module tree (a plain dict): no key in
        # state_dict(), nothing in parameters(), no cost for a sampling-only user
        self._gt_smpl = {}
        self._gt_smpl_src = dict(model_path=smpl_model_path, allow_synthetic=allow_synthetic_smpl, male=smpl_asset_male, female=smpl_asset_female)
        self.diffuse_feat_dim = 6
        dev = self.device
        self.register_buffer("body_rep_mean_buf", torch.as_tensor(body_rep_mean, dtype=torch.float32).reshape(144).clone(), persistent=False)
        self.register_buffer("body_rep_std_buf", torch.as_tensor(body_rep_std, dtype=torch.float32).reshape(144).clone(), persistent=False)
        self.body_rep_mean, self.body_rep_std = body_rep_mean, body_rep_std

        self.input_process = InputProcess(6, 512)
        self.sequence_pos_encoder = PositionalEncoding(512)
        self.embed_timestep = TimestepEmbedder(512, self.sequence_pos_encoder)
        if self.cfg.MODEL.BACKBONE.NUM_LAYERS != 50:
            raise NotImplementedError("only the ResNet-50 backbone of configs/prohmr.yaml is built")
        self.backbone = ResNet50Features()
        self.scene_enc = ResnetPointnet(out_dim=scene_feat_dim, hidden_dim=256)
        self.transl_enc = TranslEnc(3, 128)
        ctx = self.cfg.MODEL.BACKBONE.OUT_CHANNELS + 1 + (3 if with_bbox_info else 0) + (2 if with_cam_center else 0) + scene_feat_dim + 128   # :74-83
        self.context_feats_dim = ctx
        self.cond_split = (IMG_DIM, ctx, ctx + 512, ctx + 1024)
        self.diffusion_model = ModulatedGCN(adj=smpl_tree_adjacency(), in_dim=ctx + 512 + 512, hid_dim=gcn_hid_dim, out_dim=6,
                                            num_layers=diffusion_blk, nonlocal_layer=gcn_nonlocal_layer)
        self.beta_layer = FCHeadBeta(ctx)
        self.smpl = smpl_mod.create(smpl_model_path, model_type="smpl", gender="neutral", asset=smpl_asset, allow_synthetic=allow_synthetic_smpl)
        self.openpose_to_smpl = OPENPOSE_TO_SMPL_LOOSE if pelvis_vis_loosen else OPENPOSE_TO_SMPL
        self.smpl_to_openpose = [24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34]
        self.collision_tau = 0.05
        # None: the build's nearest-vertex proxy (csrc/guidance.hip), inside the one-call loop.  Else an object with the two calls the reference makes on
        # `self.smpl.coap` (COAP) / `self.smpl_volsmpl.volume` (VolumetricSMPL): collision_loss(points, smpl_output, ret_collision_mask=None) and
        # query(points, smpl_output); guide_coll / eval_coll / _penetration_term then run the reference's autograd route through the differentiable
        # SMPL.forward, and guided loops take the per-step route (the native loop cannot call Python between steps); unguided loops stay fused
        self.collision_model = None
        # What stands in for the collision model while none is attached.  'vertex' (the default): the nearest-vertex proxy, relu(tau - distance to the
        # nearest body vertex)^2.  'mesh': the mesh collision term (include/egohmr_hip.h): occupancy of the posed mesh `smpl.faces_tensor` by its
        # generalised winding number, penetration depth to the nearest face - in the guided loops, guide_coll, eval_coll / eval_coll_volsmpl, the
        # penetration term of compute_loss and its gradient.  The mesh's OWN occupancy, not a COAP / VolumetricSMPL output; meaningful on a closed
        # mesh (the real SMPL asset), defined but fractional on the synthetic asset's random faces.  collision_tau is not used by it.
        self.collision_proxy = "vertex"
        self.guide_reduction = "mean"         # COAP variant: -loss.mean() (egohmr.py:562); 'sum' = VolSMPL variant (egohmr_volsmpl.py:618)
        self.guide_denom_override = None       # sharded / sub-batch runs: the GLOBAL batch size of `-loss.mean()`, else None
        self.guide_all_points = False          # COAP variant: bbox-selected scene points (egohmr.py:550-552); True = all points (egohmr_volsmpl.py:609-612)
        self.lbs_every_step = True             # EgoHMR.forward decodes the body in every step (egohmr.py:276)
        # what a clamped activation does (|x| >= 65504 in an X2 / f16 store of the denoiser: _lib.EgoHMRRangeError from the status word): 'raise', or 'f32' =
        # switch this model to gcn_precision 'f32' (float32 activations, no such limit) and run the call again.  Calls issued with defer_status=True
        # always raise (at check_status(): their results have been handed out already)
        self.on_saturation = "raise"
        # FusedSampler.run_samples: the S samples of an item run as fused loops over about this many bodies each (loop_bodies // B samples per loop, at least
        # one; 0 = all S x B bodies in one loop).  256 bodies = the three 50 MB activation matrices of the chained hidden convs stay inside the 256 MB Infinity
        # Cache and every layer is whole rounds of tiles: chain kernel 0.188 of peak against 0.174 for one 1280-body loop (config 4: 4.74 -> 5.06 k bodies/s,
        # config 3: 2.40 -> 2.50 k; profiles/r06r_loop_bodies_ab.txt).  Results do not depend on the grouping (bodies are independent).
        self.loop_bodies = 256
        self.per_step_launches = False     # True: the separate per-step launches of rounds 2-3 instead of step_fused_kernel (same bits; A/B runs and tests)
        self.prune_passes = True           # exact: items whose 24 joints are all visible skip the image-masked pass (egohmr.py:239-254)
        # classifier-free guidance on the visibility fuse (egohmr.py:248-249, `diffuse_output_uncond + guidance_param * (diffuse_output -
        # diffuse_output_uncond)`): x0 = u + s (c - u) per joint, s = guidance_param_visible on visible joints, guidance_param (the reference's local
        # of :248, a literal 0 there) on invisible ones.  (1, 0) is the reference's fuse; see fuse_scales
        self.guidance_param = 0.0
        self.guidance_param_visible = 1.0
        self.outer_guidance = 1.0          # the scale of a ClassifierFreeSampleModel around this model while it samples (diffusion.py); 1 = none
        self.force_cfg_kernels = False     # True: scales (1, 0) run the guidance kernels too instead of the select (same bits; tests)
        # arithmetic of the hidden GCN convs: 'f32' (f32-input MFMA), 'f16x3' (split-f16 MFMA, f32-grade), 'f16' (plain f16, not parity-grade)
        self.gcn_precision = "f16x3"
        # arithmetic of the two conditioning encoders: 'f16x3' (split-f16, f32 grade - the parity path) | 'f16' (plain f16 operands and activations: the
        # encoders of BASELINE config 5's fp16 TIER, together with gcn_precision = 'f16'; NOT parity grade: 0.4 - 1.4 mm of final vertex, docs/EXPERIMENTS.md 3.3)
        self.encoder_precision = "f16x3"
        # precision schedule (docs/EXPERIMENTS.md 3.6): only the LAST k executed steps of a fused sampling loop run in gcn_precision ('f16x3'), the
        # earlier ones on plain f16 operands / f16 activations.  'auto' = the k that FusedSampler.calibrate_schedule MEASURED for the
        # loaded weights and the sampler in use (smallest k whose bodies stay within schedule_tol of the all-f16x3 loop; measured on the
        # first call per (weights, sampler) when auto_calibrate is on, else every step stays f16x3); an int = that k, on the caller's
        # responsibility; None = off.  There is no constant default: whether early rounding errors are contracted away depends on
        # d x0 / d x_t of the checkpoint.
        self.f16x3_last_steps = "auto"
        # middle tier of the schedule: of those k steps the FIRST j run two-term products, a_hi * (w_hi + w_lo) - 2 MFMAs per product
        # instead of 3, same X2 buffers.  'auto' = the j that calibrate_schedule measured behind k (same criterion, same ladder; only when
        # f16x3_last_steps is 'auto' too: an explicit k or None leaves j = 0); an int = that j (capped at k), on the caller's responsibility; 0 = off.
        self.f16x2_steps = "auto"
        self.schedule_tol = 1e-5           # metres, max vertex / joint distance to the all-f16x3 loop (the north-star bar is 1e-4)
        self.auto_calibrate = True
        # hipGraph replay of the whole T-step loop (one graph launch instead of ~5 T kernel launches), unguided loops only.  Off by
        # default: measured on MI355X (tools/latency_small.py, profiles/r02_latency_b8_ddim5.json) the loop is GPU-bound even at B = 8
        # (3.74 ms eager vs 3.73 ms replayed for DDIM-5: the eight chained convs of a step are a dependency chain of tile times),
        # so the graph only saves host CPU time.  True = use it; 'auto' = for passes * B <= 64.
        self.use_hip_graph = False
        self.fused_sampler = FusedSampler(self)
        self.to(dev)
        self.eval()

    # ------------------------------------------------------------------ reference API
    def validation_setup(self):
        self.training = False
        self.eval()

    def _std_mean(self):
        return self.body_rep_mean_buf, self.body_rep_std_buf

    def visibility(self, batch):
        vis = batch["orig_keypoints_2d"][:, :, -1] > 0                                 # :186
        vis = vis.clone()
        vis[:, 8] = True                                                               # :187
        return vis[:, self.openpose_to_smpl]                                           # :188

    # False: training_step / GaussianDiffusion.training_losses raise NotImplementedError and forward never carries a graph.  True: they run the reference's
    # training loop (egohmr.py:453-472, gaussian_diffusion.py:721-746) with the image trunk FROZEN - a forward under self.training takes the training route
    # (_forward_train): the folded ResNet-50 in eval mode under no_grad, everything else of init_optimizers' list (scene PointNet, transl_enc, beta_layer,
    # the denoiser, embed_timestep, input_process) with a graph.  Calls with self.training False do not depend on it
    frozen_trunk_training = False
    # Consulted on the training route only (behind frozen_trunk_training, whose name stays): True unfreezes the trunk's WEIGHTS - img_feats comes from the
    # backbone's autograd route (ResNet50Features.grad_params; BatchNorm in eval mode with frozen statistics, or - backbone.train_batchnorm = True - in
    # .train() on batch statistics as the reference's backbone.train(), egohmr.py:455) and init_optimizers puts backbone.parameters() in front, which
    # is the reference's list (egohmr.py:140-147)
    trunk_grad = False
    # Consulted on the training route only (behind frozen_trunk_training).  True, with torch.distributed initialised and more than one rank: the ranks
    # each take their shard of a batch and together make the optimizer step ONE process would make on the whole batch, to rounding - init_optimizers
    # broadcasts rank 0's parameters and buffers; training_step exchanges the item counts B_r, runs every train-mode BatchNorm on all ranks' rows
    # (dist.StatSync), backpropagates loss B_r / B and sums the gradients of init_optimizers' list over the ranks in one flat all-reduce before
    # optimizer.step().  NOT coordinated across the ranks, as with torch's DistributedDataParallel: the cond_mask_prob draw, the caller's timesteps and
    # the caller's noise - seed them per rank.  Without a process group, or with one rank, it changes nothing, bit for bit
    data_parallel = False

    def _data_parallel_world(self):
        """the number of ranks the training route is spread over: 1 unless data_parallel is set and a process group with more ranks exists"""
        import torch.distributed as td
        if not (self.data_parallel and td.is_available() and td.is_initialized()):
            return 1
        return td.get_world_size()

    def fuse_scales(self, eval_with_uncond=True, force_mask=False, outer=1.0):
        """(s_vis, s_inv): the guidance scales of visible / invisible joints in x0 = u + s (c - u), c the conditional output and u the masked one
        (mask_cond(force_mask=True): image only or the whole condition, as only_mask_img_cond says).  force_mask: (0, 0), the masked output alone;
        a diffuse_fuse model evaluated with its masked pass: outer * (guidance_param_visible, guidance_param); else outer * guidance_param_visible on
        every joint.  `outer` is the scale of a wrapper (diffusion.ClassifierFreeSampleModel).  Python floats, handed to the device as float32: a scale
        that is not finite there raises ValueError."""
        gv, gi, w = float(self.guidance_param_visible), float(self.guidance_param), float(outer)
        if force_mask:
            s = (0.0, 0.0)
        elif self.diffuse_fuse and eval_with_uncond:
            s = (w * gv, w * gi)
        else:
            s = (w * gv, w * gv)
        with np.errstate(over="ignore"):
            if not all(math.isfinite(v) and math.isfinite(float(np.float32(v))) for v in s):
                raise ValueError(f"guidance scales must be finite in float32: guidance_param_visible={gv}, guidance_param={gi}, outer scale={w}")
        return s

    @staticmethod
    def fuse_passes(scales) -> int:
        """Denoiser passes of a call with these scales: 1 exactly when both are 1.0 (x0 = c, no masked pass), else 2."""
        return 1 if (scales[0] == 1.0 and scales[1] == 1.0) else 2

    def sampling_scales(self, eval_with_uncond=True, force_mask=False):
        """fuse_scales with the outer scale a wrapper has set for the call in progress (outer_guidance)."""
        return self.fuse_scales(eval_with_uncond, force_mask, outer=self.outer_guidance)

    def forward(self, batch, timesteps, eval_with_uncond=True, force_mask=False):
        """One denoising evaluation (egohmr.py:173-303).  Conditioning is cached per batch object.  force_mask: the masked output alone
        (mask_cond(force_mask=True), scales (0, 0)).  Under self.training with frozen_trunk_training set: the training route (_forward_train), one pass
        whatever eval_with_uncond / force_mask say."""
        with _lib.on_device(self.device):                 # native calls launch on the CURRENT device's stream
            if self.training and self.frozen_trunk_training:
                return self._forward_train(batch, timesteps)
            return self._forward_on_device(batch, timesteps, eval_with_uncond, force_mask)

    def _check_trainable(self):
        """What the training route cannot run, refused before any device call."""
        dm = self.diffusion_model
        if dm.nonlocal_layer and not dm.nonlocal_grad:
            raise NotImplementedError("EgoHMR.frozen_trunk_training: the non-local block has no backward; the training route needs gcn_nonlocal_layer=False"
                                      " (or diffusion_model.nonlocal_grad = True, which turns the block's backward on)")
        if self.gcn_precision == "f16" or dm.precision == "f16":
            raise _lib.EgoHMRHipError(dm.GRAD_F16)

    def cond_drop_mask(self, B):
        """mask_cond's per-item draw (egohmr.py:159-160): None when cond_mask_prob is 0, else [B] uint8 (1 = the item's conditioning is dropped) from the
        reference's own call on torch's global generator."""
        if not self.cond_mask_prob > 0.0:
            return None
        return torch.bernoulli(torch.ones(B, device=self.device) * self.cond_mask_prob).to(torch.uint8)

    def _set_train_modes(self):
        """egohmr.py:454-462: the backbone goes into .train() (:455, batch statistics) exactly when EgoHMR.trunk_grad and
        ResNet50Features.train_batchnorm are both set, else it stays in eval mode; the denoiser trains its BatchNorm only behind
        ModulatedGCN.train_batchnorm - without it the denoiser stays in eval mode and its statistics frozen (a deviation from the reference, which always
        trains on batch statistics)."""
        self.training = True
        self.backbone.train(bool(self.trunk_grad and self.backbone.train_batchnorm))
        for m in (self.scene_enc, self.transl_enc, self.beta_layer, self.input_process, self.embed_timestep):
            m.train()
        self.diffusion_model.train(bool(self.diffusion_model.train_batchnorm))

    def _forward_train(self, batch, timesteps):
        """egohmr.py:173-303 under self.training, as an autograd graph, with the image trunk frozen (eval_with_uncond=False: one pass, also with
        diffuse_fuse - training_step passes that, :465).

        Constants, from the no-grad code of FusedSampler.prepare (run once per step, without its PointNet / projection part): img_feats (folded trunk, eval
        mode), the joint visibility, the camera columns, the scene (after scene_cano), transl, fx, cam_cx, cam_cy.  With a graph: scene_enc (its HIP VJP,
        grad_params set for the call), transl_enc, embed_timestep (one timestep per item, :178), input_process and beta_layer (plain torch modules), the
        conditioning assembly with the cond_mask_prob draw (train_grad.CondAssemble: one launch each way), the denoiser (ModulatedGCN.forward with
        grad_params set, in EgoHMR.gcn_precision: batch statistics behind ModulatedGCN.train_batchnorm, else eval-mode BatchNorm with frozen statistics -
        the reference always trains on batch statistics) and decode_output.  Sets batch['vis_mask_smpl'], smpl_output, scene_pcd_verts, input_transl,
        focal_length and camera_center_full like forward; like decode_output it does NOT apply the NaN rule of ehm_pack_outputs.
        With EgoHMR.trunk_grad, img_feats is not a constant: prepare leaves the trunk out and the backbone runs here behind its autograd route
        (ResNet50Features.grad_params set for the call; eval-mode BatchNorm with frozen statistics, or - ResNet50Features.train_batchnorm - the
        backbone in .train() on batch statistics, :455).
        SMPL.ordered_backward is set for the decode: the route has no order-dependent sum, so two steps on the same inputs give the same gradient bits."""
        self._check_trainable()
        dm, dev = self.diffusion_model, self.device
        x_t = _lib.f32(batch["x_t"], dev).reshape(-1, 144)
        B = x_t.shape[0]
        ts = torch.as_tensor(timesteps, device=dev).reshape(-1).long()
        if ts.numel() not in (1, B):
            raise ValueError(f"timesteps must hold one value per item: got {ts.numel()} for a batch of {B}")
        st = self.fused_sampler.prepare(batch, _constants_only=True, _no_trunk=bool(self.trunk_grad))
        n_scene, n_other = self.scene_enc.fc_c.out_features, self.context_feats_dim - IMG_DIM
        enc, bb = self.scene_enc, self.backbone
        keep = (enc.grad_params, dm.grad_params, dm.precision)
        keep_bb = bb.grad_params
        try:
            enc.grad_params = dm.grad_params = True
            dm.precision = self.gcn_precision
            dm.train(bool(dm.train_batchnorm))
            img_feats = st.img_feats
            if self.trunk_grad:                                                 # :183 with a graph (batch statistics behind backbone.train_batchnorm)
                bb.grad_params = True
                bb.train(bool(bb.train_batchnorm))
                img_feats = bb(_lib.f32(batch["img"], dev))
            scene_feats = enc(st.scene)                                                                    # :214
            transl_feat = self.transl_enc(st.transl)                                                       # :217
            cam = st.other[:, n_scene + transl_feat.shape[1]:n_other]                                      # :195-205 (ehm_item_prep wrote them)
            other = torch.cat([scene_feats, transl_feat, cam], dim=1)                                      # :220-221
            temb = self.embed_timestep(ts.expand(B)).squeeze(0)                                            # :178
            x_feat = self.input_process.poseEmbedding(x_t.reshape(B * 24, 6))                              # :234
            X = train_grad.CondAssemble.apply(img_feats, st.vis, self.cond_drop_mask(B), other, x_feat, temb, self.only_mask_img_cond)   # :190-191, :222-236
            x0 = dm(X).reshape(B, 144)                                                                     # :237, :256
        finally:
            enc.grad_params, dm.grad_params, dm.precision = keep
            bb.grad_params = keep_bb
        betas = self.beta_layer(torch.cat([img_feats, other], dim=1))                                   # :263-265
        batch["vis_mask_smpl"] = st.vis_bool                                                               # :189
        keep_ordered = self.smpl.ordered_backward
        try:
            self.smpl.ordered_backward = True                                                              # a step's gradients repeat their bits
            return self.decode_output(batch, x0, betas, _st=st)
        finally:
            self.smpl.ordered_backward = keep_ordered

    def _forward_on_device(self, batch, timesteps, eval_with_uncond, force_mask=False):
        fs = self.fused_sampler
        scales = self.sampling_scales(eval_with_uncond, force_mask)          # (raises on a non-finite scale before any device call)
        passes = self.fuse_passes(scales)
        st = fs.prepare(batch, scales=scales)
        x_t = _lib.f32(batch["x_t"], self.device).reshape(-1, 144)
        B = x_t.shape[0]
        # egohmr.py:178 embeds `timesteps` [bs] row by row.  The samplers always pass one value for the whole batch (gaussian_diffusion.py:495):
        # that is the one-launch route; a direct call with different values per item runs one denoiser evaluation per distinct value.
        ts = torch.as_tensor(timesteps, device=self.device).reshape(-1).long()
        if ts.numel() not in (1, B):
            raise ValueError(f"timesteps must hold one value per item: got {ts.numel()} for a batch of {B}")
        uniq = torch.unique(ts) if ts.numel() > 1 else ts[:1]
        if uniq.numel() == 1:
            x0 = fs.denoise_once(st, x_t, fs.timestep_vectors(uniq)[0], passes, scales)
        else:
            x0 = torch.empty(B, 144, device=self.device)
            tv = fs.timestep_vectors(uniq)
            for i, t in enumerate(uniq.tolist()):
                sel = torch.nonzero(ts == t).reshape(-1)
                x0[sel] = fs.denoise_once(st.take(sel), x_t[sel].contiguous(), tv[i], passes, scales)
        mean, std = self._std_mean()
        verts = torch.empty(B, self.smpl.num_verts, 3, device=self.device)
        joints = torch.empty(B, self.smpl.num_joints_out, 3, device=self.device)
        R = torch.empty(B, 24, 3, 3, device=self.device)
        pose6d = torch.empty(B, 144, device=self.device)
        _lib.api().ehm_smpl_forward_rot6d(self.smpl.handle(), st.betas, x0, mean, std, verts, joints, R, pose6d, None, B, _lib.stream_ptr())
        batch["vis_mask_smpl"] = st.vis_bool
        return self._pack_output(batch, st, x0, pose6d, R, verts, joints, chk=x_t.contiguous(), chk_rows=1)

    def _pack_output(self, batch, st, x0, pose6d, R, verts, joints, chk=None, chk_rows=0, last_noise=None, x_final=None):
        """The output dict of EgoHMR.forward (egohmr.py:283-303) in one launch (ehm_pack_outputs): items with a NaN / Inf in their inputs
        (st.finite) or in a row of `chk` come out as NaN, like the reference's float32 graph gives them."""
        B, J, dev = x0.shape[0], joints.shape[1], x0.device
        buf = torch.empty(B * (10 + 216 + 5 * J + 4), device=dev)
        cuts, off = [], 0
        for n in (10, 9, 207, 3 * J, 2 * J, 2, 2):
            cuts.append(buf[off:off + B * n].view(B, n))
            off += B * n
        betas, go, bp, kp3d, kp2d, focal, center = cuts
        P = _lib.ptr
        d = _lib.PackDesc(B=B, J=J, V=verts.shape[1], finite=P(st.finite), chk=P(chk), chk_rows=int(chk_rows), last_noise=P(last_noise), x_final=P(x_final),
                          x0=P(x0), pose6d=P(pose6d), R=P(R), verts=P(verts), joints=P(joints), betas_in=P(st.betas), betas_out=P(betas),
                          transl=P(st.transl), fx=P(st.fx), cx=P(st.cam_cx), cy=P(st.cam_cy), fx_norm=self.cfg.CAM.FX_NORM_COEFF, global_orient=P(go),
                          body_pose=P(bp), kp3d_full=P(kp3d), kp2d_full=P(kp2d), focal=P(focal), center=P(center), finite_out=None)
        with _lib.on_device(dev):
            _lib.api().ehm_pack_outputs(C.byref(d), _lib.stream_ptr())
        self.scene_pcd_verts = st.scene
        self.input_transl = st.transl
        self.smpl_output = smpl_mod.SMPLOutput(vertices=verts, joints=joints, full_pose=R)
        self.focal_length, self.camera_center_full = focal, center                     # :283-285
        return {
            "pred_x_start": x0,
            "pred_smpl_params": {"global_orient": go.view(B, 1, 3, 3), "body_pose": bp.view(B, 23, 3, 3), "betas": betas},
            "pred_pose_6d": pose6d,
            "pred_keypoints_3d": joints,
            "pred_vertices": verts,
            "pred_keypoints_3d_full": kp3d.view(B, J, 3),
            "pred_keypoints_2d_full": kp2d.view(B, J, 2),                              # :295-301
        }

    COLLISION_PROXIES = ("vertex", "mesh")

    @property
    def collision_proxy(self):
        return self._collision_proxy

    @collision_proxy.setter
    def collision_proxy(self, value):
        if value not in self.COLLISION_PROXIES:                      # (at the assignment: before any device call)
            raise ValueError(f"collision_proxy must be one of {self.COLLISION_PROXIES} (got {value!r})")
        self._collision_proxy = value

    def mesh_collision(self) -> bool:
        """Whether the collision term is the mesh one: collision_proxy = 'mesh' and no `collision_model` attached (that takes precedence)."""
        return self.collision_model is None and self.collision_proxy == "mesh"

    def guide_coll(self, batch, output, t, compute_grad="x_t"):
        """egohmr.py:517-570 with the build's collision proxy (vertex or mesh, `collision_proxy`) in place of COAP; returns [B,144].  With `collision_model` attached: the reference's
        own autograd route through that model (_guide_coll_model), for compute_grad 'x_t' and 'x_0' alike."""
        fs = self.fused_sampler
        st = fs.prepare(batch)
        x = _lib.f32(batch["x_t"] if compute_grad == "x_t" else output["pred_x_start"], self.device).reshape(-1, 144)
        betas = _lib.f32(output["pred_smpl_params"]["betas"], self.device)
        if self.collision_model is not None:
            if compute_grad not in ("x_t", "x_0"):                       # (the reference leaves x_t unbound for anything else, egohmr.py:519-523)
                raise ValueError(f"compute_grad must be 'x_t' or 'x_0' (got {compute_grad!r})")
            with _lib.on_device(self.device):
                return self._guide_coll_model(st.scene, x, betas)
        return fs.guidance_gradient(st, x, betas)

    # ------------------------------------------------------------------ an attached collision model (COAP / VolumetricSMPL)
    GUIDE_ZEROED_JOINTS = (0, 3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23)      # egohmr.py:567 "ignore upper body part"

    def _collision_bodies(self, betas, global_orient, body_pose):
        """The `smpl_output_mode` of egohmr.py:537-540 / :492-495: vertices, joints and the axis-angle full_pose [B,72], all in the autograd graph of the
        inputs when gradients are enabled."""
        so = self.smpl(betas=betas, body_pose=body_pose, global_orient=global_orient, return_full_pose=True, pose2rot=False)
        B = so.vertices.shape[0]
        aa = geometry.rotation_matrix_to_angle_axis(so.full_pose.reshape(-1, 3, 3)).reshape(B, -1)
        return smpl_mod.SMPLOutput(vertices=so.vertices, joints=so.joints, full_pose=aa)

    @staticmethod
    def _collision_item(bodies, i, clone=False):
        f = (lambda t: t[[i]].clone()) if clone else (lambda t: t[[i]])
        return smpl_mod.SMPLOutput(vertices=f(bodies.vertices), joints=f(bodies.joints), full_pose=f(bodies.full_pose))

    @staticmethod
    def _bbox_points(item, scene_i, cap=None):
        """egohmr.py:550-552: the scene points [1,n,3] inside the bounding box of the item's vertices, or None when there is none (one host read-back
        per item, like the reference); cap: `inds[:, cap:] = False` where more than `cap` are selected (:411-412)."""
        v = item.vertices.detach()
        bb_min, bb_max = v.min(1).values.reshape(1, 3), v.max(1).values.reshape(1, 3)
        inds = (scene_i >= bb_min).all(-1) & (scene_i <= bb_max).all(-1)
        if cap is not None and inds.sum() > cap:
            inds[:, cap:] = False
        if not inds.any():
            return None
        return scene_i[inds].unsqueeze(0)

    def _collision_losses(self, bodies, scene):
        """[B] losses of the attached model: per item over the bbox-selected points (egohmr.py:545-559); with guide_all_points ONE batched call over every
        scene point (egohmr_volsmpl.py:609-614)."""
        cm = self.collision_model
        B = bodies.vertices.shape[0]
        if self.guide_all_points:
            return cm.collision_loss(scene, bodies, ret_collision_mask=None).reshape(B)
        losses = []
        for i in range(B):
            item = self._collision_item(bodies, i)
            pts = self._bbox_points(item, scene[[i]])
            losses.append(torch.zeros((), device=self.device) if pts is None else cm.collision_loss(pts, item, ret_collision_mask=None).reshape(()))
        return torch.stack(losses)

    def _guide_coll_model(self, scene, x, betas):
        """egohmr.py:517-570 (egohmr_volsmpl.py:582-629 with guide_all_points / guide_reduction = 'sum') through `collision_model`: de-normalise,
        rot6d_to_rotmat, the differentiable SMPL.forward (ehm_smpl_backward behind it), rotation_matrix_to_angle_axis, the model's loss, then
        torch.autograd.grad of -loss.mean() (denominator: FusedSampler.guide_denom, so guide_denom_override acts as on the proxy route) or -loss.sum()
        w.r.t. the DE-NORMALISED pose, joints 3.. doubled, the upper body zeroed; an all-zero loss gives zeros."""
        B = x.shape[0]
        mean, std = self._std_mean()
        with torch.enable_grad():
            x_t = x.detach().requires_grad_() * std + mean                                               # :523, :528
            R = geometry.rot6d_to_rotmat(x_t.reshape(-1, 6), rot6d_mode="diffusion").view(B, 24, 3, 3)   # :529
            bodies = self._collision_bodies(betas.detach(), R[:, [0]], R[:, 1:])                         # :532-540
            loss = self._collision_losses(bodies, _lib.f32(scene, self.device))
            if not bool((loss != 0).any()):                                                              # :561, :569-570
                return torch.zeros(B, 144, device=self.device)
            g = torch.autograd.grad([-(loss.sum() / self.fused_sampler.guide_denom(B))], [x_t])[0]       # :562
        g = g.reshape(-1, 24, 6).clone()
        g[:, 3:] = g[:, 3:] * 2                                                                          # :564-565
        g[:, list(self.GUIDE_ZEROED_JOINTS)] = 0                                                         # :567
        return g.reshape(-1, 144)

    def _hit_share_model(self, output, query, inside):
        """egohmr.py:487-514: per item, the share of ALL its scene points that are bbox-selected and `inside(query(points, item))`."""
        p = output["pred_smpl_params"]
        with _lib.on_device(self.device), torch.no_grad():
            bodies = self._collision_bodies(_lib.f32(p["betas"], self.device), _lib.f32(p["global_orient"], self.device), _lib.f32(p["body_pose"], self.device))
            scene = _lib.f32(self.scene_pcd_verts, self.device)
            out = []
            for i in range(bodies.vertices.shape[0]):
                item = self._collision_item(bodies, i, clone=True)
                pts = self._bbox_points(item, scene[[i]])
                out.append(0.0 if pts is None else (inside(query(pts, item)).sum() / scene.shape[1]).item())
        return out

    def eval_coll(self, output):
        """egohmr.py:487-514 with the build's proxy in place of `coap.query(...) > 0.5`: per item, the share of the scene points that
        lie inside the body's bounding box AND closer than tau to its surface.  One kernel sequence for the batch, one host sync
        (`.tolist()`, the reference syncs per item); returns the reference's python list [B] of floats.  With collision_proxy = 'mesh': the share
        of the scene points inside the bounding box AND inside the posed mesh (winding number > 0.5) - the quantity the reference's metric estimates,
        computed on the mesh itself.  NOT a COAP number - unless
        `collision_model` is attached: then `collision_model.query(points, smpl_output) > 0.5` per item, as the reference runs it."""
        if self.collision_model is not None:
            return self._hit_share_model(output, self.collision_model.query, lambda occ: occ > 0.5)
        p = output["pred_smpl_params"]
        so = self.smpl(betas=p["betas"], body_pose=p["body_pose"], global_orient=p["global_orient"], pose2rot=False)
        # bbox-selected points in BOTH reference files (egohmr.py:499-505, egohmr_volsmpl.py:531-537), whatever the guidance uses
        _, _, hits = self.fused_sampler.collision(so.vertices, self.scene_pcd_verts, want_grad=False, want_hits=True, all_points=False)
        return (hits.float() / self.scene_pcd_verts.shape[1]).tolist()

    # ------------------------------------------------------------------ validation losses (egohmr.py:307-449, evaluation branch)
    def _gt_body_model(self, gender):
        m = self._gt_smpl.get(gender)
        if m is None:
            src = self._gt_smpl_src
            m = self._gt_smpl[gender] = smpl_mod.create(src["model_path"], model_type="smpl", gender=gender, asset=src[gender],
                                                        allow_synthetic=src["allow_synthetic"])
        if m.v_template.device != self.device:
            m.to(self.device)
        return m

    @property
    def smpl_male(self):
        return self._gt_body_model("male")

    @property
    def smpl_female(self):
        return self._gt_body_model("female")

    PENETRATION_POINT_CAP = 4000               # egohmr.py:411-412

    def _penetration_term(self):
        """egohmr.py:399-419 per item, with the build's collision proxy in place of `coap.collision_loss` (NOT a COAP number): the proxy over the scene
        points inside the bounding box of the item's predicted vertices; where more than 4000 points are selected the points of INDEX >= 4000 are dropped
        (`inds[:, 4000:] = False`); no selected point -> 0.  [B], no host read-back.  With `collision_model` attached the reference's loop runs as it
        stands (_penetration_term_model: its `collision_loss`, one host read-back per item)."""
        if self.collision_model is not None:
            return self._penetration_term_model()
        return self._penetration_term_proxy(self.smpl_output.vertices)[0]

    def _penetration_term_proxy(self, verts, want_grad=False):
        """The proxy's term [B] on `verts` and, with want_grad, its derivative [B,V,3] (else None): what loss_grad.ProxyPenetration runs behind."""
        verts, scene = _lib.f32(verts, self.device), _lib.f32(self.scene_pcd_verts, self.device)
        B, V, N = verts.shape[0], verts.shape[1], scene.shape[1]
        if N > self.PENETRATION_POINT_CAP:
            capped = torch.empty_like(scene)
            count = torch.empty(B, device=self.device, dtype=torch.int32)
            _lib.api().ehm_scene_cap_points(verts, scene, capped, count, B, V, N, self.PENETRATION_POINT_CAP, _lib.stream_ptr())
            scene = capped
        return self.fused_sampler.collision(verts, scene, want_grad=want_grad, all_points=False)[:2]

    def _penetration_term_model(self):
        """egohmr.py:393-418 through `collision_model.collision_loss`: the bodies of the last forward, bbox-selected points capped at index 4000 -> [B].
        With gradients enabled (compute_loss's autograd route) the bodies and the model's losses stay in the graph."""
        f32 = loss_grad.f32_graph if torch.is_grad_enabled() else _lib.f32
        so, scene = self.smpl_output, _lib.f32(self.scene_pcd_verts, self.device)
        B = so.vertices.shape[0]
        aa = geometry.rotation_matrix_to_angle_axis(f32(so.full_pose, self.device).reshape(-1, 3, 3)).reshape(B, -1)               # :397
        bodies = smpl_mod.SMPLOutput(vertices=f32(so.vertices, self.device), joints=f32(so.joints, self.device), full_pose=aa)
        out = torch.zeros(B, device=self.device)
        for i in range(B):
            item = self._collision_item(bodies, i, clone=True)
            pts = self._bbox_points(item, scene[[i]], cap=self.PENETRATION_POINT_CAP)
            if pts is not None:
                out[i] = f32(self.collision_model.collision_loss(pts, item, ret_collision_mask=None), self.device).reshape(())
        return out

    def compute_loss(self, batch, output, cur_epoch=0):
        """egohmr.py:307-449 in the evaluation branch, on the device (csrc/loss.hip: ehm_val_losses), for the output of `model(batch, t)` or of a sampling
        loop (`diffusion.val_losses`).  Fills output['losses'] with the reference's eleven keys in its order (0-d float32 device tensors),
        output['joint_vis_num_batch'] (0-d int64) and, beyond the reference, output['losses_per_item'] ({key: [B]} plus 'joint_vis_num' [B] int64 and
        'joint_vis_mask' [B,24] bool: what a sharded run needs for global means); returns `loss`.  No host synchronisation.

        A batch WITHOUT 'keypoints_3d' is a sampling-only batch: output['losses'] = {} and a zero scalar, nothing is computed.  A batch that has
        'keypoints_3d' but lacks 'keypoints_3d_full', 'gender', 'smpl_params_is_axis_angle' or a key of 'smpl_params' raises KeyError naming it.
        Ground-truth poses are axis-angle (the EgoBody loader's; `smpl_params_is_axis_angle`, read on the host, must be all-true for 'global_orient' and
        'body_pose', else NotImplementedError).  The penetration term uses the build's collision proxy, not COAP - unless `collision_model` is attached: then its
        `collision_loss` per item, as the reference runs it (_penetration_term).

        The autograd route: with gradients enabled and a prediction of `output` that requires grad (pred_vertices, pred_keypoints_3d, pred_keypoints_3d_full,
        pred_keypoints_2d_full, pred_pose_6d, an entry of pred_smpl_params or, with the penetration term active, self.smpl_output.vertices) the returned
        `loss` carries a grad_fn (loss_grad.ValLossesFunction: ehm_val_losses_backward is its VJP; first derivatives only) and has the same bits (the
        proxy's penetration term is a float-atomic sum on either route: it repeats to the last bits only);
        everything stored in `output` is detached, as the reference detaches it (:432-443).  `decode_output` builds such an output from a pred_x_start.
        self.training is not consulted.  Every other call runs without a graph, as before."""
        if "keypoints_3d" not in batch:
            output["losses"] = {}
            return torch.zeros((), device=self.device)
        for k in ("keypoints_3d_full", "gender", "smpl_params_is_axis_angle", "smpl_params", "orig_keypoints_2d"):
            if k not in batch:
                raise KeyError(k)
        sp, flags = batch["smpl_params"], batch["smpl_params_is_axis_angle"]
        for k in ("global_orient", "body_pose", "betas", "transl"):
            if k not in sp:
                raise KeyError(f"smpl_params[{k!r}]")
        for k in ("global_orient", "body_pose"):
            if k not in flags:
                raise KeyError(f"smpl_params_is_axis_angle[{k!r}]")
            f = flags[k]
            if isinstance(f, torch.Tensor) and f.is_cuda:
                raise ValueError(f"smpl_params_is_axis_angle[{k!r}] is on the device; the loader's flags stay on the host (train_egohmr.py:182)")
            if not bool(np.asarray(f).all()):
                raise NotImplementedError(f"smpl_params_is_axis_angle[{k!r}] is not all-true: compute_loss takes axis-angle ground-truth poses "
                                          "(the EgoBody loader's; egohmr.py:380-381 decodes a mixed batch inconsistently)")
        with_pen = self.weight_coap_penetration > 0 and cur_epoch >= self.start_coap_epoch                                        # :392
        with _lib.on_device(self.device):
            if self._loss_wants_grad(output, with_pen):
                loss, res = self._val_losses_graph(batch, output, with_pen)
            else:
                with torch.no_grad():
                    res = val_losses_native(self.loss_inputs(batch, output), self.loss_weights(), self._penetration_term() if with_pen else None)
                loss = None
        K = _lib.LOSS_KEYS
        output["losses"] = {k: res["losses"][i] for i, k in enumerate(K)}                                                         # :432-443
        output["joint_vis_num_batch"] = res["joint_vis_num"][0]                                                                 # :447
        output["losses_per_item"] = {**{k: res["per_item"][:, i] for i, k in enumerate(K)}, "joint_vis_num": res["per_item_vis"],
                                     "joint_vis_mask": res["vis_mask"].bool()}
        return output["losses"]["loss"] if loss is None else loss

    def _loss_wants_grad(self, output, with_pen) -> bool:
        """compute_loss's route: True = gradients are enabled and one of the predictions the total depends on requires grad."""
        if not torch.is_grad_enabled():
            return False
        ts = [output.get(k) for k in ("pred_vertices", "pred_keypoints_3d", "pred_keypoints_3d_full", "pred_keypoints_2d_full", "pred_pose_6d")]
        ts += list(output.get("pred_smpl_params", {}).values())
        if with_pen:
            ts.append(getattr(getattr(self, "smpl_output", None), "vertices", None))
        return any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)

    def _val_losses_graph(self, batch, output, with_pen):
        """The autograd route of compute_loss -> (total with a grad_fn, the detached results as val_losses_native names them)."""
        pen = None
        if with_pen:                                                                                                                    # :390-419
            if self.collision_model is not None:
                pen = loss_grad.f32_graph(self._penetration_term_model(), self.device)
            else:
                pen = loss_grad.ProxyPenetration.apply(self, loss_grad.f32_graph(self.smpl_output.vertices, self.device))
        t = self.loss_inputs(batch, output, graph=True)
        preds = [t.pop(k) for k in loss_grad.PREDICTIONS]
        loss, *rest = loss_grad.ValLossesFunction.apply(t, self.loss_weights(), pen, *preds)
        return loss, dict(zip(("losses", "joint_vis_num", "per_item", "per_item_vis", "vis_mask"), rest))

    def loss_inputs(self, batch, output, graph=False) -> dict:
        """The device arrays ehm_val_losses reads for an annotated batch and a model output, named like the descriptor's fields: the prediction as the
        output dict holds it, the male AND female ground-truth bodies (egohmr.py:344-349: axis-angle input, `transl` applied), the ground-truth rotations
        through aa_to_rotmat (:380-381), focal length and camera centre of the last forward (:283-285).  graph: the eight prediction arrays are converted
        without detaching (compute_loss's autograd route); the ground truth never carries a graph."""
        dev, g32 = self.device, _lib.f32
        f32 = loss_grad.f32_graph if graph else g32
        pp, sp = output["pred_smpl_params"], batch["smpl_params"]
        pv = f32(output["pred_vertices"], dev)
        B = pv.shape[0]
        with torch.no_grad():
            gt = {k: g32(v, dev) for k, v in sp.items()}                                   # :344, :347 (`v.float()`)
            male, female = self.smpl_male(**gt), self.smpl_female(**gt)
            rot = {k: geometry.aa_to_rotmat(gt[k].reshape(-1, 3)).reshape(B, -1).contiguous() for k in ("global_orient", "body_pose")}

        def aligned(t):                        # the vertex kernel loads 16 bytes at a time (a slice of a stacked [S,B,V,3] result may start anywhere)
            return t if t.data_ptr() % 16 == 0 else t.clone()
        t = dict(pred_vertices=aligned(pv), pred_keypoints_3d=f32(output["pred_keypoints_3d"], dev), pred_keypoints_3d_full=f32(output["pred_keypoints_3d_full"], dev),
                 pred_keypoints_2d_full=f32(output["pred_keypoints_2d_full"], dev), pred_global_orient=f32(pp["global_orient"], dev),
                 pred_body_pose=f32(pp["body_pose"], dev), pred_betas=f32(pp["betas"], dev), pred_pose_6d=f32(output["pred_pose_6d"], dev),
                 keypoints_2d=g32(batch["orig_keypoints_2d"], dev), keypoints_3d=g32(batch["keypoints_3d"], dev),
                 keypoints_3d_full=g32(batch["keypoints_3d_full"], dev), gt_vertices_male=aligned(male.vertices.contiguous()),
                 gt_vertices_female=aligned(female.vertices.contiguous()), gt_joints_male=male.joints.contiguous(), gt_joints_female=female.joints.contiguous(),
                 gender=torch.as_tensor(batch["gender"]).to(dev).long().reshape(-1).contiguous(), gt_global_orient=rot["global_orient"], gt_body_pose=rot["body_pose"],
                 gt_betas=gt["betas"], focal=g32(self.focal_length, dev), center=g32(self.camera_center_full, dev))
        if (t["gender"].numel() != B or t["pred_pose_6d"].numel() != B * 144 or t["gt_vertices_male"].shape != t["pred_vertices"].shape
                or any(t[k].shape[0] != B for k in t) or t["pred_keypoints_2d_full"].shape[1] != t["pred_keypoints_3d"].shape[1]
                or t["pred_keypoints_3d_full"].shape[1] != t["pred_keypoints_3d"].shape[1]):
            raise ValueError("compute_loss: batch and output do not describe the same B bodies")
        return t

    def loss_weights(self):
        """The nine weights of egohmr.py:422-430 in ehm_val_losses' order."""
        return [float(w) for w in (self.weight_loss_v2v, self.weight_loss_keypoints_3d, self.weight_loss_keypoints_3d_full, self.weight_loss_keypoints_2d_full,
                                   self.weight_loss_betas, self.weight_loss_body_pose, self.weight_loss_global_orient, self.weight_loss_pose_6d_ortho,
                                   self.weight_coap_penetration)]

    def decode_output(self, batch, pred_x_start, betas=None, _st=None):
        """egohmr.py:256-303 as an autograd graph: a pred_x_start [B,144] (and optionally betas [B,10]; default: the prepared batch's, a constant) -> the
        output dict of `forward` - the same keys as _pack_output - through torch ops and the differentiable geometry.rot6d_to_rotmat, SMPL.forward and
        geometry.perspective_projection, so that `compute_loss(batch, decode_output(batch, x0))` backpropagates into x0 (and betas).  Sets smpl_output,
        scene_pcd_verts, input_transl, focal_length and camera_center_full like `forward`.  It does NOT apply the NaN rule of ehm_pack_outputs (an item
        with a non-finite input is not blanked: values propagate as torch computes them)."""
        dev = self.device
        with _lib.on_device(dev):
            st = self.fused_sampler.prepare(batch) if _st is None else _st                                  # (_st: the training route's prepared constants)
            x0 = loss_grad.f32_graph(pred_x_start, dev).reshape(-1, 144)
            B = x0.shape[0]
            mean, std = self._std_mean()
            pose6d = x0 * std + mean                                                                        # :258
            R = geometry.rot6d_to_rotmat(pose6d.reshape(-1, 6), rot6d_mode="diffusion").view(B, 24, 3, 3)   # :260
            betas = st.betas if betas is None else loss_grad.f32_graph(betas, dev)
            params = {"global_orient": R[:, [0]], "body_pose": R[:, 1:], "betas": betas}                   # :268-270
            so = self.smpl(**params, return_full_pose=True, pose2rot=False)                                 # :276
            focal = (st.fx.reshape(B, 1) * self.cfg.CAM.FX_NORM_COEFF).repeat(1, 2)                          # :283-285
            center = torch.stack([st.cam_cx.reshape(B), st.cam_cy.reshape(B)], dim=-1)                     # :286
            kp2d = geometry.perspective_projection(so.joints, translation=st.transl, camera_center=center, focal_length=focal)   # :295-298
            kp2d = torch.stack([kp2d[:, :, 0] / 1920 - 0.5, kp2d[:, :, 1] / 1080 - 0.5], dim=-1)           # :299-300
        self.scene_pcd_verts, self.input_transl = st.scene, st.transl
        self.smpl_output = smpl_mod.SMPLOutput(vertices=so.vertices, joints=so.joints, full_pose=so.full_pose)
        self.focal_length, self.camera_center_full = focal, center
        return {
            "pred_x_start": x0,
            "pred_smpl_params": {k: v.clone() for k, v in params.items()},                                 # :273
            "pred_pose_6d": pose6d,
            "pred_keypoints_3d": so.joints,
            "pred_vertices": so.vertices,
            "pred_keypoints_3d_full": so.joints + st.transl.unsqueeze(1),                                  # :294
            "pred_keypoints_2d_full": kp2d,
        }

    NOT_BUILT = ("compute_loss has a backward (the loss, SMPL.forward, rot6d_to_rotmat, ModulatedGCN.forward, ResnetPointnet.forward and the ResNet-50 trunk "
                 "are differentiable, ModulatedGCN.train_batchnorm and ResNet50Features.train_batchnorm run BatchNorm in training mode; decode_output "
                 "chains them), but the image gradient and the non-local block's backward are missing; the training route of "
                 "EgoHMR.forward runs once EgoHMR.frozen_trunk_training is set - with the trunk's weights frozen unless EgoHMR.trunk_grad is set, and "
                 "its statistics frozen unless ResNet50Features.train_batchnorm is set too")

    def init_optimizers(self):
        """egohmr.py:140-147: the reference's parameter list in its order - without `backbone` while the trunk is frozen, with it in front behind
        EgoHMR.trunk_grad."""
        self.opt_params = ((list(self.backbone.parameters()) if self.trunk_grad else []) + list(self.scene_enc.parameters()) + list(self.transl_enc.parameters()) + list(self.beta_layer.parameters()) +
                           list(self.diffusion_model.parameters()) + list(self.embed_timestep.parameters()) + list(self.input_process.parameters()))
        self.optimizer = torch.optim.AdamW(params=self.opt_params, lr=self.cfg.TRAIN.LR, weight_decay=self.cfg.TRAIN.WEIGHT_DECAY)
        if self._data_parallel_world() > 1:
            self._data_parallel_setup()

    def _data_parallel_setup(self):
        """EgoHMR.data_parallel, once: every rank must hold the same list of (numel, requires_grad) - else the ranks would issue different collectives in a
        step - and then takes rank 0's parameters and buffers (moved in place, so the handles that key on them rebuild)."""
        import torch.distributed as td
        mine = [(p.numel(), bool(p.requires_grad)) for p in self.opt_params]
        lists = [None] * td.get_world_size()
        td.all_gather_object(lists, mine)
        for r, other in enumerate(lists):
            if other != mine:
                raise ValueError(f"EgoHMR.data_parallel: rank {r}'s optimizer list differs from rank {td.get_rank()}'s in (numel, requires_grad): "
                                 f"{len(other)} against {len(mine)} tensors" + "".join(
                                     f"; entry {i}: {a} against {b}" for i, (a, b) in enumerate(zip(other, mine)) if a != b)[:200])
        host = td.get_backend() == "gloo"
        by_dtype = {}
        for t in list(self.parameters()) + list(self.buffers()):
            by_dtype.setdefault((t.dtype, t.device), []).append(t)
        with torch.no_grad():
            for ts in by_dtype.values():                    # one broadcast per dtype and device (float32; the int64 num_batches_tracked)
                flat = torch.cat([t.detach().reshape(-1) for t in ts])
                flat = flat.cpu() if host and flat.is_cuda else flat
                td.broadcast(flat, src=0)
                if td.get_rank() != 0:
                    for t, v in zip(ts, flat.split([t.numel() for t in ts])):
                        t.copy_(v.view_as(t))

    def _reduce_gradients(self):
        """The gradients of init_optimizers' list, summed over the ranks in ONE flat all-reduce (flattened and unflattened with torch ops)."""
        from . import dist as ehm_dist
        params = [p for p in self.opt_params if p.requires_grad]
        for p, (name, _) in zip(self.opt_params, self._opt_param_names()):
            if p.requires_grad and p.grad is None:
                raise ValueError(f"EgoHMR.data_parallel: {name} requires grad and received none in this step; the ranks sum one gradient per tensor "
                                 "of init_optimizers' list")
        flat = torch.cat([p.grad.reshape(-1).float() for p in params])
        ehm_dist.all_reduce_sum_(flat)
        torch._foreach_copy_([p.grad for p in params], [c.view_as(p.grad) for p, c in zip(params, flat.split([p.numel() for p in params]))])

    def _opt_param_names(self):
        """(name, parameter) per entry of opt_params"""
        names = {id(p): n for n, p in self.named_parameters()}
        return [(names.get(id(p), f"opt_params[{i}]"), p) for i, p in enumerate(self.opt_params)]

    def training_step(self, batch=None, timesteps=None, cur_epoch=0):
        """egohmr.py:453-472 behind frozen_trunk_training (else NotImplementedError): the training modes (_set_train_modes; left as set, validation_setup
        restores eval), forward, compute_loss, zero_grad, backward, one step of the optimizer of init_optimizers; returns the output dict.
        Behind EgoHMR.data_parallel with more than one rank, `batch` is this rank's shard: the counts B_r are exchanged (one small collective; a rank without
        items is refused on every rank), the train-mode BatchNorms of the denoiser (diffusion_model.train_batchnorm) and of the backbone (trunk_grad +
        backbone.train_batchnorm) run on all ranks' rows, loss B_r / B is backpropagated - every term of the loss is a mean over the items, so all
        cotangents are then in units of the whole batch's mean loss and add over the ranks unweighted, ragged shards included - and the gradients are
        summed over the ranks before the optimizer step.  output['losses'] stays this rank's."""
        if not getattr(self, "frozen_trunk_training", False):
            raise NotImplementedError("training_step is not built: " + EgoHMR.NOT_BUILT)
        self._check_trainable()
        self._set_train_modes()
        if self._data_parallel_world() == 1:
            output = self.forward(batch, timesteps, eval_with_uncond=False)                                # :465
            loss = self.compute_loss(batch, output, cur_epoch=cur_epoch)
            self.optimizer.zero_grad()
            loss.backward()
            self.optimizer.step()
            return output
        from . import dist as ehm_dist
        dm, bb = self.diffusion_model, self.backbone
        sync = ehm_dist.StatSync.exchange(int(batch["x_t"].reshape(-1, 144).shape[0]), self.device)
        try:
            dm.stat_sync = sync if dm.train_batchnorm else None
            bb.stat_sync = sync if self.trunk_grad and bb.train_batchnorm else None
            output = self.forward(batch, timesteps, eval_with_uncond=False)
            loss = self.compute_loss(batch, output, cur_epoch=cur_epoch)
            self.optimizer.zero_grad()
            (loss * sync.loss_weight).backward()
        finally:
            dm.stat_sync = bb.stat_sync = None
        self._reduce_gradients()
        self.optimizer.step()
        return output


class EgoHMRVolsmpl(EgoHMR):
    """models/egohmr/egohmr_volsmpl.py: the same network with VolumetricSMPL instead of COAP behind the collision guidance.
    What differs on the sampling path (everything else in that file is a re-formatted copy of egohmr.py):
      guide_coll          :582-629  one BATCHED `volume.collision_loss(scene, smpl_output)` over ALL scene points (no per-item bounding-box
                                    selection), gradient of `-loss.sum()` (no 1/B factor); default guidance weight 30 (test_egohmr_volsmpl.py:62)
      eval_coll_volsmpl   :548-579  per item, bbox-selected points with `volume.query_fast(...) < 0` over N
      eval_coll           :519-546  the COAP metric, kept (the reference keeps COAP attached for training)
    VolumetricSMPL is a learned SDF that cannot be obtained offline: the collision term is the build's proxy (docs/EXPERIMENTS.md 3.5),
    with `sdf < 0` read as `distance to the surface < tau` (collision_proxy = 'mesh': as "inside the posed mesh").  Numbers from it are NOT VolumetricSMPL numbers - unless the user's model is attached as
    `collision_model`: guide_coll then makes the reference's one batched `collision_loss(scene, smpl_output)` call and differentiates `-loss.sum()` through
    the differentiable SMPL.forward, eval_coll_volsmpl reads its `query_fast` (or `query`) as a signed distance, and guided loops run step by step."""

    DEFAULT_COND_GRAD_WEIGHT = 30.0            # test_egohmr_volsmpl.py:62

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.guide_reduction = "sum"
        self.guide_all_points = True

    def eval_coll_volsmpl(self, output):
        """egohmr_volsmpl.py:548-579.  Without a collision model the build's proxy stands in for both metrics (bbox-selected points in both); with one,
        its `query_fast` (or, lacking that, `query`) is read as a signed distance: `< 0` = inside."""
        cm = self.collision_model
        if cm is None:
            return EgoHMR.eval_coll(self, output)
        return self._hit_share_model(output, getattr(cm, "query_fast", cm.query), lambda sdf: sdf < 0)
