"""Stage 1 of the reference's two-stage evaluation: its ProHMR-scene model (models/prohmr/prohmr_scene.py) as test_prohmr_scene.py runs it.

``ProHMRSceneTransl`` is the deterministic half, the body translation a ``--two_stage`` stage-2 run conditions on
(``results.pkl['pred_cam_full_list']``, test_prohmr_scene.py:417-426): ``pred_cam = FCHead(feats)`` (models/prohmr/smpl_flow.py:88-90,
fc_head.py:46-50) on the conditioning features of prohmr_scene.py:111-130, converted to the full-image camera by convert_pare_to_full_img_cam
(test_prohmr_scene.py:175-213).  ``ProHMRScene`` adds the rest of ``forward_step(train=False)``: the conditional normalizing flow
(``GlowFlow``: pose samples around the mode z = 0, their log-probabilities), the SMPL decode and the projections.

    ResNet-50 (img) and ResnetPointnet(512, 256) (scene)   the encoders of egohmr_amd.encoders, same kernels as EgoHMR's
    context assembly + FCHead + camera conversion          one launch of ehm_stage1_head (csrc/stage1.hip)
    the flow, either direction                             ehm_flow_context, one ehm_skinny_gemm_f32 for the per-item terms, one ehm_flow_gemm per
                                                           per-row product (~29), ehm_flow_finish (csrc/flow.hip)

The flow's definition is restated from ProHMR section 3.2 and published nflows (tests/flow_ref.py is the float64 statement the kernels are tested
against); ProHMR's fork of nflows was not at hand, so parity with a real checkpoint is unpinned until tools/verify_assets.py has read one.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .encoders import ResNet50Features, ResnetPointnet
from .synthetic import FLOW_DEPTH, FLOW_DIM, FLOW_LAYERS      # configs/prohmr.yaml MODEL.FLOW: DIM, NUM_LAYERS, LAYER_DEPTH (LAYER_HIDDEN_FEATURES = HIDDEN)

IMG_DIM, HIDDEN, CROP_RES = 2048, 1024, 224      # configs/prohmr.yaml: MODEL.FLOW.CONTEXT_FEATURES, MODEL.FC_HEAD.NUM_FEATURES, MODEL.IMAGE_SIZE


class _FCHead(nn.Module):
    """models/prohmr/fc_head.py: Linear(ctx, 1024) - ReLU - Linear(1024, 13) and the mean-parameter buffers (a parameter container)."""

    def __init__(self, ctx_dim: int):
        super().__init__()
        self.layers = nn.Sequential(nn.Linear(ctx_dim, HIDDEN), nn.ReLU(inplace=False), nn.Linear(HIDDEN, 13))
        self.register_buffer("init_cam", torch.zeros(1, 1, 3))
        self.register_buffer("init_betas", torch.zeros(1, 1, 10))


class _Flow(nn.Module):
    """The `flow` submodule of the reference (SMPLFlow) reduced to its `fc_head`: checkpoint names stay `flow.fc_head.*`."""

    def __init__(self, ctx_dim: int):
        super().__init__()
        self.fc_head = _FCHead(ctx_dim)


class ProHMRSceneTransl(nn.Module):
    """The stage-1 camera translation of ProHMRScene (prohmr_scene.py) with the reference's state_dict names: ``backbone``, ``scene_enc``,
    ``flow.fc_head``.  Load a ProHMR-scene checkpoint with egohmr_amd.io.load_stage1_checkpoint.

    ``forward(batch)`` reads ``img`` [B,3,224,224], ``scene_pcd_verts_full`` [B,N,3], ``fx``, ``cam_cx``, ``cam_cy``, ``box_size`` [B] and
    ``box_center`` [B,2] and returns ``pred_cam`` [B,3] (the weak-perspective camera of the mode, z = 0), ``pred_cam_full`` [B,3] (the body
    translation in the camera frame, what results.pkl stores) and ``pred_betas`` [B,10].

    Stage 1 takes its OWN batch: it reads the whole-scene cloud (test_prohmr_scene.py:41, scene_type='whole_scene': the 20 000 scene points in
    front of the camera), while stage 2 reads the 2 m cube cropped around this stage's translation.  The reference runs two scripts over two
    dataset configurations; so does a caller of this package.  The scene frame is the camera frame (scene_cano=False, the
    script's default)."""

    def __init__(self, with_focal_length: bool = True, with_bbox_info: bool = True, with_cam_center: bool = True, fx_norm_coeff: float = 1500.0,
                 scene_feat_dim: int = 512, device=None):
        super().__init__()
        self.with_focal_length, self.with_bbox_info, self.with_cam_center = bool(with_focal_length), bool(with_bbox_info), bool(with_cam_center)
        self.fx_norm_coeff = float(fx_norm_coeff)
        self.scene_feat_dim = int(scene_feat_dim)
        self.context_dim = (IMG_DIM + self.scene_feat_dim + (1 if self.with_focal_length else 0) + (3 if self.with_bbox_info else 0)
                            + (2 if self.with_cam_center else 0))          # prohmr_scene.py:36-45
        self.backbone = ResNet50Features()
        self.scene_enc = ResnetPointnet(out_dim=self.scene_feat_dim, hidden_dim=256)
        self.flow = _Flow(self.context_dim)
        # arithmetic of the two encoders, as EgoHMR.encoder_precision: 'f16x3' (split-f16, f32 grade) | 'f16' (plain f16, NOT parity grade)
        self.encoder_precision = "f16x3"
        self._head_key_fn, self._head_key, self._head = None, None, None
        if device is not None:
            self.to(device)
        self.eval()

    def _head_weights(self, dev):
        """W1 transposed to [K, 1024] (the kernel's layout) and the other head tensors as contiguous float32, rebuilt when a weight changes."""
        if self._head_key_fn is None:
            self._head_key_fn = _lib.TensorKey(self.flow)
        key = self._head_key_fn() + (str(dev),)
        if self._head_key != key:
            h = self.flow.fc_head
            W1 = h.layers[0].weight
            if tuple(W1.shape) != (HIDDEN, self.context_dim):
                raise ValueError(f"flow.fc_head.layers.0.weight is {tuple(W1.shape)}, the context flags need ({HIDDEN}, {self.context_dim})")
            self._head = dict(W1t=_lib.f32(W1, dev).t().contiguous(), b1=_lib.f32(h.layers[0].bias, dev), W2=_lib.f32(h.layers[2].weight, dev),
                              b2=_lib.f32(h.layers[2].bias, dev), init_cam=_lib.f32(h.init_cam, dev).reshape(3),
                              init_betas=_lib.f32(h.init_betas, dev).reshape(10))
            self._head_key = key
        return self._head

    def head(self, img_feats, scene_feats, fx, cam_cx, cam_cy, box_center, box_size) -> dict:
        """ehm_stage1_head on given features: context assembly, FCHead and the camera conversion (one launch)."""
        dev = img_feats.device
        with _lib.on_device(dev):
            st = _lib.stream_ptr()
            B = img_feats.shape[0]
            img, scene = _lib.f32(img_feats, dev), _lib.f32(scene_feats, dev)
            if img.shape != (B, IMG_DIM) or scene.shape != (B, self.scene_feat_dim):
                raise ValueError(f"features {tuple(img.shape)} / {tuple(scene.shape)}, expected [B,{IMG_DIM}] / [B,{self.scene_feat_dim}]")
            sc = [_lib.f32(x, dev).reshape(B) for x in (fx, cam_cx, cam_cy, box_size)]
            bc = _lib.f32(box_center, dev).reshape(B, 2)
            w = self._head_weights(dev)
            out = {"pred_cam": torch.empty(B, 3, device=dev), "pred_cam_full": torch.empty(B, 3, device=dev), "pred_betas": torch.empty(B, 10, device=dev)}
            P = _lib.ptr
            d = _lib.Stage1Desc(img_feats=P(img), scene_feats=P(scene), fx=P(sc[0]), cam_cx=P(sc[1]), cam_cy=P(sc[2]), box_center=P(bc), box_size=P(sc[3]),
                                W1t=P(w["W1t"]), b1=P(w["b1"]), W2=P(w["W2"]), b2=P(w["b2"]), init_cam=P(w["init_cam"]), init_betas=P(w["init_betas"]),
                                pred_cam=P(out["pred_cam"]), pred_cam_full=P(out["pred_cam_full"]), pred_betas=P(out["pred_betas"]),
                                fx_norm=self.fx_norm_coeff, crop_res=float(CROP_RES), with_cam_center=int(self.with_cam_center),
                                with_bbox_info=int(self.with_bbox_info), with_focal_length=int(self.with_focal_length), img_dim=IMG_DIM,
                                scene_dim=self.scene_feat_dim, hidden=HIDDEN, B=B)
            _lib.api().ehm_stage1_head(C.byref(d), st)
        return out

    def _encode(self, batch):
        """(img_feats [B,2048], scene_feats [B,scene_feat_dim]): the two encoders of prohmr_scene.py:111 and :127."""
        if self.encoder_precision not in ("f16x3", "f16"):
            raise ValueError(f"encoder_precision must be 'f16x3' or 'f16', not {self.encoder_precision!r}")
        self.backbone.hi_only = self.scene_enc.hi_only = self.encoder_precision == "f16"
        img = batch["img"]
        if not img.is_cuda:
            raise _lib.EgoHMRHipError(f"{type(self).__name__} runs on the HIP kernels only (got a CPU tensor); there is no CPU path")
        if img.shape[0] == 0:
            raise ValueError("empty batch")
        with _lib.on_device(img.device):
            return self.backbone(img), self.scene_enc(batch["scene_pcd_verts_full"])

    @torch.no_grad()
    def forward(self, batch) -> dict:
        img_feats, scene_feats = self._encode(batch)
        return self.head(img_feats, scene_feats, batch["fx"], batch["cam_cx"], batch["cam_cy"], batch["box_center"], batch["box_size"])


# --------------------------------------------------------------------------------------------- the conditional Glow flow
_HALF = FLOW_DIM // 2
_BN_EPS = 1e-3                                    # nflows' ResidualBlock: BatchNorm1d(features, eps=1e-3)


class _ActNorm(nn.Module):
    def __init__(self):
        super().__init__()
        self.log_scale, self.shift = nn.Parameter(torch.zeros(FLOW_DIM)), nn.Parameter(torch.zeros(FLOW_DIM))
        self.register_buffer("initialized", torch.tensor(True, dtype=torch.bool))


class _LULinear(nn.Module):
    def __init__(self):
        super().__init__()
        n = FLOW_DIM * (FLOW_DIM - 1) // 2
        self.lower_entries, self.upper_entries = nn.Parameter(torch.zeros(n)), nn.Parameter(torch.zeros(n))
        self.unconstrained_upper_diag = nn.Parameter(torch.full((FLOW_DIM,), math.log(math.e - 1)))      # softplus -> 1
        self.bias = nn.Parameter(torch.zeros(FLOW_DIM))


class _ResidualBlock(nn.Module):
    def __init__(self, ctx_dim: int, batch_norm: bool):
        super().__init__()
        if batch_norm:
            self.batch_norm_layers = nn.ModuleList([nn.BatchNorm1d(HIDDEN, eps=_BN_EPS) for _ in range(2)])
        self.context_layer = nn.Linear(ctx_dim, HIDDEN)
        self.linear_layers = nn.ModuleList([nn.Linear(HIDDEN, HIDDEN) for _ in range(2)])


class _ResidualNet(nn.Module):
    def __init__(self, ctx_dim: int, batch_norm: bool):
        super().__init__()
        self.initial_layer = nn.Linear(_HALF + ctx_dim, HIDDEN)
        self.blocks = nn.ModuleList([_ResidualBlock(ctx_dim, batch_norm) for _ in range(FLOW_DEPTH)])
        self.final_layer = nn.Linear(HIDDEN, _HALF)


class _Coupling(nn.Module):
    def __init__(self, ctx_dim: int, batch_norm: bool, even: bool):
        super().__init__()
        # (nflows' alternating mask as the initial value only: the lists are read from the checkpoint)
        tr = torch.arange(0 if even else 1, FLOW_DIM, 2)
        self.register_buffer("identity_features", torch.arange(1 if even else 0, FLOW_DIM, 2))
        self.register_buffer("transform_features", tr)
        self.transform_net = _ResidualNet(ctx_dim, batch_norm)


class _Composite(nn.Module):
    def __init__(self, transforms):
        super().__init__()
        self._transforms = nn.ModuleList(transforms)


class GlowFlow(nn.Module):
    """nflows' ConditionalGlow(144, 1024, 4, 2, context_features=ctx_dim) of models/prohmr/smpl_flow.py:24-26 with the parameter
    names of published nflows (``_transform._transforms.{3l | 3l+1 | 3l+2}`` = ActNorm | LULinear | additive coupling with a ResidualNet), so a
    checkpoint's ``flow.flow.*`` loads with strict=True.  ``batch_norm``: the ResidualNet blocks carry their two eval-mode BatchNorm1d.

    Both directions run on csrc/flow.hip.  Once per weight change the host folds each ActNorm + LULinear into one affine map (float64: A = L U
    diag(exp(log_scale)), c = L U shift + bias, and A^-1 by two triangular solves), concatenates the twelve context-side weight slices (each
    coupling's first layer and two GLU gates) into one [ctx_pad, 12 * 1024] matrix, and transposes the per-row weights.  A direction is then
    ehm_skinny_gemm_f32 for the per-item terms and 7 ehm_flow_gemm launches per block (the affine map, the first layer, 2 x 2 hidden layers, the
    last layer with the coupling update), then ehm_flow_finish.  No atomics: two calls give the same bits.  CPU tensors raise.

    Both directions are differentiable (egohmr_amd/flow_grad.py, a HIP backward behind ``flow_grad.FlowFunction``): with grad mode on, a call whose
    ``x`` / ``z`` / ``ctx`` requires grad - or, with ``grad_params = True`` (the meaning of ``ResnetPointnet.grad_params``), whose flow has a
    parameter that does - returns results with a ``grad_fn``.  Every other call runs the no-graph route.  The ResidualNet's BatchNorm is not
    differentiated: ``batch_norm=True`` raises on the autograd route."""
    grad_params = False

    def __init__(self, ctx_dim: int, batch_norm: bool = False):
        super().__init__()
        self.ctx_dim, self.batch_norm = int(ctx_dim), bool(batch_norm)
        self.ctx_pad = -(-self.ctx_dim // 32) * 32
        tr = []
        for l in range(FLOW_LAYERS):
            tr += [_ActNorm(), _LULinear(), _Coupling(self.ctx_dim, self.batch_norm, even=l % 2 == 0)]
        self._transform = _Composite(tr)
        self._key_fn, self._key, self._w = None, None, None
        self.eval()

    # ------------------------------------------------------------------ host preparation
    @staticmethod
    def fold(an, lu):
        """ActNorm + LULinear -> one affine map each way, float64 numpy: (A [144,144], c [144], A^-1, log|det A|) with s <- s A^T + c.
        (flow_grad.fold is the same map as a torch function, for the gradients of the six parameters.)"""
        D = FLOW_DIM
        f64 = lambda t: t.detach().double().cpu().numpy()
        Lm, U = np.eye(D), np.zeros((D, D))
        Lm[np.tril_indices(D, -1)] = f64(lu.lower_entries)
        U[np.triu_indices(D, 1)] = f64(lu.upper_entries)
        diag = np.log1p(np.exp(f64(lu.unconstrained_upper_diag))) + 1e-3
        U[np.diag_indices(D)] = diag
        ls, LU = f64(an.log_scale), Lm @ U
        A, c = LU * np.exp(ls)[None, :], LU @ f64(an.shift) + f64(lu.bias)
        tri = lambda M, rhs, upper: torch.linalg.solve_triangular(torch.from_numpy(M), torch.from_numpy(rhs), upper=upper).numpy()
        Ainv = np.exp(-ls)[:, None] * tri(U, tri(Lm, np.eye(D), False), True)                      # two float64 triangular solves, not inv(L U diag)
        return A, c, Ainv, float(ls.sum() + np.log(diag).sum())

    def _weights(self, dev):
        if self._key_fn is None:
            self._key_fn = _lib.TensorKey(self)
        key = self._key_fn() + (str(dev),)
        if self._key == key:
            return self._w
        D, H, ctx = FLOW_DIM, HIDDEN, self.ctx_dim
        f64 = lambda t: t.detach().double().cpu().numpy()
        dev32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        tr = self._transform._transforms
        blocks, logdet = [], 0.0
        Wctx = torch.zeros(self.ctx_pad, 3 * FLOW_LAYERS * H, device=dev)
        bctx = torch.empty(3 * FLOW_LAYERS * H, device=dev)
        for l in range(FLOW_LAYERS):
            an, lu, cp = tr[3 * l], tr[3 * l + 1], tr[3 * l + 2]
            if not bool(an.initialized):
                raise ValueError(f"GlowFlow: ActNorm {3 * l} has initialized == False (data-dependent initialisation belongs to training)")
            A, c, Ainv, ld = self.fold(an, lu)
            logdet += ld
            pad = lambda Wt: np.concatenate([Wt, np.zeros((D, 160 - D))], 1)                       # [K = 144, ldw = 160]
            w = dict(At=dev32(pad(A.T)), Ainvt=dev32(pad(Ainv.T)), c=dev32(c))
            w["A"], w["Ainv"] = dev32(A), dev32(Ainv)                                              # the backward's operands: ds A, dx Ainv
            # ---- the coupling
            idf, trf = cp.identity_features.detach().cpu().numpy().astype(np.int64), cp.transform_features.detach().cpu().numpy().astype(np.int64)
            if idf.shape != (_HALF,) or trf.shape != (_HALF,) or sorted(np.concatenate([idf, trf]).tolist()) != list(range(D)):
                raise ValueError(f"GlowFlow: coupling {3 * l + 2}: identity_features / transform_features are not a split of 0 .. {D - 1} into {_HALF} + {_HALF}")
            w["idf"], w["trf"] = (torch.from_numpy(a.astype(np.int32)).to(dev) for a in (idf, trf))
            net = cp.transform_net
            W0 = _lib.f32(net.initial_layer.weight, dev)
            if tuple(W0.shape) != (H, _HALF + ctx) or tuple(net.final_layer.weight.shape) != (_HALF, H):
                raise ValueError(f"GlowFlow: coupling {3 * l + 2}: initial_layer.weight is {tuple(W0.shape)}, final_layer.weight "
                                 f"{tuple(net.final_layer.weight.shape)}; the context width {ctx} needs ({H}, {_HALF + ctx}) and ({_HALF}, {H})")
            w["Wx"] = W0[:, :_HALF].t().contiguous()                                               # [72, 1024]
            # (the backward reads the torch-layout weights themselves, [out, in] = the [K, N] operand of dY W^T: no copy when they are float32)
            w["W0"], w["Wf_oi"], w["Wc"] = W0, _lib.f32(net.final_layer.weight, dev), []
            slot = 3 * l
            Wctx[:ctx, slot * H:(slot + 1) * H] = W0[:, _HALF:].t()
            bctx[slot * H:(slot + 1) * H] = _lib.f32(net.initial_layer.bias, dev)
            w["lin"] = []
            for k, blk in enumerate(net.blocks):
                Wc = _lib.f32(blk.context_layer.weight, dev)
                if tuple(Wc.shape) != (H, ctx):
                    raise ValueError(f"GlowFlow: coupling {3 * l + 2}: blocks.{k}.context_layer.weight is {tuple(Wc.shape)}, expected ({H}, {ctx})")
                Wctx[:ctx, (slot + 1 + k) * H:(slot + 2 + k) * H] = Wc.t()
                w["Wc"].append(Wc)
                bctx[(slot + 1 + k) * H:(slot + 2 + k) * H] = _lib.f32(blk.context_layer.bias, dev)
                for j in range(2):
                    Wl = _lib.f32(blk.linear_layers[j].weight, dev)
                    e = dict(W=Wl, Wt=Wl.t().contiguous(), b=_lib.f32(blk.linear_layers[j].bias, dev), s=None, o=None)
                    if self.batch_norm:                                                            # eval-mode BatchNorm1d as x s + o, float64
                        bn = blk.batch_norm_layers[j]
                        s = f64(bn.weight) / np.sqrt(f64(bn.running_var) + _BN_EPS)
                        e["s"], e["o"] = dev32(s), dev32(f64(bn.bias) - f64(bn.running_mean) * s)
                    w["lin"].append(e)
            Wf = torch.zeros(H, 96, device=dev)                                                    # [K = 1024, ldw = 96], 72 live columns
            Wf[:, :_HALF] = _lib.f32(net.final_layer.weight, dev).t()
            w["Wf"], w["bf"] = Wf, _lib.f32(net.final_layer.bias, dev)
            blocks.append(w)
        self._w = dict(blocks=blocks, Wctx=Wctx, bctx=bctx, logdet=logdet, log_prob_const=-_HALF * math.log(2.0 * math.pi) + logdet)
        self._key = key
        return self._w

    @property
    def logdet(self) -> float:
        """log |det dz/dx| of the x -> z direction (data independent; float64 on the host).  Needs the weights on a HIP device."""
        return self._weights(next(self.parameters()).device)["logdet"]

    # ------------------------------------------------------------------ launches
    def _padded_context(self, ctx):
        if not ctx.is_cuda:
            raise _lib.EgoHMRHipError("GlowFlow runs on the HIP kernels only (got a CPU tensor); there is no CPU path")
        ctx = _lib.f32(ctx)
        if ctx.dim() != 2 or ctx.shape[1] != self.ctx_dim:
            raise ValueError(f"context {tuple(ctx.shape)}, expected [B, {self.ctx_dim}]")
        if self.ctx_pad == self.ctx_dim:
            return ctx
        out = torch.zeros(ctx.shape[0], self.ctx_pad, device=ctx.device)
        out[:, :self.ctx_dim] = ctx
        return out

    def _item_terms(self, ctxp, w, st):
        """[B, 12 * 1024]: every coupling's context product of its first layer and of its two GLU gates, biases included."""
        B = ctxp.shape[0]
        P = torch.empty(B, w["Wctx"].shape[1], device=ctxp.device)
        _lib.api().ehm_skinny_gemm_f32(ctxp, w["Wctx"], w["bctx"], P, B, self.ctx_pad, P.shape[1], 0, st)
        return P

    @staticmethod
    def _gemm(st, X, W, Y, R, K, N, ldx, ldw, ldy, S=1, bias=None, gather=None, pro=_lib.FLOW_PRO_NONE, pro_scale=None, pro_shift=None,
              epi=_lib.FLOW_EPI_BIAS, item=None, ld_item=0, scatter=None, mask=None, add=None, aux=None, ld_mask=0, ld_add=0, w_window=0):
        P = lambda t: t if isinstance(t, int) else _lib.ptr(t)      # (an int: the address of a column window)
        d = _lib.FlowGemmDesc(X=P(X), gather=P(gather), W=P(W), bias=P(bias), pro_scale=P(pro_scale), pro_shift=P(pro_shift),
                              item=item, scatter=P(scatter), Y=P(Y), R=R, K=K, N=N, S=S, ldx=ldx, ldw=ldw, ldy=ldy, ld_item=ld_item,
                              prologue=pro, epilogue=epi, mask=P(mask), add=P(add), aux=P(aux), ld_mask=ld_mask, ld_add=ld_add,
                              w_window=w_window)
        _lib.api().ehm_flow_gemm(C.byref(d), st)

    def _coupling(self, st, w, l, state, T, U, P, R, S, subtract, keep=None):
        """state[:, tr] +/-= transform_net(state[:, id], context): six launches, in place on the state.  keep (the autograd route): a dict that
        receives what the backward reads - t_0, u1_0, u2_0, t_1, u1_1, u2_1, t_2 - from the same launches on the same operands; a GLU then writes
        t_k+1 beside t_k (`add`) instead of over it, and its value half u2 goes out through `aux` (kept, not recomputed: 2 x [R,1024] per coupling
        against one more GEMM per block in the backward)."""
        D, H, g = FLOW_DIM, HIDDEN, self._gemm
        if keep is not None:
            new = lambda: torch.empty(R, H, device=state.device)
            keep["t"], keep["u1"], keep["u2"] = [new(), new(), new()], [new(), new()], [new(), new()]
            T = keep["t"][0]
        item = lambda slot: P.data_ptr() + 4 * H * slot
        ldp = P.shape[1]
        g(st, state, w["Wx"], T, R, _HALF, H, D, H, H, S=S, gather=w["idf"], epi=_lib.FLOW_EPI_ITEM_ADD, item=item(3 * l), ld_item=ldp)
        for k in range(FLOW_DEPTH):
            e0, e1 = w["lin"][2 * k], w["lin"][2 * k + 1]
            pro = _lib.FLOW_PRO_BN_RELU if self.batch_norm else _lib.FLOW_PRO_RELU
            if keep is not None:
                U, Tn = keep["u1"][k], keep["t"][k + 1]
            g(st, T, e0["Wt"], U, R, H, H, H, H, H, bias=e0["b"], pro=pro, pro_scale=e0["s"], pro_shift=e0["o"])
            if keep is None:
                g(st, U, e1["Wt"], T, R, H, H, H, H, H, S=S, bias=e1["b"], pro=pro, pro_scale=e1["s"], pro_shift=e1["o"], epi=_lib.FLOW_EPI_GLU_RES,
                  item=item(3 * l + 1 + k), ld_item=ldp)
            else:
                g(st, U, e1["Wt"], Tn, R, H, H, H, H, H, S=S, bias=e1["b"], pro=pro, pro_scale=e1["s"], pro_shift=e1["o"], epi=_lib.FLOW_EPI_GLU_RES,
                  item=item(3 * l + 1 + k), ld_item=ldp, add=T, ld_add=H, aux=keep["u2"][k])
                T = Tn
        g(st, T, w["Wf"], state, R, H, _HALF, H, 96, D, bias=w["bf"], scatter=w["trf"],
          epi=_lib.FLOW_EPI_SCATTER_SUB if subtract else _lib.FLOW_EPI_SCATTER_ADD)

    def _run(self, ctxp, rows, S, sampling, keep=None):
        """One direction on rows [R,144] (the noise when sampling, else the poses), R = B * S.  Sampling: (pose6d, log_prob, global_orient,
        body_pose); else (log_prob, z).  keep (the autograd route): a dict that receives the per-item terms `P`, per block the coupling's
        activations (`blocks`) and the states (`states`): forward, states[l] enters affine map l and states[l + 1] leaves coupling l; sampling,
        states[l] is the state between coupling l and its affine map (a coupling leaves its identity half alone, so either holds s[:, idf]).  The
        route takes a fresh buffer per block where the no-graph route swaps two: same launches, same operands, same bits."""
        dev = rows.device
        w = self._weights(dev)
        R, D, H = rows.shape[0], FLOW_DIM, HIDDEN
        with _lib.on_device(dev):
            st = _lib.stream_ptr()
            P = self._item_terms(ctxp, w, st)
            T, U = (None, None) if keep is not None else (torch.empty(R, H, device=dev), torch.empty(R, H, device=dev))
            a, b = torch.empty(R, D, device=dev), torch.empty(R, D, device=dev)
            lp = torch.empty(R, device=dev)
            if keep is not None:
                keep.update(P=P, blocks=[{} for _ in range(FLOW_LAYERS)], states=[None] * (FLOW_LAYERS + (0 if sampling else 1)), w=w, rows=rows,
                            ctxp=ctxp, S=S)
            kept = lambda l: keep["blocks"][l] if keep is not None else None
            if sampling:
                a.copy_(rows)                                  # (the coupling updates its state in place; the noise is kept for the norm)
                for l in reversed(range(FLOW_LAYERS)):
                    wl = w["blocks"][l]
                    self._coupling(st, wl, l, a, T, U, P, R, S, subtract=True, keep=kept(l))
                    self._gemm(st, a, wl["Ainvt"], b, R, D, D, D, 160, D, pro=_lib.FLOW_PRO_SHIFT, pro_shift=wl["c"])   # (state - c) Ainv^T
                    if keep is not None:
                        keep["states"][l] = a
                        a, b = b, torch.empty(R, D, device=dev)
                    else:
                        a, b = b, a
                p6, go, bp = torch.empty(R, D, device=dev), torch.empty(R, 1, 3, 3, device=dev), torch.empty(R, 23, 3, 3, device=dev)
                _lib.api().ehm_flow_finish(rows, C.c_double(w["log_prob_const"]), lp, a, p6, go, bp, R, st)
                if keep is not None:
                    keep["x"] = a
                return p6, lp, go, bp
            x = rows
            for l in range(FLOW_LAYERS):
                wl = w["blocks"][l]
                self._gemm(st, x, wl["At"], b, R, D, D, D, 160, D, bias=wl["c"])                                        # state A^T + c
                self._coupling(st, wl, l, b, T, U, P, R, S, subtract=False, keep=kept(l))
                if keep is not None:
                    keep["states"][l], keep["states"][l + 1] = x, b
                    x, b = b, torch.empty(R, D, device=dev)
                else:
                    x, b = b, (a if x is rows else x)
            _lib.api().ehm_flow_finish(x, C.c_double(w["log_prob_const"]), lp, None, None, None, None, R, st)
            if keep is not None:
                keep["z"] = x
            return lp, x

    def _wants_grad(self, *tensors) -> bool:
        from .flow_grad import wants_grad
        return wants_grad(self, *tensors)

    def sample_and_log_prob(self, ctx, num_samples=None, z=None, _padded=None) -> dict:
        """x = inverse(z) given the context ctx [B, ctx_dim]: z [B,S,144], or S = num_samples rows per item drawn from the global generator.
        -> ``pred_pose_6d`` [B,S,144], ``log_prob`` [B,S], ``z`` [B,S,144], ``global_orient`` [B,S,1,3,3], ``body_pose`` [B,S,23,3,3] (the
        'prohmr' rot6d rule on pred_pose_6d)."""
        if self._wants_grad(ctx, z, _padded):
            from .flow_grad import run_with_grad
            return run_with_grad(self, ctx if _padded is None else _padded, z, num_samples, sampling=True)
        with torch.no_grad():
            return self._sample_and_log_prob(ctx, num_samples, z, _padded)

    def _sample_and_log_prob(self, ctx, num_samples, z, _padded, keep=None):
        ctxp = _padded if _padded is not None else self._padded_context(ctx)
        B, dev = ctxp.shape[0], ctxp.device
        if z is None:
            if num_samples is None or int(num_samples) < 1:
                raise ValueError("sample_and_log_prob needs z or num_samples >= 1")
            z = torch.randn(B * int(num_samples), FLOW_DIM, device=dev).reshape(B, int(num_samples), FLOW_DIM)
        if not z.is_cuda:
            raise _lib.EgoHMRHipError("GlowFlow runs on the HIP kernels only (got a CPU tensor); there is no CPU path")
        z = _lib.f32(z, dev)
        if z.dim() != 3 or z.shape[0] != B or z.shape[2] != FLOW_DIM:
            raise ValueError(f"z {tuple(z.shape)}, expected [{B}, S, {FLOW_DIM}]")
        S = z.shape[1]
        p6, lp, go, bp = self._run(ctxp, z.reshape(B * S, FLOW_DIM), S, sampling=True, keep=keep)
        return {"pred_pose_6d": p6.reshape(B, S, FLOW_DIM), "log_prob": lp.reshape(B, S), "z": z, "global_orient": go.reshape(B, S, 1, 3, 3),
                "body_pose": bp.reshape(B, S, 23, 3, 3)}

    def log_prob(self, x, ctx, _padded=None):
        """(log_prob [B,S], z [B,S,144]) of the poses x [B,S,144] given the context ctx [B, ctx_dim]."""
        if self._wants_grad(ctx, x, _padded):
            from .flow_grad import run_with_grad
            return run_with_grad(self, ctx if _padded is None else _padded, x, None, sampling=False)
        with torch.no_grad():
            return self._log_prob(x, ctx, _padded)

    def _log_prob(self, x, ctx, _padded, keep=None):
        ctxp = _padded if _padded is not None else self._padded_context(ctx)
        if not x.is_cuda:
            raise _lib.EgoHMRHipError("GlowFlow runs on the HIP kernels only (got a CPU tensor); there is no CPU path")
        B = ctxp.shape[0]
        x = _lib.f32(x, ctxp.device)
        if x.dim() != 3 or x.shape[0] != B or x.shape[2] != FLOW_DIM:
            raise ValueError(f"x {tuple(x.shape)}, expected [{B}, S, {FLOW_DIM}]")
        S = x.shape[1]
        lp, z = self._run(ctxp, x.reshape(B * S, FLOW_DIM), S, sampling=False, keep=keep)
        return lp.reshape(B, S), z.reshape(B, S, FLOW_DIM)

    def forward(self, ctx, num_samples=None, z=None):
        return self.sample_and_log_prob(ctx, num_samples=num_samples, z=z)


class ProHMRScene(ProHMRSceneTransl):
    """``forward_step(train=False)`` of models/prohmr/prohmr_scene.py:100-224: the translation of ``ProHMRSceneTransl`` plus ``num_samples`` bodies
    per image from the flow (``flow.flow``, a ``GlowFlow``), their log-probabilities, the SMPL decode and the projections.  ``smpl``: the
    project's body model (egohmr_amd.smpl.create), a plain attribute - its buffers are not part of the state dict, which is
    ``ProHMRSceneTransl``'s plus ``flow.flow.*``; load with ``egohmr_amd.io.load_stage1_checkpoint(model, path, flow=True)``.

    ``forward(batch, num_samples=4, z=None)``: sample 0 of every item is the mode (z = 0), samples 1 .. S-1 are drawn as
    ``torch.randn(B * (S - 1), 144)`` from the global generator, or ``z`` [B,S,144] is taken as given.  Returns the reference's keys -
    ``pred_cam`` [B,S,3], ``pred_smpl_params`` {global_orient [B,S,1,3,3], body_pose [B,S,23,3,3], betas [B,S,10]}, ``log_prob`` [B,S],
    ``conditioning_feats`` [B,ctx], ``pred_pose_6d`` [B,S,144], ``pred_keypoints_3d`` [B,S,45,3], ``pred_vertices`` [B,S,V,3], ``pred_cam_t``,
    ``pred_cam_t_full`` [B,S,3], ``pred_keypoints_3d_full``, ``pred_keypoints_2d_full``, ``pred_keypoints_2d`` - and, for use where a
    ``ProHMRSceneTransl`` was used, ``pred_cam_full`` [B,3] and ``pred_betas`` [B,10].  The camera and the betas come from FCHead, which reads the
    context only: one row per item, broadcast over the samples, with the bits of ``ProHMRSceneTransl`` on the same weights."""

    def __init__(self, smpl=None, with_focal_length: bool = True, with_bbox_info: bool = True, with_cam_center: bool = True, fx_norm_coeff: float = 1500.0,
                 scene_feat_dim: int = 512, flow_batch_norm: bool = False, device=None):
        super().__init__(with_focal_length, with_bbox_info, with_cam_center, fx_norm_coeff, scene_feat_dim)
        self.flow.flow = GlowFlow(self.context_dim, batch_norm=flow_batch_norm)
        object.__setattr__(self, "smpl", smpl)              # (not a submodule: the state dict keeps the reference's stage-1 names only)
        if device is not None:
            self.to(device)
        self.eval()

    def conditioning(self, img_feats, scene_feats, fx, cam_cx, cam_cy, box_center, box_size):
        """ehm_flow_context: the conditioning row of prohmr_scene.py:111-130, [B, ctx_pad] with a zero pad."""
        dev = img_feats.device
        B = img_feats.shape[0]
        img, scene = _lib.f32(img_feats, dev), _lib.f32(scene_feats, dev)
        if img.shape != (B, IMG_DIM) or scene.shape != (B, self.scene_feat_dim):
            raise ValueError(f"features {tuple(img.shape)} / {tuple(scene.shape)}, expected [B,{IMG_DIM}] / [B,{self.scene_feat_dim}]")
        sc = [_lib.f32(x, dev).reshape(B) for x in (fx, cam_cx, cam_cy, box_size)]
        bc = _lib.f32(box_center, dev).reshape(B, 2)
        out = torch.empty(B, self.flow.flow.ctx_pad, device=dev)
        P = _lib.ptr
        d = _lib.FlowContextDesc(img_feats=P(img), scene_feats=P(scene), fx=P(sc[0]), cam_cx=P(sc[1]), cam_cy=P(sc[2]), box_center=P(bc), box_size=P(sc[3]),
                                 out=P(out), fx_norm=self.fx_norm_coeff, with_cam_center=int(self.with_cam_center), with_bbox_info=int(self.with_bbox_info),
                                 with_focal_length=int(self.with_focal_length), img_dim=IMG_DIM, scene_dim=self.scene_feat_dim,
                                 ctx_pad=self.flow.flow.ctx_pad, B=B)
        with _lib.on_device(dev):
            _lib.api().ehm_flow_context(C.byref(d), _lib.stream_ptr())
        return out

    @torch.no_grad()
    def forward(self, batch, num_samples: int = 4, z=None) -> dict:
        from .geometry import perspective_projection
        if self.smpl is None:
            raise ValueError("ProHMRScene.forward decodes its samples: construct it with smpl=egohmr_amd.smpl.create(...)")
        img_feats, scene_feats = self._encode(batch)
        dev, B = img_feats.device, img_feats.shape[0]
        per_item = [batch[k] for k in ("fx", "cam_cx", "cam_cy", "box_center", "box_size")]
        head = self.head(img_feats, scene_feats, *per_item)
        ctxp = self.conditioning(img_feats, scene_feats, *per_item)
        if z is None:                                                                          # :138-153: the mode and S - 1 draws
            S = int(num_samples)
            if S < 1:
                raise ValueError("num_samples must be at least 1")
            z = torch.zeros(B, S, FLOW_DIM, device=dev)
            if S > 1:
                z[:, 1:] = torch.randn(B * (S - 1), FLOW_DIM, device=dev).reshape(B, S - 1, FLOW_DIM)
        f = self.flow.flow.sample_and_log_prob(None, z=z, _padded=ctxp)
        S = f["z"].shape[1]
        pred_cam = head["pred_cam"].unsqueeze(1).expand(B, S, 3).contiguous()
        betas = head["pred_betas"].unsqueeze(1).expand(B, S, 10).contiguous()
        out = {"pred_cam": pred_cam, "pred_smpl_params": {"global_orient": f["global_orient"], "body_pose": f["body_pose"], "betas": betas},
               "log_prob": f["log_prob"], "conditioning_feats": ctxp[:, :self.context_dim], "pred_pose_6d": f["pred_pose_6d"],
               "pred_cam_full": head["pred_cam_full"], "pred_betas": head["pred_betas"]}
        so = self.smpl(betas=betas.reshape(B * S, 10), body_pose=f["body_pose"].reshape(B * S, 23, 3, 3),
                       global_orient=f["global_orient"].reshape(B * S, 1, 3, 3), pose2rot=False)                   # :166-173
        kp3d = so.joints
        out["pred_keypoints_3d"], out["pred_vertices"] = kp3d.reshape(B, S, -1, 3), so.vertices.reshape(B, S, -1, 3)
        if self.with_focal_length:                                                                                  # :177-185
            fx = _lib.f32(batch["fx"], dev).reshape(B)
            focal = fx.reshape(B, 1, 1).repeat(1, S, 2) * self.fx_norm_coeff
            center = torch.stack([_lib.f32(batch["cam_cx"], dev).reshape(B), _lib.f32(batch["cam_cy"], dev).reshape(B)], -1).unsqueeze(1).repeat(1, S, 1)
        else:
            focal = 5000.0 * torch.ones(B, S, 2, device=dev)                                                        # cfg.EXTRA.FOCAL_LENGTH
            center = torch.tensor([[[960.0, 540.0]]], device=dev).repeat(B, S, 1)
        cam_t = torch.stack([pred_cam[:, :, 1], pred_cam[:, :, 2], 2 * focal[:, :, 0] / (CROP_RES * pred_cam[:, :, 0] + 1e-9)], dim=-1)   # :187-190
        out["pred_cam_t"] = cam_t
        cam_t_full = head["pred_cam_full"].unsqueeze(1).expand(B, S, 3).contiguous()                               # :196-202 (one camera per item)
        out["pred_cam_t_full"] = cam_t_full
        out["pred_keypoints_3d_full"] = out["pred_keypoints_3d"] + cam_t_full.unsqueeze(2)                          # :203-204
        k2f = perspective_projection(kp3d, translation=cam_t_full.reshape(-1, 3), camera_center=center.reshape(-1, 2), focal_length=focal.reshape(-1, 2))
        k2f = torch.stack([k2f[:, :, 0] / 1920 - 0.5, k2f[:, :, 1] / 1080 - 0.5], dim=-1)                           # :211-212
        out["pred_keypoints_2d_full"] = k2f.reshape(B, S, -1, 2)
        k2 = perspective_projection(kp3d, translation=cam_t.reshape(-1, 3), focal_length=focal.reshape(-1, 2)) / CROP_RES   # :218-222
        out["pred_keypoints_2d"] = k2.reshape(B, S, -1, 2)
        return out

    def log_prob(self, smpl_params, conditioning_feats):
        """models/prohmr/smpl_flow.py:31-50: (log_prob [B,N], z [B,N,144]) of ``smpl_params`` {global_orient [B,N,6], body_pose [B,N,138]} (the
        6-D poses the flow models) given ``conditioning_feats`` [B,ctx].  Differentiable where ``GlowFlow.log_prob`` is (torch.cat carries the
        gradient of the 6-D poses on)."""
        x = torch.cat((smpl_params["global_orient"], smpl_params["body_pose"]), dim=-1)
        return self.flow.flow.log_prob(x, conditioning_feats)
