"""Step-invariant conditioning encoders (run once per item, SURVEY.md section 0 finding 2).

The reference re-evaluates both inside every denoising step (models/egohmr/egohmr.py:183,:214);
neither depends on x_t or t, so the build evaluates them once per sampled batch.  Both run on the
hand-written split-f16 matrix-core kernels (csrc/conv.hip: the 52 bottleneck convolutions of ResNet-50
as NHWC implicit GEMMs with BatchNorm folded; csrc/linear.hip: the scene PointNet's GEMMs with the
max-pool fused; csrc/stem.hip: the 7x7 stem + ReLU + max-pool as one vector-ALU kernel).  Sub-module and
parameter names follow the reference so its checkpoints load (``backbone.*`` models/resnet.py:97-136,
``scene_enc.*`` models/respointnet.py:13-27).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib, trunk_grad
from .split_gemm import pack_weight


# measurement hook (tools/exp_encoder_precision.py): called with every X2 activation buffer an encoder kernel has just written, (buffer, channels).
# None on the product path.
_x2_debug_hook = None


class _Bottleneck(nn.Module):
    def __init__(self, cin, width, stride, project):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, width * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(width * 4)
        self.downsample = None
        if project:
            self.downsample = nn.Sequential(nn.Conv2d(cin, width * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(width * 4))

    def forward(self, x):
        raise _lib.EgoHMRHipError("_Bottleneck is a parameter container: the arithmetic runs in ResNet50Features.folded() (csrc/conv.hip); "
                                  "egohmr_amd has no eager / CPU route (tools/_eager.py holds the eager yardstick)")


class ResNet50Features(nn.Module):
    """models/resnet.py:139-150: ResNet-50 trunk, global average pool -> [B,2048]."""

    hi_only = False      # True: the plain-f16 tier of the trunk (ehm_conv_x2_desc.hi_only: hi halves only, one MFMA per product) - NOT parity grade
    # True: a call with grad mode on and a parameter that requires grad runs behind trunk_grad.TrunkFunction - the same launches, every conv's X2 output
    # kept for the backward (about 9 M values per 224 x 224 image) - and its backward fills the parameters' gradients (BatchNorm in eval mode: the
    # statistics stay frozen, conv weights and affine parameters train).  False: every call is the no-graph route, whatever the parameters say
    grad_params = False
    # True: a call under .train() (self.training) runs every BatchNorm2d on BATCH statistics (csrc/bn2d_train.hip): mean and biased variance over the
    # N H W rows of the conv's raw output, the running statistics updated in place as nn.BatchNorm2d updates them, and - behind grad_params, with a
    # graph - trunk_grad.TrunkTrainFunction, whose backward differentiates through the mean and the variance.  False: .train() is ignored, every call
    # folds the frozen running statistics
    train_batchnorm = False
    # A dist.StatSync, set for a call by EgoHMR.training_step behind EgoHMR.data_parallel: the train-mode route's BatchNorm2d statistics and their backward
    # sums then run over ALL ranks' rows (one all-gather per BatchNorm each way, also under no_grad - the running statistics still move).  None: this
    # process's rows, today's calls
    stat_sync = None
    GRAD_HI_ONLY = ("the autograd route of ResNet50Features keeps f32-grade activations for its backward; the plain-f16 tier "
                    "(ResNet50Features.hi_only = True) stores none: set hi_only = False with it")
    GRAD_IMAGE = ("ResNet50Features.grad_params differentiates the trunk with respect to its parameters only: the image gradient (the stem's data "
                  "gradient) is not built, so the input must not require grad")

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for i, (width, n, stride) in enumerate([(64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)], 1):
            blocks = []
            for b in range(n):
                blocks.append(_Bottleneck(cin, width, stride if b == 0 else 1, project=(b == 0)))
                cin = width * 4
            setattr(self, f"layer{i}", nn.Sequential(*blocks))
        self._fold_key_fn = self._fold_key = self._fold_fn = None      # current()
        self._sk_host = self._sk_event = self._sk_ws_checked = None    # _sk_status_async / check_status

    def current(self):
        """folded() for the weights as they are now: rebuilt when a parameter / buffer changes (storage or version counter)."""
        if self._fold_key_fn is None:
            self._fold_key_fn = _lib.TensorKey(self)
        key = self._fold_key_fn()
        if self._fold_key != key:
            self._fold_fn, self._fold_key = self.folded(), key
        return self._fold_fn

    def forward(self, x):
        """The module call IS the HIP path (models/resnet.py:139-150 in eval mode); there is no eager route.  With `grad_params`, grad mode on and a
        parameter that requires grad the result carries a grad_fn (trunk_grad.TrunkFunction: same launches, same bits, activations kept)."""
        train = self.train_batchnorm and self.training
        if self.grad_params and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if self.hi_only:
                raise _lib.EgoHMRHipError(self.GRAD_HI_ONLY)
            if x.requires_grad:
                raise NotImplementedError(self.GRAD_IMAGE)
            if train:
                self._check_train(x)
                return trunk_grad.TrunkTrainFunction.apply(self, x, *self.parameters())
            return trunk_grad.TrunkFunction.apply(self, x, *self.parameters())
        if train:
            self._check_train(x)
            return self.folded(train=True)(x)
        return self.current()(x)

    def _check_train(self, x):
        """What the train-mode BatchNorm route cannot run, refused before any device call: a BatchNorm2d without a fixed momentum or without running
        statistics (NotImplementedError, as ModulatedGCN refuses them) and a batch that leaves a BatchNorm2d fewer than two values per channel
        (ValueError, as torch raises it: layer4 has N * H/32 * W/32 rows)."""
        for bn in self.modules():
            if isinstance(bn, nn.BatchNorm2d) and (bn.momentum is None or not bn.track_running_stats):
                raise NotImplementedError("ResNet50Features: the train-mode route updates the running statistics with a fixed momentum; "
                                          "BatchNorm2d(momentum=None) and track_running_stats=False are not built")
        items = x.shape[0] if self.stat_sync is None else self.stat_sync.total             # (data parallel: the statistics see every rank's rows)
        if x.dim() == 4 and items * (x.shape[2] // 32) * (x.shape[3] // 32) < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)} "
                             "(layer4 of the trunk has N * H/32 * W/32 values per channel)")

    # ------------------------------------------------------------------ stream-K hand-off time-outs (csrc/conv.hip): made loud, never waited for
    def _sk_status_async(self, ws):
        """Behind a trunk pass: a stream-ordered copy of the workspace's time-out count to pinned memory + an event.  An earlier pass's word
        that has arrived is looked at first (no host wait on the product path)."""
        if ws is None:                                     # (no conv of this pass had a stream-K plan)
            return
        if self._sk_event is not None and self._sk_event.query():
            self.check_status()
        if self._sk_host is None:
            self._sk_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        _lib.api().ehm_conv_x2_workspace_status(ws, self._sk_host.data_ptr(), _lib.stream_ptr())
        self._sk_event = torch.cuda.Event()
        self._sk_event.record()
        self._sk_ws_checked = ws

    def check_status(self):
        """Raise if a stream-K conv of an earlier trunk pass timed out waiting for a partner block's partial sums (its tiles are NaN and the
        workspace's counters poisoned); the workspace is zeroed again by the call, so the next pass is clean.  Waits for that pass."""
        if self._sk_event is None:
            return
        self._sk_event.synchronize()
        self._sk_event = None
        if int(self._sk_host[0]) != 0:
            self._sk_host.zero_()
            ws = self._sk_ws_checked
            with torch.cuda.device(ws.device):
                _lib.api().ehm_conv_x2_workspace_status(ws, None, _lib.stream_ptr())

    # ------------------------------------------------------------------ inference form: BatchNorm folded into the convolutions
    def folded(self, x2_activations: bool = True, fuse_shortcut: bool = True, train: bool = False):
        """Eval-mode ResNet-50 on the matrix cores with every BatchNorm2d folded into its convolution: a FoldedTrunk (below) for the weights as they are."""
        return FoldedTrunk(self, x2_activations, fuse_shortcut, train)


class ConvPack(NamedTuple):
    """A conv's packed launch operand (pack_conv).  Ci2 / stride2: the input channels and the stride of the projection shortcut where the pack holds a
    bottleneck's last conv AND its projection as one matrix; zero otherwise."""
    buf: torch.Tensor               # X2 [Co padded to 128, KH*KW*Ci (+ Ci2)], tap-major, times `scale`
    scale: float
    bias: torch.Tensor              # float32 [Co]
    Co: int
    Ci: int
    KH: int
    KW: int
    stride: int
    pad: int
    Ci2: int = 0
    stride2: int = 0

    def out_hw(self, H, W):
        return (H + 2 * self.pad - self.KH) // self.stride + 1, (W + 2 * self.pad - self.KW) // self.stride + 1


def pack_conv(p, ds=None):
    """A unit's operands (w' [Co,Ci,KH,KW], b', stride, padding) -> ConvPack: the weight tap-major [Co, KH*KW*Ci] through split_gemm.pack_weight.
    ds: the operands of the block's projection shortcut - then p is the bottleneck's last conv and both (1 x 1) go into ONE matrix [Co, Ci + Ci_in]
    with a common scale and the summed bias."""
    w, b, stride, pad = p
    Co, Ci, KH, KW = w.shape
    w2 = w.permute(0, 2, 3, 1).reshape(Co, KH * KW * Ci)
    if ds is None:
        packed = pack_weight(w2)
        return ConvPack(packed.buf, packed.scale, b.contiguous(), Co, Ci, KH, KW, stride[0], pad[0])
    wd = ds[0]
    assert (KH, KW) == (1, 1) and wd.shape[2:] == (1, 1) and wd.shape[0] == Co and Co % 128 == 0
    packed = pack_weight(torch.cat([w2, wd.reshape(Co, -1)], dim=1))
    return ConvPack(packed.buf, packed.scale, (b.double() + ds[1].double()).float().contiguous(), Co, Ci, 1, 1, stride[0], pad[0], wd.shape[1], ds[2][0])


def x2_buffer(pixels, ch, dev, clear_last=False):
    """X2 activation matrix for ehm_conv_x2: pixels rounded up to the row tile + one all-zero row (out-of-image taps read it; ehm_conv_x2 clears it
    in its output, the stem's buffer is cleared here)"""
    rows = int(_lib.api().ehm_conv_x2_rows(pixels))
    buf = torch.empty(rows, ch, device=dev)                                         # X2 rows have the byte size of float rows
    if clear_last:
        buf[rows - 1].zero_()
    return buf


def _operands(conv, bn, stats=None):
    """a unit's launch operands: trunk_grad.fold's (w', b') in float32, the conv's stride and padding"""
    w, b = trunk_grad.fold(conv, bn, stats)
    return w.float(), b.float(), conv.stride, conv.padding


class _FoldedUnits:
    """The eval provider of FoldedTrunk's walk: the operands folded once by the trunk, their packed form kept under the unit's index."""

    def __init__(self, trunk, x, rec):
        self.trunk = trunk

    def stem(self, x):
        return self.trunk.stem_wt, self.trunk.stem_b

    def unit(self, i, x, shp):
        return self.trunk.ops[i], i

    def finish(self):
        pass


class _BatchUnits:
    """The train provider of FoldedTrunk's walk; nothing is kept between calls.  Per (conv, BatchNorm2d) unit: the RAW conv output z on the same launch
    (unfolded weight through the same pack, zero bias, no ReLU, no residual; a projection block's conv3 and downsample apart - each BatchNorm has its
    own statistics), its mean / biased variance / invstd and the running-statistics update (ehm_bn2d_train_stats), then the operands folded on the
    float32 batch statistics: the output has the bits of an eval-mode call whose running statistics are that batch's.
    rec: a trunk_grad.TrainRecord that receives what the backward needs (bn: per unit of trunk_grad.units (z or None, z's shape, mean, var, invstd),
    None for an identity block's absent downsample; the stem's operands), or None."""

    def __init__(self, trunk, x, rec):
        self.trunk, self.rec, self.sync, self.bumped = trunk, rec, trunk.module.stat_sync, []
        self.zero = torch.zeros(2048, device=x.device)
        sync = self.sync
        if sync is not None and sync.counts[sync.rank] != x.shape[0]:
            raise ValueError(f"ResNet50Features.stat_sync counts {sync.counts[sync.rank]} items for this rank, the input has {x.shape[0]}")
        if rec is not None:
            rec.bn = [None] * len(trunk.units)
            rec.sync = sync

    def note(self, i, *e):
        self.bumped.append(self.trunk.units[i][1])
        if self.rec is not None:
            self.rec.bn[i] = e

    def stem(self, x):
        N, _, H, W = x.shape
        conv, bn = self.trunk.units[0]
        raw_wt, _ = trunk_grad.stem_operands(conv.weight.detach().float(), self.zero[:64])
        z = trunk_grad.stem_preact(x, raw_wt, self.zero[:64])
        mean, var, invstd = trunk_grad.bn_stats(z, N * (H // 2) * (W // 2), 64, bn, x2=False, sync=self.sync)
        del z                                                                       # (recomputed by the backward, like the eval route's)
        self.note(0, None, (N, H // 2, W // 2), mean, var, invstd)
        wt, b = trunk_grad.stem_operands(*_operands(conv, bn, (mean, var))[:2])
        if self.rec is not None:
            self.rec.stem_wt, self.rec.stem_b = wt, b
        return wt, b

    def unit(self, i, x, shp):
        conv, bn = self.trunk.units[i]
        Co, rec = conv.out_channels, self.rec
        z, zs = self.trunk.conv_x2(x, shp, (conv.weight.detach().float(), self.zero[:Co], conv.stride, conv.padding), None, relu=False)
        mean, var, invstd = trunk_grad.bn_stats(z, zs[0] * zs[1] * zs[2], Co, bn, sync=self.sync)
        self.note(i, z if rec is not None and rec.keep_z else None, zs, mean, var, invstd)
        return _operands(conv, bn, (mean, var)), None

    def finish(self):
        """the kernels wrote the buffers through their pointers: tell torch (current() refolds on the next eval call)"""
        for bn in self.bumped:
            for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked):
                torch.autograd.graph.increment_version(t)


class FoldedTrunk:
    """What ResNet50Features.folded() returns: the trunk on HIP tensors (there is no eager / library-convolution route), every BatchNorm2d folded into
    its convolution (trunk_grad.fold: w' = w * g/sqrt(v+eps), b' = beta - mean * g/sqrt(v+eps); exact up to float re-association).
    x2_activations=True (the product path): the activations stay in the X2 split format from the stem to the average pool (ehm_conv_x2), ONE walk over
    trunk_grad.units (_walk_x2) whose operand provider says where a unit's (w', b', stride, padding) come from: _FoldedUnits (eval: folded here, once,
    packed on first use) or _BatchUnits (train=True, ResNet50Features.train_batchnorm: folded per call on the batch's statistics, nothing kept).
    x2_activations=False: float32 NHWC activations between the convolutions (ehm_conv_nhwc_split - the kernel the non-local GCN block also uses; kept
    as a second implementation the tests compare)."""

    def __init__(self, module, x2_activations=True, fuse_shortcut=True, train=False):
        self.module, self.x2_activations, self.fuse_shortcut, self.train = module, x2_activations, fuse_shortcut, train
        self.units = trunk_grad.units(module)
        with torch.no_grad():
            self.ops = [] if train else [None if u is None else _operands(*u) for u in self.units]
            # the folded parameters as trunk_grad reads them: (w', b', stride, padding) of the stem; of conv1, conv2, conv3, downsample (or None) per block
            self.stem, self.blocks = (self.ops[0], [tuple(self.ops[i:i + 4]) for i in range(1, len(self.ops), 4)]) if self.ops else (None, [])
            self.stem_wt, self.stem_b = trunk_grad.stem_operands(*self.stem[:2]) if self.ops else (None, None)
        self.packs = {}                                    # the eval operands' packed form: unit index -> ConvPack, ("dual", conv3's index) -> conv3 + projection
        self.dgrad = {}                                    # unit index -> the data gradient's pack (trunk_grad's eval-mode backward fills it)
        self.sk_ws = {}                                    # device -> scratch of the stream-K convs (one conv at a time on a stream), zeroed ONCE

    def __call__(self, x, saved=None, *, rec=None):
        """x [N,3,H,W] -> [N,2048].  saved: a list that receives (X2 buffer, (N, H, W)) of the stem's and of every conv's output in launch order
        instead of letting them go.  rec (train route): a trunk_grad.TrainRecord; its `acts` is that list."""
        if not (saved is None or isinstance(saved, list)) or (rec is not None and not self.train):
            raise TypeError("FoldedTrunk(x, saved, rec=): `saved` is a list, and a trunk_grad.TrainRecord goes in as `rec` on the train route")
        if not x.is_cuda:
            raise _lib.EgoHMRHipError("the ResNet-50 backbone needs its input on a HIP device; egohmr_amd has no CPU path")
        x = _lib.f32(x)
        if x.shape[1] != 3 or x.shape[2] % 32 or x.shape[3] % 32:
            raise _lib.EgoHMRHipError(f"the fused stem needs [N,3,H,W] images with H, W multiples of 32 (the reference feeds 224 x 224 crops); got {tuple(x.shape)}")
        with _lib.on_device(x.device):                                              # the library launches on the CURRENT device's stream
            if self.train:
                with torch.no_grad():
                    return self._walk_x2(x, saved, rec)
            return self._walk_x2(x, saved, rec) if self.x2_activations else self._walk_nhwc(x)

    def _packed(self, key, p, ds=None):
        """pack_conv(p, ds), kept under `key` (with ds: ("dual", key)); key None (the train route's per-call operands): not kept"""
        if key is None:
            return pack_conv(p, ds)
        key = key if ds is None else ("dual", key)
        if key not in self.packs:
            self.packs[key] = pack_conv(p, ds)
        return self.packs[key]

    def stem_launch(self, x, wt, b, x2=False):
        """conv1 + bn1 + relu + maxpool in one pass, NCHW in -> NHWC out (csrc/stem.hip); x2: output in the X2 split format"""
        A = _lib.api()
        N, _, H, W = x.shape
        if wt.device != x.device:
            raise _lib.EgoHMRHipError("ResNet50Features.folded(): weights and input live on different devices")
        scratch = torch.empty(A.ehm_resnet_stem_scratch_bytes(N, H, W) // 4, device=x.device)
        y = x2_buffer(N * (H // 4) * (W // 4), 64, x.device, clear_last=True) if x2 else torch.empty(N, H // 4, W // 4, 64, device=x.device)
        A.ehm_resnet_stem(x, wt, b, scratch, y, N, H, W, 1 if x2 else 0, _lib.stream_ptr())
        if x2 and _x2_debug_hook is not None:
            _x2_debug_hook(y, 64)
        return y

    def conv_nhwc(self, x, i, res=None, relu=True):
        """unit i on float32 NHWC activations (ehm_conv_nhwc_split)"""
        k, P = self._packed(i, self.ops[i]), _lib.ptr
        N, H, W, _ = x.shape
        y = torch.empty(N, *k.out_hw(H, W), k.Co, device=x.device)
        d = _lib.ConvDesc(P(x), P(k.buf), P(k.bias), P(res), P(y), N, H, W, k.Ci, k.Co, k.KH, k.KW, k.stride, k.pad, 1 if relu else 0, k.scale)
        _lib.api().ehm_conv_nhwc_split(C.byref(d), _lib.stream_ptr())
        return y

    def conv_x2(self, x, shape, p, key, res=None, relu=True, shortcut=None):
        """one bottleneck conv on X2 activations (csrc/conv.hip conv_x2_tile_kernel); shape = (N, H, W) of x; p: the unit's operands, key: what
        their packed form is cached under (_packed).
        shortcut = (block input, its shape, folded downsample): the projection shortcut accumulates inside this conv (second K segment)."""
        A, P = _lib.api(), _lib.ptr
        N, H, W = shape
        k = self._packed(key, p, None if shortcut is None else shortcut[2])
        Ho, Wo = k.out_hw(H, W)
        y = x2_buffer(N * Ho * Wo, k.Co, x.device)
        d = _lib.ConvX2Desc(P(x), x.shape[0], P(k.buf), P(k.bias), P(res), P(y), N, H, W, k.Ci, k.Co, k.KH, k.KW, k.stride, k.pad, 1 if relu else 0,
                            k.scale, None, 0)
        d.hi_only = int(bool(self.module.hi_only))                                  # the plain-f16 tier (EgoHMR.encoder_precision = 'f16'): NOT parity grade
        if shortcut is not None:
            x_in, (_, H2, W2) = shortcut[0], shortcut[1]
            d.x2, d.x2_rows, d.H2, d.W2, d.Ci2, d.stride2 = P(x_in), x_in.shape[0], H2, W2, k.Ci2, k.stride2
        need = int(A.ehm_conv_x2_workspace_bytes(C.byref(d)))                       # stream-K scratch (layers 3 / 4: tile counts that straddle the block slots)
        if need:
            ws = self.sk_ws.get(str(x.device))
            if ws is None or ws.numel() < need:
                ws = self.sk_ws[str(x.device)] = torch.zeros(need, dtype=torch.uint8, device=x.device)
            d.workspace, d.workspace_bytes, d.workspace_clean = P(ws), ws.numel(), 1
        A.ehm_conv_x2(C.byref(d), _lib.stream_ptr())
        if _x2_debug_hook is not None:
            _x2_debug_hook(y, k.Co)
        return y, (N, Ho, Wo)

    def _walk_x2(self, x, saved, rec):
        """the whole trunk with the activations in the X2 split format between the layers (taps gathered by the LDS DMA)"""
        U, conv, m = self.units, self.conv_x2, self.module
        N = x.shape[0]
        shp = (N, x.shape[2] // 4, x.shape[3] // 4)
        acts = saved if rec is None else rec.acts
        keep = (lambda *e: None) if acts is None else (lambda *e: acts.append(e))
        units = (_BatchUnits if self.train else _FoldedUnits)(self, x, rec)
        wt, b = units.stem(x)
        x = self.stem_launch(x, wt, b, x2=True)
        keep(x, shp)
        for i1 in range(1, len(U), 4):
            i2, i3, id_ = i1 + 1, i1 + 2, i1 + 3
            y, s1 = conv(x, shp, *units.unit(i1, x, shp))
            keep(y, s1)
            y, s2 = conv(y, s1, *units.unit(i2, y, s1))
            keep(y, s2)
            p3, k3 = units.unit(i3, y, s2)
            if U[id_] is None:
                x, shp = conv(y, s2, p3, k3, res=x)
            else:
                pd, kd = units.unit(id_, x, shp)
                if self.fuse_shortcut:
                    x, shp = conv(y, s2, p3, k3, shortcut=(x, shp, pd))             # out = conv3(.) + downsample(x) in one launch: no shortcut tensor
                else:
                    x, shp = conv(y, s2, p3, k3, res=conv(x, shp, pd, kd, relu=False)[0])
            keep(x, shp)
        out = torch.empty(N, x.shape[1], device=x.device)
        _lib.api().ehm_x2_group_mean(x, out, N, shp[1] * shp[2], x.shape[1], int(bool(m.hi_only)), _lib.stream_ptr())
        m._sk_status_async(self.sk_ws.get(str(x.device)))
        units.finish()
        return out

    def _walk_nhwc(self, x):
        """the second implementation: float32 NHWC activations from the stem on"""
        U, conv = self.units, self.conv_nhwc
        x = self.stem_launch(x, self.stem_wt, self.stem_b)
        for i1 in range(1, len(U), 4):
            y = conv(conv(x, i1), i1 + 1)
            x = conv(y, i1 + 2, res=x if U[i1 + 3] is None else conv(x, i1 + 3, relu=False))
        return x.mean(dim=(1, 2))


class _ResBlockFC(nn.Module):
    def __init__(self, cin, cout, hidden):
        super().__init__()
        self.fc_0 = nn.Linear(cin, hidden)
        self.fc_1 = nn.Linear(hidden, cout)
        self.shortcut = nn.Linear(cin, cout, bias=False)

    def forward(self, x):
        raise _lib.EgoHMRHipError("_ResBlockFC is a parameter container: ResnetPointnet.forward runs the block on the HIP kernels (csrc/linear.hip)")


class ResnetPointnet(nn.Module):
    """models/respointnet.py:33-59: per-point MLP with three global max-pool-concat stages -> [B,out_dim].

    Parameters keep the reference's names; the arithmetic runs on the split-f16 matrix-core kernels of
    csrc/linear.hip (f32-grade, see docs/EXPERIMENTS.md 3.3) with the per-body constant half of every block input folded
    into bias vectors, fc_1 + shortcut fused into one dual-source GEMM and the max-pool fused into its epilogue."""

    hi_only = False      # True: the plain-f16 tier (ehm_linear_desc.hi_only) - NOT parity grade
    # False: an autograd call (grad mode on, p.requires_grad) differentiates w.r.t. p only and leaves the parameters' .grad alone; True: the backward
    # also fills the 24 parameters' gradients (grad_parameters()).  Calls with no gradient to compute run the chained route either way.
    grad_params = False
    GRAD_HI_ONLY = ("the autograd route of ResnetPointnet.forward keeps f32-grade activations for its backward; the plain-f16 tier "
                    "(ResnetPointnet.hi_only = True) stores none: set hi_only = False with it")

    def __init__(self, out_dim=512, hidden_dim=256):
        super().__init__()
        self.hidden_dim = hidden_dim
        self.fc_pos_0 = nn.Linear(3, 2 * hidden_dim)
        for b in range(4):
            setattr(self, f"block_{b}", _ResBlockFC(2 * hidden_dim, hidden_dim, hidden_dim))
        self.fc_c = nn.Linear(hidden_dim, out_dim)
        self._packed = self._packed_key = self._tkey = None
        self._grad_packed = self._grad_packed_key = None                                 # pointnet_grad._weights

    def grad_parameters(self):
        """The parameters the autograd route delivers gradients to with `grad_params`, in the order of its backward (pointnet_grad.PARAM_NAMES)."""
        from .pointnet_grad import PARAM_NAMES
        return [self.get_parameter(n) for n in PARAM_NAMES]

    def _wants_grad(self, p):
        return torch.is_grad_enabled() and (p.requires_grad or (self.grad_params and any(q.requires_grad for q in self.grad_parameters())))

    # ------------------------------------------------------------------ weight preparation (once per weight version)
    @staticmethod
    def _pack(w64: torch.Tensor, device):
        """float64 [N,K] -> (X2 buffer, power-of-two scale); K padded to a multiple of 32.  Its scale rule is not split_gemm.weight_scale (at
        amax = 1.5 it gives 2048, that one 1024): unifying them would change the forward's bits."""
        w = w64.float().contiguous().to(device)
        N, K = w.shape
        Kp = (K + 31) // 32 * 32
        amax = float(w.abs().max())
        scale = 2.0 ** (12 - int(np.floor(np.log2(amax)) + 1)) if amax > 0 else 1.0
        buf = torch.empty(N, Kp, dtype=torch.float32, device=device)         # X2 has the byte size of float32 [N,Kp]
        _lib.api().ehm_split_pack(w, buf, N, K, Kp, scale, _lib.stream_ptr())
        return buf, scale, w

    def _prepare(self, device):
        if self._tkey is None:
            self._tkey = _lib.TensorKey(self)
        key = self._tkey() + (str(device),)
        if self._packed is not None and self._packed_key == key:
            return self._packed
        H = self.hidden_dim
        d = lambda t: t.detach().double()
        P = {"pos_w4": torch.cat([self.fc_pos_0.weight.detach().float(), self.fc_pos_0.bias.detach().float()[:, None]], 1).contiguous()}   # rows (w_x, w_y, w_z, bias)
        blocks = [self.block_0, self.block_1, self.block_2, self.block_3]
        b0 = blocks[0]
        P["g1_0"] = self._pack(d(b0.fc_0.weight), device) + (b0.fc_0.bias.detach().float().contiguous(),)
        s_pos = d(b0.shortcut.weight) @ d(self.fc_pos_0.weight)                          # shortcut(fc_pos(p)) folded: [H,3]
        w = torch.cat([d(b0.fc_1.weight), torch.cat([s_pos, s_pos.new_zeros(H, 29)], 1)], dim=1)   # [H, H+32]
        P["g3_0"] = self._pack(w, device) + ((d(b0.fc_1.bias) + d(b0.shortcut.weight) @ d(self.fc_pos_0.bias)).float().contiguous(),)
        for i in (1, 2, 3):
            bl = blocks[i]
            W0, S = d(bl.fc_0.weight), d(bl.shortcut.weight)
            P[f"g1_{i}"] = self._pack(W0[:, :H], device)
            P[f"g3_{i}"] = self._pack(torch.cat([d(bl.fc_1.weight), S[:, :H]], dim=1), device) + (bl.fc_1.bias.detach().float().contiguous(),)
            # pooled halves: per-body bias vectors [relu(pooled) . W0b^T + b0 | pooled . Sb^T], [B,H] x [H,2H] in exact float32 and ONE launch
            # (ehm_skinny_gemm_f32 wants W as [K,N]; its `relu` argument rectifies the input for the first H output columns)
            P[f"wvsT_{i}"] = torch.cat([W0[:, H:].t(), S[:, H:].t()], dim=1).float().contiguous().to(device)
            b0v = bl.fc_0.bias.detach().float()
            P[f"bvs_{i}"] = torch.cat([b0v, torch.zeros_like(b0v)]).contiguous().to(device)
        P["fc_cT"], P["fc_cb"] = d(self.fc_c.weight).t().float().contiguous().to(device), self.fc_c.bias.detach().float().contiguous().to(device)
        self._packed, self._packed_key = P, key
        return P

    def forward(self, p):
        """With grad mode on and p.requires_grad - or `grad_params` set and a parameter that requires grad - the result carries a grad_fn: the same
        launches, every block's relu(h) and net kept for the backward (pointnet_grad.PointnetFunction).  Every other call: the ping-pong route."""
        if not p.is_cuda:
            raise _lib.EgoHMRHipError("ResnetPointnet runs on the HIP kernels only (got a CPU tensor); there is no CPU path")
        if self._wants_grad(p):
            if self.hi_only:
                raise _lib.EgoHMRHipError(self.GRAD_HI_ONLY)
            from . import pointnet_grad
            return pointnet_grad.PointnetFunction.apply(self, p, *(self.grad_parameters() if self.grad_params else ()))
        with torch.no_grad(), _lib.on_device(p.device):                                  # the library launches on the CURRENT device's stream
            return self._forward_on_device(p)

    def _forward_on_device(self, p, save=False):
        """save: keep what the backward reads instead of ping-ponging it - every block's relu(h) and net (the last block's net is stored too) - and
        return (out, saved).  The launches and their descriptors are the same otherwise: the output has the same bits."""
        A, P_, dev, H = _lib.api(), _lib.ptr, p.device, self.hidden_dim
        P = self._prepare(dev)
        p = _lib.f32(p)
        B, N, _ = p.shape
        Np = (N + 191) // 192 * 192                                                      # row tile of csrc/linear.hip
        M = B * Np
        st = _lib.stream_ptr()
        f32buf = lambda cols: torch.empty(M, cols, dtype=torch.float32, device=dev)      # X2 buffers (same bytes as float32)
        P32, Hb, netA = f32buf(32), f32buf(H), f32buf(H)
        netB = f32buf(H) if not save else None
        rhs, nets = [Hb], [netA]                                                         # (save) the blocks' relu(h) and net
        p = p.contiguous()
        A.ehm_pointnet_lift(p, None, None, None, P32, B, N, Np, 2 * H, st)

        def gemm(A0, K0, A1, K1, W, bias, gbias, Y, colmax, relu_in0, relu_out, lift=False):
            """gbias: (per-body bias matrix [B, 2H], first column of this GEMM's H columns) or None"""
            d = _lib.LinearDesc(A0=P_(A0), A1=P_(A1), W=P_(W[0]), lift_points=P_(p) if lift else None, lift_W4=P_(P["pos_w4"]) if lift else None,
                                bias=P_(bias), group_bias=P_(gbias[0]) + 4 * gbias[1] if gbias else None, Y=P_(Y), colmax=P_(colmax),
                                M=M, N=H, K0=K0, K1=K1, rows_per_group=Np, valid_rows_per_group=N, relu_in0=int(relu_in0),
                                relu_out=int(relu_out), w_scale=W[1], hi_only=int(bool(self.hi_only)), group_bias_stride=gbias[0].shape[1] if gbias else 0)
            A.ehm_linear_split(d, st)
            if Y is not None and _x2_debug_hook is not None:
                _x2_debug_hook(Y, H)

        def small(x, Wt, bias, relu_in_cols=0):
            """[B,K] x [K,N] (+ bias) in exact float32: the per-body vectors between the big GEMMs.  The BLAS ran each of these
            256 x 256 x 256 products as one 256 x 256 workgroup (170 - 450 us, on the PointNet's critical path).
            relu_in_cols: the first that many output columns see relu(x)."""
            y = torch.empty(x.shape[0], Wt.shape[1], device=dev)
            A.ehm_skinny_gemm_f32(x, Wt, bias, y, x.shape[0], Wt.shape[0], Wt.shape[1], relu_in_cols << 1, st)
            return y

        neg_inf = float("-inf")
        # block_0 on net0 = fc_pos(p):  h = fc_0(relu(net0));  net1 = fc_1(relu(h)) + shortcut(net0)
        # (relu(net0) is produced inside the GEMM's loader from the 12 bytes of each point: ehm_linear_desc.lift_points)
        gemm(None, 2 * H, None, 0, P["g1_0"], P["g1_0"][3], None, Hb, None, False, True, lift=True)
        pooled_all = torch.full((4, B, H), neg_inf, device=dev)                         # the four column maxima, cleared by one launch
        pooled = pooled_all[0]
        gemm(Hb, H, P32, 32, P["g3_0"], P["g3_0"][3], None, netA, pooled, False, False)
        cur, nxt = netA, netB
        for i in (1, 2, 3):
            # pooled halves of fc_0(relu(cat[net, pooled])) and of shortcut(cat[net, pooled]): one launch, [B, 2H]
            vs = small(pooled, P[f"wvsT_{i}"], P[f"bvs_{i}"], relu_in_cols=H)
            if save:
                Hb, nxt = f32buf(H), f32buf(H)
                rhs.append(Hb)
                nets.append(nxt)
            gemm(cur, H, None, 0, P[f"g1_{i}"], None, (vs, 0), Hb, None, True, True)
            pooled = pooled_all[i]
            gemm(Hb, H, cur, H, P[f"g3_{i}"], P[f"g3_{i}"][3], (vs, H), nxt if (i < 3 or save) else None, pooled, False, False)
            cur, nxt = nxt, cur
        out = small(pooled, P["fc_cT"], P["fc_cb"], relu_in_cols=P["fc_cT"].shape[1])
        if save:
            return out, dict(p=p, B=B, N=N, Np=Np, rh=rhs, net=nets, pooled=pooled_all, arg=None)
        return out

