"""Shared ResNet + FPN trunk of the one-stage detectors (RetinaNet, FCOS) on the HIP path.

Same protocol as the reference's BaseNet (models/base_net.py:50-71): ``model(batch)`` in training mode returns
``{"total_loss", "cls_loss", "reg_loss"}``; the batch dict is the collator contract
(data/collators/pad_collator.py:38-49): ``data`` (N,3,H,W), ``gt_boxes`` (N,G,5), ``im_info`` (N,5).
There is no autograd: ``get_losses`` runs the forward kernels and the fused loss fwd+bwd kernels, ``backward()``
runs the explicit dgrad/wgrad schedule in reverse order and leaves fp32 gradients in the parameter arena.

Gradient convention: the gradient buffer of a post-ReLU activation T holds dL/d(pre-activation) (already masked
by T > 0).  When T has several consumers, all but the last dgrad accumulate unmasked and the last one applies the
mask in its epilogue -- so ReLU backward, residual fan-in and FrozenBN never cost a separate pass over HBM.
"""
import math

import numpy as np
import torch

from .. import ops
from ..data.raw import AffineImageBatch, RawImageBatch
from ..ops import Geom
from ..streams import SideStreams, fork, join
from . import params as P
from .. import comm as _comm
from .engine import ConvLayer, DeconvLayer, FCLayer, HostToDevice, ParamArena, TrainableStem
from .fp8_scaling import Fp8GradScaler, initial_grad_scale
from .live_norm import BatchNormState, LiveNorms
from .plan_arena import PlanArena, _Carver, _Plan, _round_up
from .wgrad_sched import WgradScheduler


class VecParam:
    """A 1-D trainable fp32 parameter that is not a conv weight (GroupNorm affine, FCOS level scales)."""

    def __init__(self, name, numel):
        self.name, self.numel = name, numel
        self.w = self.g = None

    def reserve(self, arena):
        self._i = arena.reserve(self.name, (self.numel,))

    def bind(self, arena, params):
        self.w = arena.view("w", self._i)
        self.g = arena.view("g", self._i)
        self.w.copy_(torch.from_numpy(np.asarray(params[self.name], np.float32).reshape(-1)))

    def export(self, out):
        out[self.name] = self.w.cpu().numpy().copy()


class FPNDetector:
    """Backbone + FPN forward/backward and the BaseNet module protocol; heads and losses live in subclasses."""

    TOP_BLOCK = "p6p7"      # LastLevelP6P7 (RetinaNet / FCOS); "pool" = FPNP6 (Faster R-CNN)
    HAS_FPN = True          # False: the bare ResNet trunk ending at res5 (CenterNet) -- no pyramid, lateral, P / g_P / lat buffers or top block
    BOTTOM_UP = "backbone.bottom_up"    # the ResNet's name prefix (the FPN backbone holds it as bottom_up; a bare ResNet is "backbone")
    READS_FPN_UPSAMPLE = True   # MODEL.FPN.UPSAMPLE (retinanet.py:57, fcos.py:53); Faster R-CNN's FPN does not read it (faster_rcnn.py:30-36)

    @classmethod
    def check_config(cls, cfg):
        """Refuse the config variants this build does not implement (ValueError naming the key), instead of training another network."""
        m = cfg.MODEL
        norm = m.BACKBONE.get("NORM", "FrozenBN")
        if not isinstance(norm, str) or norm not in ("FrozenBN", "BN", "SyncBN"):
            raise ValueError(f"MODEL.BACKBONE.NORM = {norm!r} is not supported: 'FrozenBN', 'BN' and 'SyncBN' are implemented")
        fa = m.BACKBONE.FREEZE_AT
        if not isinstance(fa, int) or isinstance(fa, bool) or fa < 0:
            raise ValueError(f"MODEL.BACKBONE.FREEZE_AT = {fa!r} is not supported: an integer >= 0 (0 trains the stem, 1 freezes it, "
                             ">= 2 freezes layer1 too)")
        if norm != "FrozenBN":
            if fa >= 1:
                raise ValueError(f"MODEL.BACKBONE.NORM = {norm!r} with MODEL.BACKBONE.FREEZE_AT = {fa} is not supported: the reference's parameter "
                                 "filter freezes conv1 / layer1 by name but not their norms, so gamma / beta below the frozen convolutions "
                                 "would train through a data gradient without weight gradients -- that backward pass is not built; a live "
                                 "backbone norm runs at FREEZE_AT = 0")
            cls._check_live_norm("MODEL.BACKBONE.NORM", norm, m)
        if not cls.HAS_FPN:
            return
        fnorm = m.FPN.get("NORM", None)
        if fnorm not in (None, "BN", "SyncBN"):
            raise ValueError(f"MODEL.FPN.NORM = {fnorm!r} is not supported: None (no FPN norm), 'BN' and 'SyncBN' are implemented")
        if fnorm is not None:
            cls._check_live_norm("MODEL.FPN.NORM", fnorm, m)
        if cls.READS_FPN_UPSAMPLE:
            up = m.FPN.get("UPSAMPLE", "resize")
            if up not in ("resize", "deconv"):
                raise ValueError(f"MODEL.FPN.UPSAMPLE = {up!r} is not supported: use 'resize' or 'deconv'")

    @staticmethod
    def _check_live_norm(key, norm, m):
        """What a live norm ("BN" / "SyncBN") does not run with, under either key (MODEL.BACKBONE.NORM, MODEL.FPN.NORM)."""
        if norm == "SyncBN" and _comm.world_size() > 1:
            raise ValueError(f"{key} = 'SyncBN' at world size {_comm.world_size()} is not supported: the exchange of the batch "
                             "statistics between the ranks is not built; 'SyncBN' runs at world size 1 (as 'BN'), 'BN' at any world size "
                             "(statistics of the rank's own batch)")
        if m.get("WEIGHT_DTYPE", "bf16") != "bf16":
            what = "backbone" if "BACKBONE" in key else "FPN"
            raise ValueError(f"{key} = {norm!r} with MODEL.WEIGHT_DTYPE = {m.WEIGHT_DTYPE!r} is not supported: the fp8 twins of the "
                             f"normalised {what} tensors are not built; use 'bf16'")

    @staticmethod
    def check_anchor_config(cfg, matcher=True):
        """The anchor heads (RetinaNet family, the RPN): what the assignment kernels and the head's channel count hard-wire."""
        m = cfg.MODEL
        if matcher:
            labels = list(m.MATCHER.LABELS)
            if labels != [0, -1, 1]:
                raise ValueError(f"MODEL.MATCHER.LABELS = {labels!r} is not supported: only [0, -1, 1] (background, ignore, foreground) is implemented")
            thr = list(m.MATCHER.THRESHOLDS)
            if len(thr) != 2 or not thr[0] <= thr[1]:
                raise ValueError(f"MODEL.MATCHER.THRESHOLDS = {thr!r} is not supported: two ascending thresholds [low, high] are implemented")
        scales, ratios = [list(s) for s in m.ANCHOR.SCALES], [list(r) for r in m.ANCHOR.RATIOS]
        nlev = len(m.FPN.STRIDES)
        if len(scales) not in (1, nlev) or len({len(s) for s in scales}) != 1:
            raise ValueError(f"MODEL.ANCHOR.SCALES = {scales!r} is not supported: one list, or one per level, all of the same length "
                             "(the head predicts the same number of anchors on every level)")
        if len(ratios) != 1:
            raise ValueError(f"MODEL.ANCHOR.RATIOS = {ratios!r} is not supported: only one ratio list shared by every level is implemented")

    def __init__(self, cfg, params=None, device="cuda", seed=0):
        self.check_config(cfg)
        self.cfg = cfg
        self.device = torch.device(device)
        m = cfg.MODEL
        self.training = True
        self.num_classes = cfg.DATA.NUM_CLASSES
        self.strides = list(m.FPN.STRIDES) if self.HAS_FPN else []
        self.fpn_ch = m.FPN.OUT_CHANNELS if self.HAS_FPN else None
        self.freeze_at = m.BACKBONE.FREEZE_AT
        self.img_mean, self.img_std = list(m.BACKBONE.IMG_MEAN), list(m.BACKBONE.IMG_STD)
        if params is None:
            params = self.init_params(cfg, seed)
        self._pack_table = None            # bd_weight_pack_multi's table: built by the first repack_trainable, dropped by _bind_params
        self._h2d = HostToDevice(self.device, cfg)                 # host-to-device staging (bd_h2d_submit)
        self._raw_buf = None                                       # device copy of a RawImageBatch's packed bytes (grow-only)
        self._build_layers(params)
        self._plans = {}
        self._cur = None
        self.streams = SideStreams(self.device)
        self.wgrads = WgradScheduler(self.device, m.get("WGRAD_QUEUE", "layer"), self.streams)
        self.plan_arena = PlanArena(self.device, self.streams.join_all)
        self.extra_meter = {}
        self.use_mask_bits = True          # bit-packed ReLU gates for the wide 1x1 data gradients (False: bf16 activations as masks)

    # bench.py and the tests assign these between steps; the streams and the scheduler read them at every call
    async_wgrad = property(lambda self: self.streams.enabled, lambda self, v: setattr(self.streams, "enabled", v))
    wgrad_queue_mode = property(lambda self: self.wgrads.queue_mode, lambda self, v: setattr(self.wgrads, "queue_mode", v))
    _tstream = property(lambda self: self.streams.aux_stream)
    fp8_scale_log = property(lambda self: self.fp8_scaler.scale_log)
    fp8_group_scales = property(lambda self: self.fp8_scaler.group_scales)
    fp8_last_fill = property(lambda self: self.fp8_scaler.last_fill)

    # ------------------------------------------------------------------------------------------------
    # construction
    # ------------------------------------------------------------------------------------------------
    def _build_layers(self, params):
        dev = self.device
        m = self.cfg.MODEL
        self.arena = ParamArena(dev)
        bu = self.BOTTOM_UP
        self.blocks = P.resnet_conv_table(m.BACKBONE.NAME, bu)
        self.convs = {}

        def add(name, cin, cout, k, stride, pad, bn=None, bias=False, trainable=True, cout_pad=None, norm=None):
            c = ConvLayer(name, cin, cout, k, stride, pad, dev, bn_prefix=bn, has_bias=bias, trainable=trainable, cout_pad=cout_pad, norm=norm)
            self.convs[name] = c
            return c

        # stem: frozen when FREEZE_AT >= 1 (solver/default_solver.py:83-94); at 0 its master weight and gradient live in the arena
        # (first: the arena follows the forward order) and the backward pass ends with the kernels of csrc/stem_bwd.hip
        self.stem = TrainableStem(bu + ".conv1") if self.freeze_at < 1 else None
        # MODEL.BACKBONE.NORM = "BN" / "SyncBN" (layers/backbone/build.py:27-30; FREEZE_AT = 0 only, check_config): every bnK / downsample.1
        # and the stem's bn1 is a live BatchNorm2d under the FrozenBN's name.  self.norms owns every live norm of the model, the FPN's
        # below too, and their buffers (live_norm.py): in forward order, allocated once every layer is known
        self.backbone_norm = P.backbone_norm(self.cfg)
        self.norms = LiveNorms(dev)

        def bb_norm(prefix, c):
            """(bn_prefix, norm) of one backbone convolution: the FrozenBN fold by name, or a live norm record."""
            return dict(bn=prefix) if self.backbone_norm is None else dict(norm=self.norms.add(prefix, c))

        self.stem_packed = torch.empty((64, 7, 8, 4), dtype=torch.bfloat16, device=dev)
        if self.stem is not None:
            self.stem.norm = bb_norm(bu + ".bn1", 64).get("norm")
            self.stem.packed = self.stem_packed
            self.stem.reserve(self.arena)

        for blk in self.blocks:
            pre = blk["prefix"]
            tr = not (blk["layer"] == 1 and self.freeze_at >= 2)
            blk["trainable"] = tr
            if blk["kind"] == "bottleneck":
                blk["convs"] = [
                    add(pre + ".conv1", blk["cin"], blk["ch"], 1, 1, 0, trainable=tr, **bb_norm(pre + ".bn1", blk["ch"])),
                    add(pre + ".conv2", blk["ch"], blk["ch"], 3, blk["stride"], 1, trainable=tr, **bb_norm(pre + ".bn2", blk["ch"])),
                    add(pre + ".conv3", blk["ch"], blk["cout"], 1, 1, 0, trainable=tr, **bb_norm(pre + ".bn3", blk["cout"])),
                ]
            else:
                blk["convs"] = [
                    add(pre + ".conv1", blk["cin"], blk["ch"], 3, blk["stride"], 1, trainable=tr, **bb_norm(pre + ".bn1", blk["ch"])),
                    add(pre + ".conv2", blk["ch"], blk["cout"], 3, 1, 1, trainable=tr, **bb_norm(pre + ".bn2", blk["cout"])),
                ]
            blk["ds"] = add(pre + ".downsample.0", blk["cin"], blk["cout"], 1, blk["stride"], 0, trainable=tr,
                            **bb_norm(pre + ".downsample.1", blk["cout"])) if blk["has_ds"] else None

        self.fpn_stages = [int(f[-1]) for f in m.BACKBONE.OUT_FEATURES] if self.HAS_FPN else []          # [3, 4, 5]
        self.lateral, self.output, self.upsample = {}, {}, {}
        self.fpn_norm, self.fpn_deconv = None, False
        if self.HAS_FPN:
            self._build_fpn(add)
        self.vparams = {}
        self._build_head(add, params)

        for c in list(self.convs.values()) + list(self.vparams.values()):
            c.reserve(self.arena)
        self._reserve_head(self.arena)
        self.arena.allocate()
        self.norms.allocate()
        self._finish_layers(params)

    def _reserve_head(self, arena):
        """Arena slots of head parameters that are not ConvLayers / VecParams (after every other slot: the arena follows the bucket order)."""

    def _build_fpn(self, add):
        m = self.cfg.MODEL
        dev = self.device
        ch = self.fpn_ch
        # MODEL.FPN.NORM = "BN" / "SyncBN" (fpn_backbone.py:49-76): biasless lateral / output convolutions, each followed by a BatchNorm2d
        # (in self.norms: every lateral's, then every output convolution's)
        self.fpn_norm = m.FPN.get("NORM", None)
        nrm = {(kind, s): self.norms.add(f"backbone.fpn_{kind}{s}.norm", ch) for kind in ("lateral", "output")
               for s in (self.fpn_stages if self.fpn_norm is not None else ())}
        for s, ci in zip(self.fpn_stages, m.BACKBONE.OUT_FEATURE_CHANNELS):
            self.lateral[s] = add(f"backbone.fpn_lateral{s}", ci, ch, 1, 1, 0, bias=self.fpn_norm is None, norm=nrm.get(("lateral", s)))
            self.output[s] = add(f"backbone.fpn_output{s}", ch, ch, 3, 1, 1, bias=self.fpn_norm is None, norm=nrm.get(("output", s)))
        # MODEL.FPN.UPSAMPLE = "deconv": a learned 2x upsampling per merge, named after the coarse stage it reads (fpn_backbone.py:92-103)
        self.fpn_deconv = self.READS_FPN_UPSAMPLE and m.FPN.get("UPSAMPLE", "resize") == "deconv"
        if self.fpn_deconv:
            for s in self.fpn_stages[1:]:
                self.upsample[s] = self.convs[f"backbone.fpn_upsample{s}"] = DeconvLayer(f"backbone.fpn_upsample{s}", ch, dev)
        if self.TOP_BLOCK == "p6p7":
            self.p6 = add("backbone.top_block.p6", m.FPN.TOP_BLOCK_IN_CHANNELS, ch, 3, 2, 1, bias=True)
            self.p7 = add("backbone.top_block.p7", ch, ch, 3, 2, 1, bias=True)

    def _finish_layers(self, params):
        m = self.cfg.MODEL
        dev = self.device
        # (a trainable stem needs its half-resolution output in the backward pass: FREEZE_AT = 0 always runs the two launches)
        self.fuse_stem_pool = bool(m.get("FUSE_STEM_POOL", True)) and self.stem is None
        # frozen bottleneck blocks (layer1 under FREEZE_AT = 2) in one launch each: the two mid tensors and the residual re-read never
        # reach HBM (bd_bottleneck_fwd; False: the three / four bd_conv2d_fwd launches, kept as the parity reference)
        self.fuse_frozen_blocks = bool(m.get("FUSE_FROZEN_BLOCKS", True))
        self.sparse_shortcut_grad = bool(m.get("SPARSE_SHORTCUT_GRAD", True))   # False: the shortcut's data gradient as a full-resolution pass (A/B)
        self.weight_dtype = m.get("WEIGHT_DTYPE", "bf16")
        self._q8 = {}
        # e5m2 twins of gradients written by the producing launch (False: every fp8 data gradient casts its input in a pass; a test knob)
        self.fp8_grad_twins = bool(m.get("FP8_GRAD_TWINS", True))
        assert self.weight_dtype in ("bf16", "fp8_e4m3"), self.weight_dtype
        if self.weight_dtype == "fp8_e4m3":
            self._enable_fp8_layers()
        self.fp8_scaler = Fp8GradScaler(m, dev, self.convs)
        self._bind_params(params)

    def _build_base_anchors(self):
        """The anchor heads' base anchors, one (A, 4) tensor per level: python float64 -> float32 (layers/common/anchor_generator.py:95-109)."""
        m = self.cfg.MODEL
        scales = np.asarray(m.ANCHOR.SCALES, np.float32).tolist()
        ratios = np.asarray(m.ANCHOR.RATIOS, np.float32).tolist()
        if len(ratios) == 1:
            ratios = ratios * len(self.strides)
        if len(scales) == 1:
            scales = scales * len(self.strides)
        self.base_anchors = []
        for sc_, ra_ in zip(scales, ratios):
            base = []
            for s_ in sc_:
                area = float(s_) ** 2.0
                for r_ in ra_:
                    w = math.sqrt(area / float(r_)); h = float(r_) * w
                    base.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
            self.base_anchors.append(torch.tensor(base, dtype=torch.float32, device=self.device))

    def _plan_anchors(self, pl):
        """pl.anchors, pl.A_total: every level's anchors in one (sum HWA, 4) tensor (regenerated per forward in the reference,
        retinanet.py:116; cached per shape here: a per-shape constant, not in the arena)."""
        A = self.num_anchors
        pl.A_total = pl.pyr.pix_per_img * A
        pl.anchors = torch.empty((pl.A_total, 4), dtype=torch.float32, device=self.device)
        o = 0
        for (h, w), s, base in zip(pl.sizes, self.strides, self.base_anchors):
            n = h * w * A
            ops.anchors_generate(h, w, s, self.cfg.MODEL.ANCHOR.OFFSET, base, pl.anchors[o:o + n])
            o += n

    def _enable_fp8_layers(self):
        """BASELINE config 5: fp8-e4m3 weights (one scale per output channel) for the forward of the 3x3 convolutions -- where a
        quantised copy of the input is read nine times; the HBM-bound 1x1 layers and the whole backward pass stay bf16."""
        m = self.cfg.MODEL
        # FP8_DGRAD (default True again since round 3): e5m2 gradients x e4m3 weights for the data gradients of the fp8 layers, +2.5-3.5 % on
        # the step.  Round 2 had to make it opt-in: with ONE delayed scale for all layers R101 at the batch-32 learning rate left the
        # finite range between steps 620 and 1 020 of the repeated-batch run.  Round 3: one scale per backward phase (FP8_SCALE_GROUPS)
        # with two binades of headroom below e5m2's maximum and a four-probe history -- see fp8_scaling.py and DESIGN.md (a21).
        dgrad = bool(m.get("FP8_DGRAD", True))
        scale0 = initial_grad_scale(m)
        side = {id(getattr(self, n)) for n in ("p6", "p7") if hasattr(self, n)}
        for c in self.convs.values():
            # the staggered fp8 patch kernel serves 3x3 / stride 1 with Cout > 128 (1.6x the bf16 kernel); the top block's stride-2
            # convolutions go through the generic fp8 kernel (faster than their bf16 launches, and they complete the pyramid's e4m3
            # twin); narrower or strided backbone layers are FASTER on their bf16 kernels and stay there
            if (c.k == 3 and c.cin % 16 == 0 and not isinstance(c, FCLayer)
                    and ((c.stride == 1 and c.cout > 128) or id(c) in side)):
                key = "side" if id(c) in side else "main"          # P6 / P7 run on a side stream: their own scratch
                c.enable_fp8(lambda n, key=key: self._q8_buf(key, n), m.get("FP8_ACT_SCALE", 1.0), dgrad=dgrad, grad_scale=scale0,
                             # FP8_WGRAD: 0 = bf16 weight gradients, 1 = the one-byte kernel (bd_conv2d_wgrad_fp8) for the bias-free
                             # layers (backbone conv2), 2 (default since round 4) = also the towers.  Exact on representable inputs;
                             # 1.4x the bf16 ring kernel per head-tower launch.  Round 2 kept it opt-in (no gain in the step then,
                             # and a repeated-batch run under the static scale lost convergence); under per-group delayed scales and
                             # stochastic rounding: R101 batch 32 same box 487.6 / 487.6 img/s at 0, 494.5 / 496.4 at 2; ten of ten
                             # seeds through 1 500 repeated-batch steps (profiles/r04_fp8_stability_wgrad.txt; bf16 and the
                             # FP8_WGRAD = 0 form: nine of ten each); whole-model gradient cosine vs bf16 0.9814 (0.9818 at 0) at
                             # 2 x 800 x 1344 (tests/test_r101_gpu.py)
                             wgrad=(int(m.get("FP8_WGRAD", 2)) >= (2 if c.has_bias else 1)) and dgrad)
        # the bottleneck 1x1s around an fp8 3x3 (res4 / res5 blocks after the first) on one-byte operands.  In isolation the reducing
        # direction (conv1 forward, conv3's data gradient: the input is most of the bytes) is 1.5 - 1.6x faster than its bf16 launch
        # and the expanding one about even; in the step the extra twins the neighbouring launches must write take most of it back:
        # R101 batch 32, one box: 461.3 img/s without, 463.9 with both directions (the default), 458.5 with the reducing one only
        if bool(m.get("FP8_1X1", True)):
            for blk in self.blocks:
                if blk["kind"] == "bottleneck" and blk["convs"][1].fp8 and blk["convs"][1].stride == 1:
                    for c in (blk["convs"][0], blk["convs"][2]):
                        if c.cin % 32 == 0 and c.cout % 32 == 0:
                            c.enable_fp8_1x1(m.get("FP8_ACT_SCALE", 1.0), dgrad=dgrad, grad_scale=scale0,
                                             expanding=bool(m.get("FP8_1X1_EXPANDING", True)))

    def _bind_params(self, params):
        """(Re)load every parameter from a reference-layout dict (name -> numpy) and refresh the packed bf16 copies."""
        dev = self.device
        bu = self.BOTTOM_UP
        self.stem_w = torch.from_numpy(np.asarray(params[bu + ".conv1.weight"], np.float32)).permute(0, 2, 3, 1).contiguous().to(dev)
        g, b = params[bu + ".bn1.weight"], params[bu + ".bn1.bias"]
        mu, var = params[bu + ".bn1.running_mean"], params[bu + ".bn1.running_var"]
        sc = g / np.sqrt(var + 1e-5)
        self.stem_scale = torch.from_numpy(sc.astype(np.float32)).to(dev)
        self.stem_shift = torch.from_numpy((b - mu * sc).astype(np.float32)).to(dev)
        if self.stem is not None:
            self.stem_w = self.stem.bind(self.arena, self.stem_w, self.stem_scale)
            if self.stem.norm is not None:
                self.stem.norm.bind(self.arena, params)
        self._pack_table = None                # row_scale tensors are re-created by bind()
        for c in list(self.convs.values()) + list(self.vparams.values()):
            c.bind(self.arena, params)
        self._fold_norms(pack=False)           # (repack_weights below packs everything)
        # FrozenBN vectors are constants state_dict() hands back; live backbone norms export their own (moving) values
        self._bn_params = {k: np.asarray(v, np.float32).copy() for k, v in params.items()
                           if (".bn" in k or "downsample.1" in k) and self.backbone_norm is None}
        self.repack_weights()

    def _q8_buf(self, key, nbytes):
        """Scratch for the e4m3 copy of a convolution's input, one per stream (grown on demand; stream-ordered reuse)."""
        t = self._q8.get(key)
        if t is None or t.numel() < nbytes:
            t = self._q8[key] = torch.empty((int(nbytes),), dtype=torch.uint8, device=self.device)
        return t

    def load_weights(self, weights, strict=False):
        """BaseNet.load_weights (models/base_net.py:83-89) -> utils/checkpoint.py load_matched_weights: `weights` is a dict
        or the path of a .pkl / .npz checkpoint; names are matched exactly, then by suffix, then by shape."""
        from ..utils.checkpoint import load_matched_weights
        return load_matched_weights(self, weights, strict)

    def repack_weights(self):
        """Refresh the bf16 packed copies from the fp32 masters (after load_weights / every optimizer step)."""
        ops.stem_weight_pack(self.stem_w, self.stem_scale, self.stem_packed)
        for c in self.convs.values():
            c.pack()

    def repack_trainable(self):
        """All trainable convs in ONE launch (bd_weight_pack_multi); the table holds raw pointers into the arena and the packed
        tensors, which never move after _build_layers."""
        self.fp8_scaler.apply_staged()
        if self._pack_table is None:
            ent = [(c.w, c.row_scale, c.w_fwd, c.w_dgrad, c.cout, c.k * c.k, c.cin) for c in self.convs.values()
                   if c.trainable and not isinstance(c, DeconvLayer)]
            self._pack_table = ops.build_pack_table(ent, self.device)
        ops.weight_pack_multi(self._pack_table)
        if self.stem is not None:                # the 7 x 8 x 4 layout of the stem kernels (bd_stem_weight_pack)
            ops.stem_weight_pack(self.stem_w, self.stem_scale, self.stem_packed)
        for c in self.upsample.values():        # phase-major operands of their own (bd_fpn_deconv_pack)
            c.pack()
        for c in self.convs.values():
            if (c.fp8 or c.fp8_1x1 or c.fp8_1x1_dgrad) and c.trainable:
                c.pack_fp8()
        if self.norms and not self.training:       # evaluating (ModelEMA.applied() swaps the weights in): the folded affine follows gamma / beta
            self._fold_norms()

    def _fold_norms(self, pack=True):
        """Training: the normalised convolutions run bare (no bias, no scale; the batch-norm kernels follow).  Evaluation: the running
        statistics and gamma / beta become the per-channel affine of the convolution's own launch, as FrozenBN's (scale folded into the
        packed weight, shift = its bias) -- inference launches no batch-norm kernel.  FPN norms and backbone norms alike; the stem's fold
        is stem_scale / stem_shift."""
        if not self.norms:
            return
        for c in self.convs.values():
            if c.norm is None:
                continue
            if self.training:
                c.row_scale = c.b = None
            else:
                c.norm.fold()
                c.row_scale, c.b = c.norm.fold_scale, c.norm.fold_shift
            if pack:
                c.pack()
        n = getattr(self.stem, "norm", None)
        if n is not None:
            if self.training:
                self.stem_scale = None             # (bd_stem_conv7x7_raw_fwd reads no shift)
            else:
                n.fold()
                self.stem_scale, self.stem_shift = n.fold_scale, n.fold_shift
            self.stem.row_scale = self.stem_scale
            if pack:
                ops.stem_weight_pack(self.stem_w, self.stem_scale, self.stem_packed)
        self._pack_table = None                # (it holds the row_scale pointers)

    # reference module protocol ------------------------------------------------------------------------
    def train(self, mode=True):
        switch = bool(mode) != bool(self.training)
        self.training = mode
        if switch:
            self._fold_norms()
        return self

    def load_state_dict(self, states, strict=True):
        """Parameters and buffers (the FPN norm's running statistics among them) from a state_dict() of the same architecture."""
        return self.load_weights(states, strict=strict)

    def eval(self):
        return self.train(False)

    def __call__(self, inputs):
        return self.forward(inputs)

    def forward(self, inputs):
        """BaseNet.forward (models/base_net.py:50-54)."""
        if self.training:
            return self.get_losses(inputs)
        return self.inference(inputs)

    def state_dict(self):
        out = {}
        for c in list(self.convs.values()) + list(self.vparams.values()):
            c.export(out)
        out[self.BOTTOM_UP + ".conv1.weight"] = self.stem_w.permute(0, 3, 1, 2).contiguous().cpu().numpy()
        if getattr(self.stem, "norm", None) is not None:
            self.stem.norm.export(out)
        out.update({k: v.copy() for k, v in self._bn_params.items()})
        return out

    def debug_activations(self):
        """Stored activations of the last forward as NCHW fp32 CPU tensors, keyed like oracle/model.py `_act`
        (parity tests inject them into the oracle so that both backward passes see identical ReLU gates)."""
        pl = self._cur
        N = pl.N
        out = {}

        def nchw(t, g, c=None):
            v = t.float().cpu().view(N, g.H[0], g.W[0], -1).permute(0, 3, 1, 2).contiguous()
            return v if c is None else v[:, :c].contiguous()

        def lvl(t, i, c=None):
            g = pl.pyr
            v = t.float().cpu().view(N, g.pix_per_img, -1)[:, g.off[i]: g.off[i] + g.H[i] * g.W[i]]
            v = v.reshape(N, g.H[i], g.W[i], -1).permute(0, 3, 1, 2).contiguous()
            return v if c is None else v[:, :c].contiguous()

        if self.stem is None:       # (a trainable stem: the oracle must differentiate through its own stem and max-pool, not a constant)
            out["pool"] = nchw(pl.pool_out, pl.g_pool)
        elif self.stem.norm is not None:   # under a live norm the stem's stored ReLU output: the oracle's norm and max-pool see the same gates
            out["stem_out"] = nchw(pl.stem_out, pl.g_stem)
            # (of the last backward(): dL/dz of every backbone norm, the bf16 terms its sums read)
            out["g_stem_out"] = nchw(pl.grad_stem, pl.g_stem)
            for blk, b in zip(self.blocks, pl.blk):
                for i, (t, g) in enumerate(zip(b.g_mids, b.mid_geo)):
                    out[f"g_{blk['prefix']}.a{i}"] = nchw(t, g)
                out[f"g_{blk['prefix']}.out"] = nchw(b.g_out, b.gout)
        for blk, b in zip(self.blocks, pl.blk):
            pre = blk["prefix"]
            for i, (t, g) in enumerate(zip(b.mids, b.mid_geo)):
                out[f"{pre}.a{i}"] = nchw(t, g)
            if b.idt is not None:
                out[pre + ".idt"] = nchw(b.idt, b.gout)
            out[pre + ".out"] = nchw(b.out, b.gout)
        for s in self.fpn_stages:
            out[f"lat{s}"] = nchw(pl.lat[s], pl.blk[pl.res[s]].gout)
        for i in range(pl.pyr.nlev if self.HAS_FPN else 0):
            out[f"P{self.fpn_stages[0] + i}"] = lvl(pl.P, i)
        self._debug_head(pl, out, lvl)
        return out

    def reference_grads(self):
        """Gradients of the last backward() keyed by the reference's parameter names, in the reference's layouts
        (conv weights OIHW, padding rows dropped) -- what megengine's GradManager would hand to the optimizer."""
        out = {}
        if self.stem is not None:
            self.stem.export_grad(out)
        for c in self.convs.values():
            if not c.trainable:
                continue
            c.export_grad(out)
        for v in self.vparams.values():
            out[v.name] = v.g.detach().cpu().clone()
        return out

    def state_dict_trainable_names(self):
        """Trainable parameters under the reference's names (what DetSolver.params would collect)."""
        return list(self.reference_grads_names())

    def reference_grads_names(self):
        names = [self.stem.name + ".weight"] if self.stem is not None else []
        if getattr(self.stem, "norm", None) is not None:
            names += [self.stem.norm.name + ".weight", self.stem.norm.name + ".bias"]
        for c in self.convs.values():
            if not c.trainable:
                continue
            parts = getattr(c, "parts", None)
            for n in ([p[0] for p in parts] if parts else [c.name]):
                names.append(n + ".weight")
                if c.has_bias and not c.bn_prefix:
                    names.append(n + ".bias")
            if c.norm is not None:
                names += [c.norm.name + ".weight", c.norm.name + ".bias"]
        names += [v.name for v in self.vparams.values()]
        return names

    def trainable_parameter_names(self):
        return [e[0] for e in self.arena.entries]

    # ------------------------------------------------------------------------------------------------
    # shape plan
    # ------------------------------------------------------------------------------------------------
    def _plan(self, N, Hp, Wp):
        """The plan of one padded batch shape: built once (constants + carved layout) and kept; its per-step buffers are arena views.
        Calling it for a cached shape returns the plan untouched -- the buffers of that shape's last step are still readable, as long as
        no step at another shape ran in between."""
        key = (N, Hp, Wp)
        pl = self._plans.get(key)
        if pl is not None:
            return pl
        pl = _Plan()
        pl.N, pl.Hp, pl.Wp = N, Hp, Wp
        C = pl._carve = _Carver()
        bf = torch.bfloat16

        def act(g, c):
            return C.empty((g.pixels, c), bf)

        pl.x_halo = C.empty((N, Hp + 6, Wp + 8, 4), bf)      # (bd_pad_normalize writes every element, the zero halo included)
        g2 = ops.single(N, Hp // 2, Wp // 2)
        g4 = ops.single(N, (Hp // 2 - 1) // 2 + 1, (Wp // 2 - 1) // 2 + 1)
        pl.g_stem, pl.g_pool = g2, g4
        # the fused stem + max-pool launch never materialises the half-resolution stem output (MODEL.FUSE_STEM_POOL False: two launches)
        pl.stem_out, pl.pool_out = (None if self.fuse_stem_pool else act(g2, 64)), act(g4, 64)
        if self.stem is not None:   # FREEZE_AT = 0: dL/d(pool_out) from layer1's first block, dL/d(pre-activation) of stem_out
            pl.grad_pool, pl.grad_stem = C.like(pl.pool_out), C.like(pl.stem_out)
            pl.g_image = ops.single(N, Hp, Wp)
        # (live norm, dense geometry of its convolution's output), in forward order
        normed = [(self.stem.norm, g2)] if getattr(self.stem, "norm", None) is not None else []
        # backbone
        pl.blk = []
        gin = g4
        for blk in self.blocks:
            b = _Plan()
            b.gin = gin
            b.gout = gin.conv_out(1, blk["stride"], 0) if blk["stride"] == 2 else gin
            b.fused = (self.fuse_frozen_blocks and not blk["trainable"] and blk["kind"] == "bottleneck" and blk["stride"] == 1
                       and gin.nlev == 1
                       and ops.bottleneck_fwd_supported(N, gin.H[0], gin.W[0], blk["cin"], blk["ch"], blk["cout"], blk["has_ds"]))
            if b.fused:                                   # one launch: no mid tensors, no materialised shortcut
                b.mid_geo = [gin, b.gout]
                b.mids = []
            elif blk["kind"] == "bottleneck":
                b.mid_geo = [gin, b.gout]
                b.mids = [act(gin, blk["ch"]), act(b.gout, blk["ch"])]
            else:
                b.mid_geo = [b.gout]
                b.mids = [act(b.gout, blk["ch"])]
            b.idt = act(b.gout, blk["cout"]) if (blk["has_ds"] and not b.fused) else None
            b.out = act(b.gout, blk["cout"])
            # e4m3 twin of conv1's output, written by the dense 1x1 launch for the fp8 conv2 that follows
            b.mid8 = None
            if (blk["kind"] == "bottleneck" and blk["convs"][1].fp8
                    and ops.dense_1x1_bits_ok(blk["convs"][0].desc(gin, gin))):
                b.mid8 = C.empty((gin.pixels, blk["ch"]), torch.uint8)
            b.out_bits = None
            b.g_mid8 = None
            # one-byte twins for the fp8 1x1 launches: conv2's output (conv3 reads it), the block output (the next block's conv1 reads
            # it), and in the backward pass the block's output gradient (conv3's data gradient) and conv2's data gradient (conv1's)
            b.mid8b = b.out8 = b.g_out8 = b.g_mid8a = None
            b.g_out8_ready = False
            if blk["kind"] == "bottleneck":
                u8 = lambda geo, ch: C.empty((geo.pixels, ch), torch.uint8)
                nxt = self.blocks[len(pl.blk) + 1] if len(pl.blk) + 1 < len(self.blocks) else None
                if blk["convs"][2].fp8_1x1 and blk["convs"][1].fp8 and blk["convs"][1].stride == 1:
                    b.mid8b = u8(b.gout, blk["ch"])
                if nxt is not None and nxt["kind"] == "bottleneck" and nxt["convs"][0].fp8_1x1 \
                        and ops.dense_1x1_bits_ok(blk["convs"][2].desc(b.gout, b.gout)):
                    b.out8 = u8(b.gout, blk["cout"])
                if blk["trainable"] and self.fp8_grad_twins:
                    if blk["convs"][2].fp8_1x1_dgrad and nxt is not None and nxt["kind"] == "bottleneck" and nxt["trainable"]:
                        b.g_out8 = u8(b.gout, blk["cout"])
                    if blk["convs"][0].fp8_1x1_dgrad and blk["convs"][1].fp8_dgrad:
                        b.g_mid8a = u8(gin, blk["ch"])
            if blk["trainable"]:
                b.g_mids = [C.like(t) for t in b.mids]
                b.g_out = C.like(b.out)
                if (blk["kind"] == "bottleneck" and blk["convs"][1].fp8_dgrad and self.fp8_grad_twins
                        and blk["convs"][2].dgrad_writes_twin(b.gout, b.gout)):
                    b.g_mid8 = C.empty((b.gout.pixels, blk["ch"]), torch.uint8)
                # the block output's ReLU gate, bit-packed by the conv3 launch that writes it (1 bit instead of a bf16 per element):
                # what the NEXT block's conv1 / the FPN lateral read as their data-gradient mask (dense 1x1 launches: conv1x1.hip)
                if (blk["kind"] == "bottleneck" and self.use_mask_bits
                        and ops.dense_1x1_bits_ok(blk["convs"][-1].desc(b.gout, b.gout))):
                    b.out_bits = C.empty((blk["cout"] // 32, b.gout.pixels), torch.int32)
            normed += [(c.norm, g) for c, g in zip(blk["convs"] + [blk["ds"]], b.mid_geo + [b.gout, b.gout])
                       if c is not None and c.norm is not None]
            pl.blk.append(b)
            gin = b.gout
        # feature taps (last block of layer 2..4 -> res3..res5)
        pl.res = {}
        for i, blk in enumerate(self.blocks):
            last = i + 1 == len(self.blocks) or self.blocks[i + 1]["layer"] != blk["layer"]
            if last:
                pl.res[blk["layer"] + 1] = i
        if self.HAS_FPN:
            self._plan_fpn(pl, C, act, normed)
        self._plan_tail(pl, C, act, normed)
        return pl

    def _plan_fpn(self, pl, C, act, normed):
        """The pyramid's buffers: P / g_P, the laterals and their gradients (the P6 ReLU copy follows the norm buffers, in _plan_tail)."""
        N = pl.N
        # pyramid
        sizes = [(pl.blk[pl.res[s]].gout.H[0], pl.blk[pl.res[s]].gout.W[0]) for s in self.fpn_stages]
        h5, w5 = sizes[-1]
        h6, w6 = (h5 - 1) // 2 + 1, (w5 - 1) // 2 + 1
        h7, w7 = (h6 - 1) // 2 + 1, (w6 - 1) // 2 + 1
        sizes = sizes + ([(h6, w6), (h7, w7)] if self.TOP_BLOCK == "p6p7" else [(h6, w6)])
        pl.sizes = sizes
        pl.pyr = Geom(N, [s[0] for s in sizes], [s[1] for s in sizes])
        ch = self.fpn_ch
        pl.P = act(pl.pyr, ch)
        pl.g_P = act(pl.pyr, ch)
        # e4m3 twin of the pyramid: written by the fp8 launches that produce P (FPN output convolutions, P6, P7), read by the heads'
        # first convolutions instead of a cast pass.  Only when EVERY level is written by an fp8 convolution (LastLevelP6P7).
        writers = [self.output[s] for s in self.fpn_stages] + ([self.p6, self.p7] if self.TOP_BLOCK == "p6p7" else [])
        pl.P8 = (C.empty((pl.pyr.pixels, ch), torch.uint8)
                 if self.TOP_BLOCK == "p6p7" and all(c.fp8 for c in writers) else None)
        pl.lat = {s: act(pl.blk[pl.res[s]].gout, ch) for s in self.fpn_stages}
        pl.g_lat = {s: C.like(pl.lat[s]) for s in self.fpn_stages}
        normed += [(c[s].norm, pl.blk[pl.res[s]].gout) for c in (self.lateral, self.output) for s in self.fpn_stages if c[s].norm is not None]

    def _plan_tail(self, pl, C, act, normed):
        """Norm buffers of every live norm, the head's plan, the workspaces; places the plan in the arena."""
        N, Hp, Wp = pl.N, pl.Hp, pl.Wp
        # the pre-norm output of every normalised convolution, kept for the backward pass, and the gradient with respect to it: buffers of
        # their own, never reused within a step (the FPN's top-down path still reads g_lat, the side stream's weight gradients read g_y
        # late); the reduction workspace fits the largest
        pl.norm_y, pl.norm_gy, pl.norm_geo = {}, {}, {}
        for n, g in normed:
            pl.norm_y[n.name], pl.norm_gy[n.name], pl.norm_geo[n.name] = act(g, n.C), act(g, n.C), g
        if normed:
            pl.bn_ws = C.empty((max(ops.bn_workspace_bytes(g.pixels, n.C) for n, g in normed) // 4 + 64,), torch.float32)
        if self.HAS_FPN:
            h6, w6 = pl.sizes[len(self.fpn_stages)]
            pl.p6_relu = C.empty((N * h6 * w6, self.fpn_ch), torch.bfloat16)
            pl.g_p6r = ops.single(N, h6, w6)
        self._plan_head(pl)
        # workspaces
        need = self.stem.wgrad_ws_bytes(pl.g_image, pl.g_stem) if self.stem is not None else 0
        for blk, b in zip(self.blocks, pl.blk):
            if not blk["trainable"]:
                continue
            geos = [b.gin] + b.mid_geo + [b.gout]
            for ci, c in enumerate(blk["convs"]):
                need = max(need, c.wgrad_ws_bytes(geos[ci], geos[ci + 1]))
            if blk["ds"] is not None:
                need = max(need, blk["ds"].wgrad_ws_bytes(b.gin, b.gout))
        for s in self.fpn_stages:
            gl = pl.blk[pl.res[s]].gout
            need = max(need, self.lateral[s].wgrad_ws_bytes(gl, gl), self.output[s].wgrad_ws_bytes(gl, gl))
        for li, s in enumerate(self.fpn_stages[1:]):
            gc, gf = pl.blk[pl.res[s]].gout, pl.blk[pl.res[self.fpn_stages[li]]].gout
            need = max(need, self.upsample[s].wgrad_ws_bytes(gf, gc)) if s in self.upsample else need
        if self.TOP_BLOCK == "p6p7":
            g5, g6 = pl.blk[pl.res[self.fpn_stages[-1]]].gout, pl.pyr.level(len(self.fpn_stages))
            need = max(need, self.p6.wgrad_ws_bytes(g5, g6), self.p7.wgrad_ws_bytes(pl.g_p6r, pl.pyr.level(len(self.fpn_stages) + 1)))
        need = max(need, self._head_wgrad_ws_bytes(pl))
        pl.wgrad_ws = C.empty((need // 4 + 64,), torch.float32)
        cmax = max([2048] + [c.cout for c in self.convs.values() if c.trainable and c.has_bias])      # (a class predictor may be wider)
        pl.colsum_ws = C.empty((ops.colsum_workspace_bytes(cmax) // 4,), torch.float32)
        self.plan_arena.place(pl)
        self._plans[(N, Hp, Wp)] = pl

    # ------------------------------------------------------------------------------------------------
    # plan arena
    # ------------------------------------------------------------------------------------------------
    arena_bytes = property(lambda self: self.plan_arena.nbytes)
    arena_grows = property(lambda self: self.plan_arena.grows)

    @staticmethod
    def plan_bytes(pl):
        """Bytes one plan's per-step buffers take in the arena."""
        return pl._carve.nbytes

    def reserve(self, N, H, W):
        """Grow the plan arena to fit a batch of N images of (up to) H x W without running a step: a run pre-sizes for its largest batch.
        Returns the plan of that padded shape."""
        return self._plan(N, _round_up(H, 32), _round_up(W, 32))

    def _bind_plan(self, pl):
        self.plan_arena.bind(pl)

    def _scratch(self, name, nbytes):
        return self.plan_arena.scratch(name, nbytes)

    def _head_wgrad_ws_bytes(self, pl):
        return max(c.wgrad_ws_bytes(pl.pyr, pl.pyr) for c in self._head_convs())

    # ------------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------------
    def pre_process(self, inputs):
        """RetinaNet.pre_process (retinanet.py:90-107): H2D copy + pad to x32 + normalise (fused kernel)."""
        image = inputs["data"] if isinstance(inputs, dict) else inputs
        if isinstance(image, RawImageBatch):
            # raw uint8 images of their own sizes (data/raw.py): resize, flip, pad and normalise happen in the one launch that fills x_halo
            N, H, W = image.N, image.Hmax, image.Wmax
            packed = self._raw_to_device(image)
        else:
            if not (torch.is_tensor(image) and image.is_cuda):
                image = self._h2d(image)
            image = image.to(self.device, dtype=torch.float32, non_blocking=True).contiguous()
            N, _, H, W = image.shape
        Hp, Wp = _round_up(H, 32), _round_up(W, 32)
        pl = self._plan(N, Hp, Wp)
        self._bind_plan(pl)
        if isinstance(image, AffineImageBatch):
            # CenterNet's training pipeline (data/raw.py CenterNetRawCollator): warp, flip, colour passes and normalise, one or two launches
            ws = self._scratch("affine_jitter", ops.affine_jitter_workspace_bytes(N, Hp, Wp))
            ops.affine_jitter_normalize(packed, image.descs, Hp, Wp, self.img_mean, self.img_std, pl.x_halo, ws)
        elif isinstance(image, RawImageBatch):
            ops.resize_pad_normalize(packed, image.descs, Hp, Wp, self.img_mean, self.img_std, pl.x_halo)
        else:
            ops.pad_normalize(image, Hp, Wp, self.img_mean, self.img_std, pl.x_halo)
        out = {"plan": pl}
        if isinstance(inputs, dict) and "gt_boxes" in inputs:
            gt = torch.as_tensor(np.asarray(inputs["gt_boxes"]), dtype=torch.float32) if not torch.is_tensor(inputs["gt_boxes"]) else inputs["gt_boxes"]
            gt = gt.to(self.device, dtype=torch.float32)
            if gt.shape[1] == 0:
                # a batch without a single annotation (the pad collator then yields (N, 0, 5)): one all-zero padding row keeps the
                # assignment kernels' Gmax > 0 contract; num_gt (im_info[:, 4]) is 0, so every anchor / point is background
                gt = torch.zeros((gt.shape[0], 1, 5), dtype=torch.float32, device=self.device)
            out["gt_boxes"] = gt.contiguous()
        if isinstance(inputs, dict) and "im_info" in inputs:
            info = torch.as_tensor(np.asarray(inputs["im_info"]), dtype=torch.float32) if not torch.is_tensor(inputs["im_info"]) else inputs["im_info"]
        else:
            info = torch.tensor([[Hp, Wp, H, W, 0]] * N, dtype=torch.float32)
        out["img_info"] = info.to(self.device, dtype=torch.float32).contiguous()
        return out

    def _raw_to_device(self, batch):
        """The packed bytes of a RawImageBatch -> one grow-only uint8 device buffer, in one asynchronous copy on the current stream (its
        reader, bd_resize_pad_normalize, runs there too); the batch's collator learns when its buffer is free again."""
        src = batch.packed
        buf = self._raw_buf
        if buf is None or buf.numel() < src.numel():
            buf = self._raw_buf = torch.empty((src.numel(),), dtype=torch.uint8, device=self.device)
        dst = buf[: src.numel()]
        dst.copy_(src, non_blocking=True)
        drained = torch.cuda.Event()
        drained.record()
        batch.copied(drained)
        return dst

    def _block_forward(self, blk, b, x, x8=None):
        """x8: the e4m3 twin of the block input when the previous block's conv3 wrote one (fp8 mode)."""
        convs = blk["convs"]
        if b.fused:
            ds = blk["ds"]
            return ops.bottleneck_fwd(b.gin.N, b.gin.H[0], b.gin.W[0], blk["cin"], blk["ch"], blk["cout"], x, convs[0].w_fwd, convs[0].b,
                                      convs[1].w_fwd, convs[1].b, convs[2].w_fwd, convs[2].b, ds.w_fwd if ds is not None else None,
                                      ds.b if ds is not None else None, b.out)
        idt = x
        if blk["ds"] is not None:
            blk["ds"].forward(x, b.gin, b.gout, b.idt)
            idt = b.idt
        geos = [b.gin] + b.mid_geo + [b.gout]
        t, t8 = x, x8
        for ci, c in enumerate(convs[:-1]):
            y8 = None
            if ci == 0 and b.mid8 is not None:
                y8 = b.mid8
            elif ci == 1 and b.mid8b is not None:
                y8 = b.mid8b
            c.forward(t, geos[ci], geos[ci + 1], b.mids[ci], relu=True, x8=t8, y8=y8,
                      q_scale=convs[ci + 1].act_scale if y8 is not None else 1.0)
            t, t8 = b.mids[ci], y8
        convs[-1].forward(t, geos[-2], geos[-1], b.out, add=idt, relu=True, bits=b.out_bits, x8=t8, y8=b.out8)
        return b.out

    def _conv_norm_forward(self, conv, x, gin, gout, z, gz, pl, residual=None, relu=False):
        """A convolution under a live norm, in training mode: the bare convolution into its pre-norm tensor pl.norm_y (kept for the backward
        pass), the batch statistics of that (running statistics updated), then the one-pass epilogue z = [relu](BN(y) [+ residual]).
        gz: z's geometry -- gout's dense one, or a level of the pyramid."""
        n, B = conv.norm, BatchNormState
        y = pl.norm_y[n.name]
        conv.forward(x, gin, gout, y)
        ops.bn_stats_fwd(y, gout, n.C, B.EPS, B.MOMENTUM, n.mean, n.inv_std, n.sums, n.running_mean, n.running_var, pl.bn_ws)
        ops.bn_apply_act_fwd(y, gout, n.mean, n.inv_std, n.gamma, n.beta, z, gz, n.C, residual=residual, gr=gout, relu=relu)

    def _block_forward_norm(self, blk, b, x, pl):
        """_block_forward under a live backbone norm: conv -> BN -> ReLU, the last stage conv -> BN -> + identity -> ReLU
        (models/cls/resnet.py:42-52, 94-113), the shortcut convolution conv -> BN."""
        convs = blk["convs"]
        idt = x
        if blk["ds"] is not None:
            self._conv_norm_forward(blk["ds"], x, b.gin, b.gout, b.idt, b.gout, pl)
            idt = b.idt
        geos = [b.gin] + b.mid_geo + [b.gout]
        t = x
        for ci, c in enumerate(convs):
            last = ci + 1 == len(convs)
            z = b.out if last else b.mids[ci]
            self._conv_norm_forward(c, t, geos[ci], geos[ci + 1], z, geos[ci + 1], pl, residual=idt if last else None, relu=True)
            t = z
        return b.out

    def network_forward(self, pl):
        """RetinaNet.network_forward (retinanet.py:109-118): backbone + FPN + head; logits/offsets come out already
        in the (N, sum HWA, K) layout of permute_to_N_Any_K + concat (function.py:26-32, retinanet.py:127-132).

        The stem runs as one launch (bd_stem_pool_fwd, MODEL.FUSE_STEM_POOL) while it is frozen.  Under MODEL.BACKBONE.FREEZE_AT = 0 the
        key is ignored: the backward pass reads the half-resolution stem output, so the two-launch form always runs."""
        N = pl.N
        live = self.backbone_norm is not None and self.training      # batch statistics in the backbone (evaluation: folded, the FrozenBN launches)
        if live:
            self._conv_norm_forward(self.stem, pl.x_halo, pl.g_image, pl.g_stem, pl.stem_out, pl.g_stem, pl, relu=True)
            ops.maxpool3x3s2_fwd(pl.stem_out, N, pl.g_stem.H[0], pl.g_stem.W[0], 64, pl.pool_out)
        elif self.fuse_stem_pool:
            ops.stem_pool_fwd(N, pl.Hp, pl.Wp, pl.x_halo, self.stem_packed, self.stem_shift, pl.pool_out)
        else:
            ops.stem_conv7x7_fwd(N, pl.Hp, pl.Wp, pl.x_halo, self.stem_packed, self.stem_shift, pl.stem_out)
            ops.maxpool3x3s2_fwd(pl.stem_out, N, pl.g_stem.H[0], pl.g_stem.W[0], 64, pl.pool_out)
        x = pl.pool_out
        x8 = None
        for blk, b in zip(self.blocks, pl.blk):
            x = self._block_forward_norm(blk, b, x, pl) if live else self._block_forward(blk, b, x, x8)
            x8 = b.out8
        if not self.HAS_FPN:
            return self.head_forward(pl)
        # FPN (fpn_backbone.py:123-160): top-down from the coarsest level
        st = self.fpn_stages
        nl = len(st)
        b5 = pl.blk[pl.res[st[-1]]]
        if self.TOP_BLOCK == "p6p7":
            # LastLevelP6P7 (:198-204) only needs res5 and writes its own pyramid levels: its two small-grid convs (70 workgroups for
            # P6 at 800x1344) run on the weight-gradient stream (idle in the forward pass), concurrently with the lateral / output convs below
            g6, g7 = pl.pyr.level(nl), pl.pyr.level(nl + 1)
            side = self.streams.wgrad()
            with fork(side):
                self.p6.forward(b5.out, b5.gout, g6, pl.P, y8=pl.P8)
                self._relu_level(pl.P, g6, pl.p6_relu)
                self.p7.forward(pl.p6_relu, pl.g_p6r, g7, pl.P, y8=pl.P8)
        def conv(c, x, g, z, gz, **kw):
            """One lateral / output convolution, x at the level's dense geometry g -> z at gz.  Under MODEL.FPN.NORM in training mode
            z = BN(conv(x)) with batch statistics over all N H W pixels of the level (evaluation: folded into the convolution's launch)."""
            if c.norm is not None and self.training:
                self._conv_norm_forward(c, x, g, g, z, gz, pl)
            else:
                c.forward(x, g, gz, z, **kw)

        prev, prev_geo = None, None
        for li in range(nl - 1, -1, -1):
            s = st[li]
            b = pl.blk[pl.res[s]]
            conv(self.lateral[s], b.out, b.gout, pl.lat[s], b.gout)
            if prev is not None and self.fpn_deconv:     # lat_s = lateral + deconv(lat_{s+1}), one rounding, in place
                self.upsample[st[li + 1]].forward(prev, prev_geo, pl.lat[s], add=pl.lat[s])
            elif prev is not None:
                ops.upsample2x_add_fwd(prev, prev_geo, pl.lat[s], b.gout, self.fpn_ch)
            conv(self.output[s], pl.lat[s], b.gout, pl.P, pl.pyr.level(li), y8=pl.P8)
            prev, prev_geo = pl.lat[s], b.gout
        if self.TOP_BLOCK == "p6p7":
            join(side)
        else:
            ops.subsample2x_fwd(pl.P, pl.pyr.level(nl - 1), pl.P, pl.pyr.level(nl), self.fpn_ch)   # FPNP6 (:172-183)
        self.head_forward(pl)

    def _relu_level(self, src, geo, dst):
        """dst (dense, per level) = relu(one pyramid level of src); the level is contiguous per image."""
        C = src.shape[1]
        n = geo.H[0] * geo.W[0]
        sv = src.view(geo.N, geo.pix_per_img, C)
        dv = dst.view(geo.N, n, C)
        for i in range(geo.N):
            ops.relu_bf16(sv[i, geo.off[0]: geo.off[0] + n], dv[i])

    # ------------------------------------------------------------------------------------------------
    # inference post-processing shared by the heads (layers/common/post_processing.py:50-103)
    # ------------------------------------------------------------------------------------------------
    def inference(self, inputs):
        """One image: its detections as a Container (boxes, box_scores, box_labels), as the reference returns them; a batch of N > 1
        images of one padded shape: the list of the N Containers in batch order (see inference_batch)."""
        outs = self.inference_batch(inputs)
        return outs[0] if len(outs) == 1 else outs

    def _detect_scratch(self, N, Ln, k, select_dims=None):
        """Device scratch of the post-processing chain for N images x Ln levels x top-k: built once per model and (N, Ln, k), reused by
        every call.  select_dims = (rows, K): also bd_det_select's workspace (its size does not depend on them)."""
        cache = self.__dict__.setdefault("_det_scratch", {})
        sc = cache.get((N, Ln, k))
        if sc is None:
            dev = self.device
            i32 = dict(dtype=torch.int32, device=dev)
            f32 = dict(dtype=torch.float32, device=dev)
            C = Ln * k
            max_out = self.cfg.TEST.MAX_BOXES_PER_IMAGE
            sc = cache[(N, Ln, k)] = dict(
                tk_idx=torch.empty((N, Ln, k), **i32), tk_sc=torch.empty((N, Ln, k), **f32), tk_cnt=torch.empty((N, Ln), **i32),
                boxes=torch.empty((N, C, 4), **f32), sc=torch.empty((N, C), **f32), labels=torch.empty((N, C), **i32),
                keep=torch.empty((N, max_out), **i32), num=torch.zeros((N,), **i32),
                nms_ws=torch.empty((ops.nms_batched_workspace_bytes(N, C),), dtype=torch.uint8, device=dev))
        if select_dims is not None and "sel_ws" not in sc:
            sc["sel_ws"] = torch.empty((ops.det_select_workspace_bytes(N, Ln, *select_dims, k),), dtype=torch.uint8, device=self.device)
        return sc

    def _detect(self, N, lvl_rows, K, mode, info, k=1000, logits=None, ctr=None, ctr_ld=1, ctr_off=0, scores=None, anchors=None,
                offsets=None, off_ld=4, A=1, mean=(0, 0, 0, 0), std=(1, 1, 1, 1), item_boxes=None, cls_ld=None):
        """Post-processing of N images in one launch chain.  Per image and level: score > TEST.CLS_THRESHOLD -> top-k (descending) ->
        label = idx % K, box of row idx // K; then batched NMS by label, keep MAX_BOXES_PER_IMAGE, rescale + clip by the image's own
        im_info row.  The candidates come from `logits` (bf16 [N][sum(lvl_rows)][cls_ld or K], one-stage heads: bd_det_select computes the
        scores on the fly and skips a row's pad slots) or from `scores` (fp32 [N][sum(lvl_rows) * K], the RCNN head's softmax).  Everything stays on the device; the only
        host read is the N detection counts.  Returns the list of N Containers."""
        from ..structures import Boxes, Container
        t = self.cfg.TEST
        dev = self.device
        Ln = len(lvl_rows)
        rows = sum(lvl_rows)
        row_off = [0]
        for r in lvl_rows[:-1]:
            row_off.append(row_off[-1] + r)
        s = self._detect_scratch(N, Ln, k, (rows, K) if logits is not None else None)
        if logits is not None:
            ops.det_select(logits, N, rows, K, row_off, lvl_rows, k, t.CLS_THRESHOLD, s["tk_idx"], s["tk_sc"], s["tk_cnt"], s["sel_ws"],
                           ctr=ctr, ctr_ld=ctr_ld, ctr_off=ctr_off, ld=cls_ld)
        else:
            ops.segment_topk(scores, N, rows * K, 1, 1, 0, [r * K for r in row_off], [r * K for r in lvl_rows], k, s["tk_idx"], s["tk_sc"],
                             s["tk_cnt"], min_score=t.CLS_THRESHOLD)
        ops.det_candidates(mode, s["tk_idx"], s["tk_sc"], s["tk_cnt"], N, Ln, k, row_off, K, anchors, offsets,
                           offsets.numel() // N if offsets is not None else 0, off_ld, A, mean, std, item_boxes, rows * K,
                           s["boxes"], s["sc"], s["labels"])
        max_out = t.MAX_BOXES_PER_IMAGE
        s["num"].zero_()
        ops.nms_batched(s["boxes"], s["sc"], s["labels"], t.IOU_THRESHOLD, max_out, s["keep"], s["num"], s["nms_ws"])
        # (the results are the caller's: not part of the cached scratch)
        ob = torch.empty((N, max_out, 4), dtype=torch.float32, device=dev)
        osc = torch.empty((N, max_out), dtype=torch.float32, device=dev)
        ol = torch.empty((N, max_out), dtype=torch.int32, device=dev)
        ops.det_finalize(s["boxes"], s["sc"], s["labels"], s["keep"], s["num"], max_out, info, ob, osc, ol)
        outs = []
        for i, n in enumerate(s["num"].tolist()):
            if n == 0:
                e = torch.zeros((0,))
                outs.append(Container(boxes=e, box_scores=e, box_labels=e))
            else:
                outs.append(Container(boxes=Boxes(ob[i, :n]), box_scores=osc[i, :n], box_labels=ol[i, :n]))
        return outs

    # ------------------------------------------------------------------------------------------------
    # backward (replaces GradManager.backward, solver/default_solver.py:118-124)
    # ------------------------------------------------------------------------------------------------
    def _wgrad(self, conv, x, g, gin, gout, ws, cws=None, x8=None, g8=None):
        self.wgrads.run(conv, x, g, gin, gout, ws, cws, x8, g8)

    def _begin_wgrads(self):
        self.wgrads.begin()

    def _flush_wgrads(self):
        self.wgrads.flush()

    def _join_wgrads(self):
        self.wgrads.join()

    def _norm_backward(self, n, g, gg, pl):
        """g = dL/dz of norm n at geometry gg (the masked gradient of a post-ReLU tensor IS that; an FPN output norm reads a level of
        g_P) -> dgamma / dbeta into the gradient arena and gy = dL/dy (pl.norm_gy, dense), the gradient the convolution's weight and data
        gradient read."""
        y, gy, geo = pl.norm_y[n.name], pl.norm_gy[n.name], pl.norm_geo[n.name]
        ops.bn_bwd_reduce(g, gg, y, geo, n.mean, n.inv_std, n.C, n.g_gamma, n.g_beta, pl.bn_ws)
        return ops.bn_bwd_apply(g, gg, y, geo, n.mean, n.inv_std, n.gamma, n.g_gamma, n.g_beta, n.sums[0], gy, geo, n.C)

    def _block_backward_norm(self, bi, pl, ws, cws):
        """One block of the backbone loop of backward() under a live backbone norm: the same gradient convention and residual fan-out,
        with every convolution's weight and data gradient reading its norm's g_y.  The block-output gradient G feeds bn3's (bn2's)
        backward and the shortcut: the identity add, or downsample.1's backward and the shortcut convolution.  The shortcut's data
        gradient runs as a full-resolution pass (the sparse in-place route of the FrozenBN loop is not taken; the sums are the same)."""
        blk, b = self.blocks[bi], pl.blk[bi]
        convs, ds = blk["convs"], blk["ds"]
        geos = [b.gin] + b.mid_geo + [b.gout]
        xin = pl.blk[bi - 1].out if bi > 0 else pl.pool_out
        G = b.g_out
        g_ds = None
        if ds is not None:
            g_ds = self._norm_backward(ds.norm, G, b.gout, pl)
            self._wgrad(ds, xin, g_ds, b.gin, b.gout, ws)
        g = G
        for ci in range(len(convs) - 1, 0, -1):
            gy = self._norm_backward(convs[ci].norm, g, geos[ci + 1], pl)
            self._wgrad(convs[ci], b.mids[ci - 1], gy, geos[ci], geos[ci + 1], ws)
            convs[ci].dgrad(gy, geos[ci], geos[ci + 1], b.g_mids[ci - 1], mask=b.mids[ci - 1])
            g = b.g_mids[ci - 1]
        gy = self._norm_backward(convs[0].norm, g, geos[1], pl)
        self._wgrad(convs[0], xin, gy, geos[0], geos[1], ws)
        if bi > 0:
            gx = pl.blk[bi - 1].g_out
            tapped = any(pl.res[s] == bi - 1 for s in self.fpn_stages)      # the FPN lateral of res3 / res4 wrote gx first
            if ds is not None:
                ds.dgrad(g_ds, b.gin, b.gout, gx, first=not tapped)
                convs[0].dgrad(gy, geos[0], geos[1], gx, first=False, mask=xin)
            elif tapped:
                ops.add_bf16(gx, G, gx)
                convs[0].dgrad(gy, geos[0], geos[1], gx, first=False, mask=xin)
            else:
                convs[0].dgrad(gy, geos[0], geos[1], gx, add_before=G, mask=xin)      # identity skip: gx = (dgrad + G) * mask
        elif ds is not None:        # dL/d(pool_out): no gate (bd_maxpool3x3s2_bwd applies the stem's)
            ds.dgrad(g_ds, b.gin, b.gout, pl.grad_pool, first=True)
            convs[0].dgrad(gy, geos[0], geos[1], pl.grad_pool, first=False)
        else:
            convs[0].dgrad(gy, geos[0], geos[1], pl.grad_pool, add_before=G)

    def _block_backward(self, bi, pl, ws, cws):
        """One block of the backbone loop of backward() under FrozenBN (folded into the convolutions)."""
        blk, b = self.blocks[bi], pl.blk[bi]
        st = self.fpn_stages
        convs = blk["convs"]
        geos = [b.gin] + b.mid_geo + [b.gout]
        xin = pl.blk[bi - 1].out if bi > 0 else pl.pool_out
        prev_tr = bi > 0 and self.blocks[bi - 1]["trainable"]
        G = b.g_out
        # the shortcut convolution's weight gradient needs only the block's input and output gradient: first in the side
        # stream's queue, not last (after the final block nothing is left on the main stream to hide it)
        if blk["ds"] is not None:
            self._wgrad(blk["ds"], xin, G, b.gin, b.gout, ws)
        # main branch, last conv backwards
        g = G
        # fp8 mode: the e5m2 twin of the block's output gradient, written by the next block's conv1 data gradient (its last writer)
        g8 = b.g_out8 if (b.g_out8 is not None and b.g_out8_ready) else None
        for ci in range(len(convs) - 1, 0, -1):
            # conv2's weight gradient from the twins both neighbours wrote (conv1's forward output, conv3's data gradient)
            wx8 = b.mid8 if (ci == 1 and len(convs) == 3) else None
            self._wgrad(convs[ci], b.mids[ci - 1], g, geos[ci], geos[ci + 1], ws, x8=wx8, g8=g8 if wx8 is not None else None)
            # conv3's (dense 1x1) data gradient also writes the e5m2 twin that conv2's fp8 data gradient reads, conv2's the one
            # conv1's reads
            nxt = None
            if len(convs) == 3:
                nxt = b.g_mid8 if ci == 2 else b.g_mid8a
            if nxt is not None and not convs[ci].dgrad_writes_twin(geos[ci], geos[ci + 1]):
                nxt = None
            wrote = convs[ci].dgrad(g, geos[ci], geos[ci + 1], b.g_mids[ci - 1], mask=b.mids[ci - 1], g8=g8, dx8=nxt,
                                    q_scale=convs[ci - 1].grad_scale)
            g, g8 = b.g_mids[ci - 1], (nxt if wrote else None)
        self._wgrad(convs[0], xin, g, geos[0], geos[1], ws)
        if prev_tr:
            gx = pl.blk[bi - 1].g_out
            xbits = pl.blk[bi - 1].out_bits if ops.dense_1x1_bits_ok(convs[0].desc(geos[0], geos[1])) else None
            # has the input already received a contribution (FPN lateral of res3/res4)?
            tapped = any(pl.res[s] == bi - 1 for s in st)
            # conv1's data gradient is the LAST writer of the previous block's output gradient: it also writes that gradient's e5m2
            # twin (fp8 mode) for the previous block's conv3
            pb = pl.blk[bi - 1]
            gx8 = pb.g_out8
            # ... written with the scale of its consumer, the previous block's conv3 (another scale group at a layer boundary)
            kw = dict(mask=xin, maskbits=xbits, g8=g8, dx8=gx8, q_scale=self.blocks[bi - 1]["convs"][-1].grad_scale)
            if blk["ds"] is not None and gx8 is None and self.sparse_shortcut_grad:
                # conv1 first (writes every pixel, gated), then the stride-2 shortcut adds its gradient IN PLACE at the quarter of
                # the pixels it reaches ((a m + b) m = (a + b) m for a 0 / 1 gate m): instead of a full-resolution tensor that is
                # three quarters zeros being written, read back and summed
                wrote = convs[0].dgrad(g, geos[0], geos[1], gx, first=not tapped, **kw)
                blk["ds"].dgrad(G, b.gin, b.gout, gx, first=False, mask=xin, sparse=True)
            elif blk["ds"] is not None:         # (the last writer must be the launch that can write the e5m2 twin)
                blk["ds"].dgrad(G, b.gin, b.gout, gx, first=not tapped)
                wrote = convs[0].dgrad(g, geos[0], geos[1], gx, first=False, **kw)
            else:
                if tapped:
                    ops.add_bf16(gx, G, gx)
                    wrote = convs[0].dgrad(g, geos[0], geos[1], gx, first=False, **kw)
                else:
                    # identity skip: gx = (dgrad + G) * mask
                    wrote = convs[0].dgrad(g, geos[0], geos[1], gx, add_before=G, **kw)
            pb.g_out8_ready = gx8 is not None and bool(wrote)     # what the launch actually did (a bf16 fallback drops the twin)
        elif bi == 0 and self.stem is not None:
            # dL/d(pool_out): the same residual fan-in, without a gate -- pool_out is a max-pool output, the stem's ReLU gate is
            # applied by bd_maxpool3x3s2_bwd below
            if blk["ds"] is not None:
                blk["ds"].dgrad(G, b.gin, b.gout, pl.grad_pool, first=True)
                convs[0].dgrad(g, geos[0], geos[1], pl.grad_pool, first=False)
            else:                    # BasicBlock, identity shortcut
                convs[0].dgrad(g, geos[0], geos[1], pl.grad_pool, add_before=G)

    def backward(self, on_bucket_ready=None):
        pl = self._cur
        probing = self.fp8_scaler.begin_step()
        self._begin_wgrads()
        ws, cws = pl.wgrad_ws, pl.colsum_ws
        pl.g_P8_ready = False                       # set by a head whose last data gradients wrote the e5m2 twin of dL/dP
        for b in pl.blk:
            b.g_out8_ready = False
        self.head_backward(pl, ws, cws)
        wside = self.streams.wgrad()
        side = (wside,) if wside is not None else ()
        self._flush_wgrads()
        if on_bucket_ready:
            on_bucket_ready("head", side)
        if self.HAS_FPN:
            self._fpn_backward(pl, ws, cws)
            self._flush_wgrads()
            if on_bucket_ready:
                on_bucket_ready("fpn", side)
        self._trunk_backward(pl, ws, cws, on_bucket_ready, side)
        self._join_wgrads()
        self.fp8_scaler.end_step(probing)

    def _fpn_backward(self, pl, ws, cws):
        """From dL/dP (the head wrote g_P) to the masked gradients of res3..res5's outputs."""
        pyr = pl.pyr
        st = self.fpn_stages
        nl = len(st)
        b5 = pl.blk[pl.res[st[-1]]]
        pool_top = self.TOP_BLOCK != "p6p7"
        if not pool_top:
            g6, g7 = pyr.level(nl), pyr.level(nl + 1)
            # P7 = conv(relu(P6)): d P6 = dgrad(g_P7) * (P6 > 0) + g_P6(head), written in place into g_P's P6 level
            # The two dgrads are small grids that only touch the P6/P7 levels of g_P and res5's gradient, which the main stream
            # does not read before the top lateral dgrad below: they run on the auxiliary stream next to the P3.. output-conv dgrads.
            top = self.streams.aux()
            self._wgrad(self.p7, pl.p6_relu, pl.g_P, pl.g_p6r, g7, ws, cws)
            with fork(top):
                self.p7.dgrad(pl.g_P, g6, g7, pl.g_P, mask=pl.P, add_after=pl.g_P)
                self._wgrad(self.p6, b5.out, pl.g_P, b5.gout, g6, ws, cws)
                self.p6.dgrad(pl.g_P, b5.gout, g6, b5.g_out, first=True)
        else:
            ops.subsample2x_bwd_add(pl.g_P, pyr.level(nl), pl.g_P, pyr.level(nl - 1), self.fpn_ch)      # P6 = P5[::2, ::2]
        def lateral_backward(li, g):
            """Weight and data gradient of lateral li from g = dL/d(its convolution's output): g_lat, or what the norm's backward made of it."""
            s = st[li]
            b = pl.blk[pl.res[s]]
            self._wgrad(self.lateral[s], b.out, g, b.gout, b.gout, ws, cws)
            # res_s gradient: first contribution for res3/res4, second (after P6) and final for res5 -> mask there
            if not self.blocks[pl.res[s]]["trainable"]:
                return                                     # res2 of a FREEZE_AT=2 backbone: nothing below needs the gradient
            if li == nl - 1:
                if not pool_top:
                    join(top)
                # (under a live backbone norm the gate bits are not written: bd_bn_apply_act_fwd produces the block output)
                self.lateral[s].dgrad(g, b.gout, b.gout, b.g_out, first=pool_top, mask=b.out,
                                      maskbits=None if self.backbone_norm is not None else b.out_bits)
            else:
                self.lateral[s].dgrad(g, b.gout, b.gout, b.g_out, first=True)

        normed = self.fpn_norm is not None
        if normed:       # dL/d(conv output) of every output convolution first: nothing below reads the P3.. levels of g_P again
            g_out = [self._norm_backward(self.output[s].norm, pl.g_P, pyr.level(li), pl) for li, s in enumerate(st)]
        for li in range(nl):
            s = st[li]
            b = pl.blk[pl.res[s]]
            # the output convolution's gradient: its level of g_P, or (dense) what the norm's backward made of it
            g, gg, g8 = (g_out[li], b.gout, None) if normed else (pl.g_P, pyr.level(li), pl.g_P8 if pl.g_P8_ready else None)
            self._wgrad(self.output[s], pl.lat[s], g, b.gout, gg, ws, cws)
            self.output[s].dgrad(g, b.gout, gg, pl.g_lat[s], first=True, g8=g8)
            if li > 0:   # gradient arriving through the top-down path from the finer level
                sf = st[li - 1]
                if self.fpn_deconv:
                    # fpn_upsample{s} took lat_s to the finer grid: its weight gradient (side stream) reads lat_s and the finished g_lat of
                    # the finer level, its data gradient accumulates onto g_lat_s
                    up, gf = self.upsample[s], pl.blk[pl.res[sf]].gout
                    self._wgrad(up, pl.lat[s], pl.g_lat[sf], gf, b.gout, ws, cws)
                    up.dgrad(pl.g_lat[sf], b.gout, pl.g_lat[s], add=pl.g_lat[s])
                else:
                    ops.upsample2x_add_bwd(pl.g_lat[sf], pl.blk[pl.res[sf]].gout, pl.g_lat[s], b.gout, self.fpn_ch, accumulate=True)
            if not normed:
                lateral_backward(li, pl.g_lat[s])
        if normed:
            # every g_lat is complete (the un-normalised gradient the top-down path read): through the laterals' norms, then their
            # convolutions on the gradient with respect to the convolution's output
            g_lat = [self._norm_backward(self.lateral[s].norm, pl.g_lat[s], pl.blk[pl.res[s]].gout, pl) for s in st]
            for li in range(nl):
                lateral_backward(li, g_lat[li])

    def _trunk_backward(self, pl, ws, cws, on_bucket_ready, side):
        # ---- backbone, last block first.  g_out of a block holds the masked gradient once all consumers are done:
        # res5: done above.  res3/res4 (and every inner block output): the next block's dgrads finish it.
        nb = len(self.blocks)
        for bi in range(nb - 1, -1, -1):
            blk, b = self.blocks[bi], pl.blk[bi]
            if not blk["trainable"]:
                break
            (self._block_backward_norm if self.backbone_norm is not None else self._block_backward)(bi, pl, ws, cws)
            if bi == 0 or self.blocks[bi - 1]["layer"] != blk["layer"]:
                self._flush_wgrads()
                if on_bucket_ready:
                    on_bucket_ready(f"layer{blk['layer']}", side)
        if self.stem is not None:       # FREEZE_AT = 0 (csrc/stem_bwd.hip): through the max-pool and the stem's ReLU, then conv1's weight gradient
            gs = pl.g_stem
            ops.maxpool3x3s2_bwd(pl.grad_pool, pl.stem_out, pl.pool_out, pl.N, gs.H[0], gs.W[0], 64, pl.grad_stem)
            g_stem = pl.grad_stem
            if self.stem.norm is not None:     # grad_stem is dL/dz of bn1 (gated by stem_out > 0): through the norm, no folded row scale
                g_stem = self._norm_backward(self.stem.norm, pl.grad_stem, gs, pl)
            self._wgrad(self.stem, pl.x_halo, g_stem, pl.g_image, gs, ws)
            self._flush_wgrads()
            if on_bucket_ready:
                on_bucket_ready("conv1", side)

