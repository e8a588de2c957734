"""basedet.layers.Conv2d(bias=False, norm="BN", activation="silu") and YOLOXHead (layers/head/yolo_head.py:35-121) on the HIP kernels: the
operator every YOLOX convolution ends in, and the decoupled head that writes the layout csrc/yolox.hip reads.

Calling convention of layers/center_head.py: `layer(x)` takes and returns NCHW fp32 DEVICE tensors (a host tensor raises BasedetHipError:
no CPU fallback); `forward_pm` / `backward_pm` on pixel-major bf16; `params()` (fp32 device masters by name, views an optimizer may update
in place) / `repack()` / `grads()` (copies); strict `state_dict()` / `load_state_dict()` under the reference's names; `train()` /
`eval()`.  Storage as in center_head.py: ConvBNSiLU and the predictors each hold a layers/_pm.py ParamStore (masters in the kernels'
layouts, loaded in place; `adopt()` onto a model arena, models/yolox.py YOLOX, is its move()), and YOLOXHead is a _pm.py Container of
them.  The norm is layers/batch_norm.py BatchNormAct("silu").

ConvBNSiLU = bd_conv2d_fwd (no bias, no epilogue) -> bd_bn_stats_fwd -> bd_bn_silu_fwd; backward = bd_bn_silu_bwd_reduce ->
bd_bn_silu_bwd_apply -> bd_conv2d_wgrad + bd_conv2d_dgrad.  The SiLU gate is recomputed from the pre-norm tensor inside the norm's two
backward passes (csrc/batchnorm.hip): no gate pass, no gated-gradient tensor, and the forward output is not kept for the backward.
eps 1e-3 and momentum 0.03 are YOLOXConfig's BN_EPS and BN_MOMENTUM = 0.97 (MegEngine's convention; bd_bn_stats_fwd takes torch's).

YOLOXHead.forward_pm returns (cls bf16 [N P][round_up(K, 8)], box_obj bf16 [N P][8]: raw reg 0-3, obj logit 4): the P points of an image
level after level, row-major inside a level.  The predictors write their level's rows IN PLACE through a level geometry on the output
side of the convolution descriptor -- no repack, no concatenation.  cls_preds[l] keeps K real rows padded to round_up(K, 8) (pad rows of
weight, bias and gradients are zero and stay zero: models/engine.py PaddedClsConv's invariant); reg_preds[l] and obj_preds[l] are ONE
8-row launch over reg_feat (rows 0-3 reg, 4 obj, 5-7 zero: FusedPredConv's precedent).  The stem output receives the sum of both towers'
data gradients through the accumulating dgrad (BD_EPI_ADD_BEFORE in place), not through an add pass.

The first blocks of the two towers read the same stem output but run as TWO launches each: the convolution and norm entries address
[rows][C] tensors without a channel stride, so the halves of a fused [rows][2 mid] output could not feed the second blocks without a
split pass.

Reproducibility: every forward output, and everything the backward writes, is bitwise reproducible."""
import math

import numpy as np
import torch

from .. import ops
from ._pm import BF16, Container, ParamStore, cut, load_strict, need_device, round_up8, to_nchw, to_pm, workspace
from .batch_norm import BatchNormAct

__all__ = ["ConvBNSiLU", "YOLOXHead"]

BN_EPS, BN_MOMENTUM = 1e-3, 0.03


def validate_conv(cin, cout, k, stride):
    """What the bf16 convolution entries and the norm kernels take; ValueError before the device is touched."""
    if k not in (1, 3):
        raise ValueError(f"ConvBNSiLU: kernel size {k!r} is not built (1 or 3)")
    if stride not in (1, 2):
        raise ValueError(f"ConvBNSiLU: stride {stride!r} is not built (1 or 2)")
    for name, c in (("cin", cin), ("cout", cout)):
        if not (isinstance(c, int) and c > 0 and c % 8 == 0):
            raise ValueError(f"ConvBNSiLU: {name}={c!r} must be a positive multiple of 8 (bd_conv2d_*, bd_bn_*)")


def conv_param_shapes(cin, cout, k):
    """name -> shape of one ConvBNSiLU's state, in the reference's order."""
    out = {"weight": (cout, cin, k, k)}
    out.update({f"norm.{n}": (cout,) for n in BatchNormAct.KEYS})
    return out


def head_param_shapes(num_classes, in_channels, mid_channels):
    """name -> shape of a YOLOXHead's state, in the reference's order (the module lists in the order the constructor creates them)."""
    K, mid, out = num_classes, mid_channels, {}
    for l, c in enumerate(in_channels):
        out.update({f"stems.{l}.{k}": v for k, v in conv_param_shapes(c, mid, 1).items()})
    for tower, pred, rows in (("cls_convs", ("cls_preds",), (K,)), ("reg_convs", ("reg_preds", "obj_preds"), (4, 1))):
        for l in range(len(in_channels)):
            for i in range(2):
                out.update({f"{tower}.{l}.{i}.{k}": v for k, v in conv_param_shapes(mid, mid, 3).items()})
        for p, r in zip(pred, rows):
            for l in range(len(in_channels)):
                out[f"{p}.{l}.weight"] = (r, mid, 1, 1)
                out[f"{p}.{l}.bias"] = (r,)
    return out


class ConvBNSiLU:
    """The reference's Conv2d(cin, cout, k, stride, padding=k // 2, bias=False, norm="BN", activation="silu")."""
    NORMS = ("norm",)

    def __init__(self, cin, cout, k, stride=1, seed=0, eps=BN_EPS, momentum=BN_MOMENTUM, device="cuda"):
        validate_conv(cin, cout, k, stride)
        self.cin, self.cout, self.k, self.stride, self.pad = cin, cout, k, stride, k // 2
        self.eps, self.momentum, self.device, self.training = float(eps), float(momentum), torch.device(device), True
        rng = np.random.default_rng(seed)
        # M.Conv2d's default init as layers/center_head.py SingleHead takes it: N(0, sqrt(1 / fan_in)); the master is OHWI, what
        # bd_weight_pack reads and bd_conv2d_wgrad writes
        w = (rng.standard_normal((cout, cin, k, k)) * math.sqrt(1.0 / (cin * k * k))).astype(np.float32)
        self._store = ParamStore({"weight": (cout, k, k, cin)}, self.device)
        self._store.w["weight"].copy_(torch.from_numpy(w).permute(0, 2, 3, 1))
        self.norm = BatchNormAct(cout, "silu", self.eps, self.momentum, self.device)
        self._wf = torch.empty((cout, k * k, cin), dtype=BF16, device=self.device)
        self._wd = torch.empty((cin, k * k, cout), dtype=BF16, device=self.device)
        self._saved = None
        self.repack()

    mean = property(lambda self: self.norm.mean)          # the batch statistics of the last training forward
    inv_std = property(lambda self: self.norm.inv_std)
    sums = property(lambda self: self.norm.sums)

    # ---- parameters ------------------------------------------------------------------------------------------------------------------------
    def _shapes(self):
        return conv_param_shapes(self.cin, self.cout, self.k)

    def names(self):
        return list(self._shapes())

    def params(self):
        """The trainable fp32 device masters by name (weight: the OIHW view of the OHWI master)."""
        return {"weight": self._store.w["weight"].permute(0, 3, 1, 2), "norm.weight": self.norm.p["weight"], "norm.bias": self.norm.p["bias"]}

    def pack_entry(self):
        """ops.weight_pack's arguments, and this layer's entry of a model's pack table (ops.build_pack_table)."""
        return self._store.w["weight"], None, self._wf, self._wd, self.cout, self.k * self.k, self.cin

    def repack(self):
        ops.weight_pack(*self.pack_entry())

    def refresh_eval(self):
        self.norm.refresh_eval()

    def arena_shapes(self):
        """name -> shape of the fp32 master in the kernels' layout (OHWI).  The norm's vectors are not listed: adopt() takes a norm record."""
        return dict(self._store.shapes)

    def adopt(self, w, g, norm_state):
        """Live on the caller's storage (a model's parameter arena): w / g = {"weight": fp32 view of arena_shapes()}, norm_state the
        model's norm record (BatchNormAct.adopt).  The current values move in; the same path on other storage (center_head.py adopt)."""
        self._store.move(w, g)
        self.norm.adopt(norm_state)
        self.repack()

    def state_dict(self):
        return {"weight": self._store.w["weight"].permute(0, 3, 1, 2).contiguous().cpu(), **self.norm.state("norm.")}

    def load_state_dict(self, state):
        p = load_strict(state, self._shapes(), self.device)
        self._store.w["weight"].copy_(p["weight"].permute(0, 2, 3, 1))
        self.norm.load(p, "norm.")
        self.repack()

    def train(self, mode=True):
        self.training = self.norm.training = bool(mode)
        if not self.training:
            self.refresh_eval()
        return self

    def eval(self):
        return self.train(False)

    def grads(self):
        """Copies, not views of the storage the next backward writes."""
        if self._store.g is None:
            raise RuntimeError("grads() before a backward")
        return {"weight": self._store.g["weight"].permute(0, 3, 1, 2).clone(memory_format=torch.contiguous_format),
                "norm.weight": self.norm.g["weight"].clone(), "norm.bias": self.norm.g["bias"].clone()}

    # ---- forward / backward ------------------------------------------------------------------------------------------------------------------
    def out_size(self, H, W):
        return (H + 2 * self.pad - self.k) // self.stride + 1, (W + 2 * self.pad - self.k) // self.stride + 1

    def forward_pm(self, x, N, H, W):
        """x bf16 [N H W][cin] -> bf16 [N Ho Wo][cout]; the pre-norm tensor stays in `self.y_pm` until the next forward."""
        if tuple(x.shape) != (N * H * W, self.cin) or x.dtype != BF16:
            raise ValueError(f"forward_pm: expected bf16 {(N * H * W, self.cin)}, got {x.dtype} {tuple(x.shape)}")
        Ho, Wo = self.out_size(H, W)
        gin, gout = ops.single(N, H, W), ops.single(N, Ho, Wo)
        d = ops.conv_desc(gin, gout, self.cin, self.cout, self.k, self.k, self.stride, self.pad)
        y = torch.empty((N * Ho * Wo, self.cout), dtype=BF16, device=self.device)
        ops.conv2d_fwd(d, x, self._wf, None, y)
        z = self.norm.forward_pm(y, N, Ho, Wo)          # (the norm keeps y for its backward: the same tensor as y_pm)
        self._saved = (x, d, self.training)
        self.y_pm = y
        return z

    def backward_pm(self, g, accumulate=False, dx=None, add=None, need_dx=True):
        """g bf16 [N Ho Wo][cout] -> the data gradient bf16 [N H W][cin]: a new tensor, or ADDED onto `dx` in place where one is given (the
        second reader of a shared input).  accumulate=True adds the parameter gradients onto those of the previous backward.  add: a
        bf16 [N H W][cin] gradient the input received from another reader; the NEW tensor returned is the sum and `add` keeps its bits.
        need_dx=False: no data gradient (the input is the image); returns None."""
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        x, d, training = self._saved
        if not training:
            raise RuntimeError("backward() through a norm in eval() mode is not built")
        M, C = self.y_pm.shape
        if tuple(g.shape) != (M, C) or g.dtype != BF16:
            raise ValueError(f"backward_pm: expected bf16 {(M, C)}, got {g.dtype} {tuple(g.shape)}")
        gy = self.norm.backward_pm(g, accumulate)
        gr, accumulate = self._store.grad(accumulate)
        ops.conv2d_wgrad(d, x, gy, gr["weight"], workspace(ops.conv2d_wgrad_workspace_bytes(d), self.device), accumulate=accumulate)
        if add is not None and (dx is not None or tuple(add.shape) != tuple(x.shape) or add.dtype != BF16):
            raise ValueError(f"backward_pm: add must be bf16 {tuple(x.shape)}, and is given without dx")
        if not need_dx:
            dx = None
        elif add is not None:
            dx = ops.conv2d_dgrad(d, gy, self._wd, torch.empty_like(x), add=add, flags=ops.EPI_ADD_BEFORE)
        elif dx is None:
            dx = ops.conv2d_dgrad(d, gy, self._wd, torch.empty_like(x))
        else:
            if tuple(dx.shape) != tuple(x.shape) or dx.dtype != BF16:
                raise ValueError(f"backward_pm: dx must be bf16 {tuple(x.shape)}")
            ops.conv2d_dgrad(d, gy, self._wd, dx, add=dx, flags=ops.EPI_ADD_BEFORE)
        self.gy_pm = gy
        return dx

    def __call__(self, x):
        need_device(x, "ConvBNSiLU")
        N, C, H, W = x.shape
        if C != self.cin:
            raise ValueError(f"input has {C} channels, the layer {self.cin}")
        self._in_size = (N, H, W)
        return to_nchw(self.forward_pm(to_pm(x), N, H, W), N, *self.out_size(H, W))

    forward = __call__

    def backward(self, dy, accumulate=False):
        need_device(dy, "ConvBNSiLU.backward")
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        N, H, W = self._in_size
        if tuple(dy.shape) != (N, self.cout, *self.out_size(H, W)):
            raise ValueError(f"gradient shape {tuple(dy.shape)} does not match the forward output")
        return to_nchw(self.backward_pm(to_pm(dy), accumulate), N, H, W)


class _PredConv:
    """A 1x1 predictor with bias whose `rows` real output rows are padded to `ld` (a multiple of 8) and written in place into one level of
    a [N P][ld] tensor.  The masters are the padded (ld, 1, 1, cin) weight and (ld,) bias; rows >= `rows` are zero and stay zero."""

    NORMS = ()

    def __init__(self, cin, rows, ld, rng, device):
        self.cin, self.rows, self.ld, self.device = cin, rows, ld, device
        w = np.zeros((ld, 1, 1, cin), np.float32)
        w[:rows, 0, 0] = rng.standard_normal((rows, cin)) * math.sqrt(1.0 / cin)
        self._store = ParamStore({"weight": (ld, 1, 1, cin), "bias": (ld,)}, device)
        self._store.w["weight"].copy_(torch.from_numpy(w))
        self.wf = torch.empty((ld, 1, cin), dtype=BF16, device=device)
        self.wd = torch.empty((cin, 1, ld), dtype=BF16, device=device)

    # The layer protocol on the padded masters; YOLOXHead presents them under the reference's names (_pred_views).
    def _shapes(self):
        return dict(self._store.shapes)

    arena_shapes = _shapes          # (the state is the padded masters themselves)

    def names(self):
        return list(self._store.shapes)

    def params(self):
        return dict(self._store.w)

    def grads(self):
        return {k: v.clone() for k, v in self._store.g.items()}

    def state_dict(self):
        return {k: v.detach().cpu() for k, v in self._store.w.items()}

    def load_state_dict(self, state):
        p = load_strict(state, self._store.shapes, self.device)
        for k, v in self._store.w.items():
            v.copy_(p[k])
        self.repack()

    def pack_entry(self):
        return self._store.w["weight"], None, self.wf, self.wd, self.ld, 1, self.cin

    def repack(self):
        ops.weight_pack(*self.pack_entry())

    def adopt(self, w, g):
        """Live on the caller's storage: w / g = {"weight", "bias"} fp32 views of the padded masters (ConvBNSiLU.adopt)."""
        self._store.move(w, g)
        self.repack()

    def refresh_eval(self):
        pass

    def train(self, mode=True):
        return self

    def desc(self, N, H, W, off, P):
        return ops.conv_desc(ops.single(N, H, W), ops.Geom(N, [H], [W], [off], P), self.cin, self.ld, 1, 1, 1, 0)

    def forward(self, d, x, out):
        ops.conv2d_fwd(d, x, self.wf, self._store.w["bias"], out)

    def backward(self, d, x, g, accumulate):
        gr, accumulate = self._store.grad(accumulate)
        ops.conv2d_wgrad_bias(d, x, g, gr["weight"], gr["bias"], workspace(ops.conv2d_wgrad_bias_workspace_bytes(d), self.device),
                              accumulate=accumulate)
        return ops.conv2d_dgrad(d, g, self.wd, torch.empty_like(x))


class YOLOXHead(Container):
    """yolo_head.py:35-121.  Its children are the stems, the tower blocks and the padded predictors; the reference's predictor names
    (cls_preds / reg_preds / obj_preds, real rows only) are views of the padded ones (_pred_views)."""

    def __init__(self, num_classes, in_channels=(256, 512, 1024), mid_channels=256, act="silu", depthwise=False, prior_prob=0.01, seed=0,
                 device="cuda"):
        if act != "silu":
            raise ValueError(f"YOLOXHead: act={act!r} is not built (the fused norm kernels are SiLU's)")
        if depthwise:
            raise ValueError("YOLOXHead: depthwise=True is not built (DepthwiseConvBlock)")
        if not (isinstance(num_classes, int) and num_classes >= 1):
            raise ValueError(f"YOLOXHead: num_classes={num_classes!r}")
        in_channels = list(in_channels)
        if not 1 <= len(in_channels) <= ops._lib.BD_MAX_SEGS:
            raise ValueError(f"YOLOXHead: 1 to {ops._lib.BD_MAX_SEGS} levels")
        for c in in_channels:          # every layer is validated before any of them touches the device
            validate_conv(c, mid_channels, 1, 1)
        validate_conv(mid_channels, mid_channels, 3, 1)
        K, mid = num_classes, mid_channels
        self.num_anchors, self.num_classes, self.prior_prob = 1, K, prior_prob
        self.in_channels, self.mid_channels, self.device, self.training = in_channels, mid, torch.device(device), True
        self.cls_ld = round_up8(K)
        self.stems, self.cls_convs, self.reg_convs, self.cls_preds, self.regobj_preds = [], [], [], [], []
        bias_value = -math.log((1 - prior_prob) / prior_prob)
        for l, c in enumerate(in_channels):
            s = seed + 16 * l
            self.stems.append(ConvBNSiLU(c, mid, 1, seed=s, device=device))
            self.cls_convs.append([ConvBNSiLU(mid, mid, 3, seed=s + 1 + i, device=device) for i in range(2)])
            self.reg_convs.append([ConvBNSiLU(mid, mid, 3, seed=s + 3 + i, device=device) for i in range(2)])
            rng = np.random.default_rng(s + 5)
            cp, rp = _PredConv(mid, K, self.cls_ld, rng, self.device), _PredConv(mid, 5, 8, rng, self.device)
            cp._store.w["bias"][:K] = bias_value
            rp._store.w["bias"][4] = bias_value
            self.cls_preds.append(cp)
            self.regobj_preds.append(rp)
        self._saved = None
        self.repack()

    # ---- parameters ------------------------------------------------------------------------------------------------------------------------
    def _children(self):
        """The blocks in the reference's order, then per level the padded class predictor and the fused reg + obj predictor (reg 0-3,
        obj 4, 5-7 zero).  arena_shapes() lists them in this order: every block's OHWI weight, then the predictors' padded weights and
        biases."""
        L = range(len(self.in_channels))
        out = [(f"stems.{l}", self.stems[l]) for l in L]
        out += [(f"cls_convs.{l}.{i}", self.cls_convs[l][i]) for l in L for i in range(2)]
        out += [(f"reg_convs.{l}.{i}", self.reg_convs[l][i]) for l in L for i in range(2)]
        return out + [(f"cls_preds.{l}", self.cls_preds[l]) for l in L] + [(f"regobj_preds.{l}", self.regobj_preds[l]) for l in L]

    def _shapes(self):
        return head_param_shapes(self.num_classes, self.in_channels, self.mid_channels)

    def _pred_views(self, d):
        """The reference's predictor tensors as views of the padded ones in d, a dict by the children's names."""
        K, mid, out = self.num_classes, self.mid_channels, {}
        for wb, shape in (("weight", lambda r: (r, mid, 1, 1)), ("bias", lambda r: (r,))):
            for l in range(len(self.in_channels)):
                c, r = d[f"cls_preds.{l}.{wb}"], d[f"regobj_preds.{l}.{wb}"]
                out[f"cls_preds.{l}.{wb}"] = c[:K].view(shape(K))
                out[f"reg_preds.{l}.{wb}"] = r[0:4].view(shape(4))
                out[f"obj_preds.{l}.{wb}"] = r[4:5].view(shape(1))
        return out

    def _ordered(self, d):
        """d by the children's names -> by the reference's names, in its order."""
        d = {**d, **self._pred_views(d)}
        return {k: d[k] for k in self._shapes() if k in d}

    def params(self):
        return self._ordered(super().params())

    def grads(self):
        return self._ordered(super().grads())

    def state_dict(self):
        return self._ordered(super().state_dict())

    def load_state_dict(self, state):
        """Strict, under the reference's names; the predictors load their padded tensors: the real rows from `state`, pad rows zero."""
        p = load_strict(state, self._shapes(), self.device)
        padded = {k: torch.zeros_like(v) for k, v in super().params().items() if "_preds." in k}
        for k, v in self._pred_views(padded).items():
            v.copy_(p[k])
        p.update(padded)
        for n, c in self._children():
            c.load_state_dict(cut(p, n))

    # ---- forward / backward ------------------------------------------------------------------------------------------------------------------
    def forward_pm(self, feats, N, sizes):
        """feats: per level bf16 [N H_l W_l][C_l]; sizes [(H_l, W_l)] -> (cls bf16 [N P][round_up(K, 8)], box_obj bf16 [N P][8])."""
        if len(feats) != len(self.in_channels) or len(sizes) != len(feats):
            raise ValueError(f"forward_pm: {len(self.in_channels)} levels expected")
        P = sum(h * w for h, w in sizes)
        cls = torch.empty((N * P, self.cls_ld), dtype=BF16, device=self.device)
        box_obj = torch.empty((N * P, 8), dtype=BF16, device=self.device)
        saved, off = [], 0
        for l, (x, (H, W)) in enumerate(zip(feats, sizes)):
            s = self.stems[l].forward_pm(x, N, H, W)
            cf = self.cls_convs[l][1].forward_pm(self.cls_convs[l][0].forward_pm(s, N, H, W), N, H, W)
            rf = self.reg_convs[l][1].forward_pm(self.reg_convs[l][0].forward_pm(s, N, H, W), N, H, W)
            dc, dr = self.cls_preds[l].desc(N, H, W, off, P), self.regobj_preds[l].desc(N, H, W, off, P)
            self.cls_preds[l].forward(dc, cf, cls)
            self.regobj_preds[l].forward(dr, rf, box_obj)
            saved.append((cf, rf, dc, dr))
            off += H * W
        self._saved = (saved, N, [tuple(s) for s in sizes], P)
        self.cls_pm, self.box_obj_pm = cls, box_obj
        return cls, box_obj

    def backward_pm(self, d_cls, d_box_obj, accumulate=False):
        """d_cls bf16 [N P][round_up(K, 8)], d_box_obj bf16 [N P][8] (what ops.yolox_loss_fwd_bwd writes: the pad slots hold zero) -> the
        per-level d_feats bf16 [N H_l W_l][C_l]."""
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        saved, N, sizes, P = self._saved
        if tuple(d_cls.shape) != (N * P, self.cls_ld) or tuple(d_box_obj.shape) != (N * P, 8) or d_cls.dtype != BF16 or d_box_obj.dtype != BF16:
            raise ValueError(f"backward_pm: expected bf16 {(N * P, self.cls_ld)} and {(N * P, 8)}")
        d_feats = []
        for l, (cf, rf, dc, dr) in enumerate(saved):
            g = self.cls_preds[l].backward(dc, cf, d_cls, accumulate)
            g = self.cls_convs[l][1].backward_pm(g, accumulate)
            d_stem = self.cls_convs[l][0].backward_pm(g, accumulate)
            g = self.regobj_preds[l].backward(dr, rf, d_box_obj, accumulate)
            g = self.reg_convs[l][1].backward_pm(g, accumulate)
            self.reg_convs[l][0].backward_pm(g, accumulate, dx=d_stem)          # the stem output's gradient: cls tower + reg tower
            d_feats.append(self.stems[l].backward_pm(d_stem, accumulate))
        return d_feats

    def __call__(self, feats):
        for x in feats:
            need_device(x, "YOLOXHead")
        N = int(feats[0].shape[0])
        for x, c in zip(feats, self.in_channels):
            if x.dim() != 4 or x.shape[1] != c or x.shape[0] != N:
                raise ValueError(f"YOLOXHead: level input {tuple(x.shape)}, expected (N, {c}, H, W)")
        sizes = [(int(x.shape[2]), int(x.shape[3])) for x in feats]
        cls, box_obj = self.forward_pm([to_pm(x) for x in feats], N, sizes)
        K, P = self.num_classes, sum(h * w for h, w in sizes)
        c3, b3 = cls.view(N, P, -1), box_obj.view(N, P, 8)
        logits, offsets, objs, p0 = [], [], [], 0
        for h, w in sizes:
            logits.append(to_nchw(c3[:, p0:p0 + h * w, :K], N, h, w))
            offsets.append(to_nchw(b3[:, p0:p0 + h * w, 0:4], N, h, w))
            objs.append(to_nchw(b3[:, p0:p0 + h * w, 4:5], N, h, w))
            p0 += h * w
        return logits, offsets, objs

    forward = __call__

    def backward(self, d_logits, d_offsets, d_objs, accumulate=False):
        """Gradients with respect to the three returned lists -> the per-level d_feats, NCHW fp32."""
        for t in (*d_logits, *d_offsets, *d_objs):
            need_device(t, "YOLOXHead.backward")
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        _, N, sizes, P = self._saved
        K = self.num_classes
        d_cls = torch.zeros((N, P, self.cls_ld), dtype=BF16, device=self.device)
        d_bo = torch.zeros((N, P, 8), dtype=BF16, device=self.device)
        p0 = 0
        for (h, w), gl, go, gb in zip(sizes, d_logits, d_offsets, d_objs):
            if tuple(gl.shape) != (N, K, h, w) or tuple(go.shape) != (N, 4, h, w) or tuple(gb.shape) != (N, 1, h, w):
                raise ValueError("YOLOXHead.backward: gradient shapes do not match the forward outputs")
            d_cls[:, p0:p0 + h * w, :K] = gl.permute(0, 2, 3, 1).reshape(N, h * w, K)
            d_bo[:, p0:p0 + h * w, 0:4] = go.permute(0, 2, 3, 1).reshape(N, h * w, 4)
            d_bo[:, p0:p0 + h * w, 4] = gb.reshape(N, h * w)
            p0 += h * w
        d_feats = self.backward_pm(d_cls.view(N * P, -1), d_bo.view(N * P, 8), accumulate)
        return [to_nchw(g, N, h, w) for g, (h, w) in zip(d_feats, sizes)]
