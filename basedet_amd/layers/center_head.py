"""basedet.layers.DeconvLayer / CenternetDeconv / SingleHead / CenterHead (layers/head/center_head.py) on the HIP kernels: CenterNet's
deconvolution neck (res5 -> a stride-4 map) and its three-branch head, as layers that train.

Calling convention of layers/deformable.py: `layer(x)` takes and returns NCHW fp32 DEVICE tensors (a host tensor raises BasedetHipError: no
CPU fallback); `backward(dy, accumulate=False)`; `grads()`, `state_dict()` / `load_state_dict()` (strict names and shapes) under the
reference's names; `train()` / `eval()`.  On top of it:
  * the pixel-major path: `forward_pm(x_pm, N, H, W)` / `backward_pm(g_pm)` on bf16 [N H W][C]; the NCHW methods are thin wrappers, and a
    neck (or a model) chains the stages with no NCHW / fp32 round trip in between;
  * `params()` returns the fp32 device masters by name (the state_dict's layouts), `repack()` rebuilds the bf16 operands after they were
    changed in place: an optimizer step needs no host round trip.

DeconvLayer = dcn -> dcn_bn -> ReLU -> up_sample -> up_bn -> ReLU.  The norms run on csrc/batchnorm.hip (eps 1e-5, momentum 0.1 in torch's
convention, running statistics updated in train(); in eval() the same apply launch is fed running_mean and 1 / sqrt(running_var + eps)),
up_sample on bd_fpn_deconv_* with add = NULL.  Only deconv_kernel = 4, stride 2, pad 1, out_pad 0 and output channels in multiples of 64
are built; anything else raises ValueError before the device is touched.

up_sample.weight has M.ConvTranspose2d's (in, out, 4, 4) shape.  The kernels' fp32 master is the (C_coarse, C_fine, 4, 4) conv view of
DESIGN.md 4f in OHWI: master[ci][kh][kw][co] = weight[ci][co][kh][kw], i.e. weight.permute(0, 2, 3, 1) -- `in` of the transposed
convolution is the coarse side.  init_module is reproduced as written, quirk included: after the default N(0, sqrt(1 / (16 C))) init,
weight[c, 0, :, :] is set to the bilinear stencil for every c -- only OUTPUT channel 0 gets it.

CenterHead packs the three feat_convs as one 3C-row 3x3 convolution (EPI_RELU) and runs the fused output kernel (csrc/center_head.hip);
`logits_pm` [M][round_up(K, 8)] and `wr_pm` [M][8] keep its raw outputs for ops.centernet_*; `backward_pm(d_logits_pm, d_wr_pm)` is the
training path.

Reproducibility: every forward output, and everything the head's backward writes, is bitwise reproducible.  Neck gradients downstream of a
deformable convolution's d_x are not (fp32 atomics in bd_deform_conv_bwd_data): they hold their bounds, not their bits.

Storage, as in deformable.py (layers/_pm.py ParamStore): fp32 masters in the kernels' layouts and the bf16 operands are allocated once;
params() hands out views under the reference's names, load_state_dict() copies into them, repack() packs in place, grads() returns
copies.  adopt() moves a layer onto a model's parameter arena and norm records -- the same path on other storage.  The activations are
the layers' own; the plan arena, the wgrad side stream, optimizers and EMA belong to the model."""
import math

import numpy as np
import torch

from .. import ops
from ._pm import BF16, F32, Container, ParamStore, cut, load_strict, need_device, round_up8, to_nchw, to_pm, workspace
from .batch_norm import BatchNormAct
from .deformable import DeformConvWithOff, ModulatedDeformConvWithOff

__all__ = ["DeconvLayer", "CenternetDeconv", "SingleHead", "CenterHead"]

BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def bilinear_stencil(k):
    """DeconvLayer.init_module's (k, k) stencil."""
    f = math.ceil(k / 2)
    c = (2 * f - 1 - f % 2) / (2.0 * f)
    v = np.asarray([1 - math.fabs(i / f - c) for i in range(k)])
    return v[:, None] * v[None, :]


def _validate_deconv(in_planes, out_planes, deconv_kernel, deconv_stride, deconv_pad, deconv_out_pad):
    got = dict(deconv_kernel=deconv_kernel, deconv_stride=deconv_stride, deconv_pad=deconv_pad, deconv_out_pad=deconv_out_pad)
    want = dict(deconv_kernel=4, deconv_stride=2, deconv_pad=1, deconv_out_pad=0)
    for k, v in want.items():
        if got[k] != v:
            raise ValueError(f"DeconvLayer: only {want} is built (bd_fpn_deconv_*); got {k}={got[k]!r}")
    if not (isinstance(out_planes, int) and out_planes > 0 and out_planes % 64 == 0):
        raise ValueError(f"DeconvLayer: out_planes={out_planes!r} must be a positive multiple of 64 (bd_fpn_deconv_*)")
    if not (isinstance(in_planes, int) and in_planes > 0 and in_planes % 8 == 0):
        raise ValueError(f"DeconvLayer: in_planes={in_planes!r} must be a positive multiple of 8")


def up_sample_init(C, rng):
    """up_sample.weight (in, out, 4, 4) as DeconvLayer leaves it: M.ConvTranspose2d's default N(0, sqrt(1 / fan_in)), fan_in = 16 C, then
    init_module as written -- weight[c, 0, :, :] = the bilinear stencil for every c (output channel 0 only)."""
    w = rng.standard_normal((C, C, 4, 4)) * math.sqrt(1.0 / (16 * C))
    w[:, 0, :, :] = bilinear_stencil(4)
    return w.astype(np.float32)


def deconv_param_shapes(in_planes, out_planes, modulate_deform):
    """name -> shape of one DeconvLayer's state, in the reference's order."""
    cls = ModulatedDeformConvWithOff if modulate_deform else DeformConvWithOff
    k, C = (27 if cls.MODULATED else 18), out_planes
    want = {f"dcn.{cls.OFFSET_NAME}.weight": (k, in_planes, 3, 3), f"dcn.{cls.OFFSET_NAME}.bias": (k,),
            f"dcn.{cls.DCN_NAME}.weight": (C, in_planes, 3, 3), f"dcn.{cls.DCN_NAME}.bias": (C,)}
    want.update({f"dcn_bn.{k}": (C,) for k in BatchNormAct.KEYS})
    want["up_sample.weight"] = (C, C, 4, 4)
    want.update({f"up_bn.{k}": (C,) for k in BatchNormAct.KEYS})
    return want


def neck_param_shapes(channels, modulate_deform):
    return {f"deconv{i + 1}.{k}": v for i in range(len(channels) - 1)
            for k, v in deconv_param_shapes(channels[i], channels[i + 1], modulate_deform).items()}


def head_param_shapes(in_channels, num_classes):
    C = in_channels
    return {f"{b}_head.{k}": v for b, n in (("cls", num_classes), ("wh", 2), ("reg", 2))
            for k, v in (("feat_conv.weight", (C, C, 3, 3)), ("feat_conv.bias", (C,)), ("out_conv.weight", (n, C, 1, 1)), ("out_conv.bias", (n,)))}


class DeconvLayer:
    """center_head.py:13-63."""
    NORMS = ("dcn_bn", "up_bn")

    def __init__(self, in_planes, out_planes, deconv_kernel, deconv_stride=2, deconv_pad=1, deconv_out_pad=0, modulate_deform=True, seed=0,
                 device="cuda"):
        _validate_deconv(in_planes, out_planes, deconv_kernel, deconv_stride, deconv_pad, deconv_out_pad)
        self.in_planes, self.out_planes, self.device = in_planes, out_planes, torch.device(device)
        C = out_planes
        cls = ModulatedDeformConvWithOff if modulate_deform else DeformConvWithOff
        self.dcn = cls(in_planes, out_planes, kernel_size=3, deformable_groups=1, seed=seed, device=device)
        self.dcn_bn, self.up_bn = (BatchNormAct(C, "relu", BN_EPS, BN_MOMENTUM, self.device) for _ in range(2))
        self.modulate_deform = bool(modulate_deform)
        self._store = ParamStore({"up_sample.weight": (C, 4, 4, C)}, self.device)
        self._up_wf, self._up_wd = (torch.empty(16 * C * C, dtype=BF16, device=self.device) for _ in range(2))
        # M.ConvTranspose2d's default init: N(0, sqrt(1 / fan_in)), fan_in = 16 C; then init_module
        self._up_w().copy_(torch.from_numpy(up_sample_init(C, np.random.default_rng(seed + 1))))
        self._saved = None
        self.training = True
        self.repack()

    def _up_w(self):
        """up_sample.weight as M.ConvTranspose2d has it, (in, out, 4, 4): a view of the OHWI master."""
        return self._store.w["up_sample.weight"].permute(0, 3, 1, 2)

    def arena_shapes(self):
        """name -> shape of the fp32 masters in the kernels' layouts (deformable.py arena_shapes; up_sample.weight as the OHWI conv view
        (C, 4, 4, C) that bd_fpn_deconv_pack reads and bd_fpn_deconv_wgrad writes).  The norms' vectors are not listed: adopt() takes a
        norm record for each."""
        C = self.out_planes
        out = {"dcn." + k: v for k, v in self.dcn.arena_shapes().items()}
        out["up_sample.weight"] = (C, 4, 4, C)
        return out

    def adopt(self, w, g, dcn_bn, up_bn):
        """Live on the caller's storage (a model's parameter arena): w / g = {name: fp32 view} in arena_shapes()' layouts, dcn_bn / up_bn
        the model's norm records.  See deformable.py adopt.  Every shape is checked before anything moves."""
        self._store.check(w, g)
        self.dcn.adopt(cut(w, "dcn"), cut(g, "dcn"))
        self._store.move(w, g)
        self.dcn_bn.adopt(dcn_bn)
        self.up_bn.adopt(up_bn)
        self.repack()

    def refresh_eval(self):
        self.dcn_bn.refresh_eval()
        self.up_bn.refresh_eval()

    # ---- parameters ------------------------------------------------------------------------------------------------------------------------
    def _shapes(self):
        return deconv_param_shapes(self.in_planes, self.out_planes, self.modulate_deform)

    def names(self):
        return list(self._shapes())

    def params(self):
        """The trainable fp32 device masters by name."""
        p = {"dcn." + k: v for k, v in self.dcn.params().items()}
        p.update({"dcn_bn.weight": self.dcn_bn.p["weight"], "dcn_bn.bias": self.dcn_bn.p["bias"], "up_sample.weight": self._up_w(),
                  "up_bn.weight": self.up_bn.p["weight"], "up_bn.bias": self.up_bn.p["bias"]})
        return p

    def repack(self):
        self.dcn.repack()
        ops.fpn_deconv_pack(self._store.w["up_sample.weight"], self.out_planes, self._up_wf, self._up_wd)

    def state_dict(self):
        out = {"dcn." + k: v for k, v in self.dcn.state_dict().items()}
        out.update(self.dcn_bn.state("dcn_bn."))
        out["up_sample.weight"] = self._up_w().detach().contiguous().cpu()
        out.update(self.up_bn.state("up_bn."))
        return out

    def load_state_dict(self, state):
        p = load_strict(state, self._shapes(), self.device)
        self.dcn.load_state_dict(cut(p, "dcn"))
        self.dcn_bn.load(p, "dcn_bn.")
        self.up_bn.load(p, "up_bn.")
        self._up_w().copy_(p["up_sample.weight"])
        self.repack()

    def train(self, mode=True):
        self.training = self.dcn_bn.training = self.up_bn.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    # ---- forward / backward ------------------------------------------------------------------------------------------------------------------
    def forward_pm(self, x, N, H, W):
        """x bf16 [N H W][in_planes] -> bf16 [N 2H 2W][out_planes].  The stage outputs stay in `self.stages` (dcn, dcn_bn, up_sample,
        up_bn) until the next forward."""
        C = self.out_planes
        y0 = self.dcn.forward_pm(x, N, H, W)
        z0 = self.dcn_bn.forward_pm(y0, N, H, W)
        y1 = torch.empty((N * 4 * H * W, C), dtype=BF16, device=self.device)
        ops.fpn_deconv_fwd(z0, self._up_wf, y1, N, H, W, C)
        z1 = self.up_bn.forward_pm(y1, N, 2 * H, 2 * W)
        self._saved = (z0, N, H, W)
        self.stages = dict(x=x, dcn=y0, dcn_bn=z0, up_sample=y1, up_bn=z1)
        return z1

    def backward_pm(self, g, accumulate=False):
        """g bf16 [N 2H 2W][out_planes] -> bf16 [N H W][in_planes].  The stage gradients stay in `self.stage_grads`."""
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        z0, N, H, W = self._saved
        C = self.out_planes
        g_y1 = self.up_bn.backward_pm(g, accumulate)
        gr, acc = self._store.grad(accumulate)
        ws = workspace(ops.fpn_deconv_wgrad_workspace_bytes(N, H, W, C), self.device)
        ops.fpn_deconv_wgrad(z0, g_y1, gr["up_sample.weight"], ws, N, H, W, C, accumulate=acc)
        g_z0 = ops.fpn_deconv_dgrad(g_y1, self._up_wd, torch.empty_like(z0), N, H, W, C)
        g_y0 = self.dcn_bn.backward_pm(g_z0, accumulate)
        g_x = self.dcn.backward_pm(g_y0, accumulate)
        self.stage_grads = dict(up_bn=g, up_sample=g_y1, dcn_bn=g_z0, dcn=g_y0, x=g_x)
        return g_x

    def __call__(self, x):
        need_device(x, "DeconvLayer")
        N, C, H, W = x.shape
        if C != self.in_planes:
            raise ValueError(f"input has {C} channels, the layer {self.in_planes}")
        return to_nchw(self.forward_pm(to_pm(x), N, H, W), N, 2 * H, 2 * W)

    forward = __call__

    def backward(self, dy, accumulate=False):
        need_device(dy, "DeconvLayer.backward")
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        _, N, H, W = self._saved
        if tuple(dy.shape) != (N, self.out_planes, 2 * H, 2 * W):
            raise ValueError(f"gradient shape {tuple(dy.shape)} does not match the forward output {(N, self.out_planes, 2 * H, 2 * W)}")
        return to_nchw(self.backward_pm(to_pm(dy), accumulate), N, H, W)

    def grads(self):
        """Parameter gradients of the last backward() under the reference's names, in the state_dict's layouts: copies, not views of the
        storage the next backward writes."""
        if self._store.g is None:
            raise RuntimeError("grads() before a backward")
        out = {"dcn." + k: v for k, v in self.dcn.grads().items()}
        out.update({"dcn_bn.weight": self.dcn_bn.g["weight"].clone(), "dcn_bn.bias": self.dcn_bn.g["bias"].clone(),
                    "up_sample.weight": self._store.g["up_sample.weight"].permute(0, 3, 1, 2).contiguous(),
                    "up_bn.weight": self.up_bn.g["weight"].clone(), "up_bn.bias": self.up_bn.g["bias"].clone()})
        return out


class CenternetDeconv(Container):
    """center_head.py:66-88: len(deconv_kernel_sizes) DeconvLayers, channels[i] -> channels[i + 1], named deconv1 ...  adopt()'s norms:
    {"deconvI.dcn_bn" / "deconvI.up_bn": norm record}."""

    def __init__(self, channels, deconv_kernel_sizes, modulate_deform, seed=0, device="cuda"):
        self.num_layers = len(deconv_kernel_sizes)
        if len(channels) != self.num_layers + 1:
            raise ValueError(f"CenternetDeconv: {len(channels)} channel counts for {self.num_layers} layers")
        for i in range(self.num_layers):        # every layer is validated before any of them touches the device
            _validate_deconv(channels[i], channels[i + 1], deconv_kernel_sizes[i], 2, 1, 0)
        self.channels, self.device = list(channels), torch.device(device)
        for i in range(self.num_layers):
            setattr(self, f"deconv{i + 1}", DeconvLayer(channels[i], channels[i + 1], deconv_kernel=deconv_kernel_sizes[i],
                                                        modulate_deform=modulate_deform, seed=seed + 10 * i, device=device))
        self._saved = None

    def layers(self):
        return [(f"deconv{i + 1}", getattr(self, f"deconv{i + 1}")) for i in range(self.num_layers)]

    _children = layers

    def forward_pm(self, x, N, H, W):
        for _, l in self.layers():
            x = l.forward_pm(x, N, H, W)
            H, W = 2 * H, 2 * W
        return x

    def backward_pm(self, g, accumulate=False):
        for _, l in reversed(self.layers()):
            g = l.backward_pm(g, accumulate)
        return g

    def __call__(self, x):
        need_device(x, "CenternetDeconv")
        N, C, H, W = x.shape
        if C != self.channels[0]:
            raise ValueError(f"input has {C} channels, the neck {self.channels[0]}")
        self._saved = (N, H, W)
        s = 2 ** self.num_layers
        return to_nchw(self.forward_pm(to_pm(x), N, H, W), N, s * H, s * W)

    forward = __call__

    def backward(self, dy, accumulate=False):
        need_device(dy, "CenternetDeconv.backward")
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        N, H, W = self._saved
        s = 2 ** self.num_layers
        if tuple(dy.shape) != (N, self.channels[-1], s * H, s * W):
            raise ValueError(f"gradient shape {tuple(dy.shape)} does not match the forward output")
        return to_nchw(self.backward_pm(to_pm(dy), accumulate), N, H, W)


class SingleHead:
    """center_head.py:91-103: the parameters of one branch (feat_conv 3x3 C -> C, ReLU, out_conv 1x1 C -> out_channel).  CenterHead runs
    its three branches fused; a SingleHead on its own only describes and initialises them (M.Conv2d's default: N(0, sqrt(1 / fan_in)),
    zero bias)."""

    def __init__(self, in_channel, out_channel, seed=0):
        self.in_channel, self.out_channel = in_channel, out_channel
        rng = np.random.default_rng(seed)
        C = in_channel
        self.state = {
            "feat_conv.weight": torch.from_numpy((rng.standard_normal((C, C, 3, 3)) * math.sqrt(1.0 / (9 * C))).astype(np.float32)),
            "feat_conv.bias": torch.zeros(C, dtype=F32),
            "out_conv.weight": torch.from_numpy((rng.standard_normal((out_channel, C, 1, 1)) * math.sqrt(1.0 / C)).astype(np.float32)),
            "out_conv.bias": torch.zeros(out_channel, dtype=F32),
        }

    def shapes(self):
        return {k: tuple(v.shape) for k, v in self.state.items()}


def validate_head(in_channels, num_classes):
    """What bd_center_head_out_* builds; ValueError before the device is touched."""
    C, K = in_channels, num_classes
    if not (isinstance(C, int) and C > 0 and C % 16 == 0 and C <= 128):
        raise ValueError(f"CenterHead: in_channels={C!r} must be a multiple of 16 up to 128 (bd_center_head_out_*)")
    if not (isinstance(K, int) and K >= 1 and (-(-K // 16) + 2) * (C // 16 + 1) <= 128):
        raise ValueError(f"CenterHead: num_classes={K!r} is outside what bd_center_head_out_* builds at in_channels={C}")


def validate_neck(channels, deconv_kernel_sizes):
    """CenternetDeconv's argument checks; ValueError before the device is touched."""
    if len(channels) != len(deconv_kernel_sizes) + 1:
        raise ValueError(f"CenternetDeconv: {len(channels)} channel counts for {len(deconv_kernel_sizes)} layers")
    for i in range(len(deconv_kernel_sizes)):
        _validate_deconv(channels[i], channels[i + 1], deconv_kernel_sizes[i], 2, 1, 0)


class CenterHead:
    """center_head.py:106-131."""
    BRANCHES = ("cls", "wh", "reg")
    NORMS = ()

    def __init__(self, in_channels=64, num_classes=80, prior_prob=0.1, seed=0, device="cuda"):
        C, K = in_channels, num_classes
        validate_head(C, K)
        self.in_channels, self.num_classes, self.prior_prob, self.device = C, K, prior_prob, torch.device(device)
        self.cls_ld = round_up8(K)
        self.cls_head, self.wh_head, self.reg_head = SingleHead(C, K, seed), SingleHead(C, 2, seed + 1), SingleHead(C, 2, seed + 2)
        self.cls_head.state["out_conv.bias"].fill_(-math.log((1 - prior_prob) / prior_prob))
        self._store = ParamStore(self.arena_shapes(), self.device)
        self._feat_wf = torch.empty((3 * C, 9, C), dtype=BF16, device=self.device)
        self._feat_wd = torch.empty((C, 9, 3 * C), dtype=BF16, device=self.device)
        self._saved = None
        self.training = True
        p = self.params()
        for b in self.BRANCHES:
            for k, v in getattr(self, b + "_head").state.items():
                p[f"{b}_head.{k}"].copy_(v)
        self.repack()

    def arena_shapes(self):
        """name -> shape of the fp32 masters in the kernels' layouts: the three feat_convs as ONE OHWI (3C, 3, 3, C) weight and (3C,) bias
        (cls | wh | reg), the output convolutions as they are."""
        C, K = self.in_channels, self.num_classes
        out = {"feat_conv.weight": (3 * C, 3, 3, C), "feat_conv.bias": (3 * C,)}
        for b, n in (("cls", K), ("wh", 2), ("reg", 2)):
            out[f"{b}_head.out_conv.weight"] = (n, C, 1, 1)
            out[f"{b}_head.out_conv.bias"] = (n,)
        return out

    def adopt(self, w, g):
        """Live on the caller's storage (a model's parameter arena); see deformable.py adopt."""
        self._store.move(w, g)
        self.repack()

    # ---- parameters ------------------------------------------------------------------------------------------------------------------------
    def _shapes(self):
        return head_param_shapes(self.in_channels, self.num_classes)

    def names(self):
        return list(self._shapes())

    def _branches(self, t):
        """The reference's per-branch names and OIHW shapes, in its order, as views of masters or gradients `t`."""
        C, out = self.in_channels, {}
        for i, b in enumerate(self.BRANCHES):
            out[f"{b}_head.feat_conv.weight"] = t["feat_conv.weight"][i * C:(i + 1) * C].permute(0, 3, 1, 2)
            out[f"{b}_head.feat_conv.bias"] = t["feat_conv.bias"][i * C:(i + 1) * C]
            out[f"{b}_head.out_conv.weight"] = t[f"{b}_head.out_conv.weight"]
            out[f"{b}_head.out_conv.bias"] = t[f"{b}_head.out_conv.bias"]
        return out

    def params(self):
        """The fp32 device masters by name (views).  After changing them in place, repack() rebuilds the bf16 operands."""
        return self._branches(self._store.w)

    def state_dict(self):
        return {k: v.detach().contiguous().cpu() for k, v in self.params().items()}

    def load_state_dict(self, state):
        p = load_strict(state, self._shapes(), self.device)
        for k, v in self.params().items():
            v.copy_(p[k])
        self.repack()

    def repack(self):
        """The three feat_convs are one 3C-row convolution (cls | wh | reg); the output convolutions are read as fp32 masters by the kernel."""
        C = self.in_channels
        ops.weight_pack(self._store.w["feat_conv.weight"], None, self._feat_wf, self._feat_wd, 3 * C, 9, C)

    def refresh_eval(self):
        pass

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def _desc(self, N, H, W):
        g = ops.single(N, H, W)
        return ops.conv_desc(g, g, self.in_channels, 3 * self.in_channels, 3, 3, 1, 1)

    # ---- forward / backward ------------------------------------------------------------------------------------------------------------------
    def forward_pm(self, x, N, H, W):
        """x bf16 [N H W][C] -> (logits_pm bf16 [M][round_up(K, 8)], wr_pm bf16 [M][8]): the raw outputs (no sigmoid)."""
        C, K, M, dev, p = self.in_channels, self.num_classes, N * H * W, self.device, self._store.w
        if tuple(x.shape) != (M, C) or x.dtype != BF16:
            raise ValueError(f"forward_pm: expected bf16 {(M, C)}, got {x.dtype} {tuple(x.shape)}")
        feat = torch.empty((M, 3 * C), dtype=BF16, device=dev)
        ops.conv2d_fwd(self._desc(N, H, W), x, self._feat_wf, p["feat_conv.bias"], feat, flags=ops.EPI_RELU)
        self.logits_pm = torch.empty((M, self.cls_ld), dtype=BF16, device=dev)
        self.wr_pm = torch.empty((M, 8), dtype=BF16, device=dev)
        ops.center_head_out_fwd(feat, p["cls_head.out_conv.weight"], p["cls_head.out_conv.bias"], p["wh_head.out_conv.weight"],
                                p["wh_head.out_conv.bias"], p["reg_head.out_conv.weight"], p["reg_head.out_conv.bias"], M, C, K,
                                self.logits_pm, self.wr_pm)
        self._saved = (x, feat, N, H, W)
        self.feat_pm = feat
        return self.logits_pm, self.wr_pm

    def backward_pm(self, d_logits, d_wr, accumulate=False):
        """d_logits bf16 [M][round_up(K, 8)], d_wr bf16 [M][8] (pad slots are never read) -> d_x bf16 [M][C]."""
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        x, feat, N, H, W = self._saved
        C, K, M, dev, p = self.in_channels, self.num_classes, N * H * W, self.device, self._store.w
        g, accumulate = self._store.grad(accumulate)
        d = self._desc(N, H, W)
        ws = workspace(max(ops.center_head_out_bwd_workspace_bytes(M, C, K), ops.conv2d_wgrad_bias_workspace_bytes(d)), dev)
        d_feat = torch.empty_like(feat)
        ops.center_head_out_bwd(feat, d_logits, d_wr, p["cls_head.out_conv.weight"], p["wh_head.out_conv.weight"],
                                p["reg_head.out_conv.weight"], M, C, K, d_feat,
                                *[g[f"{b}_head.out_conv.{s}"] for b in self.BRANCHES for s in ("weight", "bias")], ws, accumulate=accumulate)
        ops.conv2d_wgrad_bias(d, x, d_feat, g["feat_conv.weight"], g["feat_conv.bias"], ws, accumulate=accumulate)
        d_x = ops.conv2d_dgrad(d, d_feat, self._feat_wd, torch.empty_like(x))
        self.d_feat_pm = d_feat
        return d_x

    def __call__(self, x):
        need_device(x, "CenterHead")
        N, C, H, W = x.shape
        if C != self.in_channels:
            raise ValueError(f"input has {C} channels, the head {self.in_channels}")
        logits, wr = self.forward_pm(to_pm(x), N, H, W)
        K = self.num_classes
        return {"cls": torch.sigmoid(to_nchw(logits[:, :K], N, H, W)), "wh": to_nchw(wr[:, 0:2], N, H, W),
                "reg": to_nchw(wr[:, 2:4], N, H, W)}

    forward = __call__

    def backward(self, d_cls, d_wh, d_reg, accumulate=False):
        """Gradients with respect to the returned outputs (d_cls reaches the logits through p (1 - p)) -> d_x NCHW fp32."""
        for t in (d_cls, d_wh, d_reg):
            need_device(t, "CenterHead.backward")
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        _, _, N, H, W = self._saved
        K, M = self.num_classes, N * H * W
        pr = torch.sigmoid(self.logits_pm[:, :K].float())
        d_logits = torch.zeros((M, self.cls_ld), dtype=BF16, device=self.device)
        d_logits[:, :K] = (d_cls.permute(0, 2, 3, 1).reshape(M, K) * pr * (1 - pr)).to(BF16)
        d_wr = torch.zeros((M, 8), dtype=BF16, device=self.device)
        d_wr[:, 0:2] = d_wh.permute(0, 2, 3, 1).reshape(M, 2).to(BF16)
        d_wr[:, 2:4] = d_reg.permute(0, 2, 3, 1).reshape(M, 2).to(BF16)
        return to_nchw(self.backward_pm(d_logits, d_wr, accumulate), N, H, W)

    def grads(self):
        """Parameter gradients of the last backward() under the reference's names: copies, not views of the storage."""
        if self._store.g is None:
            raise RuntimeError("grads() before a backward")
        return {k: v.clone(memory_format=torch.contiguous_format) for k, v in self._branches(self._store.g).items()}
