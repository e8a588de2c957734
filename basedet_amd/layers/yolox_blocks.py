"""YOLOX's feature extractor on the HIP kernels: Focus (layers/blocks/basic_block.py:13-32), SPPBottleneck, Bottleneck, CSPLayer
(layers/blocks/yolo_block.py:36-133), CSPDarknet (models/cls/csp_darknet.py) and YOLOPAFPN (layers/backbone/yolo_fpn.py:93-199), forward
and backward.

Every convolution is layers/yolox_head.py's ConvBNSiLU (one storage path, layers/_pm.py ParamStore; one norm), every module a
layers/_pm.py Container of them.  What lies between the convolutions is
csrc/yolox_neck.hip: bd_focus_fwd (space-to-depth of the halo image into 12 + 4 zero channels), bd_spp_fwd / bd_spp_bwd (the three
stride-1 max-pools and their adjoint under the first-maximum rule), bd_cat2_fwd / bd_cat2_bwd (channel concatenation and split; PAFPN's
nearest 2x upsample is folded into the first operand) and bd_add_bf16 for Bottleneck's shortcut.  The convolution and norm entries
address [rows][C] without a channel stride, which is why a concatenation is a pass of its own.

Calling convention of layers/yolox_head.py: `layer(x)` takes and returns NCHW fp32 DEVICE tensors (a host tensor raises
BasedetHipError); `forward_pm` / `backward_pm(..., accumulate=False)` on pixel-major bf16; `params()` / `repack()` / `grads()` (copies);
strict `state_dict()` / `load_state_dict()` under the reference's names and order; `train()` / `eval()` (backward in eval() raises).
depthwise=True and activation != "silu" raise ValueError, and every channel count is validated, before the device is touched.

A tensor with two readers receives both gradients without an add pass: the second convolution that reads it adds its data gradient
through the accumulating dgrad (ConvBNSiLU.backward_pm dx= / add=), the second concatenation through bd_cat2_bwd's acc flags.

Reproducibility: every forward output, and everything the backward writes, is bitwise reproducible."""
import torch

from .. import ops
from ._pm import BF16, Block, Container, load_strict, need_device, to_nchw, to_pm
from .yolox_head import ConvBNSiLU, conv_param_shapes, validate_conv

__all__ = ["Focus", "SPPBottleneck", "Bottleneck", "CSPLayer", "CSPDarknet", "YOLOPAFPN"]

SPP_MAX_PLANE = 4096          # bd_spp_fwd / bd_spp_bwd: pixels of one image's plane


# ---- the convolutions of each module, in the order the reference's constructors create them: (name, cin, cout, k, stride) -------------------
def _refuse(what, depthwise, activation):
    if activation != "silu":
        raise ValueError(f"{what}: activation={activation!r} is not built (the fused norm kernels are SiLU's)")
    if depthwise:
        raise ValueError(f"{what}: depthwise=True is not built (DepthwiseConvBlock)")


def _pre(prefix, convs):
    return [(f"{prefix}.{n}", *rest) for n, *rest in convs]


def focus_convs(cin, cout, ksize):
    if cin != 3:
        raise ValueError(f"Focus: in_channels={cin!r} is not built (3: the normalised image)")
    return [("conv", 4 * cin, cout, ksize, 1)]


def spp_convs(cin, cout):
    return [("conv1", cin, cin // 2, 1, 1), ("conv2", cin // 2 * 4, cout, 1, 1)]


def bottleneck_convs(cin, cout, expansion=0.5):
    hidden = int(cout * expansion)
    return [("conv1", cin, hidden, 1, 1), ("conv2", hidden, cout, 3, 1)]


def csp_convs(cin, cout, n=1, expansion=0.5):
    hidden = int(cout * expansion)
    out = [("conv1", cin, hidden, 1, 1), ("conv2", cin, hidden, 1, 1), ("conv3", 2 * hidden, cout, 1, 1)]
    for i in range(n):
        out += _pre(f"m.{i}", bottleneck_convs(hidden, hidden, 1.0))
    return out


def darknet_convs(depth_factor, width_factor):
    d, c = max(round(depth_factor * 3), 1), int(width_factor * 64)
    out = _pre("stem", focus_convs(3, c, 3))
    for name, ci, co, n in (("dark2", c, 2 * c, d), ("dark3", 2 * c, 4 * c, 3 * d), ("dark4", 4 * c, 8 * c, 3 * d)):
        out += [(f"{name}.0", ci, co, 3, 2)] + _pre(f"{name}.1", csp_convs(co, co, n))
    out += [("dark5.0", 8 * c, 16 * c, 3, 2)] + _pre("dark5.1", spp_convs(16 * c, 16 * c)) + _pre("dark5.2", csp_convs(16 * c, 16 * c, d))
    return out


def pafpn_convs(backbone_convs, depth, width, in_channels):
    c0, c1, c2 = (int(c * width) for c in in_channels)
    n = round(3 * depth)
    return (_pre("backbone", backbone_convs) + [("lateral_conv0", c2, c1, 1, 1)] + _pre("C3_p4", csp_convs(2 * c1, c1, n))
            + [("reduce_conv1", c1, c0, 1, 1)] + _pre("C3_p3", csp_convs(2 * c0, c0, n)) + [("bu_conv2", c0, c0, 3, 2)]
            + _pre("C3_n3", csp_convs(2 * c0, c1, n)) + [("bu_conv1", c1, c1, 3, 2)] + _pre("C3_n4", csp_convs(2 * c1, c2, n)))


def _validate(convs):
    """Every convolution of a module, before any of them allocates (Focus's 12 input channels are padded to 16 on the device)."""
    for name, cin, cout, k, stride in convs:
        try:
            validate_conv(16 if cin == 12 and name.endswith("conv") else cin, cout, k, stride)
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None


def param_shapes(convs):
    """name -> shape of the state of a module with these convolutions, in the reference's order."""
    return {f"{n}.{k}": v for n, cin, cout, ks, _ in convs for k, v in conv_param_shapes(cin, cout, ks).items()}


def darknet_param_shapes(depth_factor, width_factor):
    return param_shapes(darknet_convs(depth_factor, width_factor))


def pafpn_param_shapes(depth, width, in_channels=(256, 512, 1024), backbone=None):
    return param_shapes(pafpn_convs(darknet_convs(depth, width) if backbone is None else backbone, depth, width, in_channels))


# ---- what the modules share -------------------------------------------------------------------------------------------------------------------
def _convs(specs, seed, device):
    """The ConvBNSiLU layers of validated specs by local name; each from its own seed."""
    return {n: ConvBNSiLU(cin, cout, k, stride, seed=seed + i, device=device) for i, (n, cin, cout, k, stride) in enumerate(specs)}


def _cat(a, b, M, up=False, N=0, H=0, W=0):
    Ca, Cb = int(a.shape[1]), int(b.shape[1])
    return ops.cat2_fwd(a, b, M, Ca, Cb, torch.empty((M, Ca + Cb), dtype=BF16, device=b.device), up, N, H, W)


def _split(g, Ca, up=False, N=0, H=0, W=0, d_a=None, d_b=None):
    """(d_a, d_b) of a concatenation's gradient; a given d_a / d_b already holds another reader's gradient and is added onto."""
    M, Cb = int(g.shape[0]), int(g.shape[1]) - Ca
    acc_a, acc_b = d_a is not None, d_b is not None
    if d_a is None:
        d_a = torch.empty((M // 4 if up else M, Ca), dtype=BF16, device=g.device)
    if d_b is None:
        d_b = torch.empty((M, Cb), dtype=BF16, device=g.device)
    return ops.cat2_bwd(g, M, Ca, Cb, d_a, d_b, up, N, H, W, acc_a, acc_b)


# ---- the blocks ---------------------------------------------------------------------------------------------------------------------------------
class _FocusConv(ConvBNSiLU):
    """Focus's convolution on the 16-channel tensor bd_focus_fwd writes.  The master is (cout, k, k, 16) with input channels 12-15 zero;
    they stay zero (their gradient columns are exactly zero because the input is, and params() / grads() expose the 12 real columns)."""
    REAL = 12

    def __init__(self, cout, k, seed, device):
        super().__init__(16, cout, k, 1, seed=seed, device=device)
        w = self._store.w["weight"]
        w[..., self.REAL:] = 0
        w[..., :self.REAL] *= (16 / self.REAL) ** 0.5          # N(0, sqrt(1 / fan_in)) of the 12 real channels
        self.repack()

    def _shapes(self):
        return conv_param_shapes(self.REAL, self.cout, self.k)

    def params(self):
        return dict(super().params(), weight=self._store.w["weight"].permute(0, 3, 1, 2)[:, :self.REAL])

    def state_dict(self):
        s = super().state_dict()
        return dict(s, weight=s["weight"][:, :self.REAL].contiguous())

    def load_state_dict(self, state):
        p = load_strict(state, self._shapes(), self.device)
        w = self._store.w["weight"]
        w.zero_()
        w[..., :self.REAL] = p["weight"].permute(0, 2, 3, 1)
        self.norm.load(p, "norm.")
        self.repack()

    def grads(self):
        g = super().grads()
        return dict(g, weight=g["weight"][:, :self.REAL].contiguous())

    def pad_grad(self):
        """The 4 pad columns of the weight gradient (a copy): exactly zero."""
        return self._store.g["weight"][..., self.REAL:].clone()


class Focus(Container):
    """basic_block.py:13-32 with in_channels = 3: bd_focus_fwd, then ConvBNSiLU(12 + 4 zero channels, cout, ksize)."""

    def __init__(self, in_channels=3, out_channels=32, ksize=3, stride=1, activation="silu", seed=0, device="cuda"):
        _refuse("Focus", False, activation)
        if stride != 1:
            raise ValueError(f"Focus: stride={stride!r} is not built (1)")
        _validate(focus_convs(in_channels, out_channels, ksize))
        self.cin, self.cout, self.device = in_channels, out_channels, torch.device(device)
        self.conv = _FocusConv(out_channels, ksize, seed, device)

    def _children(self):
        return [("conv", self.conv)]

    @staticmethod
    def halo(x):
        """NCHW fp32 (N, 3, H, W) -> the bf16 (N, H + 6, W + 8, 4) layout bd_pad_normalize writes (zero halo, channel 3 zero)."""
        N, C, H, W = x.shape
        out = torch.zeros((N, H + 6, W + 8, 4), dtype=BF16, device=x.device)
        out[:, 3:3 + H, 4:4 + W, :3] = x.permute(0, 2, 3, 1)
        return out

    def forward_pm(self, x_halo, N, H, W):
        """x_halo bf16 (N, H + 6, W + 8, 4) -> bf16 [N H/2 W/2][cout]."""
        if tuple(x_halo.shape) != (N, H + 6, W + 8, 4) or x_halo.dtype != BF16:
            raise ValueError(f"Focus.forward_pm: expected bf16 {(N, H + 6, W + 8, 4)}, got {x_halo.dtype} {tuple(x_halo.shape)}")
        if H % 2 or W % 2:
            raise ValueError(f"Focus: H={H} and W={W} must be even")
        s2d = ops.focus_fwd(x_halo, N, H, W, torch.empty((N * (H // 2) * (W // 2), 16), dtype=BF16, device=self.device))
        return self.conv.forward_pm(s2d, N, H // 2, W // 2)

    def backward_pm(self, g, accumulate=False):
        """Parameter gradients only: the image has no gradient."""
        return self.conv.backward_pm(g, accumulate, need_dx=False)

    def __call__(self, x):
        need_device(x, "Focus")
        N, C, H, W = x.shape
        if C != 3:
            raise ValueError(f"input has {C} channels, the layer 3")
        self._in_size = (N, H, W)
        return to_nchw(self.forward_pm(self.halo(x), N, H, W), N, H // 2, W // 2)

    forward = __call__

    def backward(self, dy, accumulate=False):
        need_device(dy, "Focus.backward")
        self.backward_pm(to_pm(dy), accumulate)


class SPPBottleneck(Block):
    """yolo_block.py:36-60, kernel_sizes (5, 9, 13): conv1 -> bd_spp_fwd -> conv2."""

    def __init__(self, in_channels, out_channels, kernel_sizes=(5, 9, 13), activation="silu", seed=0, device="cuda"):
        _refuse("SPPBottleneck", False, activation)
        if tuple(kernel_sizes) != (5, 9, 13):
            raise ValueError(f"SPPBottleneck: kernel_sizes={kernel_sizes!r} is not built ((5, 9, 13): bd_spp_fwd)")
        specs = spp_convs(in_channels, out_channels)
        _validate(specs)
        self.cin, self.cout, self.device = in_channels, out_channels, torch.device(device)
        c = _convs(specs, seed, device)
        self.conv1, self.conv2 = c["conv1"], c["conv2"]
        self._saved = None

    def _children(self):
        return [("conv1", self.conv1), ("conv2", self.conv2)]

    def forward_pm(self, x, N, H, W):
        if H * W > SPP_MAX_PLANE:
            raise ValueError(f"SPPBottleneck: a {H} x {W} map exceeds the {SPP_MAX_PLANE} pixels bd_spp_fwd holds")
        h = self.conv1.forward_pm(x, N, H, W)
        C = int(h.shape[1])
        cat = ops.spp_fwd(h, N, H, W, C, torch.empty((N * H * W, 4 * C), dtype=BF16, device=self.device))
        self._saved = (h, N, H, W)
        return self.conv2.forward_pm(cat, N, H, W)

    def backward_pm(self, g, accumulate=False, add=None):
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        h, N, H, W = self._saved
        g_cat = self.conv2.backward_pm(g, accumulate)
        d_h = ops.spp_bwd(g_cat, h, N, H, W, int(h.shape[1]), torch.empty_like(h))
        return self.conv1.backward_pm(d_h, accumulate, add=add)


class Bottleneck(Block):
    """yolo_block.py:63-88: conv1 (1x1) -> conv2 (3x3) [+ x].  With the shortcut, x receives the output gradient and conv1's data
    gradient: conv1's accumulating dgrad adds the two."""

    def __init__(self, in_channels, out_channels, shortcut=True, expansion=0.5, depthwise=False, activation="silu", seed=0, device="cuda"):
        _refuse("Bottleneck", depthwise, activation)
        specs = bottleneck_convs(in_channels, out_channels, expansion)
        _validate(specs)
        self.cin, self.cout, self.device = in_channels, out_channels, torch.device(device)
        self.use_add = bool(shortcut) and in_channels == out_channels
        c = _convs(specs, seed, device)
        self.conv1, self.conv2 = c["conv1"], c["conv2"]

    def _children(self):
        return [("conv1", self.conv1), ("conv2", self.conv2)]

    def forward_pm(self, x, N, H, W):
        y = self.conv2.forward_pm(self.conv1.forward_pm(x, N, H, W), N, H, W)
        return ops.add_bf16(y, x, torch.empty_like(y)) if self.use_add else y

    def backward_pm(self, g, accumulate=False):
        g1 = self.conv2.backward_pm(g, accumulate)
        return self.conv1.backward_pm(g1, accumulate, add=g if self.use_add else None)


class CSPLayer(Block):
    """yolo_block.py:91-133: conv3(cat(m(conv1(x)), conv2(x))).  conv1 and conv2 read the same x as two launches, as the head's towers
    do; conv2's data gradient is added onto conv1's."""

    def __init__(self, in_channels, out_channels, n=1, shortcut=True, expansion=0.5, depthwise=False, activation="silu", seed=0,
                 device="cuda"):
        _refuse("CSPLayer", depthwise, activation)
        _validate(csp_convs(in_channels, out_channels, n, expansion))
        self.cin, self.cout, self.device = in_channels, out_channels, torch.device(device)
        self.hidden = int(out_channels * expansion)
        c = _convs(csp_convs(in_channels, out_channels, 0, expansion), seed, device)
        self.conv1, self.conv2, self.conv3 = c["conv1"], c["conv2"], c["conv3"]
        self.m = [Bottleneck(self.hidden, self.hidden, shortcut, 1.0, seed=seed + 3 + 2 * i, device=device) for i in range(n)]

    def _children(self):
        return [("conv1", self.conv1), ("conv2", self.conv2), ("conv3", self.conv3)] + [(f"m.{i}", b) for i, b in enumerate(self.m)]

    def forward_pm(self, x, N, H, W):
        x1 = self.conv1.forward_pm(x, N, H, W)
        x2 = self.conv2.forward_pm(x, N, H, W)
        for b in self.m:
            x1 = b.forward_pm(x1, N, H, W)
        return self.conv3.forward_pm(_cat(x1, x2, N * H * W), N, H, W)

    def backward_pm(self, g, accumulate=False):
        d1, d2 = _split(self.conv3.backward_pm(g, accumulate), self.hidden)
        for b in reversed(self.m):
            d1 = b.backward_pm(d1, accumulate)
        dx = self.conv1.backward_pm(d1, accumulate)
        return self.conv2.backward_pm(d2, accumulate, dx=dx)


class CSPDarknet(Container):
    """csp_darknet.py: stem (Focus) and dark2 .. dark5.  forward_pm returns the named features; backward_pm takes their gradients and sums
    them where a feature also feeds the next stage (the next stage's first convolution adds its data gradient onto the feature's)."""
    STAGES = ("dark2", "dark3", "dark4", "dark5")

    def __init__(self, depth_factor, width_factor, out_features=("dark3", "dark4", "dark5"), depthwise=False, activation="silu", seed=0,
                 device="cuda"):
        _refuse("CSPDarknet", depthwise, activation)
        if not out_features or any(f not in ("stem",) + self.STAGES for f in out_features):
            raise ValueError(f"CSPDarknet: out_features={out_features!r}")
        _validate(darknet_convs(depth_factor, width_factor))
        self.depth_factor, self.width_factor, self.out_features = depth_factor, width_factor, tuple(out_features)
        self.device = torch.device(device)
        d, c = max(round(depth_factor * 3), 1), int(width_factor * 64)
        self.channels = {"stem": c, "dark2": 2 * c, "dark3": 4 * c, "dark4": 8 * c, "dark5": 16 * c}
        self.stem = Focus(3, c, 3, seed=seed, device=device)
        self.stages, s = {}, seed + 100
        for name, ci, co, n in (("dark2", c, 2 * c, d), ("dark3", 2 * c, 4 * c, 3 * d), ("dark4", 4 * c, 8 * c, 3 * d)):
            self.stages[name] = [ConvBNSiLU(ci, co, 3, 2, seed=s, device=device), CSPLayer(co, co, n, seed=s + 1, device=device)]
            s += 100
        self.stages["dark5"] = [ConvBNSiLU(8 * c, 16 * c, 3, 2, seed=s, device=device), SPPBottleneck(16 * c, 16 * c, seed=s + 1, device=device),
                                CSPLayer(16 * c, 16 * c, d, shortcut=False, seed=s + 3, device=device)]
        self._saved = None

    def _children(self):
        return [("stem", self.stem)] + [(f"{n}.{i}", l) for n in self.STAGES for i, l in enumerate(self.stages[n])]

    def forward_pm(self, x_halo, N, H, W):
        """x_halo bf16 (N, H + 6, W + 8, 4) -> ({name: bf16 [N H_f W_f][C_f]}, {name: (H_f, W_f)}) of out_features."""
        if H % 32 or W % 32:
            raise ValueError(f"CSPDarknet: H={H} and W={W} must be multiples of 32")
        x, h, w = self.stem.forward_pm(x_halo, N, H, W), H // 2, W // 2
        feats, sizes = {"stem": x}, {"stem": (h, w)}
        for name in self.STAGES:
            conv, *rest = self.stages[name]
            x = conv.forward_pm(x, N, h, w)
            h, w = conv.out_size(h, w)
            for l in rest:
                x = l.forward_pm(x, N, h, w)
            feats[name], sizes[name] = x, (h, w)
        self._saved = (N, sizes)
        return {k: feats[k] for k in self.out_features}, {k: sizes[k] for k in self.out_features}

    def backward_pm(self, d_feats, accumulate=False):
        """d_feats {name: bf16 gradient} of the features forward_pm returned (the last stage's is required).  Runs down to the stem."""
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        N, sizes = self._saved
        if set(d_feats) - set(self.out_features):
            raise ValueError(f"backward_pm: gradients of {sorted(set(d_feats) - set(self.out_features))} were not outputs")
        order = ("stem",) + self.STAGES
        last = max(order.index(k) for k in d_feats)
        g = d_feats[order[last]]          # (stages above the last gradient given take no part in this backward)
        for i in range(last, 0, -1):
            conv, *rest = self.stages[order[i]]
            for l in reversed(rest):
                g = l.backward_pm(g, accumulate)
            g = conv.backward_pm(g, accumulate, add=d_feats.get(order[i - 1]))
        self.stem.backward_pm(g, accumulate)

    def __call__(self, x):
        need_device(x, "CSPDarknet")
        N, C, H, W = x.shape
        if C != 3:
            raise ValueError(f"input has {C} channels, the layer 3")
        feats, sizes = self.forward_pm(Focus.halo(x), N, H, W)
        return {k: to_nchw(v, N, *sizes[k]) for k, v in feats.items()}

    forward = __call__

    def backward(self, d_feats, accumulate=False):
        for v in d_feats.values():
            need_device(v, "CSPDarknet.backward")
        self.backward_pm({k: to_pm(v) for k, v in d_feats.items()}, accumulate)


class YOLOPAFPN(Container):
    """yolo_fpn.py:93-199 on a CSPDarknet.  forward_pm returns (pan_out2, pan_out1, pan_out0) at strides 8 / 16 / 32; backward_pm runs the
    whole graph backwards down to the stem.  The two upsample-and-concatenate steps are bd_cat2_fwd(up=1); fpn_out0 and fpn_out1 (two
    concatenations each), dark3 and dark4 (a concatenation and the next stage), pan_out2 and pan_out1 (an output and a bottom-up
    convolution) receive their second gradient through an accumulating launch."""

    def __init__(self, bottom_up, depth=1.0, width=1.0, in_features=("dark3", "dark4", "dark5"), in_channels=(256, 512, 1024),
                 depthwise=False, activation="silu", seed=1000, device="cuda"):
        _refuse("YOLOPAFPN", depthwise, activation)
        if len(in_features) != 3 or len(in_channels) != 3 or tuple(in_features) != tuple(bottom_up.out_features):
            raise ValueError("YOLOPAFPN: three in_features, the bottom_up's out_features in order")
        c0, c1, c2 = (int(c * width) for c in in_channels)
        if [bottom_up.channels[f] for f in in_features] != [c0, c1, c2]:
            raise ValueError(f"YOLOPAFPN: in_channels * width = {[c0, c1, c2]} are not the bottom_up's {[bottom_up.channels[f] for f in in_features]}")
        _validate(pafpn_convs([], depth, width, in_channels))
        self.backbone, self.in_features, self.in_channels, self.device = bottom_up, tuple(in_features), list(in_channels), torch.device(device)
        self.widths, n = (c0, c1, c2), round(3 * depth)
        mk = lambda i, *a, **k: (ConvBNSiLU if len(a) == 4 else CSPLayer)(*a, seed=seed + 50 * i, device=device, **k)
        self.lateral_conv0 = mk(0, c2, c1, 1, 1)
        self.C3_p4 = mk(1, 2 * c1, c1, n, shortcut=False)
        self.reduce_conv1 = mk(2, c1, c0, 1, 1)
        self.C3_p3 = mk(3, 2 * c0, c0, n, shortcut=False)
        self.bu_conv2 = mk(4, c0, c0, 3, 2)
        self.C3_n3 = mk(5, 2 * c0, c1, n, shortcut=False)
        self.bu_conv1 = mk(6, c1, c1, 3, 2)
        self.C3_n4 = mk(7, 2 * c1, c2, n, shortcut=False)
        self._saved = None

    def _children(self):
        return [("backbone", self.backbone)] + [(n, getattr(self, n)) for n in ("lateral_conv0", "C3_p4", "reduce_conv1", "C3_p3", "bu_conv2",
                                                                                "C3_n3", "bu_conv1", "C3_n4")]

    def forward_pm(self, x_halo, N, H, W):
        """x_halo bf16 (N, H + 6, W + 8, 4), H and W multiples of 32 -> ((pan_out2, pan_out1, pan_out0), [(H/8, W/8), (H/16, W/16),
        (H/32, W/32)])."""
        if H % 32 or W % 32:
            raise ValueError(f"YOLOPAFPN: H={H} and W={W} must be multiples of 32")
        feats, sizes = self.backbone.forward_pm(x_halo, N, H, W)
        (x2, x1, x0), ((h2, w2), (h1, w1), (h0, w0)) = (feats[f] for f in self.in_features), (sizes[f] for f in self.in_features)
        fpn_out0 = self.lateral_conv0.forward_pm(x0, N, h0, w0)
        f_out0 = self.C3_p4.forward_pm(_cat(fpn_out0, x1, N * h1 * w1, True, N, h1, w1), N, h1, w1)
        fpn_out1 = self.reduce_conv1.forward_pm(f_out0, N, h1, w1)
        pan_out2 = self.C3_p3.forward_pm(_cat(fpn_out1, x2, N * h2 * w2, True, N, h2, w2), N, h2, w2)
        p_out1 = self.bu_conv2.forward_pm(pan_out2, N, h2, w2)
        pan_out1 = self.C3_n3.forward_pm(_cat(p_out1, fpn_out1, N * h1 * w1), N, h1, w1)
        p_out0 = self.bu_conv1.forward_pm(pan_out1, N, h1, w1)
        pan_out0 = self.C3_n4.forward_pm(_cat(p_out0, fpn_out0, N * h0 * w0), N, h0, w0)
        self._saved = (N, [(h2, w2), (h1, w1), (h0, w0)])
        return (pan_out2, pan_out1, pan_out0), [(h2, w2), (h1, w1), (h0, w0)]

    def backward_pm(self, d_outs, accumulate=False):
        """d_outs: the bf16 gradients of (pan_out2, pan_out1, pan_out0); they keep their bits.  Parameter gradients only."""
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        N, ((h2, w2), (h1, w1), (h0, w0)) = self._saved
        c0, c1, c2 = self.widths
        d2, d1, d0 = d_outs
        d_p_out0, d_fpn_out0 = _split(self.C3_n4.backward_pm(d0, accumulate), c1)
        d_pan_out1 = self.bu_conv1.backward_pm(d_p_out0, accumulate, add=d1)
        d_p_out1, d_fpn_out1 = _split(self.C3_n3.backward_pm(d_pan_out1, accumulate), c0)
        d_pan_out2 = self.bu_conv2.backward_pm(d_p_out1, accumulate, add=d2)
        _, d_x2 = _split(self.C3_p3.backward_pm(d_pan_out2, accumulate), c0, True, N, h2, w2, d_a=d_fpn_out1)
        d_f_out0 = self.reduce_conv1.backward_pm(d_fpn_out1, accumulate)
        _, d_x1 = _split(self.C3_p4.backward_pm(d_f_out0, accumulate), c1, True, N, h1, w1, d_a=d_fpn_out0)
        d_x0 = self.lateral_conv0.backward_pm(d_fpn_out0, accumulate)
        self.backbone.backward_pm(dict(zip(self.in_features, (d_x2, d_x1, d_x0))), accumulate)

    def __call__(self, x):
        need_device(x, "YOLOPAFPN")
        N, C, H, W = x.shape
        if C != 3:
            raise ValueError(f"input has {C} channels, the layer 3")
        outs, sizes = self.forward_pm(Focus.halo(x), N, H, W)
        return tuple(to_nchw(o, N, h, w) for o, (h, w) in zip(outs, sizes))

    forward = __call__

    def backward(self, d_outs, accumulate=False):
        for v in d_outs:
            need_device(v, "YOLOPAFPN.backward")
        self.backward_pm([to_pm(v) for v in d_outs], accumulate)
