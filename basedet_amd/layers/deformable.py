"""basedet.layers.DeformConvWithOff / ModulatedDeformConvWithOff (layers/blocks/deformable.py:9-63) on the HIP deformable convolution
(csrc/deform_conv.hip): an ordinary 3x3 convolution predicts the sampling offsets (and, modulated, the mask logits) from the input, the
deformable convolution samples the same input at those positions.

Only the configuration the reference instantiates (layers/head/center_head.py:22-30) is built: kernel_size=3, stride=1, padding=1,
dilation=1, deformable_groups=1; anything else raises ValueError before the device is touched.

Calling convention of layers/modules.py's heads: `layer(x)` takes and returns NCHW fp32; `layer.backward(dy)` returns dx and leaves the
parameter gradients in `layer.grads()` under the reference's names (OIHW); `state_dict()` / `load_state_dict()` carry those names too.
The offset convolution's 18 / 27 output rows are padded with zero rows to ld = 24 / 32 (as PaddedClsConv pads class rows): the pad
channels of the offset tensor are never read as data and get a +0 gradient, so the pad rows' gradients are sums of zeros.

Storage (layers/_pm.py ParamStore): the fp32 masters are allocated once, in the kernels' own layouts (arena_shapes(): OHWI, padded rows),
and so are the bf16 operands repack() writes; params() hands out OIHW views of the masters and load_state_dict() copies into them, so a
view taken once stays valid.  adopt() moves the masters and gradients onto a caller's storage; nothing else differs between a layer on
its own storage and one on a model's arena."""
import math

import numpy as np
import torch

from .. import ops
from ._pm import BF16, ParamStore, load_strict, round_up8, to_nchw, to_pm, workspace

__all__ = ["DeformConvWithOff", "ModulatedDeformConvWithOff"]


def _validate(in_channels, out_channels, kernel_size, stride, padding, dilation, deformable_groups):
    got = dict(kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation, deformable_groups=deformable_groups)
    want = dict(kernel_size=3, stride=1, padding=1, dilation=1, deformable_groups=1)
    for k, v in want.items():
        g = got[k]
        if isinstance(g, (tuple, list)) and len(g) == 2 and g[0] == g[1]:
            g = g[0]
        if g != v:
            raise ValueError(f"deformable convolution: only {want} is built (center_head.py:22-30); got {k}={got[k]!r}")
    for k, c in (("in_channels", in_channels), ("out_channels", out_channels)):
        if not (isinstance(c, int) and c > 0 and c % 8 == 0):
            raise ValueError(f"deformable convolution: {k}={c!r} must be a positive multiple of 8")


class _DeformConvBase:
    MODULATED = False
    OFFSET_NAME = "offset_conv"
    DCN_NAME = "dcn"

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, deformable_groups=1, seed=0,
                 device="cuda"):
        _validate(in_channels, out_channels, kernel_size, stride, padding, dilation, deformable_groups)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.off_channels = 27 if self.MODULATED else 18          # deformable_groups * (2 | 3) * kernel_size^2
        self.ld = round_up8(self.off_channels)
        self.device = torch.device(device)
        # MegEngine's M.Conv2d default: N(0, sqrt(1 / fan_in)), zero bias (models/params.py states it for P6 / P7)
        rng = np.random.default_rng(seed)
        std = math.sqrt(1.0 / (in_channels * 9))
        init = {name + ".weight": torch.from_numpy((rng.standard_normal((co, in_channels, 3, 3)) * std).astype(np.float32))
                for name, co in ((self.OFFSET_NAME, self.off_channels), (self.DCN_NAME, out_channels))}
        self._store = ParamStore(self.arena_shapes(), self.device)          # (zeros: the biases, the offset convolution's pad rows)
        bf = dict(dtype=BF16, device=self.device)
        self._off_wf, self._off_wd = torch.empty((self.ld, 9, in_channels), **bf), torch.empty((in_channels, 9, self.ld), **bf)
        self._dcn_wf, self._dcn_wd = torch.empty((out_channels, 9, in_channels), **bf), torch.empty((in_channels, 9, out_channels), **bf)
        self._saved = None
        self.last_offset_mask = None
        p = self.params()
        for k, v in init.items():
            p[k].copy_(v)
        self.repack()

    # ---- parameters ------------------------------------------------------------------------------------------------------------------------
    def names(self):
        return [n + s for n in (self.OFFSET_NAME, self.DCN_NAME) for s in (".weight", ".bias")]

    def _shapes(self):
        k, Cin, Cout = self.off_channels, self.in_channels, self.out_channels
        return {self.OFFSET_NAME + ".weight": (k, Cin, 3, 3), self.OFFSET_NAME + ".bias": (k,),
                self.DCN_NAME + ".weight": (Cout, Cin, 3, 3), self.DCN_NAME + ".bias": (Cout,)}

    def arena_shapes(self):
        """name -> shape of the fp32 masters in the kernels' own layouts (OHWI, the offset convolution's rows padded to ld): what a caller
        that provides the storage (adopt) reserves, for the masters and for the gradients alike."""
        ld, Cin = self.ld, self.in_channels
        return {self.OFFSET_NAME + ".weight": (ld, 3, 3, Cin), self.OFFSET_NAME + ".bias": (ld,),
                self.DCN_NAME + ".weight": (self.out_channels, 3, 3, Cin), self.DCN_NAME + ".bias": (self.out_channels,)}

    def adopt(self, w, g):
        """Live on storage the caller provides (a model's parameter arena): w / g = {name: fp32 device view} in arena_shapes()' layouts.
        The current values move into w; from here on the masters ARE those views (an optimizer step over the arena, then repack()) and
        backward writes every parameter gradient straight into g.  The pad rows of the offset convolution are zero and stay zero (their
        gradients are sums of zeros)."""
        self._store.move(w, g)
        self.repack()

    def _oihw(self, t):
        """The reference's names and OIHW shapes as views of masters or gradients `t` (the real rows of the offset convolution)."""
        k, on, dn = self.off_channels, self.OFFSET_NAME, self.DCN_NAME
        return {on + ".weight": t[on + ".weight"][:k].permute(0, 3, 1, 2), on + ".bias": t[on + ".bias"][:k],
                dn + ".weight": t[dn + ".weight"].permute(0, 3, 1, 2), dn + ".bias": t[dn + ".bias"]}

    def params(self):
        """The fp32 device masters by name (OIHW views).  After changing them in place, repack() rebuilds the bf16 operands."""
        return self._oihw(self._store.w)

    def state_dict(self):
        return {k: v.detach().contiguous().cpu() for k, v in self.params().items()}

    def load_state_dict(self, state):
        """The values move into the masters, which stay where they are (extra keys are ignored)."""
        p = load_strict(state, self._shapes(), self.device, extra_ok=True)
        for k, v in self.params().items():
            v.copy_(p[k])
        self.repack()

    def repack(self):
        """fp32 masters -> the bf16 operands of the kernels, in place."""
        w, Cin = self._store.w, self.in_channels
        ops.weight_pack(w[self.OFFSET_NAME + ".weight"], None, self._off_wf, self._off_wd, self.ld, 9, Cin)
        ops.weight_pack(w[self.DCN_NAME + ".weight"], None, self._dcn_wf, self._dcn_wd, self.out_channels, 9, Cin)

    def _offset_desc(self, N, H, W):
        g = ops.single(N, H, W)
        return ops.conv_desc(g, g, self.in_channels, self.ld, 3, 3, 1, 1)

    # ---- forward / backward ------------------------------------------------------------------------------------------------------------------
    def __call__(self, x):
        N, C, H, W = x.shape
        if C != self.in_channels:
            raise ValueError(f"input has {C} channels, the layer {self.in_channels}")
        return to_nchw(self.forward_pm(to_pm(x.to(self.device)), N, H, W), N, H, W)

    forward = __call__

    def forward_pm(self, xp, N, H, W):
        """The pixel-major path: xp bf16 [N H W][Cin] on the device -> y bf16 [N H W][Cout]; no NCHW / fp32 round trip."""
        M, C, w = N * H * W, self.in_channels, self._store.w
        if tuple(xp.shape) != (M, C) or xp.dtype != torch.bfloat16:
            raise ValueError(f"forward_pm: expected bf16 {(M, C)}, got {xp.dtype} {tuple(xp.shape)}")
        om = torch.empty((M, self.ld), dtype=torch.bfloat16, device=self.device)
        ops.conv2d_fwd(self._offset_desc(N, H, W), xp, self._off_wf, w[self.OFFSET_NAME + ".bias"], om)
        y = torch.empty((M, self.out_channels), dtype=torch.bfloat16, device=self.device)
        ops.deform_conv_fwd(xp, om, self._dcn_wf, w[self.DCN_NAME + ".bias"], y, N, H, W, C, self.out_channels, self.MODULATED)
        self._saved = (xp, om, N, H, W)
        self.last_offset_mask = om
        return y

    def backward(self, dy, accumulate=False):
        """Gradient of the last forward's output (NCHW) -> gradient of its input (NCHW fp32); parameter gradients in grads().
        accumulate: add to the parameter gradients of the previous backward instead of overwriting them."""
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        _, _, N, H, W = self._saved
        if tuple(dy.shape) != (N, self.out_channels, H, W):
            raise ValueError(f"gradient shape {tuple(dy.shape)} does not match the forward output {(N, self.out_channels, H, W)}")
        return to_nchw(self.backward_pm(to_pm(dy.to(self.device)), accumulate), N, H, W)

    def backward_pm(self, g, accumulate=False):
        """g bf16 [N H W][Cout] -> d_x bf16 [N H W][Cin]; parameter gradients in grads()."""
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        xp, om, N, H, W = self._saved
        Cin, Cout, ld, dev = self.in_channels, self.out_channels, self.ld, self.device
        M = N * H * W
        if tuple(g.shape) != (M, Cout) or g.dtype != torch.bfloat16:
            raise ValueError(f"backward_pm: expected bf16 {(M, Cout)}, got {g.dtype} {tuple(g.shape)}")
        gr, accumulate = self._store.grad(accumulate)
        on, dn = self.OFFSET_NAME, self.DCN_NAME
        d = self._offset_desc(N, H, W)
        ws = workspace(max(ops.deform_conv_wgrad_workspace_bytes(N, H, W, Cin, Cout), ops.deform_conv_bwd_data_workspace_bytes(N, H, W, Cin, Cout),
                           ops.conv2d_wgrad_bias_workspace_bytes(d)), dev)
        ops.deform_conv_wgrad(xp, om, g, gr[dn + ".weight"], gr[dn + ".bias"], ws, N, H, W, Cin, Cout, self.MODULATED, accumulate=accumulate)
        dx_dcn = torch.empty((M, Cin), dtype=torch.bfloat16, device=dev)
        d_om = torch.empty((M, ld), dtype=torch.bfloat16, device=dev)
        ops.deform_conv_bwd_data(xp, om, g, self._dcn_wd, dx_dcn, d_om, ws, N, H, W, Cin, Cout, self.MODULATED)
        # the offset convolution reads the same input: its data gradient lands on top of the deformable part
        ops.conv2d_wgrad_bias(d, xp, d_om, gr[on + ".weight"], gr[on + ".bias"], ws, accumulate=accumulate)
        dx = torch.empty_like(dx_dcn)
        ops.conv2d_dgrad(d, d_om, self._off_wd, dx, add=dx_dcn, flags=ops.EPI_ADD_BEFORE)
        self.last_d_offset_mask = d_om
        return dx

    def grads(self):
        """Parameter gradients of the last backward() under the reference's names, OIHW fp32: copies, not views of the storage."""
        if self._store.g is None:
            raise RuntimeError("grads() before a backward")
        return {k: v.clone(memory_format=torch.contiguous_format) for k, v in self._oihw(self._store.g).items()}


class DeformConvWithOff(_DeformConvBase):
    """layers/blocks/deformable.py:9-34: offset_conv (18 channels) + M.DeformableConv2d with a mask of ones (DCNv1)."""
    MODULATED = False
    OFFSET_NAME = "offset_conv"
    DCN_NAME = "dcn"


class ModulatedDeformConvWithOff(_DeformConvBase):
    """layers/blocks/deformable.py:37-63: offset_mask_conv (27 channels: 18 offsets, 9 mask logits) + M.DeformableConv2d with
    mask = sigmoid(logits) (DCNv2)."""
    MODULATED = True
    OFFSET_NAME = "offset_mask_conv"
    DCN_NAME = "dcnv2"
