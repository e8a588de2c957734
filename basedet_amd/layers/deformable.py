"""basedet.layers.DeformConvWithOff / ModulatedDeformConvWithOff (layers/blocks/deformable.py:9-63) on the HIP deformable convolution
(csrc/deform_conv.hip): an ordinary 3x3 convolution predicts the sampling offsets (and, modulated, the mask logits) from the input, the
deformable convolution samples the same input at those positions.

Only the configuration the reference instantiates (layers/head/center_head.py:22-30) is built: kernel_size=3, stride=1, padding=1,
dilation=1, deformable_groups=1; anything else raises ValueError before the device is touched.

Calling convention of layers/modules.py's heads: `layer(x)` takes and returns NCHW fp32; `layer.backward(dy)` returns dx and leaves the
parameter gradients in `layer.grads()` under the reference's names (OIHW); `state_dict()` / `load_state_dict()` carry those names too.
The offset convolution's 18 / 27 output rows are padded with zero rows to ld = 24 / 32 (as PaddedClsConv pads class rows): the pad
channels of the offset tensor are never read as data and get a +0 gradient, so the pad rows' gradients are sums of zeros."""
import math

import numpy as np
import torch

from .. import ops

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
        self.ld = (self.off_channels + 7) // 8 * 8
        self.device = torch.device(device)
        # MegEngine's M.Conv2d default: N(0, sqrt(1 / fan_in)), zero bias (models/params.py states it for P6 / P7)
        rng = np.random.default_rng(seed)
        std = math.sqrt(1.0 / (in_channels * 9))
        state = {}
        for name, co in ((self.OFFSET_NAME, self.off_channels), (self.DCN_NAME, out_channels)):
            state[name + ".weight"] = torch.from_numpy((rng.standard_normal((co, in_channels, 3, 3)) * std).astype(np.float32))
            state[name + ".bias"] = torch.zeros(co, dtype=torch.float32)
        self._grads = None
        self._saved = None
        self._ext = None               # adopt(): (masters, gradients) on the caller's storage, in the kernels' layouts
        self.last_offset_mask = None
        self.load_state_dict(state)

    # ---- parameters ------------------------------------------------------------------------------------------------------------------------
    def names(self):
        return [n + s for n in (self.OFFSET_NAME, self.DCN_NAME) for s in (".weight", ".bias")]

    def state_dict(self):
        return {k: v.detach().cpu().clone() for k, v in self._params.items()}

    def arena_shapes(self):
        """name -> shape of the fp32 masters in the kernels' own layouts (OHWI, the offset convolution's rows padded to ld): what a caller
        that provides the storage (adopt) reserves, for the masters and for the gradients alike."""
        ld, Cin = self.ld, self.in_channels
        return {self.OFFSET_NAME + ".weight": (ld, 3, 3, Cin), self.OFFSET_NAME + ".bias": (ld,),
                self.DCN_NAME + ".weight": (self.out_channels, 3, 3, Cin), self.DCN_NAME + ".bias": (self.out_channels,)}

    def adopt(self, w, g):
        """Live on storage the caller provides (a model's parameter arena): w / g = {name: fp32 device view} in arena_shapes()' layouts.
        The current values move into w; from here on the masters ARE those views (an optimizer step over the arena, then repack()),
        backward writes every parameter gradient straight into g, and params() / state_dict() / grads() keep the reference's OIHW
        layouts as views.  The pad rows of the offset convolution are zero and stay zero (their gradients are sums of zeros)."""
        k = self.off_channels
        old = self._params
        for name, shape in self.arena_shapes().items():
            if tuple(w[name].shape) != shape or tuple(g[name].shape) != shape:
                raise ValueError(f"adopt: {name!r} needs fp32 views of shape {shape}")
            w[name].zero_()
        on, dn = self.OFFSET_NAME, self.DCN_NAME
        w[on + ".weight"][:k].copy_(old[on + ".weight"].permute(0, 2, 3, 1))
        w[on + ".bias"][:k].copy_(old[on + ".bias"])
        w[dn + ".weight"].copy_(old[dn + ".weight"].permute(0, 2, 3, 1))
        w[dn + ".bias"].copy_(old[dn + ".bias"])
        self._ext = (w, g)
        self._params = {on + ".weight": w[on + ".weight"][:k].permute(0, 3, 1, 2), on + ".bias": w[on + ".bias"][:k],
                        dn + ".weight": w[dn + ".weight"].permute(0, 3, 1, 2), dn + ".bias": w[dn + ".bias"]}
        self._grads = dict(off_w=g[on + ".weight"], off_b=g[on + ".bias"], dcn_w=g[dn + ".weight"], dcn_b=g[dn + ".bias"])
        self._pack()

    def load_state_dict(self, state):
        want = {self.OFFSET_NAME + ".weight": (self.off_channels, self.in_channels, 3, 3), self.OFFSET_NAME + ".bias": (self.off_channels,),
                self.DCN_NAME + ".weight": (self.out_channels, self.in_channels, 3, 3), self.DCN_NAME + ".bias": (self.out_channels,)}
        params = {}
        for k, shape in want.items():
            if k not in state:
                raise KeyError(f"missing parameter {k!r}")
            v = torch.as_tensor(np.asarray(state[k]) if not torch.is_tensor(state[k]) else state[k]).detach().float()
            if tuple(v.shape) != shape:
                raise ValueError(f"parameter {k!r}: shape {tuple(v.shape)}, expected {shape}")
            params[k] = v.to(self.device).contiguous()
        if self._ext is not None:          # the masters stay where they are: the values move in
            for k, v in params.items():
                self._params[k].copy_(v)
        else:
            self._params = params
        self._pack()

    def _pack(self):
        """fp32 masters (OIHW) -> the bf16 operands of the kernels; the offset conv's rows padded with zero rows to ld."""
        dev, Cin, ld = self.device, self.in_channels, self.ld
        p = self._params
        if self._ext is not None:          # the masters already have the kernels' layouts: no copies, the packed operands keep their place
            w = self._ext[0]
            self._off_bias, self._dcn_bias = w[self.OFFSET_NAME + ".bias"], w[self.DCN_NAME + ".bias"]
            if getattr(self, "_ext_packed", False) is False:
                self._off_wf = torch.empty((ld, 9, Cin), dtype=torch.bfloat16, device=dev)
                self._off_wd = torch.empty((Cin, 9, ld), dtype=torch.bfloat16, device=dev)
                self._dcn_wf = torch.empty((self.out_channels, 9, Cin), dtype=torch.bfloat16, device=dev)
                self._dcn_wd = torch.empty((Cin, 9, self.out_channels), dtype=torch.bfloat16, device=dev)
                self._ext_packed = True
            ops.weight_pack(w[self.OFFSET_NAME + ".weight"], None, self._off_wf, self._off_wd, ld, 9, Cin)
            ops.weight_pack(w[self.DCN_NAME + ".weight"], None, self._dcn_wf, self._dcn_wd, self.out_channels, 9, Cin)
            return
        w_off = torch.zeros((ld, 3, 3, Cin), dtype=torch.float32, device=dev)
        w_off[: self.off_channels] = p[self.OFFSET_NAME + ".weight"].permute(0, 2, 3, 1)
        self._off_bias = torch.zeros(ld, dtype=torch.float32, device=dev)
        self._off_bias[: self.off_channels] = p[self.OFFSET_NAME + ".bias"]
        self._off_wf = torch.empty((ld, 9, Cin), dtype=torch.bfloat16, device=dev)
        self._off_wd = torch.empty((Cin, 9, ld), dtype=torch.bfloat16, device=dev)
        ops.weight_pack(w_off, None, self._off_wf, self._off_wd, ld, 9, Cin)
        w_dcn = p[self.DCN_NAME + ".weight"].permute(0, 2, 3, 1).contiguous()
        self._dcn_bias = p[self.DCN_NAME + ".bias"]
        self._dcn_wf = torch.empty((self.out_channels, 9, Cin), dtype=torch.bfloat16, device=dev)
        self._dcn_wd = torch.empty((Cin, 9, self.out_channels), dtype=torch.bfloat16, device=dev)
        ops.weight_pack(w_dcn, None, self._dcn_wf, self._dcn_wd, self.out_channels, 9, Cin)

    def _offset_desc(self, N, H, W):
        g = ops.single(N, H, W)
        return ops.conv_desc(g, g, self.in_channels, self.ld, 3, 3, 1, 1)

    # ---- forward / backward ------------------------------------------------------------------------------------------------------------------
    def params(self):
        """The fp32 device masters by name (OIHW).  After changing them in place, repack() rebuilds the bf16 operands."""
        return self._params

    def repack(self):
        self._pack()

    def __call__(self, x):
        N, C, H, W = x.shape
        if C != self.in_channels:
            raise ValueError(f"input has {C} channels, the layer {self.in_channels}")
        xp = x.to(self.device).permute(0, 2, 3, 1).reshape(N * H * W, C).to(torch.bfloat16).contiguous()
        y = self.forward_pm(xp, N, H, W)
        return y.float().view(N, H, W, -1).permute(0, 3, 1, 2).contiguous()

    forward = __call__

    def forward_pm(self, xp, N, H, W):
        """The pixel-major path: xp bf16 [N H W][Cin] on the device -> y bf16 [N H W][Cout]; no NCHW / fp32 round trip."""
        M, C = N * H * W, self.in_channels
        if tuple(xp.shape) != (M, C) or xp.dtype != torch.bfloat16:
            raise ValueError(f"forward_pm: expected bf16 {(M, C)}, got {xp.dtype} {tuple(xp.shape)}")
        om = torch.empty((M, self.ld), dtype=torch.bfloat16, device=self.device)
        ops.conv2d_fwd(self._offset_desc(N, H, W), xp, self._off_wf, self._off_bias, om)
        y = torch.empty((M, self.out_channels), dtype=torch.bfloat16, device=self.device)
        ops.deform_conv_fwd(xp, om, self._dcn_wf, self._dcn_bias, y, N, H, W, C, self.out_channels, self.MODULATED)
        self._saved = (xp, om, N, H, W)
        self.last_offset_mask = om
        return y

    def backward(self, dy, accumulate=False):
        """Gradient of the last forward's output (NCHW) -> gradient of its input (NCHW fp32); parameter gradients in grads().
        accumulate: add to the parameter gradients of the previous backward instead of overwriting them."""
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        _, _, N, H, W = self._saved
        Cin, Cout, dev = self.in_channels, self.out_channels, self.device
        if tuple(dy.shape) != (N, Cout, H, W):
            raise ValueError(f"gradient shape {tuple(dy.shape)} does not match the forward output {(N, Cout, H, W)}")
        g = dy.to(dev).permute(0, 2, 3, 1).reshape(N * H * W, Cout).to(torch.bfloat16).contiguous()
        dx = self.backward_pm(g, accumulate)
        return dx.float().view(N, H, W, Cin).permute(0, 3, 1, 2).contiguous()

    def backward_pm(self, g, accumulate=False):
        """g bf16 [N H W][Cout] -> d_x bf16 [N H W][Cin]; parameter gradients in grads()."""
        if self._saved is None:
            raise RuntimeError("backward() before a forward")
        xp, om, N, H, W = self._saved
        Cin, Cout, ld, dev = self.in_channels, self.out_channels, self.ld, self.device
        M = N * H * W
        if tuple(g.shape) != (M, Cout) or g.dtype != torch.bfloat16:
            raise ValueError(f"backward_pm: expected bf16 {(M, Cout)}, got {g.dtype} {tuple(g.shape)}")
        if self._ext is not None:
            pass                           # (the gradients are the adopted views: nothing is allocated per step)
        elif self._grads is None or not accumulate:
            accumulate = False
            self._grads = dict(off_w=torch.empty((ld, 3, 3, Cin), dtype=torch.float32, device=dev),
                               off_b=torch.empty(ld, dtype=torch.float32, device=dev),
                               dcn_w=torch.empty((Cout, 3, 3, Cin), dtype=torch.float32, device=dev),
                               dcn_b=torch.empty(Cout, dtype=torch.float32, device=dev))
        gr = self._grads
        d = self._offset_desc(N, H, W)
        nbytes = max(ops.deform_conv_wgrad_workspace_bytes(N, H, W, Cin, Cout), ops.deform_conv_bwd_data_workspace_bytes(N, H, W, Cin, Cout),
                     ops.conv2d_wgrad_bias_workspace_bytes(d))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ops.deform_conv_wgrad(xp, om, g, gr["dcn_w"], gr["dcn_b"], ws, N, H, W, Cin, Cout, self.MODULATED, accumulate=accumulate)
        dx_dcn = torch.empty((M, Cin), dtype=torch.bfloat16, device=dev)
        d_om = torch.empty((M, ld), dtype=torch.bfloat16, device=dev)
        ops.deform_conv_bwd_data(xp, om, g, self._dcn_wd, dx_dcn, d_om, ws, N, H, W, Cin, Cout, self.MODULATED)
        # the offset convolution reads the same input: its data gradient lands on top of the deformable part
        ops.conv2d_wgrad_bias(d, xp, d_om, gr["off_w"], gr["off_b"], ws, accumulate=accumulate)
        dx = torch.empty_like(dx_dcn)
        ops.conv2d_dgrad(d, d_om, self._off_wd, dx, add=dx_dcn, flags=ops.EPI_ADD_BEFORE)
        self.last_d_offset_mask = d_om
        return dx

    def grads(self):
        """Parameter gradients of the last backward() under the reference's names, OIHW fp32."""
        if self._grads is None:
            raise RuntimeError("grads() before a backward")
        gr, k = self._grads, self.off_channels
        return {self.OFFSET_NAME + ".weight": gr["off_w"][:k].permute(0, 3, 1, 2).contiguous(), self.OFFSET_NAME + ".bias": gr["off_b"][:k].clone(),
                self.DCN_NAME + ".weight": gr["dcn_w"].permute(0, 3, 1, 2).contiguous(), self.DCN_NAME + ".bias": gr["dcn_b"].clone()}


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
