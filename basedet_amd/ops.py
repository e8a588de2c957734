"""Thin torch-tensor wrappers over the C ABI (include/basedet_hip.h).  torch only carries memory and the stream.

Activations are "pixel-major" bf16 tensors of shape (N * pix_per_img, C) described by a `Geom`.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from . import _lib
from ._lib import ConvDesc, EPI_ADD_AFTER, EPI_ADD_BEFORE, EPI_MASK, EPI_RELU, EPI_SPARSE, check, f32arr, i32arr, ptr, stream_ptr


@dataclass
class Geom:
    """Pixel layout of an NHWC activation that may hold several pyramid levels per image."""
    N: int
    H: List[int]
    W: List[int]
    off: List[int] = field(default_factory=list)   # pixel offset of each level inside one image
    pix_per_img: int = 0

    def __post_init__(self):
        if not self.off:
            o = 0
            self.off = []
            for h, w in zip(self.H, self.W):
                self.off.append(o)
                o += h * w
            if not self.pix_per_img:
                self.pix_per_img = o
        if not self.pix_per_img:
            self.pix_per_img = sum(h * w for h, w in zip(self.H, self.W))

    @property
    def nlev(self):
        return len(self.H)

    @property
    def pixels(self):
        return self.N * self.pix_per_img

    def level(self, i):
        """Single-level view that keeps the parent's strides."""
        return Geom(self.N, [self.H[i]], [self.W[i]], [self.off[i]], self.pix_per_img)

    def conv_out(self, R, stride, pad):
        H = [(h + 2 * pad - R) // stride + 1 for h in self.H]
        W = [(w + 2 * pad - R) // stride + 1 for w in self.W]
        return Geom(self.N, H, W)


def single(N, H, W):
    return Geom(N, [H], [W])


def conv_desc(gin: Geom, gout: Geom, Cin, Cout, R, S, stride, pad) -> ConvDesc:
    d = ConvDesc()
    d.N, d.Cin, d.Cout, d.R, d.S, d.stride, d.pad, d.nseg = gin.N, Cin, Cout, R, S, stride, pad, gin.nlev
    assert gin.nlev == gout.nlev <= _lib.BD_MAX_SEGS
    for i in range(gin.nlev):
        d.Hi[i], d.Wi[i], d.Ho[i], d.Wo[i] = gin.H[i], gin.W[i], gout.H[i], gout.W[i]
        d.in_off[i], d.out_off[i] = gin.off[i], gout.off[i]
    d.in_pix_per_img, d.out_pix_per_img = gin.pix_per_img, gout.pix_per_img
    return d


def L():
    return _lib.load()


# ---- per-call kernel routing (bd_conv_desc.route / .sr_seed) ---------------------------------------------------------------------------
# The library keeps no routing state (round 6: the bd_*_set_* knobs are gone).  A test or an A/B harness that wants a route sets it HERE;
# every wrapper below that takes a descriptor stamps the current words into it right before the call.  Production code never touches this.
_ROUTE = [0, 0, 0, 0]          # (route + 1) words: dense 1x1 mode, 3x3 / generic bit mask, weight-gradient bit mask, fp8 forward patch kernel
_SR_SEED = [0]                 # e5m2 stochastic-rounding seed of the calls made from now on (the fp8 model sets it per step)
_ROUTE_NAMES = {"dense1x1": 0, "patch3x3": 1, "wgrad": 2, "fp8_patch": 3}


def set_route(**kw):
    """set_route(dense1x1=mode, patch3x3=mask, wgrad=mask, fp8_patch=0|1); a value of None returns that word to the library's default.
    The meanings: include/basedet_hip.h, bd_conv_desc.route."""
    for k, v in kw.items():
        _ROUTE[_ROUTE_NAMES[k]] = 0 if v is None else int(v) + 1


def reset_route():
    _ROUTE[:] = [0, 0, 0, 0]
    _SR_SEED[0] = 0


def _stamp(d):
    d.route[0], d.route[1], d.route[2], d.route[3] = _ROUTE
    d.sr_seed = _SR_SEED[0]
    return d


# ---- dense path -------------------------------------------------------------------------------------------
def conv2d_fwd(d, x, w_packed, bias, y, add=None, flags=0, bits=None, y8=None, q_scale=1.0):
    """bits: optional uint32 [Cout/32][M] output, the bit-packed ReLU mask of y; y8: optional uint8 e4m3 twin of y (dense 1x1 launches
    only: bd_conv2d_fwd_bits / bd_conv2d_fwd_ex)."""
    if y8 is not None:
        check(L().bd_conv2d_fwd_ex(C.byref(_stamp(d)), ptr(x), ptr(w_packed), ptr(bias), ptr(add), ptr(y), ptr(bits), ptr(y8), float(q_scale), flags,
                                   stream_ptr()), "bd_conv2d_fwd_ex")
        return y
    if bits is not None:
        check(L().bd_conv2d_fwd_bits(C.byref(_stamp(d)), ptr(x), ptr(w_packed), ptr(bias), ptr(add), ptr(y), ptr(bits), flags, stream_ptr()),
              "bd_conv2d_fwd_bits")
        return y
    check(L().bd_conv2d_fwd(C.byref(_stamp(d)), ptr(x), ptr(w_packed), ptr(bias), ptr(add), ptr(y), flags, stream_ptr()), "bd_conv2d_fwd")
    return y


def conv2d_dgrad(d, g, w_packed_t, dx, add=None, mask=None, flags=0, maskbits=None, dx8=None, q_scale=1.0):
    """maskbits: the ReLU mask as written by conv2d_fwd(bits=...) instead of the bf16 activation `mask` (bd_conv2d_dgrad_bits);
    dx8: optional uint8 e5m2 twin of dx * q_scale (dense 1x1 launches only: bd_conv2d_dgrad_ex)."""
    if dx8 is not None:
        check(L().bd_conv2d_dgrad_ex(C.byref(_stamp(d)), ptr(g), ptr(w_packed_t), ptr(add), ptr(mask), ptr(maskbits), ptr(dx), ptr(dx8),
                                     float(q_scale), flags, stream_ptr()), "bd_conv2d_dgrad_ex")
        return dx
    if maskbits is not None:
        check(L().bd_conv2d_dgrad_bits(C.byref(_stamp(d)), ptr(g), ptr(w_packed_t), ptr(add), ptr(maskbits), ptr(dx), flags, stream_ptr()),
              "bd_conv2d_dgrad_bits")
        return dx
    check(L().bd_conv2d_dgrad(C.byref(_stamp(d)), ptr(g), ptr(w_packed_t), ptr(add), ptr(mask), ptr(dx), flags, stream_ptr()), "bd_conv2d_dgrad")
    return dx


def conv2d_dgrad_gskip_bytes(d):
    """Scratch bytes a gradient-skipping data gradient (bd_conv_desc.gskip) needs at d.gskip_ws; 0 where the hint does not apply."""
    return int(L().bd_conv2d_dgrad_gskip_bytes(C.byref(d)))


def conv2d_gskip_map_bytes(d, of_dx=False):
    """Bytes of the liveness map of d's gradient operand g (of_dx=False) or of its data gradient dx (bd_conv_desc.gskip_gmap / gskip_dxmap)."""
    return int(L().bd_conv2d_gskip_map_bytes(C.byref(d), int(bool(of_dx))))


def gskip_map_scan(d, t, gmap, of_dx=False):
    """Fill the liveness map of tensor t (g or dx of d) by scanning all of it (bd_gskip_map_scan)."""
    check(L().bd_gskip_map_scan(C.byref(d), int(bool(of_dx)), ptr(t), ptr(gmap), gmap.numel() * gmap.element_size(), stream_ptr()),
          "bd_gskip_map_scan")
    return gmap


def gskip_desc(d, scratch=None, gmap=None, dxmap=None, dx_clean=False):
    """A copy of descriptor d with the gradient-skip hint set (include/basedet_hip.h, bd_conv_desc.gskip): its bf16 data and weight gradients
    scan g and compute only the patches a nonzero g reaches (same bits).  scratch: device tensor of conv2d_dgrad_gskip_bytes(d) bytes for
    the data gradient (the weight gradient keeps its flags in ws, sized from this descriptor).  gmap: the liveness map of g, left by the
    call that wrote g (no scan); dxmap: the map of dx for the data gradient to write; dx_clean: the promise that dx holds +0 outside
    the list the previous call left in dxmap (int32 device tensors of conv2d_gskip_map_bytes)."""
    h = ConvDesc.from_buffer_copy(d)
    h.gskip = 1
    if scratch is not None:
        h.gskip_ws = scratch.data_ptr()
        h.gskip_ws_bytes = scratch.numel() * scratch.element_size()
    if gmap is not None:
        h.gskip_gmap = gmap.data_ptr()
        h.gskip_gmap_bytes = gmap.numel() * gmap.element_size()
    if dxmap is not None:
        h.gskip_dxmap = dxmap.data_ptr()
        h.gskip_dxmap_bytes = dxmap.numel() * dxmap.element_size()
    h.gskip_dx_clean = int(bool(dx_clean))
    return h


def fwd_live_map_bytes(d):
    """Bytes of one forward liveness map (bd_conv_desc.fwd_map) of d's output geometry; 0 for a descriptor that is not 3x3 / stride 1 / pad 1."""
    return int(L().bd_fwd_live_map_bytes(C.byref(d)))


def fwd_live_maps(d, labels, A, maps, reset=False):
    """The forward liveness maps of a tower below a predictor that is read only at foreground anchors (bd_fwd_live_maps): maps[k - 1] (int32
    device tensors of fwd_live_map_bytes(d)) gets the 4 x 16 patches within k pixels of a pixel with a label > 0.  labels: int32 (N, pixels
    per image * A), pyramid order.  reset: the maps hold no state of an earlier call."""
    if labels.dtype != torch.int32 or labels.numel() != d.N * d.out_pix_per_img * A:
        raise _lib.BasedetHipError(f"fwd_live_maps: labels must be int32 with N * pixels * A = {d.N * d.out_pix_per_img * A} entries")
    nb = min(m.numel() * m.element_size() for m in maps)
    arr = (C.c_void_p * len(maps))(*[ptr(m).value for m in maps])
    check(L().bd_fwd_live_maps(C.byref(d), ptr(labels), int(A), len(maps), arr, nb, int(bool(reset)), stream_ptr()), "bd_fwd_live_maps")
    return maps


def fwd_map_desc(d, fmap, clean=False):
    """A copy of descriptor d whose forward launch follows the liveness map fmap of its output (bd_conv_desc.fwd_map): the patches on the
    map's current list get the dense launch's bits, every other patch +0.  clean: the promise that the output still holds +0 outside
    the list of the previous call with this map (bd_conv_desc.fwd_clean)."""
    h = ConvDesc.from_buffer_copy(d)
    h.fwd_map = fmap.data_ptr()
    h.fwd_map_bytes = fmap.numel() * fmap.element_size()
    h.fwd_clean = int(bool(clean))
    return h


def quantize_fp8(x, scale, q):
    """q (uint8, same element count) = e4m3(clamp(x * scale)) of a bf16 tensor."""
    check(L().bd_quantize_fp8(ptr(x), x.numel(), float(scale), ptr(q), stream_ptr()), "bd_quantize_fp8")
    return q


def weight_pack_fp8(w, row_scale, Cout, RS, Cin, act_scale, wq, wscale):
    check(L().bd_weight_pack_fp8(ptr(w), ptr(row_scale), Cout, RS, Cin, float(act_scale), ptr(wq), ptr(wscale), stream_ptr()),
          "bd_weight_pack_fp8")


def conv2d_fwd_fp8(d, xq, wq, wscale, bias, y, add=None, flags=0, y8=None, q_scale=1.0):
    """y8: optional uint8 twin of y (e4m3(y * q_scale)) for a following fp8 convolution."""
    check(L().bd_conv2d_fwd_fp8_ex(C.byref(_stamp(d)), ptr(xq), ptr(wq), ptr(wscale), ptr(bias), ptr(add), ptr(y), ptr(y8), float(q_scale), flags,
                                   stream_ptr()), "bd_conv2d_fwd_fp8")
    return y


def quantize_bf8(x, scale, q):
    """q (uint8) = e5m2(clamp(x * scale)) of a bf16 tensor (gradients); rounding: fp8_set_stochastic_rounding."""
    check(L().bd_quantize_bf8(ptr(x), x.numel(), float(scale), ptr(q), _SR_SEED[0], stream_ptr()), "bd_quantize_bf8")
    return q


def fp8_set_stochastic_rounding(seed):
    """seed != 0: the e5m2 quantisers CALLED from now on round stochastically (hash of seed and element index); 0: to nearest.  Python-side
    state: the seed travels with every call (bd_conv_desc.sr_seed, bd_quantize_bf8's argument)."""
    _SR_SEED[0] = int(seed) & 0xFFFFFFFF


def absmax_bf16(x, out):
    """out[0] (fp32, device) = max(out[0], max |x|) of a bf16 tensor."""
    check(L().bd_absmax_bf16(ptr(x), x.numel(), ptr(out), stream_ptr()), "bd_absmax_bf16")


def weight_pack_fp8_t(w, row_scale, Cout, RS, Cin, grad_scale, wq_t, wscale_t):
    check(L().bd_weight_pack_fp8_t(ptr(w), ptr(row_scale), Cout, RS, Cin, float(grad_scale), ptr(wq_t), ptr(wscale_t), stream_ptr()),
          "bd_weight_pack_fp8_t")


def conv2d_dgrad_fp8(d, g8, wq_t, wscale_t, dx, add=None, mask=None, flags=0, dx8=None, q_scale=1.0):
    check(L().bd_conv2d_dgrad_fp8(C.byref(_stamp(d)), ptr(g8), ptr(wq_t), ptr(wscale_t), ptr(add), ptr(mask), ptr(dx), ptr(dx8), float(q_scale),
                                  flags, stream_ptr()), "bd_conv2d_dgrad_fp8")
    return dx


def conv1x1_fp8(d, mode, xq, wq, wscale, bias, y, add=None, mask=None, maskbits=None, bits=None, y8=None, q_scale=1.0, flags=0):
    """Dense 1x1 launch on one-byte operands: mode 0 forward (xq e4m3), mode 1 data gradient (xq = e5m2 gradient)."""
    check(L().bd_conv1x1_fp8(C.byref(_stamp(d)), mode, ptr(xq), ptr(wq), ptr(wscale), ptr(bias), ptr(add), ptr(mask), ptr(maskbits), ptr(y),
                             ptr(bits), ptr(y8), float(q_scale), flags, stream_ptr()), "bd_conv1x1_fp8")
    return y


def conv2d_wgrad_fp8_workspace_bytes(d):
    return int(L().bd_conv2d_wgrad_fp8_workspace_bytes(C.byref(_stamp(d))))


def conv2d_wgrad_fp8(d, x8, g8, inv_scale, dw, ws, row_scale=None, accumulate=False):
    """Weight gradient of a 3x3 / stride-1 convolution from the one-byte twins (x8 e4m3, g8 e5m2); dw fp32 [Cout][9][Cin]."""
    check(L().bd_conv2d_wgrad_fp8(C.byref(_stamp(d)), ptr(x8), ptr(g8), float(inv_scale), ptr(row_scale), ptr(dw), int(accumulate), ptr(ws),
                                  ws.numel() * ws.element_size(), stream_ptr()), "bd_conv2d_wgrad_fp8")
    return dw


def conv1x1_fp8_ok(d, mode):
    """True when bd_conv1x1_fp8 takes this descriptor."""
    K, CO = (d.Cin, d.Cout) if mode == 0 else (d.Cout, d.Cin)
    return dense_1x1_bits_ok(d) and K % 128 == 0 and CO % 32 == 0


def fp8_dgrad_ok(d):
    """True when bd_conv2d_dgrad_fp8 takes this descriptor (conv3x3_pp8.hip, mode 1)."""
    same = all(d.Hi[i] == d.Ho[i] and d.Wi[i] == d.Wo[i] for i in range(d.nseg))
    return d.R == 3 and d.S == 3 and d.stride == 1 and d.pad == 1 and same and d.Cin > 128 and d.Cin % 8 == 0 and d.Cout % 16 == 0


def dense_1x1_bits_ok(d):
    """True when bd_conv2d_fwd_bits / bd_conv2d_dgrad_bits take this descriptor (conv1x1.hip)."""
    return (d.R == 1 and d.S == 1 and d.stride == 1 and d.pad == 0 and d.nseg == 1 and d.in_off[0] == 0 and d.out_off[0] == 0
            and d.in_pix_per_img == d.Hi[0] * d.Wi[0] and d.out_pix_per_img == d.Ho[0] * d.Wo[0]
            and d.Cin % 32 == 0 and d.Cout % 32 == 0 and d.N * d.in_pix_per_img * max(d.Cin, d.Cout) * 2 < 0x7fffffff)


def conv2d_wgrad_workspace_bytes(d):
    return int(L().bd_conv2d_wgrad_workspace_bytes(C.byref(_stamp(d))))


def conv2d_wgrad(d, x, g, dw, ws, row_scale=None, accumulate=False):
    check(L().bd_conv2d_wgrad(C.byref(_stamp(d)), ptr(x), ptr(g), ptr(row_scale), ptr(dw), int(accumulate), ptr(ws),
                              ws.numel() * ws.element_size(), stream_ptr()), "bd_conv2d_wgrad")
    return dw


def conv2d_wgrad_bias_workspace_bytes(d):
    return int(L().bd_conv2d_wgrad_bias_workspace_bytes(C.byref(_stamp(d))))


def conv2d_wgrad_bias(d, x, g, dw, dbias, ws, row_scale=None, accumulate=False):
    """Weight and bias gradient in one call (the 3x3 patch kernel sums g's columns while staging them)."""
    check(L().bd_conv2d_wgrad_bias(C.byref(_stamp(d)), ptr(x), ptr(g), ptr(row_scale), ptr(dw), ptr(dbias), int(accumulate), ptr(ws),
                                   ws.numel() * ws.element_size(), stream_ptr()), "bd_conv2d_wgrad_bias")
    return dw


def fpn_deconv_pack(w, C, w_fwd, w_dgrad):
    """fp32 master [C][4][4][C] (conv view, OHWI) -> the bf16 operands of fpn_deconv_fwd / fpn_deconv_dgrad."""
    check(L().bd_fpn_deconv_pack(ptr(w), C, ptr(w_fwd), ptr(w_dgrad), stream_ptr()), "bd_fpn_deconv_pack")


def fpn_deconv_fwd(x, w_fwd, y, N, Hc, Wc, C, add=None):
    """y [N][2Hc][2Wc][C] = bf16(add + conv_transpose(x [N][Hc][Wc][C], W, 4x4 / stride 2 / pad 1)); add may be y itself."""
    check(L().bd_fpn_deconv_fwd(ptr(x), ptr(w_fwd), ptr(add), ptr(y), N, Hc, Wc, 2 * Hc, 2 * Wc, C, stream_ptr()), "bd_fpn_deconv_fwd")
    return y


def fpn_deconv_dgrad(dy, w_dgrad, dx, N, Hc, Wc, C, add=None):
    """dx [N][Hc][Wc][C] = bf16(add + conv4x4s2p1(dy [N][2Hc][2Wc][C], W)); add may be dx itself."""
    check(L().bd_fpn_deconv_dgrad(ptr(dy), ptr(w_dgrad), ptr(add), ptr(dx), N, Hc, Wc, 2 * Hc, 2 * Wc, C, stream_ptr()), "bd_fpn_deconv_dgrad")
    return dx


def fpn_deconv_wgrad_workspace_bytes(N, Hc, Wc, C):
    return int(L().bd_fpn_deconv_wgrad_workspace_bytes(N, Hc, Wc, C))


def fpn_deconv_wgrad(x, dy, dw, ws, N, Hc, Wc, C, accumulate=False):
    """dw [C][4][4][C] fp32 (+)= the weight gradient of fpn_deconv_fwd (fixed-order split sums: reproducible)."""
    check(L().bd_fpn_deconv_wgrad(ptr(x), ptr(dy), ptr(dw), int(accumulate), ptr(ws), ws.numel() * ws.element_size(), N, Hc, Wc,
                                  2 * Hc, 2 * Wc, C, stream_ptr()), "bd_fpn_deconv_wgrad")
    return dw


_DCN_CONFIG = (3, 1, 1, 1, 1)      # kernel_size, stride, padding, dilation, deformable_groups: the one configuration deform_conv.hip builds


def deform_conv_fwd(x, om, w_fwd, bias, y, N, H, W, Cin, Cout, modulated, config=_DCN_CONFIG):
    """y [N H W][Cout] = bf16(bias + deformable 3x3 conv of x [N H W][Cin]) at the positions (and, modulated, masks) of om [N H W][ld]:
    the raw offset-conv output (include/basedet_hip.h, bd_deform_conv_fwd); w_fwd = weight_pack's forward layout."""
    check(L().bd_deform_conv_fwd(ptr(x), ptr(om), ptr(w_fwd), ptr(bias), ptr(y), N, H, W, Cin, Cout, om.shape[-1], int(modulated), *config,
                                 stream_ptr()), "bd_deform_conv_fwd")
    return y


def deform_conv_wgrad_workspace_bytes(N, H, W, Cin, Cout):
    return int(L().bd_deform_conv_wgrad_workspace_bytes(N, H, W, Cin, Cout))


def deform_conv_wgrad(x, om, dy, dw, dbias, ws, N, H, W, Cin, Cout, modulated, accumulate=False, config=_DCN_CONFIG):
    """dw [Cout][3][3][Cin] fp32 and dbias [Cout] fp32 (or None) (+)= the parameter gradients of deform_conv_fwd (reproducible)."""
    check(L().bd_deform_conv_wgrad(ptr(x), ptr(om), ptr(dy), ptr(dw), ptr(dbias), int(accumulate), ptr(ws), ws.numel() * ws.element_size(),
                                   N, H, W, Cin, Cout, om.shape[-1], int(modulated), *config, stream_ptr()), "bd_deform_conv_wgrad")
    return dw


def deform_conv_bwd_data_workspace_bytes(N, H, W, Cin, Cout):
    return int(L().bd_deform_conv_bwd_data_workspace_bytes(N, H, W, Cin, Cout))


def deform_conv_bwd_data(x, om, dy, w_dgrad, d_x, d_om, ws, N, H, W, Cin, Cout, modulated, add=None, config=_DCN_CONFIG):
    """d_x [N H W][Cin] = bf16(data gradient [+ add]) and d_om [N H W][ld] = the gradient of the raw offset-conv output (reproducible;
    d_x's last bits are not: fp32 atomics); w_dgrad = weight_pack's dgrad layout."""
    check(L().bd_deform_conv_bwd_data(ptr(x), ptr(om), ptr(dy), ptr(w_dgrad), ptr(add), ptr(d_x), ptr(d_om), ptr(ws),
                                      ws.numel() * ws.element_size(), N, H, W, Cin, Cout, om.shape[-1], int(modulated), *config,
                                      stream_ptr()), "bd_deform_conv_bwd_data")
    return d_x, d_om


def stem_conv7x7_fwd(N, H, W, x_halo, w_stem, bias, y):
    check(L().bd_stem_conv7x7_fwd(N, H, W, ptr(x_halo), ptr(w_stem), ptr(bias), ptr(y), stream_ptr()), "bd_stem_conv7x7_fwd")
    return y


def stem_conv7x7_raw_fwd(N, H, W, x_halo, w_stem, y):
    """The bare 7x7 convolution (no shift, no ReLU): the stem under a live backbone norm; w_stem packed without a row scale."""
    check(L().bd_stem_conv7x7_raw_fwd(N, H, W, ptr(x_halo), ptr(w_stem), ptr(y), stream_ptr()), "bd_stem_conv7x7_raw_fwd")
    return y


def stem_weight_pack(w, row_scale, w_stem):
    check(L().bd_stem_weight_pack(ptr(w), ptr(row_scale), ptr(w_stem), stream_ptr()), "bd_stem_weight_pack")


def maxpool3x3s2_bwd(g_pool, stem_out, pool_out, N, Hs, Ws, Cn, g_stem):
    """Adjoint of maxpool3x3s2_fwd, gated by stem_out > 0 (first-maximum rule, no atomics): g_stem = dL/d(pre-activation) of stem_out."""
    check(L().bd_maxpool3x3s2_bwd(ptr(g_pool), ptr(stem_out), ptr(pool_out), N, Hs, Ws, Cn, ptr(g_stem), stream_ptr()), "bd_maxpool3x3s2_bwd")
    return g_stem


def stem_conv7x7_wgrad_workspace_bytes(N, H, W):
    return int(L().bd_stem_conv7x7_wgrad_workspace_bytes(N, H, W))


def stem_conv7x7_wgrad(N, H, W, x_halo, g_stem, dw, ws, row_scale=None, accumulate=False):
    """Weight gradient of stem_conv7x7_fwd; dw fp32 [64][7][7][3] (OHWI, what stem_weight_pack reads)."""
    check(L().bd_stem_conv7x7_wgrad(N, H, W, ptr(x_halo), ptr(g_stem), ptr(row_scale), ptr(dw), int(accumulate), ptr(ws),
                                    ws.numel() * ws.element_size(), stream_ptr()), "bd_stem_conv7x7_wgrad")
    return dw


def weight_pack(w, row_scale, w_fwd, w_dgrad, Cout, RS, Cin):
    check(L().bd_weight_pack(ptr(w), ptr(row_scale), ptr(w_fwd), ptr(w_dgrad), Cout, RS, Cin, stream_ptr()), "bd_weight_pack")


def build_pack_table(entries, device):
    """entries: [(w, row_scale | None, w_fwd | None, w_dgrad | None, Cout, RS, Cin)] -> (device byte tensor of bd_pack_desc, n,
    total blocks).  The tensors must stay alive (and in place) as long as the table is used."""
    import ctypes as C
    import numpy as np
    from ._lib import PackDesc
    arr = (PackDesc * len(entries))()
    start = 0
    for i, (w, rs, wf, wd, co, r, ci) in enumerate(entries):
        arr[i].w = w.data_ptr()
        arr[i].row_scale = rs.data_ptr() if rs is not None else None
        arr[i].w_fwd = wf.data_ptr() if wf is not None else None
        arr[i].w_dgrad = wd.data_ptr() if wd is not None else None
        arr[i].Cout, arr[i].RS, arr[i].Cin, arr[i].block_start = co, r, ci, start
        start += int(L().bd_weight_pack_blocks(co, r, ci))
    raw = np.frombuffer(bytes(arr), dtype=np.uint8).copy()
    return torch.from_numpy(raw).to(device), len(entries), start


def weight_pack_multi(table):
    t, n, blocks = table
    check(L().bd_weight_pack_multi(ptr(t), n, blocks, stream_ptr()), "bd_weight_pack_multi")


def colsum_workspace_bytes(Cn):
    return int(L().bd_colsum_workspace_bytes(Cn))


def colsum_bf16(g, rows, Cn, out, ws, accumulate=False, geom=None):
    """geom: single-level Geom selecting the pixel rows of one pyramid level (default: all `rows` rows)."""
    if geom is None:
        n, ppi, off, cnt = 1, rows, 0, rows
    else:
        assert geom.nlev == 1
        n, ppi, off, cnt = geom.N, geom.pix_per_img, geom.off[0], geom.H[0] * geom.W[0]
    check(L().bd_colsum_bf16(ptr(g), n, ppi, off, cnt, Cn, ptr(out), int(accumulate), ptr(ws), ws.numel() * ws.element_size(),
                             stream_ptr()), "bd_colsum_bf16")
    return out


# ---- image ops --------------------------------------------------------------------------------------------
def pad_normalize(x, Hp, Wp, mean, std, out):
    N, _, H, W = x.shape
    check(L().bd_pad_normalize(ptr(x), N, H, W, Hp, Wp, f32arr(mean), f32arr(std), ptr(out), stream_ptr()), "bd_pad_normalize")
    return out


def pad_normalize_nchw(x, Hp, Wp, mean, std, out):
    N, _, H, W = x.shape
    check(L().bd_pad_normalize_nchw(ptr(x), N, H, W, Hp, Wp, f32arr(mean), f32arr(std), ptr(out), stream_ptr()), "bd_pad_normalize_nchw")
    return out


def resize_pad_normalize(packed, descs, Hp, Wp, mean, std, out):
    """bd_resize_pad_normalize: packed = uint8 device tensor holding the raw HWC images, descs = their _lib.ImageDesc records (host);
    out = bf16 (N, Hp + 6, Wp + 8, 4), written whole."""
    N = len(descs)
    assert packed.dtype == torch.uint8 and out.dtype == torch.bfloat16 and out.numel() == N * (Hp + 6) * (Wp + 8) * 4
    arr = descs if isinstance(descs, C.Array) else (_lib.ImageDesc * N)(*descs)
    check(L().bd_resize_pad_normalize(ptr(packed), packed.numel(), arr, N, int(Hp), int(Wp), f32arr(mean), f32arr(std), ptr(out),
                                      stream_ptr()), "bd_resize_pad_normalize")
    return out


def resize_bilinear_normalize(x, dst_h, dst_w, Hp, Wp, mean, std, out):
    """bd_resize_bilinear_normalize: x fp32 (N, 3, H, W) on the device -> out bf16 (N, Hp + 6, Wp + 8, 4), written whole: the batch resized
    to (dst_h, dst_w) by torch.nn.functional.interpolate's bilinear rule (align_corners=False), padded and normalised."""
    N, _, H, W = x.shape
    check(L().bd_resize_bilinear_normalize(ptr(x), N, H, W, int(dst_h), int(dst_w), int(Hp), int(Wp), f32arr(mean), f32arr(std), ptr(out),
                                           stream_ptr()), "bd_resize_bilinear_normalize")
    return out


def affine_jitter_workspace_bytes(N, out_h, out_w):
    return int(L().bd_affine_jitter_workspace_bytes(int(N), int(out_h), int(out_w)))


def affine_jitter_normalize(packed, descs, out_h, out_w, mean, std, out, ws=None, u8_out=None):
    """bd_affine_jitter_normalize: packed = uint8 device tensor holding the raw HWC images, descs = their _lib.AffineDesc records (host);
    out = bf16 (N, out_h + 6, out_w + 8, 4), written whole; ws = uint8 workspace of affine_jitter_workspace_bytes (needed when an image
    has contrast enabled); u8_out = optional uint8 (N, out_h, out_w, 3) for the bytes before normalisation."""
    N = len(descs)
    assert packed.dtype == torch.uint8 and out.dtype == torch.bfloat16 and out.numel() == N * (out_h + 6) * (out_w + 8) * 4
    assert u8_out is None or (u8_out.dtype == torch.uint8 and u8_out.numel() == N * out_h * out_w * 3)
    assert ws is None or ws.dtype == torch.uint8
    arr = descs if isinstance(descs, C.Array) else (_lib.AffineDesc * N)(*descs)
    check(L().bd_affine_jitter_normalize(ptr(packed), packed.numel(), arr, N, int(out_h), int(out_w), f32arr(mean), f32arr(std), ptr(out),
                                         ptr(u8_out), ptr(ws), 0 if ws is None else ws.numel(), stream_ptr()),
          "bd_affine_jitter_normalize")
    return out


def stem_pool_fwd(N, H, W, x_halo, w_stem, bias, y_pool):
    """stem_conv7x7_fwd + maxpool3x3s2_fwd in one launch (bit-identical; the half-resolution tensor is never written)."""
    check(L().bd_stem_pool_fwd(N, H, W, ptr(x_halo), ptr(w_stem), ptr(bias), ptr(y_pool), stream_ptr()), "bd_stem_pool_fwd")


def maxpool3x3s2_fwd(x, N, H, W, Cn, y):
    check(L().bd_maxpool3x3s2_fwd(ptr(x), N, H, W, Cn, ptr(y), stream_ptr()), "bd_maxpool3x3s2_fwd")
    return y


def upsample2x_add_fwd(top, gtop: Geom, lat, glat: Geom, Cn):
    check(L().bd_upsample2x_add_fwd(ptr(top), gtop.pix_per_img, gtop.off[0], ptr(lat), glat.pix_per_img, glat.off[0],
                                    gtop.N, gtop.H[0], gtop.W[0], Cn, stream_ptr()), "bd_upsample2x_add_fwd")


def upsample2x_add_bwd(dlat, glat: Geom, dtop, gtop: Geom, Cn, accumulate):
    check(L().bd_upsample2x_add_bwd(ptr(dlat), glat.pix_per_img, glat.off[0], ptr(dtop), gtop.pix_per_img, gtop.off[0],
                                    gtop.N, gtop.H[0], gtop.W[0], Cn, int(accumulate), stream_ptr()), "bd_upsample2x_add_bwd")


def relu_bf16(x, y):
    check(L().bd_relu_bf16(ptr(x), ptr(y), x.numel(), stream_ptr()), "bd_relu_bf16")
    return y


def relu_bwd_bf16(g, mask, y, add=None):
    check(L().bd_relu_bwd_bf16(ptr(g), ptr(mask), ptr(add), ptr(y), g.numel(), stream_ptr()), "bd_relu_bwd_bf16")
    return y


def add_bf16(a, b, y):
    check(L().bd_add_bf16(ptr(a), ptr(b), ptr(y), a.numel(), stream_ptr()), "bd_add_bf16")
    return y


# ---- box ops ----------------------------------------------------------------------------------------------
def anchors_generate(H, W, stride, offset, base, out):
    check(L().bd_anchors_generate(H, W, stride, float(offset), ptr(base), base.shape[0], ptr(out), stream_ptr()), "bd_anchors_generate")
    return out


def points_generate(H, W, stride, offset, A, out):
    check(L().bd_points_generate(H, W, stride, float(offset), A, ptr(out), stream_ptr()), "bd_points_generate")
    return out


def box_pairwise(b1, b2, mode):
    m, n = b1.shape[0], b2.shape[0]
    out = torch.empty((m, n), dtype=torch.float32, device=b1.device)
    check(L().bd_box_pairwise(ptr(b1), m, ptr(b2), n, mode, ptr(out), stream_ptr()), "bd_box_pairwise")
    return out


def box_encode(anchors, gt, mean, std):
    out = torch.empty_like(anchors)
    check(L().bd_box_encode(ptr(anchors), ptr(gt), anchors.shape[0], f32arr(mean), f32arr(std), ptr(out), stream_ptr()), "bd_box_encode")
    return out


def box_decode(anchors, deltas, mean, std):
    out = torch.empty_like(anchors)
    check(L().bd_box_decode(ptr(anchors), ptr(deltas), anchors.shape[0], f32arr(mean), f32arr(std), ptr(out), stream_ptr()), "bd_box_decode")
    return out


def retina_assign_encode(anchors, gt_boxes, num_gt, thr_lo, thr_hi, allow_lq, mean, std, labels, match_idx, offsets, num_fg, ws):
    A = anchors.shape[0]
    N, Gmax = gt_boxes.shape[0], gt_boxes.shape[1]
    check(L().bd_retina_assign_encode(ptr(anchors), A, ptr(gt_boxes), ptr(num_gt), N, Gmax, float(thr_lo), float(thr_hi),
                                      int(allow_lq), f32arr(mean), f32arr(std), ptr(labels), ptr(match_idx), ptr(offsets),
                                      ptr(num_fg), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()), "bd_retina_assign_encode")


def fcos_assign(points, lvl_start, soi, strides, radius, gt_boxes, num_gt, labels, offsets, ctrness, stats):
    P = points.shape[0]
    N, Gmax = gt_boxes.shape[0], gt_boxes.shape[1]
    Ln = len(strides)
    soi_flat = [float(v) for s in soi for v in s]
    check(L().bd_fcos_assign(ptr(points), P, i32arr(lvl_start), f32arr(soi_flat), i32arr(strides), Ln, float(radius),
                             ptr(gt_boxes), ptr(num_gt), N, Gmax, ptr(labels), ptr(offsets), ptr(ctrness), ptr(stats),
                             stream_ptr()), "bd_fcos_assign")


def atss_assign_workspace_bytes(N, P):
    return int(L().bd_atss_assign_workspace_bytes(N, P))


def atss_assign(points, lvl_start, strides, topk, anchor_scale, gt_boxes, num_gt, labels, offsets, ctrness, stats, ws):
    P = points.shape[0]
    N, Gmax = gt_boxes.shape[0], gt_boxes.shape[1]
    check(L().bd_atss_assign(ptr(points), P, i32arr(lvl_start), i32arr(strides), len(strides), int(topk), float(anchor_scale),
                             ptr(gt_boxes), ptr(num_gt), N, Gmax, ptr(labels), ptr(offsets), ptr(ctrness), ptr(stats), ptr(ws),
                             ws.numel() * ws.element_size(), stream_ptr()), "bd_atss_assign")


def ota_assign_workspace_bytes(N, P):
    return int(L().bd_ota_assign_workspace_bytes(N, P))


def ota_assign(points, lvl_start, strides, logits, K, pred_ltrb, gt_boxes, num_gt, alpha, gamma, reg_weight, center_radius,
               candidate_k, labels, targets, gt_ious, stats, ws, ld=None):
    """OTA.get_ground_truth, top-k matcher (models/det/ota.py:76-181).  ld: slots per row of `logits` (round_up(K, 8)); None: compact, K."""
    P = points.shape[0]
    N, Gmax = gt_boxes.shape[0], gt_boxes.shape[1]
    check(L().bd_ota_assign(ptr(points), P, i32arr(lvl_start), i32arr(strides), len(strides), ptr(logits), int(K),
                            int(K if ld is None else ld), ptr(pred_ltrb), ptr(gt_boxes), ptr(num_gt), N, Gmax, float(alpha), float(gamma), float(reg_weight), float(center_radius),
                            int(candidate_k), ptr(labels), ptr(targets), ptr(gt_ious), ptr(stats), ptr(ws),
                            ws.numel() * ws.element_size(), stream_ptr()), "bd_ota_assign")


def ota_sinkhorn_workspace_bytes(N, P, Gmax):
    return int(L().bd_ota_sinkhorn_workspace_bytes(N, P, Gmax))


def ota_assign_sinkhorn(points, lvl_start, strides, logits, K, pred_ltrb, gt_boxes, num_gt, alpha, gamma, reg_weight, center_radius,
                        labels, targets, gt_ious, stats, ws, topq=20, eps=0.1, iters=50, ld=None):
    """OTA.get_ground_truth with the SinkhornMatcher (models/det/ota.py:153-157, layers/common/matcher.py:106-121).  ld: as ota_assign."""
    P = points.shape[0]
    N, Gmax = gt_boxes.shape[0], gt_boxes.shape[1]
    check(L().bd_ota_assign_sinkhorn(ptr(points), P, i32arr(lvl_start), i32arr(strides), len(strides), ptr(logits), int(K),
                                     int(K if ld is None else ld), ptr(pred_ltrb), ptr(gt_boxes), ptr(num_gt), N, Gmax, float(alpha), float(gamma), float(reg_weight),
                                     float(center_radius), int(topq), float(eps), int(iters), ptr(labels), ptr(targets), ptr(gt_ious),
                                     ptr(stats), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()), "bd_ota_assign_sinkhorn")


def freeanchor_workspace_bytes(N, Gmax, bucket, A):
    return int(L().bd_freeanchor_workspace_bytes(N, Gmax, bucket, A))


def freeanchor_loss_fwd_bwd(logits, offsets, box_ld, anchors_per_pix, anchors, K, gt_boxes, num_gt, mean, std, iou_thresh, bucket,
                            beta, reg_weight, alpha, gamma, loss_out, d_logits, d_offsets, ws, cls_ld=None):
    """FreeAnchor bag losses + gradients (models/det/free_anchor.py:38-142); loss_out: fp32[2] = (pos_loss, neg_loss).
    cls_ld: slots per anchor row of logits / d_logits (K or round_up(K, 8)); None: compact, K."""
    A = anchors.shape[0]
    N, Gmax = gt_boxes.shape[0], gt_boxes.shape[1]
    check(L().bd_freeanchor_loss_fwd_bwd(ptr(logits), int(K if cls_ld is None else cls_ld), ptr(offsets), int(box_ld),
                                         int(anchors_per_pix), ptr(anchors), A, int(K), ptr(gt_boxes), ptr(num_gt), N, Gmax, f32arr(mean), f32arr(std), float(iou_thresh),
                                         int(bucket), float(beta), float(reg_weight), float(alpha), float(gamma), ptr(loss_out),
                                         ptr(d_logits), ptr(d_offsets), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()),
          "bd_freeanchor_loss_fwd_bwd")


def nms_workspace_bytes(n):
    return int(L().bd_nms_workspace_bytes(n))


def batched_nms(boxes, scores, idxs, iou_thresh, max_output=None):
    n = boxes.shape[0]
    dev = boxes.device
    keep = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    num = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((nms_workspace_bytes(n),), dtype=torch.uint8, device=dev)
    check(L().bd_batched_nms(ptr(boxes), ptr(scores), ptr(idxs), n, float(iou_thresh), int(max_output or 0), ptr(keep),
                             ptr(num), ptr(ws), ws.numel(), stream_ptr()), "bd_batched_nms")
    return keep[: int(num.item())]


# ---- Faster R-CNN pieces ----------------------------------------------------------------------------------
def rpn_assign_encode(anchors, gt_boxes, num_gt, thr_lo, thr_hi, allow_lq, mean, std, labels, match_idx, offsets, num_fg, ws):
    A = anchors.shape[0]
    N, Gmax = gt_boxes.shape[0], gt_boxes.shape[1]
    check(L().bd_rpn_assign_encode(ptr(anchors), A, ptr(gt_boxes), ptr(num_gt), N, Gmax, float(thr_lo), float(thr_hi),
                                   int(allow_lq), f32arr(mean), f32arr(std), ptr(labels), ptr(match_idx), ptr(offsets),
                                   ptr(num_fg), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()), "bd_rpn_assign_encode")


def sample_labels(labels, keys_pos, keys_neg, num_pos_max, num_total, num_valid):
    N, A = labels.shape
    check(L().bd_sample_labels(ptr(labels), ptr(keys_pos), ptr(keys_neg), N, A, int(num_pos_max), int(num_total), ptr(num_valid),
                               stream_ptr()), "bd_sample_labels")


def segment_topk(scores, B, batch_stride, A, ldc, coff, seg_start, seg_rows, k, out_idx, out_score, out_cnt, min_score=None):
    check(L().bd_segment_topk(ptr(scores), int(scores.dtype == torch.bfloat16), B, batch_stride, A, ldc, coff, len(seg_start),
                              i32arr(seg_start), i32arr(seg_rows), k, float(min_score or 0.0), int(min_score is not None),
                              ptr(out_idx), ptr(out_score), ptr(out_cnt), stream_ptr()), "bd_segment_topk")


def nms_batched_workspace_bytes(B, Cn):
    return int(L().bd_nms_batched_workspace_bytes(B, Cn))


def nms_batched(boxes, scores, idxs, iou_thresh, max_output, keep, num_keep, ws):
    B, Cn = scores.shape
    check(L().bd_nms_batched(ptr(boxes), ptr(scores), ptr(idxs), B, Cn, float(iou_thresh), int(max_output or 0), keep.shape[1],
                             ptr(keep), ptr(num_keep), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()), "bd_nms_batched")


def rpn_proposals_workspace_bytes(N, lvl_pixels, A, pre_k, post_k):
    return int(L().bd_rpn_proposals_workspace_bytes(N, len(lvl_pixels), i32arr(lvl_pixels), A, pre_k, post_k))


def rpn_proposals(raw, ldc, A, cls_off, box_off, geom: Geom, anchors, im_info, mean, std, pre_k, nms_thresh, post_k, rois, num_rois, ws,
                  joint_nms=False):
    """joint_nms: the batched NMS as one problem per image (rounds 1-4) instead of level by level + merge."""
    lvl_pixels = [h * w for h, w in zip(geom.H, geom.W)]
    check(L().bd_rpn_proposals(ptr(raw), ldc, A, cls_off, box_off, geom.N, geom.pix_per_img, geom.nlev, i32arr(geom.off),
                               i32arr(lvl_pixels), ptr(anchors), ptr(im_info), im_info.shape[1], f32arr(mean), f32arr(std),
                               int(pre_k), float(nms_thresh), int(post_k), ptr(rois), ptr(num_rois), ptr(ws),
                               ws.numel() * ws.element_size(), int(bool(joint_nms)), stream_ptr()), "bd_rpn_proposals")


def rcnn_sample_targets(rois, num_rois, gt_boxes, num_gt, keys_fg, keys_bg, num_samples, num_fg_max, fg_thresh, bg_hi, bg_lo,
                        mean, std, out_rois, out_labels, out_targets, out_count, total_count):
    N, post_k = rois.shape[0], rois.shape[1]
    Gmax = gt_boxes.shape[1]
    check(L().bd_rcnn_sample_targets(ptr(rois), ptr(num_rois), post_k, ptr(gt_boxes), ptr(num_gt), N, Gmax, ptr(keys_fg),
                                     ptr(keys_bg), keys_fg.shape[1], int(num_samples), int(num_fg_max), float(fg_thresh),
                                     float(bg_hi), float(bg_lo), f32arr(mean), f32arr(std), ptr(out_rois), ptr(out_labels),
                                     ptr(out_targets), ptr(out_count), ptr(total_count), stream_ptr()), "bd_rcnn_sample_targets")


def conv1x1_thin_fwd(x, w, bias, M, Cin, Cout, y):
    check(L().bd_conv1x1_thin_fwd(ptr(x), ptr(w), ptr(bias), int(M), Cin, Cout, ptr(y), stream_ptr()), "bd_conv1x1_thin_fwd")


def conv1x1_thin_bwd_workspace_bytes():
    return int(L().bd_conv1x1_thin_bwd_workspace_bytes())


def conv1x1_thin_bwd(x, g, w, M, Cin, Cout, dx, dw, dbias, cout_real, ws):
    """Data + weight + bias gradient of a thin 1x1 prediction layer in one pass over its (ReLU-output) input: bd_conv1x1_thin_bwd."""
    check(L().bd_conv1x1_thin_bwd(ptr(x), ptr(g), ptr(w), int(M), Cin, Cout, ptr(dx), ptr(dw), ptr(dbias), cout_real, ptr(ws),
                                  ws.numel() * ws.element_size(), stream_ptr()), "bd_conv1x1_thin_bwd")


def roi_align_fwd(feat, geom: Geom, nlev, strides, Cn, rois, labels, rois_per_img, pool, sample_points, out):
    R = rois.shape[0]
    check(L().bd_roi_align_fwd(ptr(feat), geom.pix_per_img, Cn, nlev, i32arr(geom.off[:nlev]), i32arr(geom.H[:nlev]),
                               i32arr(geom.W[:nlev]), i32arr(strides[:nlev]), ptr(rois), ptr(labels), R, rois_per_img, pool[0],
                               pool[1], sample_points, ptr(out), stream_ptr()), "bd_roi_align_fwd")


def roi_align_bwd(gout, geom: Geom, nlev, strides, Cn, rois, labels, rois_per_img, pool, sample_points, gfeat):
    R = rois.shape[0]
    check(L().bd_roi_align_bwd(ptr(gout), geom.pix_per_img, Cn, nlev, i32arr(geom.off[:nlev]), i32arr(geom.H[:nlev]),
                               i32arr(geom.W[:nlev]), i32arr(strides[:nlev]), ptr(rois), ptr(labels), R, rois_per_img, pool[0],
                               pool[1], sample_points, ptr(gfeat), stream_ptr()), "bd_roi_align_bwd")


def roi_align_bwd_bf16_workspace_bytes(geom: Geom, rois_per_img):
    return int(L().bd_roi_align_bwd_bf16_workspace_bytes(geom.N, geom.nlev, i32arr(geom.H), i32arr(geom.W), rois_per_img))


def roi_align_bwd_bf16(gout, geom: Geom, nlev, strides, Cn, rois, labels, rois_per_img, pool, sample_points, gfeat, ws, accumulate=False):
    check(L().bd_roi_align_bwd_bf16(ptr(gout), geom.pix_per_img, Cn, nlev, geom.nlev, i32arr(geom.off), i32arr(geom.H), i32arr(geom.W),
                                    i32arr(strides[:nlev]), ptr(rois), ptr(labels), geom.N, rois_per_img, pool[0], pool[1], sample_points,
                                    ptr(gfeat), int(bool(accumulate)), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()),
          "bd_roi_align_bwd_bf16")


def roi_pool_fwd(feat, geom: Geom, nlev, strides, Cn, rois, labels, rois_per_img, pool, out):
    """RoI max pooling (ROI_POOLER.METHOD = "roi_pool") of the first nlev levels of a pixel-major bf16 pyramid into out [R][PH*PW][C]."""
    R = rois.shape[0]
    check(L().bd_roi_pool_fwd(ptr(feat), geom.pix_per_img, Cn, nlev, i32arr(geom.off[:nlev]), i32arr(geom.H[:nlev]),
                              i32arr(geom.W[:nlev]), i32arr(strides[:nlev]), ptr(rois), ptr(labels), R, rois_per_img, pool[0],
                              pool[1], ptr(out), stream_ptr()), "bd_roi_pool_fwd")


def roi_pool_bwd_bf16_workspace_bytes(geom: Geom, rois_per_img):
    return int(L().bd_roi_pool_bwd_bf16_workspace_bytes(geom.N, geom.nlev, i32arr(geom.H), i32arr(geom.W), rois_per_img))


def roi_pool_bwd_bf16(feat, gout, geom: Geom, nlev, strides, Cn, rois, labels, rois_per_img, pool, gfeat, ws, accumulate=False):
    """Adjoint of roi_pool_fwd: `feat` is the pyramid the forward read (the argmax is found in it again), gfeat the bf16 gradient pyramid."""
    check(L().bd_roi_pool_bwd_bf16(ptr(feat), ptr(gout), geom.pix_per_img, Cn, nlev, geom.nlev, i32arr(geom.off), i32arr(geom.H),
                                   i32arr(geom.W), i32arr(strides[:nlev]), ptr(rois), ptr(labels), geom.N, rois_per_img, pool[0], pool[1],
                                   ptr(gfeat), int(bool(accumulate)), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()),
          "bd_roi_pool_bwd_bf16")


def subsample2x_fwd(src, gsrc: Geom, dst, gdst: Geom, Cn):
    check(L().bd_subsample2x_fwd(ptr(src), gsrc.pix_per_img, gsrc.off[0], gsrc.H[0], gsrc.W[0], ptr(dst), gdst.pix_per_img,
                                 gdst.off[0], Cn, gsrc.N, stream_ptr()), "bd_subsample2x_fwd")


def subsample2x_bwd_add(g_dst, gdst: Geom, g_src, gsrc: Geom, Cn):
    check(L().bd_subsample2x_bwd_add(ptr(g_dst), gdst.pix_per_img, gdst.off[0], ptr(g_src), gsrc.pix_per_img, gsrc.off[0],
                                     gsrc.H[0], gsrc.W[0], Cn, gsrc.N, stream_ptr()), "bd_subsample2x_bwd_add")


def f32_to_bf16(src, dst, accumulate=False):
    """dst = bf16(src), or bf16(float(dst) + src) with accumulate."""
    if accumulate:
        check(L().bd_f32_to_bf16_add(ptr(src), ptr(dst), src.numel(), stream_ptr()), "bd_f32_to_bf16_add")
    else:
        check(L().bd_f32_to_bf16(ptr(src), ptr(dst), src.numel(), stream_ptr()), "bd_f32_to_bf16")


def rpn_loss_fwd_bwd(raw, ldc, A, cls_off, box_off, labels, targets, rows, beta, num_valid, loss2, draw):
    check(L().bd_rpn_loss_fwd_bwd(ptr(raw), ldc, A, cls_off, box_off, ptr(labels), ptr(targets), rows, float(beta), ptr(num_valid),
                                  ptr(loss2), ptr(draw), stream_ptr()), "bd_rpn_loss_fwd_bwd")


def rcnn_loss_fwd_bwd(raw, ld, K, box_off, labels, targets, R, beta, num_samples, loss2, draw):
    check(L().bd_rcnn_loss_fwd_bwd(ptr(raw), ld, K, box_off, ptr(labels), ptr(targets), R, float(beta), ptr(num_samples),
                                   ptr(loss2), ptr(draw), stream_ptr()), "bd_rcnn_loss_fwd_bwd")


# ---- inference post-processing ----------------------------------------------------------------------------
def det_scores(logits, rows, K, scores, ctr=None, ctr_ld=1, ctr_off=0, ld=None):
    """ld: slots per row of `logits` when they are padded behind the K classes (scores stays [rows][K]); None: compact, K."""
    check(L().bd_det_scores(ptr(logits), int(K if ld is None else ld), ptr(ctr), ctr_ld, ctr_off, rows, K, ptr(scores), stream_ptr()),
          "bd_det_scores")


def rcnn_predict(raw, ld, K, box_off, rois, num_rois, rois_per_img, mean, std, scores, boxes):
    R = raw.shape[0]
    check(L().bd_rcnn_predict(ptr(raw), ld, K, box_off, ptr(rois), ptr(num_rois), rois_per_img, R, f32arr(mean), f32arr(std),
                              ptr(scores), ptr(boxes), stream_ptr()), "bd_rcnn_predict")


def det_candidates(mode, topk_idx, topk_score, topk_cnt, B, Ln, k, lvl_row_off, K, anchors, offsets, off_stride, off_ld, A, mean, std,
                   item_boxes, item_stride, boxes, scores, labels):
    """B images in one launch (one image: B = 1); off_stride / item_stride: bf16 elements / boxes between the offsets / item_boxes of two images."""
    check(L().bd_det_candidates(mode, ptr(topk_idx), ptr(topk_score), ptr(topk_cnt), B, Ln, k, i32arr(lvl_row_off), K, ptr(anchors),
                                ptr(offsets), off_stride, off_ld, A, f32arr(mean), f32arr(std), ptr(item_boxes), item_stride,
                                ptr(boxes), ptr(scores), ptr(labels), stream_ptr()), "bd_det_candidates")


def det_finalize(boxes, scores, labels, keep, num_keep, max_out, im_info, out_boxes, out_scores, out_labels):
    """scores [B][C], im_info [B][>= 4] (or the one row of B = 1): every image is rescaled and clipped by its own row."""
    B, Cn = scores.shape
    check(L().bd_det_finalize(ptr(boxes), ptr(scores), ptr(labels), ptr(keep), ptr(num_keep), B, Cn, max_out, ptr(im_info),
                              im_info.shape[-1], ptr(out_boxes), ptr(out_scores), ptr(out_labels), stream_ptr()), "bd_det_finalize")


def det_select_workspace_bytes(B, Ln, rows, K, k):
    return int(L().bd_det_select_workspace_bytes(B, Ln, rows, K, k))


def det_select(logits, B, rows, K, seg_start, seg_rows, k, min_score, out_idx, out_score, out_cnt, ws, ctr=None, ctr_ld=1, ctr_off=0,
               ld=None):
    """Scores + per-level top-k of B images straight from the bf16 logits [B][rows][K] (= det_scores -> segment_topk(min_score), bit for
    bit); seg_start / seg_rows in rows.  ld: slots per row of `logits` (round_up(K, 8)) when they are padded: same indices, scores, counts;
    None: compact, K."""
    check(L().bd_det_select(ptr(logits), int(K if ld is None else ld), ptr(ctr), ctr_ld, ctr_off, B, rows, K, len(seg_start),
                            i32arr(seg_start), i32arr(seg_rows), k, float(min_score), ptr(out_idx), ptr(out_score), ptr(out_cnt), ptr(ws),
                            ws.numel() * ws.element_size(), stream_ptr()), "bd_det_select")


# ---- losses -----------------------------------------------------------------------------------------------
def focal_loss_fwd_bwd(logits, labels, rows, K, alpha, gamma, norm, grad_scale, loss_sum, dlogits, general=False, ld=None):
    """general: the general-gamma kernel also for gamma == 2
    ld: slots per row of logits / dlogits (round_up(K, 8)) for a K that is no multiple of 8; None: compact, K"""
    check(L().bd_focal_loss_fwd_bwd(ptr(logits), ptr(labels), rows, K, int(K if ld is None else ld), float(alpha), float(gamma), ptr(norm),
                                    int(norm.dtype == torch.float32), float(grad_scale), ptr(loss_sum), ptr(dlogits), int(bool(general)),
                                    stream_ptr()), "bd_focal_loss_fwd_bwd")


def smooth_l1_fwd_bwd(pred, target, labels, pixels, A, ld, beta, norm, weight, loss_sum, dpred):
    check(L().bd_smooth_l1_fwd_bwd(ptr(pred), ptr(target), ptr(labels), pixels, A, ld, float(beta), ptr(norm),
                                   int(norm.dtype == torch.float32), float(weight), ptr(loss_sum), ptr(dpred), stream_ptr()),
          "bd_smooth_l1_fwd_bwd")


def loss_grid_cap():
    """Blocks of 256 threads the loss launches run at most; past 256 x this many rows a thread walks more than one."""
    return int(L().bd_loss_grid_cap())


IOU_LOSS_TYPES = {"iou": 0, "linear_iou": 1, "giou": 2, "square_iou": 3}     # iou_loss's loss_type (layers/losses/iou_loss.py:78)


def iou_ltrb_fwd_bwd(pred, target, weight, labels, rows, loss_type, norm, loss_weight, loss_sum, dpred):
    """loss_type: a code of IOU_LOSS_TYPES."""
    check(L().bd_iou_ltrb_fwd_bwd(ptr(pred), ptr(target), ptr(weight), ptr(labels), rows, int(loss_type), ptr(norm), float(loss_weight),
                                  ptr(loss_sum), ptr(dpred), stream_ptr()), "bd_iou_ltrb_fwd_bwd")


def bce_logits_fwd_bwd(pred, target, labels, rows, norm, loss_sum, dpred, ld=1, off=0):
    check(L().bd_bce_logits_fwd_bwd(ptr(pred), ld, off, ptr(target), ptr(labels), rows, ptr(norm), ptr(loss_sum), ptr(dpred),
                                    stream_ptr()), "bd_bce_logits_fwd_bwd")


# ---- FCOS head pieces -------------------------------------------------------------------------------------
def groupnorm_workspace_bytes(N, Ln, Cn, pix_per_img):
    return int(L().bd_groupnorm_workspace_bytes(N, Ln, Cn, int(pix_per_img)))


def _lvl_arrays(geom: Geom):
    return i32arr(geom.off), i32arr([h * w for h, w in zip(geom.H, geom.W)])


def groupnorm_fwd(y, gamma, beta, geom: Geom, Cn, eps, relu, stats, z, ws):
    off, cnt = _lvl_arrays(geom)
    check(L().bd_groupnorm_fwd(ptr(y), ptr(gamma), ptr(beta), geom.N, geom.nlev, off, cnt, geom.pix_per_img, Cn, float(eps),
                               int(relu), ptr(stats), ptr(z), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()), "bd_groupnorm_fwd")
    return z


def conv2d_fwd_gnstats_bytes(d):
    return int(L().bd_conv2d_fwd_gnstats_bytes(C.byref(d)))


def conv2d_fwd_gnstats(d, x, w_packed, bias, y, part):
    """3x3 / stride-1 convolution into 256 channels that also leaves GroupNorm's per-patch statistics in `part` (fp32, conv2d_fwd_gnstats_bytes)."""
    check(L().bd_conv2d_fwd_gnstats(C.byref(_stamp(d)), ptr(x), ptr(w_packed), ptr(bias), ptr(y), ptr(part), part.numel() * part.element_size(),
                                    stream_ptr()), "bd_conv2d_fwd_gnstats")
    return y


def groupnorm_fwd_parts(d, y, part, gamma, beta, eps, relu, stats, z):
    """GroupNorm(32, 256) (+ReLU) from the statistics conv2d_fwd_gnstats left: stats (mean, rstd) [N][L][32][2] out, z out."""
    check(L().bd_groupnorm_fwd_parts(C.byref(d), ptr(y), ptr(part), ptr(gamma), ptr(beta), float(eps), int(relu), ptr(stats), ptr(z), stream_ptr()),
          "bd_groupnorm_fwd_parts")
    return z


def groupnorm_bwd(dz, y, gamma, beta, stats, geom: Geom, Cn, relu, dy, dgamma, dbeta, ws, accumulate=False):
    """The ReLU gate (relu=True) is recomputed from y, stats, gamma, beta: the forward's output z is not an operand."""
    off, cnt = _lvl_arrays(geom)
    check(L().bd_groupnorm_bwd(ptr(dz), ptr(y), ptr(gamma), ptr(beta), ptr(stats), geom.N, geom.nlev, off, cnt, geom.pix_per_img, Cn,
                               int(relu), ptr(dy), ptr(dgamma), ptr(dbeta), int(accumulate), ptr(ws), ws.numel() * ws.element_size(),
                               stream_ptr()), "bd_groupnorm_bwd")
    return dy


# ---- BatchNorm of one pyramid level (csrc/batchnorm.hip) ------------------------------------------------------------------
def _lvl(geom: Geom):
    assert geom.nlev == 1
    return geom.pix_per_img, geom.off[0]


def bn_workspace_bytes(rows, Cn):
    return int(L().bd_bn_workspace_bytes(int(rows), Cn))


def bn_stats_fwd(y, geom: Geom, Cn, eps, momentum, mean, inv_std, sums, running_mean, running_var, ws):
    """Batch statistics of one level of y: mean, inv_std, sums = [M, sum y, sum y^2] (3, C), and the running statistics updated in place
    (None: left alone)."""
    check(L().bd_bn_stats_fwd(ptr(y), geom.N, *_lvl(geom), geom.H[0] * geom.W[0], Cn, eps, momentum, ptr(mean), ptr(inv_std), ptr(sums),
                              ptr(running_mean), ptr(running_var), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()), "bd_bn_stats_fwd")


def bn_apply_act_fwd(y, gy: Geom, mean, inv_std, gamma, beta, z, gz: Geom, Cn, residual=None, gr: Geom = None, relu=True):
    """z = [relu](gamma * (y - mean) * inv_std + beta [+ residual]) in one pass: the epilogue of every normalised convolution (the
    backbone's under MODEL.BACKBONE.NORM; the FPN's without residual and ReLU, z then possibly a level of the pyramid)."""
    rl = _lvl(gr if gr is not None else gz) if residual is not None else (0, 0)
    check(L().bd_bn_apply_act_fwd(ptr(y), *_lvl(gy), ptr(mean), ptr(inv_std), ptr(gamma), ptr(beta), ptr(residual), *rl, ptr(z), *_lvl(gz),
                                  gy.N, gy.H[0] * gy.W[0], Cn, int(bool(relu)), stream_ptr()), "bd_bn_apply_act_fwd")
    return z


def bn_bwd_reduce(g, gg: Geom, y, gy: Geom, mean, inv_std, Cn, dgamma, dbeta, ws):
    check(L().bd_bn_bwd_reduce(ptr(g), *_lvl(gg), ptr(y), *_lvl(gy), ptr(mean), ptr(inv_std), gy.N, gy.H[0] * gy.W[0], Cn, ptr(dgamma),
                               ptr(dbeta), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()), "bd_bn_bwd_reduce")


def bn_bwd_apply(g, gg: Geom, y, gy: Geom, mean, inv_std, gamma, dgamma, dbeta, count, out, go: Geom, Cn):
    check(L().bd_bn_bwd_apply(ptr(g), *_lvl(gg), ptr(y), *_lvl(gy), ptr(mean), ptr(inv_std), ptr(gamma), ptr(dgamma), ptr(dbeta), ptr(count),
                              ptr(out), *_lvl(go), gy.N, gy.H[0] * gy.W[0], Cn, stream_ptr()), "bd_bn_bwd_apply")
    return out


def bn_silu_fwd(y, gy: Geom, mean, inv_std, gamma, beta, z, gz: Geom, Cn):
    """z = silu(gamma * (y - mean) * inv_std + beta) in one pass: the epilogue of every YOLOX convolution (eval(): mean / inv_std are
    running_mean and 1 / sqrt(running_var + eps))."""
    check(L().bd_bn_silu_fwd(ptr(y), *_lvl(gy), ptr(mean), ptr(inv_std), ptr(gamma), ptr(beta), ptr(z), *_lvl(gz), gy.N, gy.H[0] * gy.W[0],
                             Cn, stream_ptr()), "bd_bn_silu_fwd")
    return z


def bn_silu_bwd_reduce(g, gg: Geom, y, gy: Geom, mean, inv_std, gamma, beta, Cn, dgamma, dbeta, ws):
    """dgamma / dbeta of conv -> BN -> SiLU from the gradient of the SiLU OUTPUT: the gate is recomputed from the pre-norm y."""
    check(L().bd_bn_silu_bwd_reduce(ptr(g), *_lvl(gg), ptr(y), *_lvl(gy), ptr(mean), ptr(inv_std), ptr(gamma), ptr(beta), gy.N,
                                    gy.H[0] * gy.W[0], Cn, ptr(dgamma), ptr(dbeta), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()),
          "bd_bn_silu_bwd_reduce")


def bn_silu_bwd_apply(g, gg: Geom, y, gy: Geom, mean, inv_std, gamma, beta, dgamma, dbeta, count, out, go: Geom, Cn):
    check(L().bd_bn_silu_bwd_apply(ptr(g), *_lvl(gg), ptr(y), *_lvl(gy), ptr(mean), ptr(inv_std), ptr(gamma), ptr(beta), ptr(dgamma),
                                   ptr(dbeta), ptr(count), ptr(out), *_lvl(go), gy.N, gy.H[0] * gy.W[0], Cn, stream_ptr()),
          "bd_bn_silu_bwd_apply")
    return out


def fcos_offsets_fwd(raw, ld, scales, geom: Geom, strides, out):
    off, cnt = _lvl_arrays(geom)
    check(L().bd_fcos_offsets_fwd(ptr(raw), ld, ptr(scales), geom.N, geom.nlev, off, cnt, i32arr(strides), geom.pix_per_img, ptr(out),
                                  stream_ptr()), "bd_fcos_offsets_fwd")
    return out


def fcos_offsets_workspace_bytes():
    return int(L().bd_fcos_offsets_workspace_bytes())


def fcos_offsets_bwd(raw, ld, scales, geom: Geom, strides, d_off, d_ctr, d_raw, dscale, ws):
    off, cnt = _lvl_arrays(geom)
    check(L().bd_fcos_offsets_bwd(ptr(raw), ld, ptr(scales), geom.N, geom.nlev, off, cnt, i32arr(strides), geom.pix_per_img, ptr(d_off),
                                  ptr(d_ctr), ptr(d_raw), ptr(dscale), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()),
          "bd_fcos_offsets_bwd")


def sgd_momentum_step(w, v, g, lr, momentum, wd, grad_scale=1.0):
    check(L().bd_sgd_momentum_step(ptr(w), ptr(v), ptr(g), w.numel(), float(lr), float(momentum), float(wd),
                                   float(grad_scale), stream_ptr()), "bd_sgd_momentum_step")


def ema_coeffs(m):
    """(m, 1 - m) as the reference hands them to its kernels (ema.py:80: `mge.tensor(m)`, `mge.tensor(1 - m)`): the difference is taken
    in Python float64, the cast to fp32 happens at the C boundary."""
    return float(m), float(1 - m)


def _same_f32(*ts):
    assert all(t.dtype == torch.float32 and t.numel() == ts[0].numel() for t in ts), "fp32 buffers of one length expected"


def ema_update(e, w, m):
    _same_f32(e, w)
    mm, om = ema_coeffs(m)
    check(L().bd_ema_update(ptr(e), ptr(w), e.numel(), mm, om, stream_ptr()), "bd_ema_update")


def sgd_momentum_ema_step(w, v, g, e, lr, momentum, wd, grad_scale, m):
    _same_f32(w, v, g, e)
    mm, om = ema_coeffs(m)
    check(L().bd_sgd_momentum_ema_step(ptr(w), ptr(v), ptr(g), ptr(e), w.numel(), float(lr), float(momentum), float(wd),
                                       float(grad_scale), mm, om, stream_ptr()), "bd_sgd_momentum_ema_step")


def swap_f32(a, b):
    _same_f32(a, b)
    check(L().bd_swap_f32(ptr(a), ptr(b), a.numel(), stream_ptr()), "bd_swap_f32")


def adam_coeffs(betas, step):
    """(beta1, 1 - beta1, beta2, 1 - beta2, 1 - beta1**step, 1 - beta2**step): the differences and the bias corrections of step `step`
    (counted from 1) are taken in Python float64, the cast to fp32 happens at the C boundary -- the way `ema_coeffs` hands 1 - m over."""
    b1, b2 = float(betas[0]), float(betas[1])
    return b1, 1 - b1, b2, 1 - b2, 1 - b1 ** step, 1 - b2 ** step


def adam_step(w, m, v, g, lr, betas, eps, wd, step, grad_scale=1.0, decoupled=False):
    """megengine.optimizer.Adam (`decoupled` False: wd * w joins the gradient) / AdamW (True: it joins the update) over fp32 buffers of one
    length in one launch (bd_adam_step); `m`, `v`: the first and second moments, `step`: this update's number, from 1."""
    _same_f32(w, m, v, g)
    check(L().bd_adam_step(ptr(w), ptr(m), ptr(v), ptr(g), w.numel(), float(lr), *adam_coeffs(betas, step), float(eps), float(wd),
                           float(grad_scale), int(bool(decoupled)), stream_ptr()), "bd_adam_step")


def adam_ema_step(w, m, v, g, e, lr, betas, eps, wd, step, grad_scale, decoupled, ema_m):
    """`adam_step`, then `ema_update(e, w, ema_m)` with the new weights, in the same launch (bd_adam_ema_step)."""
    _same_f32(w, m, v, g, e)
    mm, om = ema_coeffs(ema_m)
    check(L().bd_adam_ema_step(ptr(w), ptr(m), ptr(v), ptr(g), ptr(e), w.numel(), float(lr), *adam_coeffs(betas, step), float(eps),
                               float(wd), float(grad_scale), int(bool(decoupled)), mm, om, stream_ptr()), "bd_adam_ema_step")


def sgd_nesterov_step(w, v, g, lr, momentum, wd, grad_scale=1.0):
    """megengine.optimizer.SGD(nesterov=True): g' = g*grad_scale + wd*w; v = momentum*v + g'; w -= lr*(g' + momentum*v)
    (bd_sgd_nesterov_step)."""
    _same_f32(w, v, g)
    check(L().bd_sgd_nesterov_step(ptr(w), ptr(v), ptr(g), w.numel(), float(lr), float(momentum), float(wd), float(grad_scale),
                                   stream_ptr()), "bd_sgd_nesterov_step")


def sgd_nesterov_ema_step(w, v, g, e, lr, momentum, wd, grad_scale, m):
    """`sgd_nesterov_step`, then `ema_update(e, w, m)` with the new weights, in the same launch (bd_sgd_nesterov_ema_step)."""
    _same_f32(w, v, g, e)
    mm, om = ema_coeffs(m)
    check(L().bd_sgd_nesterov_ema_step(ptr(w), ptr(v), ptr(g), ptr(e), w.numel(), float(lr), float(momentum), float(wd),
                                       float(grad_scale), mm, om, stream_ptr()), "bd_sgd_nesterov_ema_step")


class WgradQueue:
    """bd_wgrad_queue_*: weight-gradient launches whose reduces are deferred to ONE launch per flush (the solver's gradient buckets).
    Every queued layer must keep its own workspace untouched until `flush`."""

    def __init__(self):
        self._h = C.c_void_p()
        check(L().bd_wgrad_queue_create(C.byref(self._h)), "bd_wgrad_queue_create")

    def wgrad(self, d, x, g, dw, dbias, ws, row_scale=None, accumulate=False):
        check(L().bd_conv2d_wgrad_queued(self._h, C.byref(_stamp(d)), ptr(x), ptr(g), ptr(row_scale), ptr(dw), ptr(dbias), int(accumulate), ptr(ws),
                                         ws.numel() * ws.element_size(), stream_ptr()), "bd_conv2d_wgrad_queued")

    def pending(self):
        return int(L().bd_wgrad_queue_pending(self._h))

    def flush(self):
        check(L().bd_wgrad_queue_flush(self._h, stream_ptr()), "bd_wgrad_queue_flush")

    def close(self):
        if self._h:
            L().bd_wgrad_queue_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:            # noqa: BLE001 (interpreter shutdown)
            pass


def clip_grad_value(g, lower, upper, pre_scale=1.0):
    """megengine.optimizer.clip_grad_value over the flat gradient arena, in place (engine/trainer.py:57-61)."""
    check(L().bd_clip_grad_value(ptr(g), g.numel(), float(pre_scale), float(lower), float(upper), stream_ptr()), "bd_clip_grad_value")


def clip_grad_norm_workspace_bytes():
    return int(L().bd_clip_grad_norm_workspace_bytes())


def clip_grad_norm(g, max_norm, ord=2.0, pre_scale=1.0, norm_out=None, ws=None):
    """megengine.optimizer.clip_grad_norm over the flat gradient arena, in place; the norm (of pre_scale * g) goes to norm_out[0]."""
    if ws is None:
        ws = torch.empty((clip_grad_norm_workspace_bytes(),), dtype=torch.uint8, device=g.device)
    check(L().bd_clip_grad_norm(ptr(g), g.numel(), float(pre_scale), float(max_norm), float(ord), ptr(norm_out), ptr(ws), ws.numel(),
                                stream_ptr()), "bd_clip_grad_norm")
    return norm_out


class HostStager:
    """bd_h2d_*: host batch (numpy float64 / float32 / uint8, C-contiguous) -> fp32 device tensor through the library's pinned staging
    buffer, converted by its worker threads and sent chunk by chunk (data_to_input's `Tensor(image)`, pre_processing.py:13)."""

    _DT = {"float64": 0, "float32": 1, "uint8": 2}

    def __init__(self, device, threads=0):
        self._h = C.c_void_p()
        self.device = torch.device(device)
        # torch.device("cuda") carries no index: the rank's CURRENT device is meant (one process per GPU), never device 0
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", index)
        check(L().bd_h2d_create(C.byref(self._h), int(index), int(threads)), "bd_h2d_create")
        self.threads = int(L().bd_h2d_threads(self._h))

    def supports(self, arr):
        return hasattr(arr, "dtype") and str(arr.dtype) in self._DT and getattr(arr, "flags", None) is not None and arr.flags["C_CONTIGUOUS"]

    def submit(self, arr, out=None, chunk_elems=0):
        """arr: numpy array; returns the fp32 device tensor of the same shape (valid in the current stream's order)."""
        if out is None:
            out = torch.empty(arr.shape, dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.numel() == arr.size and out.dtype == torch.float32
        check(L().bd_h2d_submit(self._h, C.c_void_p(arr.ctypes.data), self._DT[str(arr.dtype)], arr.size, ptr(out), int(chunk_elems),
                                stream_ptr()), "bd_h2d_submit")
        return out

    def close(self):
        if self._h:
            L().bd_h2d_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:            # noqa: BLE001 (interpreter shutdown)
            pass


def bottleneck_fwd_supported(N, H, W, cin, cmid, cout, has_ds):
    return bool(L().bd_bottleneck_fwd_supported(int(N), int(H), int(W), int(cin), int(cmid), int(cout), int(bool(has_ds))))


def bottleneck_fwd(N, H, W, cin, cmid, cout, x, w1, b1, w2, b2, w3, b3, wd, bd, y):
    """A frozen Bottleneck block (models/cls/resnet.py:70-113) in one launch: bd_bottleneck_fwd."""
    check(L().bd_bottleneck_fwd(int(N), int(H), int(W), int(cin), int(cmid), int(cout), ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                                ptr(w3), ptr(b3), ptr(wd), ptr(bd), ptr(y), stream_ptr()), "bd_bottleneck_fwd")
    return y


# ---- CenterNet after the last convolution (centernet.hip) -------------------------------------------------------------------------------
def centernet_targets(gt_boxes, num_gt, K, H, W, T, box_scale, min_overlap):
    """bd_centernet_targets: gt_boxes fp32 (N, Gmax, 5), num_gt int32 (N,) -> dict of score_map fp32 (N, H*W, K) (pixel-major), wh / reg
    (N, T, 2), reg_mask (N, T), index int32 (N, T), num_pos fp32 (1,)."""
    N, G = int(gt_boxes.shape[0]), int(gt_boxes.shape[1])
    dev = gt_boxes.device
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    out = dict(score_map=f(N, H * W, K), wh=f(N, T, 2), reg=f(N, T, 2), reg_mask=f(N, T),
               index=torch.empty((N, T), dtype=torch.int32, device=dev), num_pos=f(1))
    ws = torch.empty(int(L().bd_centernet_targets_workspace_bytes(N)), dtype=torch.uint8, device=dev)
    centernet_targets_into(gt_boxes, num_gt, N, G, K, H, W, T, box_scale, min_overlap, out["score_map"], out["wh"], out["reg"],
                           out["reg_mask"], out["index"], out["num_pos"], ws)
    return out


def centernet_targets_workspace_bytes(N):
    return int(L().bd_centernet_targets_workspace_bytes(N))


def centernet_targets_into(gt_boxes, num_gt, N, G, K, H, W, T, box_scale, min_overlap, score_map, wh, reg, reg_mask, index, num_pos, ws):
    check(L().bd_centernet_targets(ptr(gt_boxes), ptr(num_gt), N, G, K, H, W, T, float(box_scale), float(min_overlap), ptr(score_map),
                                   ptr(wh), ptr(reg), ptr(reg_mask), ptr(index), ptr(num_pos), ptr(ws), ws.numel() * ws.element_size(),
                                   stream_ptr()), "bd_centernet_targets")


def centernet_focal_fwd_bwd(logits, score_map, rows, K, ld, norm, weight, grad_scale, loss_sum, dlogits):
    """logits / dlogits bf16 [rows][ld], score_map fp32 [rows][K], norm = the device num_pos; loss_sum[0] += weight * loss."""
    check(L().bd_centernet_focal_fwd_bwd(ptr(logits), ptr(score_map), rows, K, ld, ptr(norm), float(weight), float(grad_scale),
                                         ptr(loss_sum), ptr(dlogits), stream_ptr()), "bd_centernet_focal_fwd_bwd")


def centernet_l1_fwd_bwd(pred, ld, off, index, reg_mask, target, N, H, W, T, weight, grad_scale, loss_sum, dpred):
    """pred / dpred bf16 [N*H*W][ld], the two channels at column off; loss_sum[0] += weight * loss; dpred is written completely."""
    check(L().bd_centernet_l1_fwd_bwd(ptr(pred), ld, off, ptr(index), ptr(reg_mask), ptr(target), N, H, W, T, float(weight),
                                      float(grad_scale), ptr(loss_sum), ptr(dpred), stream_ptr()), "bd_centernet_l1_fwd_bwd")


def centernet_decode_workspace_bytes(B, K, H, W):
    return int(L().bd_centernet_decode_workspace_bytes(B, K, H, W))


def centernet_decode(logits, ld, wh, wh_ld, wh_off, reg, reg_ld, reg_off, B, K, H, W, k, boxes, scores, classes, ws):
    """reg may be None (+0.5).  boxes fp32 [B][k][4], scores fp32 [B][k], classes int32 [B][k]."""
    check(L().bd_centernet_decode(ptr(logits), ld, ptr(wh), wh_ld, wh_off, ptr(reg), reg_ld, reg_off, B, K, H, W, k, ptr(boxes),
                                  ptr(scores), ptr(classes), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()),
          "bd_centernet_decode")


def centernet_boxes_to_image(boxes, affine, scores, classes, B, k, boxes_out, scores_out, labels_out):
    """bd_centernet_boxes_to_image: boxes fp32 [B][k][4] through the per-image 2 x 3 maps affine fp32 [B][6] into boxes_out; scores and
    classes pass through into scores_out / labels_out."""
    check(L().bd_centernet_boxes_to_image(ptr(boxes), ptr(affine), ptr(scores), ptr(classes), int(B), int(k), ptr(boxes_out),
                                          ptr(scores_out), ptr(labels_out), stream_ptr()), "bd_centernet_boxes_to_image")


# ---- CenterHead's output convolutions (center_head.hip) -----------------------------------------------------------------------------------
def center_head_out_fwd(feat, w_cls, b_cls, w_wh, b_wh, w_reg, b_reg, M, C, K, logits, wr):
    """feat bf16 [M][3C] (cls | wh | reg tower) -> logits bf16 [M][round_up(K, 8)] and wr bf16 [M][8] (wh at 0-1, reg at 2-3); weights the
    fp32 masters [K][C] / [2][C] / [2][C], biases fp32 or None (include/basedet_hip.h, bd_center_head_out_fwd)."""
    check(L().bd_center_head_out_fwd(ptr(feat), ptr(w_cls), ptr(b_cls), ptr(w_wh), ptr(b_wh), ptr(w_reg), ptr(b_reg), int(M), C, K,
                                     logits.shape[-1], ptr(logits), ptr(wr), stream_ptr()), "bd_center_head_out_fwd")
    return logits, wr


def center_head_out_bwd_workspace_bytes(M, C, K):
    return int(L().bd_center_head_out_bwd_workspace_bytes(int(M), C, K))


def center_head_out_bwd(feat, d_logits, d_wr, w_cls, w_wh, w_reg, M, C, K, d_feat, dw_cls, db_cls, dw_wh, db_wh, dw_reg, db_reg, ws,
                        accumulate=False):
    """d_feat bf16 [M][3C] (gated by feat > 0) and the fp32 parameter gradients (+)= in the masters' layout, in one pass (reproducible)."""
    check(L().bd_center_head_out_bwd(ptr(feat), ptr(d_logits), ptr(d_wr), ptr(w_cls), ptr(w_wh), ptr(w_reg), int(M), C, K,
                                     d_logits.shape[-1], ptr(d_feat), ptr(dw_cls), ptr(db_cls), ptr(dw_wh), ptr(db_wh), ptr(dw_reg),
                                     ptr(db_reg), int(accumulate), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()),
          "bd_center_head_out_bwd")
    return d_feat


# ---- YOLOX behind the head's last convolutions (yolox.hip) -----------------------------------------------------------------------------------
def yolox_assign_workspace_bytes(N, P):
    return int(L().bd_yolox_assign_workspace_bytes(N, P))


def yolox_loss_workspace_bytes():
    return int(L().bd_yolox_loss_workspace_bytes())


def _yolox_dims(cls, box_obj, points, gt_boxes):
    P, (N, Gmax) = int(points.shape[0]), (int(gt_boxes.shape[0]), int(gt_boxes.shape[1]))
    if cls.dim() != 2 or box_obj.dim() != 2 or cls.shape[0] != N * P or tuple(box_obj.shape) != (N * P, 8):
        raise ValueError(f"yolox: cls must be (N*P, ld) and box_obj (N*P, 8) with N*P = {N * P}; got {tuple(cls.shape)}, {tuple(box_obj.shape)}")
    return N, P, Gmax


def yolox_assign_into(cls, K, box_obj, points, lvl_start, strides, gt_boxes, num_gt, matched, iou_t, stats, ws):
    """bd_yolox_assign: cls bf16 (N*P, round_up(K, 8)), box_obj bf16 (N*P, 8), points fp32 (P, 2), gt_boxes fp32 (N, Gmax, 5), num_gt int32
    (N,) -> matched int32 (N, P) (gt index, -1 = background), iou_t fp32 (N, P), stats[0] = the foreground count."""
    N, P, Gmax = _yolox_dims(cls, box_obj, points, gt_boxes)
    check(L().bd_yolox_assign(ptr(points), P, i32arr(lvl_start), i32arr(strides), len(strides), ptr(cls), int(K), int(cls.shape[1]),
                              ptr(box_obj), ptr(gt_boxes), ptr(num_gt), N, Gmax, ptr(matched), ptr(iou_t), ptr(stats), ptr(ws),
                              ws.numel() * ws.element_size(), stream_ptr()), "bd_yolox_assign")


def yolox_assign(cls, K, box_obj, points, lvl_start, strides, gt_boxes, num_gt):
    """yolox_assign_into with its outputs and workspace allocated here: (matched, iou_t, stats)."""
    N, P, _ = _yolox_dims(cls, box_obj, points, gt_boxes)
    dev = cls.device
    matched = torch.empty((N, P), dtype=torch.int32, device=dev)
    iou_t = torch.empty((N, P), dtype=torch.float32, device=dev)
    stats = torch.zeros(1, dtype=torch.float32, device=dev)
    ws = torch.empty(yolox_assign_workspace_bytes(N, P), dtype=torch.uint8, device=dev)
    yolox_assign_into(cls, K, box_obj, points, lvl_start, strides, gt_boxes, num_gt, matched, iou_t, stats, ws)
    return matched, iou_t, stats


def yolox_loss_fwd_bwd_into(cls, K, box_obj, points, lvl_start, strides, gt_boxes, matched, iou_t, stats, use_l1, grad_scale, loss_out,
                            d_cls, d_box_obj, ws):
    """bd_yolox_loss_fwd_bwd: loss_out fp32 (4,) = (5 * iou, obj, cls, l1) and the gradients of their sum times grad_scale, d_cls /
    d_box_obj bf16 in the input layouts (written completely)."""
    N, P, Gmax = _yolox_dims(cls, box_obj, points, gt_boxes)
    check(L().bd_yolox_loss_fwd_bwd(ptr(points), P, i32arr(lvl_start), i32arr(strides), len(strides), ptr(cls), int(K), int(cls.shape[1]),
                                    ptr(box_obj), ptr(gt_boxes), N, Gmax, ptr(matched), ptr(iou_t), ptr(stats), int(bool(use_l1)),
                                    float(grad_scale), ptr(loss_out), ptr(d_cls), ptr(d_box_obj), ptr(ws),
                                    ws.numel() * ws.element_size(), stream_ptr()), "bd_yolox_loss_fwd_bwd")


def yolox_loss_fwd_bwd(cls, K, box_obj, points, lvl_start, strides, gt_boxes, matched, iou_t, stats, use_l1=False, grad_scale=1.0):
    """yolox_loss_fwd_bwd_into with its outputs and workspace allocated here: (loss_out, d_cls, d_box_obj)."""
    dev = cls.device
    loss_out = torch.empty(4, dtype=torch.float32, device=dev)
    d_cls, d_box_obj = torch.empty_like(cls), torch.empty_like(box_obj)
    ws = torch.empty(yolox_loss_workspace_bytes(), dtype=torch.uint8, device=dev)
    yolox_loss_fwd_bwd_into(cls, K, box_obj, points, lvl_start, strides, gt_boxes, matched, iou_t, stats, use_l1, grad_scale, loss_out,
                            d_cls, d_box_obj, ws)
    return loss_out, d_cls, d_box_obj


def yolox_candidates_into(topk_idx, topk_score, topk_cnt, K, points, lvl_start, strides, box_obj, boxes, scores, labels):
    """bd_yolox_candidates: the (B, L, k) output of det_select -> boxes fp32 (B, L*k, 4), scores (B, L*k), labels int32 (B, L*k)."""
    B, Ln, k = (int(s) for s in topk_idx.shape)
    check(L().bd_yolox_candidates(ptr(topk_idx), ptr(topk_score), ptr(topk_cnt), B, Ln, k, i32arr(lvl_start), i32arr(strides), int(K),
                                  ptr(points), int(points.shape[0]), ptr(box_obj), ptr(boxes), ptr(scores), ptr(labels), stream_ptr()),
          "bd_yolox_candidates")


def yolox_candidates(topk_idx, topk_score, topk_cnt, K, points, lvl_start, strides, box_obj):
    """yolox_candidates_into with its outputs allocated here: (boxes, scores, labels)."""
    B, Ln, k = (int(s) for s in topk_idx.shape)
    dev = topk_idx.device
    boxes = torch.empty((B, Ln * k, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((B, Ln * k), dtype=torch.float32, device=dev)
    labels = torch.empty((B, Ln * k), dtype=torch.int32, device=dev)
    yolox_candidates_into(topk_idx, topk_score, topk_cnt, K, points, lvl_start, strides, box_obj, boxes, scores, labels)
    return boxes, scores, labels


# ---- CSPDarknet / YOLOPAFPN glue (yolox_neck.hip) -------------------------------------------------------------------------------------------
def spp_fwd(x, N, H, W, Cn, cat):
    """x bf16 (N*H*W, Cn) -> cat bf16 (N*H*W, 4 Cn) = (x, maxpool5, maxpool9, maxpool13), stride 1; H * W <= 4096."""
    check(L().bd_spp_fwd(ptr(x), N, H, W, Cn, ptr(cat), stream_ptr()), "bd_spp_fwd")
    return cat


def spp_bwd(g_cat, x, N, H, W, Cn, d_x):
    """Adjoint of spp_fwd (first-maximum rule, fixed fp32 summation order, no atomics): d_x bf16 (N*H*W, Cn)."""
    check(L().bd_spp_bwd(ptr(g_cat), ptr(x), N, H, W, Cn, ptr(d_x), stream_ptr()), "bd_spp_bwd")
    return d_x


def cat2_fwd(a, b, M, Ca, Cb, out, up=False, N=0, H=0, W=0):
    """out bf16 (M, Ca + Cb) = (a, b); up: a is (N*(H/2)*(W/2), Ca), read through a nearest 2x upsample (M = N*H*W)."""
    check(L().bd_cat2_fwd(ptr(a), ptr(b), M, Ca, Cb, int(bool(up)), N, H, W, ptr(out), stream_ptr()), "bd_cat2_fwd")
    return out


def cat2_bwd(g, M, Ca, Cb, d_a, d_b, up=False, N=0, H=0, W=0, acc_a=False, acc_b=False):
    """The split of g bf16 (M, Ca + Cb): d_a (the 2x2 sums under `up`) and d_b, each written or, under its acc flag, added onto."""
    check(L().bd_cat2_bwd(ptr(g), M, Ca, Cb, int(bool(up)), N, H, W, ptr(d_a), int(bool(acc_a)), ptr(d_b), int(bool(acc_b)), stream_ptr()),
          "bd_cat2_bwd")
    return d_a, d_b


def focus_fwd(x_halo, N, H, W, out):
    """x_halo bf16 (N, H+6, W+8, 4) -> out bf16 (N*(H/2)*(W/2), 16): Focus's space-to-depth, channels 12-15 zero."""
    check(L().bd_focus_fwd(ptr(x_halo), N, H, W, ptr(out), stream_ptr()), "bd_focus_fwd")
    return out
