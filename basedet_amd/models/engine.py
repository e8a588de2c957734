"""Host-side runtime for the HIP training path: parameter arenas, packed-weight maintenance and the
conv layer object whose forward / dgrad / wgrad map 1:1 onto the C ABI (include/basedet_hip.h).

torch tensors are used as the memory carrier only -- no torch operator computes anything on this path
(allocation, zero-fill and views aside).
"""
import numpy as np
import torch

from .. import ops
from ..ops import Geom

BN_EPS = 1e-5  # basecore FrozenBatchNorm eps (un-vendored; documented choice, same as oracle/model.py)


class ParamArena:
    """Flat fp32 arenas (weights / gradients / momentum) for all trainable parameters: one SGD launch,
    contiguous buckets for the RCCL all-reduce (solver/default_solver.py:118-124)."""

    def __init__(self, device):
        self.device = device
        self.entries = []   # (name, shape, offset, numel)
        self.total = 0
        self.w = self.g = self.v = None

    def reserve(self, name, shape):
        n = int(np.prod(shape))
        off = self.total
        self.entries.append((name, tuple(shape), off, n))
        self.total += (n + 63) // 64 * 64     # 256-byte aligned slices
        return len(self.entries) - 1

    def allocate(self):
        self.w = torch.zeros(self.total, dtype=torch.float32, device=self.device)
        self.g = torch.zeros(self.total, dtype=torch.float32, device=self.device)
        self.v = torch.zeros(self.total, dtype=torch.float32, device=self.device)

    def view(self, which, idx):
        _, shape, off, n = self.entries[idx]
        return getattr(self, which)[off:off + n].view(shape)


class HostToDevice:
    """data_to_input's `Tensor(image)` (layers/common/pre_processing.py:13): a host batch (the loaders yield float64 / float32 / uint8
    numpy arrays) becomes the fp32 device tensor through bd_h2d_submit -- the library's worker threads convert it chunk by chunk into
    pinned memory and every chunk leaves with its own DMA as soon as it is converted (conversion under transfer).  The stager is created
    by the first host batch; `dst`, the tensor returned, is a view of one grow-only buffer for every input shape (the copies and their
    reader run on the current stream).  MODEL.H2D_THREADS / H2D_CHUNK_ELEMS are read, at each call, from the `cfg` given here: the model's
    config object at construction (a model that is given another config object afterwards needs another HostToDevice)."""

    def __init__(self, device, cfg):
        self.device, self.cfg = device, cfg
        self.stager = self.buf = self.dst = None

    def __call__(self, image):
        arr = image.numpy() if torch.is_tensor(image) else np.asarray(image)
        if self.stager is None:
            self.stager = ops.HostStager(self.device, int(self.cfg.MODEL.get("H2D_THREADS", 0)))
        if not self.stager.supports(arr):
            arr = np.ascontiguousarray(arr, dtype=np.float32)
        if self.buf is None or self.buf.numel() < arr.size:
            self.buf = torch.empty((arr.size,), dtype=torch.float32, device=self.device)
        self.dst = self.buf[: arr.size].view(arr.shape)
        return self.stager.submit(arr, self.dst, int(self.cfg.MODEL.get("H2D_CHUNK_ELEMS", 0)))


class ConvLayer:
    """One convolution (+ folded FrozenBN or bias).  Master weight fp32 [Cout][R][S][Cin] (OHWI);
    bf16 packed copies for the forward ([Cout][RS][Cin], BN scale folded in) and dgrad ([Cin][RS][Cout]) kernels."""

    def __init__(self, name, cin, cout, k, stride, pad, device, bn_prefix=None, has_bias=False, trainable=True,
                 cout_pad=None, norm=None):
        self.name, self.cin, self.cout_real, self.k, self.stride, self.pad = name, cin, cout, k, stride, pad
        # BatchNormState of a normalised convolution (MODEL.FPN.NORM; MODEL.BACKBONE.NORM = "BN" / "SyncBN": named by the reference's
        # bnK / downsample.1 prefix, bn_prefix then None): its slots follow the weight's
        self.norm = norm
        self.cout = cout_pad or cout          # padded channel count seen by the kernels (bbox_pred: 36 -> 40)
        self.bn_prefix, self.has_bias, self.trainable = bn_prefix, has_bias, trainable
        self.device = device
        self.w = self.b = self.gw = self.gb = None
        self.row_scale = None
        self.w_fwd = torch.empty((self.cout, k * k, cin), dtype=torch.bfloat16, device=device)
        self.w_dgrad = torch.empty((cin, k * k, self.cout), dtype=torch.bfloat16, device=device) if trainable else None
        self._desc_cache = {}
        # gradient skip (MODEL.SPARSE_BOX_BWD): the bf16 backward launches carry bd_conv_desc.gskip and compute only the patches a nonzero
        # gradient reaches (the same bits); forward launches keep the plain descriptor
        self.gskip = False
        self._gskip_cache = {}          # id(plain descriptor) -> (gskip descriptor, plain descriptor)
        self._gskip_ws = None
        # liveness maps of this step's launches (set_chain): the map of the gradient this layer reads, the map of the gradient its data
        # gradient writes, and the promise about that buffer's bytes (bd_conv_desc.gskip_gmap / gskip_dxmap / gskip_dx_clean)
        self._chain = (None, None, False)
        self._chain_cache = {}
        # forward skip (MODEL.SPARSE_BOX_FWD): descriptors that carry a forward liveness map (bd_conv_desc.fwd_map / fwd_clean)
        self._fwd_map_cache = {}
        # fp8 forward (BASELINE config 5, enable_fp8): e4m3 weights with one scale per output channel + the input cast to e4m3
        self.fp8 = False
        self.fp8_dgrad = False          # data gradient on the fp8 patch kernel too (e5m2 gradients under a static gradient scale)
        self.fp8_wgrad = False          # 3x3 weight gradient from the one-byte twins of x and g (bd_conv2d_wgrad_fp8) when both are handed over
        self.fp8_1x1 = False            # dense 1x1 launches on one-byte operands when the producer wrote the input's twin (bd_conv1x1_fp8)
        self.fp8_1x1_dgrad = False
        self.w_q8 = self.w_scale8 = self.w_q8t = self.w_scale8t = None
        self.act_scale = 1.0
        self.grad_scale = 4096.0
        self.amax_slot = None          # delayed scaling of the e5m2 gradients (fpn_base): where max |g| goes on probe steps
        self.probe_ctl = None
        self.q8_scratch = None          # callable(nbytes) -> uint8 scratch tensor on the stream this layer's forward runs on

    # -- parameters -------------------------------------------------------------------------------
    def bind(self, arena, params):
        """Load numpy parameters (reference layout) into arena views / standalone tensors."""
        w = torch.from_numpy(params[self.name + ".weight"]).permute(0, 2, 3, 1).contiguous()   # OIHW -> OHWI
        if self.cout != self.cout_real:
            pad = torch.zeros((self.cout - self.cout_real,) + tuple(w.shape[1:]))
            w = torch.cat([w, pad], 0)
        if self.trainable:
            self.w = arena.view("w", self._wi); self.gw = arena.view("g", self._wi)
            self.w.copy_(w)
        else:
            self.w = w.to(self.device)
        if self.bn_prefix:
            g, b = params[self.bn_prefix + ".weight"], params[self.bn_prefix + ".bias"]
            m, v = params[self.bn_prefix + ".running_mean"], params[self.bn_prefix + ".running_var"]
            scale = g / np.sqrt(v + BN_EPS)
            self.row_scale = torch.from_numpy(scale.astype(np.float32)).to(self.device)
            self.b = torch.from_numpy((b - m * scale).astype(np.float32)).to(self.device)
        elif self.has_bias:
            b = torch.from_numpy(params[self.name + ".bias"])
            if self.cout != self.cout_real:
                b = torch.cat([b, torch.zeros(self.cout - self.cout_real)])
            if self.trainable:
                self.b = arena.view("w", self._bi); self.gb = arena.view("g", self._bi)
                self.b.copy_(b)
            else:
                self.b = b.to(self.device)
        if self.norm is not None:
            self.norm.bind(arena, params)

    def reserve(self, arena):
        if not self.trainable:
            return
        self._wi = arena.reserve(self.name + ".weight", (self.cout, self.k, self.k, self.cin))
        if self.has_bias:
            self._bi = arena.reserve(self.name + ".bias", (self.cout,))
        if self.norm is not None:
            self.norm.reserve(arena)

    def export(self, out):
        """Back to the reference layout (OIHW numpy)."""
        out[self.name + ".weight"] = self.w[: self.cout_real].permute(0, 3, 1, 2).contiguous().cpu().numpy()
        if self.has_bias and not self.bn_prefix:
            out[self.name + ".bias"] = self.b[: self.cout_real].cpu().numpy().copy()
        if self.norm is not None:
            self.norm.export(out)

    def export_grad(self, out):
        out[self.name + ".weight"] = self.gw[: self.cout_real].permute(0, 3, 1, 2).contiguous().cpu()
        if self.gb is not None:
            out[self.name + ".bias"] = self.gb[: self.cout_real].cpu().clone()
        if self.norm is not None:
            self.norm.export_grad(out)

    def enable_fp8(self, q8_scratch, act_scale=1.0, dgrad=False, grad_scale=4096.0, wgrad=False):
        """Forward through bd_conv2d_fwd_fp8 (csrc/conv3x3_pp8.hip / conv_fp8.hip); with dgrad=True the data gradient through
        bd_conv2d_dgrad_fp8 as well (3x3 / stride 1 / Cin > 128).  The weight gradient keeps the bf16 activations and gradients."""
        assert self.cin % 16 == 0 and self.cout % 8 == 0
        self.fp8, self.q8_scratch, self.act_scale = True, q8_scratch, float(act_scale)
        self.w_q8 = torch.empty((self.cout, self.k * self.k, self.cin), dtype=torch.uint8, device=self.device)
        self.w_scale8 = torch.empty((self.cout,), dtype=torch.float32, device=self.device)
        if wgrad and self.trainable and self.k == 3 and self.stride == 1 and self.cin % 16 == 0 and self.cout % 16 == 0:
            self.fp8_wgrad, self.grad_scale = True, float(grad_scale)
        if dgrad and self.trainable and self.k == 3 and self.stride == 1 and self.cin > 128 and self.cout % 16 == 0:
            self.fp8_dgrad, self.grad_scale = True, float(grad_scale)
            self.w_q8t = torch.empty((self.cin, self.k * self.k, self.cout), dtype=torch.uint8, device=self.device)
            self.w_scale8t = torch.empty((self.cin,), dtype=torch.float32, device=self.device)

    def enable_fp8_1x1(self, act_scale=1.0, dgrad=False, grad_scale=4096.0, expanding=True):
        """1x1 / stride 1 layers: forward through bd_conv1x1_fp8 whenever the caller hands over the e4m3 twin of the input (never a cast
        pass: the launch is memory-bound, a cast would cost what the one-byte operand saves), with dgrad=True the data gradient too
        (from the e5m2 twin of the output gradient).  Weight gradients stay bf16."""
        assert self.k == 1 and self.stride == 1 and self.cin % 32 == 0 and self.cout % 32 == 0
        self.act_scale, self.grad_scale = float(act_scale), float(grad_scale)
        # expanding=False keeps only the REDUCING direction (K >= 2 x produced channels: conv1 forward, conv3's data gradient), where the
        # one-byte operand is most of the launch's bytes; the expanding direction is all epilogue (bf16 residual in, bf16 + twin + gate
        # bits out).  See FPNDetector._build_layers for what was measured
        if self.cin % 128 == 0 and (self.cin >= 2 * self.cout or expanding):
            self.fp8_1x1 = True
            self.w_q8 = torch.empty((self.cout, 1, self.cin), dtype=torch.uint8, device=self.device)
            self.w_scale8 = torch.empty((self.cout,), dtype=torch.float32, device=self.device)
        if dgrad and self.trainable and self.cout % 128 == 0 and (self.cout >= 2 * self.cin or expanding):
            self.fp8_1x1_dgrad = True
            self.w_q8t = torch.empty((self.cin, 1, self.cout), dtype=torch.uint8, device=self.device)
            self.w_scale8t = torch.empty((self.cin,), dtype=torch.float32, device=self.device)

    def pack_fp8(self):
        if self.k == 1 and (self.fp8_1x1 or self.fp8_1x1_dgrad):
            if self.fp8_1x1:
                ops.weight_pack_fp8(self.w, self.row_scale, self.cout, 1, self.cin, self.act_scale, self.w_q8, self.w_scale8)
            if self.fp8_1x1_dgrad:
                ops.weight_pack_fp8_t(self.w, self.row_scale, self.cout, 1, self.cin, self.grad_scale, self.w_q8t, self.w_scale8t)
            return
        ops.weight_pack_fp8(self.w, self.row_scale, self.cout, self.k * self.k, self.cin, self.act_scale, self.w_q8, self.w_scale8)
        if self.fp8_dgrad:
            ops.weight_pack_fp8_t(self.w, self.row_scale, self.cout, self.k * self.k, self.cin, self.grad_scale, self.w_q8t, self.w_scale8t)

    def pack(self):
        ops.weight_pack(self.w, self.row_scale, self.w_fwd, self.w_dgrad, self.cout, self.k * self.k, self.cin)
        if self.fp8 or self.fp8_1x1 or self.fp8_1x1_dgrad:
            self.pack_fp8()

    # -- kernels ----------------------------------------------------------------------------------
    def desc(self, gin: Geom, gout: Geom):
        key = (gin.N, tuple(gin.H), tuple(gin.W), tuple(gin.off), gin.pix_per_img,
               tuple(gout.H), tuple(gout.W), tuple(gout.off), gout.pix_per_img)
        d = self._desc_cache.get(key)
        if d is None:
            d = ops.conv_desc(gin, gout, self.cin, self.cout, self.k, self.k, self.stride, self.pad)
            self._desc_cache[key] = d
        return d

    def bwd_desc(self, gin: Geom, gout: Geom):
        """desc() for the data and weight gradient: with self.gskip, a copy that carries the gradient-skip hint and this layer's scratch."""
        d = self.desc(gin, gout)
        if not self.gskip:
            return d
        h = self._gskip_cache.get(id(d))
        if h is None:
            # ONE grow-only scratch per layer, whatever the number of shapes: the layer's data gradient runs once per step, on the main
            # stream, and the scan / compact launches rewrite what they read.  A larger shape replaces it: the cached descriptors hold
            # the old pointer and are rebuilt
            n = (max(ops.conv2d_dgrad_gskip_bytes(d), 4) + 3) // 4
            if self._gskip_ws is None or self._gskip_ws.numel() < n:
                self._gskip_ws = torch.empty(n, dtype=torch.int32, device=self.device)
                self._gskip_cache.clear()
            h = self._gskip_cache[id(d)] = (ops.gskip_desc(d, self._gskip_ws), d)
        gmap, dxmap, clean = self._chain
        if gmap is None and dxmap is None:
            return h[0]
        # (keyed by the maps' addresses: the plan arena re-bases them when it grows)
        key = (id(d), self._gskip_ws.data_ptr(), gmap.data_ptr() if gmap is not None else 0, dxmap.data_ptr() if dxmap is not None else 0, clean)
        c = self._chain_cache.get(key)
        if c is None:
            if len(self._chain_cache) > 64:
                self._chain_cache.clear()
            c = self._chain_cache[key] = (ops.gskip_desc(d, self._gskip_ws, gmap=gmap, dxmap=dxmap, dx_clean=clean), d)
        return c[0]

    def set_chain(self, gmap=None, dxmap=None, dx_clean=False):
        """The liveness maps this layer's NEXT hinted backward launches carry (None: scan g / write no map, as without a chain): gmap = the
        map of the gradient it reads, dxmap = the map its data gradient writes for the next layer down, dx_clean = the caller knows that
        the data gradient's output buffer still holds the layout the previous step left (see bd_conv_desc.gskip_dx_clean)."""
        self._chain = (gmap, dxmap, bool(dx_clean) and dxmap is not None) if self.gskip else (None, None, False)

    def fwd_map_desc(self, gin: Geom, gout: Geom, fmap, clean):
        """desc() with the forward liveness map of the output and the promise about the output buffer's bytes (ops.fwd_map_desc)."""
        d = self.desc(gin, gout)
        key = (id(d), fmap.data_ptr(), bool(clean))          # (keyed by the map's address: the plan arena re-bases it when it grows)
        c = self._fwd_map_cache.get(key)
        if c is None:
            if len(self._fwd_map_cache) > 64:
                self._fwd_map_cache.clear()
            c = self._fwd_map_cache[key] = (ops.fwd_map_desc(d, fmap, clean), d)
        return c[0]

    def forward(self, x, gin, gout, y, add=None, relu=False, bits=None, x8=None, y8=None, q_scale=1.0, fwd_map=None, fwd_clean=False):
        """x8: the e4m3 twin of x when a producing fp8 launch wrote one (else x is cast by bd_quantize_fp8); y8: twin of y to write
        for a following fp8 convolution.  Both are ignored on the bf16 path.  fwd_map: the forward liveness map of y (bf16 path only): only
        the patches on its list are computed, the rest of y is +0 (fwd_clean: see bd_conv_desc.fwd_clean)."""
        flags = (ops.EPI_RELU if relu else 0) | (ops.EPI_ADD_BEFORE if add is not None else 0)
        if fwd_map is not None:
            assert not self.fp8 and not self.fp8_1x1 and bits is None and y8 is None
            return ops.conv2d_fwd(self.fwd_map_desc(gin, gout, fwd_map, fwd_clean), x, self.w_fwd, self.b, y, add=add, flags=flags)
        if self.fp8_1x1 and x8 is not None and ops.conv1x1_fp8_ok(self.desc(gin, gout), 0):
            return ops.conv1x1_fp8(self.desc(gin, gout), 0, x8, self.w_q8, self.w_scale8, self.b, y, add=add, bits=bits, y8=y8,
                                   q_scale=q_scale, flags=flags)
        if self.fp8 and bits is None:
            xq = x8 if x8 is not None else ops.quantize_fp8(x, self.act_scale, self.q8_scratch(x.numel())[: x.numel()])
            return ops.conv2d_fwd_fp8(self.desc(gin, gout), xq, self.w_q8, self.w_scale8, self.b, y, add=add, flags=flags, y8=y8,
                                      q_scale=self.act_scale)
        return ops.conv2d_fwd(self.desc(gin, gout), x, self.w_fwd, self.b, y, add=add, flags=flags, bits=bits,
                              y8=y8 if (y8 is not None and ops.dense_1x1_bits_ok(self.desc(gin, gout))) else None, q_scale=q_scale)

    def gnstats_ok(self):
        """True when forward_gnstats serves this layer: a bf16 3x3 / stride-1 convolution into GroupNorm(32, 256)'s 256 channels."""
        return (not self.fp8) and self.k == 3 and self.stride == 1 and self.pad == 1 and self.cout == 256 and self.cin % 64 == 0

    def forward_gnstats(self, x, gin, gout, y, part):
        """forward() of a tower convolution that also leaves GroupNorm's per-patch statistics in `part` (ops.conv2d_fwd_gnstats)."""
        return ops.conv2d_fwd_gnstats(self.desc(gin, gout), x, self.w_fwd, self.b, y, part)

    def dgrad(self, g, gin, gout, dx, first=True, mask=None, add_after=None, maskbits=None, g8=None, dx8=None, q_scale=1.0,
              add_before=None, sparse=False):
        """dx (+)= conv^T(g); returns True when the launch also wrote the e5m2 twin dx8 (= dx * q_scale, q_scale = the CONSUMER's
        gradient scale).  first=False accumulates onto dx (pre-mask); mask = forward activation whose
        ReLU gates dx (maskbits: the same gate bit-packed, written by the producing forward launch); add_after = tensor added
        after masking (P6: gradient that bypasses the ReLU)."""
        flags, add = 0, None
        if add_after is not None:
            flags |= ops.EPI_ADD_AFTER
            add = add_after
        elif add_before is not None:                 # dx = (conv^T(g) + add_before) * mask: the identity skip's gradient joins here
            flags |= ops.EPI_ADD_BEFORE
            add = add_before
        elif not first:
            flags |= ops.EPI_ADD_BEFORE
            add = dx
            if sparse and self.stride > 1:       # strided shortcut accumulating in place: pixels no tap reaches keep their (final) value
                flags |= ops.EPI_SPARSE
        if mask is not None or maskbits is not None:
            flags |= ops.EPI_MASK
        if maskbits is not None:
            mask = None
        d = self.bwd_desc(gin, gout)
        if self.amax_slot is not None and self.probe_ctl[0] and (self.fp8_1x1_dgrad or self.fp8_dgrad):
            ops.absmax_bf16(g, self.amax_slot)
        if self.fp8_1x1_dgrad and g8 is not None and ops.conv1x1_fp8_ok(d, 1):
            ops.conv1x1_fp8(d, 1, g8, self.w_q8t, self.w_scale8t, None, dx, add=add, mask=mask, maskbits=maskbits, y8=dx8,
                            q_scale=q_scale, flags=flags)
            return dx8 is not None
        if self.fp8_dgrad and maskbits is None:
            # g8: the e5m2 twin of g (g * grad_scale) when the producing launch wrote one, else a cast pass; dx8: twin of dx to write
            gq = g8 if g8 is not None else ops.quantize_bf8(g, self.grad_scale, self.q8_scratch(g.numel())[: g.numel()])
            ops.conv2d_dgrad_fp8(d, gq, self.w_q8t, self.w_scale8t, dx, add=add, mask=mask, flags=flags, dx8=dx8, q_scale=q_scale)
            return dx8 is not None
        if dx8 is not None and not ops.dense_1x1_bits_ok(d):
            dx8 = None               # only the dense 1x1 kernel writes a twin on the bf16 path: the caller must not mark it ready
        ops.conv2d_dgrad(d, g, self.w_dgrad, dx, add=add, mask=mask, flags=flags, maskbits=maskbits, dx8=dx8, q_scale=q_scale)
        return dx8 is not None

    def dgrad_writes_twin(self, gin, gout):
        """True when dgrad(..., dx8=t) fills t: the fp8 patch kernel and the dense 1x1 kernel do, the other bf16 kernels do not."""
        return self.fp8_dgrad or ops.dense_1x1_bits_ok(self.desc(gin, gout))

    def wgrad(self, x, g, gin, gout, ws, colsum_ws=None, x8=None, g8=None, queue=None):
        """x8 / g8: the e4m3 twin of x (x * act_scale) and the e5m2 twin of g (g * grad_scale) when their producers wrote them: the
        weight gradient then runs on the one-byte kernel (the bias gradient stays a column sum of the bf16 g)."""
        d = self.bwd_desc(gin, gout)
        if self.fp8_wgrad and x8 is not None and g8 is not None:
            ops.conv2d_wgrad_fp8(d, x8, g8, 1.0 / (self.act_scale * self.grad_scale), self.gw, ws, row_scale=self.row_scale)
            if self.gb is not None:
                ops.colsum_bf16(g, g.shape[0], self.cout, self.gb, colsum_ws)
            return
        if queue is not None:        # ops.WgradQueue: the reduce waits for the caller's flush (ws stays untouched until then)
            queue.wgrad(d, x, g, self.gw, self.gb, ws, row_scale=self.row_scale)
        elif self.gb is not None:    # weight + bias gradient in one entry point (fused in the 3x3 patch kernel; colsum_ws is unused)
            ops.conv2d_wgrad_bias(d, x, g, self.gw, self.gb, ws, row_scale=self.row_scale)
        else:
            ops.conv2d_wgrad(d, x, g, self.gw, ws, row_scale=self.row_scale)

    def thin_backward_ok(self, gin: Geom):
        """True when bd_conv1x1_thin_bwd covers this layer on geometry gin: 1x1 / stride 1, 256 -> 16 (padded) channels, bf16, no BN scale,
        every pixel row of the buffer (all levels of the pyramid, contiguous)."""
        return (self.k == 1 and self.stride == 1 and self.pad == 0 and self.cin == 256 and self.cout == 16 and self.trainable
                and self.row_scale is None and self.gb is not None and not (self.fp8 or self.fp8_1x1)
                and sum(h * w for h, w in zip(gin.H, gin.W)) == gin.pix_per_img)

    def thin_forward(self, x, gin: Geom, y):
        """y = conv(x) + bias on the thin-layer kernel (fp32 master weights rounded to bf16 in the kernel, as pack() does)."""
        ops.conv1x1_thin_fwd(x, self.w, self.b, gin.pixels, self.cin, self.cout, y)

    def thin_backward(self, x, g, gin: Geom, dx, ws):
        """dx = (x > 0) * conv^T(g), dW, dbias in one pass over x (x = the ReLU output this layer reads).  Same results as
        wgrad(x, g) + dgrad(g, mask=x) up to fp32 summation order."""
        ops.conv1x1_thin_bwd(x, g, self.w, gin.pixels, self.cin, self.cout, dx, self.gw, self.gb, self.cout_real, ws)

    def wgrad_ws_bytes(self, gin, gout):
        d = self.bwd_desc(gin, gout)
        n = ops.conv2d_wgrad_bias_workspace_bytes(d) if self.gb is not None else ops.conv2d_wgrad_workspace_bytes(d)
        return max(n, ops.conv2d_wgrad_fp8_workspace_bytes(d)) if self.fp8_wgrad else n


class FusedPredConv(ConvLayer):
    """Several reference convs that read the same input, fused along Cout into one launch (FCOS bbox_pred [4] + ctrness [1]
    -> 5 rows, padded to 8).  Parameters are bound from / exported to the reference's separate tensors."""

    def __init__(self, name, parts, cin, k, stride, pad, device, cout_pad):
        self.parts = parts   # [(reference conv name, cout)]
        super().__init__(name, cin, sum(c for _, c in parts), k, stride, pad, device, has_bias=True, trainable=True, cout_pad=cout_pad)

    def bind(self, arena, params):
        merged = dict(params)
        merged[self.name + ".weight"] = np.concatenate([params[n + ".weight"] for n, _ in self.parts], 0)
        merged[self.name + ".bias"] = np.concatenate([params[n + ".bias"] for n, _ in self.parts], 0)
        super().bind(arena, merged)

    def export(self, out):
        o = 0
        for n, c in self.parts:
            out[n + ".weight"] = self.w[o:o + c].permute(0, 3, 1, 2).contiguous().cpu().numpy()
            out[n + ".bias"] = self.b[o:o + c].cpu().numpy().copy()
            o += c

    def export_grad(self, out):
        o = 0
        for n, c in self.parts:
            out[n + ".weight"] = self.gw[o:o + c].permute(0, 3, 1, 2).contiguous().cpu()
            out[n + ".bias"] = self.gb[o:o + c].cpu().clone()
            o += c


class TrainableStem:
    """backbone.bottom_up.conv1 under MODEL.BACKBONE.FREEZE_AT = 0: the 7x7 stem's fp32 master and gradient in the parameter arena, OHWI
    [64][7][7][3] like every ConvLayer master (what bd_stem_weight_pack reads and bd_stem_conv7x7_wgrad writes); state_dict, checkpoints and
    reference_grads see the reference's OIHW (64, 3, 7, 7).  The object WgradScheduler.run takes: the weight gradient runs on the side stream."""

    fp8_wgrad = False
    norm = None          # BatchNormState "<prefix>.bn1" (backbone.bottom_up.bn1; CenterNet: backbone.bn1) under MODEL.BACKBONE.NORM = "BN" / "SyncBN": right behind the weight

    def __init__(self, name="backbone.bottom_up.conv1"):
        self.name = name          # (a bare ResNet, CenterNet's: "backbone.conv1")

    def reserve(self, arena):
        self._wi = arena.reserve(self.name + ".weight", (64, 7, 7, 3))
        if self.norm is not None:
            self.norm.reserve(arena)

    def bind(self, arena, w_ohwi, row_scale):
        self.w = arena.view("w", self._wi); self.gw = arena.view("g", self._wi)
        self.w.copy_(w_ohwi)
        self.row_scale = row_scale
        return self.w

    def export_grad(self, out):
        out[self.name + ".weight"] = self.gw.permute(0, 3, 1, 2).contiguous().cpu()
        if self.norm is not None:
            self.norm.export_grad(out)

    def forward(self, x, gin, gout, y):
        """The bare convolution under a live norm (no shift, no ReLU; `packed`: the model's stem_packed, then without a row scale)."""
        ops.stem_conv7x7_raw_fwd(gin.N, gin.H[0], gin.W[0], x, self.packed, y)

    def wgrad(self, x, g, gin, gout, ws, colsum_ws=None, x8=None, g8=None, queue=None):
        """x: x_halo of the padded batch (gin: its N x Hp x Wp geometry), g: dL/d(pre-activation) of the stem output."""
        ops.stem_conv7x7_wgrad(gin.N, gin.H[0], gin.W[0], x, g, self.gw, ws, row_scale=self.row_scale)

    def wgrad_ws_bytes(self, gin, gout):
        return ops.stem_conv7x7_wgrad_workspace_bytes(gin.N, gin.H[0], gin.W[0])


def cls_ld(K):
    """Slots one anchor's class logits occupy: K rounded up to a multiple of 8 (16-byte rows of bf16)."""
    return (int(K) + 7) // 8 * 8


def pad_class_rows(a, A, K):
    """Reference rows (A*K, ...) (row a*K + k, retina_head.py:66 / point_head.py:88) -> A groups of cls_ld(K) rows, the pad rows zero."""
    ld = cls_ld(K)
    a = np.asarray(a)
    assert a.shape[0] == A * K, (a.shape, A, K)
    if ld == K:
        return a
    out = np.zeros((A, ld) + a.shape[1:], a.dtype)
    out[:, :K] = a.reshape((A, K) + a.shape[1:])
    return out.reshape((A * ld,) + a.shape[1:])


def unpad_class_rows(a, A, K):
    """The inverse gather, (A*cls_ld(K), ...) -> (A*K, ...); numpy arrays and torch tensors alike."""
    ld = cls_ld(K)
    assert a.shape[0] == A * ld, (a.shape, A, K)
    if ld == K:
        return a
    return a.reshape((A, ld) + tuple(a.shape[1:]))[:, :K].reshape((A * K,) + tuple(a.shape[1:]))


class PaddedClsConv(ConvLayer):
    """The class predictor of a one-stage head (head.cls_score) at any class count: the reference's A*K output channels (anchor-major)
    are kept as A groups of cls_ld = round_up(K, 8) rows, so that every anchor's K logits start on a 16-byte boundary of the
    [pixels][A * cls_ld] bf16 output.  bind scatters the reference's (A*K, Cin, k, k) weight and (A*K,) bias into the groups; export and
    export_grad gather back: checkpoints, state_dict, reference_grads and the EMA keep the reference's names and shapes.  K % 8 == 0: the
    mapping is the identity and this is a plain ConvLayer.

    INVARIANT: the pad rows of the weight, the bias, their gradients and the momentum are exactly zero for a whole run.  bind zeroes
    them; every loss writes a zero gradient into the pad slots of d_logits (bd_focal_loss_fwd_bwd, bd_freeanchor_loss_fwd_bwd), so
    the weight and bias gradients of the pad rows are sums of zeros; SGD with momentum and weight decay, gradient clipping, the EMA and
    the gradient all-reduce map zero to zero.  tests/test_class_count_gpu.py::test_pad_rows_stay_zero holds this."""

    def __init__(self, name, cin, A, K, k, stride, pad, device):
        self.A, self.K, self.cls_ld = int(A), int(K), cls_ld(K)
        super().__init__(name, cin, self.A * self.K, k, stride, pad, device, has_bias=True, trainable=True, cout_pad=self.A * self.cls_ld)

    def bind(self, arena, params):
        w = pad_class_rows(np.asarray(params[self.name + ".weight"], np.float32), self.A, self.K)
        b = pad_class_rows(np.asarray(params[self.name + ".bias"], np.float32), self.A, self.K)
        self.w = arena.view("w", self._wi); self.gw = arena.view("g", self._wi)
        self.w.copy_(torch.from_numpy(w).permute(0, 2, 3, 1).contiguous())             # OIHW -> OHWI
        self.b = arena.view("w", self._bi); self.gb = arena.view("g", self._bi)
        self.b.copy_(torch.from_numpy(b))

    def export(self, out):
        out[self.name + ".weight"] = unpad_class_rows(self.w, self.A, self.K).permute(0, 3, 1, 2).contiguous().cpu().numpy()
        out[self.name + ".bias"] = unpad_class_rows(self.b, self.A, self.K).cpu().numpy().copy()

    def export_grad(self, out):
        out[self.name + ".weight"] = unpad_class_rows(self.gw, self.A, self.K).permute(0, 3, 1, 2).contiguous().cpu()
        out[self.name + ".bias"] = unpad_class_rows(self.gb, self.A, self.K).cpu().clone()

    def real_logits(self, t):
        """[..., A * cls_ld] predictions or gradients -> the real class slots, [..., A * K]."""
        if self.cls_ld == self.K:
            return t
        return t.reshape(tuple(t.shape[:-1]) + (self.A, self.cls_ld))[..., : self.K].reshape(tuple(t.shape[:-1]) + (self.A * self.K,))


class FCLayer(ConvLayer):
    """megengine.module.Linear (or several that read the same input, fused along the output dimension) as a 1x1 convolution
    whose "pixels" are the rows.  The reference flattens RoI features as (c, h, w) (layers/head/rcnn.py:59); the HIP
    RoIAlign writes (h, w, c), so for `in_chw` layers the master weight is kept with permuted columns -- an elementwise SGD
    does not care -- and permuted back on export."""

    def __init__(self, name, cin, cout, device, in_chw=None, parts=None, cout_pad=None):
        self.in_chw = in_chw
        self.parts = parts          # [(reference linear name, out features)]
        super().__init__(name, cin, cout, 1, 1, 0, device, has_bias=True, trainable=True, cout_pad=cout_pad)

    def _names(self):
        return [n for n, _ in self.parts] if self.parts else [self.name]

    def _to_ours(self, w):
        if self.in_chw:
            c, h, wd = self.in_chw
            w = w.reshape(-1, c, h, wd).permute(0, 2, 3, 1).reshape(-1, c * h * wd)
        return w.contiguous()

    def _to_ref(self, w):
        if self.in_chw:
            c, h, wd = self.in_chw
            w = w.reshape(-1, h, wd, c).permute(0, 3, 1, 2).reshape(-1, c * h * wd)
        return w.contiguous()

    def bind(self, arena, params):
        w = np.concatenate([np.asarray(params[n + ".weight"], np.float32) for n in self._names()], 0)
        b = np.concatenate([np.asarray(params[n + ".bias"], np.float32) for n in self._names()], 0)
        w = self._to_ours(torch.from_numpy(w)).numpy().reshape(self.cout_real, self.cin, 1, 1)
        super().bind(arena, {self.name + ".weight": w, self.name + ".bias": b})

    def _split(self, w, b, out, to_numpy):
        w = self._to_ref(w[: self.cout_real].reshape(self.cout_real, self.cin))
        b = b[: self.cout_real]
        o = 0
        for n, c in (self.parts or [(self.name, self.cout_real)]):
            wn, bn = w[o:o + c].cpu(), b[o:o + c].cpu()
            out[n + ".weight"] = wn.numpy().copy() if to_numpy else wn.clone()
            out[n + ".bias"] = bn.numpy().copy() if to_numpy else bn.clone()
            o += c

    def export(self, out):
        self._split(self.w, self.b, out, True)

    def export_grad(self, out):
        self._split(self.gw, self.gb, out, False)


class DeconvLayer(ConvLayer):
    """The FPN's learned top-down upsampling, M.ConvTranspose2d(C, C, 4, stride=2, padding=1, bias=False) (fpn_backbone.py:92-103,
    131-138).  The reference's (C_coarse, C_fine, 4, 4) weight is the OIHW weight of a fine -> coarse Conv2d(k4, s2, p1), so the master is
    kept in that conv view (OHWI [C_coarse][4][4][C_fine]) and ConvLayer's bind / export / export_grad and arena slot apply unchanged;
    forward / dgrad / wgrad run the dedicated kernels of csrc/fpn_deconv.hip (forward = the conv view's data gradient and back)."""

    def __init__(self, name, ch, device):
        super().__init__(name, ch, ch, 4, 2, 1, device)
        self.ch = ch
        # phase-major operands of bd_fpn_deconv_fwd ([4 classes][C_fine][4 taps][C_coarse]) and bd_fpn_deconv_dgrad ([C_coarse][16][C_fine])
        self.w_fwd = torch.empty((4, ch, 4, ch), dtype=torch.bfloat16, device=device)
        self.w_dgrad = torch.empty((ch, 16, ch), dtype=torch.bfloat16, device=device)

    def pack(self):
        ops.fpn_deconv_pack(self.w, self.ch, self.w_fwd, self.w_dgrad)

    def forward(self, x, gc: Geom, y, add=None):
        """y (fine level, 2H x 2W of gc) = bf16(add + conv_transpose(x)); add may be y (the merged lateral, in place)."""
        return ops.fpn_deconv_fwd(x, self.w_fwd, y, gc.N, gc.H[0], gc.W[0], self.ch, add=add)

    def dgrad(self, dy, gc: Geom, dx, add=None):
        """dx (coarse level gc) = bf16(add + conv4x4s2p1(dy)); add = dx accumulates onto the output convolution's data gradient."""
        return ops.fpn_deconv_dgrad(dy, self.w_dgrad, dx, gc.N, gc.H[0], gc.W[0], self.ch, add=add)

    def wgrad(self, x, g, gin, gout, ws, colsum_ws=None, x8=None, g8=None, queue=None):
        """x: the coarse input (gout: its geometry), g: the fine output's gradient (gin) -- the conv view's (g, x) roles."""
        ops.fpn_deconv_wgrad(x, g, self.gw, ws, gout.N, gout.H[0], gout.W[0], self.ch)

    def wgrad_ws_bytes(self, gin, gout):
        return ops.fpn_deconv_wgrad_workspace_bytes(gout.N, gout.H[0], gout.W[0], self.ch)
