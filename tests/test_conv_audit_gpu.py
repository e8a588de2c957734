"""Per-element audit of every convolution launch of a bench-size training step (16 x 800 x 1344) against float64.

The model runs one forward + backward pass with the entry points of basedet_amd.ops wrapped (the SGD update that ends a training step
is left out: it launches no convolution, and the gradient arena it would read is compared bit for bit instead): each wrapper clones what the launch updates in
place, calls the kernel, synchronises, reads bd_conv_last_kernel(), recomputes the launch in float64 from ITS OWN operands (the packed bf16
weights the kernel received, tests/util.py) and checks every element; the kernel's output stays in place, so the step goes on with real
data.  Rows of an output buffer that the launch's levels do not cover must come back bit for bit as they were.

Bounds (derived, not tuned; S = the same operation on |operands|):
  * bf16 outputs (forward, data gradient, stem, fused blocks): the kernel rounds an fp32 value v to bf16, |bf16(v) - v| <= 2^-9 |v|, and
    |v - ref| <= delta, the fp32 accumulation error.  tol = 2^-8 |ref| + 2^-16 S: 2^-16 = 256 sequential fp32 roundings of at most
    2^-24 S each, more than the K loop of any bench descriptor takes (K = 2 304 bf16 products in MFMA steps of 16 / 32, the epilogue's
    bias / residual adds).  A tap missing from a 2 304-term sum moves the result by about S / 2 304 >> 2^-16 S.
  * elements that are exactly representable (a closed ReLU / mask gate: 0 or the bf16 `add`; a ReLU input below -2^-16 S; pixels a
    sparse strided data gradient must not touch) are compared for equality.
  * fp32 outputs (weight and bias gradients, column sums): a bound per launch from the kernel's own plan (fp32_roundings below, which
    mirrors the split plans of conv_wgrad3x3_ring.hip, conv_wgrad3x3.hip, conv_wgrad1x1_ring.hip, conv_wgrad1x1.hip and the column-sum
    pass of image_ops.hip).  A workgroup accumulates its pixel range in fp32 MFMA accumulators; each MFMA step sums K exact bf16 products
    and adds them to the accumulator: two roundings of at most 2^-24 S.  (One rounding per step is not enough: for the 720-channel
    cls_score bias on the ring kernel, 1 224 steps + 10 partials would allow 7.4e-5 S, and 1.0e-4 S is observed -- the 720 focal
    gradients are nearly one-signed, so the rounding errors add up.)  Then the fixed-order reduce adds the `splits` partials, the row
    scale and an accumulate add one rounding each.  tol = roundings x 2^-24 S, never looser than 2^-12 S.  The column-sum pass is plain
    fp32 adds: rows per thread + rows in flight + 1 024 / 32 + 32 partials + levels.
    Observed worst err / S on an MI355X (RetinaNet-R50 step, B = 16): weight gradients 8.6e-6 (conv_wgrad3x3_ring_kernel), 6.6e-7
    (conv_wgrad1x1_ring_kernel), 3.8e-7 (conv_wgrad3x3_kernel), 2.4e-7 (conv_wgrad1x1_kernel); bias gradients 1.0e-4 (ring kernel,
    cls_score).  The worst err / tol of each kernel is in the printed table.
  * A per-element bound cannot see a weight-gradient kernel drop a few pixels of a 268 800-pixel sum (one 64-pixel patch moves a weight
    by ~1e-5 S).  So every weight-gradient launch is repeated on the same descriptor (same kernel, same split plan) with g kept only at
    the first and the last pixel of every level of every image -- the pixels where a split, a patch row or a tail starts and ends -- and
    zero elsewhere: a pixel the kernel skips there costs about 1 / (2 N levels) of S, against a bound of ~1e-4 S.
  * upsample2x_add: the bilinear weights 0.75 / 0.25 are exact, <= 16 products and one add in fp32: tol = 2^-8 |ref| + 2^-19 S.

Every image of the batch is audited (the float64 references of a whole RetinaNet step take about 5 s on an MI355X).
"""
import collections
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import util as U

pytestmark = pytest.mark.gpu
SIZE = (800, 1344)
B = 16
REL_BF16, ABS_BF16 = 2.0 ** -8, 2.0 ** -16
U24 = 2.0 ** -24
MAX_F32 = 2.0 ** -12   # the loosest fp32 bound allowed


def _cdiv(a, b):
    return -(-a // b)


def _split(total, target_splits, min_per):
    """splits = clamp(target, 1, total / min_per), per = ceil(total / splits) (the plan functions of the weight-gradient kernels)."""
    splits = max(1, target_splits)
    splits = min(splits, max(total // min_per, 1))
    per = _cdiv(total, splits)
    return _cdiv(total, per), per


def fp32_roundings(d, kern, cus):
    """(weight-gradient roundings, bias-gradient roundings) of one launch, from the kernel's split plan; see the module docstring."""
    M = sum(d.N * d.Ho[s] * d.Wo[s] for s in range(d.nseg))
    if kern == "conv_wgrad3x3_ring_kernel":            # 64 ci x 128 co tiles, 8 x 8 patches, one workgroup per CU, >= 8 patches each
        tiles = _cdiv(d.Cin, 64) * _cdiv(d.Cout, 128)
        total = d.N * sum(_cdiv(d.Ho[s], 8) * _cdiv(d.Wo[s], 8) for s in range(d.nseg))
        splits, per = _split(total, cus // tiles, 8)
        px = per * 64
        steps = _cdiv(px, 32)                            # 16x16x32 MFMA: 32 pixels per step
    elif kern == "conv_wgrad3x3_kernel":               # 64 x 64 tiles, 8 x 8 (stride 1) / 4 x 8 (stride 2) patches, 512 workgroups
        ph = 8 if d.stride == 1 else 4
        tiles = _cdiv(d.Cin, 64) * _cdiv(d.Cout, 64)
        total = d.N * sum(_cdiv(d.Ho[s], ph) * _cdiv(d.Wo[s], 8) for s in range(d.nseg))
        splits, per = _split(total, 512 // tiles, 1)
        px = per * ph * 8
        steps = _cdiv(px, 16)                            # counted with 16 products per MFMA step: never fewer steps than the kernel takes
    elif kern == "conv_wgrad1x1_ring_kernel":          # 32-pixel K steps, one workgroup per CU, >= 8 steps each
        narrow = d.Cin <= 128 or d.Cout <= 128
        short_k = M < 32768 and d.Cout <= 256
        tci, tco = 128, (128 if (narrow or short_k) else 256)
        splits, per = _split(_cdiv(M, 32), cus // (_cdiv(d.Cin, tci) * _cdiv(d.Cout, tco)), 8)
        px = per * 32
        steps = _cdiv(px, 16)
    elif kern == "conv_wgrad1x1_kernel":               # 32-pixel K steps, 256 workgroups, >= 4 steps each; the tile that gives FEWER splits
        shapes = [(128, 512)] if d.Cin <= 128 else ([(512, 128), (256, 256)] if d.Cout <= 128 and d.Cin >= 512 else [(256, 256)])
        splits, per = max((_split(_cdiv(M, 32), 256 // (_cdiv(d.Cin, a) * _cdiv(d.Cout, b)), 4) for a, b in shapes), key=lambda t: t[1])
        px = per * 32
        steps = _cdiv(px, 16)
    else:                                              # a kernel this table does not know: one chain over every pixel
        splits, px = 1, M
        steps = _cdiv(M, 16)
    w = 2 * steps + splits + 2                           # two roundings per MFMA step, the reduce, row scale, accumulate
    rif = max(256 // (d.Cout // 8), 1)
    cs = _cdiv(M, 1024 * rif) + rif + 32 + 32 + d.nseg + 1
    # a bias gradient comes from the kernel's own column sums or from the column-sum pass; if the kernel sums them with one add per pixel
    # rather than in its MFMA steps, a chain is a split's pixel count
    return w, max(w, cs, px + splits + 2)


ABS_UPS = 2.0 ** -19
IMAGES = None          # None: every image of the batch in the forward / data-gradient references (else a list of image indices)

# entry points of basedet_amd.ops the wrappers replace, and the C ABI symbols that must only be reached through them
WRAPPED = ("conv2d_fwd", "conv2d_dgrad", "conv2d_wgrad", "conv2d_wgrad_bias", "colsum_bf16", "upsample2x_add_fwd", "upsample2x_add_bwd",
           "stem_pool_fwd", "bottleneck_fwd", "conv2d_fwd_gnstats", "groupnorm_fwd_parts")
CONV_ABI = ("bd_conv2d_fwd", "bd_conv2d_dgrad", "bd_conv2d_fwd_bits", "bd_conv2d_fwd_ex", "bd_conv2d_dgrad_ex", "bd_conv2d_dgrad_bits",
            "bd_conv2d_wgrad", "bd_conv2d_wgrad_bias", "bd_conv2d_wgrad_queued", "bd_conv2d_fwd_fp8_ex", "bd_conv2d_dgrad_fp8",
            "bd_conv1x1_fp8", "bd_conv2d_wgrad_fp8", "bd_conv1x1_thin_fwd", "bd_conv1x1_thin_bwd", "bd_stem_conv7x7_fwd", "bd_stem_pool_fwd",
            "bd_bottleneck_fwd", "bd_conv2d_fwd_gnstats", "bd_colsum_bf16", "bd_upsample2x_add_fwd", "bd_upsample2x_add_bwd")


def _rows(N, ppi, levels, device):
    """bool (N * ppi,): the rows of a pixel-major buffer that the levels [(off, count)] cover."""
    m = torch.zeros((N, ppi), dtype=torch.bool, device=device)
    for off, cnt in levels:
        m[:, off:off + cnt] = True
    return m.view(-1)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


class Audit:
    def __init__(self, ops):
        self.ops = ops
        self.stats = {}                            # (kernel, pass) -> [launches, worst err/tol, worst err/S]
        self.bad = []
        self.calls = collections.Counter()         # audited entry point -> launches of the step
        self.abi = collections.Counter()           # C ABI symbol -> calls
        self.bits_checked = self.bits_read = 0
        self.fused = []                            # (block shape, bit-identical?)
        self.gn_cache = {}
        self.inner = False                         # launches the audit itself issues (the separate form of a fused block)
        self.seconds = 0.0
        self.cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count

    # -- bookkeeping ------------------------------------------------------------------------------------------------
    def _kern(self):
        return self.ops.L().bd_conv_last_kernel().decode()

    def _rec(self, kern, pas, ratio, err_s=0.0, what=""):
        s = self.stats.setdefault((kern, pas), [0, 0.0, 0.0])
        s[0] += 1
        s[1] = max(s[1], ratio)
        s[2] = max(s[2], err_s)
        if not ratio <= 1.0:
            self.bad.append(f"{kern} {pas} {what}: worst err/tol = {ratio:.3g}")

    def _count(self, name):
        if not self.inner:
            self.calls[name] += 1

    def _check_bf16(self, kern, pas, got, before, ref, S, exact, cover, what):
        r = U.bound_ratio(got, ref, S, REL_BF16, ABS_BF16, exact)
        err_s = torch.nan_to_num((got.double() - ref).abs() / S, nan=0.0, posinf=0.0).max()
        self._rec(kern, pas, float(r.max()), float(err_s), what)
        if not _same_bits(got[~cover], before[~cover]):
            self.bad.append(f"{kern} {pas} {what}: wrote rows outside its levels")

    def _check_f32(self, kern, pas, got, ref, S, what, roundings):
        tol = min(roundings * U24, MAX_F32)
        err = (got.double() - ref).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / (tol * S))
        self._rec(kern, pas, float(r.max()), float(torch.nan_to_num(err / S, nan=0.0, posinf=0.0).max()), what)

    # -- wrappers ---------------------------------------------------------------------------------------------------
    def conv2d_fwd(self, d, x, w_packed, bias, y, add=None, flags=0, bits=None, y8=None, q_scale=1.0):
        self._count("conv2d_fwd")
        before = y.clone()
        add0 = add.clone() if add is not None else None
        self.orig["conv2d_fwd"](d, x, w_packed, bias, y, add=add, flags=flags, bits=bits, y8=y8, q_scale=q_scale)
        torch.cuda.synchronize()
        kern = self._kern()
        t0 = time.time()
        ref, S, ex = U.conv_ref_fwd(d, x, w_packed, bias, add0, flags, images=IMAGES)
        cover = _rows(d.N, d.out_pix_per_img, [(l[5], l[2] * l[3]) for l in U.desc_levels(d)], y.device)
        self._check_bf16(kern, "fwd", y, before, ref, S, ex, cover, f"Cin={d.Cin} Cout={d.Cout} R={d.R} s={d.stride} {d.Ho[0]}x{d.Wo[0]}")
        if bits is not None:                       # the gate bits of the kernel's own y
            self.bits_checked += 1
            if not torch.equal(U.decode_maskbits(bits, d.Cout), y.float() > 0):
                self.bad.append(f"{kern} fwd: bits != (y > 0) Cout={d.Cout}")
        self.seconds += time.time() - t0
        return y

    def conv2d_fwd_gnstats(self, d, x, w_packed, bias, y, part):
        self._count("conv2d_fwd_gnstats")
        before = y.clone()
        self.orig["conv2d_fwd_gnstats"](d, x, w_packed, bias, y, part)
        torch.cuda.synchronize()
        kern = self._kern() + "+gnstats"
        t0 = time.time()
        ref, S, ex = U.conv_ref_fwd(d, x, w_packed, bias, None, 0, images=IMAGES)
        cover = _rows(d.N, d.out_pix_per_img, [(l[5], l[2] * l[3]) for l in U.desc_levels(d)], y.device)
        self._check_bf16(kern, "fwd", y, before, ref, S, ex, cover, f"gnstats Cin={d.Cin}")
        self.gn_cache[y.data_ptr()] = (d, ref, S)
        self.seconds += time.time() - t0
        return y

    def groupnorm_fwd_parts(self, d, y, part, gamma, beta, eps, relu, stats, z):
        """The per-patch partial sums reach only this launch: its (mean, rstd) must be those of the UNROUNDED float64 convolution
        within 2^-14 of the group's mean |y| (mean) and 2^-14 relative (rstd): 2^-14 covers fp32 sums over <= 2^10 patch partials of
        <= 2^6 fp32 roundings each (per-patch sums of 64 pixels x 8 channels, then a fixed-order sum over a level's patches)."""
        self.orig["groupnorm_fwd_parts"](d, y, part, gamma, beta, eps, relu, stats, z)
        torch.cuda.synchronize()
        hit = self.gn_cache.pop(y.data_ptr(), None)
        if hit is None or IMAGES is not None:
            return z
        t0 = time.time()
        _, ref, _ = hit
        N, ppi = d.N, d.out_pix_per_img
        worst_m = worst_r = 0.0
        for li, (_, _, Ho, Wo, _, oo) in enumerate(U.desc_levels(d)):
            v = ref.view(N, ppi, 32, 8)[:, oo:oo + Ho * Wo].permute(0, 2, 1, 3).reshape(N, 32, -1)
            mu = v.mean(-1)
            rstd = 1.0 / torch.sqrt(v.var(-1, correction=0) + eps)
            st = stats[:, li].double()
            worst_m = max(worst_m, float(((st[..., 0] - mu).abs() / (2.0 ** -14 * v.abs().mean(-1))).max()))
            worst_r = max(worst_r, float(((st[..., 1] - rstd).abs() / (2.0 ** -14 * rstd)).max()))
        self._rec("groupnorm_fwd_parts", "stats", max(worst_m, worst_r), 0.0, "mean / rstd from the conv's partial sums")
        self.seconds += time.time() - t0
        return z

    def conv2d_dgrad(self, d, g, w_packed_t, dx, add=None, mask=None, flags=0, maskbits=None, dx8=None, q_scale=1.0):
        self._count("conv2d_dgrad")
        before = dx.clone()
        add0 = add.clone() if add is not None else None
        g0 = g.clone() if g.data_ptr() == dx.data_ptr() else g          # P7's data gradient reads and writes levels of one buffer
        self.orig["conv2d_dgrad"](d, g, w_packed_t, dx, add=add, mask=mask, flags=flags, maskbits=maskbits, dx8=dx8, q_scale=q_scale)
        torch.cuda.synchronize()
        kern = self._kern()
        t0 = time.time()
        if maskbits is not None:
            self.bits_read += 1
        ref, S, ex = U.conv_ref_dgrad(d, g0, w_packed_t, add0, mask, maskbits, flags, images=IMAGES)
        cover = _rows(d.N, d.in_pix_per_img, [(l[4], l[0] * l[1]) for l in U.desc_levels(d)], dx.device)
        self._check_bf16(kern, "dgrad", dx, before, ref, S, ex, cover,
                         f"Cin={d.Cin} Cout={d.Cout} R={d.R} s={d.stride} flags={flags} bits={maskbits is not None}")
        self.seconds += time.time() - t0
        return dx

    def conv2d_wgrad(self, d, x, g, dw, ws, row_scale=None, accumulate=False):
        self._count("conv2d_wgrad")
        dw0 = dw.clone() if accumulate else None
        self.orig["conv2d_wgrad"](d, x, g, dw, ws, row_scale=row_scale, accumulate=accumulate)
        torch.cuda.synchronize()
        kern = self._kern()
        t0 = time.time()
        rw, _ = fp32_roundings(d, kern, self.cus)
        ref, S, _, _ = U.conv_ref_wgrad(d, x, g, row_scale, dw0)
        self._check_f32(kern, "wgrad", dw, ref, S, f"Cin={d.Cin} Cout={d.Cout} R={d.R} s={d.stride}", rw)
        self._edge_probe(kern, d, x, g, ws, row_scale, False)
        self.seconds += time.time() - t0
        return dw

    def _edge_probe(self, kern, d, x, g, ws, row_scale, bias):
        """The same launch (descriptor, kernel, split plan) with g zero except at the first and the last pixel of every level of every
        image, into fresh outputs: a pixel the kernel skips at a split, patch or tail boundary costs ~1 / (2 N levels) of S here."""
        gp = torch.zeros_like(g)
        v, gv = gp.view(d.N, d.out_pix_per_img, -1), g.view(d.N, d.out_pix_per_img, -1)
        for _, _, Ho, Wo, _, oo in U.desc_levels(d):
            for p in (oo, oo + Ho * Wo - 1):
                v[:, p] = gv[:, p]
        dw = torch.full((d.Cout, d.R, d.S, d.Cin), 7.0, dtype=torch.float32, device=g.device)
        db = torch.full((d.Cout,), 7.0, dtype=torch.float32, device=g.device) if bias else None
        self.inner = True
        try:
            if bias:
                self.orig["conv2d_wgrad_bias"](d, x, gp, dw, db, ws, row_scale=row_scale)
            else:
                self.orig["conv2d_wgrad"](d, x, gp, dw, ws, row_scale=row_scale)
            torch.cuda.synchronize()
        finally:
            self.inner = False
        if self._kern() != kern:
            self.bad.append(f"{kern}: the edge probe went to {self._kern()}")
        rw, rb = fp32_roundings(d, kern, self.cus)
        ref, S, dbr, Sdb = U.conv_ref_wgrad(d, x, gp, row_scale, None, bias)
        self._check_f32(kern, "probe", dw, ref, S, f"edge probe Cin={d.Cin} Cout={d.Cout} R={d.R} s={d.stride}", rw)
        if bias:
            self._check_f32(kern, "probe", db, dbr, Sdb, f"edge probe bias Cout={d.Cout}", rb)

    def conv2d_wgrad_bias(self, d, x, g, dw, dbias, ws, row_scale=None, accumulate=False):
        self._count("conv2d_wgrad_bias")
        dw0 = dw.clone() if accumulate else None
        db0 = dbias.clone() if accumulate else None
        self.orig["conv2d_wgrad_bias"](d, x, g, dw, dbias, ws, row_scale=row_scale, accumulate=accumulate)
        torch.cuda.synchronize()
        kern = self._kern()
        t0 = time.time()
        rw, rb = fp32_roundings(d, kern, self.cus)
        ref, S, db, Sdb = U.conv_ref_wgrad(d, x, g, row_scale, dw0, True, db0)
        self._check_f32(kern, "wgrad", dw, ref, S, f"Cin={d.Cin} Cout={d.Cout} R={d.R} s={d.stride}", rw)
        self._check_f32(kern, "bias", dbias, db, Sdb, f"Cout={d.Cout}", rb)
        self._edge_probe(kern, d, x, g, ws, row_scale, True)
        self.seconds += time.time() - t0
        return dw

    def colsum_bf16(self, g, rows, Cn, out, ws, accumulate=False, geom=None):
        self._count("colsum_bf16")
        o0 = out.clone()
        self.orig["colsum_bf16"](g, rows, Cn, out, ws, accumulate=accumulate, geom=geom)
        torch.cuda.synchronize()
        if geom is None:
            sel = g[:rows, :Cn].double()
        else:
            sel = g.view(geom.N, geom.pix_per_img, -1)[:, geom.off[0]:geom.off[0] + geom.H[0] * geom.W[0], :Cn].reshape(-1, Cn).double()
        ref, S = sel.sum(0), sel.abs().sum(0)
        if accumulate:
            ref, S = ref + o0.double(), S + o0.double().abs()
        rif = max(256 // (Cn // 8), 1)
        self._check_f32("colsum_bf16", "bias", out, ref, S, f"C={Cn}", _cdiv(sel.shape[0], 1024 * rif) + rif + 32 + 32 + 2)
        return out

    def upsample2x_add_fwd(self, top, gtop, lat, glat, Cn):
        self._count("upsample2x_add_fwd")
        lat0 = lat.clone()
        self.orig["upsample2x_add_fwd"](top, gtop, lat, glat, Cn)
        torch.cuda.synchronize()
        N, H, W = gtop.N, gtop.H[0], gtop.W[0]
        t = top.view(N, gtop.pix_per_img, -1)[:, gtop.off[0]:gtop.off[0] + H * W].reshape(N, H, W, Cn).permute(0, 3, 1, 2).double()
        lv = lambda b: b.view(N, glat.pix_per_img, -1)[:, glat.off[0]:glat.off[0] + 4 * H * W].reshape(-1, Cn)
        up = TF.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)
        upa = TF.interpolate(t.abs(), scale_factor=2, mode="bilinear", align_corners=False)
        flat = lambda u: u.permute(0, 2, 3, 1).reshape(-1, Cn)
        ref = lv(lat0).double() + flat(up)
        S = lv(lat0).double().abs() + flat(upa)
        r = U.bound_ratio(lv(lat), ref, S, REL_BF16, ABS_UPS)
        self._rec("upsample2x_add_fwd", "fwd", float(r.max()), 0.0, f"{N}x{H}x{W}x{Cn}")
        cover = _rows(N, glat.pix_per_img, [(glat.off[0], 4 * H * W)], lat.device)
        if not _same_bits(lat[~cover], lat0[~cover]):
            self.bad.append("upsample2x_add_fwd wrote rows outside its level")

    def upsample2x_add_bwd(self, dlat, glat, dtop, gtop, Cn, accumulate):
        self._count("upsample2x_add_bwd")
        d0 = dtop.clone()
        self.orig["upsample2x_add_bwd"](dlat, glat, dtop, gtop, Cn, accumulate)
        torch.cuda.synchronize()
        N, H, W = gtop.N, gtop.H[0], gtop.W[0]
        g = dlat.view(N, glat.pix_per_img, -1)[:, glat.off[0]:glat.off[0] + 4 * H * W].reshape(N, 2 * H, 2 * W, Cn).permute(0, 3, 1, 2).double()
        outs = []
        for src in (g, g.abs()):
            t = torch.zeros((N, Cn, H, W), dtype=torch.float64, device=g.device, requires_grad=True)
            TF.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False).backward(src)
            outs.append(t.grad.permute(0, 2, 3, 1).reshape(-1, Cn))
        lv = lambda b: b.view(N, gtop.pix_per_img, -1)[:, gtop.off[0]:gtop.off[0] + H * W].reshape(-1, Cn)
        ref, S = outs
        if accumulate:
            ref, S = ref + lv(d0).double(), S + lv(d0).double().abs()
        r = U.bound_ratio(lv(dtop), ref, S, REL_BF16, ABS_UPS)
        self._rec("upsample2x_add_bwd", "bwd", float(r.max()), 0.0, f"{N}x{H}x{W}x{Cn} acc={accumulate}")

    def stem_pool_fwd(self, N, H, W, x_halo, w_stem, bias, y_pool):
        """bf16(maxpool3x3s2p1(relu(conv7x7s2p3(x) + shift))) in float64 over the whole batch.  Max and bf16 rounding commute, so
        |got - ref| <= max over the window of (2^-8 |ref_i| + delta_i) <= 2^-8 ref + 2^-16 max S_i."""
        self._count("stem_pool_fwd")
        self.orig["stem_pool_fwd"](N, H, W, x_halo, w_stem, bias, y_pool)
        torch.cuda.synchronize()
        t0 = time.time()
        Wm = w_stem.double().view(64, 7, 8, 4).permute(0, 3, 1, 2).reshape(64, 224)
        Ho, Wo = H // 2, W // 2
        Hq, Wq = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
        b = bias.double().view(64, 1)
        worst, worst_s = 0.0, 0.0
        for n in range(N):
            # the halo layout [H+6][W+8][4]: output (i, j) reads rows 2i .. 2i+6, columns 2j .. 2j+7 (column 0 of the 8 weighs zero)
            xi = x_halo[n].double().permute(2, 0, 1).unsqueeze(0)
            cols = TF.unfold(xi, (7, 8), stride=2)[0]
            nw = (W + 8 - 8) // 2 + 1
            v = (Wm @ cols + b).view(64, Ho, nw)[:, :, :Wo]
            s = (Wm.abs() @ cols.abs() + b.abs()).view(64, Ho, nw)[:, :, :Wo]
            ref = TF.max_pool2d(v.clamp_min(0).unsqueeze(0), 3, 2, 1)[0]
            S = TF.max_pool2d(s.unsqueeze(0), 3, 2, 1)[0]
            got = y_pool[n * Hq * Wq:(n + 1) * Hq * Wq].view(Hq, Wq, 64).permute(2, 0, 1)
            r = U.bound_ratio(got, ref, S, REL_BF16, ABS_BF16)
            worst = max(worst, float(r.max()))
            worst_s = max(worst_s, float(((got.double() - ref).abs() / S).max()))
        self._rec("stem_pool_kernel", "fwd", worst, worst_s, f"{N}x{H}x{W}")
        self.seconds += time.time() - t0

    def bottleneck_fwd(self, N, H, W, cin, cmid, cout, x, w1, b1, w2, b2, w3, b3, wd, bd, y):
        """The fused frozen block must equal, bit for bit, its three / four separate bd_conv2d_fwd launches on the same input, each of
        which is audited per element above."""
        self._count("bottleneck_fwd")
        ops = self.ops
        self.orig["bottleneck_fwd"](N, H, W, cin, cmid, cout, x, w1, b1, w2, b2, w3, b3, wd, bd, y)
        torch.cuda.synchronize()
        g = ops.single(N, H, W)
        bf = dict(dtype=torch.bfloat16, device=y.device)
        m1, m2, out = (torch.empty((g.pixels, c), **bf) for c in (cmid, cmid, cout))
        self.inner = True
        try:
            idt = x
            if wd is not None:
                idt = torch.empty((g.pixels, cout), **bf)
                ops.conv2d_fwd(ops.conv_desc(g, g, cin, cout, 1, 1, 1, 0), x, wd, bd, idt)
            ops.conv2d_fwd(ops.conv_desc(g, g, cin, cmid, 1, 1, 1, 0), x, w1, b1, m1, flags=ops.EPI_RELU)
            ops.conv2d_fwd(ops.conv_desc(g, g, cmid, cmid, 3, 3, 1, 1), m1, w2, b2, m2, flags=ops.EPI_RELU)
            ops.conv2d_fwd(ops.conv_desc(g, g, cmid, cout, 1, 1, 1, 0), m2, w3, b3, out, add=idt, flags=ops.EPI_RELU | ops.EPI_ADD_BEFORE)
        finally:
            self.inner = False
        same = _same_bits(out, y)
        self.fused.append(((N, H, W, cin, cmid, cout, wd is not None), same))
        if not same:
            self.bad.append(f"bottleneck_fwd {N}x{H}x{W} {cin}->{cout}: {int((out != y).sum())} elements differ from the separate launches")
        return y

    # -- install / remove -------------------------------------------------------------------------------------------
    def __enter__(self):
        ops = self.ops
        self.orig = {n: getattr(ops, n) for n in WRAPPED}
        for n in WRAPPED:
            setattr(ops, n, getattr(self, n))
        lib = ops.L()
        self._abi = {s: getattr(lib, s) for s in CONV_ABI}
        for s, f in self._abi.items():
            def counted(*a, _f=f, _s=s):
                if not self.inner:
                    self.abi[_s] += 1
                return _f(*a)
            setattr(lib, s, counted)
        return self

    def __exit__(self, *exc):
        for n, f in self.orig.items():
            setattr(self.ops, n, f)
        lib = self.ops.L()
        for s, f in self._abi.items():
            setattr(lib, s, f)

    def table(self, title):
        lines = [f"{title}: {sum(s[0] for s in self.stats.values())} audited launches, reference time {self.seconds:.1f} s",
                 f"  {'kernel':34s} {'pass':6s} {'launches':>8s} {'worst err/tol':>14s} {'worst err/S':>12s}"]
        for (k, p), (n, r, e) in sorted(self.stats.items()):
            lines.append(f"  {k:34s} {p:6s} {n:8d} {r:14.4f} {e:12.3e}")
        return "\n".join(lines)


# ---- the models ------------------------------------------------------------------------------------------------------------------------
def _dev(batch):
    return {k: ({kk: torch.from_numpy(vv).cuda() for kk, vv in v.items()} if isinstance(v, dict)
                else torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in batch.items()}


def _make(name):
    if name == "retinanet":
        from basedet_amd.models import RetinaNet
        from tests.test_model_gpu import _setup
        cfg, params, batch = _setup("resnet50", B, SIZE)
        return (lambda: RetinaNet(cfg, params=params)), batch
    from basedet_amd.configs import FCOSConfig
    from basedet_amd.models import FCOS, params as P
    from basedet_amd.utils import DummyLoader
    cfg = FCOSConfig()
    cfg.MODEL.BATCHSIZE = B
    params = P.init_fcos_params(cfg, seed=0, residual_gamma=0.25)
    batch = next(DummyLoader(B, SIZE, seed=0))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    return (lambda: FCOS(cfg, params=params)), batch


# what the RetinaNet-R50 step dispatches (tests/test_conv_gpu.py pins the same names for its descriptors)
PINNED = {("conv3x3_pp_kernel", "fwd"), ("conv3x3_pp_kernel", "dgrad"), ("conv_wgrad3x3_ring_kernel", "wgrad"),
          ("conv1x1_ring_kernel", "fwd"), ("conv1x1_ring_kernel", "dgrad"), ("conv_wgrad1x1_ring_kernel", "wgrad"),
          ("conv_igemm_kernel<32>", "fwd"), ("conv_igemm_kernel<32>", "dgrad"), ("conv_wgrad3x3_kernel", "wgrad"),
          ("conv_wgrad1x1_kernel", "wgrad")}


@pytest.fixture(scope="module", params=["retinanet", "fcos"])
def audited_step(request):
    from basedet_amd import ops
    make, batch = _make(request.param)
    # the same step without wrappers first: the audited step must leave the gradient arena bit for bit as it is
    model = make()
    model.async_wgrad = False
    model(_dev(batch))
    model.backward()
    torch.cuda.synchronize()
    arena_plain = model.arena.g.clone()
    del model
    torch.cuda.empty_cache()
    model = make()
    model.async_wgrad = False
    t0 = time.time()
    with Audit(ops) as au:
        model(_dev(batch))
        model.backward()
        torch.cuda.synchronize()
    dt = time.time() - t0
    print("\n" + au.table(f"{request.param} B={B} {SIZE[0]}x{SIZE[1]} training step ({dt:.1f} s)"))
    yield request.param, model, au, arena_plain
    del model
    torch.cuda.empty_cache()


def test_every_element_within_bound(audited_step):
    name, model, au, _ = audited_step
    assert not au.bad, "\n".join(au.bad[:20])
    assert au.stats


def test_dispatched_kernels_and_launch_counts(audited_step):
    """Every conv launch went through an audited wrapper (C ABI calls == audited calls), and their number follows the model's own layer
    list: one forward per layer outside a fused block, one weight gradient per trainable layer."""
    name, model, au, _ = audited_step
    abi = au.abi
    for s in ("bd_conv2d_wgrad_queued", "bd_conv2d_fwd_fp8_ex", "bd_conv2d_dgrad_fp8", "bd_conv1x1_fp8", "bd_conv2d_wgrad_fp8",
              "bd_conv1x1_thin_fwd", "bd_conv1x1_thin_bwd", "bd_stem_conv7x7_fwd"):
        assert abi[s] == 0, (s, abi[s])                   # none of these is on the bf16 RetinaNet / FCOS step with the default config
    c = au.calls
    assert abi["bd_conv2d_fwd"] + abi["bd_conv2d_fwd_bits"] + abi["bd_conv2d_fwd_ex"] == c["conv2d_fwd"]
    assert abi["bd_conv2d_dgrad"] + abi["bd_conv2d_dgrad_bits"] + abi["bd_conv2d_dgrad_ex"] == c["conv2d_dgrad"]
    assert abi["bd_conv2d_wgrad"] + abi["bd_conv2d_wgrad_bias"] == c["conv2d_wgrad"] + c["conv2d_wgrad_bias"]
    for n in ("stem_pool_fwd", "bottleneck_fwd", "conv2d_fwd_gnstats", "colsum_bf16", "upsample2x_add_fwd", "upsample2x_add_bwd"):
        assert abi["bd_" + n] == c[n], n
    convs = list(model.convs.values())
    fused = [blk for blk, b in zip(model.blocks, model._cur.blk) if getattr(b, "fused", False)]
    in_fused = sum(len(blk["convs"]) + (blk["ds"] is not None) for blk in fused)
    assert c["bottleneck_fwd"] == len(fused) and c["stem_pool_fwd"] == 1
    assert c["conv2d_fwd"] + c["conv2d_fwd_gnstats"] == len(convs) - in_fused
    assert c["conv2d_wgrad"] + c["conv2d_wgrad_bias"] == sum(1 for cv in convs if cv.trainable)
    assert model.wgrads.queue is None                      # WGRAD_QUEUE = "layer": no deferred reduce on this step
    if name == "retinanet":
        assert c["upsample2x_add_fwd"] == 2 and c["upsample2x_add_bwd"] == 2
        audited = set(au.stats)
        missing = {k for k in PINNED if k not in audited}
        assert not missing, missing
        dense = {k for (k, p) in au.stats if p == "fwd" and k in ("conv1x1_dense_kernel", "conv1x1_gemm_kernel")}
        assert dense, sorted(au.stats)
    else:
        assert c["conv2d_fwd_gnstats"] == 8 and ("groupnorm_fwd_parts", "stats") in au.stats


def test_relu_bits_and_fused_blocks(audited_step):
    """Forward launches that wrote gate bits wrote (y > 0) of their own y; the data gradients that read them were audited with the gate
    decoded from the bits; each fused frozen res2 block equals its separate launches bit for bit at batch 16."""
    name, model, au, _ = audited_step
    assert au.bits_checked > 0 and au.bits_read > 0, (au.bits_checked, au.bits_read)
    assert len(au.fused) == 3 and all(same for _, same in au.fused), au.fused


def test_audit_leaves_the_step_unchanged(audited_step):
    name, model, au, arena_plain = audited_step
    assert torch.equal(model.arena.g, arena_plain), int((model.arena.g != arena_plain).sum())


def test_inference_forward_audited():
    """The inference forward (one image, RetinaNet-R50 at 800 x 1344) through the same wrappers."""
    from basedet_amd import ops
    make, batch = _make("retinanet")
    one = {k: ({kk: vv[:1] for kk, vv in v.items()} if isinstance(v, dict) else v[:1]) for k, v in batch.items()}
    model = make().eval()
    model.async_wgrad = False
    with Audit(ops) as au:
        model(one)
        torch.cuda.synchronize()
    print("\n" + au.table("retinanet inference 1x800x1344"))
    assert not au.bad, "\n".join(au.bad[:20])
    assert au.calls["conv2d_dgrad"] == 0 and au.calls["conv2d_fwd"] > 0 and au.calls["stem_pool_fwd"] == 1


def test_groupnorm_fwd_bwd_on_the_bench_pyramid():
    """bd_groupnorm_fwd / bd_groupnorm_bwd (GroupNorm(32, 256) + ReLU) over 16 images of the bench pyramid (100x168 .. 7x11) against
    float64 from the same bf16 inputs.  S_z = |gamma| rstd (|y| + |mean|) + |beta|; the statistics are fp32 sums over <= 134 400
    elements in a two-stage fixed-order reduce (128-pixel slots), so the relative error of mean and rstd stays below 2^-14 (< 2^10
    roundings): z within 2^-8 |z| + 2^-14 S_z.  The backward's gate is z > 0 of the forward's own output (the kernel recomputes it with
    the forward's arithmetic); dy within 2^-8 |dy| + 2^-14 S_dy, dgamma / dbeta (fp32 sums over the batch) within 2^-14 S."""
    from basedet_amd import ops
    from basedet_amd.models.fcos import GN_EPS
    gen = torch.Generator().manual_seed(21)
    C, G = 256, 32
    pyr = ops.Geom(B, [100, 50, 25, 13, 7], [168, 84, 42, 21, 11])
    y = (torch.randn(pyr.pixels, C, generator=gen) * 2 + 0.3).to(torch.bfloat16).cuda()
    dz = torch.randn(pyr.pixels, C, generator=gen).to(torch.bfloat16).cuda()
    gamma = (torch.rand(C, generator=gen) + 0.5).cuda()
    beta = (torch.randn(C, generator=gen) * 0.2).cuda()
    stats = torch.empty((B, pyr.nlev, G, 2), dtype=torch.float32, device="cuda")
    z = torch.empty_like(y)
    dy = torch.empty_like(y)
    dgamma = torch.full((C,), 0.5, dtype=torch.float32, device="cuda")
    dbeta = torch.full((C,), -0.5, dtype=torch.float32, device="cuda")
    ws = torch.empty((ops.groupnorm_workspace_bytes(B, pyr.nlev, C, pyr.pix_per_img) // 4 + 16,), dtype=torch.float32, device="cuda")
    ops.groupnorm_fwd(y, gamma, beta, pyr, C, GN_EPS, True, stats, z, ws)
    ops.groupnorm_bwd(dz, y, gamma, beta, stats, pyr, C, True, dy, dgamma, dbeta, ws, accumulate=True)
    torch.cuda.synchronize()
    g64, b64 = gamma.double(), beta.double()
    worst = collections.defaultdict(float)
    dg, sdg = 0.5 + torch.zeros(C, dtype=torch.float64, device="cuda"), 0.5 + torch.zeros(C, dtype=torch.float64, device="cuda")
    db, sdb = -0.5 + torch.zeros_like(dg), 0.5 + torch.zeros_like(dg)
    for li in range(pyr.nlev):
        n_px = pyr.H[li] * pyr.W[li]
        lv = lambda t: t.view(B, pyr.pix_per_img, C)[:, pyr.off[li]:pyr.off[li] + n_px]
        yv = lv(y).double().view(B, n_px, G, 8)
        mu = yv.mean((1, 3), keepdim=True)
        rstd = 1.0 / torch.sqrt(yv.var((1, 3), correction=0, keepdim=True) + GN_EPS)
        xh = (yv - mu) * rstd
        gm, bm = g64.view(1, 1, G, 8), b64.view(1, 1, G, 8)
        pre = xh * gm + bm
        zr = pre.clamp_min(0)
        Sz = gm.abs() * rstd * (yv.abs() + mu.abs()) + bm.abs()
        zg = lv(z).view(B, n_px, G, 8)
        worst["z"] = max(worst["z"], float(U.bound_ratio(zg, zr, Sz, REL_BF16, 2.0 ** -14).max()))
        st = stats[:, li].double()
        worst["mean"] = max(worst["mean"], float(((st[..., 0] - mu.view(B, G)).abs() / (2.0 ** -14 * yv.abs().mean((1, 3)))).max()))
        worst["rstd"] = max(worst["rstd"], float(((st[..., 1] - rstd.view(B, G)).abs() / (2.0 ** -14 * rstd.view(B, G))).max()))
        gate = zg.float() > 0
        d = lv(dz).double().view(B, n_px, G, 8) * gate
        dxh = d * gm
        m1 = dxh.mean((1, 3), keepdim=True)
        m2 = (dxh * xh).mean((1, 3), keepdim=True)
        ref = rstd * (dxh - m1 - xh * m2)
        Sdy = rstd * (dxh.abs() + dxh.abs().mean((1, 3), keepdim=True) + xh.abs() * (dxh * xh).abs().mean((1, 3), keepdim=True))
        worst["dy"] = max(worst["dy"], float(U.bound_ratio(lv(dy).view(B, n_px, G, 8), ref, Sdy, REL_BF16, 2.0 ** -14).max()))
        dg = dg + (d * xh).sum((0, 1)).reshape(C)
        sdg = sdg + (d * xh).abs().sum((0, 1)).reshape(C)
        db = db + d.sum((0, 1)).reshape(C)
        sdb = sdb + d.abs().sum((0, 1)).reshape(C)
    worst["dgamma"] = float(((dgamma.double() - dg).abs() / (2.0 ** -14 * sdg)).max())
    worst["dbeta"] = float(((dbeta.double() - db).abs() / (2.0 ** -14 * sdb)).max())
    print("\ngroupnorm 16 x pyramid x 256, worst err/tol:", dict(worst))
    for k, v in worst.items():
        assert v <= 1.0, (k, v)
