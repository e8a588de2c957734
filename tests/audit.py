"""The audit machinery shared by tests/test_conv_audit_gpu.py and tests/test_frcnn_audit_gpu.py (a plain helper module: no test, no fixture).
Wrappers around the entry points of basedet_amd.ops that check every element of every launch of a training step against float64, and
the bounds they use.  Protocol (Audit): clone what the launch updates in place, call the kernel, synchronise, read bd_conv_last_kernel(),
recompute the launch from ITS OWN operands (tests/util.py), check every element, leave the kernel's output in place.  Rows a launch must
not touch come back bit for bit.  S is always the same operation applied to |operands|; u = 2^-24, the largest relative error of one fp32
rounding.

Bounds (derived, not tuned):
  * bf16 outputs of a K-long sum (forward, data gradient), abs_bf16: the kernel rounds an fp32 value v to bf16, |bf16(v) - v| <= 2^-9 |v|,
    and |v - ref| <= delta, the fp32 accumulation error: tol = 2^-8 |ref| + abs S.  Every partial sum is at most S, so one fp32 rounding
    costs at most u S.  A kernel sums `per_step` exact bf16 products in one MFMA step and adds the result to its accumulator: two
    roundings per step, taps x ceil(K / per_step) steps, plus three epilogue adds (bias, residual, the merge of two K halves):
    abs = (2 steps + 3) u, never tighter than 2^-16 (the merged audit's constant).  per_step comes from MFMA_K (32 for every bf16 forward /
    data-gradient kernel of the library: v_mfma_f32_16x16x32_bf16); a kernel missing from that table is counted with 16, which can only
    loosen, and is recorded in Audit.unknown -- both audit files assert that list is empty.  abs is 2^-16 while steps <= 126 (K <= 4 032
    for a 1x1, Cin <= 448 for a 3x3); res5's 3x3 512 -> 512 convolutions (K = 4 608, forward and data gradient, in every R50 / R101 step)
    get 291 u = 1.73e-5, and rcnn.fc1 (K = 12 544) 787 u = 4.7e-5.
  * K-edge probe (_k_probe): where K > K_PROBE_MIN = 4 096 that term approaches the weight S / K of one product, so the launch (forward
    or data gradient) is repeated on the same descriptor with the K-side operand kept only in the first and last column of every
    256-column block (probe_columns) and zero elsewhere: a dropped column there costs S / (K / 128).
  * elements that are exactly representable (closed ReLU / mask gates, pixels a sparse data gradient must not touch, empty RoI slots,
    padding rows and columns) are compared for equality.
  * fp32 outputs (weight and bias gradients, column sums), fp32_roundings: a bound per launch from the kernel's own split plan
    (conv_wgrad3x3_ring.hip, conv_wgrad3x3.hip, conv_wgrad1x1_ring.hip, conv_wgrad1x1.hip, the column-sum pass of image_ops.hip).  A
    workgroup accumulates its pixel range in fp32 MFMA accumulators, two roundings per MFMA step (one per step is not enough: the
    nearly one-signed focal gradients of a 720-channel bias show 1.0e-4 S where 1 224 steps + 10 partials would allow 7.4e-5 S); the
    fixed-order reduce adds `splits` partials, the row scale and an accumulate add one rounding each: tol = roundings x u S, capped at
    MAX_F32 = 2^-12 S.  The column-sum pass is plain adds: rows per thread + rows in flight + 1 024 / 32 + 32 partials + levels.  A kernel
    outside WGRAD_KNOWN takes the one-chain row (every pixel in one chain) and is recorded in Audit.unknown.
  * edge probe (_edge_probe): a per-element bound cannot see a weight-gradient kernel drop a few of 10^5 .. 10^6 pixels, so every
    weight-gradient launch is repeated with g kept only at the first and last pixel of every level of every image.
  * thin 1x1 backward, thin_bwd_roundings: dx is 16 exact products in one MFMA step (2^-16 S); a dW / db element is ceil(groups / grid)
    FMAs per lane (one per 16-pixel group the workgroup walks), four shuffle adds over the pixel lanes, ceil(grid / 8) adds per reduce
    lane and three adds over the eight reduce lanes.
  * RoIAlign, roi_weight_err: see its docstring (nine fp32 roundings on the way to a sample coordinate) and Audit.roi_align_fwd /
    _roi_bwd_check for the sums.
  * upsample2x_add: exact weights 0.75 / 0.25, <= 16 products and one add: 2^-8 |ref| + 2^-19 S.
  * stem_pool_fwd and conv2d_fwd_gnstats use the constant ABS_BF16 = 2^-16 directly: their K is fixed (7 x 8 x 4 = 224 for the stem,
    9 x 256 = 2 304 for the GroupNorm towers, which take only 256 -> 256 3x3 layers), where abs_bf16 gives 2^-16 as well.
"""
import collections
import math
import time

import torch
import torch.nn.functional as TF

from tests import util as U

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


WGRAD_KNOWN = ("conv_wgrad3x3_ring_kernel", "conv_wgrad3x3_kernel", "conv_wgrad1x1_ring_kernel", "conv_wgrad1x1_kernel")


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

# bf16 products one MFMA step of a forward / data-gradient kernel sums (v_mfma_f32_16x16x32_bf16 in every kernel listed; a kernel that is
# not listed is counted with 16: never fewer steps than it takes)
MFMA_K = {k: 32 for k in ("conv1x1_ring_kernel", "conv1x1_dense_kernel", "conv1x1_big_kernel", "conv3x3_pp_kernel", "conv3x3_pp128_kernel",
                          "conv3x3_patch_kernel", "conv_igemm_kernel<32>", "conv_igemm_kernel<64>", "conv1x1_thin_fwd_kernel")}
K_PROBE_MIN = 4096     # a K loop longer than this is repeated with the K-edge probe


def abs_bf16(K, taps=1, per_step=32):
    """The absolute term (in units of S) of a bf16 output that is an fp32 sum of `taps` x K products: two roundings of at most 2^-24 S per
    MFMA step (the step's own sum and its add to the accumulator), three epilogue adds (bias, residual, the merge of two K halves), never
    tighter than 2^-16."""
    return max(ABS_BF16, (2 * taps * _cdiv(K, per_step) + 3) * U24)


def thin_bwd_roundings(M, cus):
    """fp32 roundings of one dW / db element of conv1x1_thin_bwd_kernel + conv1x1_thin_reduce_kernel: a lane adds one product per group of
    16 pixels its workgroup walks (ceil(groups / grid) FMAs), four shuffle adds over the 16 pixel lanes, ceil(grid / 8) adds per reduce
    lane and three adds over the eight reduce lanes."""
    groups = _cdiv(M, 16)
    grid = min(groups, cus)
    return _cdiv(groups, grid) + 4 + _cdiv(grid, 8) + 3


def probe_columns(K, block=256):
    """bool (K,): the first and the last column of every `block`-column block (fc1: the first and last channel of each pooled position)."""
    c = torch.arange(K) % block
    return (c == 0) | (c == block - 1)


def roi_coord_err(H, W):
    """Bound on the error of one fp32 sample coordinate of roi_align_fwd_kernel, x = (sw + pw * bw) + (i + 0.5) * bw / S with
    sw = x1 s - 0.5, bw = ((x2 s - 0.5) - sw) / PW (s a power of two: exact).  Every value is at most P = max(H, W) + 1 in magnitude, so a
    rounding costs at most u P.  sw: 1.  bw: the two ends and their difference, 3 u P / PW, and the division, u |bw|; bw enters x with a
    factor below PW: 3 + 1.  pw * bw, the first sum, (i + 0.5) * bw and the last sum: 1 each (/ S is exact for S = 2).  Nine in all."""
    return 9 * U24 * (max(H, W) + 1)


def roi_weight_err(H, W):
    """Bound on the error of one bilinear weight against weights from float64 coordinates: a weight is a product of a row and a column
    term, each off by at most roi_coord_err (l = y - floor(y) is exact, 1 - l one rounding) and the product one more:
    2 roi_coord_err + 3 u."""
    return 2 * roi_coord_err(H, W) + 3 * U24


IMAGES = None          # None: every image of the batch in the forward / data-gradient references (else a list of image indices)

# entry points of basedet_amd.ops the wrappers replace, and the C ABI symbols that must only be reached through them
WRAPPED = ("conv2d_fwd", "conv2d_dgrad", "conv2d_wgrad", "conv2d_wgrad_bias", "colsum_bf16", "upsample2x_add_fwd", "upsample2x_add_bwd",
           "stem_pool_fwd", "bottleneck_fwd", "conv2d_fwd_gnstats", "groupnorm_fwd_parts",
           "conv1x1_thin_fwd", "conv1x1_thin_bwd", "roi_align_fwd", "roi_align_bwd_bf16", "roi_align_bwd", "f32_to_bf16", "subsample2x_fwd",
           "subsample2x_bwd_add", "rcnn_loss_fwd_bwd")
CONV_ABI = ("bd_conv2d_fwd", "bd_conv2d_dgrad", "bd_conv2d_fwd_bits", "bd_conv2d_fwd_ex", "bd_conv2d_dgrad_ex", "bd_conv2d_dgrad_bits",
            "bd_conv2d_wgrad", "bd_conv2d_wgrad_bias", "bd_conv2d_wgrad_queued", "bd_conv2d_fwd_fp8_ex", "bd_conv2d_dgrad_fp8",
            "bd_conv1x1_fp8", "bd_conv2d_wgrad_fp8", "bd_conv1x1_thin_fwd", "bd_conv1x1_thin_bwd", "bd_stem_conv7x7_fwd", "bd_stem_pool_fwd",
            "bd_bottleneck_fwd", "bd_conv2d_fwd_gnstats", "bd_colsum_bf16", "bd_upsample2x_add_fwd", "bd_upsample2x_add_bwd",
            "bd_roi_align_fwd", "bd_roi_align_bwd_bf16", "bd_roi_align_bwd", "bd_f32_to_bf16", "bd_f32_to_bf16_add", "bd_subsample2x_fwd",
            "bd_subsample2x_bwd_add", "bd_rcnn_loss_fwd_bwd")


def is_launch(symbol):
    """True for the C ABI symbols that launch device work (not the size / capability queries, handles, host staging or communication)."""
    return not (symbol.endswith(("_bytes", "_supported", "_blocks", "_pending", "_create", "_destroy", "_threads", "_string", "_version",
                                 "_last_kernel")) or symbol.startswith(("bd_comm_", "bd_h2d_", "bd_probe_")))


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
        self.reached = collections.Counter()       # every C ABI symbol called while the audit is installed (the audit's own launches excluded)
        self.unknown = []                          # launches that fell into a table's unknown-kernel row
        self.dispatch = {}                         # (pass, Cin, Cout, R, rows of level 0) -> kernel
        self.thin_geom = None                      # Geom of the pyramid the thin 1x1 layer runs over (its edge probe needs the levels)
        self.ambiguous = self.rois_seen = 0        # RoIs whose pyramid level differs between the float64 and the float32 evaluation

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

    def _abs(self, d, kern, dgrad):
        if kern not in MFMA_K:
            self.unknown.append((kern, "dgrad" if dgrad else "fwd"))
        return abs_bf16(d.Cout if dgrad else d.Cin, d.R * d.S, MFMA_K.get(kern, 16))

    def _note(self, pas, d, kern):
        self.dispatch[(pas, d.Cin, d.Cout, d.R, d.N * d.Ho[0] * d.Wo[0], d.nseg)] = kern

    def _finite(self, kern, pas, got, what):
        """bound_ratio gives 0 where the REFERENCE is NaN (rows it does not cover); an output that must be covered everywhere is checked
        for NaN / inf here."""
        if not bool(torch.isfinite(got.float()).all()):
            self.bad.append(f"{kern} {pas} {what}: non-finite output")

    def _check_bf16(self, kern, pas, got, before, ref, S, exact, cover, what, abs_s=ABS_BF16):
        r = U.bound_ratio(got, ref, S, REL_BF16, abs_s, exact)
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
        self._check_bf16(kern, "fwd", y, before, ref, S, ex, cover, f"Cin={d.Cin} Cout={d.Cout} R={d.R} s={d.stride} {d.Ho[0]}x{d.Wo[0]}",
                         self._abs(d, kern, False))
        self._note("fwd", d, kern)
        if d.Cin * d.R * d.S > K_PROBE_MIN and not self.inner:
            self._k_probe(kern, d, x, w_packed, bias, add0, flags, y)
        if bits is not None:                       # the gate bits of the kernel's own y
            self.bits_checked += 1
            if not torch.equal(U.decode_maskbits(bits, d.Cout), y.float() > 0):
                self.bad.append(f"{kern} fwd: bits != (y > 0) Cout={d.Cout}")
        self.seconds += time.time() - t0
        return y

    def _k_probe(self, kern, d, x, w_packed, bias, add, flags, y):
        """The same forward launch (descriptor, kernel) with the input kept only in the first and last column of every 256-column block
        and zero elsewhere, into a fresh output: the K-derived bound of a long K loop comes close to the weight of one product, S / K; here
        a column the kernel drops at a block boundary costs about 1 / 98 of S, under the same formula."""
        keep = probe_columns(d.Cin).to(x.device)
        xp = torch.where(keep.view(1, -1), x, torch.zeros_like(x))
        y2 = torch.full_like(y, 7.0)
        self.inner = True
        try:
            self.orig["conv2d_fwd"](d, xp, w_packed, bias, y2, add=add, flags=flags)
            torch.cuda.synchronize()
        finally:
            self.inner = False
        if self._kern() != kern:
            self.bad.append(f"{kern}: the K-edge probe went to {self._kern()}")
        ref, S, ex = U.conv_ref_fwd(d, xp, w_packed, bias, add, flags, images=IMAGES)
        cover = _rows(d.N, d.out_pix_per_img, [(l[5], l[2] * l[3]) for l in U.desc_levels(d)], y.device)
        self._check_bf16(kern, "kprobe", y2, torch.full_like(y, 7.0), ref, S, ex, cover, f"K-edge probe Cin={d.Cin} Cout={d.Cout}", self._abs(d, kern, False))

    def _k_probe_dgrad(self, kern, d, g, w_packed_t, add, aliased, mask, maskbits, flags, dx):
        """The K-edge probe of a data gradient: K runs over Cout, so g is kept only in the first and last column of every 256-column block."""
        keep = probe_columns(d.Cout).to(g.device)
        gp = torch.where(keep.view(1, -1), g, torch.zeros_like(g))
        dx2 = add.clone() if aliased else torch.full_like(dx, 7.0)                 # (an accumulating launch reads its own output buffer)
        add_arg = dx2 if aliased else add
        before = dx2.clone()
        self.inner = True
        try:
            self.orig["conv2d_dgrad"](d, gp, w_packed_t, dx2, add=add_arg, mask=mask, flags=flags, maskbits=maskbits)
            torch.cuda.synchronize()
        finally:
            self.inner = False
        if self._kern() != kern:
            self.bad.append(f"{kern}: the K-edge probe went to {self._kern()}")
        ref, S, ex = U.conv_ref_dgrad(d, gp, w_packed_t, add, mask, maskbits, flags, images=IMAGES)
        cover = _rows(d.N, d.in_pix_per_img, [(l[4], l[0] * l[1]) for l in U.desc_levels(d)], dx.device)
        self._check_bf16(kern, "kprobe", dx2, before, ref, S, ex, cover, f"K-edge probe dgrad Cin={d.Cin} Cout={d.Cout} R={d.R}", self._abs(d, kern, True))

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
                         f"Cin={d.Cin} Cout={d.Cout} R={d.R} s={d.stride} flags={flags} bits={maskbits is not None}", self._abs(d, kern, True))
        self._note("dgrad", d, kern)
        if d.Cout * d.R * d.S > K_PROBE_MIN and not self.inner:
            self._k_probe_dgrad(kern, d, g0, w_packed_t, add0, add is not None and add.data_ptr() == dx.data_ptr(), mask, maskbits, flags, dx)
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
        self._note_wgrad(d, kern)
        ref, S, _, _ = U.conv_ref_wgrad(d, x, g, row_scale, dw0)
        self._check_f32(kern, "wgrad", dw, ref, S, f"Cin={d.Cin} Cout={d.Cout} R={d.R} s={d.stride}", rw)
        self._edge_probe(kern, d, x, g, ws, row_scale, False)
        self.seconds += time.time() - t0
        return dw

    def _note_wgrad(self, d, kern):
        if kern not in WGRAD_KNOWN:
            self.unknown.append((kern, "wgrad"))
        self._note("wgrad", d, kern)

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
        self._note_wgrad(d, kern)
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

    # -- the launches only the Faster R-CNN step makes ------------------------------------------------------------------
    def _ratio(self, kern, pas, got, ref, tol, exact, what, S=None):
        """err / tol per element with an explicit tolerance tensor; `exact` elements must equal the reference."""
        g = got.double()
        err = (g - ref).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / tol)
        if exact is not None:
            r = torch.where(exact, torch.where(g == ref, torch.zeros_like(r), torch.full_like(r, float("inf"))), r)
        r = torch.nan_to_num(r, nan=float("inf"), posinf=float("inf"))
        es = float(torch.nan_to_num(err / S, nan=0.0, posinf=0.0).max()) if S is not None else 0.0
        self._rec(kern, pas, float(r.max()) if r.numel() else 0.0, es, what)
        return r

    def conv1x1_thin_fwd(self, x, w, bias, M, Cin, Cout, y):
        self._count("conv1x1_thin_fwd")
        before = y.clone()
        self.orig["conv1x1_thin_fwd"](x, w, bias, M, Cin, Cout, y)
        torch.cuda.synchronize()
        kern = self._kern()
        t0 = time.time()
        ref, S = U.thin_ref_fwd(x[:M], w, bias)
        cover = torch.zeros(y.shape[0], dtype=torch.bool, device=y.device)
        cover[:M] = True
        self._check_bf16(kern, "fwd", y[:M], before[:M], ref, S, None, cover[:M], f"thin M={M}", abs_bf16(Cin, 1, MFMA_K.get(kern, 16)))
        self._finite(kern, "fwd", y[:M], "thin")
        if kern not in MFMA_K:
            self.unknown.append((kern, "fwd"))
        if not _same_bits(y[M:], before[M:]):
            self.bad.append(f"{kern} fwd: wrote rows behind M")
        self.seconds += time.time() - t0

    def _check_thin_grads(self, kern, pas, M, dw, db, ref_w, S_w, ref_b, S_b, real):
        n = thin_bwd_roundings(M, self.cus)
        self._check_f32(kern, pas, dw.view(ref_w.shape), ref_w, S_w, f"thin dW M={M}", n)
        self._check_f32(kern, pas, db, ref_b, S_b, f"thin db M={M}", n)
        if float(dw.view(ref_w.shape)[real:].abs().max()) != 0.0 or float(db[real:].abs().max()) != 0.0:
            self.bad.append(f"{kern} {pas}: padding rows of dW / db are not zero")

    def conv1x1_thin_bwd(self, x, g, w, M, Cin, Cout, dx, dw, dbias, cout_real, ws):
        """dx: 16 exact bf16 products in one MFMA step: 2^-8 |ref| + 2^-16 S, exact zeros where the gate is closed.  dW / db: fp32 sums whose
        rounding count follows the kernel's plan (thin_bwd_roundings).  Then the edge probe: the same launch with g kept only at the first
        and last pixel of every level of every image (a fixed pattern where g is zero there)."""
        self._count("conv1x1_thin_bwd")
        before = dx.clone()
        self.orig["conv1x1_thin_bwd"](x, g, w, M, Cin, Cout, dx, dw, dbias, cout_real, ws)
        torch.cuda.synchronize()
        kern = self._kern()
        t0 = time.time()
        rdx, sdx, ex, rw, sw, rb, sb = U.thin_ref_bwd(x[:M], g[:M], w, cout_real)
        cover = torch.ones(M, dtype=torch.bool, device=dx.device)
        self._check_bf16(kern, "dgrad", dx[:M], before[:M], rdx, sdx, ex, cover, f"thin M={M}", ABS_BF16)
        self._finite(kern, "dgrad", dx[:M], "thin")
        if not _same_bits(dx[M:], before[M:]):
            self.bad.append(f"{kern} dgrad: wrote rows behind M")
        del rdx, sdx, ex
        self._check_thin_grads(kern, "wgrad", M, dw, dbias, rw, sw, rb, sb, cout_real)
        # edge probe
        geom = self.thin_geom if self.thin_geom is not None and self.thin_geom.pixels == M else None
        levels = [(0, M)] if geom is None else [(geom.off[i], geom.H[i] * geom.W[i]) for i in range(geom.nlev)]
        N, ppi = (1, M) if geom is None else (geom.N, geom.pix_per_img)
        gp = torch.zeros_like(g)
        v, gv = gp[:M].view(N, ppi, -1), g[:M].view(N, ppi, -1)
        # (the RPN loss leaves a gradient at the 256 sampled anchors of an image only: where the kept row of g is all zero the probe puts a
        # fixed bf16 pattern there, +-2^-6 (1 + o % 3) in the real output channels -- or it would sum nothing)
        o = torch.arange(Cout, device=g.device)
        pat = (((1 + o % 3) * (1 - 2 * (o % 2))).to(torch.float32) * 2.0 ** -6 * (o < cout_real)).to(g.dtype)
        for off, cnt in levels:
            for q in (off, off + cnt - 1):
                row = gv[:, q]
                v[:, q] = torch.where((row != 0).any(1, keepdim=True), row, pat.view(1, -1).expand_as(row))
        dx2 = torch.full_like(dx, 7.0)
        dw2 = torch.full_like(dw, 7.0)
        db2 = torch.full_like(dbias, 7.0)
        self.inner = True
        try:
            self.orig["conv1x1_thin_bwd"](x, gp, w, M, Cin, Cout, dx2, dw2, db2, cout_real, ws)
            torch.cuda.synchronize()
        finally:
            self.inner = False
        if self._kern() != kern:
            self.bad.append(f"{kern}: the edge probe went to {self._kern()}")
        rdx, sdx, ex, rw, sw, rb, sb = U.thin_ref_bwd(x[:M], gp[:M], w, cout_real)
        self._check_bf16(kern, "probe", dx2[:M], dx2[:M], rdx, sdx, ex, cover, f"thin edge probe dx M={M}", ABS_BF16)
        self._finite(kern, "probe", dx2[:M], "thin dx")
        del dx2, rdx, sdx, ex
        self._check_thin_grads(kern, "probe", M, dw2, db2, rw, sw, rb, sb, cout_real)
        self.seconds += time.time() - t0

    def _roi_levels(self, rois, labels, strides, nlev):
        l64 = U.roi_levels(rois, strides[:nlev], torch.float64)
        l32 = U.roi_levels(rois, strides[:nlev], torch.float32)
        valid = torch.ones_like(l64, dtype=torch.bool) if labels is None else labels >= 0
        amb = (l64 != l32) & valid
        if not self.inner:
            self.ambiguous += int(amb.sum())
            self.rois_seen += int(valid.sum())
        return l64, l32, amb

    def roi_align_fwd(self, feat, geom, nlev, strides, Cn, rois, labels, rois_per_img, pool, sample_points, out):
        """tol = 2^-8 |ref| (the bf16 rounding) + 34 x 2^-24 S (16 products, 16 adds, the 1 / S^2 scale, all below S) + roi_weight_err(level)
        x F (the 16 bilinear weights come from fp32 sample coordinates; F = the unweighted |feat| over each sample's four corners, or over
        the 4 x 4 pixels around its cell where the coordinate is within roi_coord_err of a cell edge and may land in the next cell).  Empty slots are
        exact zeros.  A RoI whose level differs between float64 and float32 may match either."""
        self._count("roi_align_fwd")
        before = out.clone()
        self.orig["roi_align_fwd"](feat, geom, nlev, strides, Cn, rois, labels, rois_per_img, pool, sample_points, out)
        torch.cuda.synchronize()
        t0 = time.time()
        l64, l32, amb = self._roi_levels(rois, labels, strides, nlev)
        R = rois.shape[0]
        if not _same_bits(out.view(-1)[R * pool[0] * pool[1] * Cn:], before.view(-1)[R * pool[0] * pool[1] * Cn:]):
            self.bad.append("roi_align_fwd wrote behind its last RoI")
        del before
        out = out.view(-1)[:R * pool[0] * pool[1] * Cn]
        ratio = None
        for lv in ((l64,) if not bool(amb.any()) else (l64, l32)):
            ref, S, F, ex = U.roi_align_ref_fwd(feat, geom, nlev, strides, Cn, rois, labels, rois_per_img, pool, sample_points, lv,
                                                edge_eps=[roi_coord_err(geom.H[l], geom.W[l]) for l in range(nlev)])
            werr = torch.tensor([roi_weight_err(geom.H[l], geom.W[l]) for l in range(nlev)], dtype=torch.float64, device=feat.device)[lv]
            tol = REL_BF16 * ref.abs() + 34 * U24 * S + werr.view(R, 1) * F
            g = out.view(R, -1).double()
            err = (g - ref).abs()
            r = torch.where(err == 0, torch.zeros_like(err), err / tol)
            r = torch.where(ex, torch.where(g == 0, torch.zeros_like(r), torch.full_like(r, float("inf"))), r)
            r = torch.nan_to_num(r, nan=float("inf"), posinf=float("inf"))
            if ratio is None:
                ratio, es = r, float(torch.nan_to_num(err / S, nan=0.0, posinf=0.0).max())
            else:
                ratio = torch.where(amb.view(R, 1), torch.minimum(ratio, r), ratio)
            del ref, S, F, ex, tol, err
        self._rec("roi_align_fwd_kernel", "fwd", float(ratio.max()), es, f"R={R} C={Cn} pool={tuple(pool)}")
        self.seconds += time.time() - t0

    def _roi_bwd_check(self, kern, got, before, gout, geom, nlev, strides, Cn, rois, labels, rois_per_img, pool, sample_points, rel, what):
        """got (N * ppi, C) = before + the adjoint of RoIAlign: tol = rel |ref| + (2 cnt + 4) x 2^-24 S (capped at MAX_F32 S; cnt = the
        (sample, corner) terms the reference counts for the pixel: one multiply-add each in the kernel's separable sums, the add onto the
        old value and the 1 / S^2 scales) + roi_weight_err(level) x G (fp32 sample coordinates)."""
        l64, l32, amb = self._roi_levels(rois, labels, strides, nlev)
        ratio, es = None, 0.0
        werr = torch.zeros(geom.pix_per_img, dtype=torch.float64, device=got.device)
        for l in range(nlev):
            werr[geom.off[l]:geom.off[l] + geom.H[l] * geom.W[l]] = roi_weight_err(geom.H[l], geom.W[l])
        werr = werr.repeat(geom.N).view(-1, 1)
        for lv in ((l64,) if not bool(amb.any()) else (l64, l32)):
            ref, S, G, cnt = U.roi_align_ref_bwd(gout, geom, nlev, strides, Cn, rois, labels, rois_per_img, pool, sample_points, lv)
            if before is not None:
                ref += before.double()
                S += before.double().abs()
            tol = rel * ref.abs() + torch.clamp((2 * cnt + 4) * U24, max=MAX_F32).view(-1, 1) * S + werr * G
            err = (got.double() - ref).abs()
            r = torch.nan_to_num(torch.where(err == 0, torch.zeros_like(err), err / tol), nan=float("inf"), posinf=float("inf"))
            if ratio is None:
                ratio, es = r, float(torch.nan_to_num(err / S, nan=0.0, posinf=0.0).max())
                ref0, S0 = ref, S
            else:       # a pixel whose sum holds an ambiguous RoI may match either level; every other pixel keeps the first verdict
                moved = (ref != ref0) | (S != S0)
                ratio = torch.where(moved, torch.minimum(ratio, r), ratio)
            del ref, S, G, cnt, tol, err
        self._rec(kern, "bwd", float(ratio.max()), es, what)

    def roi_align_bwd_bf16(self, gout, geom, nlev, strides, Cn, rois, labels, rois_per_img, pool, sample_points, gfeat, ws, accumulate=False):
        """The tiled fixed-order sum: every pixel of every level of the pyramid is written (accumulate: added to what it holds, one bf16
        rounding of the fp32 sum)."""
        self._count("roi_align_bwd_bf16")
        before = gfeat.clone() if accumulate else None
        self.orig["roi_align_bwd_bf16"](gout, geom, nlev, strides, Cn, rois, labels, rois_per_img, pool, sample_points, gfeat, ws, accumulate=accumulate)
        torch.cuda.synchronize()
        t0 = time.time()
        self._roi_bwd_check("roi_align_bwd_tile_kernel", gfeat, before, gout, geom, nlev, strides, Cn, rois, labels, rois_per_img, pool,
                            sample_points, REL_BF16, f"R={rois.shape[0]} C={Cn} acc={accumulate}")
        self.seconds += time.time() - t0

    def roi_align_bwd(self, gout, geom, nlev, strides, Cn, rois, labels, rois_per_img, pool, sample_points, gfeat):
        """The fp32 scatter: float atomics onto what the buffer holds; the order of the sum is free, its length is the contribution count.
        No bf16 rounding (relative term: one fp32 rounding)."""
        self._count("roi_align_bwd")
        before = gfeat.clone()
        self.orig["roi_align_bwd"](gout, geom, nlev, strides, Cn, rois, labels, rois_per_img, pool, sample_points, gfeat)
        torch.cuda.synchronize()
        t0 = time.time()
        self._roi_bwd_check("roi_align_bwd_kernel", gfeat, before, gout, geom, nlev, strides, Cn, rois, labels, rois_per_img, pool,
                            sample_points, U24, f"R={rois.shape[0]} C={Cn} pool={tuple(pool)}")
        self.seconds += time.time() - t0

    def f32_to_bf16(self, src, dst, accumulate=False):
        """bf16(src): one rounding, 2^-8 |ref|; with accumulate one fp32 add in front: + 2^-24 S."""
        self._count("f32_to_bf16")
        before = dst.clone() if accumulate else None
        self.orig["f32_to_bf16"](src, dst, accumulate=accumulate)
        torch.cuda.synchronize()
        ref, S = U.f32_to_bf16_ref(src, before)
        r = U.bound_ratio(dst.view_as(src), ref, S, REL_BF16, U24)
        self._finite("f32_to_bf16", "conv", dst, f"n={src.numel()}")
        self._rec("f32_to_bf16_add_kernel" if accumulate else "f32_to_bf16_kernel", "conv", float(r.max()), 0.0, f"n={src.numel()}")

    def subsample2x_fwd(self, src, gsrc, dst, gdst, Cn):
        """A copy: the destination level equals the even pixels of the source level bit for bit; every other row keeps its bits."""
        self._count("subsample2x_fwd")
        before = dst.clone()
        self.orig["subsample2x_fwd"](src, gsrc, dst, gdst, Cn)
        torch.cuda.synchronize()
        N, n = gdst.N, gdst.H[0] * gdst.W[0]
        want = U.subsample2x_ref(before if src.data_ptr() == dst.data_ptr() else src, gsrc, gdst)
        got = dst.view(N, gdst.pix_per_img, -1)[:, gdst.off[0]:gdst.off[0] + n]
        same = _same_bits(got, want)
        cover = _rows(N, gdst.pix_per_img, [(gdst.off[0], n)], dst.device)
        self._rec("subsample_fwd_kernel", "fwd", 0.0 if same else float("inf"), 0.0, f"{N}x{gsrc.H[0]}x{gsrc.W[0]}x{Cn}")
        if not _same_bits(dst[~cover], before[~cover]):
            self.bad.append("subsample2x_fwd wrote rows outside its level")

    def subsample2x_bwd_add(self, g_dst, gdst, g_src, gsrc, Cn):
        """Even pixels of the source level: bf16 of the two-term sum (one fp32 add, one bf16 rounding: 2^-8 |ref| + 2^-24 S); every other
        pixel of the buffer keeps its bits."""
        self._count("subsample2x_bwd_add")
        assert g_dst.data_ptr() == g_src.data_ptr(), "the audit expects both levels in one buffer"
        before = g_src.clone()
        self.orig["subsample2x_bwd_add"](g_dst, gdst, g_src, gsrc, Cn)
        torch.cuda.synchronize()
        N, n = gsrc.N, gsrc.H[0] * gsrc.W[0]
        ref, S, touched = U.subsample2x_ref_bwd(before, gdst, gsrc)
        got = g_src.view(N, gsrc.pix_per_img, -1)[:, gsrc.off[0]:gsrc.off[0] + n]
        r = U.bound_ratio(got, ref, S, REL_BF16, U24)
        self._finite("subsample_bwd_kernel", "bwd", got, "source level")
        self._rec("subsample_bwd_kernel", "bwd", float(r.max()), 0.0, f"{N}x{gsrc.H[0]}x{gsrc.W[0]}x{Cn}")
        old = before.view(N, gsrc.pix_per_img, -1)[:, gsrc.off[0]:gsrc.off[0] + n]
        if not _same_bits(got[~touched], old[~touched]):
            self.bad.append("subsample2x_bwd_add changed pixels off the even grid")
        cover = _rows(N, gsrc.pix_per_img, [(gsrc.off[0], n)], g_src.device)
        if not _same_bits(g_src[~cover], before[~cover]):
            self.bad.append("subsample2x_bwd_add wrote rows outside the source level")

    def rcnn_loss_fwd_bwd(self, raw, ld, K, box_off, labels, targets, R, beta, num_samples, loss2, draw):
        """Every element of d_rcnn_raw from the same bf16 logits.  Logit columns: the fp32 softmax p = exp(x - lse) carries a relative
        error of at most amp x 2^-23 with amp = 2 max |x| + 8 (the roundings of x - lse, of lse = log(sum) + max and a few ulp of expf /
        logf act on the ARGUMENT), then one subtraction, the 1 / count scale and the bf16 rounding: tol = 2^-8 |ref| + amp 2^-22 S with
        S = (p + onehot) / count.  Delta columns: sign(x) / count, or x / (beta count) inside the quadratic zone (a subtraction, a division, a
        scale: 4 x 2^-24 S).  Everything else is an exact zero.  The losses: fp32 sums over R rows in a fixed tree of at most R / 256 + 16
        adds on top of the rows' own amp 2^-23."""
        self._count("rcnn_loss_fwd_bwd")
        l0 = loss2.clone()
        d0 = draw.clone()
        self.orig["rcnn_loss_fwd_bwd"](raw, ld, K, box_off, labels, targets, R, beta, num_samples, loss2, draw)
        torch.cuda.synchronize()
        if not _same_bits(draw[R:], d0[R:]):
            self.bad.append("rcnn_loss_fwd_bwd wrote rows behind R")
        del d0
        ns = int(num_samples.view(-1)[0])
        o = U.rcnn_loss_ref(raw[:R], ld, K, box_off, labels.view(-1)[:R], targets.view(-1, 4)[:R], beta, ns)
        absf = torch.full((R, ld), 4 * U24, dtype=torch.float64, device=raw.device)
        absf[:, :K + 1] = o["amp"] * 2.0 ** -22
        tol = REL_BF16 * o["draw"].abs() + absf * o["S_draw"]
        self._ratio("rcnn_loss_kernel", "grad", draw[:R], o["draw"], tol, o["exact"], f"R={R} samples={ns}", o["S_draw"])
        amp = float(o["amp"].max())
        for i, k in enumerate(("cls", "box")):
            ref, S = o[k] + float(l0[i]), o["S_" + k] + abs(float(l0[i]))
            tol_l = (_cdiv(R, 256) + 16 + 2 * amp) * U24 * S
            err = abs(float(loss2[i]) - ref)
            self._rec("rcnn_loss_kernel", k, 0.0 if err == 0 else err / tol_l, err / S if S else 0.0, f"loss {k} = {ref:.6g}")

    # -- install / remove -------------------------------------------------------------------------------------------
    def __enter__(self):
        ops = self.ops
        self.orig = {n: getattr(ops, n) for n in WRAPPED}
        for n in WRAPPED:
            setattr(ops, n, getattr(self, n))
        lib = ops.L()
        from basedet_amd import _lib
        self._abi = {s: getattr(lib, s) for s in _lib.SIGNATURES if is_launch(s)}
        for s, f in self._abi.items():
            def counted(*a, _f=f, _s=s):
                if not self.inner:
                    self.reached[_s] += 1
                    if _s in CONV_ABI:
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

