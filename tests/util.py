"""Helpers shared by the GPU parity tests (layout conversions, reference convs on CPU fp32)."""
import numpy as np
import torch
import torch.nn.functional as TF


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def nchw_to_pm(x):
    """(N,C,H,W) fp32 -> pixel-major (N*H*W, C) bf16 on cuda."""
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous().to(torch.bfloat16).cuda()


def pm_to_nchw(t, n, h, w):
    c = t.shape[1]
    return t.float().cpu().reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous()


def oihw_to_ohwi(w):
    return w.permute(0, 2, 3, 1).contiguous()


def rel_l2(a, b):
    a = a.double().flatten()
    b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def pack_weights(ops, w_oihw, row_scale=None):
    """fp32 OIHW (cpu) -> (w_fwd, w_dgrad) bf16 packed device tensors via bd_weight_pack."""
    co, ci, r, s = w_oihw.shape
    w = oihw_to_ohwi(w_oihw).cuda()
    wf = torch.empty((co, r * s, ci), dtype=torch.bfloat16, device="cuda")
    wd = torch.empty((ci, r * s, co), dtype=torch.bfloat16, device="cuda")
    rs = None if row_scale is None else row_scale.cuda()
    ops.weight_pack(w, rs, wf, wd, co, r * s, ci)
    return wf, wd


def bf16_ulps(got, ref):
    """Distance in bf16 steps between a bf16 tensor and a high-precision reference rounded to bf16 (elementwise, int32).
    The bit patterns are mapped to a monotone integer line on which +0 and -0 coincide."""
    def key(t):
        v = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(v < 0, -(v & 0x7FFF), v)
    return (key(got) - key(ref.to(torch.bfloat16))).abs()


def f32_ulps(got, ref):
    """Distance of fp32 values from a float64 reference in units of the fp32 spacing at the reference (elementwise, float64)."""
    r = ref.double()
    e = torch.frexp(r.float().abs().clamp_min(torch.finfo(torch.float32).tiny))[1]
    return (got.double() - r).abs() / torch.ldexp(torch.ones_like(r), (e - 24).to(torch.int32))


# ---- float64 reference of the pixel-major, multi-level convolutions (bd_conv_desc) ----------------------------------------------------
# Every function works on whatever device its operands live on (float64 unfold / fold / matmul, one image at a time: no cuDNN / MIOpen
# convolution, which has no float64 form on ROCm).  Each result comes with S, the same operation applied to |operands| (|x|, |w|, |g|,
# |bias|, |add|): the scale the kernel's fp32 accumulation error is measured against.  Rows of the output buffer that no level of the
# descriptor covers (other pyramid levels, images not asked for) are NaN in both.
EPI_RELU, EPI_ADD_BEFORE, EPI_ADD_AFTER, EPI_MASK, EPI_SPARSE = 1, 2, 4, 8, 16


def desc_levels(d):
    """[(Hi, Wi, Ho, Wo, in_off, out_off)] of a bd_conv_desc."""
    return [(d.Hi[i], d.Wi[i], d.Ho[i], d.Wo[i], d.in_off[i], d.out_off[i]) for i in range(d.nseg)]


def _img_level(t, ppi, n, off, H, W):
    """(H*W, C) rows of image n, level at pixel offset `off`, of a pixel-major buffer t (N*ppi, C)."""
    return t[n * ppi + off: n * ppi + off + H * W]


def _unfold(xi, H, W, R, S, stride, pad):
    """xi (H*W, C) float64 -> cols (C*R*S, Ho*Wo) (torch.unfold order: channel slowest)."""
    return TF.unfold(xi.t().reshape(1, -1, H, W), (R, S), padding=pad, stride=stride)[0]


def _fold(cols, H, W, R, S, stride, pad):
    """cols (C*R*S, Ho*Wo) -> (H*W, C): the adjoint of _unfold (sums the taps landing on one input pixel)."""
    return TF.fold(cols.unsqueeze(0), (H, W), (R, S), padding=pad, stride=stride)[0].reshape(-1, H * W).t()


def _images(d, images):
    return range(d.N) if images is None else images


def decode_maskbits(bits, C):
    """uint32 [C/32][M] (bit b of word (g, m) = channel 32 g + b of pixel m; stored as int32) -> bool (M, C)."""
    b = bits.to(torch.int64) & 0xFFFFFFFF
    sh = torch.arange(32, device=bits.device, dtype=torch.int64).view(1, 32, 1)
    return ((b.unsqueeze(1) >> sh) & 1).reshape(C, -1).t().bool()


def _epilogue(acc, s, flags, bias, add, gate):
    """The bd_conv2d_fwd / _dgrad epilogue on float64 (acc, S); returns (ref, S, exact).  exact marks elements the kernel must reproduce
    bit for bit: a closed gate (the value is 0 or add, both representable) and a ReLU whose input is below -2^-16 S (the fp32 sum is
    negative too, so max(v, 0) is exactly 0)."""
    if bias is not None:
        acc = acc + bias
        s = s + bias.abs()
    if add is not None and flags & EPI_ADD_BEFORE:
        acc = acc + add
        s = s + add.abs()
    exact = torch.zeros_like(acc, dtype=torch.bool)
    if flags & EPI_RELU:
        exact |= acc < -(2.0 ** -16) * s
        acc = acc.clamp_min(0.0)
    if gate is not None:
        exact |= ~gate
        acc = torch.where(gate, acc, torch.zeros_like(acc))
        s = torch.where(gate, s, torch.zeros_like(s))
    if add is not None and flags & EPI_ADD_AFTER:
        acc = acc + add
        s = s + add.abs()
    return acc, s, exact


def conv_ref_fwd(d, x, w_fwd, bias=None, add=None, flags=0, images=None):
    """y = epi(conv(x, w) + bias [+ add]) of bd_conv2d_fwd: x (N*in_ppi, Cin) bf16, w_fwd the packed bf16 (Cout, R*S, Cin) the kernel
    read.  Returns (ref, S, exact), float64 (N*out_ppi, Cout)."""
    dev = x.device
    Cin, Cout, R, S_, st, pad = d.Cin, d.Cout, d.R, d.S, d.stride, d.pad
    W = w_fwd.double().view(Cout, R, S_, Cin).permute(0, 3, 1, 2).reshape(Cout, Cin * R * S_)
    Wa = W.abs()
    b = bias.double() if bias is not None else None
    ref = torch.full((d.N * d.out_pix_per_img, Cout), float("nan"), dtype=torch.float64, device=dev)
    sm, ex = ref.clone(), torch.zeros(ref.shape, dtype=torch.bool, device=dev)
    for Hi, Wi, Ho, Wo, io, oo in desc_levels(d):
        for n in _images(d, images):
            xi = _img_level(x, d.in_pix_per_img, n, io, Hi, Wi).double()
            if R == 1 and S_ == 1 and st == 1 and pad == 0:
                acc, s = xi @ W.t(), xi.abs() @ Wa.t()
            else:
                cols = _unfold(xi, Hi, Wi, R, S_, st, pad)
                acc, s = (W @ cols).t(), (Wa @ cols.abs()).t()
            a = _img_level(add, d.out_pix_per_img, n, oo, Ho, Wo).double() if add is not None else None
            r0 = n * d.out_pix_per_img + oo
            ref[r0:r0 + Ho * Wo], sm[r0:r0 + Ho * Wo], ex[r0:r0 + Ho * Wo] = _epilogue(acc, s, flags, b, a, None)
    return ref, sm, ex


def conv_ref_dgrad(d, g, w_dgrad, add=None, mask=None, maskbits=None, flags=0, images=None):
    """dx = epi(conv_transpose(g, w) [+ add]) of bd_conv2d_dgrad / _bits: g (N*out_ppi, Cout), w_dgrad the packed bf16 (Cin, R*S, Cout);
    EPI_MASK gates with mask > 0 (bf16 activation) or with the decoded maskbits ([Cin/32][N*in_ppi]); EPI_SPARSE leaves the input pixels
    that no tap reaches as `add` holds them (exact).  Returns (ref, S, exact), float64 (N*in_ppi, Cin)."""
    dev = g.device
    Cin, Cout, R, S_, st, pad = d.Cin, d.Cout, d.R, d.S, d.stride, d.pad
    # cols row (ci, r, s) = sum_co w[co, ci, r, s] g[co]: the unfold order of _fold
    Wc = w_dgrad.double().reshape(Cin * R * S_, Cout)
    Wca = Wc.abs()
    gate_all = decode_maskbits(maskbits, Cin) if maskbits is not None else None
    ref = torch.full((d.N * d.in_pix_per_img, Cin), float("nan"), dtype=torch.float64, device=dev)
    sm, ex = ref.clone(), torch.zeros(ref.shape, dtype=torch.bool, device=dev)
    for Hi, Wi, Ho, Wo, io, oo in desc_levels(d):
        reached = None
        if flags & EPI_SPARSE:
            ones = torch.ones((R * S_, Ho * Wo), dtype=torch.float64, device=dev)
            reached = _fold(ones, Hi, Wi, R, S_, st, pad)[:, 0] > 0
        for n in _images(d, images):
            gi = _img_level(g, d.out_pix_per_img, n, oo, Ho, Wo).double()
            if R == 1 and S_ == 1 and st == 1 and pad == 0:
                acc, s = gi @ Wc.t(), gi.abs() @ Wca.t()
            else:
                acc = _fold(Wc @ gi.t(), Hi, Wi, R, S_, st, pad)
                s = _fold(Wca @ gi.abs().t(), Hi, Wi, R, S_, st, pad)
            a = _img_level(add, d.in_pix_per_img, n, io, Hi, Wi).double() if add is not None else None
            gate = None
            if flags & EPI_MASK:
                if gate_all is not None:
                    gate = _img_level(gate_all, d.in_pix_per_img, n, io, Hi, Wi)
                else:
                    gate = _img_level(mask, d.in_pix_per_img, n, io, Hi, Wi).float() > 0
            r, s, e = _epilogue(acc, s, flags, None, a, gate)
            if reached is not None:
                keep = ~reached.unsqueeze(1)
                r, s, e = torch.where(keep, a, r), torch.where(keep, torch.zeros_like(s), s), e | keep
            r0 = n * d.in_pix_per_img + io
            ref[r0:r0 + Hi * Wi], sm[r0:r0 + Hi * Wi], ex[r0:r0 + Hi * Wi] = r, s, e
    return ref, sm, ex


def conv_ref_wgrad(d, x, g, row_scale=None, dw0=None, bias=False, db0=None):
    """bd_conv2d_wgrad / _wgrad_bias: dw (Cout, R, S, Cin) = row_scale[co] * sum over every image and level of g x (+ dw0 when the launch
    accumulates), db (Cout,) = sum g (+ db0).  Returns (dw, S_dw, db, S_db) in float64 (db, S_db None without bias)."""
    dev = x.device
    Cin, Cout, R, S_, st, pad = d.Cin, d.Cout, d.R, d.S, d.stride, d.pad
    acc = torch.zeros((Cout, Cin * R * S_), dtype=torch.float64, device=dev)
    s = torch.zeros_like(acc)
    db = torch.zeros((Cout,), dtype=torch.float64, device=dev)
    sdb = torch.zeros_like(db)
    for Hi, Wi, Ho, Wo, io, oo in desc_levels(d):
        for n in range(d.N):
            xi = _img_level(x, d.in_pix_per_img, n, io, Hi, Wi).double()
            gi = _img_level(g, d.out_pix_per_img, n, oo, Ho, Wo).double()
            if R == 1 and S_ == 1 and st == 1 and pad == 0:
                acc += gi.t() @ xi
                s += gi.abs().t() @ xi.abs()
            else:
                cols = _unfold(xi, Hi, Wi, R, S_, st, pad)
                acc += gi.t() @ cols.t()
                s += gi.abs().t() @ cols.abs().t()
            db += gi.sum(0)
            sdb += gi.abs().sum(0)
    acc = acc.view(Cout, Cin, R, S_).permute(0, 2, 3, 1)
    s = s.view(Cout, Cin, R, S_).permute(0, 2, 3, 1)
    if row_scale is not None:
        rs = row_scale.double().view(Cout, 1, 1, 1)
        acc, s = acc * rs, s * rs.abs()
    if dw0 is not None:
        acc, s = acc + dw0.double(), s + dw0.double().abs()
    if not bias:
        return acc, s, None, None
    if db0 is not None:
        db, sdb = db + db0.double(), sdb + db0.double().abs()
    return acc, s, db, sdb


def bound_ratio(got, ref, S, rel, abs_s, exact=None):
    """err / tol per element, tol = rel |ref| + abs_s S; elements marked exact must match bit for bit (ratio 0 or inf).  NaN rows of ref
    are not covered by the reference: ratio 0 there (the caller checks them separately)."""
    g = got.double()
    err = (g - ref).abs()
    tol = rel * ref.abs() + abs_s * S
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    if exact is not None:
        r = torch.where(exact, torch.where(g == ref, torch.zeros_like(r), torch.full_like(r, float("inf"))), r)
    return torch.nan_to_num(r, nan=0.0, posinf=float("inf"))
