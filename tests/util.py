"""Helpers shared by the GPU parity tests (layout conversions, reference convs on CPU fp32)."""
import math

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


def flat_storage(shapes, device="cuda"):
    """What a model's parameter arena gives a layer's adopt(): one flat fp32 tensor for the masters and one for the gradients, and
    {name: view} of each in `shapes` (the layer's arena_shapes()), in 256-byte aligned slices like ParamArena's.
    -> (w_flat, g_flat, w_views, g_views); the gradients start at NaN."""
    pad = lambda s: (math.prod(s) + 63) // 64 * 64
    total = sum(pad(s) for s in shapes.values())
    flats, views = [], []
    for fill in (0.0, float("nan")):
        f, v, o = torch.full((total,), fill, dtype=torch.float32, device=device), {}, 0
        for k, s in shapes.items():
            v[k] = f[o:o + math.prod(s)].view(s)
            o += pad(s)
        flats.append(f)
        views.append(v)
    return flats[0], flats[1], views[0], views[1]


def lies_inside(t, flat):
    return flat.data_ptr() <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= flat.data_ptr() + flat.numel() * flat.element_size()


def norm_record(C, device="cuda"):
    """A hand-filled record with models/live_norm.py BatchNormState's fields, for BatchNormAct.adopt: every vector a view of one tensor
    (zeros, as LiveNorms.allocate leaves them; the two gradient vectors start at NaN)."""
    import types
    buf = torch.zeros((11, C), dtype=torch.float32, device=device)
    buf[9:] = float("nan")
    return types.SimpleNamespace(buf=buf, gamma=buf[0], beta=buf[1], running_mean=buf[2], running_var=buf[3], mean=buf[4], inv_std=buf[5],
                                 sums=buf[6:9], g_gamma=buf[9], g_beta=buf[10])


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


# ---- float64 references of the launches only the Faster R-CNN step makes ---------------------------------------------------------------
# Same conventions as conv_ref_*: torch float64 on the operands' device, S = the same operation on |operands|.
def thin_ref_fwd(x, w, bias, chunk=1 << 18):
    """bd_conv1x1_thin_fwd: y = x bf16(w)^T + bias; x (M, Cin) bf16, w (Cout, Cin) the fp32 MASTER weight (the kernel rounds it to bf16
    itself).  Returns (ref, S), float64 (M, Cout)."""
    W = w.reshape(w.shape[0], -1).to(torch.bfloat16).double()
    b = bias.double() if bias is not None else torch.zeros(W.shape[0], dtype=torch.float64, device=x.device)
    M = x.shape[0]
    ref = torch.empty((M, W.shape[0]), dtype=torch.float64, device=x.device)
    S = torch.empty_like(ref)
    for r0 in range(0, M, chunk):
        xi = x[r0:r0 + chunk].double()
        ref[r0:r0 + chunk] = xi @ W.t() + b
        S[r0:r0 + chunk] = xi.abs() @ W.abs().t() + b.abs()
    return ref, S


def thin_ref_bwd(x, g, w, cout_real, chunk=1 << 18, dx=True):
    """bd_conv1x1_thin_bwd: dx = (x != 0) * g bf16(w) (x is a ReLU output: the gate is closed exactly where x is zero, and dx is an
    exact zero there), dW = g^T x, db = sum g; rows cout_real .. of dW / db are exact zeros.
    Returns (dx, S_dx, exact_dx, dW, S_dW, db, S_db); the first three are None with dx=False."""
    Cout = g.shape[1]
    W = w.reshape(Cout, -1).to(torch.bfloat16).double()
    M, Cin = x.shape
    dev = x.device
    rdx = sdx = ex = None
    if dx:
        rdx = torch.empty((M, Cin), dtype=torch.float64, device=dev)
        sdx = torch.empty_like(rdx)
        ex = torch.empty((M, Cin), dtype=torch.bool, device=dev)
    dW = torch.zeros((Cout, Cin), dtype=torch.float64, device=dev)
    sW = torch.zeros_like(dW)
    db = torch.zeros((Cout,), dtype=torch.float64, device=dev)
    sb = torch.zeros_like(db)
    for r0 in range(0, M, chunk):
        xi, gi = x[r0:r0 + chunk].double(), g[r0:r0 + chunk].double()
        if dx:
            open_ = xi != 0
            rdx[r0:r0 + chunk] = (gi @ W) * open_
            sdx[r0:r0 + chunk] = (gi.abs() @ W.abs()) * open_
            ex[r0:r0 + chunk] = ~open_
        dW += gi.t() @ xi
        sW += gi.abs().t() @ xi.abs()
        db += gi.sum(0)
        sb += gi.abs().sum(0)
    for t in (dW, sW, db, sb):
        t[cout_real:] = 0
    return rdx, sdx, ex, dW, sW, db, sb


def roi_levels(rois, strides, dtype):
    """assign_rois (roi_pool.py:12-25): floor(4 + log2(sqrt(area) / 224)) clamped to the levels of `strides`, evaluated in `dtype` from
    the fp32 boxes; a NaN or -inf argument gives the lowest level.  Returns int64 level indices."""
    lo, hi = int(math.log2(strides[0])), int(math.log2(strides[-1]))
    b = rois.to(dtype)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    v = 4.0 + torch.log(torch.sqrt(area) / 224.0) / 0.6931471805599453
    lv = torch.full(v.shape, lo, dtype=torch.int64, device=rois.device)
    ok = (v == v) & (v > lo)
    fl = torch.floor(torch.where(ok, v, torch.zeros_like(v))).clamp(lo, hi).to(torch.int64)
    return torch.where(ok, torch.where(v >= hi, torch.full_like(lv, hi), fl), lv) - lo


def _roi_samples(rois, scale, H, W, PH, PW, SP):
    """Sample points of RoIs (r, 4) on one level in float64 (the coordinates of roi_align_fwd_kernel, from the fp32 boxes):
    returns (idx (r, PH*PW, SP*SP, 4) int64 pixel index y * W + x of the four corners, wgt same shape float64 (zero for a sample outside
    the [-1, size] window), cell (r, PH*PW, SP*SP) int64 index of the top-left corner, frac (r, PH*PW, SP*SP, 2) the offsets (ly, lx) of the
    sample inside its cell)."""
    b = rois.double()
    dev = rois.device
    sw, sh = b[:, 0] * scale - 0.5, b[:, 1] * scale - 0.5
    bw, bh = ((b[:, 2] * scale - 0.5) - sw) / PW, ((b[:, 3] * scale - 0.5) - sh) / PH
    ar = lambda n: torch.arange(n, dtype=torch.float64, device=dev)
    # (r, P, SP) sample coordinates along each axis
    ys = sh.view(-1, 1, 1) + ar(PH).view(1, -1, 1) * bh.view(-1, 1, 1) + (ar(SP).view(1, 1, -1) + 0.5) * bh.view(-1, 1, 1) / SP
    xs = sw.view(-1, 1, 1) + ar(PW).view(1, -1, 1) * bw.view(-1, 1, 1) + (ar(SP).view(1, 1, -1) + 0.5) * bw.view(-1, 1, 1) / SP

    def lin(c, n):
        ok = ~((c < -1.0) | (c > n))
        c = c.clamp_min(0.0)
        i0 = torch.floor(c).to(torch.int64)
        top = i0 >= n - 1
        i0 = torch.where(top, torch.full_like(i0, n - 1), i0)
        i1 = torch.where(top, i0, i0 + 1)
        l = torch.where(top, torch.zeros_like(c), c - i0.double())
        return i0, i1, 1.0 - l, l, ok
    y0, y1, hy, ly, oky = lin(ys, H)
    x0, x1, hx, lx, okx = lin(xs, W)
    r = rois.shape[0]
    # broadcast to (r, PH, PW, SPy, SPx)
    Y = lambda t: t.view(r, PH, 1, SP, 1)
    X = lambda t: t.view(r, 1, PW, 1, SP)
    ok = (Y(oky) & X(okx)).double()
    idx = torch.stack([Y(y0) * W + X(x0), Y(y0) * W + X(x1), Y(y1) * W + X(x0), Y(y1) * W + X(x1)], -1)
    wgt = torch.stack([Y(hy) * X(hx), Y(hy) * X(lx), Y(ly) * X(hx), Y(ly) * X(lx)], -1) * ok.unsqueeze(-1)
    shape = (r, PH * PW, SP * SP)
    frac = torch.stack([Y(ly).expand(r, PH, PW, SP, SP), X(lx).expand(r, PH, PW, SP, SP)], -1).reshape(shape + (2,))
    return idx.reshape(shape + (4,)), wgt.reshape(shape + (4,)), idx[..., 0].reshape(shape), frac


def _box4(a, H, W):
    """(H*W, C) -> the sum of a over the 4 x 4 pixels (y-1 .. y+2, x-1 .. x+2) around every pixel (zero outside the map)."""
    t = a.t().reshape(1, -1, H, W)
    t = TF.pad(t, (1, 2, 1, 2))
    return (TF.avg_pool2d(t, 4, stride=1) * 16.0)[0].reshape(-1, H * W).t()


def roi_align_ref_fwd(feat, geom, nlev, strides, C, rois, labels, rois_per_img, pool, SP, levels, rois_chunk=128, edge_eps=None):
    """bd_roi_align_fwd: out (R, PH*PW*C) = the mean over SP x SP bilinear samples per bin of the level `levels[r]` map of image
    r // rois_per_img; slots with label < 0 give zeros (exact).  Returns (ref, S, F, exact): S weighs |feat| with the same weights; F is
    the UNWEIGHTED mean over the samples of the sum of |feat| over each sample's four corners -- the scale an error of the bilinear
    WEIGHTS (fp32 sample coordinates in the kernel) is measured against.  A sample whose offset in its cell is within edge_eps[level] of 0
    or 1 (None: every sample) may land in the neighbouring cell when its coordinate is rounded: it counts the 4 x 4 pixels around its cell."""
    PH, PW = pool
    R = rois.shape[0]
    dev = feat.device
    nb = PH * PW
    ref = torch.zeros((R, nb, C), dtype=torch.float64, device=dev)
    S, F = torch.zeros_like(ref), torch.zeros_like(ref)
    valid = torch.ones(R, dtype=torch.bool, device=dev) if labels is None else labels >= 0
    img = torch.arange(R, device=dev) // rois_per_img
    for n in range(geom.N):
        for l in range(nlev):
            sel = torch.nonzero((img == n) & (levels == l) & valid).view(-1)
            if sel.numel() == 0:
                continue
            H, W = geom.H[l], geom.W[l]
            f = feat[n * geom.pix_per_img + geom.off[l]: n * geom.pix_per_img + geom.off[l] + H * W].double()
            fa = f.abs()
            f4 = _box4(fa, H, W)
            for c0 in range(0, sel.numel(), rois_chunk):
                s = sel[c0:c0 + rois_chunk]
                idx, wgt, cell, frac = _roi_samples(rois[s], 1.0 / strides[l], H, W, PH, PW, SP)
                w = wgt.unsqueeze(-1)
                ref[s] = (f[idx] * w).sum((2, 3)) / (SP * SP)
                S[s] = (fa[idx] * w).sum((2, 3)) / (SP * SP)
                wide = f4[cell]
                if edge_eps is not None:
                    near = ((frac < edge_eps[l]) | (frac > 1.0 - edge_eps[l])).any(-1)
                    wide = torch.where(near.unsqueeze(-1), wide, fa[idx].sum(3))
                F[s] = wide.sum(2) / (SP * SP)
    exact = (~valid).view(R, 1, 1).expand(R, nb, C)
    return ref.view(R, -1), S.view(R, -1), F.view(R, -1), exact.reshape(R, -1)


def roi_align_ref_bwd(gout, geom, nlev, strides, C, rois, labels, rois_per_img, pool, SP, levels, rois_chunk=128):
    """The adjoint of roi_align_ref_fwd: gout (R, PH*PW*C) -> (ref, S, G, cnt) over the whole pixel-major pyramid (N * ppi, C) float64
    (levels no RoI is pooled from, and pixels no sample reaches, are zero): ref the gradient, S the same sum over |gout|, G the sum of
    |gout| / SP^2 over every sample whose cell lies within the 4 x 4 pixels around the pixel (the scale of a weight error), cnt (N * ppi,)
    the number of (sample, corner) terms the pixel's sum has."""
    PH, PW = pool
    R = rois.shape[0]
    dev = gout.device
    nb = PH * PW
    shape = (geom.N * geom.pix_per_img, C)
    ref = torch.zeros(shape, dtype=torch.float64, device=dev)
    S, G = torch.zeros_like(ref), torch.zeros_like(ref)
    cnt = torch.zeros(shape[0], dtype=torch.float64, device=dev)
    valid = torch.ones(R, dtype=torch.bool, device=dev) if labels is None else labels >= 0
    img = torch.arange(R, device=dev) // rois_per_img
    gv = gout.view(R, nb, C)
    for n in range(geom.N):
        for l in range(nlev):
            sel = torch.nonzero((img == n) & (levels == l) & valid).view(-1)
            if sel.numel() == 0:
                continue
            H, W = geom.H[l], geom.W[l]
            r0 = n * geom.pix_per_img + geom.off[l]
            acc = torch.zeros((H * W, C), dtype=torch.float64, device=dev)
            sa, ga = torch.zeros_like(acc), torch.zeros_like(acc)
            ca = torch.zeros(H * W, dtype=torch.float64, device=dev)
            for c0 in range(0, sel.numel(), rois_chunk):
                s = sel[c0:c0 + rois_chunk]
                idx, wgt, cell, frac = _roi_samples(rois[s], 1.0 / strides[l], H, W, PH, PW, SP)
                g = gv[s].double() / (SP * SP)                                     # (r, nb, C)
                contrib = g.view(-1, nb, 1, 1, C) * wgt.unsqueeze(-1)              # (r, nb, SP^2, 4, C)
                acc.index_add_(0, idx.reshape(-1), contrib.reshape(-1, C))
                sa.index_add_(0, idx.reshape(-1), contrib.abs().reshape(-1, C))
                ca.index_add_(0, idx.reshape(-1), (wgt.reshape(-1) != 0).double())
                ga.index_add_(0, cell.reshape(-1), g.abs().view(-1, nb, 1, C).expand(-1, nb, SP * SP, C).reshape(-1, C))
            ref[r0:r0 + H * W], S[r0:r0 + H * W], cnt[r0:r0 + H * W] = acc, sa, ca
            # a sample of cell (y0, x0) can reach pixels y0 - 1 .. y0 + 2: pixel p collects the cells p - 2 .. p + 1 (the mirrored window)
            G[r0:r0 + H * W] = _box4(ga.flip(0), H, W).flip(0)
    return ref, S, G, cnt


def subsample2x_ref(src, gsrc, gdst):
    """bd_subsample2x_fwd: level gdst = the even pixels of level gsrc; returns the (N, Hd*Wd, C) tensor the destination level must hold
    (same dtype: a copy)."""
    N, Hs, Ws = gsrc.N, gsrc.H[0], gsrc.W[0]
    v = src.view(N, gsrc.pix_per_img, -1)[:, gsrc.off[0]:gsrc.off[0] + Hs * Ws].reshape(N, Hs, Ws, -1)
    return v[:, ::2, ::2].reshape(N, gdst.H[0] * gdst.W[0], -1)


def subsample2x_ref_bwd(g_before, gdst, gsrc):
    """bd_subsample2x_bwd_add on a buffer that holds both levels: g[src level][2y, 2x] += g[dst level][y, x].  Returns (ref, S, touched)
    for the rows of the source level, (N, Hs*Ws, C) float64 / bool (touched: the even grid; every other pixel keeps its bits)."""
    N, Hs, Ws = gsrc.N, gsrc.H[0], gsrc.W[0]
    Hd, Wd = gdst.H[0], gdst.W[0]
    C = g_before.shape[1]
    s = g_before.view(N, gsrc.pix_per_img, C)[:, gsrc.off[0]:gsrc.off[0] + Hs * Ws].reshape(N, Hs, Ws, C).double()
    d = g_before.view(N, gdst.pix_per_img, C)[:, gdst.off[0]:gdst.off[0] + Hd * Wd].reshape(N, Hd, Wd, C).double()
    ref, S = s.clone(), s.abs()
    ref[:, ::2, ::2] += d
    S[:, ::2, ::2] += d.abs()
    touched = torch.zeros((N, Hs, Ws, 1), dtype=torch.bool, device=g_before.device)
    touched[:, ::2, ::2] = True
    return ref.view(N, Hs * Ws, C), S.view(N, Hs * Ws, C), touched.expand(N, Hs, Ws, C).reshape(N, Hs * Ws, C)


def f32_to_bf16_ref(src, dst_before=None):
    """bd_f32_to_bf16 (dst = bf16(src)) and bd_f32_to_bf16_add (dst = bf16(float(dst) + src)); returns (ref, S) float64."""
    ref, S = src.double(), src.double().abs()
    if dst_before is not None:
        ref, S = ref + dst_before.double().view_as(ref), S + dst_before.double().abs().view_as(ref)
    return ref, S


def rcnn_loss_ref(raw, ld, K, box_off, labels, targets, beta, num_samples):
    """bd_rcnn_loss_fwd_bwd (rcnn.py:65-83) from the bf16 prediction rows raw (R, ld): softmax cross-entropy over the K + 1 logits and
    smooth-L1 (beta; plain L1 below 1e-5) on the four deltas of the ground-truth class of foreground rows, both divided by
    max(num_samples, 1).  Returns a dict: draw / S_draw (R, ld) float64, exact (R, ld) bool (label -1 rows, the columns outside the logits
    and the row's own deltas: exact zeros), amp (R, 1) = 2 max |logit| + 8 (the fp32 exp / log argument error in units of 2^-23),
    cls / box the two losses, S_cls / S_box their scales."""
    r = raw.double()
    R = r.shape[0]
    dev = raw.device
    gs = 1.0 / max(float(num_samples), 1.0)
    lab = labels.view(-1).to(torch.int64)
    valid = lab >= 0
    lc = lab.clamp_min(0)
    logits = r[:, :K + 1]
    lse = torch.logsumexp(logits, 1, keepdim=True)
    p = torch.exp(logits - lse)
    onehot = torch.zeros_like(p).scatter_(1, lc.view(-1, 1), 1.0)
    draw = torch.zeros((R, ld), dtype=torch.float64, device=dev)
    S = torch.zeros_like(draw)
    exact = torch.ones((R, ld), dtype=torch.bool, device=dev)
    draw[:, :K + 1] = (p - onehot) * gs
    S[:, :K + 1] = (p + onehot) * gs
    exact[:, :K + 1] = False
    fg = lab > 0
    cols = box_off + (lc - 1).clamp_min(0).view(-1, 1) * 4 + torch.arange(4, device=dev).view(1, 4)          # (R, 4)
    x = torch.gather(r, 1, cols) - targets.double().view(R, 4)
    xs = torch.gather(r, 1, cols).abs() + targets.double().view(R, 4).abs()
    if beta < 1e-5:
        gbox, sbox = torch.sign(x), torch.ones_like(x)
        lbox, slbox = x.abs(), xs
    else:
        gbox = torch.where(x.abs() < beta, x / beta, torch.sign(x))
        sbox = torch.where(x.abs() < beta, xs / beta, torch.ones_like(x))
        lbox = torch.where(x.abs() < beta, 0.5 * x * x / beta, x.abs() - 0.5 * beta)
        slbox = torch.where(x.abs() < beta, 0.5 * xs * xs / beta, xs + 0.5 * beta)
    fgc = fg.view(-1, 1).expand(R, 4)
    rows = torch.arange(R, device=dev).view(-1, 1).expand(R, 4)
    draw[rows[fgc], cols[fgc]] = gbox[fgc] * gs
    S[rows[fgc], cols[fgc]] = sbox[fgc] * gs
    exact[rows[fgc], cols[fgc]] = False
    dead = ~valid
    draw[dead], S[dead], exact[dead] = 0.0, 0.0, True
    xl = torch.gather(logits, 1, lc.view(-1, 1))
    cls_rows = torch.where(valid.view(-1, 1), lse - xl, torch.zeros_like(lse))
    s_rows = torch.where(valid.view(-1, 1), lse.abs() + xl.abs(), torch.zeros_like(lse))
    fg4 = fgc.double()
    return dict(draw=draw, S_draw=S, exact=exact, amp=2.0 * logits.abs().max(1, keepdim=True)[0] + 8.0,
                cls=float(cls_rows.sum() * gs), S_cls=float(s_rows.sum() * gs),
                box=float((lbox * fg4).sum() * gs), S_box=float((slbox * fg4).sum() * gs))


# ---- OTA assignment on edge-case gts (tests/test_ota_edges_gpu.py, tests/test_ota_edges_cpu.py) ----------------------------------------
# The pyramid of a 320 x 448 image: P = 2987 points = three 1024-point passes of the selection loops, the last one ragged (939).
OTA_EDGE_IMAGE = (320, 448)
OTA_EDGE_SIZES = ((40, 56), (20, 28), (10, 14), (5, 7), (3, 4))
OTA_EDGE_STRIDES = (8, 16, 32, 64, 128)
OTA_ARGS = (0.25, 2.0, 1.5, 2.5, 10)              # alpha, gamma, reg_weight, center_radius, candidate_k (OTAConfig)
# name -> (seed, gt counts per image, Gmax, K): the arguments of ota_edge_problem
OTA_EDGE_CASES = {
    "g100_0_37_1": (41, (100, 0, 37, 1), 100, 80),
    "g1_1": (12, (1, 1), 1, 80),
    "k13_ld16": (41, (100, 0, 37, 1), 100, 13),
}


def ota_edge_problem(seed, counts, Gmax, K, kinds=("zero_area", "outside", "dup")):
    """One OTA assignment problem on the 320 x 448 pyramid.  Gts as tests/test_assign_edges_gpu.py::edge_gts draws them (quarter-pixel
    coordinates, centres anywhere in the image, sides of 4 .. 200 px: the small ones hold fewer points than their dynamic k, so the
    +1e6 "outside" branch of the cost decides their selection); images with >= 8 gts get, from the end of their valid rows, a zero-area
    box, a box wholly outside the image and an exact copy of gt 0 with another class; rows >= num_gt hold NaN / 1e30.
    The copy's class logit is a copy of gt 0's at every point: the two cost rows are then the same numbers, every point they select is
    a conflict whose argmin is an exact tie, and "lowest gt index wins" decides the label.
    Images with a zero-area gt also hold a few "tie points" whose cost against that gt is one and the same smallest number (below).
    Predictions as tests/test_ota_gpu.py::_problem: ltrb towards a random gt plus noise.  Logits and predictions are bf16 values.
    Returns a dict: pts (per level), allp (P, 2), lvl_start, strides, gt (N, Gmax, 5), num (N,), logits (N, P, K), pred (N, P, 4),
    planted {(image, kind): gt row}, tie_points {image: point indices}."""
    from oracle import box_ops
    rng = np.random.default_rng(seed)
    H, W = OTA_EDGE_IMAGE
    pts = box_ops.point_anchors(list(OTA_EDGE_SIZES), list(OTA_EDGE_STRIDES), 0.5, 1)
    allp = np.concatenate(pts, 0).astype(np.float32)
    P, N = allp.shape[0], len(counts)
    gt = np.zeros((N, Gmax, 5), np.float32)
    planted = {}
    for n, G in enumerate(counts):
        cx, cy = rng.uniform(0, W, G), rng.uniform(0, H, G)
        w, h = 4 * 50 ** rng.random(G), 4 * 50 ** rng.random(G)              # 4 .. 200 px, as many below 28 px as above
        b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)
        gt[n, :G, :4] = np.round(b * 4) / 4
        gt[n, :G, 4] = rng.integers(1, K + 1, G)
        if G >= 8:
            s = G - 1
            for k in kinds:
                if k == "zero_area":
                    gt[n, s, :4] = [150.0, 100.0, 150.0, 160.0]                  # x1 == x2
                    gt[n, s, 4] = ((int(gt[n, 0, 4]) + 1) % K) + 1               # a class of its own among the planted rows
                elif k == "outside":
                    gt[n, s, :4] = [W + 50.0, H + 20.0, W + 300.0, H + 200.0]
                elif k == "dup":
                    gt[n, s] = gt[n, 0]
                    gt[n, s, 4] = (int(gt[n, 0, 4]) % K) + 1
                planted[(n, k)] = s
                s -= 1
        if G < Gmax:
            gt[n, G:] = np.where(rng.random((Gmax - G, 5)) < 0.5, np.nan, 1e30).astype(np.float32)
    num = np.asarray(counts, np.int32)
    pred = np.zeros((N, P, 4), np.float32)
    for n in range(N):
        if num[n] == 0:
            pred[n] = rng.uniform(0, 60, (P, 4))
            continue
        b = gt[n, rng.integers(0, num[n], P), :4]
        d = np.stack([allp[:, 0] - b[:, 0], allp[:, 1] - b[:, 1], b[:, 2] - allp[:, 0], b[:, 3] - allp[:, 1]], 1)
        pred[n] = np.maximum(d * rng.uniform(0.7, 1.3, (P, 4)) + rng.normal(0, 2.0, (P, 4)), 0)
    logits = rng.normal(-2.5, 1.2, (N, P, K)).astype(np.float32)
    for (n, k), s in planted.items():
        if k == "dup":
            logits[n, :, int(gt[n, s, 4]) - 1] = logits[n, :, int(gt[n, 0, 4]) - 1]
    tie_points = {}
    for (n, k), s in planted.items():
        if k == "zero_area":
            # the points the zero-area gt must choose among: a confident logit of its class, nothing else, and an empty predicted box
            # (IoU 0).  Their cost against that gt is one number, the smallest of its row; dyn_k is 1: the lowest index wins.
            # Image 0 has them in all three 1024-point passes, the other images only in the second and third.
            idx = [1024 * q + 37 + 301 * j for q in ((0, 1, 2) if n == 0 else (1, 2)) for j in range(2)]
            c = int(gt[n, s, 4]) - 1
            logits[n, :, c] = np.minimum(logits[n, :, c], -2.0)      # every other point: a class cost >= 0.4, several fp32 steps at 1e6 away
            logits[n, idx, :] = -6.0
            logits[n, idx, c] = 4.0
            pred[n, idx] = 0.0
            tie_points[n] = idx
    lvl_start = np.cumsum([0] + [h * w for h, w in OTA_EDGE_SIZES]).tolist()
    return dict(pts=pts, allp=allp, lvl_start=lvl_start, strides=list(OTA_EDGE_STRIDES), gt=gt, num=num, planted=planted, tie_points=tie_points,
                logits=bf16_round(torch.from_numpy(logits)).numpy(), pred=bf16_round(torch.from_numpy(pred)).numpy())


def ota_cost_tol(c):
    """How far two evaluations of one OTA cost may lie apart: 1e-4 |c| below the outside penalty (the re-associated class cost plus the
    exp / log intrinsics), 0.125 = two fp32 spacings at 1e6 above it (the pre-penalty costs differ by far less than one spacing, so the
    two sums land on the same or on neighbouring grid points)."""
    c = abs(float(c))
    return 1e-4 * c if c < 1e5 else 0.125


def ota_topk_selection(cost, ious, candidate_k=10):
    """OTATopkMatcher before its conflict step, from the oracle's cost / IoU matrices (G, P): (dyn_k (G,), the fp32 sums of the
    candidate_k largest IoUs (G,), the match matrix (G, P) bool, the costs of every row sorted ascending)."""
    G, P = cost.shape
    topk = -np.sort(-ious, axis=1, kind="stable")[:, :min(candidate_k, P)]
    sums = np.zeros(G, np.float32)
    for v in topk.T:
        sums = (sums + v).astype(np.float32)
    dyn = np.maximum(1, sums.astype(np.int64))
    mm = np.zeros((G, P), bool)
    for g in range(G):
        mm[g, np.argsort(cost[g], kind="stable")[: dyn[g]]] = True
    return dyn, sums, mm, np.sort(cost, axis=1)


def ota_topk_excuse(p, lab_o, lab_x, tgt_x, allp, gtl, cost, sel):
    """Why point p of one image may carry another label (lab_x, with ltrb target tgt_x) than the oracle's lab_o: "a", "b", "c" or None.
    cost (G, P) is the oracle's, sel = ota_topk_selection of it, gtl (G, 5) the valid gt rows.
      a  selection tie: a gt that selects p on one side only has cost(g, p) within ota_cost_tol of its dyn_k-th or (dyn_k + 1)-th
         smallest cost.  The gts in question: the oracle's selectors of p that the other side did not assign p to, and the gt the other
         side assigned p to (the one of class lab_x whose encoding of p is tgt_x, bit for bit) if the oracle did not select p for it;
      b  conflict tie: the two smallest costs of p's column are within ota_cost_tol of each other;
      c  dynamic-k tie: for one of the gts of (a) the sum of the 10 largest IoUs is within 1e-5 of an integer (the two sides' IoUs
         agree to 2e-6, ten of them are summed)."""
    from oracle import box_ops
    dyn, sums, mm, srt = sel
    G, P = cost.shape
    theirs = []
    if lab_x > 0:
        enc = box_ops.point_encode(allp[p][None, :], gtl[:, :4]).astype(np.float32)
        theirs = [g for g in range(G) if int(gtl[g, 4]) == lab_x and np.array_equal(enc[g], tgt_x)]
    one_sided = [g for g in theirs if not mm[g, p]] + [g for g in np.nonzero(mm[:, p])[0] if g not in theirs]
    for g in one_sided:
        c = cost[g, p]
        kth = [srt[g, dyn[g] - 1]] + ([srt[g, dyn[g]]] if dyn[g] < P else [])
        if min(abs(float(c) - float(t)) for t in kth) <= ota_cost_tol(c):
            return "a"
    if G >= 2:
        two = np.sort(cost[:, p])[:2]
        if float(two[1]) - float(two[0]) <= ota_cost_tol(two[0]):
            return "b"
    for g in one_sided:
        if abs(float(sums[g]) - round(float(sums[g]))) <= 1e-5:
            return "c"
    return None


def ota_topk_compare(prob, ref, lab_x, tgt_x):
    """The label maps of ref = ota_ground_truth(...) (top-k) and of another evaluation of the same problem: (number of foreground
    points of the oracle, the cap on differing points, [(image, point, excuse)] of every differing point)."""
    lab_o, _, _, aux = ref
    nfg = int((lab_o > 0).sum())
    out = []
    sels = {}
    for n, p in np.argwhere(lab_x != lab_o):
        G = int(prob["num"][n])
        if n not in sels:
            sels[n] = ota_topk_selection(aux[n][0], aux[n][1], OTA_ARGS[4])
        out.append((int(n), int(p), ota_topk_excuse(p, int(lab_o[n, p]), int(lab_x[n, p]), tgt_x[n, p], prob["allp"], prob["gt"][n, :G],
                                                    aux[n][0], sels[n])))
    return nfg, max(1, int(0.005 * nfg)), out


# ---- guard bands (tests/test_guard_cpu.py, tests/test_guard_gpu.py) --------------------------------------------------------------------
# A kernel test that allocates its operands at exactly their logical size cannot see a load or store that runs past them: the caching
# allocator rounds every block up, and the stray access lands in padding nobody inspects.  guarded() puts a tensor between two guards
# of a known bit pattern inside ONE allocation the test owns; gapped_geom() does the same between the levels and images of a pixel-major
# pyramid.  Everything is compared as integer bit patterns (NaN != NaN).
GUARD_MIN_ROWS = 512
GUARD_MIN_BYTES = 4096
GUARD_ALIGN = 256                        # the interior keeps the alignment the 16-byte vector / buffer loads of the library assume
FILLS = ("zero", "nan", "max")           # what an INPUT's guards and gaps hold; outputs hold "sentinel"
_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
# (even element, odd element) bit patterns.  nan: the quiet NaN of the format (e4m3 bytes: 0x7f).  max: the largest finite value, sign
# alternating (fmaxf drops a NaN: a max-pool that reads out of range passes a NaN-only test).  sentinel: a NaN with a payload no kernel
# produces by accident (one-byte tensors: 0xff, NaN in e4m3 and e5m2, which the saturating quantisers never write).
_PATTERNS = {
    (torch.bfloat16, "nan"): (0x7FC0, 0x7FC0), (torch.bfloat16, "max"): (0x7F7F, 0xFF7F), (torch.bfloat16, "sentinel"): (0x7FA5, 0x7FA5),
    (torch.float32, "nan"): (0x7FC00000, 0x7FC00000), (torch.float32, "max"): (0x7F7FFFFF, 0xFF7FFFFF),
    (torch.float32, "sentinel"): (0x7FA5A5A5, 0x7FA5A5A5),
    (torch.uint8, "nan"): (0x7F, 0x7F), (torch.uint8, "max"): (0x7E, 0xFE), (torch.uint8, "sentinel"): (0xFF, 0xFF),
    # one-byte tensors that hold e5m2 (guarded(..., fmt="e5m2")): 0x7e is a NaN there, the largest finite value is 0x7b
    ("e5m2", "nan"): (0x7F, 0x7F), ("e5m2", "max"): (0x7B, 0xFB), ("e5m2", "sentinel"): (0xFF, 0xFF),
}


def _signed(v, bits):
    return v - (1 << bits) if bits > 8 and v >= 1 << (bits - 1) else v


def fill_pattern(dtype, fill, n, device="cpu", fmt=None):
    """n elements of the fill's bit pattern, as the integer dtype of the same width.  fmt: the number format a one-byte tensor holds
    ("e5m2"; default e4m3)."""
    it = _INT_OF_SIZE[torch.empty(0, dtype=dtype).element_size()]
    if fill == "zero":
        return torch.zeros(n, dtype=it, device=device)
    bits = 8 * torch.empty(0, dtype=dtype).element_size()
    even, odd = (_signed(v, bits) for v in _PATTERNS[(fmt or dtype, fill)])
    out = torch.full((n,), even, dtype=it, device=device)
    out[1::2] = odd
    return out


def guard_rows_for(row_bytes, guard_rows=None):
    """Rows of one guard: at least GUARD_MIN_ROWS (or guard_rows) and GUARD_MIN_BYTES, rounded up to a multiple of GUARD_ALIGN bytes."""
    g = max(guard_rows or GUARD_MIN_ROWS, -(-GUARD_MIN_BYTES // row_bytes))
    step = GUARD_ALIGN // math.gcd(row_bytes, GUARD_ALIGN)
    return -(-g // step) * step


def bits_of(t):
    """The integer view of a tensor's bit patterns."""
    return t.view(_INT_OF_SIZE[t.element_size()])


def count_sentinel(t):
    """Elements of t that still hold the output sentinel."""
    return int((bits_of(t) == int(fill_pattern(t.dtype, "sentinel", 1)[0])).sum())


class GuardError(AssertionError):
    pass


class Guarded:
    """One allocation [front guard | interior | back guard]; .t is the interior: (rows, cols), or (rows,) for cols=None.  Gap rows of a
    gapped geometry (set_gaps) are part of the interior and are checked like the guards."""
    PLACES = ("front guard", "back guard", "level gap", "image gap")

    def __init__(self, rows, cols, dtype, device, guard_rows, fill, name, fmt=None):
        self.name, self.dtype, self.fill, self.fmt = name, dtype, fill, fmt
        self.rows, self.cols = rows, (1 if cols is None else cols)
        es = torch.empty(0, dtype=dtype).element_size()
        self.g = guard_rows_for(self.cols * es, guard_rows)
        slack = GUARD_ALIGN // es
        n = (2 * self.g + rows) * self.cols
        self.store = torch.empty(n + slack, dtype=dtype, device=device)
        lead = (-self.store.data_ptr() % GUARD_ALIGN) // es             # host allocations are not 256-byte aligned by themselves
        self.whole = self.store[lead:lead + n]
        bits_of(self.whole).copy_(fill_pattern(dtype, fill, n, device, fmt))
        self._rows2d = self.whole.view(2 * self.g + rows, self.cols)
        inner = self._rows2d[self.g:self.g + rows]
        self.t = inner.view(rows) if cols is None else inner
        self.kind = None
        self._snap = None

    def _row_pattern(self, first_elem):
        """(1, cols) bit pattern of a row whose first element has flat index `first_elem` in the allocation (the sign alternates per element)."""
        p = fill_pattern(self.dtype, self.fill, self.cols + 1, self.whole.device, self.fmt)
        return p[first_elem % 2:first_elem % 2 + self.cols].view(1, -1)

    def set(self, data):
        """Copy data into the interior (before set_gaps: the gaps are filled afterwards)."""
        self.t.copy_(data.to(self.t.device).view_as(self.t))
        return self

    def set_gaps(self, kind):
        """kind (rows,) int8: 0 = a row some level owns, 1 = a row between two levels, 2 = a row behind an image's last level.  The gap rows
        get the fill and are checked from now on."""
        assert kind.numel() == self.rows
        self.kind = kind.to(self.whole.device)
        rows = torch.nonzero(self.kind > 0).view(-1)
        body = bits_of(self._rows2d[self.g:self.g + self.rows])
        if self.cols % 2 == 0 or self.fill != "max":
            body[rows] = self._row_pattern(0).expand(rows.numel(), -1)
        else:
            par = ((rows + self.g) * self.cols) % 2
            p = fill_pattern(self.dtype, self.fill, self.cols + 1, self.whole.device, self.fmt)
            body[rows] = torch.where(par.view(-1, 1) == 0, p[:self.cols].view(1, -1), p[1:].view(1, -1))
        return self

    def _regions(self):
        """[(place, first row in the allocation, rows tensor or None for a contiguous block, row count)]"""
        out = [("front guard", 0, None, self.g), ("back guard", self.g + self.rows, None, self.g)]
        if self.kind is not None:
            for place, k in (("level gap", 1), ("image gap", 2)):
                rows = torch.nonzero(self.kind == k).view(-1)
                if rows.numel():
                    out.append((place, self.g, rows, rows.numel()))
        return out

    def check(self, ignore=()):
        """Raise GuardError unless both guards and every gap row hold the fill, bit for bit.  ignore: places to leave out (only the helper's
        own test uses it, to show that each place is looked at)."""
        whole = bits_of(self._rows2d)
        for place, r0, rows, cnt in self._regions():
            if place in ignore:
                continue
            got = whole[r0:r0 + cnt] if rows is None else whole[r0 + rows]
            idx = torch.arange(r0, r0 + cnt, device=whole.device) if rows is None else r0 + rows
            if self.cols % 2 == 0 or self.fill != "max":
                want = self._row_pattern(0)
            else:
                p = fill_pattern(self.dtype, self.fill, self.cols + 1, whole.device, self.fmt)
                want = torch.where(((idx * self.cols) % 2).view(-1, 1) == 0, p[:self.cols].view(1, -1), p[1:].view(1, -1))
            bad = got != want
            nbad = int(bad.sum())
            if nbad:
                first = int(torch.nonzero(bad.any(1)).view(-1)[0])
                row = int(idx[first]) - (0 if place == "front guard" else self.g + self.rows if place == "back guard" else self.g)
                col = int(torch.nonzero(bad[first]).view(-1)[0])
                raise GuardError(f"{self.name}: {place} changed: {nbad} element(s), first at row {row} (column {col}) of the "
                                 f"{'guard' if 'guard' in place else 'interior'}; fill {self.fill!r}")

    def snapshot(self):
        """Remember every bit of the allocation (inputs: guards, gaps and data must come back unchanged)."""
        self._snap = bits_of(self.whole).clone()
        return self

    def assert_unchanged(self):
        self.check()
        same = bits_of(self.whole) == self._snap
        if not bool(same.all()):
            bad = torch.nonzero(~same.view(-1)).view(-1)
            raise GuardError(f"{self.name}: input changed: {bad.numel()} element(s), first at interior row "
                             f"{int(bad[0]) // self.cols - self.g} (column {int(bad[0]) % self.cols})")


def guarded(rows, cols, dtype, device, guard_rows=None, fill="sentinel", name="tensor", fmt=None):
    """(interior view, handle): a contiguous (rows, cols) tensor -- (rows,) elements with cols=None -- inside one larger allocation whose
    guards in front and behind are each >= 512 rows and >= 4 KiB, a multiple of 256 bytes, and hold `fill` (the interior too, until it is
    written).  handle.check() compares the guards with the fill as integers.  fmt="e5m2": a one-byte tensor of e5m2 numbers (its +-max differs)."""
    h = Guarded(rows, cols, dtype, device, guard_rows, fill, name, fmt)
    return h.t, h


def gapped_geom(N, levels, gap=GUARD_MIN_ROWS):
    """An ops.Geom of `levels` [(H, W)] per image in which `gap` rows that no level owns follow every level: off[i] leaves them between
    levels, pix_per_img behind the last level of every image.  Returns (geom, kind): kind (N * pix_per_img,) int8 on the CPU, 0 = owned,
    1 = gap between two levels, 2 = gap behind an image's last level (Guarded.set_gaps)."""
    from basedet_amd import ops
    off, o = [], 0
    for h, w in levels:
        off.append(o)
        o += h * w + gap
    geom = ops.Geom(N, [h for h, _ in levels], [w for _, w in levels], off, o)
    kind = torch.ones(N, o, dtype=torch.int8)
    for i, (h, w) in enumerate(levels):
        kind[:, off[i]:off[i] + h * w] = 0
    kind[:, off[-1] + levels[-1][0] * levels[-1][1]:] = 2
    return geom, kind.view(-1)
