"""float64 restatement of the deformable convolution that csrc/deform_conv.hip computes (include/basedet_hip.h, bd_deform_conv_fwd).

x (N, H, W, Cin); om (N, H, W, ld): channel 2k = dy, 2k + 1 = dx of tap k = 3 i + j, (modulated) 18 + k = mask logit; w (Cout, 3, 3, Cin);
bias (Cout,).  Output pixel (y, x), tap (i, j) samples at h = y - 1 + i + dy, w = x - 1 + j + dx with explicit floor / corner gathers; the
`inside` factor (-1 < h < H and -1 < w < W) is a constant of the graph, so every gradient vanishes outside; a corner counts only inside the
image.  Gradients come from autograd: those of the floor formula, i.e. the right-hand derivative at an integer coordinate.

S (the scale the kernels' rounding errors are measured against, as tests/util.py's conv_ref_* return it) is the same sum with every term
replaced by its magnitude: |x|, |w|, |bias|, |dy| for the forward, d_x, d_w and d_bias (the bilinear and mask factors are >= 0); for d_om,
whose terms carry the signs of d(weight)/d(coordinate), sum_ci G |d weight_c / d h| |v_c| over the four corners with G = |dy| |w|."""
import torch


def _corners(x, h, w):
    """Corner values (zero outside the image), fractions and the inside factor at positions h, w (N, H, W); x (N, H, W, C)."""
    N, H, W, _ = x.shape
    inside = ((h > -1) & (h < H) & (w > -1) & (w < W)).to(x.dtype)
    h0, w0 = torch.floor(h).detach(), torch.floor(w).detach()
    lh, lw = h - h0, w - w0
    n = torch.arange(N).view(N, 1, 1).expand(N, H, W)

    def at(yy, xx):
        ok = ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).to(x.dtype)
        return x[n, yy.clamp(0, H - 1).long(), xx.clamp(0, W - 1).long()] * ok.unsqueeze(-1)
    return (at(h0, w0), at(h0, w0 + 1), at(h0 + 1, w0), at(h0 + 1, w0 + 1)), lh, lw, inside


def _positions(om, k, H, W):
    ys = torch.arange(H, dtype=om.dtype).view(1, H, 1)
    xs = torch.arange(W, dtype=om.dtype).view(1, 1, W)
    return ys - 1 + k // 3 + om[..., 2 * k], xs - 1 + k % 3 + om[..., 2 * k + 1]


def columns(x, om, modulated):
    """col (N, H, W, 9, Cin) = m * bilinear sample of x for every tap."""
    _, H, W, _ = x.shape
    cols = []
    for k in range(9):
        h, w = _positions(om, k, H, W)
        (v00, v01, v10, v11), lh, lw, inside = _corners(x, h, w)
        lh, lw = lh.unsqueeze(-1), lw.unsqueeze(-1)
        val = inside.unsqueeze(-1) * ((1 - lh) * (1 - lw) * v00 + (1 - lh) * lw * v01 + lh * (1 - lw) * v10 + lh * lw * v11)
        m = torch.sigmoid(om[..., 18 + k]) if modulated else torch.ones_like(h)
        cols.append(m.unsqueeze(-1) * val)
    return torch.stack(cols, dim=3)


def forward(x, om, w, bias, modulated):
    col = columns(x, om, modulated)
    return torch.einsum("nhwkc,okc->nhwo", col, w.reshape(w.shape[0], 9, -1)) + bias


def _s_dom(x, om, w, dy, modulated):
    """Sum of the magnitudes of the terms of d_om (module docstring)."""
    N, H, W, _ = x.shape
    xa = x.abs()
    G = torch.einsum("nhwo,okc->nhwkc", dy.abs(), w.abs().reshape(w.shape[0], 9, -1))
    S = torch.zeros_like(om)
    for k in range(9):
        h, ww = _positions(om, k, H, W)
        (a00, a01, a10, a11), lh, lw, inside = _corners(xa, h, ww)
        lh, lw = lh.unsqueeze(-1), lw.unsqueeze(-1)
        m = torch.sigmoid(om[..., 18 + k]) if modulated else torch.ones_like(h)
        g = G[:, :, :, k]
        S[..., 2 * k] = m * inside * (g * ((a00 + a10) * (1 - lw) + (a01 + a11) * lw)).sum(-1)
        S[..., 2 * k + 1] = m * inside * (g * ((a00 + a01) * (1 - lh) + (a10 + a11) * lh)).sum(-1)
        if modulated:
            val = (1 - lh) * (1 - lw) * a00 + (1 - lh) * lw * a01 + lh * (1 - lw) * a10 + lh * lw * a11
            S[..., 18 + k] = m * (1 - m) * inside * (g * val).sum(-1)
    return S


def oracle(x, om, w, bias, dy, modulated):
    """Everything the kernels produce, float64: dict(y, d_x, d_om, d_w, d_b) and S_* of each.  Operands: any float dtype, shapes of the
    module docstring; dy (N, H, W, Cout)."""
    x, om, w, bias, dy = (t.detach().double().cpu() for t in (x, om, w, bias, dy))
    out = {}
    leaves = [t.clone().requires_grad_(True) for t in (x, om, w, bias)]
    y = forward(*leaves, modulated)
    out["y"] = y.detach()
    out["d_x"], out["d_om"], out["d_w"], out["d_b"] = torch.autograd.grad(y, leaves, dy)
    leaves = [x.abs().requires_grad_(True), om, w.abs().requires_grad_(True), bias.abs().requires_grad_(True)]
    ya = forward(*leaves, modulated)
    out["S_y"] = ya.detach()
    out["S_d_x"], out["S_d_w"], out["S_d_b"] = torch.autograd.grad(ya, [leaves[0], leaves[2], leaves[3]], dy.abs())
    out["S_d_om"] = _s_dom(x, om, w, dy, modulated)
    return out
