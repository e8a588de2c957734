"""float64 restatement (torch, CPU) of what basedet.layers.CenternetDeconv / CenterHead and csrc/center_head.hip compute.

Layouts are the reference's: activations NCHW, convolution weights OIHW, `up_sample.weight` (C_in, C_out, 4, 4) as M.ConvTranspose2d keeps
it.  Parameters are passed as a dict under the layers' names (state_dict()).

faithful=True rounds to bf16 at exactly the points where the device stores bf16: every convolution weight operand, and every stage output
(offset conv, deformable conv, norm + ReLU, up_sample, feat_conv + ReLU, the head's outputs); gradients, which the device also stores as
bf16 between stages, are rounded by the straight-through `_r` on their way back.  faithful=False is plain float64 on the fp32 masters."""
import math

import numpy as np
import torch
import torch.nn.functional as TF

import deform_conv_oracle as DO

EPS, MOMENTUM = 1e-5, 0.1


class _RoundBoth(torch.autograd.Function):
    """bf16 rounding of a value in forward and of its gradient in backward."""
    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _r(x, faithful):
    return _RoundBoth.apply(x) if faithful else x


def _w(w, faithful):
    """A weight operand: the bf16 copy the kernels multiply with (gradient passes straight through to the fp32 master)."""
    return w + (w.to(torch.bfloat16).to(w.dtype) - w).detach() if faithful else w


# ---- the fused output kernel (bd_center_head_out_fwd / _bwd) ---------------------------------------------------------------------------------
def head_out(feat, w_cls, b_cls, w_wh, b_wh, w_reg, b_reg, d_logits=None, d_wr=None):
    """feat (M, 3C) holding bf16 values; weights the fp32 masters (rounded to bf16 here, as the kernel does); biases or None.  d_logits
    (M, K) and d_wr (M, 4) (real slots only).  Returns a dict of float64 results and of S = the same sums over magnitudes."""
    f = feat.double()
    M, C = f.shape[0], f.shape[1] // 3
    ws = [w.to(torch.bfloat16).double() for w in (w_cls, w_wh, w_reg)]
    bs = [torch.zeros(w.shape[0], dtype=torch.float64) if b is None else b.double() for w, b in zip(ws, (b_cls, b_wh, b_reg))]
    tw = [f[:, i * C:(i + 1) * C] for i in range(3)]
    out = {}
    ys = [t @ w.t() + b for t, w, b in zip(tw, ws, bs)]
    Ss = [t.abs() @ w.abs().t() + b.abs() for t, w, b in zip(tw, ws, bs)]
    out["logits"], out["S_logits"] = ys[0], Ss[0]
    out["wr"], out["S_wr"] = torch.cat(ys[1:], 1), torch.cat(Ss[1:], 1)
    if d_logits is not None:
        gs = [d_logits.double(), d_wr.double()[:, :2], d_wr.double()[:, 2:4]]
        open_ = f != 0
        out["d_feat"] = torch.cat([g @ w for g, w in zip(gs, ws)], 1) * open_
        out["S_d_feat"] = torch.cat([g.abs() @ w.abs() for g, w in zip(gs, ws)], 1) * open_
        out["closed"] = ~open_
        for name, g, t in zip(("cls", "wh", "reg"), gs, tw):
            out["dw_" + name], out["S_dw_" + name] = g.t() @ t, g.abs().t() @ t.abs()
            out["db_" + name], out["S_db_" + name] = g.sum(0), g.abs().sum(0)
    return out


# ---- initialisation ------------------------------------------------------------------------------------------------------------------------------
def bilinear_stencil(k=4):
    """DeconvLayer.init_module's stencil, computed by hand: f = ceil(k / 2), c = (2 f - 1 - f % 2) / (2 f); for k = 4: f = 2, c = 0.75,
    1 - |i / 2 - 0.75| = (0.25, 0.75, 0.75, 0.25)."""
    f = math.ceil(k / 2)
    c = (2 * f - 1 - f % 2) / (2.0 * f)
    v = torch.tensor([1 - abs(i / f - c) for i in range(k)], dtype=torch.float64)
    return v[:, None] * v[None, :]


# ---- the neck ------------------------------------------------------------------------------------------------------------------------------------
def batch_norm(x, p, prefix, training):
    """(y, new running_mean, new running_var): MegEngine's BatchNorm2d -- biased variance to normalise, unbiased into the running
    statistics, momentum 0.1 in torch's convention -- which is torch's own convention."""
    rm, rv = p[prefix + ".running_mean"].double().clone(), p[prefix + ".running_var"].double().clone()
    y = TF.batch_norm(x, rm, rv, p[prefix + ".weight"].double(), p[prefix + ".bias"].double(), training=training, momentum=MOMENTUM, eps=EPS)
    return y, rm, rv


def dcn_names(modulated):
    return ("offset_mask_conv", "dcnv2") if modulated else ("offset_conv", "dcn")


def dcn_stage(x, p, prefix, modulated, faithful, om_used=None):
    """DeformConvWithOff / ModulatedDeformConvWithOff: x NCHW -> (y NCHW, om NHWC with ld channels).  om_used: sampling positions to use
    instead of the computed ones (the device's own, tests/test_deform_conv_gpu.py's composition), gradients still flowing through the
    offset convolution."""
    off, dcn = dcn_names(modulated)
    K, ld = (27, 32) if modulated else (18, 24)
    N, _, H, W = x.shape
    om = TF.conv2d(x, _w(p[f"{prefix}.{off}.weight"], faithful), p[f"{prefix}.{off}.bias"], padding=1).permute(0, 2, 3, 1)
    om = _r(torch.cat([om, torch.zeros(N, H, W, ld - K, dtype=om.dtype)], -1), faithful)
    if om_used is not None:
        om = om + (om_used - om).detach()
    y = DO.forward(x.permute(0, 2, 3, 1), om, _w(p[f"{prefix}.{dcn}.weight"], faithful).permute(0, 2, 3, 1), p[f"{prefix}.{dcn}.bias"], modulated)
    return _r(y.permute(0, 3, 1, 2), faithful), om


def deconv_layer(x, p, prefix, modulated, training=True, faithful=False, stats=None):
    """DeconvLayer.forward: dcn -> dcn_bn -> ReLU -> up_sample -> up_bn -> ReLU.  stats: a dict that receives the new running statistics."""
    y, _ = dcn_stage(x, p, prefix + ".dcn", modulated, faithful)
    y, rm, rv = batch_norm(y, p, prefix + ".dcn_bn", training)
    if stats is not None:
        stats[prefix + ".dcn_bn.running_mean"], stats[prefix + ".dcn_bn.running_var"] = rm, rv
    y = _r(torch.relu(y), faithful)
    y = _r(TF.conv_transpose2d(y, _w(p[prefix + ".up_sample.weight"], faithful), stride=2, padding=1), faithful)
    y, rm, rv = batch_norm(y, p, prefix + ".up_bn", training)
    if stats is not None:
        stats[prefix + ".up_bn.running_mean"], stats[prefix + ".up_bn.running_var"] = rm, rv
    return _r(torch.relu(y), faithful)


def neck(x, p, num_layers, modulated, training=True, faithful=False, stats=None):
    for i in range(num_layers):
        x = deconv_layer(x, p, f"deconv{i + 1}", modulated, training, faithful, stats)
    return x


# ---- the head ------------------------------------------------------------------------------------------------------------------------------------
def head_raw(x, p, faithful=False):
    """CenterHead before the sigmoid: (cls logits, wh, reg), NCHW."""
    outs = []
    for name in ("cls", "wh", "reg"):
        f = TF.conv2d(x, _w(p[name + "_head.feat_conv.weight"], faithful), p[name + "_head.feat_conv.bias"], padding=1)
        f = _r(torch.relu(f), faithful)
        outs.append(_r(TF.conv2d(f, _w(p[name + "_head.out_conv.weight"], faithful), p[name + "_head.out_conv.bias"]), faithful))
    return tuple(outs)


def head(x, p, faithful=False):
    cls, wh, reg = head_raw(x, p, faithful)
    return {"cls": torch.sigmoid(cls), "wh": wh, "reg": reg}


# ---- the losses behind the head: tests/centernet_oracle.py's focal_loss (on sigmoid(logits)) and l1_loss -----------------------------------------
def total_loss(cls_logits, wh, reg, tgt, wh_weight=0.1, reg_weight=1.0):
    """modified_focal_loss + wh_weight reg_l1_loss(wh) + reg_weight reg_l1_loss(reg) (models/det/centernet.py:165-187) from NCHW float64
    head outputs; tgt: score_map (N, K, H, W), reg_mask (N, T), index (N, T), wh / reg (N, T, 2), torch tensors."""
    import centernet_oracle as CO
    mask, index = tgt["reg_mask"].double(), tgt["index"]
    return (CO.focal_loss(torch.sigmoid(cls_logits), tgt["score_map"].double())
            + wh_weight * CO.l1_loss(wh, mask, index, tgt["wh"].double()) + reg_weight * CO.l1_loss(reg, mask, index, tgt["reg"].double()))


def double_params(p, requires_grad=False):
    return {k: v.detach().double().clone().requires_grad_(requires_grad and "running" not in k) for k, v in p.items()}


# ---- the problem the CPU and GPU tests share -----------------------------------------------------------------------------------------------------
CHANNELS, KERNELS, N, H0, W0, T = [128, 64, 64], [4, 4], 2, 3, 5, 8          # 3 x 5 -> 12 x 20
TRAIN_LR, TRAIN_STEPS = 0.02, 20      # plain SGD on one fixed batch; tests/test_center_head_cpu.py shows the float64 oracle's loss falls with it


def init_params(K, modulated, seed=0):
    """A state for CenternetDeconv(CHANNELS, KERNELS, modulated) + CenterHead(64, K): the layers' default shapes and scales, with norms,
    biases and running statistics away from their trivial values so that a dropped term shows."""
    from basedet_amd.layers import center_head as L
    rng = np.random.default_rng(seed)
    shapes = dict(L.neck_param_shapes(CHANNELS, modulated))
    shapes.update(L.head_param_shapes(CHANNELS[-1], K))
    p = {}
    for k, s in shapes.items():
        if k.endswith("up_sample.weight"):
            v = L.up_sample_init(s[0], rng)
        elif k.endswith("running_mean"):
            v = rng.normal(0, 0.1, s)
        elif k.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, s)
        elif "_bn." in k and k.endswith(".weight"):
            v = rng.uniform(0.6, 1.4, s)
        elif k.endswith(".bias"):
            v = rng.normal(0, 0.1, s) + (-math.log(9.0) if k == "cls_head.out_conv.bias" else 0.0)
        else:
            v = rng.standard_normal(s) * math.sqrt(1.0 / (s[1] * s[2] * s[3]))
        p[k] = torch.from_numpy(np.asarray(v, np.float32))
    return p


def problem(K, seed=0):
    """(x NCHW holding bf16 values, targets as torch tensors) on the 12 x 20 map; the targets come from tests/centernet_oracle.py."""
    import centernet_oracle as CO
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(N, CHANNELS[0], H0, W0, generator=g).to(torch.bfloat16).float()
    H, W = 4 * H0, 4 * W0
    gt, num = CO.target_problem(N, K, H, W, T, seed=seed)
    ref = CO.targets(gt, num, K, H, W, T, CO.BOX_SCALE, CO.MIN_OVERLAP)
    assert ref["reg_mask"].sum() > 0 and CO.radius_margin_ulps(ref["radius"]).min() > 1
    tgt = {k: torch.from_numpy(np.asarray(ref[k])) for k in ("score_map", "wh", "reg", "reg_mask", "index")}
    tgt["index"] = tgt["index"].long()
    return x, gt, num, tgt


def loss_and_grads(x, p, tgt, modulated, faithful):
    """(loss, {name: gradient}) of the whole chain in float64."""
    q = double_params(p, requires_grad=True)
    f = neck(x.double(), q, len(KERNELS), modulated, True, faithful)
    loss = total_loss(*head_raw(f, q, faithful), tgt)
    names = [k for k in q if q[k].requires_grad]
    grads = torch.autograd.grad(loss, [q[k] for k in names])
    return float(loss.detach()), dict(zip(names, grads))
