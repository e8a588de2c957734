"""float64 restatement (torch, CPU) of what basedet.layers.ConvBNSiLU / YOLOXHead and the bd_bn_silu_* kernels compute, differentiated with
torch.autograd.

Layouts are the reference's: activations NCHW, convolution weights OIHW, norm vectors (C,).  Parameters are passed as a dict under the
layers' names (state_dict()).

faithful=True rounds to bf16 at exactly the points where the device stores bf16: every convolution weight operand, every convolution
output y, every norm + SiLU output z, the predictors' outputs; gradients, which the device also stores as bf16 between stages, are rounded
by the straight-through `_r` on their way back.  faithful=False is plain float64 on the fp32 masters."""
import numpy as np
import torch
import torch.nn.functional as TF

EPS, MOMENTUM = 1e-3, 0.03
STRIDES = (8, 16, 32)


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


# ---- SiLU, by formula (numpy float64): what the kernel tests compare with ------------------------------------------------------------------------
def sigmoid_pair(u):
    """(sigma(u), sigma(-u)) without overflow and without 1 - sigma."""
    u = np.asarray(u, np.float64)
    e = np.exp(-np.abs(u))
    inv = 1.0 / (1.0 + e)
    return np.where(u >= 0, inv, e * inv), np.where(u >= 0, e * inv, inv)


def silu(u):
    return np.asarray(u, np.float64) * sigmoid_pair(u)[0]


def silu_grad(u):
    """d silu / du = sigma(u) (1 + u sigma(-u))."""
    s, sm = sigmoid_pair(u)
    return s * (1.0 + np.asarray(u, np.float64) * sm)


def bn_silu_fwd(y, mean, inv_std, gamma, beta):
    """z (float64) from bf16-valued y (M, C) and the fp32 statistics / parameters the kernel is handed."""
    u = gamma.astype(np.float64) * ((y.astype(np.float64) - mean.astype(np.float64)) * inv_std.astype(np.float64)) + beta.astype(np.float64)
    return silu(u), u


def bn_silu_bwd(g, y, mean, inv_std, gamma, beta, dgamma=None, dbeta=None):
    """(g_u, xhat, dgamma, dbeta, gy) in float64; gy from the dgamma / dbeta given (the kernel's own) or from the float64 sums."""
    g, y = g.astype(np.float64), y.astype(np.float64)
    xh = (y - mean.astype(np.float64)) * inv_std.astype(np.float64)
    u = gamma.astype(np.float64) * xh + beta.astype(np.float64)
    gu = g * silu_grad(u)
    dg, db = (gu * xh).sum(0), gu.sum(0)
    M = y.shape[0]
    dgu = dg if dgamma is None else dgamma.astype(np.float64)
    dbu = db if dbeta is None else dbeta.astype(np.float64)
    gy = gamma.astype(np.float64) * inv_std.astype(np.float64) * (gu - dbu / M - xh * dgu / M)
    return gu, xh, dg, db, gy


# ---- the layers ----------------------------------------------------------------------------------------------------------------------------------
def conv_bn_silu(x, p, prefix, k, stride=1, training=True, faithful=False, stats=None, eps=EPS, momentum=MOMENTUM):
    """Conv2d(bias=False, norm="BN", activation="silu"): biased batch variance to normalise, unbiased into the running statistics
    (MegEngine's BatchNorm2d = torch's convention with momentum 1 - 0.97).  stats: a dict that receives the new running statistics."""
    pre = prefix + "." if prefix else ""
    y = _r(TF.conv2d(x, _w(p[pre + "weight"], faithful), None, stride=stride, padding=k // 2), faithful)
    rm, rv = p[pre + "norm.running_mean"].detach().double().clone(), p[pre + "norm.running_var"].detach().double().clone()
    u = TF.batch_norm(y, rm, rv, p[pre + "norm.weight"], p[pre + "norm.bias"], training=training, momentum=momentum, eps=eps)
    if stats is not None:
        stats[pre + "norm.running_mean"], stats[pre + "norm.running_var"] = rm, rv
    return _r(u * torch.sigmoid(u), faithful)


def head(feats, p, training=True, faithful=False, stats=None):
    """YOLOXHead.forward: per-level NCHW inputs -> (logits, offsets, objs) lists, NCHW."""
    logits, offsets, objs = [], [], []
    for l, x in enumerate(feats):
        s = conv_bn_silu(x, p, f"stems.{l}", 1, 1, training, faithful, stats)
        c = r = s
        for i in range(2):
            c = conv_bn_silu(c, p, f"cls_convs.{l}.{i}", 3, 1, training, faithful, stats)
            r = conv_bn_silu(r, p, f"reg_convs.{l}.{i}", 3, 1, training, faithful, stats)
        logits.append(_r(TF.conv2d(c, _w(p[f"cls_preds.{l}.weight"], faithful), p[f"cls_preds.{l}.bias"]), faithful))
        offsets.append(_r(TF.conv2d(r, _w(p[f"reg_preds.{l}.weight"], faithful), p[f"reg_preds.{l}.bias"]), faithful))
        objs.append(_r(TF.conv2d(r, _w(p[f"obj_preds.{l}.weight"], faithful), p[f"obj_preds.{l}.bias"]), faithful))
    return logits, offsets, objs


def pack(logits, offsets, objs):
    """The three lists -> (cls (N, P, K), box_obj (N, P, 5)): level after level, row-major inside a level."""
    N = logits[0].shape[0]
    f = lambda t: t.permute(0, 2, 3, 1).reshape(N, t.shape[2] * t.shape[3], t.shape[1])
    return torch.cat([f(t) for t in logits], 1), torch.cat([torch.cat([f(o), f(b)], 2) for o, b in zip(offsets, objs)], 1)


def double_params(p, requires_grad=False):
    return {k: v.detach().double().clone().requires_grad_(requires_grad and "running" not in k) for k, v in p.items()}


# ---- the YOLOX losses on torch tensors, the assignment taken as given (tests/yolox_oracle.py losses(), restated for autograd inputs) -------------
def yolox_losses(cls, bo, pts, stride, gt, matched, iou_t, nf, use_l1):
    """cls (N, P, K), bo (N, P, 5) float64 tensors with history; pts (P, 2), stride (P,), gt (N, G, 5) xyxy + 1-based label; matched (N, P)
    int, iou_t (N, P).  -> [5 * iou, obj, cls, l1] float64 scalars."""
    K = cls.shape[2]
    pts, st, gt = (torch.as_tensor(np.asarray(a), dtype=torch.float64) for a in (pts, stride, np.nan_to_num(np.asarray(gt, np.float64), nan=0.0)))
    m = torch.as_tensor(np.asarray(matched)).long()
    fg = m >= 0
    nf = max(float(nf), 1.0)
    n_idx = torch.nonzero(fg)[:, 0]
    g = gt[n_idx, m[fg]]
    raw = bo[..., :4][fg]
    p, s = pts.expand(fg.shape[0], -1, -1)[fg], st.expand(fg.shape[0], -1)[fg]
    xc, yc = raw[:, 0] * s + p[:, 0], raw[:, 1] * s + p[:, 1]
    w, h = s * torch.exp(raw[:, 2]), s * torch.exp(raw[:, 3])
    x1, y1, x2, y2 = xc - w / 2, yc - h / 2, xc + w / 2, yc + h / 2
    iw = torch.clamp(torch.minimum(x2, g[:, 2]) - torch.maximum(x1, g[:, 0]), min=0)
    ih = torch.clamp(torch.minimum(y2, g[:, 3]) - torch.maximum(y1, g[:, 1]), min=0)
    inter = iw * ih
    union = (x2 - x1) * (y2 - y1) + (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) - inter
    iou = torch.clamp(inter / union, min=0)
    bce = TF.binary_cross_entropy_with_logits
    l_iou = 5 * (1 - iou ** 2).sum() / nf
    l_obj = bce(bo[..., 4], fg.double(), reduction="sum") / nf
    tgt = torch.zeros((int(fg.sum()), K), dtype=torch.float64)
    lab = g[:, 4].long() - 1
    ok = (lab >= 0) & (lab < K)
    tgt[torch.nonzero(ok)[:, 0], lab[ok]] = torch.as_tensor(np.asarray(iou_t), dtype=torch.float64)[fg][ok]
    l_cls = bce(cls[fg], tgt, reduction="sum") / nf
    if use_l1:
        t = torch.stack([((g[:, 0] + g[:, 2]) / 2 - p[:, 0]) / s, ((g[:, 1] + g[:, 3]) / 2 - p[:, 1]) / s,
                         torch.log((g[:, 2] - g[:, 0]) / s + 1e-8), torch.log((g[:, 3] - g[:, 1]) / s + 1e-8)], 1)
        l_l1 = (raw - t).abs().sum() / nf
    else:
        l_l1 = torch.zeros((), dtype=torch.float64)
    return [l_iou, l_obj, l_cls, l_l1]


# ---- the problems the CPU and GPU tests share ----------------------------------------------------------------------------------------------------
N, SIZES = 2, [(8, 12), (4, 6), (2, 3)]          # P = 126; a 64 x 96 image at strides 8 / 16 / 32
IN_CHANNELS, MID = [8, 16, 24], 8                # the smallest widths bd_conv2d_* take (multiples of 8), three different inputs


def head_state(K, seed=0):
    """A YOLOXHead state with every norm away from its initial values, so that each parameter matters."""
    from basedet_amd.layers.yolox_head import head_param_shapes
    g = torch.Generator().manual_seed(100 + seed + K)
    prior = -float(np.log((1 - 0.01) / 0.01))
    p = {}
    for k, shape in head_param_shapes(K, IN_CHANNELS, MID).items():
        if k.endswith("norm.weight"):
            v = 1.0 + 0.3 * torch.randn(shape, generator=g)
        elif k.endswith("norm.bias") or k.endswith("running_mean"):
            v = 0.3 * torch.randn(shape, generator=g)
        elif k.endswith("running_var"):
            v = 0.5 + torch.rand(shape, generator=g)
        elif k.endswith(".bias"):
            v = (prior if k.startswith(("cls_preds", "obj_preds")) else 0.0) + 0.1 * torch.randn(shape, generator=g)
        else:
            v = torch.randn(shape, generator=g) * (1.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        p[k] = v.float()
    return p


def head_inputs(seed=0):
    g = torch.Generator().manual_seed(7 + seed)
    return [torch.randn(N, c, h, w, generator=g).to(torch.bfloat16).float() for c, (h, w) in zip(IN_CHANNELS, SIZES)]


def head_loss_and_grads(feats, p0, K, gt, matched, iou_t, nf, use_l1, faithful):
    """(four losses, {name: parameter gradient}, [d_feats]) of the sum of the four losses through the head."""
    import yolox_oracle as YO
    p = double_params(p0, True)
    xs = [x.double().clone().requires_grad_(True) for x in feats]
    cls, bo = pack(*head(xs, p, True, faithful))
    pts, _, st = YO.points(SIZES, STRIDES)
    parts = yolox_losses(cls, bo, pts, st, gt, matched, iou_t, nf, use_l1)
    sum(parts).backward()
    return (np.array([float(v.detach()) for v in parts]), {k: v.grad.detach() for k, v in p.items() if v.requires_grad},
            [x.grad.detach() for x in xs])
