"""The reference's CenterNet tail (models/det/centernet.py) restated for the tests of csrc/centernet.hip.

targets: numpy float32 where the reference's tensors are float32 (boxes, centres, radius), float64 for the Gaussian window, which is
then cast, as gaussian2D / draw_gaussian do.  Losses and decode: float64 on the literal formulas (torch autograd for the gradients).
Choices the reference leaves open are the library's (include/basedet_hip.h): a centre cell outside the map -> reg_mask 0, index 0,
nothing drawn; more than T boxes -> the first T; decode ties -> class ascending, then pixel ascending."""
import numpy as np
import torch

F32 = np.float32
CLIP_LO, CLIP_HI = 1e-12, float(F32(1 - 1e-7))


def radius_f32(w, h, mo):
    """get_gaussian_radius (centernet.py:394-423) before the clip and the truncation: float32 arrays in, float32 out."""
    w, h = np.asarray(w, F32), np.asarray(h, F32)
    omm, opm, m2, mm1, a34 = F32(1 - mo), F32(1 + mo), F32(-2 * mo), F32(mo - 1), F32(4 * (4 * mo))
    s = h + w
    r1 = (s + np.sqrt(s * s - F32(4) * (w * h * omm / opm))) / F32(2)
    b2 = F32(2) * s
    r2 = (b2 + np.sqrt(b2 * b2 - F32(16) * (omm * w * h))) / F32(2)
    b3 = m2 * s
    r3 = (b3 + np.sqrt(b3 * b3 - a34 * (mm1 * w * h))) / F32(2)
    out = np.minimum(np.minimum(r1, r2), r3)
    assert out.dtype == F32
    return out


def targets(gt_boxes, num_gt, K, H, W, T, box_scale, mo):
    """-> dict: score_map (N, K, H, W) f32, wh / reg (N, T, 2) f32, reg_mask (N, T) f32, index (N, T) i32, num_pos float,
    radius: the float32 radii (before clip / truncation) of every slot that draws."""
    N = gt_boxes.shape[0]
    smap = np.zeros((N, K, H, W), F32)
    wh, reg = np.zeros((N, T, 2), F32), np.zeros((N, T, 2), F32)
    mask, index = np.zeros((N, T), F32), np.zeros((N, T), np.int32)
    radii = []
    for n in range(N):
        b = np.asarray(gt_boxes[n, :int(num_gt[n])], F32)
        keep = ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)
        b = b[keep][:T]
        box = b[:, :4] * F32(box_scale)
        cls = b[:, 4].astype(np.int32) - 1
        ctr = np.stack([(box[:, 0] + box[:, 2]) / F32(2), (box[:, 1] + box[:, 3]) / F32(2)], 1)
        bw, bh = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
        rad = radius_f32(bw, bh, mo)
        for t in range(b.shape[0]):
            wh[n, t] = (bw[t], bh[t])
            fx, fy = ctr[t]
            if not (-1 < fx < W and -1 < fy < H):
                continue
            cx, cy = int(fx), int(fy)                           # truncation, as astype("int32")
            index[n, t], mask[n, t] = cy * W + cx, 1
            reg[n, t] = (fx - F32(cx), fy - F32(cy))
            if not 0 <= cls[t] < K:
                continue
            radii.append(rad[t])
            r = int(max(rad[t], F32(0)))
            sigma = (2 * r + 1) / 6
            for y in range(max(cy - r, 0), min(cy + r + 1, H)):
                for x in range(max(cx - r, 0), min(cx + r + 1, W)):
                    v = F32(np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sigma * sigma)))
                    smap[n, cls[t], y, x] = max(smap[n, cls[t], y, x], v)
    return dict(score_map=smap, wh=wh, reg=reg, reg_mask=mask, index=index, num_pos=float((smap == 1).sum()),
                radius=np.asarray(radii, F32))


def radius_margin_ulps(radii):
    """Distance of every (positive) float32 radius from the nearest integer, in units of its own float32 spacing."""
    r = np.asarray(radii, np.float64)
    r = r[r > 0]
    return np.abs(r - np.rint(r)) / np.spacing(r.astype(F32)).astype(np.float64)


def focal_loss(pred, gt):
    """modified_focal_loss (centernet.py:218-242) on torch float64 probabilities; differentiable."""
    pos = (gt == 1).double()
    neg = (gt < 1).double()
    p = torch.clip(pred, CLIP_LO, CLIP_HI)
    pos_loss = (torch.log(p) * (1 - p) ** 2 * pos).sum()
    neg_loss = (torch.log(1 - p) * p ** 2 * (1 - gt) ** 4 * neg).sum()
    n = pos.sum()
    return -neg_loss if n == 0 else -(pos_loss + neg_loss) / n


def focal_from_logits(x, gt):
    """loss, d loss / d logit and the clip mask, float64, from logits x (any shape) and gt of the same shape."""
    x = x.double().clone().requires_grad_(True)
    p = torch.sigmoid(x)
    loss = focal_loss(p, gt.double())
    loss.backward()
    pd = p.detach()
    return float(loss.detach()), x.grad, (pd < CLIP_LO) | (pd > CLIP_HI)


def l1_loss(output, mask, index, target):
    """reg_l1_loss (centernet.py:208-215): output (N, C, H, W), mask (N, T), index (N, T) int, target (N, T, C); differentiable."""
    n, c = output.shape[:2]
    fm = output.reshape(n, c, -1).permute(0, 2, 1)
    pred = torch.gather(fm, 1, index.long().unsqueeze(-1).expand(-1, -1, c))
    m = mask.unsqueeze(2).expand_as(pred).to(output.dtype)
    return (pred * m - target * m).abs().sum() / (m.sum() + 1e-4)


def decode(scores, wh, reg, k):
    """CenterNetDecoder.decode: scores (B, K, H, W) float32 (already sigmoid), wh / reg (B, H*W, 2) float (reg may be None) ->
    classes (B, k), pixel (B, k), scores (B, k) float32, boxes (B, k, 4) float64.  Order: score descending, class, pixel ascending."""
    B, K, H, W = scores.shape
    s = np.asarray(scores, F32)
    pad = np.full((B, K, H + 2, W + 2), -np.inf, F32)
    pad[:, :, 1:-1, 1:-1] = s
    mx = np.max(np.stack([pad[:, :, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]), 0)
    kept = np.where(mx == s, s, F32(0)).reshape(B, K * H * W)
    cls, pix, sc, boxes = (np.zeros((B, k), np.int64), np.zeros((B, k), np.int64), np.zeros((B, k), F32), np.zeros((B, k, 4)))
    for b in range(B):
        order = np.argsort(-kept[b].astype(np.float64), kind="stable")[:k]        # stable: flat index = class * HW + pixel ascending
        cls[b], pix[b], sc[b] = order // (H * W), order % (H * W), kept[b][order]
        w2 = np.asarray(wh[b], np.float64)[pix[b]] / 2
        off = np.asarray(reg[b], np.float64)[pix[b]] if reg is not None else np.full((k, 2), 0.5)
        c = np.stack([pix[b] % W, pix[b] // W], 1) + off
        boxes[b] = np.concatenate([c - w2, c + w2], 1)
    return cls, pix, sc, boxes


# ---- the problems the CPU and GPU tests share ---------------------------------------------------------------------------------------------
BOX_SCALE, MIN_OVERLAP = 0.25, 0.7
TARGET_SHAPES = [(2, 3, 12, 20, 8), (1, 1, 5, 7, 4), (2, 80, 128, 128, 128), (3, 20, 33, 65, 16)]        # (N, K, H, W, T)


def hand_boxes(K, H, W):
    """Hand cases in map cells (x1, y1, x2, y2, label), in slot order: a zero-width box (dropped), label 0 (slot kept, nothing drawn),
    windows clipped at the left / top and at the right / bottom edge, a radius-0 box, two boxes in one cell, two same-class boxes
    whose discs overlap."""
    c2 = min(2, K)
    return np.asarray([
        [3, 1, 3, 4, 1],
        [1, 1, 4, 4, 0],
        [-2.5, -2.5, 3.5, 3.5, 1],
        [W - 3.5, H - 3.5, W + 2.5, H + 2.5, 1],
        [1.25, 1.25, 2.75, 2.75, c2],
        [3.0, 2.0, 5.0, 4.0, 1], [3.25, 2.25, 5.25, 4.25, 1],
        [1.0, 0.5, 5.0, 4.5, c2], [3.0, 0.5, 7.0, 4.5, c2],
    ], np.float64)


def target_problem(N, K, H, W, T, seed=0):
    """gt_boxes (N, G, 5) float32 in input pixels and num_gt (N,): image 0 holds the hand cases and random boxes, more than T in all;
    image 1 (if any) holds none; the others T // 2 random boxes.  Rows past num_gt hold NaN."""
    rng = np.random.default_rng(seed)

    def rand(n):
        cx, cy = rng.uniform(0, W, n), rng.uniform(0, H, n)
        w, h = min(H, W) ** rng.random(n), min(H, W) ** rng.random(n)
        b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, rng.integers(1, K + 1, n)], 1)
        return b
    hand = hand_boxes(K, H, W)
    G = max(T + 4, len(hand) + 4)
    gt = np.full((N, G, 5), np.nan, F32)
    num = np.zeros(N, np.int32)
    for n in range(N):
        if n == 0:
            b = np.concatenate([hand, rand(G - len(hand))], 0)
        elif n == 1:
            b = np.zeros((0, 5))
        else:
            b = rand(T // 2)
        b[:, :4] = np.round(b[:, :4] / BOX_SCALE * 4) / 4            # input pixels, on a quarter-pixel grid
        gt[n, :len(b)] = b
        num[n] = len(b)
    return gt, num
