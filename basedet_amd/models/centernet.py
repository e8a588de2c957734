"""CenterNet after the network's last convolution, on the kernels of csrc/centernet.hip -- the reference's names and signatures
(models/det/centernet.py): ground truth (`centernet_ground_truth`, CenterNetGT), `modified_focal_loss`, `reg_l1_loss`, `gather_feature`
and `CenterNetDecoder`.  The deconvolution neck and CenterHead are layers (basedet_amd/layers/center_head.py); the
res5-only trunk and the CenterNet class itself are the next step.

Tensors are the reference's: NCHW fp32 on the HIP device (host tensors raise: there is no CPU path).  The kernels read the head's
convolution output -- pixel-major bf16 LOGITS -- so the functions that take probabilities, as the reference's do, turn them back into
logits and round them to bf16 on the way in; a model step hands the convolution output to basedet_amd.ops directly.

What runs where: `centernet_ground_truth`, the two losses (value and gradient, through a torch.autograd.Function) and
`CenterNetDecoder.decode` are one HIP entry each.  `gather_feature`, `pseudo_nms` and `topk_score` are the reference's stand-alone
helpers, kept as device tensor indexing / pooling for callers that use them on their own (decode does not: its kernel fuses them).
CenterNetGT's per-image methods and `transform_boxes` / `generate_src_and_dst` are host numpy, as gaussian2D and transform_boxes
are in the reference."""
import numpy as np
import torch
import torch.nn.functional as TF

from basedet_amd import ops
from basedet_amd._lib import BasedetHipError

__all__ = ["CenterNetGT", "CenterNetDecoder", "centernet_ground_truth", "gather_feature", "modified_focal_loss", "reg_l1_loss"]


def _dev(*tensors):
    for t in tensors:
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise BasedetHipError("basedet_amd.models.centernet needs tensors on a HIP device; there is no CPU fallback")


def _ld(K):
    return (K + 7) // 8 * 8


def _to_pm(x, ld):
    """(N, C, H, W) fp32 -> pixel-major bf16 (N*H*W, ld), the slots >= C zero."""
    n, c, h, w = x.shape
    out = torch.zeros((n * h * w, ld), dtype=torch.bfloat16, device=x.device)
    out[:, :c] = x.permute(0, 2, 3, 1).reshape(n * h * w, c)
    return out


def _from_pm(t, n, c, h, w):
    return t[:, :c].float().reshape(n, h, w, c).permute(0, 3, 1, 2)


def centernet_ground_truth(gt_boxes, num_gt, cfg):
    """CenterNet.get_ground_truth (centernet.py:74-127): gt_boxes fp32 (N, G, 5) xyxy + 1-based label, num_gt int32 (N,) -- the img_info
    count of the reference -- and the config -> gt_dict {score_map (N, K, H, W), wh, reg (N, T, 2), reg_mask (N, T), index int32 (N, T)}
    plus num_pos (1,), the number of map elements equal to 1.  score_map is a view of the kernel's pixel-major (N, H*W, K) map."""
    _dev(gt_boxes, num_gt)
    m = cfg.MODEL
    K, T = int(cfg.DATA.NUM_CLASSES), int(m.HEAD.TENSOR_DIM)
    H, W = (int(v) for v in m.OUTPUT_SIZE)
    out = ops.centernet_targets(gt_boxes.float().contiguous(), num_gt.to(torch.int32).contiguous(), K, H, W, T, 1 / m.HEAD.DOWN_SCALE,
                                m.HEAD.MIN_OVERLAP)
    out["score_map"] = out["score_map"].view(gt_boxes.shape[0], H, W, K).permute(0, 3, 1, 2)
    return out


def gather_feature(fmap, index, mask=None, use_transform=False):
    """centernet.py:189-205: rows `index` (B, T) of fmap (B, P, C) -- or of an NCHW map with use_transform -- optionally only the rows
    where mask is set, flattened to (-1, C)."""
    _dev(fmap, index, mask)
    if use_transform:
        fmap = fmap.flatten(2).transpose(1, 2)
    C = fmap.shape[-1]
    rows = torch.gather(fmap, 1, index.long().unsqueeze(-1).expand(-1, -1, C))
    if mask is None:
        return rows
    return rows[mask.bool()].reshape(-1, C)


class _Focal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt):
        n, k, h, w = pred.shape
        ld = _ld(k)
        p = pred.float()
        logits = _to_pm(torch.log(p) - torch.log1p(-p), ld)
        gmap = gt.float().permute(0, 2, 3, 1).reshape(n * h * w, k).contiguous()
        num_pos = (gmap == 1).sum().float().reshape(1)
        loss = torch.zeros(1, dtype=torch.float32, device=pred.device)
        d = torch.empty_like(logits)
        ops.centernet_focal_fwd_bwd(logits, gmap, n * h * w, k, ld, num_pos, 1.0, 1.0, loss, d)
        den = p * (1 - p)                       # d logit / d p = 1 / (p (1 - p)); the kernel's gradient is 0 where p is 0 or 1 (clipped)
        g = _from_pm(d, n, k, h, w)
        ctx.save_for_backward(torch.where(den > 0, g / den, torch.zeros_like(g)))
        ctx.dtype = pred.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        return (g * gout).to(ctx.dtype), None


def modified_focal_loss(pred, gt):
    """centernet.py:218-242: pred the head's probabilities (N, K, H, W), gt the score map."""
    if pred.shape != gt.shape or pred.dim() != 4:
        raise ValueError("modified_focal_loss: pred and gt are (N, K, H, W) tensors of one shape")
    _dev(pred, gt)
    return _Focal.apply(pred, gt)


class _RegL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, mask, index, target):
        n, c, h, w = output.shape
        t = index.shape[1]
        pm = _to_pm(output.float(), 8)
        loss = torch.zeros(1, dtype=torch.float32, device=output.device)
        d = torch.empty_like(pm)
        ops.centernet_l1_fwd_bwd(pm, 8, 0, index.to(torch.int32).contiguous(), mask.float().contiguous(), target.float().contiguous(),
                                 n, h, w, t, 1.0, 1.0, loss, d)
        ctx.save_for_backward(_from_pm(d, n, c, h, w))
        ctx.dtype = output.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        return (g * gout).to(ctx.dtype), None, None, None


def reg_l1_loss(output, mask, index, target):
    """centernet.py:208-215: output (N, 2, H, W), mask (N, T), index (N, T), target (N, T, 2)."""
    if output.shape[1] != 2 or tuple(target.shape) != tuple(index.shape) + (2,) or mask.shape != index.shape:
        raise ValueError("reg_l1_loss: output (N, 2, H, W), mask and index (N, T), target (N, T, 2)")
    _dev(output, mask, index, target)
    return _RegL1.apply(output, mask, index, target)


class CenterNetDecoder:

    @staticmethod
    def decode(fmap, wh, reg=None, cat_spec_wh=False, K=100):
        """centernet.py:247-291: fmap the head's probabilities (B, C, H, W), wh / reg (B, 2, H, W) -> (bboxes (B, K, 4), scores (B, K, 1),
        clses (B, K, 1) float32).  Ties come out by class, then pixel (bd_centernet_decode)."""
        if cat_spec_wh:
            raise ValueError("CenterNetDecoder.decode: cat_spec_wh=True (a wh pair per class) is not built")
        b, c, h, w = fmap.shape
        if wh.shape[1] != 2 or (reg is not None and reg.shape[1] != 2):
            raise ValueError("CenterNetDecoder.decode: wh and reg have two channels")
        if not 0 < K <= min(2048, h * w):
            raise ValueError(f"CenterNetDecoder.decode: K={K} must lie in 1..min(2048, H*W)")
        _dev(fmap, wh, reg)
        ld = _ld(c)
        p = fmap.float()
        logits = _to_pm(torch.log(p) - torch.log1p(-p), ld)
        whp = _to_pm(wh.float(), 8)
        regp = _to_pm(reg.float(), 8) if reg is not None else None
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=fmap.device)
        boxes, scores = f(b, K, 4), f(b, K)
        classes = torch.empty((b, K), dtype=torch.int32, device=fmap.device)
        ws = torch.empty(ops.centernet_decode_workspace_bytes(b, c, h, w), dtype=torch.uint8, device=fmap.device)
        ops.centernet_decode(logits, ld, whp, 8, 0, regp, 8, 0, b, c, h, w, K, boxes, scores, classes, ws)
        return boxes, scores.reshape(b, K, 1), classes.float().reshape(b, K, 1)

    @staticmethod
    def transform_boxes(boxes, center, size, output_size, scale=1):
        """centernet.py:293-311 on the host: the affine map of three point pairs (cv2.getAffineTransform(dst, src)) solved with
        numpy.linalg, applied to the box corners."""
        if isinstance(boxes, torch.Tensor):
            boxes = boxes.detach().cpu().numpy()
        boxes = np.asarray(boxes).reshape(-1, 4)
        src, dst = CenterNetDecoder.generate_src_and_dst(center, size, output_size)
        a = np.column_stack((np.float32(dst).astype(np.float64), np.ones(3)))
        trans = np.linalg.solve(a, np.float32(src).astype(np.float64)).T            # (2, 3): trans @ (x, y, 1) of dst = src
        pts = boxes.reshape(-1, 2).astype(np.float64)
        return (pts @ trans[:, :2].T + trans[:, 2]).reshape(-1, 4)

    @staticmethod
    def pseudo_nms(fmap, pool_size=3):
        """centernet.py:313-325: keep the elements that equal the maximum of their pool_size window, zero the others."""
        _dev(fmap)
        f = fmap.float()
        peak = TF.max_pool2d(f, pool_size, stride=1, padding=(pool_size - 1) // 2) == f
        return f * peak.float()

    @staticmethod
    def topk_score(scores, K=40):
        """centernet.py:327-352: the K best per class plane, then the K best of those per image -> (scores, pixel index, class, y, x),
        each (batch, K)."""
        _dev(scores)
        b, c, h, w = scores.shape
        per_cls, pix = torch.topk(scores.reshape(b, c, h * w), K)
        best, pos = torch.topk(per_cls.reshape(b, c * K), K)
        pix = torch.gather(pix.reshape(b, c * K), 1, pos)
        return best, pix, (pos // K).to(torch.int32), (pix // w).float(), (pix % w).float()

    @staticmethod
    def generate_src_and_dst(center, size, output_size):
        """centernet.py:354-375: three points of the source square (its centre, the point half a side above it, and that point moved
        half a side to the left) and the same three of the output map, float32 (3, 2) each."""
        side = size[0] if np.ndim(size) else size        # a scalar is a square's side
        dst_w, dst_h = output_size

        def corners(c, width):
            half = width * -0.5
            pts = np.zeros((3, 2), dtype=np.float32)
            pts[0] = c
            pts[1] = pts[0].astype(np.float64) + (0.0, half)
            pts[2] = pts[1].astype(np.float64) + (half, 0.0)
            return pts
        return corners(center, side), corners((dst_w * 0.5, dst_h * 0.5), dst_w)


class CenterNetGT:
    """The per-image helpers of the reference on host numpy arrays (float32 where the reference's tensors are).  The batch path is
    centernet_ground_truth: one launch for all images."""

    @staticmethod
    def generate_score_map(fmap, gt_class, gt_wh, centers_int, min_overlap):
        """centernet.py:380-391: fmap (K, H, W) float32 array, changed in place and returned."""
        radius = CenterNetGT.get_gaussian_radius(gt_wh, min_overlap)
        radius = np.maximum(radius, 0).astype(np.int32)
        for i in range(len(gt_class)):
            c = int(gt_class[i])
            if c >= 0:
                fmap[c] = CenterNetGT.draw_gaussian(fmap[c], centers_int[i], int(radius[i]))
        return fmap

    @staticmethod
    def get_gaussian_radius(box_size, min_overlap):
        """centernet.py:393-423 (the "bug version"), float32, one rounding per operation, in the order written."""
        box = np.asarray(box_size, dtype=np.float32)
        if box.size == 0:
            return np.zeros((0,), np.float32)
        f = np.float32
        width, height = box[..., 0], box[..., 1]
        b1 = height + width
        c1 = width * height * f(1 - min_overlap) / f(1 + min_overlap)
        sq1 = np.sqrt(b1 * b1 - f(4) * c1)
        r1 = (b1 + sq1) / f(2)
        b2 = f(2) * (height + width)
        c2 = f(1 - min_overlap) * width * height
        sq2 = np.sqrt(b2 * b2 - f(16) * c2)
        r2 = (b2 + sq2) / f(2)
        b3 = f(-2 * min_overlap) * (height + width)
        c3 = f(min_overlap - 1) * width * height
        sq3 = np.sqrt(b3 * b3 - f(4 * (4 * min_overlap)) * c3)
        r3 = (b3 + sq3) / f(2)
        return np.minimum(np.minimum(r1, r2), r3)

    @staticmethod
    def gaussian2D(radius, sigma=1):
        """centernet.py:425-432: the (2m+1, 2n+1) float64 Gaussian window, values below eps * max cut to 0."""
        m, n = radius
        dy = np.arange(-m, m + 1).reshape(-1, 1)
        dx = np.arange(-n, n + 1).reshape(1, -1)
        g = np.exp(-(dx * dx + dy * dy) / (2 * sigma * sigma))
        g[g < np.finfo(g.dtype).eps * g.max()] = 0
        return g

    @staticmethod
    def draw_gaussian(fmap, center, radius, k=1):
        """centernet.py:434-452: fmap (H, W) <- max(fmap, k * window) over the part of the window that lies inside the map."""
        g = CenterNetGT.gaussian2D((radius, radius), sigma=(2 * radius + 1) / 6).astype(np.float32)
        cx, cy = int(center[0]), int(center[1])
        H, W = fmap.shape[:2]
        x0, x1 = cx - min(cx, radius), cx + min(W - cx, radius + 1)
        y0, y1 = cy - min(cy, radius), cy + min(H - cy, radius + 1)
        if x1 > x0 and y1 > y0:
            win = g[y0 - cy + radius:y1 - cy + radius, x0 - cx + radius:x1 - cx + radius]
            fmap[y0:y1, x0:x1] = np.maximum(fmap[y0:y1, x0:x1], win * k)
        return fmap
