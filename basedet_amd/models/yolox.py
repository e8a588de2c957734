"""YOLOX behind the head's last convolutions, on the kernels of csrc/yolox.hip (models/det/yolox.py:119-135, 150-408 of the reference):
the SimOTA assignment (`yolox_assignments`), the four losses with gradients back to the head outputs (`yolox_losses`) and the inference
chain (`yolox_inference`: bd_det_select -> bd_yolox_candidates -> bd_nms_batched -> bd_det_finalize).  The decoupled head is
layers.YOLOXHead, and `yolox_head_step` runs it against the kernels here with no repack; the feature extractor is layers.YOLOPAFPN on
layers.CSPDarknet, and `yolox_network_step` is one training step of the whole network from the normalised image down to the stem's
parameter gradients.  `YOLOX` is the detector: those layers adopt()ed onto one parameter arena and one LiveNorms,
pre_process with the multi-scale resize (bd_resize_bilinear_normalize), get_losses / backward for Solver.minimize, and inference from an
image batch; solver.YOLOXSolver trains it.  The mosaic / mixup input is not built yet.

The kernels read the layout a fused head will write -- cls bf16 (N*P, round_up(K, 8)) and box_obj bf16 (N*P, 8): raw reg 0-3, obj logit
4 -- with the P points of an image level after level, row-major inside a level.  `yolox_losses` and `yolox_inference` take the
reference's three per-level NCHW fp32 lists and pack them into that layout on the way in (one rounding to bf16); a model step hands the
head's output to basedet_amd.ops directly.  Tensors live on the HIP device: host tensors raise BasedetHipError, there is no CPU path.

One departure from the reference: the gt is xyxy everywhere, and both IoUs are between the gt box and the predicted box."""
import torch

from basedet_amd import ops
from basedet_amd.layers._pm import need_device_all, round_up8
from basedet_amd.layers.box_ops import FastPointGenerator

__all__ = ["YOLOX", "yolox_assignments", "yolox_losses", "yolox_inference", "pack_head_outputs", "yolox_head_step", "yolox_network_step"]

_MODULE = "basedet_amd.models.yolox"          # (named in the refusal of a host tensor)


def _check_levels(logits, offsets, objs, strides):
    if not (len(logits) == len(offsets) == len(objs) == len(strides)) or not logits:
        raise ValueError("yolox: logits, offsets, objs and strides must be lists of one length, one entry per level")
    if len(strides) > ops._lib.BD_MAX_SEGS:
        raise ValueError(f"yolox: at most {ops._lib.BD_MAX_SEGS} levels")
    for x, o, b in zip(logits, offsets, objs):
        if x.dim() != 4 or o.dim() != 4 or b.dim() != 4 or o.shape[1] != 4 or b.shape[1] != 1 or x.shape[1] != logits[0].shape[1]:
            raise ValueError("yolox: per level logits (N, K, H, W), offsets (N, 4, H, W) and objs (N, 1, H, W)")
        if x.shape[0] != logits[0].shape[0] or x.shape[2:] != o.shape[2:] or x.shape[2:] != b.shape[2:] or o.shape[0] != x.shape[0] or b.shape[0] != x.shape[0]:
            raise ValueError("yolox: the three outputs of a level must share N, H and W")


def pack_head_outputs(logits, offsets, objs):
    """The reference's per-level NCHW lists -> (cls bf16 (N*P, round_up(K, 8)), box_obj bf16 (N*P, 8), sizes [(H, W)]); pad slots zero."""
    N, K = int(logits[0].shape[0]), int(logits[0].shape[1])
    sizes = [(int(x.shape[2]), int(x.shape[3])) for x in logits]
    P = sum(h * w for h, w in sizes)
    dev = logits[0].device
    cls = torch.zeros((N, P, round_up8(K)), dtype=torch.bfloat16, device=dev)
    box_obj = torch.zeros((N, P, 8), dtype=torch.bfloat16, device=dev)
    p0 = 0
    for x, o, b, (h, w) in zip(logits, offsets, objs, sizes):
        cls[:, p0:p0 + h * w, :K] = x.permute(0, 2, 3, 1).reshape(N, h * w, K)
        box_obj[:, p0:p0 + h * w, :4] = o.permute(0, 2, 3, 1).reshape(N, h * w, 4)
        box_obj[:, p0:p0 + h * w, 4] = b.reshape(N, h * w)
        p0 += h * w
    return cls.view(N * P, -1), box_obj.view(N * P, 8), sizes


def _unpack(d_cls, d_box_obj, N, K, sizes, dtype):
    P = sum(h * w for h, w in sizes)
    dc, db = d_cls.view(N, P, -1), d_box_obj.view(N, P, 8)
    gl, go, gb = [], [], []
    p0 = 0
    for h, w in sizes:
        gl.append(dc[:, p0:p0 + h * w, :K].to(dtype).reshape(N, h, w, K).permute(0, 3, 1, 2))
        go.append(db[:, p0:p0 + h * w, :4].to(dtype).reshape(N, h, w, 4).permute(0, 3, 1, 2))
        gb.append(db[:, p0:p0 + h * w, 4:5].to(dtype).reshape(N, h, w, 1).permute(0, 3, 1, 2))
        p0 += h * w
    return gl, go, gb


def _points(sizes, strides, device):
    gen = FastPointGenerator(strides)
    pts = torch.cat(gen([torch.empty((1, 1, h, w), device=device) for h, w in sizes]), 0)
    return pts, gen.level_starts(sizes)


def yolox_assignments(cls, box_obj, points, strides, gt_boxes, num_gt, K=None, lvl_start=None):
    """get_assignments for a batch (yolox.py:296-408): cls bf16 (N*P, round_up(K, 8)), box_obj bf16 (N*P, 8), points fp32 (P, 2) or the
    per-level list FastPointGenerator returns, gt_boxes fp32 (N, Gmax, 5) xyxy + 1-based label, num_gt int32 (N,) -> (matched int32
    (N, P): gt index or -1, iou_t fp32 (N, P): pred_ious_this_matching, stats fp32 (1,): the foreground count).  K defaults to the row
    width of cls; lvl_start is needed only when points is one tensor."""
    if isinstance(points, (list, tuple)):
        lvl_start = [0]
        for p in points:
            lvl_start.append(lvl_start[-1] + int(p.shape[0]))
        points = torch.cat(list(points), 0)
    if lvl_start is None:
        raise ValueError("yolox_assignments: points given as one tensor need lvl_start")
    need_device_all((cls, box_obj, points, gt_boxes, num_gt), _MODULE)
    K = int(cls.shape[1]) if K is None else int(K)
    return ops.yolox_assign(cls, K, box_obj, points.float().contiguous(), lvl_start, list(strides), gt_boxes.float().contiguous(),
                            num_gt.to(torch.int32).contiguous())


class _Losses(torch.autograd.Function):
    """total_loss and its four parts from one assignment and one loss launch; the kernel's gradient of the total is what backward hands
    out (times the incoming gradient)."""

    @staticmethod
    def forward(ctx, gt_boxes, num_gt, strides, use_l1, nlev, *heads):
        logits, offsets, objs = heads[:nlev], heads[nlev:2 * nlev], heads[2 * nlev:]
        N, K = int(logits[0].shape[0]), int(logits[0].shape[1])
        cls, box_obj, sizes = pack_head_outputs(logits, offsets, objs)
        points, lvl_start = _points(sizes, strides, cls.device)
        gt = gt_boxes.float().contiguous()
        matched, iou_t, stats = ops.yolox_assign(cls, K, box_obj, points, lvl_start, list(strides), gt, num_gt.to(torch.int32).contiguous())
        parts, d_cls, d_box_obj = ops.yolox_loss_fwd_bwd(cls, K, box_obj, points, lvl_start, list(strides), gt, matched, iou_t, stats,
                                                        use_l1=use_l1, grad_scale=1.0)
        gl, go, gb = _unpack(d_cls, d_box_obj, N, K, sizes, logits[0].dtype)
        ctx.save_for_backward(*gl, *go, *gb)
        ctx.mark_non_differentiable(parts)
        return parts.sum(), parts

    @staticmethod
    def backward(ctx, gout, _gparts):
        return (None, None, None, None, None, *[g * gout for g in ctx.saved_tensors])


def yolox_losses(logits, offsets, objs, gt_boxes, num_gt, strides, use_l1=False):
    """YOLOX.get_losses behind network_forward (yolox.py:155-265): the reference's three per-level NCHW lists, gt_boxes (N, Gmax, 5) and
    num_gt (N,) -> {total_loss, iou_loss (times 5), l1_loss, obj_loss, cls_loss}.  total_loss carries the gradient to the inputs."""
    _check_levels(logits, offsets, objs, strides)
    need_device_all((*logits, *offsets, *objs, gt_boxes, num_gt), _MODULE)
    total, parts = _Losses.apply(gt_boxes, num_gt, tuple(int(s) for s in strides), bool(use_l1), len(logits), *logits, *offsets, *objs)
    return {"total_loss": total, "iou_loss": parts[0], "l1_loss": parts[3], "obj_loss": parts[1], "cls_loss": parts[2]}


def _head_losses(head, feats, N, sizes, gt_boxes, num_gt, strides, use_l1=False, points=None):
    """The forward half of a head step: forward_pm -> ops.yolox_assign -> ops.yolox_loss_fwd_bwd.  Returns (parts, d_cls, d_box_obj,
    (matched, iou_t, stats)); points = a cached (points, lvl_start) of these sizes."""
    cls, box_obj = head.forward_pm(feats, N, sizes)
    points, lvl_start = points if points is not None else _points(sizes, strides, cls.device)
    gt = gt_boxes.float().contiguous()
    K = head.num_classes
    matched, iou_t, stats = ops.yolox_assign(cls, K, box_obj, points, lvl_start, list(strides), gt, num_gt.to(torch.int32).contiguous())
    parts, d_cls, d_box_obj = ops.yolox_loss_fwd_bwd(cls, K, box_obj, points, lvl_start, list(strides), gt, matched, iou_t, stats,
                                                    use_l1=use_l1, grad_scale=1.0)
    return parts, d_cls, d_box_obj, (matched, iou_t, stats)


def yolox_head_step(head, feats, N, sizes, gt_boxes, num_gt, strides, use_l1=False):
    """One training step of a layers.YOLOXHead on its own layout, no repack: forward_pm -> ops.yolox_assign -> ops.yolox_loss_fwd_bwd ->
    backward_pm.  feats: per level bf16 (N H_l W_l, C_l); sizes [(H_l, W_l)].  Returns (parts fp32 (4,) = 5 * iou, obj, cls, l1;
    d_feats per level; (matched, iou_t, stats))."""
    need_device_all((*feats, gt_boxes, num_gt), _MODULE)
    parts, d_cls, d_box_obj, assigned = _head_losses(head, feats, N, sizes, gt_boxes, num_gt, strides, use_l1)
    return parts, head.backward_pm(d_cls, d_box_obj), assigned


def yolox_network_step(fpn, head, x_halo, N, H, W, gt_boxes, num_gt, strides=(8, 16, 32), use_l1=False):
    """One training step of layers.YOLOPAFPN + layers.YOLOXHead: PAFPN forward -> yolox_head_step -> PAFPN backward, pixel-major bf16
    throughout.  x_halo: the bf16 (N, H + 6, W + 8, 4) image bd_pad_normalize / bd_resize_pad_normalize / bd_affine_jitter_normalize
    write, H and W multiples of 32.  Returns (parts fp32 (4,) = 5 * iou, obj, cls, l1; (matched, iou_t, stats)); the parameter gradients
    are in fpn.grads() and head.grads()."""
    need_device_all((x_halo, gt_boxes, num_gt), _MODULE)
    feats, sizes = fpn.forward_pm(x_halo, N, H, W)
    parts, d_feats, assigned = yolox_head_step(head, list(feats), N, sizes, gt_boxes, num_gt, strides, use_l1)
    fpn.backward_pm(d_feats)
    return parts, assigned


def _detect_packed(cls, box_obj, K, sizes, img_info, cfg, strides, k, cache=None):
    """The inference chain behind the pack, for B images: cls bf16 (B*P, round_up(K, 8)) and box_obj bf16 (B*P, 8) as the head writes
    them -> bd_det_select -> bd_yolox_candidates -> bd_nms_batched -> bd_det_finalize.  cache: a dict that keeps the scratch of a
    (B, sizes, k) between calls (the model's); the results are new tensors, the caller's, either way."""
    from basedet_amd.structures import Boxes, Container
    t = cfg.TEST
    dev = cls.device
    Ln, max_out = len(sizes), int(t.MAX_BOXES_PER_IMAGE)
    P = sum(h * w for h, w in sizes)
    B = int(cls.shape[0]) // P
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    key = (B, tuple(sizes), k, K)
    sc = cache.get(key) if cache is not None else None
    if sc is None:
        points, lvl_start = _points(sizes, strides, dev)
        sc = dict(points=points, lvl_start=lvl_start, tk_idx=torch.empty((B, Ln, k), **i32), tk_sc=torch.empty((B, Ln, k), **f32),
                  tk_cnt=torch.empty((B, Ln), **i32),
                  ws=torch.empty((ops.det_select_workspace_bytes(B, Ln, P, K, k),), dtype=torch.uint8, device=dev),
                  boxes=torch.empty((B, Ln * k, 4), **f32), scores=torch.empty((B, Ln * k), **f32), labels=torch.empty((B, Ln * k), **i32),
                  keep=torch.empty((B, max_out), **i32), num=torch.zeros((B,), **i32),
                  nms_ws=torch.empty((ops.nms_batched_workspace_bytes(B, Ln * k),), dtype=torch.uint8, device=dev))
        if cache is not None:
            cache[key] = sc
    lvl_start = sc["lvl_start"]
    ops.det_select(cls, B, P, K, lvl_start[:-1], [h * w for h, w in sizes], k, t.CLS_THRESHOLD, sc["tk_idx"], sc["tk_sc"], sc["tk_cnt"],
                   sc["ws"], ctr=box_obj, ctr_ld=8, ctr_off=4, ld=round_up8(K))
    ops.yolox_candidates_into(sc["tk_idx"], sc["tk_sc"], sc["tk_cnt"], K, sc["points"], lvl_start, list(strides), box_obj, sc["boxes"],
                              sc["scores"], sc["labels"])
    sc["num"].zero_()
    ops.nms_batched(sc["boxes"], sc["scores"], sc["labels"], t.IOU_THRESHOLD, max_out, sc["keep"], sc["num"], sc["nms_ws"])
    ob, osc, ol = torch.empty((B, max_out, 4), **f32), torch.empty((B, max_out), **f32), torch.empty((B, max_out), **i32)
    ops.det_finalize(sc["boxes"], sc["scores"], sc["labels"], sc["keep"], sc["num"], max_out, img_info.float().contiguous(), ob, osc, ol)
    outs = []
    for i, n in enumerate(sc["num"].tolist()):
        if n == 0:
            e = torch.zeros((0,))
            outs.append(Container(boxes=e, box_scores=e, box_labels=e))
        else:
            outs.append(Container(boxes=Boxes(ob[i, :n]), box_scores=osc[i, :n], box_labels=ol[i, :n]))
    return outs


def yolox_inference(logits, offsets, objs, img_info, cfg, strides=(8, 16, 32), k=1000):
    """YOLOX.inference behind network_forward (yolox.py:112-148) for a batch: per image and level score = sqrt(sigmoid(cls) sigmoid(obj))
    > TEST.CLS_THRESHOLD -> top-k -> decode -> batched NMS by label (TEST.IOU_THRESHOLD) -> the first TEST.MAX_BOXES_PER_IMAGE, scaled
    and clipped by the image's img_info row (h, w, original h, original w).  Returns the list of per-image Containers (boxes,
    box_scores, box_labels).  The body behind the pack is the one YOLOX.inference_batch runs on the head's own outputs."""
    _check_levels(logits, offsets, objs, strides)
    need_device_all((*logits, *offsets, *objs, img_info), _MODULE)
    cls, box_obj, sizes = pack_head_outputs(logits, offsets, objs)
    return _detect_packed(cls, box_obj, int(logits[0].shape[1]), sizes, img_info, cfg, strides, k)


# the detector lives in a module of its own, imported by its absolute name: `basedet.models.yolox` (the alias package) and this module
# then hold ONE class, the one registers.models has
from basedet_amd.models.yolox_detector import YOLOX  # noqa: E402, F401
