"""Inference at 800x1344 (batch 1, like the reference) of RetinaNet-R50, FCOS-R50 and Faster R-CNN-R50 against the numpy post-processing
oracle, oracle/rcnn_ops.py detect_postprocess (:294-318: per-level threshold + top-k, batched NMS, rescale, clip).

The oracle runs on the kernels' own fp32 scores -- recomputed with ops.det_scores from the plan's logits (RetinaNet, FCOS) or taken
from rcnn_predict (Faster R-CNN) -- so an fp32-ulp difference in a sigmoid cannot reorder near-ties; test_postprocess_gpu.py bounds
those kernels on their own.  Likewise the boxes the oracle sees are the device's decode (ops.box_decode / rcnn_predict; the point
decode is exact), each checked against oracle/box_ops.py box_decode with the tolerance of test_boxops_gpu.py, so an IoU within one
ulp of the NMS threshold cannot flip a decision.  Labels and keep order are compared exactly; boxes and scores with the tolerances
of test_model_gpu.py's 128x160 inference tests.

The classification bias is set from a first forward so that a fixed fraction of the items clears TEST.CLS_THRESHOLD; the regimes
that matter are then asserted from the oracle's per-level counts: a level cut at its top-k, a level that is not (one-stage models),
and NMS returning exactly MAX_BOXES_PER_IMAGE."""
import numpy as np
import pytest
import torch

from oracle import box_ops as ob
from oracle import rcnn_ops as orc

pytestmark = pytest.mark.gpu
SIZE = (800, 1344)
IM_INFO = (800, 1344, 600, 1100)          # resized h, w; original h, w: an anisotropic rescale


def _batch(seed=0):
    from basedet_amd.utils import DummyLoader
    b = next(DummyLoader(1, SIZE, seed=seed))
    return {"data": (b["data"] * 255).astype(np.float32), "im_info": np.asarray([IM_INFO], np.float32)}


def _shift_for_fraction(frac_of, target):
    """Bisection for the logit shift d with frac_of(d) = target (frac_of increasing in d)."""
    lo, hi = -30.0, 30.0
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if frac_of(mid) < target else (lo, mid)
    return 0.5 * (lo + hi)


def _level_split(a, rows):
    out, o = [], 0
    for r in rows:
        out.append(a[o:o + r]); o += r
    return out


def _compare(out, sc_l, bx_l, K, cfg, k, tol):
    """Oracle on the device's scores and boxes; returns the oracle's per-level candidate counts and the detection count."""
    t = cfg.TEST
    counts = [len(orc.topk_desc(s, k, t.CLS_THRESHOLD)[0]) for s in sc_l]
    rb, rs, rl = orc.detect_postprocess(sc_l, bx_l, K, np.asarray(IM_INFO, np.float32), t.CLS_THRESHOLD, t.IOU_THRESHOLD,
                                        t.MAX_BOXES_PER_IMAGE, topk=k)
    assert out["boxes"].shape[0] == len(rs)
    assert np.array_equal(out["box_labels"].cpu().numpy(), rl)
    np.testing.assert_allclose(out["box_scores"].cpu().numpy(), rs, rtol=tol[0])
    np.testing.assert_allclose(out["boxes"].float().cpu().numpy(), rb, rtol=tol[0], atol=tol[1])
    return counts, len(rs)


def _assert_regimes(name, counts, n_det, k, cfg, one_stage=True):
    print(f"{name} 1x800x1344: candidates per level {counts} (k = {k}), detections {n_det}")
    assert max(counts) == k, "no level is cut at its top-k"
    if one_stage:
        assert min(counts) < k, "every level is cut"
    assert n_det == cfg.TEST.MAX_BOXES_PER_IMAGE


def test_retinanet_r50_inference_full_size():
    from basedet_amd import ops
    from basedet_amd.models import RetinaNet
    from tests.test_model_gpu import _setup
    cfg, params, _ = _setup("resnet50", 1, SIZE, seed=5)
    params["head.cls_score.weight"] = params["head.cls_score.weight"] * 8
    params["head.bbox_pred.weight"] = params["head.bbox_pred.weight"] * 8
    batch = _batch(5)
    thr = cfg.TEST.CLS_THRESHOLD
    model = RetinaNet(cfg, params=params).eval()
    model(batch)
    logits = model._plan(1, *SIZE).logits.float().reshape(-1)
    d = _shift_for_fraction(lambda s: float((torch.sigmoid(logits + s) > thr).float().mean()), 3e-3)
    params["head.cls_score.bias"] = params["head.cls_score.bias"] + np.float32(d)
    model = RetinaNet(cfg, params=params).eval()
    out = model(batch)
    pl = model._plan(1, *SIZE)
    K, A = model.num_classes, model.num_anchors
    rows = pl.pyr.pix_per_img * A
    assert rows == 201600
    scores = torch.empty((rows * K,), dtype=torch.float32, device="cuda")
    ops.det_scores(pl.logits, rows, K, scores)
    m = cfg.MODEL.BOX_REG
    deltas = pl.offsets[:, : A * 4].float().reshape(-1, 4).contiguous()
    boxes = ops.box_decode(pl.anchors, deltas, m.MEAN, m.STD).cpu().numpy()
    np.testing.assert_allclose(boxes, ob.box_decode(pl.anchors.cpu().numpy(), deltas.cpu().numpy(), m.MEAN, m.STD), rtol=1e-5, atol=1e-3)
    lvl_rows = [h * w * A for h, w in pl.sizes]
    counts, n = _compare(out, _level_split(scores.cpu().numpy(), [r * K for r in lvl_rows]), _level_split(boxes, lvl_rows), K, cfg,
                         1000, (1e-5, 1e-3))
    _assert_regimes("RetinaNet-R50", counts, n, 1000, cfg)


def test_fcos_r50_inference_full_size():
    from basedet_amd import ops
    from basedet_amd.configs import FCOSConfig
    from basedet_amd.models import FCOS, params as P
    cfg = FCOSConfig()
    cfg.MODEL.BATCHSIZE = 1
    params = P.init_fcos_params(cfg, seed=0, residual_gamma=0.25)
    params["head.cls_score.weight"] = params["head.cls_score.weight"] * 8
    params["head.bbox_pred.bias"] = np.full_like(params["head.bbox_pred.bias"], 1.5)
    batch = _batch(0)
    thr = cfg.TEST.CLS_THRESHOLD
    model = FCOS(cfg, params=params).eval()
    model(batch)
    pl = model._plan(1, *SIZE)
    logits, ctr = pl.logits.float(), torch.sigmoid(pl.raw[:, 4:5].float())
    d = _shift_for_fraction(lambda s: float((torch.sqrt(torch.sigmoid(logits + s) * ctr) > thr).float().mean()), 5e-3)
    params["head.cls_score.bias"] = params["head.cls_score.bias"] + np.float32(d)
    model = FCOS(cfg, params=params).eval()
    out = model(batch)
    pl = model._plan(1, *SIZE)
    K = model.num_classes
    rows = pl.pyr.pix_per_img
    assert rows == 22400
    scores = torch.empty((rows * K,), dtype=torch.float32, device="cuda")
    ops.det_scores(pl.logits, rows, K, scores, ctr=pl.raw, ctr_ld=8, ctr_off=4)
    boxes = ob.point_decode(pl.points.cpu().numpy(), pl.offsets.float().cpu().numpy())
    lvl_rows = [h * w for h, w in pl.sizes]
    counts, n = _compare(out, _level_split(scores.cpu().numpy(), [r * K for r in lvl_rows]), _level_split(boxes, lvl_rows), K, cfg,
                         1000, (1e-5, 1e-3))
    _assert_regimes("FCOS-R50", counts, n, 1000, cfg)


def test_faster_rcnn_r50_inference_full_size():
    """One level of R x K items (R = TEST_POST_NMS_TOPK proposals), top-k 2048: the cut and the 100-box NMS cap are the regimes."""
    from basedet_amd.configs import FasterRCNNConfig
    from basedet_amd.models import FasterRCNN, params as P
    cfg = FasterRCNNConfig()
    cfg.MODEL.BATCHSIZE = 1
    params = P.init_faster_rcnn_params(cfg, 0, residual_gamma=0.25)
    for k in ("rpn.rpn_cls_score.weight", "rpn.rpn_bbox_offsets.weight", "rcnn.pred_cls.weight", "rcnn.pred_delta.weight",
              "rcnn.fc1.weight", "rcnn.fc2.weight", "rpn.rpn_conv.weight"):
        params[k] = (params[k] * 3).astype(np.float32)
    batch = _batch(0)
    thr = cfg.TEST.CLS_THRESHOLD
    model = FasterRCNN(cfg, params=params).eval()
    model(batch)
    pl = model._cur
    K = model.num_classes
    nr = int(pl.num_rois[0].item())
    lg = pl.inf["raw"][:nr, : K + 1].double()

    def frac(s):            # background logit lowered by s
        x = lg.clone(); x[:, 0] -= s
        return float((torch.softmax(x, 1)[:, 1:] > thr).double().mean())
    d = _shift_for_fraction(frac, 0.05)
    params["rcnn.pred_cls.bias"] = params["rcnn.pred_cls.bias"].copy()
    params["rcnn.pred_cls.bias"][0] -= np.float32(d)
    model = FasterRCNN(cfg, params=params).eval()
    out = model(batch)
    pl = model._cur
    R = pl.rois.shape[1]
    nr = int(pl.num_rois[0].item())
    assert 0 < nr <= R
    raw = pl.inf["raw"].float().cpu().numpy()
    rois = pl.rois[0].cpu().numpy()
    boxes = pl.inf["boxes"].cpu().numpy()
    m = cfg.MODEL.RCNN_BOX_REG
    ref = ob.box_decode(np.repeat(rois[:nr], K, axis=0), raw[:nr, K + 1: K + 1 + 4 * K].reshape(nr * K, 4), m.MEAN, m.STD)
    np.testing.assert_allclose(boxes[: nr * K], ref, rtol=1e-5, atol=1e-3)
    scores = pl.inf["scores"].cpu().numpy()
    assert np.all(scores[nr * K:] == -np.inf)
    counts, n = _compare(out, [scores], [boxes], K, cfg, 2048, (1e-4, 1e-2))
    _assert_regimes("Faster R-CNN-R50", counts, n, 2048, cfg, one_stage=False)
