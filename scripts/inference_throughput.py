"""Inference throughput of RetinaNet-R50 and Faster R-CNN-R50 at 800x1344 on synthetic images, batch 1 / 4 / 16:

    python scripts/inference_throughput.py [--models retinanet,faster_rcnn] [--batches 1,4,16] [--repeats 7] [--warmup 2]

Per model and N, in ONE process (so every figure of a table shares the box and its clocks):
  batched    N images in one `inference_batch` call, wall clock around a device synchronisation, img/s of the median run;
  per-image  the loop the evaluator ran before batches existed: N single-image calls.  For RetinaNet the loop runs the chain that
             `inference` was then made of (det_scores -> segment_topk -> det_candidates -> nms_batched -> det_finalize, one count read per
             image), rebuilt here from the same operators at B = 1;
  chain ms   the post-processing chain alone on the plan's tensors of a batch-N forward, between two HIP events: the chain `_detect`
             runs (bd_det_select first for RetinaNet) and, for RetinaNet, the same batched chain with det_scores + segment_topk(B = N)
             in the place of bd_det_select.
The classification bias is shifted from a first forward so that a realistic share of the items clears TEST.CLS_THRESHOLD (the recipe of
tests/test_fullsize_inference_gpu.py): random-initialised heads would leave nothing above it and the selection nothing to do."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from basedet_amd import ops  # noqa: E402

SIZE = (800, 1344)


def bisect(frac_of, target):
    lo, hi = -30.0, 30.0
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if frac_of(mid) < target else (lo, mid)
    return 0.5 * (lo + hi)


def batch(n, seed=0):
    from basedet_amd.utils import DummyLoader
    b = next(DummyLoader(n, SIZE, seed=seed))
    info = np.tile(np.asarray([[*SIZE, 600, 1100, 0]], np.float32), (n, 1))
    return {"data": torch.from_numpy((b["data"] * 255).astype(np.float32)).cuda(), "im_info": torch.from_numpy(info).cuda()}


def build_retinanet():
    from basedet_amd.configs import RetinaNetConfig
    from basedet_amd.models import RetinaNet, params as P
    cfg = RetinaNetConfig()
    params = P.init_retinanet_params(cfg, 0, residual_gamma=0.25)
    params["head.cls_score.weight"] = params["head.cls_score.weight"] * 8
    params["head.bbox_pred.weight"] = params["head.bbox_pred.weight"] * 8
    model = RetinaNet(cfg, params=params).eval()
    model.inference(batch(1))
    logits = model._plan(1, *SIZE).logits.float().reshape(-1)
    thr = cfg.TEST.CLS_THRESHOLD
    d = bisect(lambda s: float((torch.sigmoid(logits + s) > thr).float().mean()), 3e-3)
    params["head.cls_score.bias"] = params["head.cls_score.bias"] + np.float32(d)
    return cfg, RetinaNet(cfg, params=params).eval()


def build_faster_rcnn():
    from basedet_amd.configs import FasterRCNNConfig
    from basedet_amd.models import FasterRCNN, params as P
    cfg = FasterRCNNConfig()
    params = P.init_faster_rcnn_params(cfg, 0, residual_gamma=0.25)
    for k in ("rpn.rpn_cls_score.weight", "rpn.rpn_bbox_offsets.weight", "rcnn.pred_cls.weight", "rcnn.pred_delta.weight",
              "rcnn.fc1.weight", "rcnn.fc2.weight", "rpn.rpn_conv.weight"):
        params[k] = (params[k] * 3).astype(np.float32)
    model = FasterRCNN(cfg, params=params).eval()
    model.inference(batch(1))
    pl = model._cur
    K = model.num_classes
    lg = pl.inf["raw"][: int(pl.num_rois[0].item()), : K + 1].double()
    thr = cfg.TEST.CLS_THRESHOLD

    def frac(s):
        x = lg.clone(); x[:, 0] -= s
        return float((torch.softmax(x, 1)[:, 1:] > thr).double().mean())
    params["rcnn.pred_cls.bias"] = params["rcnn.pred_cls.bias"].copy()
    params["rcnn.pred_cls.bias"][0] -= np.float32(bisect(frac, 0.05))
    return cfg, FasterRCNN(cfg, params=params).eval()


class LegacyRetinaChain:
    """The post-processing `RetinaNet.inference` ran before bd_det_select: fp32 scores of every item, then the per-level top-k reads them."""

    def __init__(self, cfg, model):
        self.cfg, self.m = cfg, model
        self.buf = {}

    def _scratch(self, N, rows, K, k, Ln):
        key = (N, rows)
        if key not in self.buf:
            i32 = dict(dtype=torch.int32, device="cuda")
            f32 = dict(dtype=torch.float32, device="cuda")
            C, mo = Ln * k, self.cfg.TEST.MAX_BOXES_PER_IMAGE
            self.buf[key] = dict(scores=torch.empty((N, rows * K), **f32), idx=torch.empty((N, Ln, k), **i32), sc=torch.empty((N, Ln, k), **f32),
                                 cnt=torch.empty((N, Ln), **i32), boxes=torch.empty((N, C, 4), **f32), csc=torch.empty((N, C), **f32),
                                 lab=torch.empty((N, C), **i32), keep=torch.empty((N, mo), **i32), num=torch.zeros((N,), **i32),
                                 ws=torch.empty((ops.nms_batched_workspace_bytes(N, C),), dtype=torch.uint8, device="cuda"),
                                 ob=torch.empty((N, mo, 4), **f32), os=torch.empty((N, mo), **f32), ol=torch.empty((N, mo), **i32))
        return self.buf[key]

    def run(self, pl, info, read_counts):
        m, t = self.m, self.cfg.TEST
        N, K, A, k = pl.N, m.num_classes, m.num_anchors, 1000
        lvl_rows = [h * w * A for h, w in pl.sizes]
        rows = sum(lvl_rows)
        row_off = [0]
        for r in lvl_rows[:-1]:
            row_off.append(row_off[-1] + r)
        s = self._scratch(N, rows, K, k, len(lvl_rows))
        ops.det_scores(pl.logits, N * rows, K, s["scores"])
        ops.segment_topk(s["scores"], N, rows * K, 1, 1, 0, [r * K for r in row_off], [r * K for r in lvl_rows], k, s["idx"], s["sc"], s["cnt"],
                         min_score=t.CLS_THRESHOLD)
        reg = self.cfg.MODEL.BOX_REG
        ops.det_candidates(0, s["idx"], s["sc"], s["cnt"], N, len(lvl_rows), k, row_off, K, pl.anchors, pl.offsets,
                           pl.offsets.numel() // N, m.box_ld, A, reg.MEAN, reg.STD, None, 0, s["boxes"], s["csc"], s["lab"])
        s["num"].zero_()
        ops.nms_batched(s["boxes"], s["csc"], s["lab"], t.IOU_THRESHOLD, t.MAX_BOXES_PER_IMAGE, s["keep"], s["num"], s["ws"])
        ops.det_finalize(s["boxes"], s["csc"], s["lab"], s["keep"], s["num"], t.MAX_BOXES_PER_IMAGE, info, s["ob"], s["os"], s["ol"])
        return s["num"].tolist() if read_counts else None

    def inference_one(self, inputs):
        pre = self.m.pre_process(inputs)
        self.m.network_forward(pre["plan"])
        return self.run(pre["plan"], pre["img_info"], True)


def wall(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def events(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="retinanet,faster_rcnn")
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    print(f"# device {torch.cuda.get_device_name(0)}; {a.repeats} timed runs after {a.warmup} warm-up runs, medians; one process", flush=True)
    for name in a.models.split(","):
        cfg, model = build_retinanet() if name == "retinanet" else build_faster_rcnn()
        legacy = LegacyRetinaChain(cfg, model) if name == "retinanet" else None
        for N in (int(x) for x in a.batches.split(",")):
            b = batch(N, seed=N)
            singles = [{"data": b["data"][i:i + 1], "im_info": b["im_info"][i:i + 1]} for i in range(N)]
            t_b, _ = wall(lambda: model.inference_batch(b), a.warmup, a.repeats)
            if legacy is not None:
                t_l, _ = wall(lambda: [legacy.inference_one(s) for s in singles], max(1, a.warmup - 1), max(3, a.repeats // 2))
            else:
                t_l, _ = wall(lambda: [model.inference(s) for s in singles], a.warmup, a.repeats)
            outs = model.inference_batch(b)            # leaves the batch-N plan's tensors in place for the chain timing
            ndet = sum(int(o["box_scores"].numel()) for o in outs)
            pl = model._plan(N, *SIZE)
            info = b["im_info"]
            rec = {"model": name, "N": N, "batched_img_s": round(N / t_b, 2), "batched_ms": round(t_b * 1e3, 3),
                   "per_image_loop_img_s": round(N / t_l, 2), "per_image_loop_ms": round(t_l * 1e3, 3), "detections": ndet}
            if name == "retinanet":
                K, A = model.num_classes, model.num_anchors
                reg = cfg.MODEL.BOX_REG
                new = lambda: model._detect(N, [h * w * A for h, w in pl.sizes], K, 0, info, logits=pl.logits, anchors=pl.anchors,   # noqa: E731
                                            offsets=pl.offsets, off_ld=model.box_ld, A=A, mean=reg.MEAN, std=reg.STD)
                rec["chain_ms_det_select"] = round(events(new, a.warmup, a.repeats)[0], 3)
                rec["chain_ms_scores_topk"] = round(events(lambda: legacy.run(pl, info, True), 1, max(3, a.repeats // 2))[0], 3)
            else:
                K, R = model.num_classes, pl.rois.shape[1]
                ch = lambda: model._detect(N, [R], K, 2, info, k=2048, scores=pl.inf["scores"], item_boxes=pl.inf["boxes"])  # noqa: E731
                rec["chain_ms"] = round(events(ch, a.warmup, a.repeats)[0], 3)
            print(json.dumps(rec), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
