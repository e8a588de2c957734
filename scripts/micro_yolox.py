"""The three YOLOX entries of csrc/yolox.hip at the workload's shape, timed: batch 16 of 640 x 640 (P = 8400 points on strides 8 / 16 / 32),
K = 80 classes, 40 gts per image.

  assign      bd_yolox_assign (prep, one workgroup per (gt, image), resolve).  The share of the per-gt launch is estimated from a
              second run with num_gt = 1 on the same data: prep and resolve barely change, the per-gt launch shrinks 40-fold
  loss        bd_yolox_loss_fwd_bwd with use_l1; bytes moved = d_cls and d_box_obj written, box_obj, matched and iou_t read, the cls
              rows of the foreground read -- over the time, as a fraction of the HBM rate of MI355X_MICROARCH.md (8 TB/s)
  candidates  bd_det_select + bd_yolox_candidates of the inference chain (k = 1000, TEST.CLS_THRESHOLD = 0.001)

    python scripts/micro_yolox.py [--repeats 20] [--iters 10]

Prints a final JSON line; p50 / p95 over the repeats, microseconds per call.  A measurement, not a test: nothing is asserted about time."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from basedet_amd import ops  # noqa: E402
import yolox_oracle as O  # noqa: E402

N, H, W, K, G = 16, 640, 640, 80, 40
HBM_BYTES_PER_S = 8.0e12


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _pcts(v):
    return {"p50": round(float(np.percentile(v, 50)), 2), "p95": round(float(np.percentile(v, 95)), 2)}


def _time(fn, repeats, iters):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("micro_yolox.py needs a HIP device")
    repeats, iters = _arg("--repeats", 20), _arg("--iters", 10)
    rng = np.random.default_rng(0)
    prob = O._base(N, H, W, K, G, rng)
    for n in range(N):
        prob["num"][n] = G
        prob["gt"][n] = O._rand_gts(rng, G, H, W, K, lo=16.0)
    prob = O._finish(prob, rng)
    P = prob["pts"].shape[0]
    dev = "cuda"
    cls = torch.from_numpy(prob["cls"]).to(torch.bfloat16).reshape(N * P, -1).to(dev)
    box_obj = torch.from_numpy(prob["box_obj"]).to(torch.bfloat16).reshape(N * P, 8).to(dev)
    pts, gt = torch.from_numpy(prob["pts"]).to(dev), torch.from_numpy(prob["gt"]).to(dev)
    num, one = torch.from_numpy(prob["num"]).to(dev), torch.ones(N, dtype=torch.int32, device=dev)
    start, strides = prob["lvl_start"], prob["strides"]
    matched = torch.empty((N, P), dtype=torch.int32, device=dev)
    iou_t, stats = torch.empty((N, P), dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
    ws = torch.empty(ops.yolox_assign_workspace_bytes(N, P), dtype=torch.uint8, device=dev)
    res = {"shape": dict(N=N, P=P, K=K, gts=G)}
    t1 = _time(lambda: ops.yolox_assign_into(cls, K, box_obj, pts, start, strides, gt, one, matched, iou_t, stats, ws), repeats, iters)
    t = _time(lambda: ops.yolox_assign_into(cls, K, box_obj, pts, start, strides, gt, num, matched, iou_t, stats, ws), repeats, iters)
    nfg = int(stats[0])
    res["assign_us"], res["assign_one_gt_us"], res["foreground"] = _pcts(t), _pcts(t1), nfg
    loss, d_cls, d_box = torch.empty(4, device=dev), torch.empty_like(cls), torch.empty_like(box_obj)
    lws = torch.empty(ops.yolox_loss_workspace_bytes(), dtype=torch.uint8, device=dev)
    t = _time(lambda: ops.yolox_loss_fwd_bwd_into(cls, K, box_obj, pts, start, strides, gt, matched, iou_t, stats, True, 1.0, loss, d_cls,
                                                  d_box, lws), repeats, iters)
    rows, ld = N * P, cls.shape[1]
    moved = rows * ld * 2 + rows * 16 * 2 + rows * 8 + nfg * ld * 2
    res["loss_us"] = _pcts(t)
    res["loss_bytes"] = moved
    res["loss_hbm_fraction"] = round(moved / (np.percentile(t, 50) * 1e-6) / HBM_BYTES_PER_S, 4)
    k, L = 1000, len(strides)
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    tk_idx, tk_sc, tk_cnt = torch.empty((N, L, k), **i32), torch.empty((N, L, k), **f32), torch.empty((N, L), **i32)
    sws = torch.empty(ops.det_select_workspace_bytes(N, L, P, K, k), dtype=torch.uint8, device=dev)
    boxes, scores, labels = torch.empty((N, L * k, 4), **f32), torch.empty((N, L * k), **f32), torch.empty((N, L * k), **i32)
    lvl_rows = [b - a for a, b in zip(start[:-1], start[1:])]

    def select():
        ops.det_select(cls, N, P, K, start[:-1], lvl_rows, k, 0.001, tk_idx, tk_sc, tk_cnt, sws, ctr=box_obj, ctr_ld=8, ctr_off=4, ld=ld)

    def cand():
        ops.yolox_candidates_into(tk_idx, tk_sc, tk_cnt, K, pts, start, strides, box_obj, boxes, scores, labels)
    res["det_select_us"] = _pcts(_time(select, repeats, iters))
    res["candidates_us"] = _pcts(_time(cand, repeats, iters))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
