"""The Objects365 class count on the one-stage heads: RetinaNet-R50-FPN at DATA.NUM_CLASSES = 365 (cls_score: 9 x 368 = 3312 channels),
800 x 1344, synthetic batches, and FCOS-R50 at 365 classes beside FCOS at 368 (the same launch shapes: cls_ld = 368 for both).

    python scripts/obj365_step.py [--batch 16] [--warmup 3] [--steps 10] [--step-limit 120] [--only retinanet|fcos365|fcos368]

Prints one line per workload: the losses of the last step (they must be finite) and ms/step over the timed steps.  Every step runs under
--step-limit seconds: a watchdog thread of the interpreter (faulthandler.dump_traceback_later(exit=True)) is armed before the step and
disarmed after the device has finished it; when it fires it prints the stack and ends the process, also while the main thread is blocked
inside a HIP call."""
import argparse
import faulthandler
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(name, family, K, args):
    from basedet_amd import configs, models
    from basedet_amd.models import params as P
    from basedet_amd.solver import DetSolver
    from basedet_amd.utils import DummyLoader
    cfg = getattr(configs, "RetinaNetConfig" if family == "RetinaNet" else "FCOSConfig")()
    cfg.MODEL.BATCHSIZE = args.batch
    cfg.DATA.NUM_CLASSES = K
    params = (P.init_retinanet_params if family == "RetinaNet" else P.init_fcos_params)(cfg, 0)
    batch = next(DummyLoader(args.batch, (800, 1344), seed=0))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    gt = batch["gt_boxes"]
    gt[..., 4] = np.where(gt[..., 2] > gt[..., 0], (gt[..., 4].astype(np.int64) * 7) % K + 1, 0)        # classes spread over 1..K
    model = getattr(models, family)(cfg, params=params)
    solver = DetSolver.build(cfg, model)
    batch = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}       # resident in HBM before the timed region
    out = None
    t0 = None
    for it in range(args.warmup + args.steps):
        if it == args.warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        faulthandler.dump_traceback_later(args.step_limit, exit=True)
        out = solver.minimize(model, batch)
        torch.cuda.synchronize()          # (one host wait per step, < 0.1 % of it: the limit covers the step's execution, not its enqueue)
        faulthandler.cancel_dump_traceback_later()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    losses = {k: float(v) for k, v in out.items()}
    assert all(math.isfinite(v) for v in losses.values()), losses
    ld = getattr(model, "cls_ld", K)
    print(f"{name}: K={K} cls_ld={ld} batch={args.batch} {ms:.2f} ms/step {args.batch / ms * 1e3:.1f} img/s losses={losses}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    for name, family, K in (("retinanet", "RetinaNet", 365), ("fcos365", "FCOS", 365), ("fcos368", "FCOS", 368)):
        if args.only in (None, name):
            run(name, family, K, args)


if __name__ == "__main__":
    main()
