"""Multi-scale training run on the synthetic recipe stream (DATA.DUMMY_MULTISCALE): K steps of one model, one JSON line.

    python scripts/multiscale_run.py --model retinanet --batch 16 --steps 60 [--max-shapes 8] [--plan-sizes] [--workers 12]

Batches come from MultiScaleDummyLoader (AUG.TRAIN_VALUE resize + flip, aspect grouping, pad collation) and are made ahead of the
device in worker processes (the numpy resize costs far more than a step).  --max-shapes S keeps the first S distinct padded shapes of
the stream and skips batches of any other (a sequence short enough for a build that keeps one plan per shape).  Each step is timed
alone (forward + backward + optimizer step, synchronised): img/s counts the steps that are not a shape's first visit, and the first
visits' mean time is reported apart.  Memory: torch.cuda.memory_allocated / memory_reserved at the end and their peaks; the plan
arena's bytes; with --plan-sizes, the bytes of one plan at 16 x 800 x 1344 for RetinaNet, FCOS and Faster R-CNN (R50)."""
import argparse
import concurrent.futures as cf
import json
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _configs():
    from basedet_amd.configs import FasterRCNNConfig, FCOSConfig, RetinaNetConfig
    return {"retinanet": RetinaNetConfig, "fcos": FCOSConfig, "faster_rcnn": FasterRCNNConfig}


def _model(name, batch, backbone="resnet50"):
    from basedet_amd.models import FCOS, FasterRCNN, RetinaNet, params as P
    cfg = _configs()[name]()
    cfg.MODEL.BATCHSIZE = batch
    cfg.MODEL.BACKBONE.NAME = backbone
    cls, init = {"retinanet": (RetinaNet, P.init_retinanet_params), "fcos": (FCOS, P.init_fcos_params),
                 "faster_rcnn": (FasterRCNN, P.init_faster_rcnn_params)}[name]
    return cfg, cls(cfg, params=init(cfg, seed=0))


def plan_bytes(model, pl):
    """Device bytes of one plan's per-step buffers: the carved layout where plans live in the arena, else the plan's own tensors."""
    if hasattr(model, "plan_bytes"):
        return int(model.plan_bytes(pl))
    seen, total = set(), 0

    def walk(v):
        nonlocal total
        if torch.is_tensor(v):
            s = v.untyped_storage()
            if s.data_ptr() not in seen:
                seen.add(s.data_ptr())
                total += s.nbytes()
        elif isinstance(v, (list, tuple)):
            for x in v:
                walk(x)
        elif isinstance(v, dict):
            for x in v.values():
                walk(x)
        elif hasattr(v, "__dict__") and type(v).__name__ == "_Plan":
            for x in v.__dict__.values():
                walk(x)
    walk(pl)
    # per-shape constants are not per-step buffers
    for k in ("anchors", "points"):
        t = getattr(pl, k, None)
        if torch.is_tensor(t):
            total -= t.untyped_storage().nbytes()
    return total


def _make(args):
    loader, b, idx = args
    return b, loader.make_batch(b, idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="retinanet", choices=sorted(_configs()))
    ap.add_argument("--backbone", default="resnet50")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--max-shapes", type=int, default=0, help="keep only the first S distinct padded shapes of the stream (0: all)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--plan-sizes", action="store_true", help="also report the bytes of one 16 x 800 x 1344 plan per detector")
    ap.add_argument("--mem-at", type=int, default=0, help="also report held memory after this many steps")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    from basedet_amd.solver import DetSolver
    from basedet_amd.utils.dummy import MultiScaleDummyLoader

    out = {}
    if args.plan_sizes:
        for name in ("retinanet", "fcos", "faster_rcnn"):
            _, m = _model(name, 16)
            out[f"plan_bytes_{name}_16x800x1344"] = plan_bytes(m, m._plan(16, 800, 1344))
            del m
            torch.cuda.empty_cache()

    cfg, model = _model(args.model, args.batch, args.backbone)
    solver = DetSolver.build(cfg, model)
    solver.optimizer.param_groups[0]["lr"] = 1e-4
    loader = MultiScaleDummyLoader(args.batch, cfg.AUG.TRAIN_VALUE, seed=args.seed)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    alloc0 = torch.cuda.memory_allocated()

    # the shape of a batch is known from its indices only after the resize: pick the batches in the workers' output order
    pool = cf.ProcessPoolExecutor(max_workers=args.workers, mp_context=mp.get_context("spawn"))     # fresh children: no GPU state
    pending = []

    def refill():
        while len(pending) < 2 * args.workers:
            b, idx = loader.next_indices()
            pending.append(pool.submit(_make, (loader, b, idx)))

    seen, visits = {}, {}
    first_t, steady_t, steady_img = [], 0.0, 0
    losses = []
    mem_at = None
    step = 0
    t_start = time.perf_counter()
    while step < args.steps:
        refill()
        _, batch = pending.pop(0).result()
        N, _, H, W = batch["data"].shape
        key = (N, (H + 31) // 32 * 32, (W + 31) // 32 * 32)
        if key not in seen and args.max_shapes and len(seen) >= args.max_shapes:
            continue
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = solver.minimize(model, batch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        losses.append(float(o["total_loss"]))
        if key in seen:
            steady_t += dt
            steady_img += N
        else:
            first_t.append(dt)
            seen[key] = step
        visits[key] = visits.get(key, 0) + 1
        step += 1
        if step % 100 == 0:
            print(f"step {step}: {len(seen)} shapes, {time.perf_counter() - t_start:.0f} s", file=sys.stderr, flush=True)
        if args.mem_at and step == args.mem_at:
            mem_at = dict(allocated=torch.cuda.memory_allocated() - alloc0, reserved=torch.cuda.memory_reserved())
    pool.shutdown(cancel_futures=True)
    torch.cuda.synchronize()
    out.update(dict(
        model=args.model, backbone=args.backbone, batch=args.batch, steps=args.steps, distinct_shapes=len(seen),
        min_visits=min(visits.values()), shapes=[list(k[1:]) for k in seen],
        img_per_s_steady=(steady_img / steady_t) if steady_t > 0 else None,
        first_visit_ms_mean=1e3 * float(np.mean(first_t)), losses_finite=bool(np.all(np.isfinite(losses))),
        loss_first=losses[0], loss_last=losses[-1],
        memory_allocated_end=torch.cuda.memory_allocated() - alloc0, memory_allocated_peak=torch.cuda.max_memory_allocated() - alloc0,
        memory_reserved_end=torch.cuda.memory_reserved(), memory_reserved_peak=torch.cuda.max_memory_reserved(),
        arena_bytes=int(getattr(model, "arena_bytes", 0)), plans=len(model._plans)))
    if mem_at is not None:
        out[f"memory_after_{args.mem_at}_steps"] = mem_at
    print(json.dumps(out))


if __name__ == "__main__":
    main()
