"""The YOLOX detector as a whole at YOLOX-s's shapes (depth 0.33, width 0.5), batch 16, a 640 x 640 loader batch resized to 512 and to 800.

Protocol of scripts/micro_yolox_neck.py: device events around back-to-back calls of one leg, `--rounds` alternations of `--iters` calls
after a warm-up of every leg, operands rotating over `--copies` independent sets so that a call does not find them in the last-level cache.
Legs, all in one process:
  resize_512 / resize_800   bd_resize_bilinear_normalize, [16][3][640][640] fp32 -> the bf16 halo image; bytes = the input read once
                            plus the output written once, the floor = bytes / `--peak-gbps`
  step_512 / step_800       one Solver.minimize of the model (pre_process with the resize, forward, losses, backward, the two
                            optimizer launches, the repack) at that target_size
  infer_640                 one inference_batch in eval() on the 640 x 640 batch
`python scripts/micro_yolox_model.py [--iters K] [--rounds R] [--copies C] [--peak-gbps G]`; one line per (round, leg), a JSON summary line.
Nothing is asserted about time."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from basedet_amd import ops  # noqa: E402
from basedet_amd.configs import YOLOXConfig  # noqa: E402
from basedet_amd.models import YOLOX  # noqa: E402
from basedet_amd.solver import YOLOXSolver  # noqa: E402

N, H, W = 16, 640, 640
SIZES = (512, 800)


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(iters):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    if not torch.cuda.is_available():
        raise SystemExit("micro_yolox_model.py needs a HIP device")
    rounds, iters, copies, peak = _arg("--rounds", 5), _arg("--iters", 10), _arg("--copies", 3), _arg("--peak-gbps", 8000)
    dev = "cuda"
    cfg = YOLOXConfig()
    cfg.MODEL.DEPTH_FACTOR, cfg.MODEL.WIDTH_FACTOR, cfg.MODEL.BATCHSIZE = 0.33, 0.5, N
    model = YOLOX(cfg)
    solver = YOLOXSolver.build(cfg, model)
    rng = np.random.default_rng(0)
    batches = []
    for _ in range(copies):
        gt = np.zeros((N, 8, 5), np.float32)
        for i in range(N):
            for j in range(8):
                cx, cy, w, h = rng.uniform(64, W - 64), rng.uniform(64, H - 64), rng.uniform(24, 200), rng.uniform(24, 200)
                gt[i, j] = [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, 1 + rng.integers(80)]
        batches.append({"data": torch.from_numpy(rng.uniform(0, 255, (N, 3, H, W)).astype(np.float32)).to(dev),
                        "gt_boxes": torch.from_numpy(gt).to(dev),
                        "im_info": torch.tensor([[H, W, H, W, 8]] * N, dtype=torch.float32, device=dev)})
    legs = {}
    for s in SIZES:
        halo = torch.empty((N, s + 6, s + 8, 4), dtype=torch.bfloat16, device=dev)
        legs[f"resize_{s}"] = ((lambda i, s=s, halo=halo: ops.resize_bilinear_normalize(batches[i % copies]["data"], s, s, s, s, (0, 0, 0),
                                                                                       (1, 1, 1), halo)), N * 3 * H * W * 4 + halo.numel() * 2)

        def step(i, s=s):
            model.target_size = (s, s)
            solver.minimize(model, batches[i % copies])
        legs[f"step_{s}"] = (step, 0)

    def infer(i):
        model.inference_batch({"data": batches[i % copies]["data"]})

    res = {k: [] for k in list(legs) + ["infer_640"]}
    model.train()
    for fn, _ in legs.values():
        _timed(fn, copies)
    model.eval()
    _timed(infer, copies)
    for rnd in range(rounds):
        model.train()
        for k, (fn, nbytes) in legs.items():
            ms = _timed(fn, iters)
            res[k].append(ms * 1e3)
            tail = f"  {nbytes / ms / 1e6:8.1f} GB/s of {nbytes / 1e6:.1f} MB" if nbytes else ""
            print(f"round {rnd} {k:12s} {ms * 1e3:9.1f} us{tail}", flush=True)
        model.eval()          # (the host reads the N detection counts: the leg includes that synchronisation)
        ms = _timed(infer, iters)
        res["infer_640"].append(ms * 1e3)
        print(f"round {rnd} {'infer_640':12s} {ms * 1e3:9.1f} us", flush=True)
    out = {"shape": dict(N=N, H=H, W=W, depth=0.33, width=0.5, sizes=list(SIZES))}
    for k, t in res.items():
        nbytes = legs[k][1] if k in legs else 0
        med = statistics.median(t)
        out[k] = {"us_median": round(med, 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1)}
        if nbytes:
            out[k].update({"MB": round(nbytes / 1e6, 1), "GBps_at_median": round(nbytes / med / 1e3, 1), "floor_us": round(nbytes / peak / 1e3, 1)})
    print(json.dumps({"micro_yolox_model": out}))


if __name__ == "__main__":
    main()
