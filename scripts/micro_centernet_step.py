"""The CenterNet-R50 training step at the recipe's shape: batch 16, 512 x 512 input, 80 classes, OUTPUT_SIZE (128, 128).

Protocol of scripts/micro_center_head.py: device events around back-to-back calls of one leg, `--rounds` alternations of `--iters` calls
after a warm-up of every leg, all in one process (the backward leg: ONE call per round, behind the forward it needs).  Legs:
  forward     model(batch): pre-processing, trunk, neck, head, targets and the three losses
  backward    model.backward(): head, neck, trunk
  optimizer   the fused SGD launch over the arena and the repack of every bf16 operand
  step        solver.minimize(model, batch): the three together
`python scripts/micro_centernet_step.py [--iters K] [--rounds R] [--batch N] [--out FILE]`; one line per (round, leg) and a JSON summary
line, also written to FILE (default profiles/centernet_step.txt).  No earlier measurement of this model exists: the numbers stand alone."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from basedet_amd.configs import CenterNetConfig  # noqa: E402
from basedet_amd.models import CenterNet  # noqa: E402
from basedet_amd.solver import DetSolver  # noqa: E402


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    if not torch.cuda.is_available():
        raise SystemExit("micro_centernet_step.py needs a HIP device")
    rounds, iters, N = _arg("--rounds", 5), _arg("--iters", 5), _arg("--batch", 16)
    out_path = _arg("--out", os.path.join(ROOT, "profiles", "centernet_step.txt"), str)
    cfg = CenterNetConfig()
    cfg.MODEL.BATCHSIZE, cfg.MODEL.WEIGHTS = N, None
    model = CenterNet(cfg)
    solver = DetSolver.build(cfg, model)
    rng = np.random.default_rng(0)
    G = 32
    xy = rng.uniform(0, 384, (N, G, 2))
    wh = rng.uniform(8, 128, (N, G, 2))
    gt = np.concatenate([xy, np.minimum(xy + wh, 512), rng.integers(1, 81, (N, G, 1))], -1).astype(np.float32)
    batch = dict(data=torch.from_numpy(rng.uniform(0, 255, (N, 3, 512, 512)).astype(np.float32)).cuda(), gt_boxes=torch.from_numpy(gt).cuda(),
                 im_info=torch.tensor([[512, 512, 512, 512, G]] * N, dtype=torch.float32).cuda())
    legs = dict(forward=lambda: model(batch), backward=lambda: model.backward(), optimizer=lambda: solver.optimizer.step(),
                step=lambda: solver.minimize(model, batch))
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    lines, times = [], {k: [] for k in legs}
    for r in range(rounds):
        for name, fn in legs.items():
            if name == "backward":
                model(batch)                    # (a backward needs the forward of its step)
            ms = _timed(fn, iters if name != "backward" else 1)
            times[name].append(ms)
            lines.append(f"round {r} {name:9s} {ms:9.3f} ms")
            print(lines[-1])
    summary = dict(model="CenterNet-R50", batch=N, input=[512, 512], rounds=rounds, iters={k: (1 if k == "backward" else iters) for k in legs},
                   median_ms={k: round(statistics.median(v), 3) for k, v in times.items()},
                   img_per_s_step=round(N / statistics.median(times["step"]) * 1e3, 1), device=torch.cuda.get_device_name(0))
    lines.append(json.dumps(summary))
    print(lines[-1])
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
