"""What the moving average of the weights (TRAINER.EMA) costs per step, on the RetinaNet-R50 parameter arena.

Three legs alternate on one device (`--rounds` alternations, `--iters` launches each, after a warm-up of every leg):
  (a) bd_sgd_momentum_step alone                    20 B/param   (read w, v, g; write w, v)
  (b) (a) followed by bd_ema_update                 32 B/param   (+ read w, e; write e)
  (c) bd_sgd_momentum_ema_step                      28 B/param   (read w, v, g, e; write w, v, e)
The byte counts are what the arithmetic needs; GB/s is that count over the measured time.  Back-to-back launches over four 151 MB buffers
can keep part of them in the last-level cache, which a training step (gigabytes of activations between two optimizer launches) does
not: `--step` therefore also times the whole training step of the flagship workload (RetinaNet-R50, batch 16, 800 x 1344, DummyLoader
batch resident on the device, as bench.py runs it) with EMA off, fused into the SGD launch, and as a separate pass, alternating.
`python scripts/micro_ema.py [--iters K] [--rounds R] [--step [--step-iters S]]`; one line per (round, leg) and a JSON summary line."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from basedet_amd import ops  # noqa: E402

BYTES = {"sgd": 20, "sgd+ema": 32, "fused": 28}


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def arena_elements():
    """Length of the trainable arena of RetinaNet-R50 (FREEZE_AT = 2)."""
    from basedet_amd.configs import RetinaNetConfig
    from basedet_amd.models import RetinaNet
    cfg = RetinaNetConfig()
    cfg.MODEL.BATCHSIZE = 16
    model = RetinaNet(cfg)
    n = model.arena.total
    del model
    torch.cuda.empty_cache()
    return n


def launches(rounds, iters):
    n = arena_elements()
    w, v, g, e = (torch.randn(n, device="cuda") * s for s in (0.05, 0.01, 0.01, 0.05))
    lr, mom, wd, m = 1e-6, 0.9, 1e-4, 0.9995          # a tiny rate: thousands of launches on one gradient must stay finite
    legs = {
        "sgd": lambda: ops.sgd_momentum_step(w, v, g, lr, mom, wd, 1.0),
        "sgd+ema": lambda: (ops.sgd_momentum_step(w, v, g, lr, mom, wd, 1.0), ops.ema_update(e, w, m)),
        "fused": lambda: ops.sgd_momentum_ema_step(w, v, g, e, lr, mom, wd, 1.0, m),
    }
    for fn in legs.values():
        _timed(fn, 10)
    res = {k: [] for k in legs}
    for rnd in range(rounds):
        for k, fn in legs.items():
            ms = _timed(fn, iters)
            res[k].append(ms * 1e3)
            print(f"round {rnd} {k:8s} {ms * 1e3:8.1f} us  {BYTES[k] * n / ms / 1e6:7.1f} GB/s at {BYTES[k]} B/param", flush=True)
    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(e).all())
    out = {"elements": n}
    for k, t in res.items():
        out[k] = {"us_median": round(statistics.median(t), 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1),
                  "GBps_at_median": round(BYTES[k] * n / statistics.median(t) / 1e3, 1), "bytes_per_param": BYTES[k]}
    out["fused_not_slower_than_separate"] = out["fused"]["us_median"] <= out["sgd+ema"]["us_median"]
    return out


def steps(rounds, iters):
    from basedet_amd.configs import RetinaNetConfig
    from basedet_amd.layers import ModelEMA
    from basedet_amd.models import RetinaNet, params as P
    from basedet_amd.solver import DetSolver
    from basedet_amd.utils import DummyLoader
    N, size = 16, (800, 1344)
    cfg = RetinaNetConfig()
    cfg.MODEL.BATCHSIZE = N
    model = RetinaNet(cfg, params=P.init_retinanet_params(cfg, seed=0, residual_gamma=0.2))
    solver = DetSolver.build(cfg, model)
    solver.optimizer.param_groups[0]["lr"] = 1e-5
    hb = next(DummyLoader(N, size, seed=0))
    batch = {"data": torch.from_numpy(hb["data"].astype(np.float32)).cuda(), "gt_boxes": torch.from_numpy(hb["gt_boxes"]).cuda(),
             "im_info": torch.from_numpy(hb["im_info"]).cuda()}
    ema = ModelEMA(model, 0.9995, burnin_iter=0)

    def off():
        solver.minimize(model, batch)

    def fused():
        solver.minimize(model, batch, ema=ema)
        ema.step()

    def separate():
        solver.minimize(model, batch)
        ema.step()

    legs = {"ema off": off, "ema fused": fused, "ema separate": separate}
    for fn in legs.values():
        _timed(fn, 5)
    res = {k: [] for k in legs}
    for rnd in range(rounds):
        for k, fn in legs.items():
            ms = _timed(fn, iters)
            res[k].append(ms)
            print(f"round {rnd} step, {k:12s} {ms:8.2f} ms  {N / ms * 1e3:7.1f} img/s", flush=True)
    return {k: {"ms_median": round(statistics.median(t), 2), "ms_min": round(min(t), 2), "ms_max": round(max(t), 2),
                "img_per_s_at_median": round(N / statistics.median(t) * 1e3, 1)} for k, t in res.items()}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("micro_ema.py needs a HIP device")
    rounds = _arg("--rounds", 5)
    out = {"micro_ema": launches(rounds, _arg("--iters", 50))}
    if "--step" in sys.argv:
        out["train_step_retinanet_r50_b16"] = steps(rounds, _arg("--step-iters", 15))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
