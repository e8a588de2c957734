"""What one optimizer launch costs per step, on the RetinaNet-R50 parameter arena: the four launches of csrc/optim.hip next to the two SGD
launches they stand beside (SOLVER.OPTIMIZER_NAME).

Six legs alternate on one device (`--rounds` alternations, `--iters` launches each, after a warm-up of every leg):
  bd_sgd_momentum_step          20 B/param   (read w, v, g; write w, v)
  bd_sgd_momentum_ema_step      28 B/param   (+ read e; write e)
  bd_sgd_nesterov_step          20 B/param
  bd_sgd_nesterov_ema_step      28 B/param
  bd_adam_step (AdamW)          28 B/param   (read w, m, v, g; write w, m, v)
  bd_adam_ema_step (AdamW)      36 B/param   (+ read e; write e)
The byte counts are what the arithmetic needs; GB/s is that count over the measured time.  Back-to-back launches over 151 MB buffers can
keep part of them in the last-level cache, which a training step does not (scripts/micro_ema.py --step times whole steps).
`python scripts/micro_optim.py [--iters K] [--rounds R] [--out FILE]`: one line per (round, leg), the table, and a JSON summary line;
`--out` also writes all of it to FILE (profiles/optim_step.txt is such a file)."""
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from basedet_amd import ops  # noqa: E402
from micro_ema import _timed, arena_elements  # noqa: E402

LEGS = [("sgd", "bd_sgd_momentum_step", 20), ("sgd+ema", "bd_sgd_momentum_ema_step", 28),
        ("nesterov", "bd_sgd_nesterov_step", 20), ("nesterov+ema", "bd_sgd_nesterov_ema_step", 28),
        ("adamw", "bd_adam_step", 28), ("adamw+ema", "bd_adam_ema_step", 36)]
BASELINE = "sgd+ema"


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def launches(rounds, iters, emit):
    n = arena_elements()
    w, v, g, e = (torch.randn(n, device="cuda") * s for s in (0.05, 0.01, 0.01, 0.05))
    v2 = torch.rand(n, device="cuda") * 1e-4                  # a second moment: non-negative
    lr, mom, wd, m, betas, eps = 1e-6, 0.9, 1e-4, 0.9995, (0.9, 0.999), 1e-8      # a tiny rate: thousands of launches must stay finite
    step = 1000                                               # (the bias corrections are arguments: the step number costs nothing)
    fns = {
        "sgd": lambda: ops.sgd_momentum_step(w, v, g, lr, mom, wd, 1.0),
        "sgd+ema": lambda: ops.sgd_momentum_ema_step(w, v, g, e, lr, mom, wd, 1.0, m),
        "nesterov": lambda: ops.sgd_nesterov_step(w, v, g, lr, mom, wd, 1.0),
        "nesterov+ema": lambda: ops.sgd_nesterov_ema_step(w, v, g, e, lr, mom, wd, 1.0, m),
        "adamw": lambda: ops.adam_step(w, v, v2, g, lr, betas, eps, wd, step, 1.0, True),
        "adamw+ema": lambda: ops.adam_ema_step(w, v, v2, g, e, lr, betas, eps, wd, step, 1.0, True, m),
    }
    for fn in fns.values():
        _timed(fn, 10)
    res = {k: [] for k, _, _ in LEGS}
    for rnd in range(rounds):
        for k, _, nbytes in LEGS:
            ms = _timed(fns[k], iters)
            res[k].append(ms * 1e3)
            emit(f"round {rnd} {k:13s} {ms * 1e3:8.1f} us  {nbytes * n / ms / 1e6:7.1f} GB/s at {nbytes} B/param")
    assert all(bool(torch.isfinite(t).all()) for t in (w, v, v2, e))
    out = {"elements": n}
    for k, _, nbytes in LEGS:
        t = res[k]
        gbps = [nbytes * n / us / 1e3 for us in t]
        out[k] = {"us_median": round(statistics.median(t), 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1),
                  "GBps_at_median": round(nbytes * n / statistics.median(t) / 1e3, 1), "GBps_min": round(min(gbps), 1),
                  "GBps_max": round(max(gbps), 1), "bytes_per_param": nbytes}
    return out


def table(out, emit):
    base = out[BASELINE]
    emit(f"median (min .. max) over the alternations; last column: achieved GB/s over that of bd_sgd_momentum_ema_step "
         f"({base['GBps_at_median']:.1f} GB/s, {base['GBps_min']:.1f} .. {base['GBps_max']:.1f} between alternations)")
    for k, entry, nbytes in LEGS:
        r = out[k]
        emit(f"  {entry:26s} {k:13s} {nbytes} B/param   {r['us_median']:7.1f} us ({r['us_min']:.1f} .. {r['us_max']:.1f})   "
             f"{r['GBps_at_median']:7.1f} GB/s   {r['GBps_at_median'] / base['GBps_at_median']:.3f}")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("micro_optim.py needs a HIP device")
    rounds, iters, path = _arg("--rounds", 5), _arg("--iters", 50), _arg("--out", None, str)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"optimizer launches alone, RetinaNet-R50 arena; `python scripts/micro_optim.py --rounds {rounds} --iters {iters}`, the legs "
         f"alternate inside one process; GB/s = the leg's byte count / time")
    out = launches(rounds, iters, emit)
    emit(f"{out['elements']} fp32 elements per buffer")
    table(out, emit)
    emit(json.dumps({"micro_optim": out}))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
