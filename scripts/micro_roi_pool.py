"""What the two poolers of the box head cost per launch: RoI max pooling (ROI_POOLER.METHOD = "roi_pool": bd_roi_pool_fwd,
bd_roi_pool_bwd_bf16) beside RoIAlign (bd_roi_align_fwd, bd_roi_align_bwd_bf16) on the same inputs.

The Faster R-CNN training shape: batch 16, 800 x 1344 (pyramid 200 x 336 down to 13 x 21), 512 RoIs per image, 7 x 7 bins, C = 256, bf16
N(0, 1) features.  The RoIs are proposal-like: side lengths log-uniform in 16 .. 700 pixels, aspect ratios 1/2 .. 2, clipped to the image;
one slot in eight is empty (label -1).  Four legs alternate on one device (`--rounds` alternations, `--iters` launches each, after a
warm-up of every leg); both backward legs accumulate on top of a gradient pyramid, as the training step does.
  bytes: `min bytes` is what a launch must move at least -- the pooled tensor once (written by a forward, read by a backward) plus the
  pyramid's RoI levels once; how often a window or a stencil is read again out of the caches is what the time shows.
`python scripts/micro_roi_pool.py [--iters K] [--rounds R] [--out FILE]`: one line per (round, leg), the table, and a JSON summary line;
`--out` also writes all of it to FILE (profiles/roi_pool_ab.txt is such a file)."""
import json
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from basedet_amd import ops  # noqa: E402
from micro_ema import _timed  # noqa: E402

N, IMG, S, POOL, C = 16, (800, 1344), 512, (7, 7), 256
STRIDES = [4, 8, 16, 32, 64]
NLEV = 4
LEGS = [("align fwd", "bd_roi_align_fwd"), ("pool fwd", "bd_roi_pool_fwd"), ("align bwd", "bd_roi_align_bwd_bf16"),
        ("pool bwd", "bd_roi_pool_bwd_bf16")]


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def inputs():
    geom = ops.Geom(N, [-(-IMG[0] // s) for s in STRIDES], [-(-IMG[1] // s) for s in STRIDES])
    rng = np.random.default_rng(0)
    side = np.exp(rng.uniform(np.log(16), np.log(700), (N, S)))
    ratio = np.exp(rng.uniform(np.log(0.5), np.log(2.0), (N, S)))
    w, h = side * np.sqrt(ratio), side / np.sqrt(ratio)
    cx, cy = rng.uniform(0, IMG[1], (N, S)), rng.uniform(0, IMG[0], (N, S))
    rois = np.stack([np.clip(cx - w / 2, 0, IMG[1]), np.clip(cy - h / 2, 0, IMG[0]), np.clip(cx + w / 2, 0, IMG[1]),
                     np.clip(cy + h / 2, 0, IMG[0])], -1).astype(np.float32)
    labels = rng.integers(0, 80, (N, S)).astype(np.int32)
    labels[:, ::8] = -1
    dev = "cuda"
    t = dict(geom=geom, rois=torch.from_numpy(rois).view(-1, 4).to(dev), labels=torch.from_numpy(labels).view(-1).to(dev),
             feat=torch.randn((geom.pixels, C), device=dev).to(torch.bfloat16),
             gout=torch.randn((N * S, POOL[0] * POOL[1] * C), device=dev).to(torch.bfloat16),
             out=torch.empty((N * S, POOL[0] * POOL[1] * C), dtype=torch.bfloat16, device=dev),
             gfeat=torch.zeros((geom.pixels, C), dtype=torch.bfloat16, device=dev))
    t["ws_align"] = torch.empty((ops.roi_align_bwd_bf16_workspace_bytes(geom, S),), dtype=torch.uint8, device=dev)
    t["ws_pool"] = torch.empty((ops.roi_pool_bwd_bf16_workspace_bytes(geom, S),), dtype=torch.uint8, device=dev)
    return t


def launches(rounds, iters, emit):
    t = inputs()
    g = t["geom"]
    fns = {
        "align fwd": lambda: ops.roi_align_fwd(t["feat"], g, NLEV, STRIDES, C, t["rois"], t["labels"], S, POOL, 2, t["out"]),
        "pool fwd": lambda: ops.roi_pool_fwd(t["feat"], g, NLEV, STRIDES, C, t["rois"], t["labels"], S, POOL, t["out"]),
        "align bwd": lambda: ops.roi_align_bwd_bf16(t["gout"], g, NLEV, STRIDES, C, t["rois"], t["labels"], S, POOL, 2, t["gfeat"], t["ws_align"],
                                                    accumulate=True),
        "pool bwd": lambda: ops.roi_pool_bwd_bf16(t["feat"], t["gout"], g, NLEV, STRIDES, C, t["rois"], t["labels"], S, POOL, t["gfeat"],
                                                  t["ws_pool"], accumulate=True),
    }
    for k, fn in fns.items():
        _timed(fn, 3)
        t["gfeat"].zero_()              # (thousands of accumulations on one gradient would overflow bf16)
    res = {k: [] for k, _ in LEGS}
    for rnd in range(rounds):
        for k, _ in LEGS:
            t["gfeat"].zero_()
            ms = _timed(fns[k], iters)
            res[k].append(ms * 1e3)
            emit(f"round {rnd} {k:10s} {ms * 1e3:9.1f} us")
    pooled = N * S * POOL[0] * POOL[1] * C * 2
    pyr = N * sum(g.H[l] * g.W[l] for l in range(NLEV)) * C * 2
    out = {"N": N, "image": IMG, "rois_per_img": S, "pool": POOL, "C": C, "min_bytes": pooled + pyr}
    for k, _ in LEGS:
        v = res[k]
        out[k] = {"us_median": round(statistics.median(v), 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1)}
    return out


def table(out, emit):
    emit("median (min .. max) over the alternations; last column: the leg's time over RoIAlign's")
    for k, entry in LEGS:
        r, base = out[k], out["align " + k.split()[1]]
        emit(f"  {entry:24s} {k:10s} {r['us_median']:9.1f} us ({r['us_min']:.1f} .. {r['us_max']:.1f})   "
             f"{out['min_bytes'] / r['us_median'] / 1e3:7.1f} GB/s of min bytes   {r['us_median'] / base['us_median']:.3f}")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("micro_roi_pool.py needs a HIP device")
    rounds, iters, path = _arg("--rounds", 5), _arg("--iters", 20), _arg("--out", None, str)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"box-head poolers alone, batch {N}, {IMG[0]} x {IMG[1]}, {S} RoIs per image, {POOL[0]} x {POOL[1]}, C = {C}; "
         f"`python scripts/micro_roi_pool.py --rounds {rounds} --iters {iters}`, the legs alternate inside one process")
    out = launches(rounds, iters, emit)
    table(out, emit)
    emit(json.dumps({"micro_roi_pool": out}))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
