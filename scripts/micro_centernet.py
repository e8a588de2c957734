"""Launch times of the CenterNet tail (csrc/centernet.hip) at the recipe's shape: batch 16, 80 classes, a 128 x 128 output map, T = 128.

Four legs alternate on one device (`--rounds` alternations of `--iters` calls each, after a warm-up of every leg), timed with device
events around back-to-back calls of one entry:
  targets  bd_centernet_targets        zero + draw the fp32 score map              84 MB written
  focal    bd_centernet_focal_fwd_bwd  bf16 logits + fp32 map -> bf16 gradient      42 + 84 + 42 = 168 MB
  l1       bd_centernet_l1_fwd_bwd     dense bf16 gradient of an 8-channel map       4 MB written (+ 2048 gathered rows)
  decode   bd_centernet_decode         bf16 logits -> fp32 peak map -> top-100      42 MB read + 84 MB written + 84 MB read once at least
The byte counts are what the arithmetic needs, from the shapes; GB/s is that count over the measured time, `floor_us` the count over
`--peak-gbps` (default 8000, the HBM3E figure of the MI355X).  The maps of one leg (up to 168 MB) fit the 256 MB last-level cache, which
a training step -- gigabytes of activations between two of these launches -- would have flushed: the legs rotate over `--copies`
independent operand sets (default 4) so that a call does not find its operands where the previous call of the leg left them.
`python scripts/micro_centernet.py [--iters K] [--rounds R] [--copies C]`; one line per (round, leg) and a JSON summary line."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from basedet_amd import ops  # noqa: E402

N, K, H, W, T, TOPK = 16, 80, 128, 128, 128, 100
LD = 80


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


def boxes(seed):
    """COCO-like load: 128 boxes per image on a 512 x 512 input, sides log-uniform in 8 .. 256 px."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 4 * W, (N, T, 2))
    s = 8 * 32 ** rng.random((N, T, 2))
    gt = np.concatenate([c - s / 2, c + s / 2, rng.integers(1, K + 1, (N, T, 1))], 2).astype(np.float32)
    return torch.from_numpy(gt).cuda(), torch.full((N,), T, dtype=torch.int32, device="cuda")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("micro_centernet.py needs a HIP device")
    rounds, iters, copies = _arg("--rounds", 5), _arg("--iters", 20), _arg("--copies", 4)
    peak = _arg("--peak-gbps", 8000)
    rows = N * H * W
    sets = []
    for c in range(copies):
        g = torch.Generator(device="cuda").manual_seed(c)
        gt, num = boxes(c)
        tg = ops.centernet_targets(gt, num, K, H, W, T, 0.25, 0.7)
        sets.append(dict(
            gt=gt, num=num, tg=tg, ws_t=torch.empty(int(ops.L().bd_centernet_targets_workspace_bytes(N)), dtype=torch.uint8, device="cuda"),
            logits=(torch.randn(rows, LD, generator=g, device="cuda") * 2 - 2).to(torch.bfloat16),
            dlogits=torch.empty(rows, LD, dtype=torch.bfloat16, device="cuda"),
            whreg=(torch.rand(rows, 8, generator=g, device="cuda") * 8).to(torch.bfloat16),
            dwhreg=torch.empty(rows, 8, dtype=torch.bfloat16, device="cuda"),
            loss=torch.zeros(1, device="cuda"),
            boxes=torch.empty(N, TOPK, 4, device="cuda"), scores=torch.empty(N, TOPK, device="cuda"),
            classes=torch.empty(N, TOPK, dtype=torch.int32, device="cuda"),
            ws_d=torch.empty(ops.centernet_decode_workspace_bytes(N, K, H, W), dtype=torch.uint8, device="cuda")))

    def targets(i):
        s = sets[i % copies]
        t = s["tg"]
        ops.centernet_targets_into(s["gt"], s["num"], N, T, K, H, W, T, 0.25, 0.7, t["score_map"], t["wh"], t["reg"], t["reg_mask"], t["index"],
                                   t["num_pos"], s["ws_t"])

    def focal(i):
        s = sets[i % copies]
        ops.centernet_focal_fwd_bwd(s["logits"], s["tg"]["score_map"], rows, K, LD, s["tg"]["num_pos"], 1.0, 1.0, s["loss"], s["dlogits"])

    def l1(i):
        s = sets[i % copies]
        ops.centernet_l1_fwd_bwd(s["whreg"], 8, 0, s["tg"]["index"], s["tg"]["reg_mask"], s["tg"]["wh"], N, H, W, T, 0.1, 1.0, s["loss"],
                                 s["dwhreg"])

    def decode(i):
        s = sets[i % copies]
        ops.centernet_decode(s["logits"], LD, s["whreg"], 8, 0, s["whreg"], 8, 2, N, K, H, W, TOPK, s["boxes"], s["scores"], s["classes"],
                             s["ws_d"])

    map_b, lg_b = rows * K * 4, rows * LD * 2
    legs = {"targets": (targets, map_b), "focal": (focal, lg_b + map_b + lg_b), "l1": (l1, rows * 8 * 2 + N * T * (16 + 4 + 4 + 8)),
            "decode": (decode, lg_b + map_b + map_b)}
    for fn, _ in legs.values():
        _timed(fn, 2 * copies)
    res = {k: [] for k in legs}
    for rnd in range(rounds):
        for k, (fn, nbytes) in legs.items():
            ms = _timed(fn, iters)
            res[k].append(ms * 1e3)
            print(f"round {rnd} {k:8s} {ms * 1e3:9.1f} us  {nbytes / ms / 1e6:8.1f} GB/s of {nbytes / 1e6:.1f} MB", flush=True)
    out = {"shape": dict(N=N, K=K, H=H, W=W, T=T, k=TOPK), "num_pos": [float(s["tg"]["num_pos"][0]) for s in sets]}
    for k, t in res.items():
        nbytes = legs[k][1]
        med = statistics.median(t)
        out[k] = {"us_median": round(med, 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1), "MB": round(nbytes / 1e6, 1),
                  "GBps_at_median": round(nbytes / med / 1e3, 1), "floor_us": round(nbytes / peak / 1e3, 1)}
    print(json.dumps({"micro_centernet": out}))


if __name__ == "__main__":
    main()
