"""conv -> BN -> SiLU and YOLOXHead at the recipe's shape: batch 16, 640 x 640 input -> levels 80 x 80 / 40 x 40 / 20 x 20 with 256 / 512 / 1024
channels, mid 256, K = 80.

Protocol of scripts/micro_center_head.py: device events around back-to-back calls of one leg, `--rounds` alternations of `--iters` calls
after a warm-up of every leg, operands rotating over `--copies` independent sets so that a call does not find them in the last-level cache.
Legs, all in one process:
  silu_fwd                 bd_bn_silu_fwd on [16 80 80][256] (read y, write z: 4 bytes per element)
  silu_bwd                 bd_bn_silu_bwd_reduce + bd_bn_silu_bwd_apply (read g, y; read g, y, write gy: 10 bytes per element)
  relu_bwd                 the ReLU chain of the same shape: bd_relu_bwd_bf16 + bd_bn_bwd_reduce + bd_bn_bwd_apply (14 bytes per element)
  head_l{0,1,2}_{fwd,bwd}  forward_pm / backward_pm of a one-level YOLOXHead at 80^2 / 40^2 / 20^2, 256 / 512 / 1024 -> 256
`python scripts/micro_yolox_head.py [--iters K] [--rounds R] [--copies C] [--peak-gbps G]`; one line per (round, leg), a JSON summary line."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from basedet_amd import ops  # noqa: E402
from basedet_amd.layers import YOLOXHead  # noqa: E402

N, K, MID = 16, 80, 256
LEVELS = [(80, 80, 256), (40, 40, 512), (20, 20, 1024)]
H, W, C = 80, 80, 256
M = N * H * W
BF, F32 = torch.bfloat16, torch.float32
EPS, MOM = 1e-3, 0.03


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
        raise SystemExit("micro_yolox_head.py needs a HIP device")
    rounds, iters, copies, peak = _arg("--rounds", 5), _arg("--iters", 10), _arg("--copies", 3), _arg("--peak-gbps", 8000)
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    e = lambda *s, dt=BF: torch.empty(s, dtype=dt, device=dev)
    geom = ops.single(N, H, W)
    gamma, beta = 1 + 0.3 * rn(C), 0.5 * rn(C)
    ws = e(ops.bn_workspace_bytes(M, C), dt=torch.uint8)
    sets = []
    for _ in range(copies):
        s = dict(y=rn(M, C).to(BF), g=(0.1 * rn(M, C)).to(BF), z=e(M, C), gm=e(M, C), gy=e(M, C), mean=e(C, dt=F32), inv_std=e(C, dt=F32),
                 sums=e(3, C, dt=F32), dg=e(C, dt=F32), db=e(C, dt=F32))
        ops.bn_stats_fwd(s["y"], geom, C, EPS, MOM, s["mean"], s["inv_std"], s["sums"], None, None, ws)
        ops.bn_apply_act_fwd(s["y"], geom, s["mean"], s["inv_std"], gamma, beta, s["z"], geom, C, relu=True)
        s["zr"] = s["z"].clone()
        sets.append(s)

    def silu_fwd(i):
        s = sets[i % copies]
        ops.bn_silu_fwd(s["y"], geom, s["mean"], s["inv_std"], gamma, beta, s["z"], geom, C)

    def silu_bwd(i):
        s = sets[i % copies]
        ops.bn_silu_bwd_reduce(s["g"], geom, s["y"], geom, s["mean"], s["inv_std"], gamma, beta, C, s["dg"], s["db"], ws)
        ops.bn_silu_bwd_apply(s["g"], geom, s["y"], geom, s["mean"], s["inv_std"], gamma, beta, s["dg"], s["db"], s["sums"][0], s["gy"], geom, C)

    def relu_bwd(i):
        s = sets[i % copies]
        ops.relu_bwd_bf16(s["g"], s["zr"], s["gm"])
        ops.bn_bwd_reduce(s["gm"], geom, s["y"], geom, s["mean"], s["inv_std"], C, s["dg"], s["db"], ws)
        ops.bn_bwd_apply(s["gm"], geom, s["y"], geom, s["mean"], s["inv_std"], gamma, s["dg"], s["db"], s["sums"][0], s["gy"], geom, C)

    el = M * C
    legs = {"silu_fwd": (silu_fwd, 4 * el), "silu_bwd": (silu_bwd, 10 * el), "relu_bwd": (relu_bwd, 14 * el)}
    for l, (h, w, c) in enumerate(LEVELS):
        head = YOLOXHead(K, [c], MID)
        P = h * w
        xs = [rn(N * P, c).to(BF) for _ in range(copies)]
        dc = [(0.01 * rn(N * P, K)).to(BF) for _ in range(copies)]
        db = [torch.cat([0.01 * rn(N * P, 5), torch.zeros(N * P, 3, device=dev)], 1).to(BF) for _ in range(copies)]
        legs[f"head_l{l}_fwd"] = ((lambda i, hd=head, xs=xs, h=h, w=w: hd.forward_pm([xs[i % copies]], N, [(h, w)])), 0)
        legs[f"head_l{l}_bwd"] = ((lambda i, hd=head, dc=dc, db=db: hd.backward_pm(dc[i % copies], db[i % copies])), 0)

    for fn, _ in legs.values():
        _timed(fn, copies)
    res = {k: [] for k in legs}
    for rnd in range(rounds):
        for k, (fn, nbytes) in legs.items():
            ms = _timed(fn, iters)
            res[k].append(ms * 1e3)
            tail = f"  {nbytes / ms / 1e6:8.1f} GB/s of {nbytes / 1e6:.1f} MB" if nbytes else ""
            print(f"round {rnd} {k:12s} {ms * 1e3:9.1f} us{tail}", flush=True)
    out = {"shape": dict(N=N, K=K, mid=MID, levels=LEVELS)}
    for k, t in res.items():
        nbytes = legs[k][1]
        med = statistics.median(t)
        out[k] = {"us_median": round(med, 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1)}
        if nbytes:
            out[k].update({"MB": round(nbytes / 1e6, 1), "GBps_at_median": round(nbytes / med / 1e3, 1), "floor_us": round(nbytes / peak / 1e3, 1)})
    print(json.dumps({"micro_yolox_head": out}))


if __name__ == "__main__":
    main()
