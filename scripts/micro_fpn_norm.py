"""Per-launch timing of the four batch-norm kernels (csrc/batchnorm.hip) at the five RetinaNet level sizes of a batch of 16 at 800 x 1344,
256 channels, against the bytes each pass must move (bf16 tensors; the fp32 vectors and partial sums are noise): statistics read y;
apply reads y and writes z; the backward reduction reads g and y; the backward apply reads g and y and writes g_y.
`python scripts/micro_fpn_norm.py [--iters K]`; one line per (level, kernel) and a JSON summary line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from basedet_amd import ops  # noqa: E402

LEVELS = ((100, 168), (50, 84), (25, 42), (13, 21), (7, 11))


def _timed(fn, iters):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 20
    N, C = 16, 256
    f = lambda: torch.ones(C, dtype=torch.float32, device="cuda")
    out = {}
    for H, W in LEVELS:
        geo = ops.single(N, H, W)
        M = geo.pixels
        y = (torch.randn(M, C, device="cuda") * 2 + 1).to(torch.bfloat16)
        g = torch.randn(M, C, device="cuda").to(torch.bfloat16)
        z, gy = torch.empty_like(y), torch.empty_like(y)
        mean, inv_std, gamma, beta, dg, db, rm, rv = (f() for _ in range(8))
        sums = torch.empty((3, C), dtype=torch.float32, device="cuda")
        ws = torch.empty(ops.bn_workspace_bytes(M, C) // 4 + 64, dtype=torch.float32, device="cuda")
        t = M * C * 2          # bytes of one bf16 tensor
        runs = {
            "stats_fwd": (lambda: ops.bn_stats_fwd(y, geo, C, 1e-5, 0.1, mean, inv_std, sums, rm, rv, ws), t),
            "apply_fwd": (lambda: ops.bn_apply_act_fwd(y, geo, mean, inv_std, gamma, beta, z, geo, C, relu=False), 2 * t),
            "bwd_reduce": (lambda: ops.bn_bwd_reduce(g, geo, y, geo, mean, inv_std, C, dg, db, ws), 2 * t),
            "bwd_apply": (lambda: ops.bn_bwd_apply(g, geo, y, geo, mean, inv_std, gamma, dg, db, sums[0], gy, geo, C), 3 * t),
        }
        for name, (fn, nbytes) in runs.items():
            ms = _timed(fn, iters)
            out[f"{H}x{W} {name}"] = (round(ms * 1e3, 1), round(nbytes / ms / 1e6, 1))
            print(f"{H:3d}x{W:<3d} {name:10s} {ms * 1e3:8.1f} us  {nbytes / 1e6:7.1f} MB  {nbytes / ms / 1e6:7.1f} GB/s", flush=True)
    print(json.dumps({"micro_fpn_norm_us_gbps": out}))


if __name__ == "__main__":
    main()
