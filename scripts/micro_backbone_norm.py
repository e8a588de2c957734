"""Per-launch timing of the batch-norm launches MODEL.BACKBONE.NORM = "BN" / "SyncBN" adds to the step (csrc/batchnorm.hip), at the layer1,
layer2 and layer4 output shapes of a batch of 16 at 800 x 1344, against the bytes each pass must move (bf16 tensors; the fp32 vectors and
partial sums are noise): statistics read y; bd_bn_apply_act_fwd reads y (and the residual) and writes z; the backward reduction reads g
and y; the backward apply reads g and y and writes g_y.  Then a RetinaNet-R50 training step (forward + backward + SGD, batch 16,
800 x 1344, FREEZE_AT = 0) with the norm on and off.
`python scripts/micro_backbone_norm.py [--iters K] [--no-step]`; one line per (shape, kernel) and a JSON summary line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from basedet_amd import ops  # noqa: E402

SHAPES = (("layer1", 200, 336, 256), ("layer2", 100, 168, 512), ("layer4", 25, 42, 2048))


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


def _step_ms(norm, iters):
    import numpy as np
    from basedet_amd.configs import RetinaNetConfig
    from basedet_amd.models import RetinaNet
    from basedet_amd.solver import DetSolver
    from basedet_amd.utils import DummyLoader
    cfg = RetinaNetConfig()
    cfg.merge(dict(MODEL=dict(BATCHSIZE=16, BACKBONE=dict(FREEZE_AT=0, NORM=norm))))
    model = RetinaNet(cfg, seed=0)
    solver = DetSolver.build(cfg, model)
    batch = next(DummyLoader(16, (800, 1344), seed=0))
    batch["data"] = torch.from_numpy((batch["data"] * 255).astype(np.float32)).cuda()
    ms = _timed(lambda: solver.minimize(model, batch), iters)
    return ms, model.plan_bytes(model.reserve(16, 800, 1344))


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 20
    N = 16
    out = {}
    for name, H, W, C in SHAPES:
        f = lambda: torch.ones(C, dtype=torch.float32, device="cuda")
        geo = ops.single(N, H, W)
        M = geo.pixels
        y = (torch.randn(M, C, device="cuda") * 2 + 1).to(torch.bfloat16)
        g, r = torch.randn(M, C, device="cuda").to(torch.bfloat16), torch.randn(M, C, device="cuda").to(torch.bfloat16)
        z, gy = torch.empty_like(y), torch.empty_like(y)
        mean, inv_std, gamma, beta, dg, db, rm, rv = (f() for _ in range(8))
        sums = torch.empty((3, C), dtype=torch.float32, device="cuda")
        ws = torch.empty(ops.bn_workspace_bytes(M, C) // 4 + 64, dtype=torch.float32, device="cuda")
        t = M * C * 2          # bytes of one bf16 tensor
        runs = {
            "stats_fwd": (lambda: ops.bn_stats_fwd(y, geo, C, 1e-5, 0.1, mean, inv_std, sums, rm, rv, ws), t),
            "apply_act": (lambda: ops.bn_apply_act_fwd(y, geo, mean, inv_std, gamma, beta, z, geo, C), 2 * t),
            "apply_act+res": (lambda: ops.bn_apply_act_fwd(y, geo, mean, inv_std, gamma, beta, z, geo, C, residual=r, gr=geo), 3 * t),
            "bwd_reduce": (lambda: ops.bn_bwd_reduce(g, geo, y, geo, mean, inv_std, C, dg, db, ws), 2 * t),
            "bwd_apply": (lambda: ops.bn_bwd_apply(g, geo, y, geo, mean, inv_std, gamma, dg, db, sums[0], gy, geo, C), 3 * t),
        }
        for kname, (fn, nbytes) in runs.items():
            ms = _timed(fn, iters)
            out[f"{name} {kname}"] = (round(ms * 1e3, 1), round(nbytes / ms / 1e9, 2))
            print(f"{name} {H:3d}x{W:<3d}x{C:<4d} {kname:13s} {ms * 1e3:8.1f} us  {nbytes / 1e6:7.1f} MB  {nbytes / ms / 1e9:5.2f} TB/s", flush=True)
        del y, g, r, z, gy
    res = {"micro_backbone_norm_us_tbps": out}
    if "--no-step" not in sys.argv:
        for norm in ("BN", "FrozenBN"):
            ms, plan = _step_ms(norm, max(3, iters // 4))
            res[f"retinanet_r50_b16_step_ms_{norm}"] = round(ms, 1)
            res[f"retinanet_r50_b16_plan_bytes_{norm}"] = plan
            print(f"RetinaNet-R50 batch 16 800x1344 FREEZE_AT=0 NORM={norm}: {ms:.1f} ms / step, plan {plan / 2 ** 30:.2f} GiB", flush=True)
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
