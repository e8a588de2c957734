"""Per-launch times of the deformable convolution (csrc/deform_conv.hip) at CenterNet-R50's three DeconvLayers (batch 16, 512 x 512 input:
16x16 2048 -> 256, 32x32 256 -> 128, 64x64 128 -> 64), forward, data gradient and weight gradient, each next to the plain
bd_conv2d_fwd / _dgrad / _wgrad of the same shape: the same FLOPs with regular reads -- a floor, not a target.  Offsets N(0, 2 px), random
mask logits (DCNv2 form); the two variants alternate on one device, three rounds, the best round counts.
`python scripts/micro_deform_conv.py [--iters K]`; one line per (round, shape, pass, variant) and a JSON summary line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from basedet_amd import ops  # noqa: E402

LAYERS = ((16, 16, 2048, 256), (32, 32, 256, 128), (64, 64, 128, 64))


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
    N, ld = 16, 32
    bf = dict(dtype=torch.bfloat16, device="cuda")
    res = {}
    for rnd in range(3):
        for (H, W, Cin, Cout) in LAYERS:
            g = ops.single(N, H, W)
            M = g.pixels
            d = ops.conv_desc(g, g, Cin, Cout, 3, 3, 1, 1)
            x = torch.randn(M, Cin, device="cuda").to(torch.bfloat16)
            dy = torch.randn(M, Cout, device="cuda").to(torch.bfloat16)
            om = torch.randn(M, ld, device="cuda")
            om[:, :18] *= 2.0
            om = om.to(torch.bfloat16)
            master = torch.randn(Cout, 9, Cin, device="cuda") * (1.0 / (9 * Cin)) ** 0.5
            bias = torch.randn(Cout, device="cuda")
            wf, wd = torch.empty((Cout, 9, Cin), **bf), torch.empty((Cin, 9, Cout), **bf)
            ops.weight_pack(master, None, wf, wd, Cout, 9, Cin)
            y, dx, d_om = torch.empty((M, Cout), **bf), torch.empty((M, Cin), **bf), torch.empty((M, ld), **bf)
            nbytes = max(ops.conv2d_wgrad_workspace_bytes(d), ops.deform_conv_wgrad_workspace_bytes(N, H, W, Cin, Cout),
                         ops.deform_conv_bwd_data_workspace_bytes(N, H, W, Cin, Cout))
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            dw, db = torch.zeros((Cout, 3, 3, Cin), device="cuda"), torch.zeros(Cout, device="cuda")
            flops = 2.0 * M * Cout * 9 * Cin
            runs = {
                "fwd": (lambda: ops.deform_conv_fwd(x, om, wf, bias, y, N, H, W, Cin, Cout, True),
                        lambda: ops.conv2d_fwd(d, x, wf, bias, y)),
                "bwd_data": (lambda: ops.deform_conv_bwd_data(x, om, dy, wd, dx, d_om, ws, N, H, W, Cin, Cout, True),
                             lambda: ops.conv2d_dgrad(d, dy, wd, dx)),
                "wgrad": (lambda: ops.deform_conv_wgrad(x, om, dy, dw, db, ws, N, H, W, Cin, Cout, True),
                          lambda: ops.conv2d_wgrad(d, x, dy, dw, ws)),
            }
            for name, (dcn, plain) in runs.items():
                for var, fn in (("deform", dcn), ("plain", plain)):
                    ms = _timed(fn, iters)
                    res.setdefault(f"{H}x{W} {Cin}->{Cout} {name} {var}", []).append(ms * 1e3)
                    print(f"round {rnd} {H}x{W} {Cin:4d}->{Cout:3d} {name:8s} {var:6s} {ms * 1e3:9.1f} us  {flops / ms / 1e9:7.1f} TF/s", flush=True)
    summary = {k: round(min(v), 1) for k, v in res.items()}
    print(json.dumps({"micro_deform_conv_us_best_of_3": summary}))


if __name__ == "__main__":
    main()
