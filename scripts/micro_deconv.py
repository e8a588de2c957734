"""Per-launch A/B of the FPN deconv kernels (csrc/fpn_deconv.hip) against the generic convolution kernels running the same math on the
conv view (Conv2d(k4, s2, p1), Cin = fine, Cout = coarse): forward = bd_conv2d_dgrad, data gradient = bd_conv2d_fwd, weight gradient =
bd_conv2d_wgrad.  Batch 16 at the 800 x 1344 FPN shapes; the two variants alternate on one device, three rounds.
`python scripts/micro_deconv.py [--iters K]`; one line per (round, shape, pass, variant) and a JSON summary line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from basedet_amd import ops  # noqa: E402

PEAK_TFLOPS = 2500.0          # MI355X dense bf16 MFMA peak (TFLOP/s)


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
    bf = dict(dtype=torch.bfloat16, device="cuda")
    res = {}
    for rnd in range(3):
        for (H, W) in ((25, 42), (50, 84)):
            gc, gf = ops.single(N, H, W), ops.single(N, 2 * H, 2 * W)
            d = ops.conv_desc(gf, gc, C, C, 4, 4, 2, 1)
            x = torch.randn(gc.pixels, C, device="cuda").to(torch.bfloat16)
            dy = torch.randn(gf.pixels, C, device="cuda").to(torch.bfloat16)
            y, dx = torch.empty((gf.pixels, C), **bf), torch.empty((gc.pixels, C), **bf)
            master = torch.randn(C, 4, 4, C, device="cuda") * 0.02
            wf, wd = torch.empty((4, C, 4, C), **bf), torch.empty((C, 16, C), **bf)
            ops.fpn_deconv_pack(master, C, wf, wd)
            gw_f, gw_d = torch.empty((C, 16, C), **bf), torch.empty((C, 16, C), **bf)
            ops.weight_pack(master, None, gw_f, gw_d, C, 16, C)
            ws = torch.empty((max(ops.conv2d_wgrad_workspace_bytes(d), ops.fpn_deconv_wgrad_workspace_bytes(N, H, W, C)) // 4 + 64,),
                             device="cuda")
            dw = torch.zeros((C, 4, 4, C), device="cuda")
            flops = 2.0 * gf.pixels * C * 4 * C           # useful work of every pass (each fine pixel reads 2 x 2 taps)
            runs = {
                "fwd": (lambda: ops.fpn_deconv_fwd(x, wf, y, N, H, W, C, add=y),
                        lambda: ops.conv2d_dgrad(d, x, gw_d, y, add=y, flags=ops.EPI_ADD_BEFORE)),
                "dgrad": (lambda: ops.fpn_deconv_dgrad(dy, wd, dx, N, H, W, C, add=dx),
                          lambda: ops.conv2d_fwd(d, dy, gw_f, None, dx, add=dx, flags=ops.EPI_ADD_BEFORE)),
                "wgrad": (lambda: ops.fpn_deconv_wgrad(x, dy, dw, ws, N, H, W, C),
                          lambda: ops.conv2d_wgrad(d, dy, x, dw, ws)),
            }
            for name, (ded, gen) in runs.items():
                for var, fn in (("dedicated", ded), ("generic", gen)):
                    ms = _timed(fn, iters)
                    tf = flops / ms / 1e9
                    res.setdefault(f"{H}x{W}->{2 * H}x{2 * W} {name} {var}", []).append(ms * 1e3)
                    print(f"round {rnd} {H}x{W}->{2 * H}x{2 * W} {name:5s} {var:9s} {ms * 1e3:8.1f} us  {tf:7.1f} TF/s  "
                          f"{tf / PEAK_TFLOPS:.3f} of peak", flush=True)
    summary = {k: round(min(v), 1) for k, v in res.items()}
    print(json.dumps({"micro_deconv_us_best_of_3": summary}))


if __name__ == "__main__":
    main()
