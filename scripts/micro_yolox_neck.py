"""The kernels of csrc/yolox_neck.hip and YOLOPAFPN as a whole at YOLOX-s's shapes: batch 16, 640 x 640 input, width 0.5, depth 0.33 -> dark3 /
dark4 / dark5 = 80 x 80 x 128 / 40 x 40 x 256 / 20 x 20 x 512.

Protocol of scripts/micro_yolox_head.py: device events around back-to-back calls of one leg, `--rounds` alternations of `--iters` calls
after a warm-up of every leg, operands rotating over `--copies` independent sets so that a call does not find them in the last-level cache.
Legs, all in one process (bytes = what the operation must read and write once):
  focus_fwd          bd_focus_fwd, 16 x 640 x 640 -> [16 320 320][16]
  spp_fwd / spp_bwd  bd_spp_fwd / bd_spp_bwd on [16 20 20][256] -> 1024 (SPPBottleneck(512, 512)'s hidden width)
  cat_p4 / cat_p3    bd_cat2_fwd(up=1): fpn_out0 [16 20 20][256] with dark4 -> [16 40 40][512]; fpn_out1 [16 40 40][128] with dark3 -> [16 80 80][256]
  cat_n3 / cat_n4    bd_cat2_fwd: [16 40 40][128 + 128]; [16 20 20][256 + 256]
  *_bwd of the four  bd_cat2_bwd with the accumulate flags the PAFPN backward uses (acc_a = 1 for the two upsampling ones)
  pafpn_fwd / _bwd   YOLOPAFPN(CSPDarknet(0.33, 0.5), 0.33, 0.5).forward_pm / backward_pm from the halo image down to the stem
`python scripts/micro_yolox_neck.py [--iters K] [--rounds R] [--copies C] [--peak-gbps G]`; one line per (round, leg), a JSON summary line."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from basedet_amd import ops  # noqa: E402
from basedet_amd.layers import CSPDarknet, YOLOPAFPN  # noqa: E402

N, H, W = 16, 640, 640
DEPTH, WIDTH = 0.33, 0.5
BF = torch.bfloat16
# name -> (up, h, w of the output, Ca, Cb)
CATS = {"cat_p4": (1, 40, 40, 256, 256), "cat_p3": (1, 80, 80, 128, 128), "cat_n3": (0, 40, 40, 128, 128), "cat_n4": (0, 20, 20, 256, 256)}


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
        raise SystemExit("micro_yolox_neck.py needs a HIP device")
    rounds, iters, copies, peak = _arg("--rounds", 5), _arg("--iters", 10), _arg("--copies", 3), _arg("--peak-gbps", 8000)
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev).to(BF)
    e = lambda *s: torch.empty(s, dtype=BF, device=dev)
    legs = {}

    halos = [torch.zeros((N, H + 6, W + 8, 4), dtype=BF, device=dev) for _ in range(copies)]
    for h in halos:
        h[:, 3:3 + H, 4:4 + W, :3] = rn(N, H, W, 3)
    s2d = e(N * (H // 2) * (W // 2), 16)
    legs["focus_fwd"] = (lambda i: ops.focus_fwd(halos[i % copies], N, H, W, s2d), 2 * (N * H * W * 4 + s2d.numel()))

    Ms, Cs = N * 20 * 20, 256
    u = [torch.randn(Ms, Cs, generator=g, device=dev) for _ in range(copies)]
    xs = [(t * torch.sigmoid(t)).to(BF) for t in u]          # SiLU outputs, as conv1 hands them over
    gs = [rn(Ms, 4 * Cs) for _ in range(copies)]
    cat, dxs = e(Ms, 4 * Cs), e(Ms, Cs)
    legs["spp_fwd"] = (lambda i: ops.spp_fwd(xs[i % copies], N, 20, 20, Cs, cat), 2 * 5 * Ms * Cs)
    legs["spp_bwd"] = (lambda i: ops.spp_bwd(gs[i % copies], xs[i % copies], N, 20, 20, Cs, dxs), 2 * 6 * Ms * Cs)

    for name, (up, h, w, Ca, Cb) in CATS.items():
        M = N * h * w
        Ma = M // 4 if up else M
        a, b, gr = [rn(Ma, Ca) for _ in range(copies)], [rn(M, Cb) for _ in range(copies)], [rn(M, Ca + Cb) for _ in range(copies)]
        out, da, db = e(M, Ca + Cb), torch.zeros((Ma, Ca), dtype=BF, device=dev), e(M, Cb)
        moved = 2 * (Ma * Ca + M * Cb)
        legs[name] = ((lambda i, a=a, b=b, M=M, Ca=Ca, Cb=Cb, out=out, up=up, h=h, w=w: ops.cat2_fwd(a[i % copies], b[i % copies], M, Ca, Cb, out,
                                                                                                  up, N, h, w)), moved + 2 * M * (Ca + Cb))
        legs[name + "_bwd"] = ((lambda i, gr=gr, M=M, Ca=Ca, Cb=Cb, da=da, db=db, up=up, h=h, w=w: ops.cat2_bwd(gr[i % copies], M, Ca, Cb, da, db, up,
                                                                                                               N, h, w, acc_a=up)),
                               moved + 2 * M * (Ca + Cb) + (2 * Ma * Ca if up else 0))

    fpn = YOLOPAFPN(CSPDarknet(DEPTH, WIDTH), DEPTH, WIDTH)
    outs, sizes = fpn.forward_pm(halos[0], N, H, W)
    d_outs = [[(0.01 * torch.randn(o.shape, generator=g, device=dev)).to(BF) for o in outs] for _ in range(copies)]
    legs["pafpn_fwd"] = (lambda i: fpn.forward_pm(halos[i % copies], N, H, W), 0)
    legs["pafpn_bwd"] = (lambda i: fpn.backward_pm(d_outs[i % copies]), 0)

    for fn, _ in legs.values():
        _timed(fn, copies)
    res = {k: [] for k in legs}
    for rnd in range(rounds):
        for k, (fn, nbytes) in legs.items():
            ms = _timed(fn, iters)
            res[k].append(ms * 1e3)
            tail = f"  {nbytes / ms / 1e6:8.1f} GB/s of {nbytes / 1e6:.1f} MB" if nbytes else ""
            print(f"round {rnd} {k:12s} {ms * 1e3:9.1f} us{tail}", flush=True)
    out = {"shape": dict(N=N, H=H, W=W, depth=DEPTH, width=WIDTH, sizes=sizes)}
    for k, t in res.items():
        nbytes = legs[k][1]
        med = statistics.median(t)
        out[k] = {"us_median": round(med, 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1)}
        if nbytes:
            out[k].update({"MB": round(nbytes / 1e6, 1), "GBps_at_median": round(nbytes / med / 1e3, 1), "floor_us": round(nbytes / peak / 1e3, 1)})
    print(json.dumps({"micro_yolox_neck": out}))


if __name__ == "__main__":
    main()
