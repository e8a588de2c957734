"""CenterNet's neck and head at the recipe's shape: batch 16, res5 2048 x 16 x 16 -> 64 x 128 x 128, K = 80 (262 144 output pixels).

Protocol of scripts/micro_centernet.py: device events around back-to-back calls of one leg, `--rounds` alternations of `--iters` calls
after a warm-up of every leg, operands rotating over `--copies` independent sets so that a call does not find them in the last-level cache.
Two groups of legs, all in one process:
  fused_fwd / fused_bwd       bd_center_head_out_fwd / _bwd on feat [M][192]
  generic_fwd / generic_bwd   the same math on the generic kernels: three 1x1 launches per direction on separate tower buffers [M][64]
                              (wh / reg padded to 8 output rows), backward = three data gradients, a ReLU-gate pass over each tower's
                              gradient and three weight + bias gradients
  deconv{1,2,3}_{fwd,bwd}, head_{fwd,bwd}   forward_pm / backward_pm of each DeconvLayer and of CenterHead (feat_conv + fused kernel)
`python scripts/micro_center_head.py [--iters K] [--rounds R] [--copies C] [--peak-gbps G]`; one line per (round, leg), a JSON summary line."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from basedet_amd import ops  # noqa: E402
from basedet_amd.layers import CenterHead, CenternetDeconv  # noqa: E402

N, K, C, H0, W0 = 16, 80, 64, 16, 16
CHANNELS = [2048, 256, 128, 64]
H, W = 8 * H0, 8 * W0
M, LD = N * H * W, 80
BF = torch.bfloat16


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
        raise SystemExit("micro_center_head.py needs a HIP device")
    rounds, iters, copies, peak = _arg("--rounds", 5), _arg("--iters", 10), _arg("--copies", 3), _arg("--peak-gbps", 8000)
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    e = lambda *s, dt=BF: torch.empty(s, dtype=dt, device=dev)
    w = [rn(K, C) / 8, rn(2, C) / 8, rn(2, C) / 8]
    b = [rn(K), rn(2), rn(2)]
    geom = ops.single(N, H, W)
    descs = [ops.conv_desc(geom, geom, C, co, 1, 1, 1, 0) for co in (LD, 8, 8)]
    packed = []
    for wi, co in zip(w, (LD, 8, 8)):
        wp = torch.zeros(co, 1, 1, C, device=dev)
        wp[:wi.shape[0], 0, 0] = wi
        wf, wd = e(co, 1, C), e(C, 1, co)
        ops.weight_pack(wp, None, wf, wd, co, 1, C)
        bp = torch.zeros(co, device=dev)
        packed.append((wf, wd, bp))
    ws_f = e(ops.center_head_out_bwd_workspace_bytes(M, C, K), dt=torch.uint8)
    ws_g = e(max(ops.conv2d_wgrad_bias_workspace_bytes(d) for d in descs), dt=torch.uint8)
    sets = []
    for _ in range(copies):
        feat = torch.relu(rn(M, 3 * C)).to(BF)
        sets.append(dict(
            feat=feat, towers=[feat[:, i * C:(i + 1) * C].contiguous() for i in range(3)],
            d_logits=rn(M, LD).to(BF), d_wr=rn(M, 8).to(BF), logits=e(M, LD), wr=e(M, 8), d_feat=e(M, 3 * C),
            outs=[e(M, LD), e(M, 8), e(M, 8)], d_tw=[e(M, C) for _ in range(3)], d_gated=[e(M, C) for _ in range(3)],
            gw=[e(K, C, dt=torch.float32), e(K, dt=torch.float32), e(2, C, dt=torch.float32), e(2, dt=torch.float32),
                e(2, C, dt=torch.float32), e(2, dt=torch.float32)],
            gw_g=[(e(co, 1, 1, C, dt=torch.float32), e(co, dt=torch.float32)) for co in (LD, 8, 8)]))

    def fused_fwd(i):
        s = sets[i % copies]
        ops.center_head_out_fwd(s["feat"], w[0], b[0], w[1], b[1], w[2], b[2], M, C, K, s["logits"], s["wr"])

    def fused_bwd(i):
        s = sets[i % copies]
        ops.center_head_out_bwd(s["feat"], s["d_logits"], s["d_wr"], w[0], w[1], w[2], M, C, K, s["d_feat"], *s["gw"], ws_f)

    def generic_fwd(i):
        s = sets[i % copies]
        for d, (wf, _, bp), x, y in zip(descs, packed, s["towers"], s["outs"]):
            ops.conv2d_fwd(d, x, wf, bp, y)

    def generic_bwd(i):
        s = sets[i % copies]
        grads = (s["d_logits"], s["d_wr"], s["d_wr"])          # (the 8-wide gradient buffers stand in for the padded wh / reg gradients)
        for d, (_, wd, _), x, gr, dt, dg, (dw, db) in zip(descs, packed, s["towers"], grads, s["d_tw"], s["d_gated"], s["gw_g"]):
            ops.conv2d_dgrad(d, gr, wd, dt)
            ops.relu_bwd_bf16(dt, x, dg)
            ops.conv2d_wgrad_bias(d, x, gr, dw, db, ws_g)

    fwd_b = M * (3 * C + LD + 8) * 2
    bwd_b = M * (3 * C + LD + 8 + 3 * C) * 2
    legs = {"fused_fwd": (fused_fwd, fwd_b), "generic_fwd": (generic_fwd, fwd_b), "fused_bwd": (fused_bwd, bwd_b),
            "generic_bwd": (generic_bwd, bwd_b)}

    neck = CenternetDeconv(CHANNELS, [4, 4, 4], True)
    head = CenterHead(C, K)
    xs = [rn(N * H0 * W0, CHANNELS[0]).to(BF) for _ in range(copies)]
    h, wd_ = H0, W0
    x = xs[0]
    for name, layer in neck.layers():           # one forward / backward so that every stage has its saved input
        layer._micro_in = [x] + [torch.randn_like(x.float()).to(BF) for _ in range(copies - 1)]
        x = layer.forward_pm(x, N, h, wd_)
        layer._micro_g = [torch.randn_like(x.float()).to(BF) for _ in range(copies)]
        layer._micro_hw = (h, wd_)
        h, wd_ = 2 * h, 2 * wd_
    head_in = [x] + [torch.randn_like(x.float()).to(BF) for _ in range(copies - 1)]
    for name, layer in neck.layers():
        hh, ww = layer._micro_hw
        legs[name + "_fwd"] = ((lambda i, l=layer, hh=hh, ww=ww: l.forward_pm(l._micro_in[i % copies], N, hh, ww)), 0)
        legs[name + "_bwd"] = ((lambda i, l=layer: l.backward_pm(l._micro_g[i % copies])), 0)
    legs["head_fwd"] = ((lambda i: head.forward_pm(head_in[i % copies], N, H, W)), 0)
    legs["head_bwd"] = ((lambda i: head.backward_pm(sets[i % copies]["d_logits"], sets[i % copies]["d_wr"])), 0)

    for fn, _ in legs.values():
        _timed(fn, copies)
    res = {k: [] for k in legs}
    for rnd in range(rounds):
        for k, (fn, nbytes) in legs.items():
            ms = _timed(fn, iters)
            res[k].append(ms * 1e3)
            tail = f"  {nbytes / ms / 1e6:8.1f} GB/s of {nbytes / 1e6:.1f} MB" if nbytes else ""
            print(f"round {rnd} {k:12s} {ms * 1e3:9.1f} us{tail}", flush=True)
    out = {"shape": dict(N=N, K=K, C=C, H=H, W=W, channels=CHANNELS)}
    for k, t in res.items():
        nbytes = legs[k][1]
        med = statistics.median(t)
        out[k] = {"us_median": round(med, 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1)}
        if nbytes:
            out[k].update({"MB": round(nbytes / 1e6, 1), "GBps_at_median": round(nbytes / med / 1e3, 1), "floor_us": round(nbytes / peak / 1e3, 1)})
    print(json.dumps({"micro_center_head": out}))


if __name__ == "__main__":
    main()
