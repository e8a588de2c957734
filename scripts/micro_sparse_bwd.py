"""Same-process A/B of the gradient skip (bd_conv_desc.gskip) on the box tower's head descriptor (16 x the five 800 x 1344 levels,
256 -> 256): data gradient (conv3x3_pp.hip, scan + compaction + tiles) and weight + bias gradient (conv_wgrad3x3_ring.hip, scan + walk +
reduce), dense against hinted, with g live in random 3 x 3 blobs covering ~1 %, 4 %, 25 % and 100 % of the pixels.  HIP events per call
(all launches of the call), interleaved rounds, median; the results are checked bit for bit.  "chain" = the same hinted calls inside a chain
(bd_conv_desc.gskip_gmap / gskip_dxmap / gskip_dx_clean): g's liveness map was left by its producer (here: one bd_gskip_map_scan outside the
timed region), so nothing is scanned or compacted; the data gradient leaves dx's map and, at a fixed shape, clears only what died.
usage: python scripts/micro_sparse_bwd.py [rounds=5]"""
import os
import sys
_here = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_here))
import numpy as np
import torch
from basedet_amd import ops

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N = 16
PYR = ([100, 50, 25, 13, 7], [168, 84, 42, 21, 11])


def live_mask(geo, frac, rng):
    if frac >= 1.0:
        return torch.ones(geo.pixels, dtype=torch.bool)
    m = np.zeros((N, geo.pix_per_img), bool)
    for n in range(N):
        for H, W, o in zip(geo.H, geo.W, geo.off):
            v = m[n, o:o + H * W].reshape(H, W)
            k = max(1, int(H * W * frac / 9))
            for y, x in zip(rng.integers(0, H, k), rng.integers(0, W, k)):
                v[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = True
    return torch.from_numpy(m.reshape(-1))


def timed(fn, reps=3):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def main():
    rng = np.random.default_rng(0)
    geo = ops.Geom(N, list(PYR[0]), list(PYR[1]))
    d = ops.conv_desc(geo, geo, 256, 256, 3, 3, 1, 1)
    scratch = torch.empty(ops.conv2d_dgrad_gskip_bytes(d) // 4 + 1, dtype=torch.int32, device="cuda")
    hd = ops.gskip_desc(d, scratch)
    x = torch.randn(geo.pixels, 256, device="cuda").to(torch.bfloat16)
    w = (torch.randn(256, 9, 256, device="cuda") * 0.05).to(torch.bfloat16)
    act = torch.randn(geo.pixels, 256, device="cuda").to(torch.bfloat16)
    gmap = torch.empty(ops.conv2d_gskip_map_bytes(d) // 4 + 1, dtype=torch.int32, device="cuda")
    dxmap = torch.empty(ops.conv2d_gskip_map_bytes(d, True) // 4 + 1, dtype=torch.int32, device="cuda")
    cd0 = ops.gskip_desc(d, gmap=gmap, dxmap=dxmap)                  # first call on a buffer: no promise
    cd = ops.gskip_desc(d, gmap=gmap, dxmap=dxmap, dx_clean=True)
    descs = (d, hd, cd)
    ws = [torch.empty(ops.conv2d_wgrad_bias_workspace_bytes(k) // 4 + 64, device="cuda") for k in descs]
    print(f"head descriptor: {N} x {list(zip(*PYR))}, 256 -> 256; us per call (median of {rounds} rounds)")
    print(f"  {'live px':>8s} {'dgrad dense':>12s} {'dgrad gskip':>12s} {'dgrad chain':>12s} {'wgrad dense':>12s} {'wgrad gskip':>12s} "
          f"{'wgrad chain':>12s}  same bits")
    for frac in (0.01, 0.04, 0.25, 1.0):
        live = live_mask(geo, frac, rng).cuda()
        g = torch.randn(geo.pixels, 256, device="cuda").to(torch.bfloat16)
        g = torch.where(live[:, None], g, torch.zeros((), dtype=torch.bfloat16, device="cuda")).contiguous()
        outs = [(torch.empty_like(act), torch.empty(256, 3, 3, 256, device="cuda"), torch.empty(256, device="cuda")) for _ in descs]
        t = [([], []) for _ in descs]
        ops.gskip_map_scan(d, g, gmap)
        ops.conv2d_dgrad(cd0, g, w, outs[2][0], mask=act, flags=ops.EPI_MASK)
        for _ in range(rounds):
            for i, k in enumerate(descs):
                dx, dw, db = outs[i]
                t[i][0].append(timed(lambda: ops.conv2d_dgrad(k, g, w, dx, mask=act, flags=ops.EPI_MASK)))
                t[i][1].append(timed(lambda: ops.conv2d_wgrad_bias(k, x, g, dw, db, ws[i])))
        same = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16),
                               b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16))
                   for o in outs[1:] for a, b in zip(outs[0], o))
        med = lambda v: float(np.median(v))
        print(f"  {float(live.float().mean()) * 100:7.2f}% {med(t[0][0]):12.1f} {med(t[1][0]):12.1f} {med(t[2][0]):12.1f} {med(t[0][1]):12.1f} "
              f"{med(t[1][1]):12.1f} {med(t[2][1]):12.1f}  {same}")


if __name__ == "__main__":
    main()
