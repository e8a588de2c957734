"""Same-process A/B of the forward skip (bd_conv_desc.fwd_map) on the box tower's head descriptor (16 x the five 800 x 1344 levels,
256 -> 256, bias + ReLU): the dense launch against the sparse forward instance of conv3x3_pp.hip with ~1 %, 4 %, 22 % and 100 % of the
4 x 16 patches on the list (random foreground pixels, the depth-1 map), without and with the promise (fwd_clean), and the map launch
itself (bd_fwd_live_maps, four depths).  HIP events per call, interleaved rounds, median; the live patches are checked bit for bit and the
dead ones for +0.  The 100 % row is the penalty of following a full list instead of launching densely (no tail split, list reads).
usage: python scripts/micro_sparse_fwd.py [rounds=5]"""
import os
import sys
_here = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_here))
import numpy as np
import torch
from basedet_amd import ops

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N, A = 16, 9
PYR = ([100, 50, 25, 13, 7], [168, 84, 42, 21, 11])


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
    x = torch.randn(geo.pixels, 256, device="cuda").to(torch.bfloat16)
    w = (torch.randn(256, 9, 256, device="cuda") * 0.05).to(torch.bfloat16)
    b = torch.randn(256, device="cuda")
    ints = ops.fwd_live_map_bytes(d) // 4
    p4 = (ints - 8) // 3
    maps = [torch.zeros(ints, dtype=torch.int32, device="cuda") for _ in range(4)]
    dense = torch.empty(geo.pixels, 256, dtype=torch.bfloat16, device="cuda")
    y = torch.empty_like(dense)
    print(f"head descriptor: {N} x {list(zip(*PYR))}, 256 -> 256, {p4} patches; us per call (median of {rounds} rounds)")
    print(f"  {'live':>8s} {'dense':>10s} {'sparse':>10s} {'sparse+promise':>15s} {'map launch':>11s}  same bits")
    for frac in (0.01, 0.04, 0.22, 1.0):
        lab = np.zeros((N, geo.pix_per_img, A), np.int32)
        if frac >= 1.0:
            lab[:, :, 0] = 1
        else:
            k = max(1, int(N * geo.pix_per_img * frac / 40))          # (a pixel's depth-1 neighbourhood touches one or two 64-pixel patches)
            lab.reshape(-1, A)[rng.integers(0, N * geo.pix_per_img, k), 4] = 1
        lab = torch.from_numpy(lab.reshape(N, -1)).cuda()
        ops.fwd_live_maps(d, lab, A, maps, reset=True)
        d0, d1 = ops.fwd_map_desc(d, maps[0]), ops.fwd_map_desc(d, maps[0], clean=True)
        ops.conv2d_fwd(d0, x, w, b, y, flags=ops.EPI_RELU)
        ops.fwd_live_maps(d, lab, A, maps, reset=False)                # (the previous list = this one: the promise holds for every call below)
        t = [[], [], [], []]
        for _ in range(rounds):
            t[0].append(timed(lambda: ops.conv2d_fwd(d, x, w, b, dense, flags=ops.EPI_RELU)))
            t[1].append(timed(lambda: ops.conv2d_fwd(d0, x, w, b, y, flags=ops.EPI_RELU)))
            t[2].append(timed(lambda: ops.conv2d_fwd(d1, x, w, b, y, flags=ops.EPI_RELU)))
        for _ in range(rounds):
            t[3].append(timed(lambda: ops.fwd_live_maps(d, lab, A, maps, reset=False), reps=2))       # (an even number of flips: maps[0] as above)
        live = maps[0][8:8 + p4].cpu().numpy() != 0
        m = np.zeros((N, geo.pix_per_img), bool)
        q = 0
        for n in range(N):
            for H, W, o in zip(geo.H, geo.W, geo.off):
                v = m[n, o:o + H * W].reshape(H, W)
                for by in range(-(-H // 4)):
                    for bx in range(-(-W // 16)):
                        if live[q]:
                            v[4 * by:4 * by + 4, 16 * bx:16 * bx + 16] = True
                        q += 1
        m = torch.from_numpy(m.reshape(-1)).cuda()
        same = torch.equal(y.view(torch.int16)[m], dense.view(torch.int16)[m]) and int((y.view(torch.int16)[~m] != 0).sum()) == 0
        med = lambda v: float(np.median(v))
        print(f"  {live.mean() * 100:7.2f}% {med(t[0]):10.1f} {med(t[1]):10.1f} {med(t[2]):15.1f} {med(t[3]):11.1f}  {same}")


if __name__ == "__main__":
    main()
