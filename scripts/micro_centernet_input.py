"""CenterNet's training input on the device, timed: 16 raw 480 x 640 uint8 images through the pipeline of CenterNetConfig.AUG.TRAIN_VALUE
into 512 x 512 (data/raw.py CenterNetRawCollator -> FPNDetector.pre_process -> bd_affine_jitter_normalize).

  entry_all_stages   bd_affine_jitter_normalize with every stage on: the counter memset and the two launches (warp + flip + brightness
                     into the workspace; contrast + saturation + lighting + normalise)
  entry_no_contrast  the same descriptors with the contrast bit cleared: the single fused launch (no workspace traffic); the difference
                     to the row above is what the reduction costs
  pre_process        host collate (parameter draws, boxes, packing), the copy of the packed bytes and the launches, end to end

    python scripts/micro_centernet_input.py [--repeats 30] [--iters 10]

Prints one line per repeat and a final JSON line; p50 / p95 over the repeats.  A measurement, not a test: nothing is asserted about time."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from basedet_amd import _lib, ops  # noqa: E402
from basedet_amd.data import CenterNetRawCollator  # noqa: E402

N, SRC, OUT = 16, (480, 640), 512


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _pcts(v):
    return {"p50": round(float(np.percentile(v, 50)), 3), "p95": round(float(np.percentile(v, 95)), 3)}


def samples(seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N):
        h, w = SRC
        n = int(rng.integers(1, 8))
        x = np.sort(rng.uniform(0, w, (n, 2)), axis=1)
        y = np.sort(rng.uniform(0, h, (n, 2)), axis=1)
        boxes = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32)
        out.append((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), boxes, rng.integers(1, 81, (n,)).astype(np.float32), (h, w)))
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("micro_centernet_input.py needs a HIP device")
    from basedet_amd.configs import CenterNetConfig
    from basedet_amd.models import CenterNet
    repeats, iters = _arg("--repeats", 30), _arg("--iters", 10)
    cfg = CenterNetConfig()
    cfg.merge(dict(MODEL=dict(BATCHSIZE=N, WEIGHTS=None)))
    model = CenterNet(cfg)
    smp = samples()
    collate = CenterNetRawCollator(cfg.AUG.TRAIN_VALUE, np.random.default_rng(1))

    res = {"host_ms": [], "device_ms": [], "end_to_end_ms": []}
    for rnd in range(repeats + 3):                   # three warm-up rounds
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch = collate(smp)
        t1 = time.perf_counter()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        pl = model.pre_process(batch)["plan"]
        e.record()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rnd >= 3:
            res["host_ms"].append((t1 - t0) * 1e3); res["device_ms"].append(s.elapsed_time(e)); res["end_to_end_ms"].append((t2 - t0) * 1e3)
            print(f"repeat {rnd - 3}: host {res['host_ms'][-1]:8.2f} dev {res['device_ms'][-1]:7.3f} e2e {res['end_to_end_ms'][-1]:8.2f} ms",
                  flush=True)
    out = {"images": N, "source": list(SRC), "output": [OUT, OUT], "repeats": repeats, "pre_process": {m: _pcts(v) for m, v in res.items()},
           "h2d_bytes": int(batch["data"].packed.numel())}

    # ---- the entry alone, with and without the reduction, alternating -------------------------------------------------------------------
    descs = batch["data"].descs
    fused = []
    for d in descs:
        c = _lib.AffineDesc.from_buffer_copy(d)
        c.stages &= ~_lib.AFFINE_CONTRAST
        fused.append(c)
    packed = batch["data"].packed.cuda()
    halo = torch.empty_like(pl.x_halo)
    ws = torch.empty(ops.affine_jitter_workspace_bytes(N, OUT, OUT), dtype=torch.uint8, device="cuda")
    kern = {"entry_all_stages": lambda: ops.affine_jitter_normalize(packed, descs, OUT, OUT, model.img_mean, model.img_std, halo, ws),
            "entry_no_contrast": lambda: ops.affine_jitter_normalize(packed, fused, OUT, OUT, model.img_mean, model.img_std, halo, ws)}

    def timed(fn):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / iters * 1e3
    for fn in kern.values():
        timed(fn)
    kt = {k: [] for k in kern}
    for _ in range(repeats):
        for k, fn in kern.items():
            kt[k].append(timed(fn))
    px = N * OUT * OUT
    moved = {"entry_all_stages": halo.numel() * 2 + 8 * px, "entry_no_contrast": halo.numel() * 2}      # + the source taps (cache-resident)
    out["kernels"] = {"launches_per_sample": iters}
    for k, v in kt.items():
        p = _pcts(v)
        out["kernels"][k] = {"us": p, "bytes_written_and_reread": moved[k], "GBps_at_p50": round(moved[k] / p["p50"] / 1e3, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
