"""Two ways of feeding the same 16 raw images to FPNDetector.pre_process, timed on one device in one run.

  (A) the existing way: numpy Compose per sample (data/transforms.py: bilinear resize, flip, CHW), DetectionPadCollator (fp32
      (N, 3, Hmax, Wmax)), then pre_process on that host batch (bd_h2d_submit + bd_pad_normalize);
  (B) the raw way: RawBatchCollator (parameters and boxes on the host, the uint8 bytes packed into one pinned buffer), then pre_process on
      the RawImageBatch (one copy + bd_resize_pad_normalize).

Input: 16 seeded synthetic uint8 images of 480 x 640, ShortestEdgeResize to short edge 800 (-> 800 x 1067, padded 800 x 1088),
RandomHorizontalFlip(0.5), both ways drawing the same RNG stream.  After a warm-up of both ways (which also checks that they leave the
same bits in the plan's x_halo), `--repeats` (default 30) alternations; each timed region starts and ends with a device synchronise.
Per way: host time (samples -> batch dict), device time of pre_process (events around its copies and launch), end to end, and the
bytes that cross the link.  Then the two kernels alone at that output shape, alternating, `--iters` launches per sample: both write the
same 8 bytes per output pixel.  p50 and p95 of everything; one JSON line at the end with the two verdicts:
  e2e_B_faster      B's end-to-end p50 is below A's by more than A's own p95 - p50
  kernel_not_slower bd_resize_pad_normalize's p50 does not exceed bd_pad_normalize's by more than bd_pad_normalize's p95 - p50
`python scripts/micro_input_pipeline.py [--repeats R] [--iters K]`"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from basedet_amd import ops  # noqa: E402
from basedet_amd.data import DetectionPadCollator, RawBatchCollator, build_transform  # noqa: E402

N, SRC = 16, (480, 640)
SPEC = (("ShortestEdgeResize", dict(min_size=(800,), max_size=1333, sample_style="choice")),
        ("RandomHorizontalFlip", dict(prob=0.5)), ("ToMode", dict(mode="CHW")))


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
        out.append((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), boxes, rng.integers(0, 80, (n,)).astype(np.float32), (h, w)))
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("micro_input_pipeline.py needs a HIP device")
    from basedet_amd.configs import RetinaNetConfig
    from basedet_amd.models import RetinaNet
    repeats, iters = max(_arg("--repeats", 30), 30), _arg("--iters", 10)
    cfg = RetinaNetConfig()
    cfg.MODEL.BATCHSIZE = N
    model = RetinaNet(cfg)
    smp = samples()
    compose = build_transform(SPEC, "train", rng=np.random.default_rng(1))
    pad = DetectionPadCollator()
    raw = RawBatchCollator(build_transform(SPEC, "train", rng=np.random.default_rng(1)))

    def host_a():
        done = []
        for img, boxes, cat, info in smp:
            im, bx, ct = compose((img, boxes, cat))
            done.append((im, bx, ct, info))
        return pad(done)

    def one(host):
        """(host ms, device ms of pre_process, end-to-end ms, the batch, the plan)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch = host()
        t1 = time.perf_counter()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        pl = model.pre_process(batch)["plan"]
        e.record()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, s.elapsed_time(e), (t2 - t0) * 1e3, batch, pl

    ways = {"A_numpy_pad_collate": host_a, "B_raw_collate": lambda: raw(smp)}
    for _ in range(3):                               # warm-up; both ways draw the same stream, so they must leave the same bits
        *_, batch_a, pl = one(ways["A_numpy_pad_collate"])
        x_a = pl.x_halo.clone()
        *_, batch_b, pl = one(ways["B_raw_collate"])
        assert torch.equal(pl.x_halo.view(torch.int16), x_a.view(torch.int16)), "the two ways disagree on x_halo"
    del x_a
    res = {k: {"host_ms": [], "device_ms": [], "end_to_end_ms": []} for k in ways}
    for rnd in range(repeats):
        for k, host in ways.items():
            h, d, t, _, _ = one(host)
            res[k]["host_ms"].append(h); res[k]["device_ms"].append(d); res[k]["end_to_end_ms"].append(t)
        print(f"repeat {rnd}: " + "  ".join(f"{k} host {res[k]['host_ms'][-1]:8.2f} dev {res[k]['device_ms'][-1]:7.3f} "
                                            f"e2e {res[k]['end_to_end_ms'][-1]:8.2f} ms" for k in ways), flush=True)
    out = {"images": N, "source": list(SRC), "resized": list(batch_a["data"].shape[2:]), "repeats": repeats}
    for k in ways:
        out[k] = {m: _pcts(v) for m, v in res[k].items()}
    out["A_numpy_pad_collate"]["h2d_bytes"] = int(batch_a["data"].nbytes)
    out["B_raw_collate"]["h2d_bytes"] = int(batch_b["data"].packed.numel())

    # ---- the two kernels alone, same output shape, alternating --------------------------------------------------------------------
    rb = batch_b["data"]
    Hp, Wp = pl.Hp, pl.Wp
    x_f32 = torch.from_numpy(batch_a["data"]).cuda()
    packed = rb.packed.cuda()
    halo = torch.empty_like(pl.x_halo)
    kern = {"bd_pad_normalize": lambda: ops.pad_normalize(x_f32, Hp, Wp, model.img_mean, model.img_std, halo),
            "bd_resize_pad_normalize": lambda: ops.resize_pad_normalize(packed, rb.descs, Hp, Wp, model.img_mean, model.img_std, halo)}

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
    written = halo.numel() * 2
    read = {"bd_pad_normalize": x_f32.numel() * 4, "bd_resize_pad_normalize": packed.numel()}
    out["kernels"] = {"padded": [Hp, Wp], "launches_per_sample": iters}
    for k, v in kt.items():
        p = _pcts(v)
        out["kernels"][k] = {"us": p, "bytes_written": written, "bytes_read_once": read[k],
                             "GBps_at_p50": round((written + read[k]) / p["p50"] / 1e3, 1)}
    a, b = out["A_numpy_pad_collate"]["end_to_end_ms"], out["B_raw_collate"]["end_to_end_ms"]
    out["e2e_B_faster"] = bool(a["p50"] - b["p50"] > a["p95"] - a["p50"])
    ko, kn = out["kernels"]["bd_pad_normalize"]["us"], out["kernels"]["bd_resize_pad_normalize"]["us"]
    out["kernel_not_slower"] = bool(kn["p50"] <= ko["p50"] + (ko["p95"] - ko["p50"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
