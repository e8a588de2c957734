"""What the three NMS entry points cost, timed with HIP events on the library that BASEDET_HIP_LIB names (default: the in-tree build):
  rpn_proposals   bd_rpn_proposals at the configured Faster R-CNN shape: N = 16, the five-level 800 x 1344 pyramid, A = 3, pre_k 2000,
                  post_k 1000, threshold 0.7, random bf16 head output (top-k + decode + the per-level NMS + merge + gather)
  nms_batched     bd_nms_batched at B = 16, C = 5000, 80 labels
  batched_nms     bd_batched_nms at n = 3000, 80 labels
`python scripts/micro_nms.py [--iters K]` times the loaded library once and prints one JSON line (ms per call).
`python scripts/micro_nms.py --ab OTHER_LIB [--rounds R]` compares OTHER_LIB (a build of the parent commit: BD_LIB_NAME at build time)
with the in-tree library: R alternations, one fresh process per library and run.  A case passes if the in-tree median is no slower than
OTHER_LIB's median plus OTHER_LIB's own max - min spread."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = ("rpn_proposals", "nms_batched", "batched_nms")


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _timed(fn, iters):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def _boxes(rng, shape, W=1344, H=800):
    import numpy as np
    cx, cy = rng.uniform(0, W, shape), rng.uniform(0, H, shape)
    w, h = rng.uniform(8, 200, shape), rng.uniform(8, 200, shape)
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(np.float32)


def measure(iters):
    import numpy as np
    import torch
    from basedet_amd import ops
    from oracle import box_ops as ob
    if not torch.cuda.is_available():
        raise SystemExit("micro_nms.py needs a HIP device")
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    legs = {}

    N, A, ldc, pre_k, post_k = 16, 3, 16, 2000, 1000
    strides = [4, 8, 16, 32, 64]
    sizes = [((800 + s - 1) // s, (1344 + s - 1) // s) for s in strides]
    ppi = sum(h * w for h, w in sizes)
    raw = np.zeros((N, ppi, ldc), np.float32)
    raw[:, :, :A] = rng.normal(0, 2, (N, ppi, A))
    raw[:, :, A:5 * A] = rng.normal(0, 0.5, (N, ppi, 4 * A))
    raw = torch.from_numpy(raw).to(torch.bfloat16).cuda().reshape(N * ppi, ldc).contiguous()
    anchors = dev(np.concatenate(ob.default_anchors(sizes, strides, [[x] for x in [32, 64, 128, 256, 512]], [[0.5, 1, 2]], 0.5), 0))
    im_info = dev(np.array([[800, 1344, 800, 1344, 1]] * N, np.float32))
    geom = ops.Geom(N, [s[0] for s in sizes], [s[1] for s in sizes])
    rois = torch.empty((N, post_k, 4), dtype=torch.float32, device="cuda")
    num = torch.empty((N,), dtype=torch.int32, device="cuda")
    ws = torch.empty((ops.rpn_proposals_workspace_bytes(N, [h * w for h, w in sizes], A, pre_k, post_k),), dtype=torch.uint8, device="cuda")
    legs["rpn_proposals"] = lambda: ops.rpn_proposals(raw, ldc, A, 0, A, geom, anchors, im_info, [0, 0, 0, 0], [1, 1, 1, 1], pre_k, 0.7, post_k,
                                                      rois, num, ws)

    B, C = 16, 5000
    bb, bs, bi = dev(_boxes(rng, (B, C))), dev(rng.uniform(0, 1, (B, C)).astype(np.float32)), dev(rng.integers(0, 80, (B, C)).astype(np.int32))
    keep = torch.empty((B, C), dtype=torch.int32, device="cuda")
    nk = torch.empty((B,), dtype=torch.int32, device="cuda")
    bws = torch.empty((ops.nms_batched_workspace_bytes(B, C),), dtype=torch.uint8, device="cuda")
    legs["nms_batched"] = lambda: ops.nms_batched(bb, bs, bi, 0.5, 0, keep, nk, bws)

    n = 3000
    sb, ss, si = dev(_boxes(rng, (n,))), dev(rng.uniform(0, 1, n).astype(np.float32)), dev(rng.integers(0, 80, n).astype(np.int32))
    L = ops.L()
    skeep = torch.empty((n,), dtype=torch.int32, device="cuda")
    snum = torch.zeros((1,), dtype=torch.int32, device="cuda")
    sws = torch.empty((ops.nms_workspace_bytes(n),), dtype=torch.uint8, device="cuda")
    legs["batched_nms"] = lambda: ops.check(L.bd_batched_nms(ops.ptr(sb), ops.ptr(ss), ops.ptr(si), n, 0.5, 0, ops.ptr(skeep), ops.ptr(snum),
                                                             ops.ptr(sws), sws.numel(), ops.stream_ptr()), "bd_batched_nms")
    out = {}
    for k, fn in legs.items():
        _timed(fn, 5)
        out[k] = round(_timed(fn, iters), 4)
    out["kept"] = {"rpn_proposals": int(num.sum()), "nms_batched": int(nk.sum()), "batched_nms": int(snum.item())}
    return out


def ab(other, rounds, iters):
    libs = {"parent": os.path.abspath(other), "change": None}
    res = {k: {c: [] for c in CASES} for k in libs}
    kept = {}
    for rnd in range(rounds):
        for name, lib in libs.items():
            env = dict(os.environ)
            env.pop("BASEDET_HIP_LIB", None)
            if lib:
                env["BASEDET_HIP_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--iters", str(iters)], env=env, capture_output=True, text=True,
                               timeout=300)
            if p.returncode != 0:
                raise SystemExit(f"{name} run failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
            r = json.loads(p.stdout.strip().splitlines()[-1])
            kept.setdefault(name, r["kept"])
            assert kept[name] == r["kept"]
            for c in CASES:
                res[name][c].append(r[c])
            print(f"round {rnd} {name:6s} " + "  ".join(f"{c} {r[c]:.4f} ms" for c in CASES), flush=True)
    assert kept["parent"] == kept["change"], f"the two libraries keep different numbers of boxes: {kept}"
    out = {"kept": kept["change"]}
    for c in CASES:
        p, q = res["parent"][c], res["change"][c]
        pm, qm, spread = statistics.median(p), statistics.median(q), max(p) - min(p)
        out[c] = {"parent_ms": p, "change_ms": q, "parent_median": pm, "change_median": qm, "parent_spread": round(spread, 4),
                  "change_over_parent": round(qm / pm, 3), "pass": qm <= pm + spread}
    print(json.dumps(out))
    return all(out[c]["pass"] for c in CASES)


def main():
    iters = _arg("--iters", 50)
    if "--ab" in sys.argv:
        raise SystemExit(0 if ab(_arg("--ab", None, str), _arg("--rounds", 3), iters) else 1)
    print(json.dumps(measure(iters)))


if __name__ == "__main__":
    main()
