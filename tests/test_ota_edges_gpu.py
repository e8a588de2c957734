"""OTA target assignment (bd_ota_assign, bd_ota_assign_sinkhorn; basedet_amd/csrc/ota.hip) past 1024 points, with 0 .. 100 gts and on
degenerate gts, against oracle.box_ops.ota_ground_truth on the same bf16-valued logits and predictions.

The problems (tests/util.py::ota_edge_problem) live on the pyramid of a 320 x 448 image: P = 2987 points, so every 1024-thread loop of
the kernels makes three passes, the last one ragged.  gt counts [100, 0, 37, 1] (Gmax = 100: the Sinkhorn row loops wrap their 16 waves
seven times) and [1, 1] (Gmax = 1); K = 80, and K = 13 through ld = 16 with +30 in the three padding slots of every logits row.  Images
with >= 8 gts hold a zero-area gt, a gt outside the image and a copy of gt 0 with another class; rows >= num_gt hold NaN / 1e30.
Two plants have exact ties that only the index rules decide, on both sides alike, so the labels there must match without any excuse:
  * the tie points: equal smallest cost against the zero-area gt (dyn_k = 1), spread over the 1024-point passes -- the carried rank
    (eq_base) of ota_gt_kernel decides; image 2 has none in the first pass;
  * the copy of gt 0: its class logit is a copy of gt 0's, the two cost rows are the same numbers, every point both select is a
    conflict with an exact tie at the minimum -- "lowest gt index" of ota_resolve_kernel decides.
Elsewhere a label may differ only at max(1, 0.5 % of the foreground) points (top-k; max(1, fg // 20) for Sinkhorn), each with an excuse
from the oracle's own matrices (util.ota_topk_excuse; Sinkhorn: the two largest rescaled plan entries within 1e-3 relative).

Observed on the CPU (tests/test_ota_edges_cpu.py: the oracle's literal class cost against the kernel's association, and the oracle's
matrices with one index rule broken); both tests print the device's figures (foreground, cap, every differing point and its excuse):
  case          top-k fg   literal vs re-associated   rank rule broken   argmin rule broken   Sinkhorn fg
  g100_0_37_1   340        0 differing points         3 (cap 1)          7 (cap 1)            239
  g1_1          10         0                          -                  -                    3
  k13_ld16      340        0                          3 (cap 1)          7 (cap 1)            240
"""
import functools

import numpy as np
import pytest
import torch

from tests import util as U

pytestmark = pytest.mark.gpu

CASES = sorted(U.OTA_EDGE_CASES)
SENT = -7


@functools.lru_cache(maxsize=None)
def _problem(name):
    return U.ota_edge_problem(*U.OTA_EDGE_CASES[name])


@functools.lru_cache(maxsize=None)
def _case(name, matching):
    """(problem, oracle result) of one case, computed once; nothing writes to either."""
    from oracle import box_ops
    prob = _problem(name)
    ref = box_ops.ota_ground_truth(prob["pts"], prob["strides"], prob["logits"], prob["pred"], prob["gt"], prob["num"], *U.OTA_ARGS,
                                   matching=matching)
    return prob, ref


def _launch(prob, matching):
    """One launch into sentinel-filled buffers: (labels, targets, ious, stats) as numpy."""
    from basedet_amd import ops
    N, P, K = prob["logits"].shape
    ld = (K + 7) // 8 * 8
    lg = torch.full((N * P, ld), 30.0, dtype=torch.bfloat16)              # slots >= K: garbage the kernel must mask
    lg[:, :K] = torch.from_numpy(prob["logits"]).reshape(N * P, K).to(torch.bfloat16)
    pr = torch.from_numpy(prob["pred"]).reshape(N * P, 4).to(torch.bfloat16)
    dev = "cuda"
    labels = torch.full((N, P), SENT, dtype=torch.int32, device=dev)
    targets = torch.full((N, P, 4), float(SENT), dtype=torch.float32, device=dev)
    ious = torch.full((N, P), float(SENT), dtype=torch.float32, device=dev)
    stats = torch.full((2,), float(SENT), dtype=torch.float32, device=dev)
    args = (torch.from_numpy(prob["allp"]).to(dev), prob["lvl_start"], prob["strides"], lg.to(dev), K, pr.to(dev),
            torch.from_numpy(prob["gt"]).to(dev), torch.from_numpy(prob["num"]).to(dev)) + U.OTA_ARGS[:4]
    kw = dict(ld=ld) if ld != K else {}
    if matching == "topk":
        ws = torch.full((ops.ota_assign_workspace_bytes(N, P),), 0xA5, dtype=torch.uint8, device=dev)
        ops.ota_assign(*args, U.OTA_ARGS[4], labels, targets, ious, stats, ws, **kw)
    else:
        ws = torch.full((ops.ota_sinkhorn_workspace_bytes(N, P, prob["gt"].shape[1]),), 0xA5, dtype=torch.uint8, device=dev)
        ops.ota_assign_sinkhorn(*args, labels, targets, ious, stats, ws, topq=20, eps=0.1, iters=50, **kw)
    torch.cuda.synchronize()
    return labels.cpu().numpy(), targets.cpu().numpy(), ious.cpu().numpy(), stats.cpu().numpy()


def _check_outputs(prob, ref, out, out2):
    """What holds for both matchers: no sentinel or NaN left, targets of agreeing foreground, zeros on background, the empty image,
    the statistics, and the same bits from a second launch."""
    lab_o, tgt_o, iou_o, _ = ref
    lab, tgt, iou_t, st = out
    for a, b in zip(out, out2):
        assert np.array_equal(a, b)
    assert np.isfinite(tgt).all() and np.isfinite(iou_t).all() and np.isfinite(st).all()
    assert (lab != SENT).all() and (tgt != SENT).all() and (iou_t != SENT).all() and (st != SENT).all()
    assert (lab >= 0).all() and (lab <= prob["logits"].shape[2]).all()
    fg = (lab == lab_o) & (lab_o > 0)
    np.testing.assert_array_equal(tgt[fg], tgt_o[fg])
    np.testing.assert_allclose(iou_t[fg], iou_o[fg], rtol=2e-6, atol=1e-7)
    assert (tgt[lab == 0] == 0).all() and (iou_t[lab == 0] == 0).all()
    for n in np.nonzero(prob["num"] == 0)[0]:
        assert (lab[n] == 0).all() and (tgt[n] == 0).all() and (iou_t[n] == 0).all() and (lab_o[n] == 0).all()
    nfg = int((lab > 0).sum())
    assert st[0] == nfg and st[1] == 2 * nfg


@pytest.mark.parametrize("name", CASES)
def test_ota_topk_edge_cases(name):
    prob, ref = _case(name, "topk")
    lab_o, _, _, aux = ref
    # ---- the oracle side: the case reaches what it is meant to reach
    fg_idx = np.nonzero(lab_o > 0)[1]
    assert (fg_idx >= 1024).any() and (fg_idx >= 2048).any()
    nfg, cap, _ = U.ota_topk_compare(prob, ref, lab_o, ref[1])
    exact, never = [], []                 # (image, point) the point-index rule decides; (image, point, class) the gt-index rule forbids
    short = 0
    for n, G in enumerate(prob["num"]):
        if G == 0:
            continue
        cost = aux[n][0]
        dyn, _, mm, srt = U.ota_topk_selection(cost, aux[n][1], U.OTA_ARGS[4])
        short += int(((cost < 1e5).sum(1) < dyn).sum())
        for kind in ("zero_area", "outside"):
            if (n, kind) in prob["planted"]:
                s = prob["planted"][(n, kind)]
                assert mm[s].any() and (cost[s] >= 1e6).all()
        if n in prob["tie_points"]:
            s, idx = prob["planted"][(n, "zero_area")], prob["tie_points"][n]
            assert dyn[s] == 1 and (cost[s, idx] == srt[s, 0]).all() and srt[s, len(idx)] > srt[s, 0] + 0.125
            assert lab_o[n, idx[0]] == int(prob["gt"][n, s, 4]) and (lab_o[n, idx[1:]] == 0).all()
            exact += [(n, p) for p in idx]
        if (n, "dup") in prob["planted"]:
            s = prob["planted"][(n, "dup")]
            assert np.array_equal(cost[0], cost[s])
            both = np.nonzero(mm[0] & mm[s] & (cost[0] == cost.min(0)))[0]
            assert (lab_o[n, both] == int(prob["gt"][n, 0, 4])).all()
            never += [(n, p, int(prob["gt"][n, s, 4])) for p in both]
    assert short >= 1                                                # a gt with fewer inside points than its dynamic k: +1e6 decides
    if prob["planted"]:
        assert len(never) > cap                                      # more gt-index conflicts than the cap would let through
    # ---- the device
    out = _launch(prob, "topk")
    _check_outputs(prob, ref, out, _launch(prob, "topk"))
    lab, tgt = out[0], out[1]
    _, _, diff = U.ota_topk_compare(prob, ref, lab, tgt)
    print(f"{name}: top-k foreground {nfg}, cap {cap}, differing points {diff}")
    assert len(diff) <= cap, (len(diff), nfg)
    assert all(e is not None for _, _, e in diff), diff
    for n, p in exact:                    # the tie points: several fp32 steps below every other cost of the row, no rounding can mix them
        assert lab[n, p] == lab_o[n, p], (n, p, int(lab[n, p]), int(lab_o[n, p]))
    for n, p, c in never:                 # gt 0 and its copy cost the same on the device too: the copy (higher index) never wins
        assert lab[n, p] != c, (n, p, c)


@pytest.mark.parametrize("name", CASES)
def test_ota_sinkhorn_edge_cases(name):
    """topq = 20, eps = 0.1, 50 iterations on the same problems, degenerate rows included (the reference's plan stays finite on them)."""
    prob, ref = _case(name, "sinkhorn")
    lab_o, _, _, aux = ref
    P = lab_o.shape[1]
    nfg = int((lab_o > 0).sum())
    assert nfg >= 1
    ious = [a[1] for a in _case(name, "topk")[1][3]]
    for n, G in enumerate(prob["num"]):
        if G == 0:
            continue
        cost_bg, pi = aux[n]
        assert np.isfinite(pi).all() and np.isfinite(cost_bg).all()
        ious_m = (ious[n] * (cost_bg[:-1] < 1e5)).astype(np.float32)          # IoU x inside mask, as the matcher sees it (ota.py:155)
        top = -np.sort(-ious_m, axis=1, kind="stable")[:, :20]
        mu = np.zeros(G, np.float32)
        for v in top.T:
            mu = (mu + v).astype(np.float32)
        assert P - np.maximum(1, mu.astype(np.int64)).sum() > 0
    out = _launch(prob, "sinkhorn")
    _check_outputs(prob, ref, out, _launch(prob, "sinkhorn"))
    lab = out[0]
    diff = [(int(n), int(p)) for n, p in np.argwhere(lab != lab_o)]
    print(f"{name}: Sinkhorn foreground {nfg}, cap {max(1, nfg // 20)}, differing points {diff}")
    assert len(diff) <= max(1, nfg // 20), (len(diff), nfg)
    for n, p in diff:
        col = np.sort(aux[n][1][:, p])[::-1]
        assert col[0] - col[1] < 1e-3 * max(col[0], 1e-30), (n, p, col[:3])

