"""csrc/centernet.hip against tests/centernet_oracle.py: targets, heat-map focal loss, gathered L1 loss, decode and the Python surface.
Operands live in guarded() allocations (tests/util.py) whose guards are checked; every launch runs twice and must repeat its bits."""
import functools
import math

import numpy as np
import pytest
import torch

import centernet_oracle as O
import util as U
from basedet_amd import ops

pytestmark = pytest.mark.gpu
BF, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8


def _in(data, name, fill="nan"):
    """A guarded device copy of data; int32 data travels in a float32 allocation of the same bits (guarded() knows float formats)."""
    data = data.contiguous()
    rows, cols = (data.shape[0], None) if data.dim() == 1 else (data.shape[0], int(np.prod(data.shape[1:])))
    is_int = data.dtype == I32
    t, h = U.guarded(rows, cols, F32 if is_int else data.dtype, "cuda", fill=fill, name=name)
    if is_int:
        U.bits_of(h.t).copy_(data.view_as(h.t))
        t = h.t.view(I32)
    else:
        h.set(data)
    return t, h.snapshot()


def _out(rows, cols, dtype, name):
    t, h = U.guarded(rows, cols, F32 if dtype == I32 else dtype, "cuda", name=name)
    return (t.view(I32) if dtype == I32 else t), h


def _twice(launch, outs, ins):
    """Run launch() twice on sentinel-filled outputs: the guards hold, the inputs come back unchanged, the two results have the same bits."""
    res = []
    for _ in range(2):
        for t, h in outs:
            U.bits_of(h.t).copy_(U.fill_pattern(h.dtype, "sentinel", h.t.numel(), "cuda").view_as(U.bits_of(h.t)))
        launch()
        torch.cuda.synchronize()
        for _, h in outs:
            h.check()
        for h in ins:
            h.assert_unchanged()
        res.append([U.bits_of(t).clone() for t, _ in outs])
    for a, b in zip(*res):
        assert torch.equal(a, b), "the launch is not reproducible"


def _ld(K):
    return (K + 7) // 8 * 8


# ---- targets ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _target_ref(shape):
    gt, num = O.target_problem(*shape)
    return gt, num, O.targets(gt, num, *shape[1:], O.BOX_SCALE, O.MIN_OVERLAP)


@pytest.mark.parametrize("shape", O.TARGET_SHAPES)
def test_targets(shape):
    N, K, H, W, T = shape
    gt, num, ref = _target_ref(shape)
    assert num.max() > T and (N == 1 or num.min() == 0)
    g, hg = _in(torch.from_numpy(gt).reshape(N, -1), "gt_boxes")
    ng, hn = _in(torch.from_numpy(num), "num_gt", fill="zero")
    outs = [_out(N * H * W, K, F32, "score_map"), _out(N * T, 2, F32, "wh"), _out(N * T, 2, F32, "reg"), _out(N * T, None, F32, "reg_mask"),
            _out(N * T, None, I32, "index"), _out(1, None, F32, "num_pos")]
    (sm, _), (wh, _), (reg, _), (mask, _), (index, _), (npos, _) = outs
    ws = torch.empty(int(ops.L().bd_centernet_targets_workspace_bytes(N)), dtype=U8, device="cuda")
    _twice(lambda: ops.centernet_targets_into(g, ng, N, gt.shape[1], K, H, W, T, O.BOX_SCALE, O.MIN_OVERLAP, sm, wh, reg, mask, index,
                                              npos, ws), outs, [hg, hn])
    np.testing.assert_array_equal(index.cpu().numpy().reshape(N, T), ref["index"])
    np.testing.assert_array_equal(mask.cpu().numpy().reshape(N, T), ref["reg_mask"])
    np.testing.assert_array_equal(wh.cpu().numpy().reshape(N, T, 2), ref["wh"])
    np.testing.assert_array_equal(reg.cpu().numpy().reshape(N, T, 2), ref["reg"])
    assert float(npos[0]) == ref["num_pos"] > 0
    got = sm.view(N, H, W, K).permute(0, 3, 1, 2).cpu().numpy()             # the reference's (N, K, H, W) view
    want = ref["score_map"]
    assert int((U.bits_of(sm) == 0).sum()) == int((want == 0).sum())                  # +0 outside every window
    np.testing.assert_array_equal(got != 0, want != 0)
    np.testing.assert_array_equal(got == 1, want == 1)
    nz = want != 0
    rel = np.abs(got[nz].astype(np.float64) - want[nz]) / want[nz]
    print(f"targets {shape}: nonzero {nz.sum()}, max rel err 2^{math.log2(max(rel.max(), 1e-30)):.1f}")
    assert rel.max() <= 2.0 ** -18


# ---- focal loss ------------------------------------------------------------------------------------------------------------------------
GRID_CAP = 4096                  # bd_loss_grid_cap(): past 256 x GRID_CAP vectors of 8 slots a thread walks more than one
FOCAL_SHAPES = [(2 * 12 * 20, 3), (35, 1), (2 * 128 * 128, 80), (3 * 33 * 65, 20), (256 * GRID_CAP + 77, 1)]


def _focal_problem(rows, K, with_pos, seed=5):
    g = torch.Generator().manual_seed(seed + rows + K)
    ld = _ld(K)
    x = U.bf16_round(torch.randn(rows, K, generator=g) * 2 - 2)
    flat = x.view(-1)
    for i, v in enumerate((20.0, -20.0, 40.0, -40.0, 20.0, -40.0)):         # both clip bounds active, on positives and negatives
        flat[(i * 7919 + 3) % flat.numel()] = v
    gt = torch.rand(rows, K, generator=g) ** 8                               # mostly small, as a score map is
    gt[torch.rand(rows, K, generator=g) < 0.6] = 0
    if with_pos:
        pos = torch.randperm(rows * K, generator=g)[:max(2, rows * K // 300)]
        gt.view(-1)[pos] = 1.0
        gt.view(-1)[(4 * 7919 + 3) % flat.numel()] = 1.0                     # a clipped positive
    logits = torch.full((rows, ld), 3.0)                                     # pad slots: a logit that would add loss if it were read
    logits[:, :K] = x
    return x, gt, logits.to(BF)


@pytest.mark.parametrize("with_pos", [True, False])
@pytest.mark.parametrize("rows,K", FOCAL_SHAPES)
def test_focal(rows, K, with_pos):
    assert ops.loss_grid_cap() == GRID_CAP
    if not with_pos and rows * K > 100000:
        rows = 4099                                                          # the num_pos = 0 rule needs no second full-size map
    ld = _ld(K)
    x, gt, logits = _focal_problem(rows, K, with_pos)
    weight, gscale = 1.5, 0.25
    ref_loss, ref_grad, clipped = O.focal_from_logits(x, gt)
    assert bool(clipped.any()) and bool((clipped & (x > 0)).any()) and bool((clipped & (x < 0)).any())
    lg, hl = _in(logits, "logits")
    sm, hs = _in(gt, "score_map")
    npos, hp = _in(torch.tensor([float((gt == 1).sum())]), "num_pos")
    assert (float(npos[0]) > 0) == with_pos
    d, hd = _out(rows, ld, BF, "dlogits")
    loss = torch.zeros(1, dtype=F32, device="cuda")
    seen = []

    def launch():
        loss.zero_()
        ops.centernet_focal_fwd_bwd(lg, sm, rows, K, ld, npos, weight, gscale, loss, d)
        seen.append(float(loss[0]))
    _twice(launch, [(d, hd)], [hl, hs, hp])
    assert seen[0] == seen[1]
    rel = abs(seen[0] - weight * ref_loss) / abs(weight * ref_loss)
    got = d.float().cpu()
    want = ref_grad * weight * gscale
    err = (got[:, :K].double() - want).abs()
    tol = 2.0 ** -8 * want.abs() + 2.0 ** -9 * want.abs().max()
    print(f"focal ({rows}, {K}) pos={with_pos}: loss {seen[0]:.6g} rel err 2^{math.log2(max(rel, 1e-30)):.1f}, grad err / tol "
          f"{float((err / tol).max()):.3f}")
    assert rel <= 2.0 ** -16
    assert bool((err <= tol).all())
    bits = U.bits_of(d).cpu()
    assert bool((bits[:, :K][clipped] == 0).all()) and bool((bits[:, K:] == 0).all())        # +0, not -0


# ---- L1 loss ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 2])
@pytest.mark.parametrize("shape", O.TARGET_SHAPES)
def test_l1(shape, off):
    N, K, H, W, T = shape
    _, _, ref = _target_ref(shape)
    ld, HW = 8, H * W
    g = torch.Generator().manual_seed(11 + N * H)
    index = torch.from_numpy(ref["index"]).clone()
    mask = torch.from_numpy(ref["reg_mask"]).clone()
    target = torch.from_numpy(ref["wh"]).clone()
    index[0, 1] = index[0, 2] = index[0, 0]                                  # three slots on one pixel
    mask[0, :3] = 1
    pred = U.bf16_round(torch.randn(N * HW, ld, generator=g) * 3 + 2)
    target[0, 3] = pred[int(index[0, 3]), off:off + 2]                       # pred == target at one slot: sign(0) = 0
    assert mask[0, 3] == 1
    weight, gscale = 0.1, 4.0
    for case_mask in (mask, torch.zeros_like(mask)):
        out = pred[:, off:off + 2].double().reshape(N, H, W, 2).permute(0, 3, 1, 2).clone().requires_grad_(True)
        ref_loss = O.l1_loss(out, case_mask.double(), index, target.double())
        ref_loss.backward()
        want = out.grad.permute(0, 2, 3, 1).reshape(N * HW, 2) * weight * gscale
        p, hp = _in(pred.to(BF), "pred")
        ix, hi = _in(index.reshape(-1).to(I32), "index", fill="zero")
        mk, hm = _in(case_mask.reshape(-1), "reg_mask")
        tg, ht = _in(target.reshape(N * T, 2), "target")
        d, hd = _out(N * HW, ld, BF, "dpred")
        loss = torch.zeros(1, dtype=F32, device="cuda")
        seen = []

        def launch():
            loss.zero_()
            ops.centernet_l1_fwd_bwd(p, ld, off, ix, mk, tg, N, H, W, T, weight, gscale, loss, d)
            seen.append(float(loss[0]))
        _twice(launch, [(d, hd)], [hp, hi, hm, ht])
        assert seen[0] == seen[1]
        got = d.float().cpu()
        bits = U.bits_of(d).cpu()
        touched = torch.zeros(N * HW, ld, dtype=torch.bool)
        touched[:, off:off + 2] = (want != 0)
        assert bool((bits[~touched] == 0).all())                             # exact +0 off the gathered pixels, pad channels included
        err = (got[:, off:off + 2].double() - want).abs()
        if float(case_mask.sum()) == 0:
            assert seen[0] == 0.0 and bool((bits == 0).all())
            continue
        rel = abs(seen[0] - weight * float(ref_loss.detach())) / (weight * float(ref_loss.detach()))
        tol = 2.0 ** -8 * want.abs() + 2.0 ** -9 * want.abs().max()
        print(f"l1 {shape} off={off}: loss {seen[0]:.6g} rel err 2^{math.log2(max(rel, 1e-30)):.1f}, grad err / tol {float((err / tol).max()):.3f}")
        assert rel <= 2.0 ** -16 and bool((err <= tol).all())


# ---- decode ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,H,W,k,with_reg", [(1, 1, 5, 7, 35, True), (2, 3, 12, 20, 100, False), (2, 80, 128, 128, 100, True)])
def test_decode(B, K, H, W, k, with_reg):
    g = torch.Generator().manual_seed(17 + K)
    ld, HW = _ld(K), H * W
    x = torch.randn(B, HW, K, generator=g) * 2 - 2
    xv = x.view(B, H, W, K)
    xv[0, 1:4, 2:5, 0] = 2.5                                                 # a plateau of equal bf16 logits: all nine are kept and tie
    xv[0, 0, 0, K - 1], xv[0, 0, 2, K - 1], xv[0, 2, 0, K - 1] = 17.0, 18.0, 20.0      # differ in bf16, all sigmoid to 1.0f
    xv[B - 1, H - 1, W - 1, 0], xv[B - 1, H - 1, W - 2, 0] = 17.5, 17.0      # neighbours that tie after the sigmoid: both are kept
    x = U.bf16_round(x)
    logits = torch.zeros(B * HW, ld)
    logits[:, :K] = x.reshape(B * HW, K)
    wh = U.bf16_round(torch.rand(B * HW, 8, generator=g) * 20 + 1)
    reg = U.bf16_round(torch.rand(B * HW, 8, generator=g))
    lg, hl = _in(logits.to(BF), "logits")
    whd, hw = _in(wh.to(BF), "wh")
    rgd, hr = _in(reg.to(BF), "reg")
    # the oracle's scores: the library's own fp32 sigmoid (bd_det_scores), which decode must reproduce bit for bit
    sc = torch.empty(B * HW, K, dtype=F32, device="cuda")
    ops.det_scores(lg, B * HW, K, sc, ld=ld)
    scores = sc.view(B, HW, K).permute(0, 2, 1).reshape(B, K, H, W).cpu().numpy()
    assert (scores == 1.0).sum() >= 5
    off = 2
    rcls, rpix, rsc, rbox = O.decode(scores, wh[:, off:off + 2].reshape(B, HW, 2).numpy(),
                                     reg[:, 4:6].reshape(B, HW, 2).numpy() if with_reg else None, k)
    outs = [_out(B * k, 4, F32, "boxes"), _out(B * k, None, F32, "scores"), _out(B * k, None, I32, "classes")]
    (boxes, _), (scs, _), (cls, _) = outs
    ws, hws = _out(ops.centernet_decode_workspace_bytes(B, K, H, W), None, U8, "ws")
    _twice(lambda: ops.centernet_decode(lg, ld, whd, 8, off, rgd if with_reg else None, 8, 4, B, K, H, W, k, boxes, scs, cls, ws),
           outs, [hl, hw, hr])
    hws.check()
    np.testing.assert_array_equal(cls.cpu().numpy().reshape(B, k), rcls)
    np.testing.assert_array_equal(scs.cpu().numpy().reshape(B, k), rsc)
    gb = boxes.cpu().numpy().reshape(B, k, 4).astype(np.float64)
    # the selected pixel of every slot, from the box centre: xs = x + reg_x with reg in [0, 1)
    cx, cy = (gb[..., 0] + gb[..., 2]) / 2, (gb[..., 1] + gb[..., 3]) / 2
    regs = reg[:, 4:6].reshape(B, HW, 2).numpy().astype(np.float64) if with_reg else np.full((B, HW, 2), 0.5)
    for b in range(B):
        np.testing.assert_allclose(cx[b] - regs[b, rpix[b], 0], rpix[b] % W, rtol=0, atol=1e-3)
        np.testing.assert_allclose(cy[b] - regs[b, rpix[b], 1], rpix[b] // W, rtol=0, atol=1e-3)
    err = np.abs(gb - rbox) / np.maximum(np.abs(rbox), 1.0)
    print(f"decode ({B}, {K}, {H}, {W}, {k}): ties at 1.0: {(rsc == 1.0).sum()}, max box rel err 2^{math.log2(max(err.max(), 1e-30)):.1f}")
    assert err.max() <= 2.0 ** -8


# ---- Python surface --------------------------------------------------------------------------------------------------------------------
class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_python_surface():
    from basedet.models import centernet as cn
    shape = O.TARGET_SHAPES[0]
    N, K, H, W, T = shape
    gt, num, ref = _target_ref(shape)
    cfg = _Cfg(DATA=_Cfg(NUM_CLASSES=K), MODEL=_Cfg(OUTPUT_SIZE=(H, W), HEAD=_Cfg(TENSOR_DIM=T, DOWN_SCALE=4, MIN_OVERLAP=O.MIN_OVERLAP)))
    gd = cn.centernet_ground_truth(torch.from_numpy(gt).cuda(), torch.from_numpy(num).cuda(), cfg)
    assert tuple(gd["score_map"].shape) == (N, K, H, W)
    sm = gd["score_map"].cpu().numpy()
    np.testing.assert_array_equal(sm != 0, ref["score_map"] != 0)             # through the (N, K, H, W) view: a swapped axis shows here
    np.testing.assert_allclose(sm, ref["score_map"], rtol=2.0 ** -18, atol=0)
    np.testing.assert_array_equal(gd["index"].cpu().numpy(), ref["index"])
    assert float(gd["num_pos"][0]) == ref["num_pos"]
    g = torch.Generator().manual_seed(23)
    x = U.bf16_round(torch.randn(N, K, H, W, generator=g) * 2 - 2)
    p64 = torch.sigmoid(x.double())
    pred = p64.float().cuda().requires_grad_(True)
    out = U.bf16_round(torch.randn(N, 2, H, W, generator=g) * 3 + 2)
    outd = out.clone().cuda().requires_grad_(True)
    loss = cn.modified_focal_loss(pred, gd["score_map"]) + 0.1 * cn.reg_l1_loss(outd, gd["reg_mask"], gd["index"], gd["wh"])
    loss.backward()
    pr = p64.clone().requires_grad_(True)
    orf = out.double().requires_grad_(True)
    lf = O.focal_loss(pr, torch.from_numpy(ref["score_map"]).double())
    ll = O.l1_loss(orf, torch.from_numpy(ref["reg_mask"]).double(), torch.from_numpy(ref["index"]), torch.from_numpy(ref["wh"]).double())
    (lf + 0.1 * ll).backward()
    # the surface rounds fp32 probabilities back to bf16 logits and the score map carries 2^-18: the loss to 2^-14, the gradients as the kernels'
    assert abs(float(loss) - float(lf + 0.1 * ll)) <= 2.0 ** -14 * float(lf + 0.1 * ll)
    for got, want in ((pred.grad.cpu().double(), pr.grad), (outd.grad.cpu().double(), orf.grad)):
        assert bool(((got - want).abs() <= 2.0 ** -7 * want.abs() + 2.0 ** -8 * want.abs().max()).all())
    # decode + transform_boxes against the oracle on the same probabilities
    whm = U.bf16_round(torch.rand(N, 2, H, W, generator=g) * 10 + 1)
    boxes, scores, clses = cn.CenterNetDecoder.decode(pred.detach(), whm.cuda(), None, K=20)
    assert tuple(boxes.shape) == (N, 20, 4) and tuple(scores.shape) == (N, 20, 1) and tuple(clses.shape) == (N, 20, 1)
    lg = torch.zeros(N * H * W, 8)
    lg[:, :K] = x.permute(0, 2, 3, 1).reshape(-1, K)
    sc = torch.empty(N * H * W, K, dtype=F32, device="cuda")
    ops.det_scores(lg.to(BF).cuda(), N * H * W, K, sc, ld=8)
    rcls, rpix, rsc, rbox = O.decode(sc.view(N, H * W, K).permute(0, 2, 1).reshape(N, K, H, W).cpu().numpy(),
                                     whm.permute(0, 2, 3, 1).reshape(N, H * W, 2).numpy(), None, 20)
    np.testing.assert_array_equal(clses.cpu().numpy()[..., 0], rcls)
    np.testing.assert_array_equal(scores.cpu().numpy()[..., 0], rsc)
    np.testing.assert_allclose(boxes.cpu().numpy(), rbox, rtol=2.0 ** -8, atol=2.0 ** -8)
    tb = cn.CenterNetDecoder.transform_boxes(boxes[0], np.asarray([W * 2, H * 2]), np.asarray([W * 4, H * 4]), (W, H))
    np.testing.assert_allclose(tb, boxes[0].cpu().numpy().astype(np.float64) * 4, rtol=1e-9, atol=1e-6)
