"""The fused loss kernels (csrc/losses.hip) and FCOS's per-level scale (csrc/norm.hip fcos_offsets_*) at production sizes,
element by element against a float64 torch restatement computed on the device.

Every kernel here caps its grid (losses.hip loss_grid: 4096 blocks of 256 threads; norm.hip OFF_BLOCKS = 512) and walks the rest
with a grid stride, so the code that only a second pass reaches -- focal_g2_kernel's (row, chunk) carry and its 4-way unrolled loads,
the later partial-sum slots -- is only exercised at these sizes.  The restated expressions are those of oracle/box_ops.py
(sigmoid_focal_loss :496-506, sigmoid_focal_loss_grad :509-523, smooth_l1_loss :526-532, ltrb_iou / iou_loss_ltrb :535-569,
binary_cross_entropy :489-493) and oracle/rcnn_ops.py rpn_losses (:252-266).

Gradients are compared in bf16 steps (util.bf16_ulps) against the float64 value rounded to bf16; loss sums against the float64
sum with a relative bound; dscale against the float64 sum relative to the sum of the magnitudes of its terms."""
import numpy as np
import pytest
import torch

from util import bf16_ulps

pytestmark = pytest.mark.gpu

FCOS_SIZES = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]     # 800x1344, strides 8..128: 22 400 points
FCOS_STRIDES = [8, 16, 32, 64, 128]
RPN_PIXELS = 200 * 336 + 100 * 168 + 50 * 84 + 25 * 42 + 13 * 21     # P2..P6 at 800x1344: 89 523


def _ops():
    from basedet_amd import ops
    return ops


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _labels(n, K, gen, p_pos=0.07, p_ign=0.05):
    """0 background, 1..K positive class, -1 ignored."""
    u = torch.rand(n, generator=gen, device="cuda")
    cls = torch.randint(1, K + 1, (n,), generator=gen, device="cuda", dtype=torch.int32)
    lab = torch.zeros(n, dtype=torch.int32, device="cuda")
    lab = torch.where(u < p_pos, cls, lab)
    return torch.where(u > 1 - p_ign, torch.full_like(lab, -1), lab)


def _norm(kind, nfg):
    if kind == "int":
        return torch.tensor([nfg], dtype=torch.int32, device="cuda"), float(max(nfg, 1))
    v = nfg * 0.75 + 0.3                                    # a non-integer normaliser (FCOS's centre-ness sum)
    return torch.tensor([v], dtype=torch.float32, device="cuda"), float(np.float32(max(v, 1.0)))


def _chunks(n, step):
    for a in range(0, n, step):
        yield a, min(n, a + step)


# ---- focal loss ------------------------------------------------------------------------------------------------
def _focal_ref(x, lab, K, alpha, gamma):
    """float64 loss and d loss / d x of sigmoid_focal_loss on rows x [r, K] with integer labels (oracle/box_ops.py:496-523)."""
    t = (torch.arange(1, K + 1, device=x.device)[None, :] == lab[:, None].long()).double()
    p = torch.sigmoid(x)
    ce = torch.nn.functional.softplus(x) - t * x
    pt = t * (1 - p) + (1 - t) * p
    a = t * alpha + (1 - t) * (1 - alpha) if alpha >= 0 else 1.0
    loss = a * ce * pt ** gamma
    grad = a * ((p - t) * pt ** gamma + ce * gamma * pt ** (gamma - 1) * (1 - 2 * t) * p * (1 - p))
    return loss, grad


# (rows, K): 680 000 x 80 -> 6.8M vectors of 8 logits: one full outer pass of 4 x 1 048 576, then u = 0, 1 full and u = 2 ragged;
# 2 266 667 x 24 (kv = 3: the chunk carry fires on every stride) -> 6 800 001 vectors; 3 225 600 x 80: RetinaNet's bench batch (16 images
# at 800x1344, 9 anchors) -> 32.3M vectors, 7.7 outer passes
FOCAL_CASES = [(680_000, 80, k, n) for k in ("g2", "general2", "general1.5") for n in ("int", "float")]
FOCAL_CASES += [(2_266_667, 24, k, n) for k in ("g2", "general2", "general1.5") for n in ("int", "float")]
FOCAL_CASES += [(3_225_600, 80, "g2", "int"), (3_225_600, 80, "g2", "float"), (3_225_600, 80, "general1.5", "float")]


@pytest.mark.parametrize("rows,K,kernel,norm_kind", FOCAL_CASES)
def test_focal_loss_past_the_grid_cap(rows, K, kernel, norm_kind):
    ops = _ops()
    gen = _gen(rows + K)
    general = kernel != "g2"
    alpha, gamma, grad_scale = 0.25, (1.5 if kernel == "general1.5" else 2.0), 0.37
    x = (torch.randn((rows, K), generator=gen, device="cuda") * 3).to(torch.bfloat16)
    lab = _labels(rows, K, gen)
    # coverage: positives at every position 0..7 of a vector in vectors reached by every u of the unrolled group, and ignored rows in
    # a later outer pass
    kv, nvec = K // 8, rows * (K // 8)
    stride = min(4096, -(-nvec // 256)) * 256
    pos_rows = torch.nonzero(lab > 0).squeeze(1)
    vec = pos_rows * kv + (lab[pos_rows].long() - 1) // 8
    combos = ((lab[pos_rows].long() - 1) % 8) * 4 + (vec // stride) % 4
    assert torch.unique(combos).numel() == 32
    assert bool(((torch.nonzero(lab < 0).squeeze(1) * kv) >= 4 * stride).any())
    assert nvec > 4 * stride and nvec % (4 * stride) > 2 * stride     # past one outer pass, ragged inside the unrolled group

    nfg = int((lab > 0).sum())
    norm, normv = _norm(norm_kind, nfg)
    loss = torch.zeros((1,), dtype=torch.float32, device="cuda")
    dl = torch.full((rows, K), 5.0, dtype=torch.bfloat16, device="cuda")
    ops.focal_loss_fwd_bwd(x, lab, rows, K, alpha, gamma, norm, grad_scale, loss, dl, general=general)

    ref_sum, worst = 0.0, 0
    for a, b in _chunks(rows, 1 << 17):
        xl, ll = x[a:b].double(), lab[a:b]
        l64, g64 = _focal_ref(xl, ll, K, alpha, gamma)
        valid = (ll >= 0)[:, None]
        ref_sum += float((l64 * valid).sum())
        g64 = g64 * valid * (grad_scale / normv)
        worst = max(worst, int(bf16_ulps(dl[a:b], g64).max()))
        ign = ll < 0
        assert bool((dl[a:b][ign].view(torch.int16) == 0).all()), "ignored rows must get exact zeros"
    ref = ref_sum / normv
    rel = abs(float(loss.item()) - ref) / ref
    print(f"focal {rows}x{K} {kernel} norm={norm_kind}: max {worst} bf16 ulp, loss rel err {rel:.2e}")
    # observed 1 (gamma = 2 kernel), 0 (general kernel); before log1p_small and sigmoid(-x) in losses.hip: 209 and 8, from the logits
    # a confident answer (|x| > 8) gives
    assert worst <= 1
    assert rel < 3e-5                 # observed <= 2.3e-6


# ---- smooth L1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 0.11])
@pytest.mark.parametrize("norm_kind", ["int", "float"])
def test_smooth_l1_past_the_grid_cap(beta, norm_kind):
    """RetinaNet's box loss at the bench batch: 16 x 22 400 pixels, A = 9 anchors in 40-channel rows (10 slots per pixel:
    3.6M slots, 3.4 passes).  The padding slot a = 9 of every pixel must be written as exact zeros."""
    ops = _ops()
    gen = _gen(11)
    pixels, A, ld, weight = 16 * 22400, 9, 40, 1.7
    pred = torch.randn((pixels, ld), generator=gen, device="cuda").to(torch.bfloat16)
    tgt = torch.randn((pixels * A, 4), generator=gen, device="cuda")
    lab = _labels(pixels * A, 80, gen, p_pos=0.3)
    nfg = int((lab > 0).sum())
    norm, normv = _norm(norm_kind, nfg)
    loss = torch.zeros((1,), dtype=torch.float32, device="cuda")
    dp = torch.full((pixels, ld), 3.0, dtype=torch.bfloat16, device="cuda")
    ops.smooth_l1_fwd_bwd(pred, tgt, lab, pixels, A, ld, beta, norm, weight, loss, dp)
    assert bool((dp[:, A * 4:].view(torch.int16) == 0).all())
    p = pred[:, : A * 4].double().reshape(-1, 4)
    d = p - tgt.double()
    fg = (lab > 0)[:, None]
    if beta < 1e-5:
        l64, g64 = d.abs(), torch.sign(d)
    else:
        l64 = torch.where(d.abs() < beta, 0.5 * d * d / beta, d.abs() - 0.5 * beta)
        g64 = torch.where(d.abs() < beta, d / beta, torch.sign(d))
    g64 = g64 * fg * (weight / normv)
    got = dp[:, : A * 4].reshape(-1, 4)
    worst = int(bf16_ulps(got, g64).max())
    assert bool((got[lab <= 0].view(torch.int16) == 0).all())
    ref = float((l64 * fg).sum()) * weight / normv
    rel = abs(float(loss.item()) - ref) / ref
    print(f"smooth_l1 beta={beta} norm={norm_kind}: max {worst} bf16 ulp, loss rel err {rel:.2e}")
    assert worst <= 1                 # observed 1 (beta = 0.11), 0 (beta = 0)
    assert rel < 3e-5                 # observed <= 1.1e-6


# ---- RPN losses ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 0.11])
def test_rpn_loss_past_the_grid_cap(beta):
    """rpn_loss_kernel at Faster R-CNN's bench batch: 16 x 89 523 pixels x A = 3 -> 4.3M (pixel, anchor) items, 4.1 passes; the fused
    16-channel row holds 3 logits at 0, 12 offsets at 3, and a padding channel 15 the kernel never writes."""
    ops = _ops()
    gen = _gen(13)
    rows, A, ldc = 16 * RPN_PIXELS, 3, 16
    raw = (torch.randn((rows, ldc), generator=gen, device="cuda") * 2).to(torch.bfloat16)
    u = torch.rand(rows * A, generator=gen, device="cuda")
    lab = torch.where(u < 0.03, 1, torch.where(u < 0.10, 0, -1)).to(torch.int32)
    targets = torch.randn((rows * A, 4), generator=gen, device="cuda")
    nvalid = int((lab >= 0).sum())
    nv = torch.tensor([nvalid], dtype=torch.int32, device="cuda")
    loss = torch.zeros((2,), dtype=torch.float32, device="cuda")
    draw = torch.full((rows, ldc), 7.0, dtype=torch.bfloat16, device="cuda")
    ops.rpn_loss_fwd_bwd(raw, ldc, A, 0, A, lab, targets, rows, beta, nv, loss, draw)
    assert bool((draw[:, 5 * A:] == 7.0).all()), "the padding channel is not the kernel's to write"
    r = raw.double()
    x, labd = r[:, :A].reshape(-1), lab.double()
    valid, fg = lab >= 0, lab > 0
    gs = 1.0 / max(nvalid, 1)
    cls64 = (torch.nn.functional.softplus(x) - labd * x) * valid
    gc64 = (torch.sigmoid(x) - labd) * valid * gs
    d = r[:, A:5 * A].reshape(-1, 4) - targets.double()
    if beta < 1e-5:
        box64, gb64 = d.abs(), torch.sign(d)
    else:
        box64 = torch.where(d.abs() < beta, 0.5 * d * d / beta, d.abs() - 0.5 * beta)
        gb64 = torch.where(d.abs() < beta, d / beta, torch.sign(d))
    box64, gb64 = box64 * fg[:, None], gb64 * fg[:, None] * gs
    wc = int(bf16_ulps(draw[:, :A].reshape(-1), gc64).max())
    wb = int(bf16_ulps(draw[:, A:5 * A].reshape(-1, 4), gb64).max())
    got = loss.cpu().numpy().astype(np.float64)
    rc = abs(got[0] - float(cls64.sum()) * gs) / (float(cls64.sum()) * gs)
    rb = abs(got[1] - float(box64.sum()) * gs) / (float(box64.sum()) * gs)
    print(f"rpn_loss beta={beta}: cls grad {wc} / box grad {wb} bf16 ulp, loss rel err cls {rc:.2e} box {rb:.2e}")
    assert wc <= 1 and wb <= 1        # observed 0, 0
    assert rc < 3e-5 and rb < 3e-5    # observed <= 2.5e-6


# ---- GIoU and centre-ness BCE (FCOS) ---------------------------------------------------------------------------
def _giou_loss64(p, t, eps=1e-8):
    """1 - giou of ltrb distances (oracle/box_ops.py ltrb_iou :535-553, iou_loss_ltrb :556-569)."""
    b1 = torch.cat([-p[:, :2], p[:, 2:]], 1)
    b2 = torch.cat([-t[:, :2], t[:, 2:]], 1)
    a1 = (b1[:, 2] - b1[:, 0]).clamp_min(0) * (b1[:, 3] - b1[:, 1]).clamp_min(0)
    a2 = (b2[:, 2] - b2[:, 0]).clamp_min(0) * (b2[:, 3] - b2[:, 1]).clamp_min(0)
    wi = (torch.minimum(b1[:, 2], b2[:, 2]) - torch.maximum(b1[:, 0], b2[:, 0])).clamp_min(0)
    hi = (torch.minimum(b1[:, 3], b2[:, 3]) - torch.maximum(b1[:, 1], b2[:, 1])).clamp_min(0)
    ai = wi * hi
    au = a1 + a2 - ai
    iou = ai / au.clamp_min(eps)
    gw = torch.maximum(b1[:, 2], b2[:, 2]) - torch.minimum(b1[:, 0], b2[:, 0])
    gh = torch.maximum(b1[:, 3], b2[:, 3]) - torch.minimum(b1[:, 1], b2[:, 1])
    ac = gw * gh
    return 1 - (iou - (ac - au) / ac.clamp_min(eps))


@pytest.mark.parametrize("rows", [16 * 22400, 1_200_000])
def test_giou_and_bce_past_the_grid_cap(rows):
    """FCOS's box and centre-ness losses at the bench batch (358 400 points) and past the 1 048 576-row grid pass."""
    ops = _ops()
    gen = _gen(rows)
    lw = 2.0
    pred = (torch.rand((rows, 4), generator=gen, device="cuda") * 59.5 + 0.5).to(torch.bfloat16)
    tgt = torch.rand((rows, 4), generator=gen, device="cuda") * 59.5 + 0.5
    w = torch.rand(rows, generator=gen, device="cuda")
    lab = _labels(rows, 80, gen, p_pos=0.5, p_ign=0.0)
    fg = lab > 0
    wsum = float(w[fg].double().sum())
    norm = torch.tensor([wsum], dtype=torch.float32, device="cuda")
    loss = torch.zeros((1,), dtype=torch.float32, device="cuda")
    dp = torch.full((rows, 4), 3.0, dtype=torch.bfloat16, device="cuda")
    ops.iou_ltrb_fwd_bwd(pred, tgt, w, lab, rows, ops.IOU_LOSS_TYPES["giou"], norm, lw, loss, dp)
    gs = lw / max(float(np.float32(wsum)), 1.0)
    p = pred.double().requires_grad_(True)
    l64 = _giou_loss64(p, tgt.double()) * w.double() * fg
    (l64.sum() * gs).backward()
    g64 = p.grad
    worst = int(bf16_ulps(dp, g64).max())
    assert bool((dp[~fg].view(torch.int16) == 0).all())
    ref = float(l64.sum()) * gs
    rel = abs(float(loss.item()) - ref) / ref
    print(f"giou rows={rows}: max {worst} bf16 ulp, loss rel err {rel:.2e}")
    assert worst <= 4                 # observed 3 (cancellation between the d iou and d hull terms, rounded to bf16)
    assert rel < 5e-6                 # observed <= 4.8e-7

    # centre-ness BCE on channel 4 of FCOS's 8-channel raw rows
    raw = (torch.randn((rows, 8), generator=gen, device="cuda") * 2).to(torch.bfloat16)
    t = torch.rand(rows, generator=gen, device="cuda")
    nf = float(fg.sum())
    nft = torch.tensor([nf], dtype=torch.float32, device="cuda")
    loss.zero_()
    dx = torch.full((rows,), 3.0, dtype=torch.bfloat16, device="cuda")
    ops.bce_logits_fwd_bwd(raw, t, lab, rows, nft, loss, dx, ld=8, off=4)
    x = raw[:, 4].double()
    td = t.double()
    bl64 = (torch.nn.functional.softplus(x) - td * x) * fg
    bg64 = (torch.sigmoid(x) - td) * fg / nf
    bworst = int(bf16_ulps(dx, bg64).max())
    assert bool((dx[~fg].view(torch.int16) == 0).all())
    bref = float(bl64.sum()) / nf
    brel = abs(float(loss.item()) - bref) / bref
    print(f"bce rows={rows}: max {bworst} bf16 ulp, loss rel err {brel:.2e}")
    assert bworst <= 3                # observed 2 (sigmoid(x) - t cancels where the target is close to the probability)
    assert brel < 6e-6                # observed <= 5.9e-7


# ---- FCOS per-level scale ------------------------------------------------------------------------------------------
def test_fcos_offsets_fwd_bwd_at_the_bench_batch():
    """fcos_offsets_fwd / fcos_offsets_bwd (+ fcos_dscale_final) on 16 x 22 400 points over the five FCOS levels: the backward runs
    512 blocks of 256 threads, so every thread walks 2.7 points.  Scales of both signs; exact zeros in raw (relu's gate closed)."""
    ops = _ops()
    from basedet_amd.ops import Geom
    gen = _gen(17)
    N = 16
    geom = Geom(N, [h for h, _ in FCOS_SIZES], [w for _, w in FCOS_SIZES])
    P = N * geom.pix_per_img
    raw = (torch.randn((P, 8), generator=gen, device="cuda") * 2).to(torch.bfloat16)
    raw[torch.rand((P, 8), generator=gen, device="cuda") < 0.05] = 0
    scales = torch.tensor([1.3, -0.7, 0.9, -1.1, 0.55], dtype=torch.float32, device="cuda")
    out = torch.full((P, 4), 3.0, dtype=torch.bfloat16, device="cuda")
    ops.fcos_offsets_fwd(raw, 8, scales, geom, FCOS_STRIDES, out)

    lvl = torch.zeros(geom.pix_per_img, dtype=torch.long, device="cuda")
    for i, o in enumerate(geom.off):
        lvl[o:] = i
    lvl = lvl.repeat(N)
    sc = scales.double()[lvl][:, None]
    st = torch.tensor(FCOS_STRIDES, dtype=torch.float64, device="cuda")[lvl][:, None]
    r = raw[:, :4].double()
    fwd64 = (r * sc).clamp_min(0) * st
    fworst = int(bf16_ulps(out, fwd64).max())

    d_off = torch.randn((P, 4), generator=gen, device="cuda").to(torch.bfloat16)
    d_ctr = torch.randn((P,), generator=gen, device="cuda").to(torch.bfloat16)
    d_raw = torch.full((P, 8), 3.0, dtype=torch.bfloat16, device="cuda")
    dscale = torch.full((5,), 9.0, dtype=torch.float32, device="cuda")
    ws = torch.empty((ops.fcos_offsets_workspace_bytes(),), dtype=torch.uint8, device="cuda")
    ops.fcos_offsets_bwd(raw, 8, scales, geom, FCOS_STRIDES, d_off, d_ctr, d_raw, dscale, ws)
    on = (r * sc) > 0
    go = d_off.double()
    draw64 = torch.where(on, go * st * sc, torch.zeros_like(go))
    bworst = int(bf16_ulps(d_raw[:, :4], draw64).max())
    assert torch.equal(d_raw[:, 4].view(torch.int16), d_ctr.view(torch.int16)), "d_ctr column must be copied bit for bit"
    assert bool((d_raw[:, 5:].view(torch.int16) == 0).all()), "padding channels must be exact zeros"
    terms = torch.where(on, go * st * r, torch.zeros_like(go)).sum(1)
    ds64 = torch.zeros(5, dtype=torch.float64, device="cuda").index_add_(0, lvl, terms)
    mag = torch.zeros(5, dtype=torch.float64, device="cuda").index_add_(0, lvl, terms.abs())
    drel = ((dscale.double() - ds64).abs() / mag).max().item()
    print(f"fcos_offsets: fwd {fworst} / bwd {bworst} bf16 ulp, dscale err / sum|terms| {drel:.2e}")
    assert fworst <= 1 and bworst <= 1     # observed 0, 0
    assert drel < 4e-8                     # observed 3.7e-9
