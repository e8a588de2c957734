"""The float64 references of the launches only the Faster R-CNN step makes (tests/util.py: thin_ref_*, roi_align_ref_*, subsample2x_ref*,
f32_to_bf16_ref, rcnn_loss_ref) against independent forms at small sizes: the numpy oracle's RoIAlign loop and the reference's own
known-answer vector, the adjoint identity <A x, y> = <x, A^T y>, and torch autograd in float64.  The GPU audit
(tests/test_frcnn_audit_gpu.py) trusts these references; its bound helpers (tests/audit.py) are checked here as well."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from basedet_amd import ops
from oracle import rcnn_ops as orc
from tests import audit as A
from tests import util as U

BF = torch.bfloat16
STRIDES = [4, 8, 16, 32]


def _pyramid(N, sizes, C, gen, extra_levels=1):
    """A pixel-major bf16 pyramid (N * ppi, C) with one more (unpooled) level behind the RoI levels, and its Geom."""
    H = [h for h, _ in sizes] + [3] * extra_levels
    W = [w for _, w in sizes] + [5] * extra_levels
    geom = ops.Geom(N, H, W)
    return torch.randn(geom.pixels, C, generator=gen).to(BF), geom


def _feats(buf, geom, nlev):
    v = buf.float().view(geom.N, geom.pix_per_img, -1)
    return [v[:, geom.off[l]:geom.off[l] + geom.H[l] * geom.W[l]].reshape(geom.N, geom.H[l], geom.W[l], -1).numpy() for l in range(nlev)]


def _rois(gen, N, per, img_hw):
    """Boxes of every pyramid level, some hanging over the image border, some empty slots (label -1)."""
    side = torch.tensor([20.0, 90.0, 150.0, 300.0, 500.0, 1000.0])[torch.randint(0, 6, (N * per,), generator=gen)]
    side = side * (0.7 + 0.6 * torch.rand(N * per, generator=gen))
    cx = torch.rand(N * per, generator=gen) * img_hw[1]
    cy = torch.rand(N * per, generator=gen) * img_hw[0]
    asp = 0.5 + torch.rand(N * per, generator=gen)
    rois = torch.stack([cx - side * asp / 2, cy - side / asp / 2, cx + side * asp / 2, cy + side / asp / 2], 1).float()
    labels = torch.randint(-1, 4, (N * per,), generator=gen).to(torch.int32)
    return rois, labels


def test_roi_levels_match_the_oracle_and_the_known_values():
    def sq(s):
        return [10.0, 20.0, 10.0 + s, 20.0 + s]
    rois = torch.tensor([sq(224), sq(223.9), sq(112), sq(111), sq(448), sq(2000), sq(8), sq(0), [5.0, 5.0, 1.0, 9.0]])
    for dt in (torch.float32, torch.float64):
        assert U.roi_levels(rois, STRIDES, dt).tolist() == [2, 1, 1, 0, 3, 3, 0, 0, 0]
    gen = torch.Generator().manual_seed(3)
    r, _ = _rois(gen, 4, 64, (200, 320))
    assert U.roi_levels(r, STRIDES, torch.float32).tolist() == orc.assign_roi_levels(r.numpy(), STRIDES).tolist()
    assert U.roi_levels(r, [1], torch.float64).tolist() == [0] * r.shape[0]


def test_roi_align_reference_known_answer():
    """The reference's own vector (tests/layers/test_roi_pool.py:32-45): 5 x 5 arange map, RoI [1, 1, 3, 3], stride 1, pool 4."""
    k = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_kat.npz"))
    feat = torch.from_numpy(k["roi_feat"]).permute(0, 2, 3, 1).reshape(25, 1).to(BF)
    feat = torch.cat([feat, feat, feat, feat, feat, feat, feat, feat], 1).contiguous()          # 8 identical channels
    rois = torch.from_numpy(k["roi_rois"][:, 1:]).float()
    geom = ops.single(1, 5, 5)
    lv = U.roi_levels(rois, [1], torch.float64)
    ref, S, F, ex = U.roi_align_ref_fwd(feat, geom, 1, [1], 8, rois, None, 1, (4, 4), 2, lv)
    for c in range(8):
        assert np.array_equal(ref.view(16, 8)[:, c].reshape(4, 4).numpy(), k["roi_align_4x4"])
    assert torch.equal(ref, S) and not ex.any() and bool((F >= S).all())


@pytest.mark.parametrize("pool", [(7, 7), (14, 14), (3, 5)])
def test_roi_align_reference_against_the_oracle(pool):
    gen = torch.Generator().manual_seed(pool[0])
    N, C, per = 2, 8, 24
    sizes = [(50, 80), (25, 40), (13, 20), (7, 10)]
    buf, geom = _pyramid(N, sizes, C, gen)
    rois, labels = _rois(gen, N, per, (200, 320))
    lv = U.roi_levels(rois, STRIDES, torch.float32)
    assert len(set(lv.tolist())) == 4 and bool((labels < 0).any())
    ref, S, F, ex = U.roi_align_ref_fwd(buf, geom, 4, STRIDES, C, rois, labels, per, pool, 2, lv, rois_chunk=7)
    bidx = np.arange(N * per) // per
    want = orc.roi_align(_feats(buf, geom, 4), rois.numpy(), bidx, STRIDES, pool[0], pool[1], 2).reshape(N * per, -1)
    want[labels.numpy() < 0] = 0
    # the oracle computes coordinates and sums in float32: a few 1e-5 of the 4 x 4 neighbourhood's magnitude
    err = (ref - torch.from_numpy(want).double()).abs()
    assert bool((err <= 2e-4 * F + 1e-6 * S).all()), float((err / (F + 1e-30)).max())
    assert bool((ref[labels < 0] == 0).all()) and bool(ex[labels < 0].all()) and not bool(ex[labels >= 0].any())
    assert bool((S >= ref.abs() - 1e-12).all()) and bool((F >= S - 1e-12).all())
    # with edge_eps, F shrinks to the four corners except for samples next to a cell edge; it still bounds S, and eps = 1 keeps the wide form
    _, S2, Fn, _ = U.roi_align_ref_fwd(buf, geom, 4, STRIDES, C, rois, labels, per, pool, 2, lv, edge_eps=[1e-4] * 4)
    _, _, Fw, _ = U.roi_align_ref_fwd(buf, geom, 4, STRIDES, C, rois, labels, per, pool, 2, lv, edge_eps=[1.0] * 4)
    assert torch.equal(S2, S) and torch.equal(Fw, F) and bool((Fn <= F + 1e-12).all()) and bool((Fn >= S - 1e-12).all()) and float(Fn.sum()) < 0.6 * float(F.sum())
    # the adjoint: against the oracle's scatter, and <A x, y> = <x, A^T y> with x = the bf16 pyramid
    g = torch.randn(N * per, ref.shape[1], generator=gen).to(BF)
    gr, gS, gG, cnt = U.roi_align_ref_bwd(g, geom, 4, STRIDES, C, rois, labels, per, pool, 2, lv, rois_chunk=5)
    gm = g.float().numpy().reshape(N * per, pool[0] * pool[1], C).copy()
    gm[labels.numpy() < 0] = 0
    want_g = orc.roi_align_backward(gm, [(N, h, w, C) for h, w in sizes], rois.numpy(), bidx, STRIDES, pool[0], pool[1], 2)
    v = gr.view(N, geom.pix_per_img, C)
    for l, (h, w) in enumerate(sizes):
        got = v[:, geom.off[l]:geom.off[l] + h * w].reshape(N, h, w, C)
        Gl = gG.view(N, geom.pix_per_img, C)[:, geom.off[l]:geom.off[l] + h * w].reshape(N, h, w, C)
        e = (got - torch.from_numpy(want_g[l])).abs()
        assert bool((e <= 2e-4 * Gl + 1e-9).all()), (l, float(e.max()))
    assert bool((v[:, geom.off[4]:] == 0).all())                                   # the unpooled level
    lhs = float((ref * g.double()).sum())
    rhs = float((buf.double() * gr).sum())
    assert abs(lhs - rhs) <= 1e-10 * float((S * g.double().abs()).sum())
    assert bool((gS >= gr.abs() - 1e-12).all()) and float(cnt.sum()) > 0
    # cnt counts the nonzero-weight (sample, corner) terms: the same total as the forward's
    total = 0
    for n in range(N):
        for l in range(4):
            sel = torch.nonzero((torch.arange(N * per) // per == n) & (lv == l) & (labels >= 0)).view(-1)
            if sel.numel():
                total += int((U._roi_samples(rois[sel], 1.0 / STRIDES[l], sizes[l][0], sizes[l][1], pool[0], pool[1], 2)[1] != 0).sum())
    assert int(cnt.sum()) == total


def test_roi_samples_outside_the_window_and_at_the_border():
    """A sample below -1 or above the size contributes nothing; one between -1 and 0 clamps onto the first row with full weight; the last
    row / column has a single corner (both indices equal, weight on the first)."""
    rois = torch.tensor([[-40.0, -40.0, -12.0, -12.0], [-2.0, -2.0, 2.0, 2.0], [36.0, 36.0, 60.0, 60.0]])
    idx, wgt, cell, frac = U._roi_samples(rois, 0.25, 10, 10, 2, 2, 2)
    assert float(wgt[0].abs().sum()) == 0.0
    assert bool(torch.allclose(wgt[1].sum(-1), torch.ones(4, 4, dtype=torch.float64)))
    assert int(idx[1].max()) <= 11 and int(idx[1, 0].min()) == 0              # samples at -0.875 .. -0.125: clamped onto pixel (0, 0)
    assert bool(((frac >= 0) & (frac < 1)).all())
    inside = wgt[2].sum(-1)
    assert bool(((inside == 0) | ((inside - 1).abs() < 1e-12)).all()) and int(idx[2].max()) == 99


def test_thin_references_against_autograd():
    gen = torch.Generator().manual_seed(5)
    M, Cin, Cout, real = 301, 256, 16, 15
    x = torch.randn(M, Cin, generator=gen).clamp_min(0).to(BF)
    x[7, 3] = -0.0                                                        # a negative zero is a closed gate too
    w = torch.randn(Cout, Cin, generator=gen) * 0.05
    w[real:] = 0
    bias = torch.randn(Cout, generator=gen)
    g = torch.randn(M, Cout, generator=gen).to(BF)
    g[:, real:] = 0
    wb = w.to(BF).double().requires_grad_(True)
    xd = x.double().requires_grad_(True)
    bd = bias.double().requires_grad_(True)
    y = xd @ wb.t() + bd
    ref, S = U.thin_ref_fwd(x, w, bias, chunk=64)
    assert torch.allclose(ref, y.detach(), rtol=0, atol=1e-12) and bool((S >= ref.abs() - 1e-12).all())
    y.backward(g.double())
    dx, sdx, ex, dW, sW, db, sb = U.thin_ref_bwd(x, g, w, real, chunk=50)
    assert torch.allclose(dx, xd.grad * (x.double() != 0), rtol=0, atol=1e-12)
    assert torch.equal(ex, x.float() == 0) and bool(ex[7, 3]) and bool((dx[ex] == 0).all()) and bool((sdx[ex] == 0).all())
    assert torch.allclose(dW, wb.grad, rtol=0, atol=1e-10) and torch.allclose(db, bd.grad, rtol=0, atol=1e-10)
    assert bool((dW[real:] == 0).all()) and bool((db[real:] == 0).all()) and bool((sW >= dW.abs() - 1e-12).all()) and bool((sb >= db.abs()).all())
    # a gradient in the padding row must not reach dW / db
    g2 = g.clone()
    g2[:, real:] = 1.0
    out = U.thin_ref_bwd(x, g2, w, real, dx=False)
    assert out[0] is None and bool((out[3][real:] == 0).all()) and bool((out[5][real:] == 0).all())


@pytest.mark.parametrize("beta", [0.0, 1.0 / 9.0])
def test_rcnn_loss_reference_against_autograd(beta):
    gen = torch.Generator().manual_seed(11)
    R, K = 97, 5
    box_off, ld = K + 1, 32
    raw = (torch.randn(R, ld, generator=gen) * 2).to(BF)
    labels = torch.randint(-1, K + 1, (R,), generator=gen).to(torch.int32)
    targets = torch.randn(R, 4, generator=gen)
    ns = int((labels >= 0).sum())
    out = U.rcnn_loss_ref(raw, ld, K, box_off, labels, targets, beta, ns)
    r = raw.double().requires_grad_(True)
    v = labels >= 0
    lab = labels.to(torch.int64)
    cls = TF.cross_entropy(r[v, :K + 1], lab[v], reduction="sum") / ns
    fg = lab > 0
    d = r[:, box_off:box_off + 4 * K].reshape(R, K, 4)[fg, lab[fg] - 1] - targets.double()[fg]
    box = (d.abs() if beta < 1e-5 else torch.where(d.abs() < beta, 0.5 * d * d / beta, d.abs() - 0.5 * beta)).sum() / ns
    (cls + box).backward()
    assert abs(out["cls"] - float(cls)) < 1e-12 and abs(out["box"] - float(box)) < 1e-12
    assert torch.allclose(out["draw"], r.grad, rtol=0, atol=1e-14)
    assert bool((out["draw"][~v] == 0).all()) and bool(out["exact"][~v].all())
    assert bool((out["draw"][:, box_off + 4 * K:] == 0).all()) and bool(out["exact"][:, box_off + 4 * K:].all())
    assert not bool(out["exact"][v][:, :K + 1].any()) and bool((out["draw"][out["exact"]] == 0).all())
    assert bool((out["S_draw"] >= out["draw"].abs() - 1e-15).all()) and out["S_cls"] >= out["cls"] and out["S_box"] >= out["box"]
    cls_np, box_np = orc.rcnn_losses(raw.float().numpy()[v.numpy(), :K + 1], raw.float().numpy()[v.numpy(), box_off:box_off + 4 * K].reshape(-1, K, 4),
                                     labels.numpy()[v.numpy()], targets.numpy()[v.numpy()], beta)
    assert abs(cls_np - out["cls"]) < 1e-9 and abs(box_np - out["box"]) < 1e-9


def test_subsample_and_conversion_references():
    gen = torch.Generator().manual_seed(2)
    N, C = 2, 8
    geom = ops.Geom(N, [13, 7], [21, 11])
    buf = torch.randn(geom.pixels, C, generator=gen).to(BF)
    want = U.subsample2x_ref(buf, geom.level(0), geom.level(1))
    x = buf.view(N, geom.pix_per_img, C)[:, :13 * 21].reshape(N, 13, 21, C).permute(0, 3, 1, 2).float()
    assert torch.equal(want.float().reshape(N, 7, 11, C).permute(0, 3, 1, 2), TF.max_pool2d(x, 1, 2))
    ref, S, touched = U.subsample2x_ref_bwd(buf, geom.level(1), geom.level(0))
    xd = x.double().requires_grad_(True)
    gd = buf.view(N, geom.pix_per_img, C)[:, 13 * 21:].reshape(N, 7, 11, C).permute(0, 3, 1, 2).double()
    TF.max_pool2d(xd, 1, 2).backward(gd)
    assert torch.allclose(ref.reshape(N, 13, 21, C).permute(0, 3, 1, 2), x.double() + xd.grad, rtol=0, atol=0)
    assert int(touched[:, :, 0].sum()) == N * 7 * 11 and bool((ref[~touched] == buf.view(N, geom.pix_per_img, C)[:, :13 * 21].double()[~touched]).all())
    src = torch.randn(64, 8, generator=gen)
    ref, S = U.f32_to_bf16_ref(src)
    assert torch.equal(ref, src.double())
    ref, S = U.f32_to_bf16_ref(src, buf[:64])
    assert torch.equal(ref, src.double() + buf[:64].double()) and bool((S >= ref.abs()).all())


def test_k_derived_bf16_term_and_thin_plan():
    """abs_bf16(K): two fp32 roundings per 32-product MFMA step plus three epilogue adds, never below 2^-16 -- which it equals up to 126
    steps (K <= 4 032 for a 1x1, Cin <= 448 for a 3x3).  It is ABOVE 2^-16 for res5's 3x3 512 -> 512 convolutions (K = 4 608: 291 x 2^-24,
    forward and data gradient, also in the RetinaNet / FCOS audit, whose bound on those launches grew by 14 %) and for rcnn.fc1
    (K = 12 544: 787 x 2^-24, still below the weight S / K of one product)."""
    for K in (64, 256, 576, 1024, 2048, 2304, 4032):
        assert A.abs_bf16(K) == A.ABS_BF16
    assert A.abs_bf16(4064) == 257 * A.U24
    for cin in (64, 128, 256):
        assert A.abs_bf16(cin, taps=9) == A.ABS_BF16
    assert A.abs_bf16(512, taps=9) == 291 * A.U24 and A.abs_bf16(2048) == A.ABS_BF16
    assert A.roi_coord_err(200, 336) == 9 * 337 * A.U24 and A.roi_weight_err(200, 336) == 2 * A.roi_coord_err(200, 336) + 3 * A.U24
    assert A.abs_bf16(12544) == (2 * 392 + 3) * A.U24 and A.abs_bf16(12544) < 1.0 / 12544
    assert A.abs_bf16(2304, per_step=16) == (2 * 144 + 3) * A.U24
    # the thin backward's plan at C4: 89 523 groups over 256 workgroups
    assert A.thin_bwd_roundings(16 * 89523, 256) == 350 + 4 + 32 + 3
    assert A.thin_bwd_roundings(100, 256) == 1 + 4 + 1 + 3
    assert A.probe_columns(12544).sum() == 98 and A.probe_columns(12544)[[0, 255, 256, 12543]].all()
