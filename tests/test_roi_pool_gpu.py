"""RoI max pooling on the model's pyramid (bd_roi_pool_fwd / bd_roi_pool_bwd_bf16, csrc/rcnn_ops.hip): ROI_POOLER.METHOD = "roi_pool".

Forward: exact equality with oracle.rcnn_ops.roi_pool_max per level on the bf16 values (a maximum of bf16 values has no rounding), levels
from oracle.rcnn_ops.assign_roi_levels.  Backward: a reference written here -- the first maximum of every window in row-major order takes
the bin's gradient, float64 sums of the bf16 gradients -- with a bound derived per pixel and channel:
    |got - ref| <= 2^-8 |ref| + n 2^-24 sum|terms|
(one bf16 rounding of the total; an fp32 accumulation bound over the n terms that meet there).  Elements that no bin selects are exactly 0
(accumulate = 0) or keep their bits (accumulate = 1).  Guard bands: both launches at a gapped geometry, no byte outside the tensors changes."""
import functools

import numpy as np
import pytest
import torch

from oracle import rcnn_ops as orc
from tests import util as U

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
STRIDES = [4, 8, 16, 32, 64]
LEVELS = [(128, 160), (64, 80), (32, 40), (16, 20), (8, 10)]       # the pyramid of a 512 x 640 image
NLEV = 4                                                            # RoI levels (P6 only receives zeros)
N = 2
# slots of the named cases
EDGE, OUTSIDE, TINY, FLIPPED, NEGATIVE, CONSTANT, EMPTY_A, EMPTY_B = 0, 1, 2, 3, 4, 5, 7, 8
NAMED = {EDGE: (500.0, 400.0, 900.0, 800.0),          # level 2 (stride 16, 32 x 40): x2 = 56 > 40, y2 = 50 > 32
         OUTSIDE: (2000.0, 2000.0, 2300.0, 2300.0),   # level 2: x1 = 125 > 40 -- every bin is empty
         TINY: (100.0, 100.0, 104.0, 104.0),          # level 0: 2 x 2 pixels, fewer than any pooled size here -- bins overlap
         FLIPPED: (300.0, 200.0, 250.0, 260.0),       # x2 < x1: rw = 1
         NEGATIVE: (88.0, 88.0, 152.0, 152.0),        # level 0, inside the all-negative patch of image 0
         CONSTANT: (260.0, 260.0, 340.0, 340.0)}      # level 0, inside the constant patch of image 1
NEG_PATCH = (0, 20, 40, 20, 40)       # image, rows, columns of level 0
CONST_PATCH = (1, 60, 90, 60, 90)


def _ops():
    from basedet_amd import ops
    return ops


def _geom(levels=LEVELS):
    return _ops().Geom(N, [h for h, _ in levels], [w for _, w in levels])


@functools.lru_cache(maxsize=None)
def _feat(C, seed=0):
    """(N * pix_per_img, C) bf16 on the CPU: N(0, 1), an all-negative and a constant patch on level 0."""
    g = _geom()
    f = torch.randn((N, g.pix_per_img, C), generator=torch.Generator().manual_seed(seed)).to(BF)
    H, W = LEVELS[0]
    l0 = f[:, :H * W].view(N, H, W, C)
    n, y0, y1, x0, x1 = NEG_PATCH
    l0[n, y0:y1, x0:x1] = -l0[n, y0:y1, x0:x1].abs() - 0.125
    n, y0, y1, x0, x1 = CONST_PATCH
    l0[n, y0:y1, x0:x1] = 0.5
    return f.view(-1, C)


@functools.lru_cache(maxsize=None)
def _rois(S, seed=1):
    """(N, S, 4) float32 boxes with coordinates >= 0 and areas on all four levels, the named cases in their slots; labels (N, S) int32."""
    rng = np.random.default_rng(seed)
    rois = np.zeros((N, S, 4), np.float32)
    side = [(8, 110), (115, 220), (230, 440), (450, 640)]
    for n in range(N):
        for i in range(S):
            lo, hi = side[i % 4]
            s, ratio = rng.uniform(lo, hi), rng.uniform(0.8, 1.25)
            w, h = s * ratio, s / ratio
            x1, y1 = rng.uniform(0, max(640 - 0.6 * w, 1)), rng.uniform(0, max(512 - 0.6 * h, 1))
            rois[n, i] = (x1, y1, x1 + w, y1 + h)
    labels = rng.integers(0, 5, (N, S)).astype(np.int32)
    for slot, box in NAMED.items():
        rois[1 if slot == CONSTANT else 0, slot] = box
        labels[:, slot] = 1
    labels[:, [EMPTY_A, EMPTY_B]] = -1
    return rois, labels


def _window(p, start, b, n):
    return min(max(int(np.floor(np.float32(p) * b)) + start, 0), n), min(max(int(np.ceil(np.float32(p + 1) * b)) + start, 0), n)


def _windows(roi, stride, H, W, PH, PW):
    """[(hs, he, ws, we)] per bin, the rule of oracle.rcnn_ops.roi_pool_max."""
    x1, y1, x2, y2 = [int(np.floor(np.float32(v) * np.float32(1.0 / stride) + np.float32(0.5))) for v in roi]
    rw, rh = max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)
    bh, bw = np.float32(rh) / np.float32(PH), np.float32(rw) / np.float32(PW)
    return [_window(ph, y1, bh, H) + _window(pw, x1, bw, W) for ph in range(PH) for pw in range(PW)]


def _level_nhwc(feat, g, l):
    C = feat.shape[1]
    return feat.float().numpy().reshape(g.N, g.pix_per_img, C)[:, g.off[l]:g.off[l] + g.H[l] * g.W[l]].reshape(g.N, g.H[l], g.W[l], C)


def ref_fwd(feat, g, strides, rois, labels, pool):
    """(R, PH*PW, C) float32: oracle.rcnn_ops.roi_pool_max per level, bin-major; empty slots give zero rows."""
    R, C = rois.shape[0], feat.shape[1]
    S = R // g.N
    lv = orc.assign_roi_levels(rois, strides)
    out = np.zeros((R, pool[0] * pool[1], C), np.float32)
    for l in range(len(strides)):
        idx = np.nonzero((lv == l) & (labels >= 0))[0]
        if idx.size == 0:
            continue
        nchw = np.ascontiguousarray(_level_nhwc(feat, g, l).transpose(0, 3, 1, 2))
        rois5 = np.concatenate([(idx // S).astype(np.float32)[:, None], rois[idx]], 1)
        o = orc.roi_pool_max(nchw, rois5, 1.0 / strides[l], pool[0], pool[1])
        out[idx] = o.reshape(idx.size, C, -1).transpose(0, 2, 1)
    return out, lv


def ref_bwd(feat, g, strides, rois, labels, pool, gout):
    """float64 sums, term counts and sums of |terms| per (pixel, channel): every bin's gradient to the FIRST maximum of its window."""
    R, C = rois.shape[0], feat.shape[1]
    S = R // g.N
    lv = orc.assign_roi_levels(rois, strides)
    ref = np.zeros((g.N * g.pix_per_img, C), np.float64)
    mag = np.zeros_like(ref)
    cnt = np.zeros(ref.shape, np.int32)
    ar = np.arange(C)
    lvls = [_level_nhwc(feat, g, l) for l in range(len(strides))]
    go = gout.double().numpy()
    for r in range(R):
        if labels[r] < 0:
            continue
        l, n = int(lv[r]), r // S
        H, W = g.H[l], g.W[l]
        for b, (hs, he, ws, we) in enumerate(_windows(rois[r], strides[l], H, W, pool[0], pool[1])):
            if he <= hs or we <= ws:
                continue
            first = lvls[l][n, hs:he, ws:we].reshape(-1, C).argmax(0)        # numpy: the first occurrence, here in row-major order
            rows = n * g.pix_per_img + g.off[l] + (hs + first // (we - ws)) * W + ws + first % (we - ws)
            ref[rows, ar] += go[r, b]
            mag[rows, ar] += np.abs(go[r, b])
            cnt[rows, ar] += 1
    return ref, mag, cnt


def run_fwd(feat, g, rois, labels, S, pool, C):
    ops = _ops()
    out = torch.full((rois.shape[0], pool[0] * pool[1] * C), float("nan"), dtype=BF, device="cuda")
    ops.roi_pool_fwd(feat.cuda(), g, NLEV, STRIDES, C, torch.from_numpy(rois).cuda(), None if labels is None else torch.from_numpy(labels).cuda(),
                     S, pool, out)
    torch.cuda.synchronize()
    return out.cpu().view(rois.shape[0], pool[0] * pool[1], C)


def run_bwd(feat, g, rois, labels, S, pool, C, gout, prior=None):
    ops = _ops()
    ws = torch.empty((ops.roi_pool_bwd_bf16_workspace_bytes(g, S),), dtype=torch.uint8, device="cuda")
    gf = torch.full((g.pixels, C), float("nan"), dtype=BF, device="cuda") if prior is None else prior.clone().cuda()
    ops.roi_pool_bwd_bf16(feat.cuda(), gout.cuda(), g, NLEV, STRIDES, C, torch.from_numpy(rois).cuda(), torch.from_numpy(labels).cuda(), S, pool,
                          gf, ws, accumulate=prior is not None)
    torch.cuda.synchronize()
    return gf.cpu()


def check_bwd(got, ref, mag, cnt, prior=None):
    """The derived bound on every touched element; untouched ones exactly zero / bit-identical to what was there."""
    touched = cnt > 0
    n = cnt.astype(np.float64)
    if prior is not None:
        p = prior.double().numpy()
        ref, mag, n = ref + p, mag + np.abs(p), n + 1
    gd = got.double().numpy()
    tol = 2.0 ** -8 * np.abs(ref) + n * 2.0 ** -24 * mag
    err = np.abs(gd - ref)
    worst = float((err[touched] / np.maximum(tol[touched], 1e-300)).max()) if touched.any() else 0.0
    print(f"touched {int(touched.sum())}, most terms on one element {int(cnt.max())}, worst error / bound {worst:.3f}")
    assert bool((err[touched] <= tol[touched]).all()), worst
    bits = U.bits_of(got).numpy()
    want = np.zeros_like(bits) if prior is None else U.bits_of(prior).numpy()
    assert np.array_equal(bits[~touched], want[~touched])


def _assert_named_cases(feat, g, rois, labels, lv, pool, out):
    """Every named case is present in these inputs, and does what its name says."""
    S = rois.shape[0] // N
    PH, PW = pool
    assert set(lv[labels >= 0].tolist()) == {0, 1, 2, 3}
    wins = {k: _windows(rois[(1 if k == CONSTANT else 0) * S + k], STRIDES[lv[(1 if k == CONSTANT else 0) * S + k]],
                        *LEVELS[lv[(1 if k == CONSTANT else 0) * S + k]], PH, PW) for k in NAMED}
    assert lv[EDGE] == 2 and 900 / 16 > LEVELS[2][1] and 800 / 16 > LEVELS[2][0]
    assert wins[EDGE][-1][1] == LEVELS[2][0] and wins[EDGE][-1][3] == LEVELS[2][1]            # the last bin is cut at the map's edges
    assert all(he <= hs or we <= ws for hs, he, ws, we in wins[OUTSIDE]) and not out[OUTSIDE].any()
    t = np.array(wins[TINY])
    assert lv[TINY] == 0 and 0 < t[:, 1].max() - t[:, 0].min() < PH and 0 < t[:, 3].max() - t[:, 2].min() < PW          # fewer pixels than bins:
    assert (t[:, 1] > t[:, 0]).all() and (t[:, 3] > t[:, 2]).all()                                                      # no bin is empty, so bins share pixels
    assert rois[FLIPPED, 2] < rois[FLIPPED, 0] and all(we - ws <= 1 for _, _, ws, we in wins[FLIPPED])
    assert (labels[[EMPTY_A, EMPTY_B, S + EMPTY_A, S + EMPTY_B]] < 0).all()
    assert not out[[EMPTY_A, EMPTY_B, S + EMPTY_A, S + EMPTY_B]].any()
    n, y0, y1, x0, x1 = NEG_PATCH
    assert lv[NEGATIVE] == 0 and all(y0 <= hs < he <= y1 and x0 <= ws < we <= x1 for hs, he, ws, we in wins[NEGATIVE])
    assert (out[NEGATIVE] < 0).all()                      # the negative maximum, not the 0 of an empty bin
    n, y0, y1, x0, x1 = CONST_PATCH
    assert lv[S + CONSTANT] == 0 and all(y0 <= hs < he <= y1 and x0 <= ws < we <= x1 for hs, he, ws, we in wins[CONSTANT])
    assert (out[S + CONSTANT] == 0.5).all()


FWD_CASES = [(pool, S, 256) for pool in ((7, 7), (14, 14), (3, 5)) for S in (512, 37)] + [(pool, 37, 64) for pool in ((7, 7), (14, 14), (3, 5))]


@pytest.mark.parametrize("pool,S,C", FWD_CASES)
def test_forward_equals_oracle(pool, S, C):
    g = _geom()
    feat = _feat(C)
    rois, labels = _rois(S)
    rois, labels = rois.reshape(-1, 4), labels.reshape(-1)
    want, lv = ref_fwd(feat, g, STRIDES[:NLEV], rois, labels, pool)
    got = run_fwd(feat, g, rois, labels, S, pool, C).float().numpy()
    _assert_named_cases(feat, g, rois, labels, lv, pool, got)
    assert np.array_equal(got, want), int((got != want).sum())


def test_forward_without_labels_pools_every_slot():
    g = _geom()
    feat = _feat(64)
    rois, labels = _rois(37)
    rois = rois.reshape(-1, 4)
    want, _ = ref_fwd(feat, g, STRIDES[:NLEV], rois, np.zeros(rois.shape[0], np.int32), (7, 7))
    got = run_fwd(feat, g, rois, None, 37, (7, 7), 64).float().numpy()
    assert np.array_equal(got, want)


def _gout(R, nb, C, seed=3):
    return torch.randn((R, nb * C), generator=torch.Generator().manual_seed(seed)).to(BF).view(R, nb, C)


@pytest.mark.parametrize("pool,S,C,accumulate", [((7, 7), 512, 256, False), ((7, 7), 37, 64, True), ((3, 5), 37, 256, False),
                                                 ((14, 14), 37, 64, False), ((3, 5), 512, 64, True)])
def test_backward_against_first_maximum_reference(pool, S, C, accumulate):
    """The forward's inputs (every named case among them); with `accumulate` on a pre-filled gradient pyramid.  Run twice: equal bits."""
    g = _geom()
    feat = _feat(C)
    rois, labels = _rois(S)
    rois, labels = rois.reshape(-1, 4), labels.reshape(-1)
    gout = _gout(rois.shape[0], pool[0] * pool[1], C)
    prior = torch.randn((g.pixels, C), generator=torch.Generator().manual_seed(4)).to(BF) if accumulate else None
    ref, mag, cnt = ref_bwd(feat, g, STRIDES[:NLEV], rois, labels, pool, gout)
    assert cnt.max() > 1 and (cnt == 0).any()
    assert cnt.reshape(N, g.pix_per_img, C)[:, g.off[NLEV]:].max() == 0            # nothing lands on P6
    got = run_bwd(feat, g, rois, labels, S, pool, C, gout, prior)
    check_bwd(got, ref, mag, cnt, prior)
    again = run_bwd(feat, g, rois, labels, S, pool, C, gout, prior)
    assert torch.equal(U.bits_of(got), U.bits_of(again))


def test_backward_512_identical_rois_meet_on_each_pixel():
    S, C, pool = 512, 64, (7, 7)
    g = _geom()
    feat = _feat(C)
    rois = np.zeros((N, S, 4), np.float32)
    rois[0, :] = (100.0, 100.0, 300.0, 260.0)
    rois[1, :] = (10.0, 10.0, 50.0, 40.0)
    labels = np.ones((N, S), np.int32)
    labels[1] = -1
    rois, labels = rois.reshape(-1, 4), labels.reshape(-1)
    gout = _gout(N * S, 49, C, seed=5)
    ref, mag, cnt = ref_bwd(feat, g, STRIDES[:NLEV], rois, labels, pool, gout)
    assert cnt.max() >= 512 and cnt.reshape(N, -1)[1].max() == 0
    got = run_bwd(feat, g, rois, labels, S, pool, C, gout)
    check_bwd(got, ref, mag, cnt)
    assert torch.equal(U.bits_of(got), U.bits_of(run_bwd(feat, g, rois, labels, S, pool, C, gout)))


@pytest.mark.parametrize("pool", [(7, 7), (3, 5)])
def test_backward_constant_patch_goes_to_first_pixel_of_each_window(pool):
    """Every pixel of every window ties: the whole gradient lands on the window's first pixel (row-major), as the forward chose it."""
    C, S = 64, 1
    g = _geom()
    feat = _feat(C)
    rois = np.array([NAMED[CONSTANT], NAMED[CONSTANT]], np.float32)
    labels = np.array([-1, 1], np.int32)            # image 1 holds the constant patch
    nb = pool[0] * pool[1]
    gout = torch.ones((2, nb, C), dtype=BF)
    got = run_bwd(feat, g, rois, labels, S, pool, C, gout).float().numpy().reshape(N, g.pix_per_img, C)
    H, W = LEVELS[0]
    want = np.zeros((H, W), np.float32)
    for hs, he, ws, we in _windows(rois[1], 4, H, W, *pool):
        want[hs, ws] += 1.0
    assert want.sum() == nb
    assert not got[0].any() and not got[1, H * W:].any()
    assert np.array_equal(got[1, :H * W].reshape(H, W, C), np.broadcast_to(want[:, :, None], (H, W, C)))


@pytest.mark.parametrize("fill", ["nan", "max"])
def test_guard_bands(fill):
    """Both launches on guarded tensors at a gapped geometry (tests/util.py): the guards and the gap rows of the inputs hold `fill`, those of
    the outputs the sentinel; no byte outside the tensors changes, the inputs come back bit for bit, every owned output row is written and
    the results equal those of the dense layout."""
    ops = _ops()
    C, S, pool = 64, 24, (3, 5)
    levels = [(33, 41), (17, 21), (9, 11), (5, 6), (3, 3)]
    gg, kind = U.gapped_geom(N, levels)
    gd = _geom(levels)
    gen = torch.Generator().manual_seed(8)
    dense = torch.randn((gd.pixels, C), generator=gen).to(BF)
    rng = np.random.default_rng(9)
    rois = np.zeros((N * S, 4), np.float32)
    for i in range(N * S):
        s = rng.uniform(4, 230)
        x1, y1 = rng.uniform(0, 150), rng.uniform(0, 120)          # a 132 x 164 image: many boxes reach past its edges
        rois[i] = (x1, y1, x1 + s * rng.uniform(0.7, 1.4), y1 + s)
    rois[0] = (160.0, 128.0, 400.0, 300.0)                          # starts on the last row / column
    rois[1] = (900.0, 900.0, 1000.0, 1000.0)                        # outside
    labels = rng.integers(0, 3, N * S).astype(np.int32)
    labels[5] = -1
    gout = _gout(N * S, pool[0] * pool[1], C, seed=10)

    def scatter(t):            # dense rows -> rows of the gapped layout
        full = torch.zeros((gg.pixels, C), dtype=t.dtype)
        for n in range(N):
            for l, (h, w) in enumerate(levels):
                full[n * gg.pix_per_img + gg.off[l]: n * gg.pix_per_img + gg.off[l] + h * w] = t[n * gd.pix_per_img + gd.off[l]: n * gd.pix_per_img + gd.off[l] + h * w]
        return full

    want_out = torch.empty((N * S, pool[0] * pool[1] * C), dtype=BF, device="cuda")
    ops.roi_pool_fwd(dense.cuda(), gd, NLEV, STRIDES, C, torch.from_numpy(rois).cuda(), torch.from_numpy(labels).cuda(), S, pool, want_out)
    want_g = torch.empty((gd.pixels, C), dtype=BF, device="cuda")
    ops.roi_pool_bwd_bf16(dense.cuda(), gout.cuda(), gd, NLEV, STRIDES, C, torch.from_numpy(rois).cuda(), torch.from_numpy(labels).cuda(), S, pool,
                          want_g, torch.empty((ops.roi_pool_bwd_bf16_workspace_bytes(gd, S),), dtype=torch.uint8, device="cuda"))

    ins = []

    def inp(name, data, gaps=False):
        data = data.view(data.shape[0], -1)
        t, h = U.guarded(data.shape[0], data.shape[1], data.dtype, "cuda", fill=fill, name=name)
        h.set(data)
        if gaps:
            h.set_gaps(kind)
        ins.append(h.snapshot())
        return t

    feat_t = inp("feat", scatter(dense), gaps=True)
    rois_t = inp("rois", torch.from_numpy(rois))
    labels_t = inp("labels", torch.from_numpy(labels).view(torch.float32).view(-1, 1)).view(-1).view(torch.int32)     # (the fills are float patterns)
    gout_t = inp("gout", gout)
    out_t, out_h = U.guarded(N * S, pool[0] * pool[1] * C, BF, "cuda", name="out")
    gf_t, gf_h = U.guarded(gg.pixels, C, BF, "cuda", name="gfeat")
    gf_h.set_gaps(kind)
    nws = ops.roi_pool_bwd_bf16_workspace_bytes(gg, S)
    ws_t, ws_h = U.guarded(nws, None, torch.uint8, "cuda", name="ws")
    ops.roi_pool_fwd(feat_t, gg, NLEV, STRIDES, C, rois_t, labels_t, S, pool, out_t)
    ops.roi_pool_bwd_bf16(feat_t, gout_t, gg, NLEV, STRIDES, C, rois_t, labels_t, S, pool, gf_t, ws_t)
    torch.cuda.synchronize()
    for h in ins:
        h.assert_unchanged()
    for h in (out_h, gf_h, ws_h):
        h.check()
    assert torch.equal(U.bits_of(out_t), U.bits_of(want_out))
    owned = (kind == 0).cuda()
    assert U.count_sentinel(gf_t[owned]) == 0
    assert torch.equal(U.bits_of(gf_t[owned]), U.bits_of(scatter(want_g.cpu()).cuda()[owned]))
