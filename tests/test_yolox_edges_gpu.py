"""The YOLOX kernels where the other YOLOX tests do not reach: past the grid caps of the element-wise launches, in the second trip of the
batch-norm reductions, on exact cost ties of the SimOTA assignment, on the kinks of the IoU loss, at grad_scale != 1 and at the widths
and depth of the default model (YOLOXConfig: depth 1, width 1, batch 8, multi-scale up to 832 x 832).

Every test asserts the precondition that makes it what it is (a vector count above a cap, a row count above one trip), with the
kernel's constant named beside it: a later change of a cap fails the test instead of moving it back below the threshold.  The large
operands are compared on the device; only verdicts and per-channel vectors come to the host.

  A  yx_loss_kernel / yx_loss_finalize_kernel at 1 159 200 vectors (cap: 4096 workgroups x 256 threads), against O.losses;
  B  grad_scale 0.5 / 2 (bits of the scaled grad_scale = 1 run) and 1/3 (the oracle's gradients / 3);
  C  O.kink_problem(): min / max ties, disjoint and enclosing gts, labels outside 1..K, matched = Gmax, a zero-area gt under use_l1;
  D  O.tie_problem(): exact cost ties inside yx_gt_kernel, across its 1024-point chunks -- matched equals the oracle, no excuses;
  E  cat2_fwd_kernel / cat2_bwd_kernel above 16384 workgroups x 256 threads (Focus is left out: its launch has the same cap, which needs
     16.7 M output pixels, an input no configuration reaches);
  F  bn_stats_final_kernel / bn_bwd_final_kernel above 128 slots x 128 rows, with the apply passes that consume their results;
  G  SPPBottleneck, CSPLayer and Focus at the default model's channel counts and depth, on tiny planes."""
import functools
import math

import numpy as np
import pytest
import torch

import test_yolox_blocks_gpu as TB
import test_yolox_gpu as TY
import util as U
import yolox_blocks_oracle as BO
import yolox_oracle as O
from basedet_amd import ops
from util import bf16_ulps, bits_of, gapped_geom, guarded

pytestmark = pytest.mark.gpu
BF, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8
DEV = "cuda"
NF = TY.NF
YX_LOSS_TRIP = 4096 * 256            # yolox.hip: YX_GRID_CAP workgroups of 256 threads, one 8-slot vector per thread and trip
CAT2_TRIP = 16384 * 256              # yolox_neck.hip: grid_for(total, 256, 16384), one 16-byte vector per thread and trip
BN_TRIP = 128 * 128                  # batchnorm.hip: BN_FL slot lanes of BN_SLOT rows each


# ---- the loss ------------------------------------------------------------------------------------------------------------------------------
def _loss(prob, matched, iou_t, nf, use_l1, grad_scale=1.0):
    """tests/test_yolox_gpu.py's _loss with a grad_scale: (loss4 on the host, d_cls (N, P, ld), d_box_obj (N, P, 8) on the device)."""
    N, P = prob["cls"].shape[:2]
    K = prob["K"]
    t, hs = TY._operands(prob)
    mt, hm = TY._in(torch.from_numpy(matched.astype(np.int32)).reshape(-1), "matched", fill="zero")
    ut, hu = TY._in(torch.from_numpy(iou_t.astype(np.float32)).reshape(-1), "iou_t")
    st, hst = TY._in(torch.tensor([float(nf)]), "stats")
    outs = [TY._out(4, None, F32, "loss_out"), TY._out(N * P, t["cls"].shape[1], BF, "d_cls"), TY._out(N * P, 8, BF, "d_box_obj")]
    (loss, _), (d_cls, _), (d_box, _) = outs
    ws = torch.empty(ops.yolox_loss_workspace_bytes(), dtype=U8, device=DEV)
    TY._twice(lambda: ops.yolox_loss_fwd_bwd_into(t["cls"], K, t["box_obj"], t["points"], prob["lvl_start"], prob["strides"], t["gt"],
                                                  mt.view(N, P), ut.view(N, P), st, use_l1, grad_scale, loss, d_cls, d_box, ws),
              outs, hs[:4] + [hm, hu, hst])
    return loss.cpu().numpy(), d_cls.view(N, P, -1), d_box.view(N, P, 8)


def _far(got, ref, rtol=3e-2, atol=2e-6):
    """Elements of a device tensor outside np.allclose's |got - ref| <= atol + rtol |ref| of a float64 host reference (counted on the
    device; a NaN counts)."""
    r = torch.from_numpy(np.ascontiguousarray(ref)).to(got.device)
    return int((~((got.double() - r).abs() <= atol + rtol * r.abs())).sum())


def _check_losses(loss, ref_loss, use_l1, what):
    for j, name in enumerate(("iou", "obj", "cls", "l1")):
        if name == "l1" and not use_l1:
            assert loss[j] == 0
            continue
        rel = abs(float(loss[j]) - ref_loss[j]) / abs(ref_loss[j])
        print(f"loss {what} l1={use_l1} {name}: {loss[j]:.6f} vs {ref_loss[j]:.6f}, rel err 2^{math.log2(max(rel, 1e-30)):.1f}")
        assert rel <= 2.0 ** -16, (name, float(loss[j]), ref_loss[j])


def _check_zeros(d_cls, d_box, matched, K, Gmax):
    """Exactly +0: background rows of d_cls and of the box gradient, pad columns, slots 5-7 of d_box_obj."""
    bg = torch.from_numpy((matched < 0) | (matched >= Gmax)).to(DEV)
    assert int((bits_of(d_cls)[bg] != 0).sum()) == 0
    assert int((bits_of(d_cls)[..., K:] != 0).sum()) == 0 and int((bits_of(d_box)[..., 5:] != 0).sum()) == 0
    assert int((bits_of(d_box)[bg][:, :4] != 0).sum()) == 0


@functools.lru_cache(maxsize=None)
def _big_reference(use_l1):
    prob, m, u = O.big_loss_problem()
    return O.losses(prob, m, u, NF, use_l1)


@pytest.mark.parametrize("use_l1", [False, True])
def test_loss_past_the_grid_cap(use_l1):
    """(3, 640 x 640, K = 365): 1 159 200 vectors, so 110 624 threads take a second vector (the accumulators carry over, the `continue` of
    the vectors with c0 != 0 runs inside a loop that repeats) and the finalize kernel walks all 4096 partial rows, 16 per thread.  The
    bounds of tests/test_yolox_gpu.py hold unchanged.  Every term of the four sums is >= 0, so sum |terms| is the loss itself and the
    worst case of the fp32 chain is (2 x 8 adds per thread + 8 in the block tree + 16 + 8 in the finalize) 2^-24 = 2^-18.4 relative,
    inside the 2^-16 asserted; the measured share of it is printed."""
    prob, m, u = O.big_loss_problem()
    N, P, ld = prob["cls"].shape
    K, Gmax = prob["K"], prob["gt"].shape[1]
    nvec = N * P * ld // 8
    assert nvec > YX_LOSS_TRIP and nvec <= 2 * YX_LOSS_TRIP
    ref_loss, ref_dc, ref_db = _big_reference(use_l1)
    loss, d_cls, d_box = _loss(prob, m, u, NF, use_l1)
    _check_losses(loss, ref_loss, use_l1, O.BIG_SHAPE)
    chain = (2 * 8 + 8 + 16 + 8) * 2.0 ** -24
    print("rel err / fp32 chain bound:", [f"{abs(float(loss[j]) - ref_loss[j]) / ref_loss[j] / chain:.3f}" for j in range(4) if ref_loss[j]])
    assert _far(d_cls[..., :K], ref_dc) == 0
    assert _far(d_box[..., :5], ref_db) == 0
    _check_zeros(d_cls, d_box, m, K, Gmax)
    assert int((bits_of(d_cls) != 0).any(-1).sum()) == int((m >= 0).sum())          # every foreground row was written, in both trips


def test_grad_scale():
    """The 96 x 160 shared problem with use_l1.  grad_scale = 0.5 and 2: the four losses keep the bits of the grad_scale = 1 run, and every
    gradient is the bf16 rounding of the scaled fp32 value -- a power of two commutes with both roundings, so the bits equal the scaled
    grad_scale = 1 result wherever neither is subnormal or overflows (at least 99 % of the non-zero elements).  grad_scale = 1/3: the
    oracle's gradients / 3 at the tolerance of test_loss."""
    shape = O.SHAPES[1]
    prob = O.problem(shape)
    K = prob["K"]
    m_o, u_o, _ = O.reference(shape)
    ref_loss, ref_dc, ref_db = O.losses(prob, m_o, u_o, NF, True)
    loss1, dc1, db1 = _loss(prob, m_o, u_o, NF, True, 1.0)
    tiny, big = 2.0 ** -126, float(torch.finfo(BF).max)
    for s in (0.5, 2.0):
        loss, dc, db = _loss(prob, m_o, u_o, NF, True, s)
        assert np.array_equal(loss.view(np.uint32), loss1.view(np.uint32)), (s, loss, loss1)
        for got, one, name in ((dc, dc1, "d_cls"), (db, db1, "d_box_obj")):
            x1 = one.float()
            xs = x1 * s
            nz = x1 != 0
            ok = nz & (x1.abs() >= tiny) & (xs.abs() >= tiny) & (xs.abs() <= big)
            share = float(ok.sum()) / float(nz.sum())
            print(f"grad_scale {s} {name}: {int(nz.sum())} non-zero elements, {share:.4f} of them comparable")
            assert share >= 0.99
            assert torch.equal(bits_of(got)[ok], bits_of(xs.to(BF))[ok]), (s, name)
            assert int((bits_of(got)[~nz] != 0).sum()) == 0
    loss, dc, db = _loss(prob, m_o, u_o, NF, True, 1.0 / 3.0)
    assert np.array_equal(loss.view(np.uint32), loss1.view(np.uint32))
    assert _far(dc[..., :K], ref_dc / 3) == 0 and _far(db[..., :5], ref_db / 3) == 0
    assert _far(dc1[..., :K], ref_dc) == 0 and _far(db1[..., :5], ref_db) == 0


@pytest.mark.parametrize("use_l1", [False, True])
def test_loss_kinks(use_l1):
    """O.kink_problem() against O.losses, whose torch float64 autograd defines the rules the kernel states: half the gradient to each
    side of a min / max tie (a wrong weight is a factor of two, or a non-zero gradient where prediction = gt has none), no box gradient
    from a disjoint gt, background terms in every class column of a label outside 1..K, matched = Gmax as background.

    One pair of elements is not decided by the float64 statement: under use_l1 the point `equal` has raw w = h = 0 and a gt as wide as
    the stride, so its L1 target is log(1 + 1e-8), which is 0 in fp32 and 1e-8 in float64 -- |raw - target| sits on the kink of |x| in
    one and beside it in the other.  There the L1 term may contribute any subgradient, [-1, 1] / nf; the IoU term is still compared."""
    prob = O.kink_problem()
    m, u, cases = prob["matched"], prob["iou_t"], prob["cases"]
    K, Gmax = prob["K"], prob["gt"].shape[1]
    ref_loss, ref_dc, ref_db = O.losses(prob, m, u, NF, use_l1)
    loss, d_cls, d_box = _loss(prob, m, u, NF, use_l1)
    _check_losses(loss, ref_loss, use_l1, "kinks")
    got_dc, got_db = d_cls[..., :K].float().cpu().numpy(), d_box[..., :5].float().cpu().numpy()
    for name, p in cases.items():
        print(f"{name:10s} d_box got {got_db[0, p]} ref {ref_db[0, p]}")
    assert np.allclose(got_dc, ref_dc, rtol=3e-2, atol=2e-6)
    free = np.zeros(ref_db.shape, bool)
    if use_l1:
        free[0, cases["equal"], 2:4] = True
        iou_only = O.losses(prob, m, u, NF, False)[2]
        assert np.all(np.abs(got_db[free] - iou_only[free]) <= 1.0 / NF + 2e-6)
    assert np.allclose(got_db[~free], ref_db[~free], rtol=3e-2, atol=2e-6)
    _check_zeros(d_cls, d_box, m, K, Gmax)
    assert m[0, prob["bg_gmax"]] == Gmax and np.abs(ref_db[0, cases["edge_x1"], :4]).max() > 1e-3


# ---- the assignment ------------------------------------------------------------------------------------------------------------------------
def test_assign_ties():
    """O.tie_problem(): only exact ties decide (tests/test_yolox_cpu.py shows it), so the rule both sides state -- lowest point index,
    then lowest gt index -- must give the oracle's matched with no differing point; O.compare's excuses are not consulted.  gt 1 of
    image 0 needs the carry of the tie rank from the first 1024-point chunk into the second: without it, or with one tie too many
    taken, point 1058 becomes foreground."""
    prob = O.tie_problem()
    P = prob["pts"].shape[0]
    assert 1024 < P <= 2048                                              # yx_gt_kernel: two trips of its 1024-thread workgroup
    m_o, u_o, _ = O.assign(prob)
    m, u, nfg = TY._assign(prob)
    diff = np.argwhere(m != m_o)
    print("assign ties: foreground", np.argwhere(m >= 0).tolist(), "differing", diff.tolist())
    assert diff.shape[0] == 0
    assert nfg == (m_o >= 0).sum() == 4 and m[0, 132] == 1 and m[0, 1058] == -1
    assert np.abs(u.astype(np.float64) - u_o).max() <= 2.0 ** -12 and (u[m < 0] == 0).all()


# ---- bd_cat2_fwd / bd_cat2_bwd -------------------------------------------------------------------------------------------------------------
def _bf16_step(ref):
    """yolox_blocks_oracle.bf16_step on a float64 device tensor."""
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)


def _cat2_big(N, H, W, Ca, Cb, up, seed):
    """tests/test_yolox_blocks_gpu.py's _cat2_case with every operand and every comparison on the device."""
    M = N * H * W
    Ma = M // 4 if up else M
    assert M * (Ca + Cb) // 8 > CAT2_TRIP and Ma * (Ca // 8) + M * (Cb // 8) > CAT2_TRIP
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda r, c: torch.randn(r, c, generator=g, device=DEV).to(BF)
    a, b, grad, old_a, old_b = rnd(Ma, Ca), rnd(M, Cb), rnd(M, Ca + Cb), rnd(Ma, Ca), rnd(M, Cb)
    ab, ah = TB._in(a, "a")
    bb, bh = TB._in(b, "b", fill="max")
    gb, gh = TB._in(grad, "g")
    a_up = a.view(N, H // 2, W // 2, Ca).repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(M, Ca) if up else a
    want = torch.cat([a_up, b], 1)
    outs = []
    for _ in range(2):
        ob, oh = TB._out(M, Ca + Cb, "out")
        ops.cat2_fwd(ab, bb, M, Ca, Cb, ob, up, N, H, W)
        torch.cuda.synchronize()
        oh.check()
        outs.append(ob.clone())
    assert torch.equal(bits_of(outs[0]), bits_of(outs[1])) and torch.equal(bits_of(outs[0]), bits_of(want))
    del outs, want, a_up
    ga, gbb = grad[:, :Ca].float(), grad[:, Ca:].float()
    if up:
        g4 = ga.view(N, H // 2, 2, W // 2, 2, Ca)
        s32 = ((g4[:, :, 0, :, 0] + g4[:, :, 0, :, 1]) + g4[:, :, 1, :, 0]) + g4[:, :, 1, :, 1]
        s32, s64 = s32.reshape(Ma, Ca), g4.double().sum((2, 4)).reshape(Ma, Ca)
    else:
        s32, s64 = ga, ga.double()
    for acc_a, acc_b in TB.ACCS:
        res = []
        for _ in range(2):
            dab, dah = TB._out(Ma, Ca, "d_a")
            dbb, dbh = TB._out(M, Cb, "d_b")
            if acc_a:
                dab.copy_(old_a)
            if acc_b:
                dbb.copy_(old_b)
            ops.cat2_bwd(gb, M, Ca, Cb, dab, dbb, up, N, H, W, acc_a, acc_b)
            torch.cuda.synchronize()
            dah.check(), dbh.check()
            res.append((dab.clone(), dbb.clone()))
        assert torch.equal(bits_of(res[0][0]), bits_of(res[1][0])) and torch.equal(bits_of(res[0][1]), bits_of(res[1][1]))
        wa32 = (s32 + old_a.float()) if acc_a else s32
        wb32 = (gbb + old_b.float()) if acc_b else gbb
        assert torch.equal(bits_of(res[0][0]), bits_of(wa32.to(BF))), (acc_a, acc_b, "d_a")
        assert torch.equal(bits_of(res[0][1]), bits_of(wb32.to(BF))), (acc_a, acc_b, "d_b")
        wa64 = s64 + (old_a.double() if acc_a else 0.0)
        wb64 = gbb.double() + (old_b.double() if acc_b else 0.0)
        for got, ref in ((res[0][0], wa64), (res[0][1], wb64)):
            assert bool(((got.double() - ref).abs() <= _bf16_step(ref)).all())
        del res
    ah.assert_unchanged(), bh.assert_unchanged(), gh.assert_unchanged()


def test_cat2_past_the_grid_cap():
    """M = 2 x 482 x 128 rows of (8, 264) channels: 4 195 328 vectors, 1024 more than one trip of the capped grid, forward and backward
    (the four acc combinations).  Forward: the bits of torch.cat; backward: the fp32 restatement, and one bf16 step of float64."""
    _cat2_big(2, 482, 128, 8, 264, False, seed=1)


def test_cat2_upsample_past_the_grid_cap():
    """The same through the nearest upsample.  There the backward launch has M / 4 * Ca / 8 + M * Cb / 8 vectors, so the even-sized shape
    is 2 x 496 x 128: 4 221 952 vectors backward, 4 317 184 forward."""
    _cat2_big(2, 496, 128, 8, 264, True, seed=2)


# ---- batch norm: the second stage of the reductions in more than one trip ---------------------------------------------------------------
EPS, MOM = 1e-5, 0.1
BN_ROWS = [(1, 16385), (1, 128 * 257 + 77), (5, 26221)]


def _bn_data(M, C, seed, silu):
    """y, g (M, C) bf16 on the device and gamma, beta, running statistics (fp32, host), as the _inputs of tests/test_batchnorm_gpu.py
    (silu False: channel 0 mean 100 sigma, 1 constant, 2 all zero, gamma of both signs) and of tests/test_yolox_head_gpu.py (silu True:
    channel 0 and 1 as before, gamma[2] = 0, channel 3 with u spread over +-100, |gamma| log-uniform in [0.1, 60], every 7th row of g
    zero); the other channels are the ordinary normal sample with a random scale and offset."""
    rng = np.random.default_rng(seed)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(DEV)
    y = torch.randn(M, C, generator=gen, device=DEV) * f(rng.uniform(0.2, 3.0, C)) + f(rng.uniform(-2.0, 2.0, C))
    y[:, 0] = 100.0 + torch.randn(M, generator=gen, device=DEV)
    y[:, 1] = 3.25
    g = torch.randn(M, C, generator=gen, device=DEV) * 0.1 + f(rng.uniform(-0.05, 0.05, C))
    if silu:
        g[::7] = 0.0
        gamma = (0.1 * 600.0 ** rng.random(C) * np.where(rng.random(C) < 0.5, -1.0, 1.0)).astype(np.float32)
        gamma[:4] = [1.5, -0.75, 0.0, 40.0]
        beta = rng.uniform(-3.0, 3.0, C).astype(np.float32)
        beta[3] = 0.0
    else:
        y[:, 2] = 0.0
        gamma = rng.standard_normal(C).astype(np.float32)
        gamma[:4] = [1.5, -0.75, 0.5, -1.25]
        beta = rng.standard_normal(C).astype(np.float32)
    rm0, rv0 = rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2.0, C).astype(np.float32)
    rm0[2] = 0.0
    return y.to(BF), g.to(BF), gamma, beta, rm0, rv0


def _bn_buffers(N, n, C, y, g):
    """Guarded operands of one case: (geometry of the level, {name: (tensor, handle)}, rows of the level in the buffers).  N = 1: dense.
    N > 1: the second of two levels per image in gapped buffers (off != 0, pix_per_img > n), so image boundaries fall inside the 128-row
    slots and every row address goes through pix_per_img / off."""
    M = N * n
    if N == 1:
        geo, rows, pixels, kind = ops.single(1, 1, M), None, M, None
    else:
        h = next(d for d in range(2, 200) if n % d == 0)
        geom, kind = gapped_geom(N, [(3, 5), (h, n // h)], gap=64)
        geo, pixels = geom.level(1), geom.pixels
        rows = (torch.arange(N).view(-1, 1) * geom.pix_per_img + geom.off[1] + torch.arange(n).view(1, -1)).view(-1).to(DEV)
        assert geom.off[1] > 0 and geom.pix_per_img > n and n % 128 != 0
    bufs = {}
    for name, fill, data in (("y", "nan", y), ("g", "max", g), ("z", "sentinel", None), ("gy", "sentinel", None)):
        t, hd = guarded(pixels, C, BF, DEV, fill=fill, name=name)
        if data is not None:
            if rows is None:
                hd.set(data)
            else:
                t[rows] = data
        if kind is not None:
            hd.set_gaps(kind)
        if data is not None:
            hd.snapshot()
        bufs[name] = (t, hd)
    return geo, bufs, rows


def _rows_of(t, rows):
    return t if rows is None else t[rows]


def _check_untouched(bufs, rows):
    bufs["y"][1].assert_unchanged(), bufs["g"][1].assert_unchanged()
    for name in ("z", "gy"):
        t, hd = bufs[name]
        hd.check()
        if rows is not None:                                              # the rows of the other level keep the sentinel
            other = torch.ones(t.shape[0], dtype=torch.bool, device=DEV)
            other[rows] = False
            other &= (hd.kind == 0)
            assert U.count_sentinel(t[other]) == int(other.sum()) * t.shape[1], name


def _plain_chain(N, n, C, seed):
    """bd_bn_stats_fwd -> bd_bn_apply_act_fwd -> bd_bn_bwd_reduce -> bd_bn_bwd_apply with the bounds of tests/test_batchnorm_gpu.py's
    _check, evaluated in float64 on the device."""
    M = N * n
    y, g, gamma, beta, rm0, rv0 = _bn_data(M, C, seed, False)
    geo, bufs, rows = _bn_buffers(N, n, C, y, g)
    f = lambda: torch.empty(C, dtype=F32, device=DEV)
    d = lambda a: torch.from_numpy(np.asarray(a)).to(DEV)
    ws = torch.empty(ops.bn_workspace_bytes(M, C) // 4 + 16, dtype=F32, device=DEV)
    runs = []
    for _ in range(2):
        o = dict(mean=f(), inv_std=f(), sums=torch.empty((3, C), dtype=F32, device=DEV), rm=d(rm0), rv=d(rv0), dgamma=f(), dbeta=f())
        yb, gb, zb, ob = (bufs[k][0] for k in ("y", "g", "z", "gy"))
        ops.bn_stats_fwd(yb, geo, C, EPS, MOM, o["mean"], o["inv_std"], o["sums"], o["rm"], o["rv"], ws)
        ops.bn_apply_act_fwd(yb, geo, o["mean"], o["inv_std"], d(gamma), d(beta), zb, geo, C, relu=False)
        ops.bn_bwd_reduce(gb, geo, yb, geo, o["mean"], o["inv_std"], C, o["dgamma"], o["dbeta"], ws)
        ops.bn_bwd_apply(gb, geo, yb, geo, o["mean"], o["inv_std"], d(gamma), o["dgamma"], o["dbeta"], o["sums"][0], ob, geo, C)
        torch.cuda.synchronize()
        runs.append(dict(o, z=_rows_of(zb, rows).clone(), gout=_rows_of(ob, rows).clone()))
    _check_untouched(bufs, rows)
    for k in runs[0]:
        assert torch.equal(bits_of(runs[0][k]), bits_of(runs[1][k])), k
    o = runs[0]
    y64, g64 = y.double(), g.double()
    mu, var = y64.mean(0), y64.var(0, unbiased=False)
    sig = var.sqrt()
    mean, inv_std = o["mean"].double(), o["inv_std"].double()
    em = float(((mean - mu).abs() / (mu.abs() + sig + 1e-300)).max())
    assert bool(((mean - mu).abs() <= 1e-5 * (mu.abs() + sig)).all()), em
    got_var = 1.0 / inv_std ** 2 - EPS
    live = var > 0
    assert int(live.sum()) == C - 2 and not bool(live[1]) and not bool(live[2])
    rel = (got_var[live] - var[live]).abs() / var[live]
    print(f"bn M={M} C={C}: mean err / (|mu| + sigma) {em:.2e}; rel var err {float(rel.max()):.2e}, on the mean-100-sigma channel "
          f"{float(abs(got_var[0] - var[0]) / var[0]):.2e}")
    assert bool((rel <= 1e-4).all())
    want = np.float32(1.0) / np.sqrt(np.float32(EPS))
    assert bool((o["inv_std"][~live] == float(want)).all())
    sums = o["sums"].double()
    sq = (y64 ** 2).sum(0)
    assert bool((sums[0] == M).all())
    assert bool(((sums[1] - mu * M).abs() <= 1e-5 * (mu.abs() + sig) * M).all())
    assert bool(((sums[2] - sq).abs() <= 1e-5 * sq).all())
    rm_ref = (1 - MOM) * d(rm0).double() + MOM * mu
    rv_ref = (1 - MOM) * d(rv0).double() + MOM * var * M / max(M - 1, 1)
    assert bool(((o["rm"].double() - rm_ref).abs() <= 1e-5 * (mu.abs() + sig)).all())
    assert bool(((o["rv"].double() - rv_ref).abs() <= 1e-4 * rv_ref).all())
    gam, bet = d(gamma).double(), d(beta).double()
    xh = (y64 - mean) * inv_std
    assert int(bf16_ulps(o["z"], gam * xh + bet).max()) <= 1
    dg, db = o["dgamma"].double(), o["dbeta"].double()
    tg = g64 * xh
    eg = float(((dg - tg.sum(0)).abs() / (tg.abs().sum(0) + 1e-300)).max())
    eb = float(((db - g64.sum(0)).abs() / (g64.abs().sum(0) + 1e-300)).max())
    print(f"bn M={M} C={C}: dgamma err / sum|terms| {eg:.2e}, dbeta {eb:.2e}")
    assert bool(((dg - tg.sum(0)).abs() <= 1e-5 * tg.abs().sum(0)).all())
    assert bool(((db - g64.sum(0)).abs() <= 1e-5 * g64.abs().sum(0)).all())
    assert int(bf16_ulps(o["gout"], gam * inv_std * (g64 - db / M - xh * dg / M)).max()) <= 1


def _silu_chain(N, n, C, seed):
    """bd_bn_stats_fwd -> bd_bn_silu_fwd -> bd_bn_silu_bwd_reduce -> bd_bn_silu_bwd_apply with the bounds of
    tests/test_yolox_head_gpu.py's _check, evaluated in float64 on the device."""
    M = N * n
    y, g, gamma, beta, _, _ = _bn_data(M, C, seed, True)
    geo, bufs, rows = _bn_buffers(N, n, C, y, g)
    f = lambda: torch.empty(C, dtype=F32, device=DEV)
    d = lambda a: torch.from_numpy(np.asarray(a)).to(DEV)
    ws = torch.empty(ops.bn_workspace_bytes(M, C) // 4 + 16, dtype=F32, device=DEV)
    runs = []
    for _ in range(2):
        o = dict(mean=f(), inv_std=f(), sums=torch.empty((3, C), dtype=F32, device=DEV), dgamma=f(), dbeta=f())
        yb, gb, zb, ob = (bufs[k][0] for k in ("y", "g", "z", "gy"))
        ops.bn_stats_fwd(yb, geo, C, EPS, MOM, o["mean"], o["inv_std"], o["sums"], None, None, ws)
        ops.bn_silu_fwd(yb, geo, o["mean"], o["inv_std"], d(gamma), d(beta), zb, geo, C)
        ops.bn_silu_bwd_reduce(gb, geo, yb, geo, o["mean"], o["inv_std"], d(gamma), d(beta), C, o["dgamma"], o["dbeta"], ws)
        ops.bn_silu_bwd_apply(gb, geo, yb, geo, o["mean"], o["inv_std"], d(gamma), d(beta), o["dgamma"], o["dbeta"], o["sums"][0], ob, geo, C)
        torch.cuda.synchronize()
        runs.append(dict(o, z=_rows_of(zb, rows).clone(), gout=_rows_of(ob, rows).clone()))
    _check_untouched(bufs, rows)
    for k in runs[0]:
        assert torch.equal(bits_of(runs[0][k]), bits_of(runs[1][k])), k
    o = runs[0]
    y64, g64 = y.double(), g.double()
    mean, inv_std, gam, bet = o["mean"].double(), o["inv_std"].double(), d(gamma).double(), d(beta).double()
    xh = (y64 - mean) * inv_std
    u = gam * xh + bet
    assert float(u.max()) > 80 and float(u.min()) < -80, "the inputs are meant to spread u over +-100"
    e = torch.exp(-u.abs())
    inv = 1.0 / (1.0 + e)
    s, sm = torch.where(u >= 0, inv, e * inv), torch.where(u >= 0, e * inv, inv)
    dz = bf16_ulps(o["z"], u * s)
    gu = g64 * (s * (1.0 + u * sm))
    dg, db = o["dgamma"].double(), o["dbeta"].double()
    dgy = bf16_ulps(o["gout"], gam * inv_std * (gu - db / M - xh * dg / M))
    tg = gu * xh
    eg = float(((dg - tg.sum(0)).abs() / (tg.abs().sum(0) + 1e-300)).max())
    eb = float(((db - gu.sum(0)).abs() / (gu.abs().sum(0) + 1e-300)).max())
    print(f"bn silu M={M} C={C}: z max {int(dz.max())} ulp, gy max {int(dgy.max())} ulp; dgamma err / sum|terms| {eg:.2e}, dbeta {eb:.2e}")
    assert int(dz.max()) <= 1 and int(dgy.max()) <= 1
    assert bool(((dg - tg.sum(0)).abs() <= 1e-5 * tg.abs().sum(0)).all())
    assert bool(((db - gu.sum(0)).abs() <= 1e-5 * gu.abs().sum(0)).all())


@pytest.mark.parametrize("C", [8, 264])
@pytest.mark.parametrize("N,n", BN_ROWS)
def test_bn_reductions_past_one_trip(N, n, C):
    """bn_stats_final_kernel and bn_bwd_final_kernel give each of their 128 lanes the slots lane, lane + 128, ...: a second trip starts at
    16 385 rows.  M = 16 385 (slot 128 holds one row), 128 x 257 + 77 (three trips, a ragged last slot) and 131 072 + 33 (nine trips)
    at C = 8 and C = 264, on the statistics, both backward reductions (plain and SiLU) and the apply passes that read their results; the
    bounds are those of tests/test_batchnorm_gpu.py and tests/test_yolox_head_gpu.py, none of which depends on the row count.
    131 105 = 5 x 13 x 2017 has no factor 3, so that case runs as N = 5 images of 26 221 rows each inside gapped two-level buffers.

    Where the rest of the suite stands: the unit tests of these entry points stop at 3150 rows; the ResNet families
    (tests/test_backbone_norm_gpu.py, tests/test_fpn_norm_gpu.py, tests/test_live_norm_families_gpu.py) all run at 2 x 128 x 160, whose
    largest normalised tensor is the stem's 2 x 64 x 80 = 10 240 rows; the YOLOX model tests stay under 8000.  None passes 16 384."""
    M = N * n
    assert M > BN_TRIP and -(-M // 128) > 128 and M in (16385, 32973, 131105)
    _plain_chain(N, n, C, seed=M + C)
    _silu_chain(N, n, C, seed=M + C + 1)


def test_bn_stats_refuses_2_to_the_24_rows():
    """N * n = 2^24 rows (the fp32 row count stops being exact) is refused before any launch: BD_EINVAL, the outputs keep their sentinel.
    Nothing is read, so the allocation behind y is small."""
    from basedet_amd._lib import BasedetHipError
    C = 8
    geo = ops.Geom(4096, [64], [64])
    assert geo.N * geo.H[0] * geo.W[0] == 1 << 24
    y = torch.zeros((64, C), dtype=BF, device=DEV)
    outs = [guarded(C, None, F32, DEV, name=k) for k in ("mean", "inv_std", "running_mean", "running_var")]
    sums, sh = guarded(3, C, F32, DEV, name="sums")
    ws = torch.zeros(1024, dtype=F32, device=DEV)
    with pytest.raises(BasedetHipError) as e:
        ops.bn_stats_fwd(y, geo, C, EPS, MOM, outs[0][0], outs[1][0], sums, outs[2][0], outs[3][0], ws)
    assert "(code -1)" in str(e.value) and "2^24" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for t, h in outs + [(sums, sh)]:
        h.check()
        assert U.count_sentinel(t) == t.numel()
    ok = ops.Geom(4095, [64], [64])                                      # one image fewer passes the row check (and fails on the workspace)
    with pytest.raises(BasedetHipError) as e:
        ops.bn_stats_fwd(y, ok, C, EPS, MOM, outs[0][0], outs[1][0], sums, outs[2][0], outs[3][0], ws)
    assert "(code -3)" in str(e.value), str(e.value)


# ---- the default model's blocks on tiny planes -------------------------------------------------------------------------------------------
def test_spp_bottleneck_at_the_default_width():
    """SPPBottleneck(1024, 1024): 512 hidden channels, a 2048-channel concatenation."""
    import basedet.layers as BL
    TB._block_case(lambda: BL.SPPBottleneck(1024, 1024), BO.spp_bottleneck, 2, 1024, 3, 5, seed=21)


def test_csp_layer_of_dark5_at_the_default_width():
    """CSPLayer(1024, 1024, n=3, shortcut=False), dark5's."""
    import basedet.layers as BL
    layer = TB._block_case(lambda: BL.CSPLayer(1024, 1024, 3, False), BO.csp_layer, 2, 1024, 2, 3, seed=22, n=3, shortcut=False)
    assert len(layer.m) == 3


def test_csp_layer_of_dark3_at_the_default_depth():
    """CSPLayer(256, 256, n=9): nine bottlenecks with shortcuts, nine accumulating backward passes."""
    import basedet.layers as BL
    layer = TB._block_case(lambda: BL.CSPLayer(256, 256, 9, True), BO.csp_layer, 2, 256, 4, 6, seed=23, n=9, shortcut=True)
    assert len(layer.m) == 9


def test_focus_at_the_default_width():
    """Focus(3, 64, 3), the default stem."""
    import basedet.layers as BL
    TB._block_case(lambda: BL.Focus(3, 64, 3), BO.focus, 2, 3, 6, 10, seed=24, image=True)
