"""csrc/batchnorm.hip (MODEL.FPN.NORM = "BN" / "SyncBN") against float64 NumPy computed from the same bf16 inputs.

Bounds:
  * mean within 1e-5 (|mu| + sigma) of float64; the biased variance within 1e-4 relative on every non-constant channel (a fixed-order Chan
    combination in fp32 errs at a few ulp log2 M ~ 1e-6: x100 margin, and a raw fp32 sum of squares misses it on the channel whose mean
    is 100 sigma); the running statistics to the same bounds;
  * apply / backward apply: every bf16 output within one bf16 ulp of the float64 formula evaluated on the kernel's own fp32 statistics;
  * dgamma / dbeta within 1e-5 sum |terms| of float64 (xhat from the fp32 mean / inv_std the kernel is handed);
  * two runs give identical bits for every output.
"""
import numpy as np
import pytest
import torch

from util import bf16_ulps, bits_of, gapped_geom, guarded

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
SHAPES = [(2, 1, 1, 8), (1, 13, 21, 24), (2, 7, 11, 256), (3, 25, 42, 256)]


def _inputs(M, C, seed):
    """y, g (M, C) bf16-representable fp32; gamma (both signs), beta, running statistics.  Channel 0: mean 100 sigma, 1: constant,
    2: all zero, the rest: random scale and offset."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((M, C)) * rng.uniform(0.2, 3.0, C) + rng.uniform(-2.0, 2.0, C)
    y[:, 0] = 100.0 + rng.standard_normal(M)
    y[:, 1] = 3.25
    y[:, 2] = 0.0
    g = rng.standard_normal((M, C)) * 0.1 + rng.uniform(-0.05, 0.05, C)
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(torch.bfloat16)
    gamma = rng.standard_normal(C).astype(np.float32)
    gamma[:4] = [1.5, -0.75, 0.5, -1.25]
    beta = rng.standard_normal(C).astype(np.float32)
    rm0, rv0 = rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2.0, C).astype(np.float32)
    rm0[2] = 0.0          # the all-zero channel has never seen anything else: its running mean stays exactly zero
    return t(y), t(g), gamma, beta, rm0, rv0


def _run(ops, y, gy, g, gg, z, gz, gout, go, C, gamma, beta, rm0, rv0):
    """The four kernels on one level; returns every output (device tensors)."""
    dev = "cuda"
    f = lambda: torch.empty(C, dtype=torch.float32, device=dev)
    M = gy.N * gy.H[0] * gy.W[0]
    ws = torch.empty(ops.bn_workspace_bytes(M, C) // 4 + 16, dtype=torch.float32, device=dev)
    o = dict(mean=f(), inv_std=f(), sums=torch.empty((3, C), dtype=torch.float32, device=dev), rm=torch.from_numpy(rm0).to(dev),
             rv=torch.from_numpy(rv0).to(dev), dgamma=f(), dbeta=f())
    gam, bet = torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev)
    ops.bn_stats_fwd(y, gy, C, EPS, MOM, o["mean"], o["inv_std"], o["sums"], o["rm"], o["rv"], ws)
    ops.bn_apply_act_fwd(y, gy, o["mean"], o["inv_std"], gam, bet, z, gz, C, relu=False)
    ops.bn_bwd_reduce(g, gg, y, gy, o["mean"], o["inv_std"], C, o["dgamma"], o["dbeta"], ws)
    ops.bn_bwd_apply(g, gg, y, gy, o["mean"], o["inv_std"], gam, o["dgamma"], o["dbeta"], o["sums"][0], gout, go, C)
    torch.cuda.synchronize()
    return o


def _check(o, y, g, z, gout, gamma, beta, rm0, rv0):
    """y, g, z, gout: (M, C) CPU tensors of the level's rows."""
    y64, g64 = y.double().numpy(), g.double().numpy()
    M = y64.shape[0]
    mu, var = y64.mean(0), y64.var(0)
    sig = np.sqrt(var)
    mean, inv_std = o["mean"].cpu().double().numpy(), o["inv_std"].cpu().double().numpy()
    print("max mean err / (|mu| + sigma)", np.max(np.abs(mean - mu) / (np.abs(mu) + sig + 1e-300)))
    assert np.all(np.abs(mean - mu) <= 1e-5 * (np.abs(mu) + sig))
    got_var = 1.0 / inv_std ** 2 - EPS
    live = var > 0
    assert live.sum() >= y64.shape[1] - 2 and not live[1] and not live[2]
    rel = np.abs(got_var[live] - var[live]) / var[live]
    print("max rel var err", rel.max(), "on the mean-100-sigma channel", abs(got_var[0] - var[0]) / var[0])
    # (inv_std is fp32: reading the variance back from it costs 2 x 2^-24 (1 + eps / var) relative, far below the bound)
    assert np.all(rel <= 1e-4)
    # sigma^2 = 0: inv_std = 1 / sqrt(1e-5), the correctly rounded fp32 operations
    want = np.float32(1.0) / np.sqrt(np.float32(EPS))
    assert np.all(o["inv_std"].cpu().numpy()[~live] == want)
    sums = o["sums"].cpu().double().numpy()
    assert np.all(sums[0] == M)
    assert np.all(np.abs(sums[1] - mu * M) <= 1e-5 * (np.abs(mu) + sig) * M)
    assert np.all(np.abs(sums[2] - (y64 ** 2).sum(0)) <= 1e-5 * (y64 ** 2).sum(0))
    rm_ref = (1 - MOM) * rm0.astype(np.float64) + MOM * mu
    rv_ref = (1 - MOM) * rv0.astype(np.float64) + MOM * var * M / max(M - 1, 1)
    assert np.all(np.abs(o["rm"].cpu().double().numpy() - rm_ref) <= 1e-5 * (np.abs(mu) + sig))
    assert np.all(np.abs(o["rv"].cpu().double().numpy() - rv_ref) <= 1e-4 * rv_ref)
    # apply: the float64 formula on the kernel's own statistics
    xh = (y64 - mean) * inv_std
    zr = gamma.astype(np.float64) * xh + beta.astype(np.float64)
    assert int(bf16_ulps(z, torch.from_numpy(zr)).max()) <= 1
    # dgamma / dbeta
    dg, db = o["dgamma"].cpu().double().numpy(), o["dbeta"].cpu().double().numpy()
    tg = g64 * xh
    print("dgamma err / sum|terms|", np.max(np.abs(dg - tg.sum(0)) / (np.abs(tg).sum(0) + 1e-300)),
          "dbeta", np.max(np.abs(db - g64.sum(0)) / (np.abs(g64).sum(0) + 1e-300)))
    assert np.all(np.abs(dg - tg.sum(0)) <= 1e-5 * np.abs(tg).sum(0))
    assert np.all(np.abs(db - g64.sum(0)) <= 1e-5 * np.abs(g64).sum(0))
    # backward apply on the kernel's own dgamma / dbeta
    gr = gamma.astype(np.float64) * inv_std * (g64 - db / M - xh * dg / M)
    assert int(bf16_ulps(gout, torch.from_numpy(gr)).max()) <= 1


def _same_bits(a, b):
    for k in a:
        assert torch.equal(bits_of(a[k]), bits_of(b[k])), k


@pytest.mark.parametrize("N,H,W,C", SHAPES)
def test_bn_kernels_match_float64(N, H, W, C):
    from basedet_amd import ops
    M = N * H * W
    y, g, gamma, beta, rm0, rv0 = _inputs(M, C, seed=M * 7 + C)
    geo = ops.single(N, H, W)
    yd, gd = y.cuda(), g.cuda()
    outs = []
    for _ in range(2):
        z = torch.empty((M, C), dtype=torch.bfloat16, device="cuda")
        gout = torch.empty_like(z)
        o = _run(ops, yd, geo, gd, geo, z, geo, gout, geo, C, gamma, beta, rm0, rv0)
        outs.append(dict(o, z=z, gout=gout))
    _check(outs[0], y, g, outs[0]["z"].cpu(), outs[0]["gout"].cpu(), gamma, beta, rm0, rv0)
    _same_bits(outs[0], outs[1])


def test_bn_level_inside_a_multi_level_buffer():
    """Three levels per image, the middle one normalised: non-zero offset, row stride != n; the gradient and both outputs live in gapped
    buffers of their own geometry.  The other levels, the gaps and the guard bands keep their bits."""
    from basedet_amd import ops
    N, C, levels, li = 2, 64, [(5, 7), (7, 11), (3, 4)], 1
    H, W = levels[li]
    n, M = H * W, N * H * W
    y, g, gamma, beta, rm0, rv0 = _inputs(M, C, seed=11)
    geom, kind = gapped_geom(N, levels, gap=64)
    lvl = geom.level(li)
    rows = (torch.arange(N).view(-1, 1) * geom.pix_per_img + geom.off[li] + torch.arange(n).view(1, -1)).view(-1)
    rng = np.random.default_rng(12)

    def buf(name, fill, data):
        t, h = guarded(geom.pixels, C, torch.bfloat16, "cuda", fill=fill, name=name)
        body = torch.from_numpy(rng.standard_normal((geom.pixels, C)).astype(np.float32)).to(torch.bfloat16)
        if data is not None:
            body[rows] = data
        h.set(body).set_gaps(kind).snapshot()
        return t, h
    yb, yh = buf("y", "nan", y)
    gb, gh = buf("g", "max", g)
    zb, zh = buf("z", "sentinel", None)
    ob, oh = buf("g_y", "sentinel", None)
    o = _run(ops, yb, lvl, gb, lvl, zb, lvl, ob, lvl, C, gamma, beta, rm0, rv0)
    yh.assert_unchanged()
    gh.assert_unchanged()
    other = torch.ones(geom.pixels, dtype=torch.bool)
    other[rows] = False
    for t, h in ((zb, zh), (ob, oh)):
        h.check()
        before = h._snap.view(-1, C)[h.g:h.g + geom.pixels].cpu()
        assert torch.equal(bits_of(t).cpu()[other], before[other]), h.name
    _check(o, y, g, zb.cpu()[rows], ob.cpu()[rows], gamma, beta, rm0, rv0)


def test_bn_refuses_bad_arguments():
    from basedet_amd import ops
    from basedet_amd._lib import BasedetHipError
    geo = ops.single(1, 2, 2)
    t = torch.zeros((4, 12), dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(12, dtype=torch.float32, device="cuda")
    ws = torch.zeros(64, dtype=torch.float32, device="cuda")
    with pytest.raises(BasedetHipError):                 # C % 8 != 0
        ops.bn_stats_fwd(t, geo, 12, EPS, MOM, f, f, None, None, None, ws)
    t = torch.zeros((4, 16), dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(16, dtype=torch.float32, device="cuda")
    with pytest.raises(BasedetHipError):                 # the level does not fit its image's rows
        ops.bn_stats_fwd(t, ops.Geom(1, [2], [2], [2], 4), 16, EPS, MOM, f, f, None, None, None, ws)
    with pytest.raises(BasedetHipError):                 # in place
        ops.bn_bwd_apply(t, geo, t, geo, f, f, f, f, f, f, t, geo, 16)
    with pytest.raises(BasedetHipError):                 # workspace
        ops.bn_stats_fwd(t, geo, 16, EPS, MOM, f, f, None, None, None, ws[:2])
