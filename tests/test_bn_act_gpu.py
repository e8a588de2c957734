"""bd_bn_apply_act_fwd (csrc/batchnorm.hip) and bd_stem_conv7x7_raw_fwd (csrc/stem.hip): the two launches MODEL.BACKBONE.NORM = "BN" /
"SyncBN" adds to the forward pass.

bd_bn_apply_act_fwd, z = [relu](gamma (y - mean) inv_std + beta [+ residual]), against float64 NumPy on the same bf16 inputs and the kernel's
own fp32 statistics: every output within one bf16 ulp (tests/test_batchnorm_gpu.py's bound for the apply kernels), over residual x ReLU, on
that file's hard channels (mean 100 sigma, constant, all zero, gamma < 0) and a residual that cancels gamma xhat + beta to near zero; two
runs give the same bits; one run inside guarded, gapped buffers; the FPN's form (no residual, no ReLU, a dense y into one level of a
pyramid z).  The raw stem launch against conv2d of the bf16-rounded operands with no
affine and no ReLU at tests/test_conv_gpu.py's TOL (1e-2 rel-L2), its output guarded."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from test_batchnorm_gpu import EPS, MOM, _inputs
from util import bf16_round, bf16_ulps, bits_of, gapped_geom, guarded, oihw_to_ohwi, rel_l2

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 1, 8), (1, 13, 21, 24), (2, 7, 11, 64), (1, 5, 6, 2048)]
TOL = 1e-2          # tests/test_conv_gpu.py


def _stats(ops, y, geo, C):
    f = lambda: torch.empty(C, dtype=torch.float32, device="cuda")
    M = geo.N * geo.H[0] * geo.W[0]
    ws = torch.empty(ops.bn_workspace_bytes(M, C) // 4 + 16, dtype=torch.float32, device="cuda")
    mean, inv_std = f(), f()
    ops.bn_stats_fwd(y, geo, C, EPS, MOM, mean, inv_std, None, None, None, ws)
    return mean, inv_std


def _residual(y, gamma, beta, seed):
    """Half of the channels: random; the other half: -(gamma xhat + beta) rounded to bf16, so the sum is the rounding residue."""
    rng = np.random.default_rng(seed)
    y64 = y.double().numpy()
    mu, var = y64.mean(0), y64.var(0)
    z = gamma.astype(np.float64) * (y64 - mu) / np.sqrt(var + EPS) + beta.astype(np.float64)
    r = rng.standard_normal(z.shape)
    r[:, 1::2] = -z[:, 1::2]
    return torch.from_numpy(r.astype(np.float32)).to(torch.bfloat16)


def _ref(y, res, mean, inv_std, gamma, beta, relu):
    z = gamma.astype(np.float64) * (y.double().numpy() - mean) * inv_std + beta.astype(np.float64)
    if res is not None:
        z = z + res.double().numpy()
    return torch.from_numpy(np.maximum(z, 0.0) if relu else z)


@pytest.mark.parametrize("N,H,W,C", SHAPES)
def test_bn_apply_act_matches_float64(N, H, W, C):
    from basedet_amd import ops
    M = N * H * W
    y, _, gamma, beta, _, _ = _inputs(M, C, seed=M * 5 + C)
    res = _residual(y, gamma, beta, seed=M + C)
    geo = ops.single(N, H, W)
    yd, rd = y.cuda(), res.cuda()
    gam, bet = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
    mean, inv_std = _stats(ops, yd, geo, C)
    m64, s64 = mean.cpu().double().numpy(), inv_std.cpu().double().numpy()
    for with_res in (False, True):
        for relu in (False, True):
            outs = []
            for _ in range(2):
                z = torch.empty((M, C), dtype=torch.bfloat16, device="cuda")
                ops.bn_apply_act_fwd(yd, geo, mean, inv_std, gam, bet, z, geo, C, residual=rd if with_res else None, gr=geo, relu=relu)
                outs.append(z)
            torch.cuda.synchronize()
            ref = _ref(y, res if with_res else None, m64, s64, gamma, beta, relu)
            ulps = int(bf16_ulps(outs[0].cpu(), ref).max())
            print("residual", with_res, "relu", relu, "max bf16 ulps", ulps)
            assert ulps <= 1, (with_res, relu, ulps)
            assert torch.equal(bits_of(outs[0]), bits_of(outs[1]))
            if relu:
                assert float(outs[0].float().min()) >= 0


def test_bn_apply_act_inside_gapped_guarded_buffers():
    """The middle one of three levels, y / residual / z each in a guarded buffer with poisoned row gaps: inputs keep their bits, z changes
    on the level's rows only."""
    from basedet_amd import ops
    N, C, levels, li = 2, 64, [(5, 7), (7, 11), (3, 4)], 1
    H, W = levels[li]
    n, M = H * W, N * H * W
    y, _, gamma, beta, _, _ = _inputs(M, C, seed=21)
    res = _residual(y, gamma, beta, seed=22)
    geom, kind = gapped_geom(N, levels, gap=64)
    lvl = geom.level(li)
    rows = (torch.arange(N).view(-1, 1) * geom.pix_per_img + geom.off[li] + torch.arange(n).view(1, -1)).view(-1)
    rng = np.random.default_rng(23)

    def buf(name, fill, data):
        t, h = guarded(geom.pixels, C, torch.bfloat16, "cuda", fill=fill, name=name)
        body = torch.from_numpy(rng.standard_normal((geom.pixels, C)).astype(np.float32)).to(torch.bfloat16)
        if data is not None:
            body[rows] = data
        h.set(body).set_gaps(kind).snapshot()
        return t, h
    yb, yh = buf("y", "nan", y)
    rb, rh = buf("residual", "max", res)
    zb, zh = buf("z", "sentinel", None)
    gam, bet = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
    mean, inv_std = _stats(ops, yb, lvl, C)
    ops.bn_apply_act_fwd(yb, lvl, mean, inv_std, gam, bet, zb, lvl, C, residual=rb, gr=lvl, relu=True)
    torch.cuda.synchronize()
    yh.assert_unchanged()
    rh.assert_unchanged()
    zh.check()
    other = torch.ones(geom.pixels, dtype=torch.bool)
    other[rows] = False
    before = zh._snap.view(-1, C)[zh.g:zh.g + geom.pixels].cpu()
    assert torch.equal(bits_of(zb).cpu()[other], before[other])
    ref = _ref(y, res, mean.cpu().double().numpy(), inv_std.cpu().double().numpy(), gamma, beta, True)
    assert int(bf16_ulps(zb.cpu()[rows], ref).max()) <= 1


@pytest.mark.parametrize("C", [8, 264])
def test_bn_apply_act_dense_into_pyramid_levels(C):
    """What the FPN's output norms launch: no residual, no ReLU, a dense y written into ONE level of a two-level pyramid z -- level 1, then
    level 0.  C = 8 is one chunk; C = 264 crosses the 256-channel tile (blockIdx.y = 1 runs with one live chunk lane).  Each level within
    one bf16 ulp of float64 NumPy; the level not written, the rows between the levels and between the images and the guards keep their
    sentinel bits, and the second launch leaves the first one's level alone."""
    from basedet_amd import ops
    N, levels = 2, [(5, 7), (3, 4)]
    geom, kind = gapped_geom(N, levels, gap=16)
    zb, zh = guarded(geom.pixels, C, torch.bfloat16, "cuda", fill="sentinel", name="z")
    zh.set_gaps(kind).snapshot()
    before = zh._snap.view(-1, C)[zh.g:zh.g + geom.pixels].cpu()
    rows = [(torch.arange(N).view(-1, 1) * geom.pix_per_img + geom.off[li] + torch.arange(h * w).view(1, -1)).view(-1)
            for li, (h, w) in enumerate(levels)]
    done = {}
    for li in (1, 0):
        H, W = levels[li]
        M = N * H * W
        y, _, gamma, beta, _, _ = _inputs(M, C, seed=31 + li + C)
        dense = ops.single(N, H, W)
        yd, gam, bet = y.cuda(), torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
        mean, inv_std = _stats(ops, yd, dense, C)
        ops.bn_apply_act_fwd(yd, dense, mean, inv_std, gam, bet, zb, geom.level(li), C, residual=None, relu=False)
        torch.cuda.synchronize()
        zh.check()
        got = zb.cpu()
        ref = _ref(y, None, mean.cpu().double().numpy(), inv_std.cpu().double().numpy(), gamma, beta, False)
        ulps = int(bf16_ulps(got[rows[li]], ref).max())
        print("C", C, "level", li, "max bf16 ulps", ulps)
        assert ulps <= 1, (li, ulps)
        done[li] = bits_of(got[rows[li]]).clone()
        for lj in (0, 1):
            if lj in done:
                assert torch.equal(bits_of(got[rows[lj]]), done[lj]), lj
            else:
                assert torch.equal(bits_of(got[rows[lj]]), before[rows[lj]]), lj


def test_bn_apply_act_refuses_bad_arguments():
    from basedet_amd import ops
    from basedet_amd._lib import BasedetHipError
    geo = ops.single(1, 2, 2)
    f = torch.zeros(16, dtype=torch.float32, device="cuda")
    t = torch.zeros((4, 16), dtype=torch.bfloat16, device="cuda")
    z = torch.zeros_like(t)
    with pytest.raises(BasedetHipError):          # in place: the backward pass reads y
        ops.bn_apply_act_fwd(t, geo, f, f, f, f, t, geo, 16)
    with pytest.raises(BasedetHipError):          # onto the shortcut
        ops.bn_apply_act_fwd(t, geo, f, f, f, f, z, geo, 16, residual=z, gr=geo)
    with pytest.raises(BasedetHipError):          # C % 8
        ops.bn_apply_act_fwd(t, geo, f, f, f, f, z, geo, 12)


@pytest.mark.parametrize("N,Hp,Wp", [(1, 32, 32), (2, 64, 96)])
def test_raw_stem_launch(N, Hp, Wp):
    """bd_stem_conv7x7_raw_fwd = the 7x7 / 2 convolution alone: against conv2d on the bf16 operands (no scale, no shift, no ReLU; negative
    outputs survive), output guarded; the default launch with scale 1 / shift 0 is its ReLU, value for value."""
    from basedet_amd import ops
    H, W = Hp - 5, Wp - 9
    g = torch.Generator().manual_seed(Hp * 3 + Wp)
    img = torch.rand(N, 3, H, W, generator=g) * 255
    mean, std = [103.530, 116.280, 123.675], [57.375, 57.12, 58.395]
    xh = torch.empty((N, Hp + 6, Wp + 8, 4), dtype=torch.bfloat16, device="cuda")
    ops.pad_normalize(img.cuda(), Hp, Wp, mean, std, xh)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.05
    wst = torch.empty((64, 7, 8, 4), dtype=torch.bfloat16, device="cuda")
    ops.stem_weight_pack(oihw_to_ohwi(w).cuda(), None, wst)
    Ho, Wo = Hp // 2, Wp // 2
    y, yh = guarded(N * Ho * Wo, 64, torch.bfloat16, "cuda", fill="sentinel", name="y")
    ops.stem_conv7x7_raw_fwd(N, Hp, Wp, xh, wst, y)
    torch.cuda.synchronize()
    yh.check()
    xo = (TF.pad(img, (0, Wp - W, 0, Hp - H)) - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
    ref = TF.conv2d(bf16_round(xo), bf16_round(w), None, stride=2, padding=3)
    got = y.float().cpu().view(N, Ho, Wo, 64).permute(0, 3, 1, 2)
    err = rel_l2(got, ref)
    print("raw stem rel-L2", err)
    assert err < TOL
    assert float(got.min()) < 0
    yr = torch.empty((N * Ho * Wo, 64), dtype=torch.bfloat16, device="cuda")
    ops.stem_conv7x7_fwd(N, Hp, Wp, xh, wst, torch.zeros(64, device="cuda"), yr)
    assert torch.equal(yr.float(), torch.relu(y.float()))
