"""bd_bn_silu_* (csrc/batchnorm.hip), basedet.layers.ConvBNSiLU and YOLOXHead against the float64 oracle of tests/yolox_head_oracle.py.

Kernels (operands in guarded allocations, every launch twice with the same bits):
  * z and gy within ONE bf16 step of the float64 formula on the same bf16 inputs and the kernel's own fp32 statistics / sums;
  * dgamma / dbeta within 1e-5 sum |terms| of float64 -- tests/test_batchnorm_gpu.py's bound for bd_bn_bwd_reduce, the terms being
    g_u * xhat and g_u with g_u = g * silu'(u);
  * bd_bn_silu_bwd_apply == bd_bn_bwd_apply bit for bit where the gate is exactly 1 in fp32.
Layers and head: the ratio form of DESIGN.md 4v -- the device's rel-L2 distance from the float64 oracle is at most TWICE the distance of the
bf16-faithful oracle from it; a quantity that is exactly zero in the oracle is bounded absolutely."""
import functools

import numpy as np
import pytest
import torch

import util
import yolox_head_oracle as O
from util import bf16_ulps, bits_of, gapped_geom, guarded

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
EPS, MOM = O.EPS, O.MOMENTUM
DEV = "cuda"


# ---- kernels ---------------------------------------------------------------------------------------------------------------------------------
def _inputs(M, C, seed):
    """y, g (M, C) bf16; gamma, beta fp32.  Channel 0: |mean| = 100 sigma; 1: constant; 2: gamma = 0; 3: u spread over +-100 and beyond
    (exp(-|u|) down to fp32 denormals and zero); the rest: |gamma| log-uniform in [0.1, 60], both signs.  Every 7th row of g is zero."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((M, C)) * rng.uniform(0.2, 3.0, C) + rng.uniform(-2.0, 2.0, C)
    y[:, 0] = 100.0 + rng.standard_normal(M)
    y[:, 1] = 3.25
    g = rng.standard_normal((M, C)) * 0.1 + rng.uniform(-0.05, 0.05, C)
    g[::7] = 0.0
    gamma = (0.1 * 600.0 ** rng.random(C) * np.where(rng.random(C) < 0.5, -1.0, 1.0)).astype(np.float32)
    gamma[:4] = [1.5, -0.75, 0.0, 40.0]
    beta = rng.uniform(-3.0, 3.0, C).astype(np.float32)
    beta[3] = 0.0
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(BF)
    return t(y), t(g), gamma, beta


def _run(ops, y, gy, g, gg, z, gz, gout, go, C, gamma, beta):
    """stats -> silu fwd -> silu reduce -> silu apply on one level; returns every fp32 output (device tensors)."""
    f = lambda: torch.empty(C, dtype=F32, device=DEV)
    M = gy.N * gy.H[0] * gy.W[0]
    ws = torch.empty(ops.bn_workspace_bytes(M, C) // 4 + 16, dtype=F32, device=DEV)
    o = dict(mean=f(), inv_std=f(), sums=torch.empty((3, C), dtype=F32, device=DEV), dgamma=f(), dbeta=f())
    gam, bet = torch.from_numpy(gamma).to(DEV), torch.from_numpy(beta).to(DEV)
    ops.bn_stats_fwd(y, gy, C, EPS, MOM, o["mean"], o["inv_std"], o["sums"], None, None, ws)
    ops.bn_silu_fwd(y, gy, o["mean"], o["inv_std"], gam, bet, z, gz, C)
    ops.bn_silu_bwd_reduce(g, gg, y, gy, o["mean"], o["inv_std"], gam, bet, C, o["dgamma"], o["dbeta"], ws)
    ops.bn_silu_bwd_apply(g, gg, y, gy, o["mean"], o["inv_std"], gam, bet, o["dgamma"], o["dbeta"], o["sums"][0], gout, go, C)
    torch.cuda.synchronize()
    return o


def _check(o, y, g, z, gout, gamma, beta, what):
    """y, g, z, gout: (M, C) CPU tensors of the level's rows."""
    mean, inv_std = o["mean"].cpu().numpy(), o["inv_std"].cpu().numpy()
    y64, g64 = y.double().numpy(), g.double().numpy()
    zr, u = O.bn_silu_fwd(y64, mean, inv_std, gamma, beta)
    if y64.shape[0] >= 127:
        assert u.max() > 80 and u.min() < -80, "the inputs are meant to spread u over +-100"
    dz = bf16_ulps(z, torch.from_numpy(zr))
    dg, db = o["dgamma"].cpu().numpy(), o["dbeta"].cpu().numpy()
    gu, xh, dg64, db64, gr = O.bn_silu_bwd(g64, y64, mean, inv_std, gamma, beta, dg, db)
    dgy = bf16_ulps(gout, torch.from_numpy(gr))
    tg = gu * xh
    eg = np.max(np.abs(dg - dg64) / (np.abs(tg).sum(0) + 1e-300))
    eb = np.max(np.abs(db - db64) / (np.abs(gu).sum(0) + 1e-300))
    print(f"{what}: z max {int(dz.max())} ulp, exactly equal {float((dz == 0).double().mean()):.4f}; gy max {int(dgy.max())} ulp, exactly equal "
          f"{float((dgy == 0).double().mean()):.4f}; dgamma err / sum|terms| {eg:.2e}, dbeta {eb:.2e}")
    assert int(dz.max()) <= 1
    assert int(dgy.max()) <= 1
    assert np.all(np.abs(dg - dg64) <= 1e-5 * np.abs(tg).sum(0))
    assert np.all(np.abs(db - db64) <= 1e-5 * np.abs(gu).sum(0))


def _same_bits(a, b):
    for k in a:
        assert torch.equal(bits_of(a[k]), bits_of(b[k])), k


@pytest.mark.parametrize("C", [8, 24, 264])
@pytest.mark.parametrize("M", [1, 127, 129, 1030])
def test_bn_silu_kernels_match_float64(M, C):
    from basedet_amd import ops
    y, g, gamma, beta = _inputs(M, C, seed=M * 7 + C)
    geo = ops.single(1, 1, M)
    yb, yh = guarded(M, C, BF, DEV, fill="nan", name="y")
    gb, gh = guarded(M, C, BF, DEV, fill="max", name="g")
    yh.set(y).snapshot(), gh.set(g).snapshot()
    outs = []
    for _ in range(2):
        zb, zh = guarded(M, C, BF, DEV, fill="sentinel", name="z")
        ob, oh = guarded(M, C, BF, DEV, fill="sentinel", name="gy")
        o = _run(ops, yb, geo, gb, geo, zb, geo, ob, geo, C, gamma, beta)
        zh.check(), oh.check()
        outs.append(dict(o, z=zb.clone(), gout=ob.clone()))
    yh.assert_unchanged(), gh.assert_unchanged()
    _check(outs[0], y, g, outs[0]["z"].cpu(), outs[0]["gout"].cpu(), gamma, beta, f"M={M} C={C}")
    _same_bits(outs[0], outs[1])


def test_bn_silu_level_inside_a_two_level_buffer():
    """N = 2, two levels per image, the second one normalised: off != 0, and y, z, g, gy each in a gapped buffer of its OWN geometry.  The
    other level, the gaps and the guard bands keep their bits."""
    from basedet_amd import ops
    N, C, levels, li = 2, 24, [(3, 5), (5, 7)], 1
    H, W = levels[li]
    n, M = H * W, N * H * W
    y, g, gamma, beta = _inputs(M, C, seed=11)
    rng = np.random.default_rng(12)
    bufs = {}
    for name, gap, fill, data in (("y", 64, "nan", y), ("g", 96, "max", g), ("z", 128, "sentinel", None), ("gy", 160, "sentinel", None)):
        geom, kind = gapped_geom(N, levels, gap=gap)
        rows = (torch.arange(N).view(-1, 1) * geom.pix_per_img + geom.off[li] + torch.arange(n).view(1, -1)).view(-1)
        t, h = guarded(geom.pixels, C, BF, DEV, fill=fill, name=name)
        body = torch.from_numpy(rng.standard_normal((geom.pixels, C)).astype(np.float32)).to(BF)
        if data is not None:
            body[rows] = data
        h.set(body).set_gaps(kind).snapshot()
        bufs[name] = (t, h, geom.level(li), rows, geom)
    assert len({(b[2].pix_per_img, b[2].off[0]) for b in bufs.values()}) == 4
    (yb, yh, ly, _, _), (gb, gh, lg, _, _), (zb, zh, lz, rz, geoz), (ob, oh, lo, ro, geoo) = (bufs[k] for k in ("y", "g", "z", "gy"))
    o = _run(ops, yb, ly, gb, lg, zb, lz, ob, lo, C, gamma, beta)
    z1, o1 = zb.clone(), ob.clone()
    o2 = _run(ops, yb, ly, gb, lg, zb, lz, ob, lo, C, gamma, beta)
    yh.assert_unchanged(), gh.assert_unchanged()
    for t, h, rows, geom in ((zb, zh, rz, geoz), (ob, oh, ro, geoo)):
        h.check()
        other = torch.ones(geom.pixels, dtype=torch.bool)
        other[rows] = False
        before = h._snap.view(-1, C)[h.g:h.g + geom.pixels].cpu()
        assert torch.equal(bits_of(t).cpu()[other], before[other]), h.name
    _check(o, y, g, zb.cpu()[rz], ob.cpu()[ro], gamma, beta, "level in a two-level buffer")
    _same_bits(o, o2)
    assert torch.equal(bits_of(z1), bits_of(zb)) and torch.equal(bits_of(o1), bits_of(ob))


def test_bn_silu_bwd_apply_is_bn_bwd_apply_where_the_gate_is_one():
    """gamma, beta with u in [55, 85]: exp(-u) < 2^-79, so sigma(u) rounds to 1 in fp32 and the gate sigma(u) (1 + u sigma(-u)) is exactly
    1 in the apply kernel's fp64 as well (u exp(-u) < 2^-72): g_u = g, and the two apply kernels evaluate the same fp64 expression on the
    same operands."""
    from basedet_amd import ops
    M, C = 1030, 24
    y, g, _, _ = _inputs(M, C, seed=5)
    rng = np.random.default_rng(6)
    geo = ops.single(1, 1, M)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(DEV)
    mean, inv_std, sums = (torch.empty(s, dtype=F32, device=DEV) for s in (C, C, (3, C)))
    ws = torch.empty(ops.bn_workspace_bytes(M, C) // 4 + 16, dtype=F32, device=DEV)
    yd, gd = y.to(DEV), g.to(DEV)
    ops.bn_stats_fwd(yd, geo, C, EPS, MOM, mean, inv_std, sums, None, None, ws)
    xh = (y.double().numpy() - mean.cpu().double().numpy()) * inv_std.cpu().double().numpy()
    gamma = (rng.uniform(0.5, 2.0, C) * np.where(rng.random(C) < 0.5, -1.0, 1.0)).astype(np.float32)
    gamma = (gamma * np.minimum(1.0, 15.0 / (np.abs(gamma) * np.abs(xh).max(0) + 1e-30))).astype(np.float32)       # |gamma xhat| <= 15
    beta = np.full(C, 70.0, np.float32)
    u = gamma.astype(np.float64) * xh + 70.0
    assert u.min() >= 55.0 and u.max() <= 85.0
    dg, db = f(rng.standard_normal(C)), f(rng.standard_normal(C))
    a, b = torch.empty_like(yd), torch.empty_like(yd)
    ops.bn_bwd_apply(gd, geo, yd, geo, mean, inv_std, f(gamma), dg, db, sums[0], a, geo, C)
    ops.bn_silu_bwd_apply(gd, geo, yd, geo, mean, inv_std, f(gamma), f(beta), dg, db, sums[0], b, geo, C)
    assert torch.equal(bits_of(a), bits_of(b))


def test_bn_silu_refuses_bad_arguments():
    """Every refusal comes before any launch: the output keeps its sentinel."""
    from basedet_amd import ops
    from basedet_amd._lib import BasedetHipError
    geo = ops.single(1, 2, 2)
    C = 16
    t, g = (torch.zeros((4, C), dtype=BF, device=DEV) for _ in range(2))
    out, oh = guarded(4, C, BF, DEV, fill="sentinel", name="out")
    oh.snapshot()
    f = torch.ones(C, dtype=F32, device=DEV)
    ws = torch.zeros(256, dtype=F32, device=DEV)
    bad_geo = ops.Geom(1, [2], [2], [2], 4)          # the level does not fit its image's rows
    t12, f12 = torch.zeros((4, 12), dtype=BF, device=DEV), torch.ones(12, dtype=F32, device=DEV)
    cases = [
        ("(code -1)", lambda: ops.bn_silu_fwd(t, geo, f, f, f, f, t, geo, C)),                                   # z == y
        ("(code -1)", lambda: ops.bn_silu_bwd_apply(g, geo, t, geo, f, f, f, f, f, f, f, g, geo, C)),            # gy == g
        ("(code -1)", lambda: ops.bn_silu_fwd(t12, geo, f12, f12, f12, f12, out, geo, 12)),                      # C % 8 != 0
        ("(code -1)", lambda: ops.bn_silu_bwd_reduce(g, geo, t12, geo, f12, f12, f12, f12, 12, f12, f12, ws)),
        ("(code -1)", lambda: ops.bn_silu_bwd_apply(g, geo, t12, geo, f12, f12, f12, f12, f12, f12, f12, out, geo, 12)),
        ("(code -1)", lambda: ops.bn_silu_fwd(t, bad_geo, f, f, f, f, out, geo, C)),                             # bad geometry
        ("(code -1)", lambda: ops.bn_silu_fwd(t, geo, f, f, f, f, out, bad_geo, C)),
        ("(code -1)", lambda: ops.bn_silu_bwd_reduce(g, bad_geo, t, geo, f, f, f, f, C, f, f, ws)),
        ("(code -1)", lambda: ops.bn_silu_bwd_apply(g, geo, t, geo, f, f, f, f, f, f, f, out, bad_geo, C)),
        ("(code -3)", lambda: ops.bn_silu_bwd_reduce(g, geo, t, geo, f, f, f, f, C, f, f, ws[:2])),              # a short workspace: BD_EWORKSPACE
        ("(code -1)", lambda: ops.bn_silu_fwd(t, geo, f, f, None, f, out, geo, C)),                              # null pointers: BD_EINVAL
        ("(code -1)", lambda: ops.bn_silu_fwd(None, geo, f, f, f, f, out, geo, C)),
        ("(code -1)", lambda: ops.bn_silu_bwd_reduce(g, geo, t, geo, f, f, f, None, C, f, f, ws)),
        ("(code -1)", lambda: ops.bn_silu_bwd_apply(g, geo, t, geo, f, f, f, f, f, f, None, out, geo, C)),
    ]
    dg = torch.full((C,), 7.0, dtype=F32, device=DEV)
    cases.append(("(code -3)", lambda: ops.bn_silu_bwd_reduce(g, geo, t, geo, f, f, f, f, C, dg, dg, ws[:2])))
    for code, fn in cases:
        with pytest.raises(BasedetHipError) as e:
            fn()
        assert code in str(e.value), str(e.value)
    torch.cuda.synchronize()
    oh.assert_unchanged()
    assert bool((dg == 7.0).all()) and bool((t == 0).all())


# ---- the ratio bound -----------------------------------------------------------------------------------------------------------------------------
FP32_SUM = 2.0 ** -20


def _ratio(dev, o64, of, name):
    dev, o64, of = (torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).double().cpu() for t in (dev, o64, of))
    if float(o64.abs().max()) == 0.0:          # exactly zero in the oracle: absolute (one bf16 step of nothing is nothing)
        assert float(dev.abs().max()) == 0.0, name
        return
    d, f = util.rel_l2(dev, o64), util.rel_l2(of, o64)
    print(f"{name}: device {d:.3e} faithful {f:.3e} ratio {d / max(f, 1e-300):.2f}")
    # FP32_SUM: where the faithful oracle has NO rounding point (a bias gradient is the plain sum of the bf16 gradient it is handed, and
    # the oracle adds in float64) its distance is exactly 0, while the device adds at most N P = 252 terms in fp32: a random walk of
    # 2^-24 steps, sqrt(252) 2^-24 < 2^-20.  Everywhere else the term is 1000 times below the bf16 distances and changes nothing.
    assert d <= 2 * f + FP32_SUM, name


# ---- ConvBNSiLU ----------------------------------------------------------------------------------------------------------------------------------
def _layer_oracle(x, p0, dy, k, faithful):
    p = O.double_params(p0, True)
    xr = x.double().clone().requires_grad_(True)
    st1, st2 = {}, {}
    z = O.conv_bn_silu(xr, p, "", k, 1, True, faithful, st1)
    (z * dy.double()).sum().backward()
    q = dict(p)
    q.update({k_: v for k_, v in st1.items()})
    O.conv_bn_silu(xr.detach(), {k_: v.detach() for k_, v in q.items()}, "", k, 1, True, faithful, st2)
    q0 = {k_: v.detach() for k_, v in p.items()}
    ze = O.conv_bn_silu(xr.detach(), q0, "", k, 1, False, faithful)
    out = dict(z=z.detach(), d_x=xr.grad, ze=ze)
    out.update({"g." + k_: v.grad for k_, v in p.items() if v.requires_grad})
    out.update({"s1." + k_: v for k_, v in st1.items()})
    out.update({"s2." + k_: v for k_, v in st2.items()})
    return out


@pytest.mark.parametrize("k", [1, 3])
def test_conv_bn_silu_layer(k):
    import basedet.layers as BL
    from basedet_amd._lib import BasedetHipError
    N, C, H, W = 2, 32, 5, 7
    g = torch.Generator().manual_seed(40 + k)
    x = torch.randn(N, C, H, W, generator=g).to(BF).float()
    dy = (0.1 * torch.randn(N, C, H, W, generator=g)).to(BF).float()
    p0 = {"weight": torch.randn(C, C, k, k, generator=g) / (C * k * k) ** 0.5, "norm.weight": 1.0 + 0.3 * torch.randn(C, generator=g),
          "norm.bias": 0.5 * torch.randn(C, generator=g), "norm.running_mean": 0.3 * torch.randn(C, generator=g),
          "norm.running_var": 0.5 + torch.rand(C, generator=g)}
    layer = BL.ConvBNSiLU(C, C, k)
    assert list(layer.state_dict()) == list(p0) and layer.eps == 1e-3 and layer.momentum == 0.03
    layer.load_state_dict(p0)
    z = layer(x.cuda())
    d_x = layer.backward(dy.cuda())
    grads = {k_: v.clone() for k_, v in layer.grads().items()}
    s1 = layer.state_dict()
    z2 = layer(x.cuda())
    d_x2 = layer.backward(dy.cuda())
    s2 = layer.state_dict()
    assert torch.equal(z, z2) and torch.equal(d_x, d_x2) and all(torch.equal(grads[k_], v) for k_, v in layer.grads().items())
    # accumulate=True adds the parameter gradients; dx=... adds the data gradient in place
    layer.backward(dy.cuda(), accumulate=True)
    for k_, v in layer.grads().items():
        assert torch.allclose(v, 2 * grads[k_], rtol=1e-6, atol=0), k_
    dx_pm = layer.backward_pm(util.nchw_to_pm(dy), dx=util.nchw_to_pm(d_x.cpu()).clone())
    assert util.rel_l2(util.pm_to_nchw(dx_pm, N, H, W), 2 * d_x.cpu()) < 2.0 ** -7
    with pytest.raises(BasedetHipError):
        layer(x)
    layer.load_state_dict(p0)
    layer.eval()
    ze = layer(x.cuda())
    assert torch.equal(ze, layer(x.cuda())) and layer.state_dict()["norm.running_mean"].equal(p0["norm.running_mean"])
    with pytest.raises(RuntimeError):
        layer.backward(dy.cuda())
    layer.train()
    o64, of = _layer_oracle(x, p0, dy, k, False), _layer_oracle(x, p0, dy, k, True)
    got = dict(z=z, d_x=d_x, ze=ze)
    got.update({"g." + k_: v for k_, v in grads.items()})
    got.update({f"s{i}.norm.{n}": s[f"norm.{n}"] for i, s in ((1, s1), (2, s2)) for n in ("running_mean", "running_var")})
    assert set(got) == set(o64)
    for name in sorted(got):
        _ratio(got[name], o64[name], of[name], f"k={k} {name}")


@pytest.mark.parametrize("k,stride", [(1, 1), (3, 2)])
def test_conv_bn_silu_grads_do_not_alias_the_storage(k, stride):
    """What grads() returned after one backward does not change at the next, which overwrites the same storage (k = 1: the OIHW view of
    the OHWI weight gradient is contiguous as it stands, so only a copy keeps it).  The norm's batch statistics are the layer's."""
    import basedet.layers as BL
    N, C, H, W = 2, 16, 5, 7
    g = torch.Generator().manual_seed(50 + k)
    x = torch.randn(N, C, H, W, generator=g).cuda()
    layer = BL.ConvBNSiLU(C, C, k, stride=stride, seed=9)
    z = layer(x)
    dy = (0.1 * torch.randn(z.shape, generator=g)).to(BF).float().cuda()
    layer.backward(dy)
    assert layer.mean is layer.norm.mean and layer.inv_std is layer.norm.inv_std and layer.sums is layer.norm.sums
    kept = layer.grads()
    copy = {k_: v.clone() for k_, v in kept.items()}
    layer.backward(2 * dy)
    again = layer.grads()
    assert list(kept) == ["weight", "norm.weight", "norm.bias"]
    assert all(torch.equal(kept[k_], copy[k_]) and not torch.equal(again[k_], kept[k_]) for k_ in kept)


# ---- YOLOXHead -----------------------------------------------------------------------------------------------------------------------------------
def _pm(feats):
    return [util.nchw_to_pm(x) for x in feats]


@functools.lru_cache(maxsize=None)
def _head_case(K):
    """One training forward and one backward from random output gradients, twice (the bits must repeat); the oracles once."""
    import basedet.layers as BL
    p0, feats = O.head_state(K), O.head_inputs()
    head = BL.YOLOXHead(K, O.IN_CHANNELS, O.MID)
    init = head.state_dict()
    head.load_state_dict(p0)
    N, P, ld = O.N, sum(h * w for h, w in O.SIZES), (K + 7) // 8 * 8
    g = torch.Generator().manual_seed(50 + K)
    d_cls = torch.zeros(N * P, ld)
    d_cls[:, :K] = 0.05 * torch.randn(N * P, K, generator=g)
    d_bo = torch.zeros(N * P, 8)
    d_bo[:, :5] = 0.05 * torch.randn(N * P, 5, generator=g)
    d_cls, d_bo = d_cls.to(BF), d_bo.to(BF)
    runs = []
    for _ in range(2):
        cls, bo = head.forward_pm(_pm(feats), N, O.SIZES)
        d_feats = head.backward_pm(d_cls.cuda(), d_bo.cuda())
        torch.cuda.synchronize()
        runs.append(dict(cls=cls.clone(), bo=bo.clone(), d_feats=[t.clone() for t in d_feats], grads={k: v.clone() for k, v in head.grads().items()}))
    held = lambda preds, which, k: [getattr(c._store, which)[k].clone() for c in preds]
    pads = dict(cw=held(head.cls_preds, "w", "weight"), cb=held(head.cls_preds, "w", "bias"), cgw=held(head.cls_preds, "g", "weight"),
                cgb=held(head.cls_preds, "g", "bias"), rw=held(head.regobj_preds, "w", "weight"), rb=held(head.regobj_preds, "w", "bias"),
                rgw=held(head.regobj_preds, "g", "weight"), rgb=held(head.regobj_preds, "g", "bias"))
    orc = {}
    for faithful in (False, True):
        p = O.double_params(p0, True)
        xs = [x.double().clone().requires_grad_(True) for x in feats]
        outs = O.head(xs, p, True, faithful)
        c, b = O.pack(*outs)
        ((c * d_cls.double().view(N, P, ld)[..., :K]).sum() + (b * d_bo.double().view(N, P, 8)[..., :5]).sum()).backward()
        orc[faithful] = dict(cls=c.detach(), bo=b.detach(), outs=[[t.detach() for t in l] for l in outs], d_feats=[x.grad for x in xs],
                             grads={k: v.grad for k, v in p.items() if v.requires_grad})
    return dict(head=head, init=init, p0=p0, feats=feats, runs=runs, pads=pads, orc=orc, K=K, N=N, P=P, ld=ld)


KS = [3, 80, 5]


@pytest.mark.parametrize("K", KS)
def test_head_forward_layout_and_pads(K):
    c = _head_case(K)
    r, N, P, ld, head = c["runs"][0], c["N"], c["P"], c["ld"], c["head"]
    assert tuple(r["cls"].shape) == (N * P, ld) and tuple(r["bo"].shape) == (N * P, 8) and r["cls"].dtype == BF
    for k in ("cls", "bo"):
        assert torch.equal(bits_of(r[k]), bits_of(c["runs"][1][k])), k
    # pad slots hold +0 (all bits clear)
    assert int(bits_of(r["cls"])[:, K:].abs().max()) == 0 if ld > K else True
    assert int(bits_of(r["bo"])[:, 5:].abs().max()) == 0
    # the NCHW wrapper returns the same values, level by level at the level's row offset
    logits, offsets, objs = head([x.cuda() for x in c["feats"]])
    c3, b3 = r["cls"].view(N, P, ld).float(), r["bo"].view(N, P, 8).float()
    p0 = 0
    o64, of = c["orc"][False], c["orc"][True]
    for l, (h, w) in enumerate(O.SIZES):
        assert tuple(logits[l].shape) == (N, K, h, w) and tuple(offsets[l].shape) == (N, 4, h, w) and tuple(objs[l].shape) == (N, 1, h, w)
        rows = lambda t, a, b: t[:, p0:p0 + h * w, a:b].reshape(N, h, w, b - a).permute(0, 3, 1, 2)
        assert torch.equal(logits[l], rows(c3, 0, K)) and torch.equal(offsets[l], rows(b3, 0, 4)) and torch.equal(objs[l], rows(b3, 4, 5))
        for name, got, i in (("logits", logits[l], 0), ("offsets", offsets[l], 1), ("objs", objs[l], 2)):
            _ratio(got, o64["outs"][i][l], of["outs"][i][l], f"K={K} level {l} {name}")
        p0 += h * w
    from basedet_amd._lib import BasedetHipError
    with pytest.raises(BasedetHipError):
        head(c["feats"])


@pytest.mark.parametrize("K", KS)
def test_head_backward(K):
    c = _head_case(K)
    r, r2, o64, of = c["runs"][0], c["runs"][1], c["orc"][False], c["orc"][True]
    assert list(r["grads"]) == [k for k in c["p0"] if "running" not in k]
    for k in r["grads"]:
        assert torch.equal(bits_of(r["grads"][k].contiguous()), bits_of(r2["grads"][k].contiguous())), k
        _ratio(r["grads"][k], o64["grads"][k], of["grads"][k], f"K={K} d {k}")
    for l, (h, w) in enumerate(O.SIZES):
        assert torch.equal(bits_of(r["d_feats"][l]), bits_of(r2["d_feats"][l]))
        _ratio(util.pm_to_nchw(r["d_feats"][l], c["N"], h, w), o64["d_feats"][l], of["d_feats"][l], f"K={K} d_feats[{l}]")
    # pad rows of the predictors' weights, biases and gradients are exactly zero
    pd = c["pads"]
    for l in range(len(O.SIZES)):
        for key in ("cw", "cb", "cgw", "cgb"):
            assert int(bits_of(pd[key][l][K:]).abs().sum()) == 0 if c["ld"] > K else True, key
        for key in ("rw", "rb", "rgw", "rgb"):
            assert int(bits_of(pd[key][l][5:]).abs().sum()) == 0, key
    # the NCHW wrapper of the backward is the pixel-major path
    head = c["head"]
    head.load_state_dict(c["p0"])
    outs = head([x.cuda() for x in c["feats"]])
    g = torch.Generator().manual_seed(3)
    d = [[(0.05 * torch.randn(t.shape, generator=g)).cuda() for t in l] for l in outs]
    dx = head.backward(*d)
    assert [tuple(t.shape) for t in dx] == [tuple(x.shape) for x in c["feats"]] and all(bool(torch.isfinite(t).all()) for t in dx)
    head.load_state_dict(c["p0"])


def test_head_state_dict_and_initial_biases():
    import basedet.layers as BL
    c = _head_case(5)
    head, init, p0 = c["head"], c["init"], c["p0"]
    assert list(init) == list(p0) and all(tuple(init[k].shape) == tuple(p0[k].shape) for k in p0)
    prior = -float(np.log((1 - 0.01) / 0.01))
    for l in range(3):
        assert bool((init[f"cls_preds.{l}.bias"] == np.float32(prior)).all()) and bool((init[f"obj_preds.{l}.bias"] == np.float32(prior)).all())
        assert bool((init[f"reg_preds.{l}.bias"] == 0).all())
        assert bool((init[f"stems.{l}.norm.weight"] == 1).all()) and bool((init[f"stems.{l}.norm.running_var"] == 1).all())
    head.load_state_dict(p0)
    back = head.state_dict()
    assert all(torch.equal(back[k], p0[k]) for k in p0)
    other = BL.YOLOXHead(5, O.IN_CHANNELS, O.MID, seed=9)
    feats = _pm(c["feats"])
    a = head.eval().forward_pm(feats, O.N, O.SIZES)
    b = other.eval().forward_pm(feats, O.N, O.SIZES)
    assert not torch.equal(a[0], b[0])
    other.load_state_dict(back)
    b = other.eval().forward_pm(feats, O.N, O.SIZES)
    assert torch.equal(bits_of(a[0]), bits_of(b[0])) and torch.equal(bits_of(a[1]), bits_of(b[1]))
    head.train()
    with pytest.raises(KeyError):
        head.load_state_dict({k: v for k, v in p0.items() if k != "obj_preds.2.bias"})
    with pytest.raises(KeyError):
        head.load_state_dict(dict(p0, extra=torch.zeros(1)))
    with pytest.raises(ValueError):
        head.load_state_dict(dict(p0, **{"stems.0.norm.weight": torch.zeros(O.MID, 1)}))
    head.load_state_dict(p0)


# ---- wiring, end to end ------------------------------------------------------------------------------------------------------------------------
def _gts(K, seed=4, Gmax=4):
    import yolox_oracle as YO
    rng = np.random.default_rng(seed)
    H, W = O.SIZES[0][0] * O.STRIDES[0], O.SIZES[0][1] * O.STRIDES[0]
    gt, num = np.zeros((O.N, Gmax, 5), np.float32), np.array([Gmax, 2], np.int32)
    for n in range(O.N):
        gt[n, :num[n]] = YO._rand_gts(rng, int(num[n]), H, W, K)
    return gt, num


@pytest.mark.parametrize("use_l1", [False, True])
def test_end_to_end_wiring(use_l1):
    """Head -> bd_yolox_assign -> bd_yolox_loss_fwd_bwd -> backward_pm.  The oracle takes the DEVICE's assignment (matched, iou_t, the
    foreground count) as given: SimOTA is discrete and has its own tests."""
    from basedet_amd.models.yolox import yolox_head_step
    K = 5
    c = _head_case(K)
    head, p0, feats = c["head"], c["p0"], c["feats"]
    head.load_state_dict(p0)
    head.train()
    gt, num = _gts(K)
    parts, d_feats, (matched, iou_t, stats) = yolox_head_step(head, _pm(feats), O.N, O.SIZES, torch.from_numpy(gt).cuda(),
                                                              torch.from_numpy(num).cuda(), O.STRIDES, use_l1)
    torch.cuda.synchronize()
    grads = {k: v.clone() for k, v in head.grads().items()}
    m, it, nf = matched.cpu().numpy().reshape(O.N, -1), iou_t.cpu().numpy().reshape(O.N, -1), float(stats.cpu()[0])
    assert nf >= 1 and (m >= 0).sum() == nf
    l64, g64, x64 = O.head_loss_and_grads(feats, p0, K, gt, m, it, nf, use_l1, False)
    lf, gf, xf = O.head_loss_and_grads(feats, p0, K, gt, m, it, nf, use_l1, True)
    got = parts.cpu().double().numpy()
    print("losses (5 iou, obj, cls, l1): device", got, "faithful", lf, "float64", l64)
    if not use_l1:
        assert got[3] == 0.0 and l64[3] == 0.0
    _ratio(got, l64, lf, "the four losses")
    assert set(grads) == set(g64)
    for k in sorted(g64):
        _ratio(grads[k], g64[k], gf[k], f"use_l1={use_l1} d {k}")
    for l, (h, w) in enumerate(O.SIZES):
        _ratio(util.pm_to_nchw(d_feats[l], O.N, h, w), x64[l], xf[l], f"use_l1={use_l1} d_feats[{l}]")
    head.load_state_dict(p0)


def test_short_training_run():
    """Twenty plain SGD steps through params() / repack() on one fixed batch: the total loss after step 20 is below that of step 1 and every
    tensor stays finite.  No value is pinned."""
    from basedet_amd.models.yolox import yolox_head_step
    K, LR = 5, 0.01
    c = _head_case(K)
    head, feats = c["head"], _pm(c["feats"])
    head.load_state_dict(c["p0"])
    head.train()
    gt, num = _gts(K)
    gt, num = torch.from_numpy(gt).cuda(), torch.from_numpy(num).cuda()
    losses = []
    for _ in range(20):
        parts, d_feats, _ = yolox_head_step(head, feats, O.N, O.SIZES, gt, num, O.STRIDES, True)
        losses.append(float(parts.sum().cpu()))
        g = head.grads()
        assert all(bool(torch.isfinite(v).all()) for v in g.values()) and all(bool(torch.isfinite(t.float()).all()) for t in d_feats)
        for k, v in head.params().items():
            v.sub_(LR * g[k])
        head.repack()
    print("losses:", " ".join(f"{v:.4f}" for v in losses))
    assert all(np.isfinite(losses)) and all(bool(torch.isfinite(v).all()) for v in head.state_dict().values())
    assert losses[-1] < losses[0]
    for cp, rp in zip(head.cls_preds, head.regobj_preds):          # the pad rows stayed zero through the optimizer steps
        assert int(bits_of(cp._store.w["weight"][K:]).abs().sum()) == 0 and int(bits_of(rp._store.w["weight"][5:]).abs().sum()) == 0
    head.load_state_dict(c["p0"])
