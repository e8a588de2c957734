"""csrc/yolox_neck.hip and basedet_amd/layers/yolox_blocks.py against torch and the float64 oracle of tests/yolox_blocks_oracle.py.

Kernels (operands in guarded allocations, every launch twice with the same bits):
  * bd_spp_fwd, bd_cat2_fwd, bd_focus_fwd and the copies of bd_cat2_bwd: bit for bit;
  * bd_spp_bwd: |got - ref| <= one bf16 step of ref + (n - 1) 2^-24 sum |terms|, n the element's term count -- the rounding of the result
    plus the worst case of an fp32 sum of n terms (each of the n - 1 additions is off by at most 2^-24 of a partial sum, and no partial
    sum exceeds sum |terms|); exact where the gradient is made of multiples of 2^-10, whose fp32 sums are exact in any order;
  * the 2x2 sums and accumulations of bd_cat2_bwd: the bits of the fp32 restatement in the stated order, and within one bf16 step of
    float64.
Layers: the ratio form of DESIGN.md 4v, as tests/test_yolox_head_gpu.py -- the device's rel-L2 distance from the float64 oracle is at most
TWICE the distance of the bf16-faithful oracle from it."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import util
import yolox_blocks_oracle as O
from util import bits_of, guarded

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
SPP_LIMIT = 4096


def _pm(x):
    """(N, C, H, W) -> pixel-major (N*H*W, C) bf16, on the host."""
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous().to(BF)


def _nchw(t, n, h, w):
    return t.float().cpu().reshape(n, h, w, -1).permute(0, 3, 1, 2).contiguous()


def _in(data, name, fill="nan"):
    t, h = guarded(data.shape[0], data.shape[1], BF, DEV, fill=fill, name=name)
    h.set(data).snapshot()
    return t, h


def _out(rows, cols, name):
    return guarded(rows, cols, BF, DEV, fill="sentinel", name=name)


# ---- bd_spp_fwd / bd_spp_bwd ---------------------------------------------------------------------------------------------------------------------
SPP_CASES = [(1, 1, 1, 8), (2, 2, 2, 8), (1, 3, 5, 16), (2, 7, 13, 24), (1, 14, 15, 8), (1, 20, 20, 64), (1, 64, 64, 8)]
KINDS = ["distinct", "constant", "silu"]


def _plane(kind, N, H, W, C, seed):
    """x (N, C, H, W) of bf16 values.  distinct: no two pixels of a plane are equal; constant: SiLU's plateau everywhere; silu: the
    bf16-rounded SiLU of a normal sample, which ties constantly near its minimum -0.278."""
    g = torch.Generator().manual_seed(seed)
    if kind == "constant":
        return torch.full((N, C, H, W), -0.2783203125)
    if kind == "silu":
        u = torch.randn(N, C, H, W, generator=g)
        return (u * torch.sigmoid(u)).to(BF).float()
    pos = torch.arange(0x0080, 0x7F80, dtype=torch.int32)          # every positive normal bf16, and their negatives
    pool = torch.cat([pos, pos + 0x8000]).to(torch.int16)
    idx = torch.stack([torch.randperm(pool.numel(), generator=g)[:H * W] for _ in range(N * C)])
    return pool[idx].view(torch.bfloat16).float().view(N, C, H, W)


def _grad(kind, shape, seed):
    """silu: 0.1 N(0, 1) rounded to bf16.  Otherwise multiples of 2^-10 up to 127 / 1024: bf16 values whose sums of up to 276 terms are
    exact in fp32, so the device's sum is the float64 sum and equality after the one rounding is required, not hoped for (+ 0.0: no -0
    among them, which the device would hand on where autograd's sum with its zero-filled buffers gives +0)."""
    g = torch.Generator().manual_seed(seed)
    r = 0.1 * torch.randn(shape, generator=g)
    return r.to(BF).float() if kind == "silu" else torch.clamp(torch.round(r * 1024), -127, 127) / 1024 + 0.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,H,W,C", SPP_CASES)
def test_spp_fwd_and_bwd(N, H, W, C, kind):
    from basedet_amd import ops
    x = _plane(kind, N, H, W, C, seed=H * 31 + W)
    if kind == "distinct":
        assert all(len(set(p.tolist())) == H * W for p in x.view(N * C, H * W))
    g_cat = _grad(kind, (N, 4 * C, H, W), seed=H * 17 + W + 1)
    M = N * H * W
    xb, xh = _in(_pm(x), "x")
    gb, gh = _in(_pm(g_cat), "g_cat", fill="max")
    runs = []
    for _ in range(2):
        cb, ch = _out(M, 4 * C, "cat")
        db, dh = _out(M, C, "d_x")
        ops.spp_fwd(xb, N, H, W, C, cb)
        ops.spp_bwd(gb, xb, N, H, W, C, db)
        torch.cuda.synchronize()
        ch.check(), dh.check()
        runs.append((cb.clone(), db.clone()))
    xh.assert_unchanged(), gh.assert_unchanged()
    assert torch.equal(bits_of(runs[0][0]), bits_of(runs[1][0])) and torch.equal(bits_of(runs[0][1]), bits_of(runs[1][1]))
    # forward: torch's max_pool2d on the same values, bit for bit
    want = torch.cat([x] + [TF.max_pool2d(x, k, 1, k // 2) for k in (5, 9, 13)], 1)
    assert torch.equal(bits_of(runs[0][0].cpu()), bits_of(_pm(want)))
    # backward: the float64 adjoint
    ref, abs_terms, count = (t.numpy() for t in O.spp_bwd_terms(x, g_cat))
    got = _nchw(runs[0][1], N, H, W).double().numpy()
    assert count.max() <= 1 + 25 + 81 + 169
    bound = O.bf16_step(ref) + (count - 1) * 2.0 ** -24 * abs_terms
    worst = float(np.max(np.abs(got - ref) / bound))
    print(f"spp_bwd {kind} N={N} {H}x{W} C={C}: max |got - ref| / bound = {worst:.3f}; most terms in one element {int(count.max())}")
    assert worst <= 1.0
    if kind != "silu":
        assert torch.equal(bits_of(runs[0][1].cpu()), bits_of(_pm(torch.from_numpy(ref))))


def test_spp_plane_limit():
    """64 x 64 = 4096 pixels is taken (SPP_CASES); one pixel more is refused before any launch, as are C % 8 != 0 and null pointers."""
    from basedet_amd import ops
    from basedet_amd._lib import BasedetHipError
    H, W = 17, 241
    assert H * W == SPP_LIMIT + 1
    x = torch.zeros((H * W, 8), dtype=BF, device=DEV)
    cat, ch = _out(H * W, 32, "cat")
    d_x, dh = _out(H * W, 8, "d_x")
    ch.snapshot(), dh.snapshot()
    for fn in (lambda: ops.spp_fwd(x, 1, H, W, 8, cat), lambda: ops.spp_bwd(cat, x, 1, H, W, 8, d_x),
               lambda: ops.spp_fwd(x, 1, 4, 4, 12, cat), lambda: ops.spp_bwd(cat, x, 1, 4, 4, 12, d_x),
               lambda: ops.spp_fwd(None, 1, 4, 4, 8, cat), lambda: ops.spp_bwd(cat, None, 1, 4, 4, 8, d_x),
               lambda: ops.spp_fwd(x, 0, 4, 4, 8, cat)):
        with pytest.raises(BasedetHipError) as e:
            fn()
        assert "(code -1)" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    ch.assert_unchanged(), dh.assert_unchanged()


# ---- bd_cat2_fwd / bd_cat2_bwd -------------------------------------------------------------------------------------------------------------------
CHANNELS = [(8, 8), (24, 8), (8, 264)]
ACCS = [(0, 0), (1, 0), (0, 1), (1, 1)]


def _cat2_case(M, Ca, Cb, up, N, H, W, seed):
    from basedet_amd import ops
    g = torch.Generator().manual_seed(seed)
    Ma = M // 4 if up else M
    a, b = torch.randn(Ma, Ca, generator=g).to(BF), torch.randn(M, Cb, generator=g).to(BF)
    grad = torch.randn(M, Ca + Cb, generator=g).to(BF)
    old_a, old_b = torch.randn(Ma, Ca, generator=g).to(BF), torch.randn(M, Cb, generator=g).to(BF)
    ab, ah = _in(a, "a")
    bb, bh = _in(b, "b", fill="max")
    gb, gh = _in(grad, "g")
    # forward
    if up:
        a_up = a.view(N, H // 2, W // 2, Ca).repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(M, Ca)
    else:
        a_up = a
    want = torch.cat([a_up, b], 1)
    outs = []
    for _ in range(2):
        ob, oh = _out(M, Ca + Cb, "out")
        ops.cat2_fwd(ab, bb, M, Ca, Cb, ob, up, N, H, W)
        torch.cuda.synchronize()
        oh.check()
        outs.append(ob.clone())
    assert torch.equal(bits_of(outs[0]), bits_of(outs[1])) and torch.equal(bits_of(outs[0].cpu()), bits_of(want))
    # backward: the fp32 restatement in the stated order (row-major 2x2 sum, then the held value), and float64
    ga, gbb = grad[:, :Ca].float(), grad[:, Ca:].float()
    if up:
        g4 = ga.view(N, H // 2, 2, W // 2, 2, Ca)
        s32 = ((g4[:, :, 0, :, 0] + g4[:, :, 0, :, 1]) + g4[:, :, 1, :, 0]) + g4[:, :, 1, :, 1]
        s32, s64 = s32.reshape(Ma, Ca), g4.double().sum((2, 4)).reshape(Ma, Ca)
    else:
        s32, s64 = ga, ga.double()
    for acc_a, acc_b in ACCS:
        res = []
        for _ in range(2):
            dab, dah = _out(Ma, Ca, "d_a")
            dbb, dbh = _out(M, Cb, "d_b")
            if acc_a:
                dab.copy_(old_a)
            if acc_b:
                dbb.copy_(old_b)
            ops.cat2_bwd(gb, M, Ca, Cb, dab, dbb, up, N, H, W, acc_a, acc_b)
            torch.cuda.synchronize()
            dah.check(), dbh.check()
            res.append((dab.clone().cpu(), dbb.clone().cpu()))
        assert torch.equal(bits_of(res[0][0]), bits_of(res[1][0])) and torch.equal(bits_of(res[0][1]), bits_of(res[1][1]))
        wa32 = (s32 + old_a.float()) if acc_a else s32
        wb32 = (gbb + old_b.float()) if acc_b else gbb
        assert torch.equal(bits_of(res[0][0]), bits_of(wa32.to(BF))), (acc_a, acc_b, "d_a")
        assert torch.equal(bits_of(res[0][1]), bits_of(wb32.to(BF))), (acc_a, acc_b, "d_b")
        wa64 = s64 + (old_a.double() if acc_a else 0.0)
        wb64 = gbb.double() + (old_b.double() if acc_b else 0.0)
        for got, ref in ((res[0][0], wa64), (res[0][1], wb64)):
            assert np.all(np.abs(got.double().numpy() - ref.numpy()) <= O.bf16_step(ref.numpy()))
    ah.assert_unchanged(), bh.assert_unchanged(), gh.assert_unchanged()


@pytest.mark.parametrize("Ca,Cb", CHANNELS)
@pytest.mark.parametrize("M", [1, 127, 129, 1030])
def test_cat2(M, Ca, Cb):
    _cat2_case(M, Ca, Cb, False, 0, 0, 0, seed=M + Ca + Cb)


@pytest.mark.parametrize("Ca,Cb", CHANNELS)
@pytest.mark.parametrize("N,H,W", [(1, 2, 2), (2, 6, 10), (1, 20, 14)])
def test_cat2_through_the_nearest_upsample(N, H, W, Ca, Cb):
    _cat2_case(N * H * W, Ca, Cb, True, N, H, W, seed=H + W + Ca + Cb)


def test_cat2_refuses_bad_arguments():
    from basedet_amd import ops
    from basedet_amd._lib import BasedetHipError
    a, b = torch.zeros((64, 8), dtype=BF, device=DEV), torch.zeros((64, 8), dtype=BF, device=DEV)
    out, oh = _out(64, 16, "out")
    oh.snapshot()
    for fn in (lambda: ops.cat2_fwd(a, b, 15, 8, 8, out, True, 1, 3, 5),          # odd H
               lambda: ops.cat2_fwd(a, b, 12, 8, 8, out, True, 1, 4, 3),          # odd W
               lambda: ops.cat2_bwd(out, 15, 8, 8, a, b, True, 1, 3, 5),
               lambda: ops.cat2_fwd(a, b, 16, 8, 8, out, True, 1, 4, 2),          # M != N H W
               lambda: ops.cat2_fwd(a, b, 16, 12, 8, out), lambda: ops.cat2_fwd(a, b, 16, 8, 0, out),
               lambda: ops.cat2_bwd(out, 16, 8, 12, a, b), lambda: ops.cat2_fwd(None, b, 16, 8, 8, out),
               lambda: ops.cat2_bwd(out, 16, 8, 8, a, None), lambda: ops.cat2_fwd(a, b, 0, 8, 8, out)):
        with pytest.raises(BasedetHipError) as e:
            fn()
        assert "(code -1)" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    oh.assert_unchanged()
    assert bool((a == 0).all()) and bool((b == 0).all())


# ---- bd_focus_fwd --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W", [(1, 2, 2), (2, 6, 10), (1, 64, 96)])
def test_focus_fwd(N, H, W):
    """Bitwise against the reference's slicing; channels 12-15 are +0; the halo and the layout's fourth channel hold NaN and none of it
    reaches the output."""
    from basedet_amd import ops
    from basedet_amd._lib import BasedetHipError
    g = torch.Generator().manual_seed(H + W)
    img = torch.randn(N, 3, H, W, generator=g).to(BF)
    halo = torch.full((N, H + 6, W + 8, 4), float("nan"), dtype=BF)
    halo[:, 3:3 + H, 4:4 + W, :3] = img.permute(0, 2, 3, 1)
    hb, hh = _in(halo.view(N * (H + 6), (W + 8) * 4), "x_halo")
    Mo = N * (H // 2) * (W // 2)
    outs = []
    for _ in range(2):
        ob, oh = _out(Mo, 16, "out")
        ops.focus_fwd(hb.view(N, H + 6, W + 8, 4), N, H, W, ob)
        torch.cuda.synchronize()
        oh.check()
        outs.append(ob.clone().cpu())
    hh.assert_unchanged()
    want = torch.zeros((Mo, 16), dtype=BF)
    want[:, :12] = _pm(O.space_to_depth(img.float()))
    assert torch.equal(bits_of(outs[0]), bits_of(outs[1])) and torch.equal(bits_of(outs[0]), bits_of(want))
    assert int(bits_of(outs[0])[:, 12:].abs().max()) == 0
    for bad in ((N, H + 1, W), (N, H, W - 1), (0, H, W)):
        with pytest.raises(BasedetHipError):
            ops.focus_fwd(hb, *bad, ob)


# ---- the ratio bound (tests/test_yolox_head_gpu.py) ---------------------------------------------------------------------------------------------
FP32_SUM = 2.0 ** -20


def _ratio(dev, o64, of, name, worst=None):
    dev, o64, of = (torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).double().cpu() for t in (dev, o64, of))
    assert dev.shape == o64.shape, (name, dev.shape, o64.shape)
    if float(o64.abs().max()) == 0.0:
        assert float(dev.abs().max()) == 0.0, name
        return
    d, f = util.rel_l2(dev, o64), util.rel_l2(of, o64)
    if worst is not None:
        worst.append((d / max(2 * f + FP32_SUM, 1e-300), name, d, f))
    # FP32_SUM: where the faithful oracle has no rounding point its distance is exactly 0 while the device adds in fp32 (see
    # tests/test_yolox_head_gpu.py); everywhere else the term is far below the bf16 distances.
    assert d <= 2 * f + FP32_SUM, f"{name}: device {d:.3e} faithful {f:.3e}"


def _report(worst, what):
    r, name, d, f = max(worst)
    print(f"{what}: {len(worst)} quantities, the largest device / bound = {r:.3f} at {name} (device {d:.3e}, faithful {f:.3e})")


# ---- the blocks ------------------------------------------------------------------------------------------------------------------------------------
def _block_case(make, fn, N, C, H, W, seed, image=False, **kw):
    """Forward, one backward and an accumulated one of a block, against the two oracles."""
    from basedet_amd._lib import BasedetHipError
    layer = make()
    p0 = O.random_state(layer._shapes(), seed)
    assert list(layer.state_dict()) == list(p0)
    layer.load_state_dict(p0)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g).to(BF).float()
    z = layer(x.cuda())
    dy = (0.1 * torch.randn(z.shape, generator=g)).to(BF).float()
    d_x = layer.backward(dy.cuda())
    g1 = layer.grads()
    z2 = layer(x.cuda())
    d_x2 = layer.backward(dy.cuda())
    assert torch.equal(z, z2) and all(torch.equal(g1[k], v) for k, v in layer.grads().items())
    layer.backward(dy.cuda(), accumulate=True)
    g2 = layer.grads()
    with pytest.raises(BasedetHipError):
        layer(x)
    worst = []
    (z64,), dx64, g64, _ = O.run(fn, x, p0, dy, False, **kw)
    (zf,), dxf, gf, _ = O.run(fn, x, p0, dy, True, **kw)
    _ratio(z, z64, zf, "output", worst)
    if image:
        assert d_x is None
    else:
        assert torch.equal(d_x, d_x2)
        _ratio(d_x, dx64, dxf, "d_x", worst)
    assert list(g1) == list(g64)
    for k in g64:
        _ratio(g1[k], g64[k], gf[k], f"d {k}", worst)
        _ratio(g2[k], 2 * g64[k], 2 * gf[k], f"accumulated d {k}", worst)
    _report(worst, type(layer).__name__)
    layer.eval()
    layer(x.cuda())
    with pytest.raises(RuntimeError):
        layer.backward(dy.cuda())
    return layer


def test_focus_layer():
    import basedet.layers as BL
    layer = _block_case(lambda: BL.Focus(3, 16, 3), O.focus, 2, 3, 6, 10, seed=1, image=True)
    assert tuple(layer.state_dict()["conv.weight"].shape) == (16, 12, 3, 3) and tuple(layer.params()["conv.weight"].shape) == (16, 12, 3, 3)
    # the pad input channels: zero in the master, exactly zero in the gradient (the input is zero there)
    assert int(bits_of(layer.conv._store.w["weight"][..., 12:]).abs().max()) == 0 and int(bits_of(layer.conv.pad_grad()).abs().max()) == 0
    assert float(layer.conv._store.g["weight"][..., :12].abs().max()) > 0


@pytest.mark.parametrize("H,W", [(2, 2), (5, 3)])
def test_spp_bottleneck_layer(H, W):
    import basedet.layers as BL
    _block_case(lambda: BL.SPPBottleneck(64, 64), O.spp_bottleneck, 2, 64, H, W, seed=2 + H)


@pytest.mark.parametrize("shortcut", [True, False])
def test_bottleneck_layer(shortcut):
    import basedet.layers as BL
    layer = _block_case(lambda: BL.Bottleneck(16, 16, shortcut), O.bottleneck, 2, 16, 6, 10, seed=5 + shortcut, use_add=shortcut)
    assert layer.use_add == shortcut


@pytest.mark.parametrize("C,n,shortcut", [(16, 1, True), (32, 3, False)])
def test_csp_layer(C, n, shortcut):
    import basedet.layers as BL
    _block_case(lambda: BL.CSPLayer(C, C, n, shortcut), O.csp_layer, 2, C, 6, 10, seed=8 + n, n=n, shortcut=shortcut)


# ---- CSPDarknet(0.33, 0.125) and YOLOPAFPN on it -------------------------------------------------------------------------------------------------
DEPTH, WIDTH, FEATS = 0.33, 0.125, ("dark3", "dark4", "dark5")


@functools.lru_cache(maxsize=None)
def _net():
    import basedet.layers as BL
    fpn = BL.YOLOPAFPN(BL.CSPDarknet(DEPTH, WIDTH), DEPTH, WIDTH)
    return fpn, O.random_state(fpn._shapes(), 3)


@functools.lru_cache(maxsize=None)
def _net_case(H, W):
    """The backbone alone and the whole PAFPN: one training forward and backward each on the device, the oracles once."""
    import basedet.layers as BL
    N = 2
    fpn, p0 = _net()
    fpn.train()
    fpn.load_state_dict(p0)
    g = torch.Generator().manual_seed(H + W)
    x = torch.randn(N, 3, H, W, generator=g).to(BF).float()
    halo = BL.Focus.halo(x.cuda())
    sizes = [(H // s, W // s) for s in (8, 16, 32)]
    chans = [fpn.backbone.channels[f] for f in FEATS]
    d = [(0.1 * torch.randn(N, c, h, w, generator=g)).to(BF).float() for c, (h, w) in zip(chans, sizes)]
    d_pm = [_pm(t).cuda() for t in d]
    out = dict(N=N, x=x, d=d, sizes=sizes)
    # the backbone alone
    pb = {k[len("backbone."):]: v for k, v in p0.items() if k.startswith("backbone.")}
    feats, fs = fpn.backbone.forward_pm(halo, N, H, W)
    assert [fs[f] for f in FEATS] == sizes
    fpn.backbone.backward_pm(dict(zip(FEATS, d_pm)))
    torch.cuda.synchronize()
    out["dark"] = ([_nchw(feats[f], N, *fs[f]) for f in FEATS], fpn.backbone.grads())
    fn = lambda x_, p_, **kw: {f: v for f, v in O.darknet(x_, p_, DEPTH, **kw).items() if f in FEATS}
    out["dark_orc"] = {fa: O.run(fn, x, pb, d, fa) for fa in (False, True)}
    # the PAFPN, twice: the bits repeat
    fpn.load_state_dict(p0)
    runs = []
    for _ in range(2):
        fpn.load_state_dict(p0)
        outs, ss = fpn.forward_pm(halo, N, H, W)
        fpn.backward_pm(d_pm)
        torch.cuda.synchronize()
        runs.append(([o.clone() for o in outs], fpn.grads()))
    assert ss == sizes
    out["fpn"], out["fpn2"] = runs
    out["state_after"] = fpn.state_dict()
    out["fpn_orc"] = {fa: O.run(lambda x_, p_, **kw: O.pafpn(x_, p_, DEPTH, **kw), x, p0, d, fa) for fa in (False, True)}
    return out


SIZES = [(64, 64), (96, 160)]


@pytest.mark.parametrize("H,W", SIZES)
def test_csp_darknet(H, W):
    c = _net_case(H, W)
    outs, grads = c["dark"]
    (o64, _, g64, _), (of, _, gf, _) = c["dark_orc"][False], c["dark_orc"][True]
    worst = []
    for i, f in enumerate(FEATS):
        _ratio(outs[i], o64[i], of[i], f, worst)
    assert list(grads) == list(g64)
    for k in g64:
        _ratio(grads[k], g64[k], gf[k], f"d {k}", worst)
    _report(worst, f"CSPDarknet {H}x{W}")


@pytest.mark.parametrize("H,W", SIZES)
def test_yolo_pafpn(H, W):
    c = _net_case(H, W)
    (outs, grads), (outs2, grads2) = c["fpn"], c["fpn2"]
    (o64, _, g64, s64), (of, _, gf, sf) = c["fpn_orc"][False], c["fpn_orc"][True]
    worst = []
    for i, (h, w) in enumerate(c["sizes"]):
        assert torch.equal(bits_of(outs[i]), bits_of(outs2[i]))
        _ratio(_nchw(outs[i], c["N"], h, w), o64[i], of[i], f"pan_out{2 - i}", worst)
    assert list(grads) == list(g64)
    for k in g64:
        assert torch.equal(grads[k], grads2[k]), k
        _ratio(grads[k], g64[k], gf[k], f"d {k}", worst)
    for k in s64:          # the running statistics moved as the oracle's
        _ratio(c["state_after"][k], s64[k], sf[k], k, worst)
    _report(worst, f"YOLOPAFPN {H}x{W}")


def test_pafpn_state_round_trip_eval_and_refusals():
    import basedet.layers as BL
    from basedet_amd._lib import BasedetHipError
    fpn, p0 = _net()
    fpn.load_state_dict(p0)
    back = fpn.state_dict()
    assert list(back) == list(p0) and all(torch.equal(back[k], p0[k]) for k in p0)
    N, H, W = 2, 64, 64
    x = torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(9)).to(BF).float()
    halo = BL.Focus.halo(x.cuda())
    fpn.eval()
    a, sizes = fpn.forward_pm(halo, N, H, W)
    other = BL.YOLOPAFPN(BL.CSPDarknet(DEPTH, WIDTH, seed=77), DEPTH, WIDTH, seed=78).eval()
    b, _ = other.forward_pm(halo, N, H, W)
    assert not torch.equal(a[0], b[0])
    other.load_state_dict(back)
    other.eval()
    b, _ = other.forward_pm(halo, N, H, W)
    assert all(torch.equal(bits_of(s), bits_of(t)) for s, t in zip(a, b))
    assert all(torch.equal(v, p0[k]) for k, v in fpn.state_dict().items())          # eval() moves no running statistic
    # eval() against the oracle with the running statistics
    p = O.double_params(p0)
    o64 = O.pafpn(x.double(), p, DEPTH, training=False, faithful=False)
    of = O.pafpn(x.double(), p, DEPTH, training=False, faithful=True)
    nchw = fpn(x.cuda())
    for i, (h, w) in enumerate(sizes):
        assert torch.equal(nchw[i].cpu(), _nchw(a[i], N, h, w))
        _ratio(nchw[i], o64[i], of[i], f"eval pan_out{2 - i}")
    with pytest.raises(RuntimeError):
        fpn.backward_pm([torch.zeros_like(t) for t in a])
    with pytest.raises(BasedetHipError):
        fpn(x)
    with pytest.raises(ValueError):
        fpn.forward_pm(halo, N, 64, 48)
    with pytest.raises(KeyError):
        fpn.load_state_dict({k: v for k, v in p0.items() if k != "C3_p4.conv3.weight"})
    with pytest.raises(ValueError):
        fpn.load_state_dict(dict(p0, **{"backbone.stem.conv.weight": torch.zeros(8, 16, 3, 3)}))
    fpn.train()
    fpn.load_state_dict(p0)


def test_network_descends():
    """Twenty plain SGD steps of yolox_network_step on one 64 x 64 batch of 2 images with 3 gts each: the total loss after the last step is
    below the first, and every gradient is finite.  No value is pinned."""
    import basedet.layers as BL
    from basedet_amd.models.yolox import yolox_network_step
    N, H, W, K, LR = 2, 64, 64, 3, 0.01
    fpn = BL.YOLOPAFPN(BL.CSPDarknet(DEPTH, WIDTH, seed=5), DEPTH, WIDTH, seed=6)
    head = BL.YOLOXHead(num_classes=K, in_channels=(32, 64, 128), mid_channels=32, seed=7)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((N, 3, H, W)).astype(np.float32))
    halo = BL.Focus.halo(x.cuda())
    gt = np.zeros((N, 3, 5), np.float32)
    for n in range(N):
        for j in range(3):
            cx, cy, w, h = rng.uniform(16, 48), rng.uniform(16, 48), rng.uniform(12, 30), rng.uniform(12, 30)
            gt[n, j] = [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, 1 + (n + j) % K]
    gt, num = torch.from_numpy(gt).cuda(), torch.full((N,), 3, dtype=torch.int32).cuda()
    losses = []
    for _ in range(20):
        parts, _ = yolox_network_step(fpn, head, halo, N, H, W, gt, num, (8, 16, 32), True)
        losses.append(float(parts.sum().cpu()))
        for m in (fpn, head):
            g = m.grads()
            assert all(bool(torch.isfinite(v).all()) for v in g.values())
            for k, v in m.params().items():
                v.sub_(LR * g[k])
            m.repack()
    print("total loss, step 1 .. 20:", " ".join(f"{v:.4f}" for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert int(bits_of(fpn.backbone.stem.conv._store.w["weight"][..., 12:]).abs().max()) == 0          # Focus's pad columns stayed zero
