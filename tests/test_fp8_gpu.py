"""fp8 (OCP e4m3) forward path of BASELINE config 5 (csrc/conv_fp8.hip: v_mfma_scale_f32_16x16x128_f8f6f4).

The reference has no fp8 mode (its mixed-precision hook is fp16 autocast, solver/default_solver.py:66-76), so the tolerances here are
STATED AND MEASURED against fp32: e4m3 keeps 3 mantissa bits (relative rounding error up to 2^-4 per operand), which on these shapes
gives a convolution rel-L2 of 2.5-4 % against the fp32 result of the same bf16 inputs (bound asserted: 6e-2), and the RetinaNet loss
at initialisation within 5e-2 of the fp32 oracle / 3e-2 of the bf16 path.  Structure (operand layout of the 16x16x128 MFMA, taps,
strides, levels, channel tails) is checked EXACTLY: on inputs whose values are e4m3 numbers the kernel must reproduce the fp32
convolution up to the final bf16 rounding (ties aside)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests.util import bf16_round, nchw_to_pm, pm_to_nchw, rel_l2

pytestmark = pytest.mark.gpu

CASES = [
    # N, Cin, Cout, sizes [(H, W)...], R, stride
    (2, 256, 256, [(13, 21)], 3, 1),
    (1, 128, 136, [(20, 17)], 3, 1),                       # Cout tail (136 = 128 + 8)
    (2, 80, 72, [(11, 9)], 3, 1),                          # K tail (80 = 5 x 16, one partial K step), Cout < 128
    (2, 256, 256, [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)], 3, 1),   # the shared-weight head over five pyramid levels
    (1, 512, 256, [(15, 22)], 3, 2),                       # P6-style stride 2 on odd sizes
    (2, 256, 64, [(9, 14)], 1, 1),                         # 1x1
]


def _ops():
    from basedet_amd import ops
    return ops


def _run(ops, N, Cin, Cout, sizes, R, stride, x_lv, w, bias, add_lv=None, relu=False, act_scale=1.0, twin=False):
    pad = R // 2
    gin = ops.Geom(N, [h for h, _ in sizes], [w_ for _, w_ in sizes])
    gout = gin.conv_out(R, stride, pad)
    d = ops.conv_desc(gin, gout, Cin, Cout, R, R, stride, pad)
    x = torch.empty((N, gin.pix_per_img, Cin), dtype=torch.bfloat16)
    for (h, w_), o, xl in zip(sizes, gin.off, x_lv):
        x[:, o:o + h * w_] = xl.permute(0, 2, 3, 1).reshape(N, h * w_, Cin).to(torch.bfloat16)
    x = x.reshape(-1, Cin).cuda()
    add = None
    if add_lv is not None:
        add = torch.empty((N, gout.pix_per_img, Cout), dtype=torch.bfloat16)
        for h, w_, o, al in zip(gout.H, gout.W, gout.off, add_lv):
            add[:, o:o + h * w_] = al.permute(0, 2, 3, 1).reshape(N, h * w_, Cout).to(torch.bfloat16)
        add = add.reshape(-1, Cout).cuda()
    wq = torch.empty((Cout, R * R, Cin), dtype=torch.uint8, device="cuda")
    ws = torch.empty((Cout,), dtype=torch.float32, device="cuda")
    ops.weight_pack_fp8(w.permute(0, 2, 3, 1).contiguous().cuda(), None, Cout, R * R, Cin, act_scale, wq, ws)
    xq = torch.empty((x.numel(),), dtype=torch.uint8, device="cuda")
    ops.quantize_fp8(x, act_scale, xq)
    y = torch.empty((gout.pixels, Cout), dtype=torch.bfloat16, device="cuda")
    flags = (ops.EPI_RELU if relu else 0) | (ops.EPI_ADD_BEFORE if add is not None else 0)
    y8 = torch.zeros((gout.pixels, Cout), dtype=torch.uint8, device="cuda") if twin else None
    ops.conv2d_fwd_fp8(d, xq, wq, ws, None if bias is None else bias.cuda(), y, add=add, flags=flags, y8=y8, q_scale=0.5)
    if twin:
        # the e4m3 twin is e4m3(y_fp32 * q_scale): within half an e4m3 ulp (2^-4 relative; 2^-10 absolute in the subnormals) of y * q_scale
        dec = y8.view(torch.float8_e4m3fn).float().cpu()
        want = (y.float().cpu() * 0.5).clamp(-448, 448)
        assert bool(((dec - want).abs() <= want.abs() * 2.0 ** -4 * 1.01 + 2.0 ** -10 + want.abs() * 2.0 ** -8).all())
    yv = y.float().cpu().view(N, gout.pix_per_img, Cout)
    return [yv[:, o:o + h * w_].reshape(N, h, w_, Cout).permute(0, 3, 1, 2) for h, w_, o in zip(gout.H, gout.W, gout.off)], (wq, ws, xq)


@pytest.fixture(params=[1, 0], ids=["patch", "generic"])
def fp8_kernel(request):
    """1: 3x3 / stride 1 / Cout > 128 launches take the fp8 instance of the staggered patch kernel (conv3x3_pp8.hip); 0: every shape
    through the generic per-tap kernel (conv_fp8.hip)."""
    ops = _ops()
    ops.set_route(fp8_patch=request.param)
    yield request.param
    ops.set_route(fp8_patch=1)


@pytest.mark.parametrize("case", CASES)
def test_fp8_conv_structure_is_exact_on_e4m3_inputs(case, fp8_kernel):
    """Inputs and weights drawn from e4m3 numbers (weights: every channel's largest magnitude is 448 / 64 = 7 so that the per-channel
    scale is the exact power of two 2^-6): products and partial sums are exact in fp32, the only rounding is the bf16 store."""
    ops = _ops()
    N, Cin, Cout, sizes, R, stride = case
    g = torch.Generator().manual_seed(5 + Cin + Cout + R)
    vals = torch.tensor([0.0, 0.25, 0.5, 1.0, 1.5, -0.5, -1.0, 2.0, 3.0, -0.125])
    x_lv = [vals[torch.randint(0, len(vals), (N, Cin, h, w), generator=g)] for h, w in sizes]
    wv = torch.tensor([0.0, 0.875, -0.875, 1.75, -3.5, 0.4375, 7.0, -7.0])
    w = wv[torch.randint(0, len(wv) - 2, (Cout, Cin, R, R), generator=g)]
    w[:, 0, 0, 0] = 7.0                                            # max |w| per output channel = 7 -> scale 7 / 448 = 2^-6
    bias = torch.randn(Cout, generator=g)
    got, (wq, ws, xq) = _run(ops, N, Cin, Cout, sizes, R, stride, x_lv, w, bias, twin=True)
    assert torch.equal(ws.cpu(), torch.full((Cout,), 2.0 ** -6))
    for xl, gl in zip(x_lv, got):
        ref = bf16_round(TF.conv2d(xl, w, bias, stride=stride, padding=R // 2))
        # every product and partial sum is exact in fp32, so only the last bf16 rounding is left: equal up to ties (the MFMA's
        # internal summation order can land a half-way value on the other side) -- at most one bf16 ulp, on at most 1 in 1000 outputs
        bad = gl != ref
        assert float(bad.float().mean()) < 1e-3, float(bad.float().mean())
        assert bool(((gl - ref).abs() <= ref.abs() * 2.0 ** -7 + 1e-6).all()), float((gl - ref).abs().max())


@pytest.mark.parametrize("case", CASES[:5] + [(1, 256, 720, [(25, 42), (13, 21)], 3, 1), (2, 1024, 512, [(10, 12)], 3, 1)])
def test_fp8_conv_tolerance_on_random_data(case, fp8_kernel):
    ops = _ops()
    N, Cin, Cout, sizes, R, stride = case
    g = torch.Generator().manual_seed(11 + Cin + Cout)
    x_lv = [torch.relu(bf16_round(torch.randn(N, Cin, h, w, generator=g))) for h, w in sizes]        # post-ReLU activations
    w = torch.randn(Cout, Cin, R, R, generator=g) / np.sqrt(Cin * R * R)
    bias = torch.randn(Cout, generator=g) * 0.1
    ho = [(h + 2 * (R // 2) - R) // stride + 1 for h, _ in sizes]
    wo = [(w_ + 2 * (R // 2) - R) // stride + 1 for _, w_ in sizes]
    add_lv = [bf16_round(torch.randn(N, Cout, a, b, generator=g)) for a, b in zip(ho, wo)]
    got, _ = _run(ops, N, Cin, Cout, sizes, R, stride, x_lv, w, bias, add_lv=add_lv, relu=True)
    num = den = 0.0
    for xl, al, gl in zip(x_lv, add_lv, got):
        ref = torch.relu(TF.conv2d(xl, w, bias, stride=stride, padding=R // 2) + al)
        num += float((gl - ref).double().pow(2).sum()); den += float(ref.double().pow(2).sum())
    rel = (num / den) ** 0.5
    print(f"fp8 conv rel-L2 vs fp32 {case[:3]} R={R} s={stride}: {rel:.4f}")
    assert rel < 6e-2, rel


def test_quantize_matches_torch_e4m3_cast():
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(4096 * 16, generator=g) * 30).to(torch.bfloat16)
    x[:8] = torch.tensor([0.0, 448.0, -448.0, 1000.0, -1e4, 2.0 ** -9, 2.0 ** -10 * 1.5, 0.017], dtype=torch.bfloat16)
    q = torch.empty((x.numel(),), dtype=torch.uint8, device="cuda")
    ops.quantize_fp8(x.cuda(), 1.0, q)
    want = x.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(q.cpu(), want)
    ops.quantize_fp8(x.cuda(), 0.5, q)
    want = (x.float() * 0.5).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(q.cpu(), want)


def test_retinanet_fp8_step_tolerance():
    """RetinaNet-R18 training step with WEIGHT_DTYPE = fp8_e4m3: same discrete targets; losses within 5e-2 of the fp32 oracle and 3e-2
    of the bf16 path at initialisation; gradients (bf16 backward on fp8-forward activations) cosine >= 0.98 with the bf16 path."""
    from basedet_amd.models import RetinaNet, params as P
    from oracle.model import Oracle
    from tests.test_model_gpu import _setup
    cfg, params, batch = _setup("resnet18", 2, (128, 160))
    names = P.trainable_names(params, cfg.MODEL.BACKBONE.FREEZE_AT)
    ref, aux = Oracle(params, P.oracle_arch(cfg), trainable=names).retinanet_losses(batch)
    m16 = RetinaNet(cfg, params=params)
    out16 = m16(batch)
    m16.backward()
    g16 = m16.reference_grads()
    cfg.MODEL.WEIGHT_DTYPE = "fp8_e4m3"
    cfg.MODEL.FP8_DGRAD = False                   # the forward-only mode (the e5m2 data gradients: test_retinanet_r50_fp8_backward_variants)
    m8 = RetinaNet(cfg, params=params)
    assert any(c.fp8 for c in m8.convs.values()) and not all(c.fp8 for c in m8.convs.values())
    out8 = m8(batch)
    m8.backward()
    torch.cuda.synchronize()
    g8 = m8.reference_grads()
    assert np.array_equal(m8._cur.labels.cpu().numpy(), aux["labels"])
    for k in ("cls_loss", "reg_loss", "total_loss"):
        v8, v16, vr = float(out8[k]), float(out16[k]), float(ref[k].detach())
        print(f"{k}: fp8 {v8:.5f} bf16 {v16:.5f} fp32 oracle {vr:.5f}")
        assert abs(v8 - vr) / abs(vr) < 5e-2 and abs(v8 - v16) / abs(v16) < 3e-2, (k, v8, v16, vr)
    a = torch.cat([g8[n].double().reshape(-1) for n in names])
    b = torch.cat([g16[n].double().reshape(-1) for n in names])
    cos = float(torch.dot(a, b) / (a.norm() * b.norm()))
    print("gradient cosine fp8-forward vs bf16:", cos)
    assert cos > 0.98, cos
    logits8 = m8._cur.logits.float()
    logits16 = m16._cur.logits.float()
    rel = float((logits8 - logits16).norm() / logits16.norm())
    print("logits rel-L2 fp8 vs bf16:", rel)
    assert rel < 8e-2, rel


def test_retinanet_r50_fp8_backward_variants():
    """RetinaNet-R50 (bottlenecks: the dense 1x1 kernel writes conv2's e5m2 gradient twin) with WEIGHT_DTYPE = fp8_e4m3, three backward
    variants on the same fp8 forward: (a) bf16 data gradients (FP8_DGRAD False), (b) fp8 data gradients with cast passes
    (FP8_GRAD_TWINS False), (c) fp8 data gradients with producer-written twins (the default).  Stated tolerances: losses equal to
    1e-5 (same forward); gradient cosine (b) vs (c) >= 0.999 (a twin is rounded from the fp32 accumulator, a cast from its bf16 rounding);
    (b), (c) vs (a) >= 0.985; (a), (b), (c) vs the bf16 model >= 0.98; no non-finite gradient; per-tensor norm ratio in [0.8, 1.25] for every tensor above the e5m2 underflow floor."""
    from basedet_amd.models import RetinaNet, params as P
    from tests.test_model_gpu import _setup
    cfg, params, batch = _setup("resnet50", 2, (160, 192))
    names = P.trainable_names(params, cfg.MODEL.BACKBONE.FREEZE_AT)

    def run(**kw):
        for k in ("WEIGHT_DTYPE", "FP8_DGRAD", "FP8_GRAD_TWINS", "FP8_1X1", "FP8_WGRAD"):
            cfg.MODEL.pop(k, None)
        kw.setdefault("FP8_WGRAD", 0)              # (a) - (d) compare the forward / data-gradient variants on bf16 weight gradients; (e) turns
        for k, v in kw.items():                    # the one-byte weight-gradient kernel on (2: the default since round 4)
            cfg.MODEL[k] = v
        # round-to-nearest gradients here: the variants are compared with each other value by value (stochastic rounding, the training
        # default, is unbiased but lifts tensors that live below the e5m2 floor to the floor's noise level: its own test below)
        cfg.MODEL.FP8_STOCHASTIC_ROUNDING = False
        m = RetinaNet(cfg, params=params)
        out = m(batch)
        m.backward()
        torch.cuda.synchronize()
        g = m.reference_grads()
        return m, {k: float(v) for k, v in out.items()}, g

    m16, l16, g16 = run()
    ma, la, ga = run(WEIGHT_DTYPE="fp8_e4m3", FP8_DGRAD=False)
    mb, lb, gb = run(WEIGHT_DTYPE="fp8_e4m3", FP8_DGRAD=True, FP8_GRAD_TWINS=False)
    mc, lc, gc = run(WEIGHT_DTYPE="fp8_e4m3", FP8_DGRAD=True)
    assert not any(c.fp8_dgrad for c in ma.convs.values()) and any(c.fp8_dgrad for c in mc.convs.values())
    # the bottleneck 1x1s around the fp8 3x3s run on one-byte operands too (forward and data gradient), fed by producer-written twins
    assert any(c.fp8_1x1 for c in mc.convs.values()) and any(c.fp8_1x1_dgrad for c in mc.convs.values())
    assert any(b.out8 is not None for b in mc._cur.blk) and any(b.mid8b is not None for b in mc._cur.blk)
    assert any(b.g_out8 is not None and b.g_out8_ready for b in mc._cur.blk) and any(b.g_mid8a is not None for b in mc._cur.blk)
    md, ld, gd = run(WEIGHT_DTYPE="fp8_e4m3", FP8_DGRAD=True, FP8_1X1=False)         # (d): the 1x1 layers on bf16, as (c) otherwise
    me, le, ge = run(WEIGHT_DTYPE="fp8_e4m3", FP8_DGRAD=True, FP8_WGRAD=2)           # (e): as (c) with the 3x3 weight gradients from the twins (the default)
    assert any(c.fp8_wgrad for c in me.convs.values()) and not any(c.fp8_wgrad for c in mc.convs.values())
    assert not any(c.fp8_1x1 for c in md.convs.values())
    assert mc._cur.g_P8 is not None and mb._cur.g_P8 is None
    assert any(getattr(b, "g_mid8", None) is not None for b in mc._cur.blk)
    for k in la:                                   # the same forward; the loss sums are float atomics (order-dependent last bits)
        assert abs(la[k] - lb[k]) < 1e-5 * abs(la[k]) and abs(la[k] - lc[k]) < 1e-5 * abs(la[k]), (k, la, lb, lc)

    def flat(g):
        return torch.cat([g[n].double().reshape(-1) for n in names])

    def cos(x, y):
        return float(torch.dot(x, y) / (x.norm() * y.norm()))

    f16, fa, fb, fc = flat(g16), flat(ga), flat(gb), flat(gc)
    c_ce = cos(fc, flat(ge))
    print(f"cosine fp8 vs bf16 3x3 weight gradients (same forward, same data gradients): {c_ce:.5f}")
    assert c_ce >= 0.99, c_ce
    c_cd = cos(fc, flat(gd))
    print(f"cosine fp8 1x1 layers vs bf16 1x1 layers (both with fp8 3x3): {c_cd:.5f}; losses {lc} vs {ld}")
    assert c_cd >= 0.99, c_cd
    for k in lc:
        assert abs(lc[k] - ld[k]) < 2e-2 * abs(ld[k]), (k, lc, ld)
    for f in (fa, fb, fc):
        assert bool(torch.isfinite(f).all())
    c_bc, c_ab, c_ac = cos(fb, fc), cos(fa, fb), cos(fa, fc)
    c16 = [cos(f16, f) for f in (fa, fb, fc)]
    print(f"cosine twins vs casts {c_bc:.5f}; fp8-dgrad vs bf16-dgrad {c_ab:.5f} / {c_ac:.5f}; vs the bf16 model {c16}")
    assert c_bc >= 0.999 and c_ab >= 0.985 and c_ac >= 0.985 and min(c16) >= 0.98, (c_bc, c_ab, c_ac, c16)
    # per tensor: e5m2 gradients with the static scale 4096 bottom out at 2^-16 / 4096 = 3.7e-9 (smaller values flush to zero), so a
    # tensor whose whole gradient is below 1e-3 of the global norm may only SHRINK; every other tensor keeps its norm within 25 %
    total = float(fa.norm())
    worst, small = 1.0, []
    for n in names:
        na, nc = float(ga[n].double().norm()), float(gc[n].double().norm())
        if na < 1e-3 * total:
            small.append((n, na, nc))
            assert nc <= 1.25 * na + 1e-12, (n, na, nc)
            continue
        worst = max(worst, nc / na, na / nc)
    print("worst per-tensor gradient norm ratio (twins vs bf16 data gradients):", worst, "| below the floor:", small)
    assert worst < 1.25, worst


DG_CASES = [
    # N, Cin, Cout, sizes, (the data gradient produces Cin channels: the patch kernel needs Cin > 128)
    (2, 256, 256, [(13, 21)]),
    (1, 256, 720, [(12, 20), (6, 10), (3, 5)]),            # the class-score gradient: K = 720 (tail of the sixth 128-channel block)
    (2, 192, 80, [(9, 11)]),                               # channel tail on the produced side (192 of 256), K = 80
]


def _run_dgrad(ops, N, Cin, Cout, sizes, g_lv, w, grad_scale, add_lv=None, mask_lv=None, twin=False):
    geo = ops.Geom(N, [h for h, _ in sizes], [w_ for _, w_ in sizes])
    d = ops.conv_desc(geo, geo, Cin, Cout, 3, 3, 1, 1)

    def pack(levels, C):
        t = torch.empty((N, geo.pix_per_img, C), dtype=torch.bfloat16)
        for (h, w_), o, xl in zip(sizes, geo.off, levels):
            t[:, o:o + h * w_] = xl.permute(0, 2, 3, 1).reshape(N, h * w_, C).to(torch.bfloat16)
        return t.reshape(-1, C).cuda()

    g = pack(g_lv, Cout)
    g8 = torch.empty((g.numel(),), dtype=torch.uint8, device="cuda")
    ops.quantize_bf8(g, grad_scale, g8)
    wq = torch.empty((Cin, 9, Cout), dtype=torch.uint8, device="cuda")
    ws = torch.empty((Cin,), dtype=torch.float32, device="cuda")
    ops.weight_pack_fp8_t(w.permute(0, 2, 3, 1).contiguous().cuda(), None, Cout, 9, Cin, grad_scale, wq, ws)
    dx = torch.empty((geo.pixels, Cin), dtype=torch.bfloat16, device="cuda")
    add = pack(add_lv, Cin) if add_lv is not None else None
    mask = pack(mask_lv, Cin) if mask_lv is not None else None
    flags = (ops.EPI_ADD_BEFORE if add is not None else 0) | (ops.EPI_MASK if mask is not None else 0)
    dx8 = torch.zeros((geo.pixels, Cin), dtype=torch.uint8, device="cuda") if twin else None
    ops.conv2d_dgrad_fp8(d, g8, wq, ws, dx, add=add, mask=mask, flags=flags, dx8=dx8, q_scale=grad_scale)
    if twin:
        dec = dx8.view(torch.float8_e5m2).float().cpu()
        want = (dx.float().cpu() * grad_scale).clamp(-57344, 57344)
        assert bool(((dec - want).abs() <= want.abs() * 2.0 ** -3 * 1.01 + 2.0 ** -17 + want.abs() * 2.0 ** -8).all())
    v = dx.float().cpu().view(N, geo.pix_per_img, Cin)
    return [v[:, o:o + h * w_].reshape(N, h, w_, Cin).permute(0, 3, 1, 2) for (h, w_), o in zip(sizes, geo.off)], ws


@pytest.mark.parametrize("case", DG_CASES)
def test_fp8_dgrad_structure_is_exact_on_representable_inputs(case):
    """Gradient values that are e5m2 numbers (after the power-of-two gradient scale) and weights that are e4m3 numbers with a per-input-
    channel maximum of 7 (scale exactly 2^-6): the fp8 data gradient must reproduce torch's fp32 conv-transpose up to the bf16 store."""
    ops = _ops()
    N, Cin, Cout, sizes = case
    g = torch.Generator().manual_seed(21 + Cin + Cout)
    GS = 2.0 ** 12
    gv = torch.tensor([0.0, 1.0, -1.0, 1.5, 0.5, -0.75, 2.0, -3.0, 0.25]) / GS              # e5m2 numbers / GS
    g_lv = [gv[torch.randint(0, len(gv), (N, Cout, h, w), generator=g)] for h, w in sizes]
    wv = torch.tensor([0.0, 0.875, -0.875, 1.75, -3.5, 0.4375])
    w = wv[torch.randint(0, len(wv), (Cout, Cin, 3, 3), generator=g)]
    w[0, :, 0, 0] = 7.0                                                                     # max over (co, tap) per input channel = 7
    got, ws = _run_dgrad(ops, N, Cin, Cout, sizes, g_lv, w, GS, twin=True)
    assert torch.equal(ws.cpu(), torch.full((Cin,), 2.0 ** -6 / GS))
    for gl, dl in zip(g_lv, got):
        ref = bf16_round(TF.conv_transpose2d(gl, w, stride=1, padding=1))
        bad = dl != ref
        assert float(bad.float().mean()) < 1e-3, float(bad.float().mean())
        assert bool(((dl - ref).abs() <= ref.abs() * 2.0 ** -7 + 1e-9).all()), float((dl - ref).abs().max())


@pytest.mark.parametrize("case", DG_CASES[:2])
def test_fp8_dgrad_tolerance_on_random_data(case):
    """e5m2 keeps two mantissa bits: measured rel-L2 of the data gradient against fp32 on the same bf16 inputs 6-8 % (bound 1.2e-1),
    with the accumulate + ReLU-mask epilogue."""
    ops = _ops()
    N, Cin, Cout, sizes = case
    g = torch.Generator().manual_seed(31 + Cin + Cout)
    g_lv = [bf16_round(torch.randn(N, Cout, h, w, generator=g) * 3e-4) for h, w in sizes]      # gradient-sized values
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cin * 9)
    add_lv = [bf16_round(torch.randn(N, Cin, h, w_, generator=g) * 1e-4) for h, w_ in sizes]
    mask_lv = [torch.relu(bf16_round(torch.randn(N, Cin, h, w_, generator=g))) for h, w_ in sizes]
    got, _ = _run_dgrad(ops, N, Cin, Cout, sizes, g_lv, w, 2.0 ** 12, add_lv=add_lv, mask_lv=mask_lv)
    num = den = 0.0
    for gl, al, ml, dl in zip(g_lv, add_lv, mask_lv, got):
        ref = (TF.conv_transpose2d(gl, w, stride=1, padding=1) + al) * (ml > 0)
        num += float((dl - ref).double().pow(2).sum()); den += float(ref.double().pow(2).sum())
    rel = (num / den) ** 0.5
    print(f"fp8 dgrad rel-L2 vs fp32 {case[:3]}: {rel:.4f}")
    assert rel < 1.2e-1, rel


# ---- the dense 1x1 launches on one-byte operands (csrc/conv1x1.hip: conv1x1_fp8_kernel) -----------------------------------------------
D1_CASES = [
    # N, Cin, Cout, H, W
    (2, 256, 128, 13, 17),
    (1, 1024, 256, 20, 21),
    (1, 128, 544, 9, 11),            # produced-channel tail (544 = 4 x 128 + 32), one K step
    (3, 512, 512, 7, 31),
]


def _exact_weights(Cout, Cin, g, col=False):
    """Weights whose per-channel scale is the exact power of two 2^-6: every output channel (col=False) / input channel (col=True)
    has largest magnitude 7 = 448 / 64, all values e4m3 numbers / 64."""
    wv = torch.tensor([0.0, 0.875, -0.875, 1.75, -3.5, 0.4375])
    w = wv[torch.randint(0, len(wv), (Cout, Cin), generator=g)]
    if col:
        w[0, :] = 7.0
    else:
        w[:, 0] = 7.0
    return w


@pytest.mark.parametrize("case", D1_CASES)
def test_fp8_dense_1x1_forward_is_exact_on_e4m3_inputs(case):
    """bd_conv1x1_fp8 mode 0 on e4m3-valued inputs and power-of-two-scaled weights: exact fp32 sums, so equal to the fp32 convolution up
    to the bf16 store (ties aside); residual + ReLU epilogue; ybits = (y > 0) bit for bit; the e4m3 twin within half an e4m3 ulp."""
    ops = _ops()
    N, Cin, Cout, H, W = case
    g = torch.Generator().manual_seed(31 + Cin + Cout)
    vals = torch.tensor([0.0, 0.25, 0.5, 1.0, 1.5, -0.5, -1.0, 2.0, 3.0, -0.125])
    x = vals[torch.randint(0, len(vals), (N, Cin, H, W), generator=g)]
    w = _exact_weights(Cout, Cin, g)
    bias = torch.randn(Cout, generator=g)
    res = bf16_round(torch.randn(N, Cout, H, W, generator=g))
    geo = ops.single(N, H, W)
    d = ops.conv_desc(geo, geo, Cin, Cout, 1, 1, 1, 0)
    assert ops.conv1x1_fp8_ok(d, 0)
    M = N * H * W
    xp = nchw_to_pm(x)
    xq = torch.empty((M * Cin,), dtype=torch.uint8, device="cuda")
    ops.quantize_fp8(xp, 1.0, xq)
    wq = torch.empty((Cout, 1, Cin), dtype=torch.uint8, device="cuda")
    ws = torch.empty((Cout,), dtype=torch.float32, device="cuda")
    ops.weight_pack_fp8(w.view(Cout, 1, Cin).contiguous().cuda(), None, Cout, 1, Cin, 1.0, wq, ws)
    assert torch.equal(ws.cpu(), torch.full((Cout,), 2.0 ** -6))
    y = torch.empty((M, Cout), dtype=torch.bfloat16, device="cuda")
    ybits = torch.full((Cout // 32, M), -1, dtype=torch.int32, device="cuda")
    y8 = torch.zeros((M, Cout), dtype=torch.uint8, device="cuda")
    ops.conv1x1_fp8(d, 0, xq, wq, ws, bias.cuda(), y, add=nchw_to_pm(res), bits=ybits, y8=y8, q_scale=0.5,
                    flags=ops.EPI_RELU | ops.EPI_ADD_BEFORE)
    ref = bf16_round(torch.relu(TF.conv2d(x, w.view(Cout, Cin, 1, 1), bias) + res))
    got = pm_to_nchw(y, N, H, W)
    bad = got != ref
    assert float(bad.float().mean()) < 1e-3, float(bad.float().mean())
    assert bool(((got - ref).abs() <= ref.abs() * 2.0 ** -7 + 1e-6).all())
    yb = (y.float() > 0).cpu().numpy().reshape(M, Cout // 32, 32)
    want = (yb.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32).T
    assert np.array_equal(ybits.cpu().numpy().view(np.uint32), want)
    dec = y8.view(torch.float8_e4m3fn).float().cpu()
    wantq = (y.float().cpu() * 0.5).clamp(-448, 448)
    assert bool(((dec - wantq).abs() <= wantq.abs() * 2.0 ** -4 * 1.01 + 2.0 ** -10 + wantq.abs() * 2.0 ** -8).all())


@pytest.mark.parametrize("case", D1_CASES)
def test_fp8_dense_1x1_dgrad_is_exact_on_representable_inputs(case):
    """bd_conv1x1_fp8 mode 1 (e5m2 gradients x e4m3 transposed weights, per-input-channel scale 2^-6 / grad_scale): on e5m2-valued
    gradients the data gradient equals the fp32 transposed convolution up to the bf16 store; accumulate + bf16 gate, the bit-packed gate
    gives the same bits, and the e5m2 twin is within half an e5m2 ulp."""
    ops = _ops()
    N, Cin, Cout, H, W = case
    Cin, Cout = Cout, Cin                     # the data gradient's K is Cout: reuse the cases with K % 128 == 0 on that side
    if Cout % 128 != 0 or Cin % 32 != 0:
        pytest.skip("K = Cout must be a multiple of 128")
    g = torch.Generator().manual_seed(41 + Cin + Cout)
    GS = 64.0
    gv = torch.tensor([0.0, 0.25, 0.5, 1.0, 1.5, -0.5, -1.0, 2.0, 3.0, -0.125]) / GS          # g * GS are e5m2 numbers
    gy = gv[torch.randint(0, len(gv), (N, Cout, H, W), generator=g)]
    w = _exact_weights(Cout, Cin, g, col=True)
    acc0 = bf16_round(torch.randn(N, Cin, H, W, generator=g) * 0.1)
    act = torch.relu(bf16_round(torch.randn(N, Cin, H, W, generator=g)))
    geo = ops.single(N, H, W)
    d = ops.conv_desc(geo, geo, Cin, Cout, 1, 1, 1, 0)
    assert ops.conv1x1_fp8_ok(d, 1)
    M = N * H * W
    g8 = torch.empty((M * Cout,), dtype=torch.uint8, device="cuda")
    ops.quantize_bf8(nchw_to_pm(gy), GS, g8)
    wq = torch.empty((Cin, 1, Cout), dtype=torch.uint8, device="cuda")
    ws = torch.empty((Cin,), dtype=torch.float32, device="cuda")
    ops.weight_pack_fp8_t(w.view(Cout, 1, Cin).contiguous().cuda(), None, Cout, 1, Cin, GS, wq, ws)
    assert torch.equal(ws.cpu(), torch.full((Cin,), 2.0 ** -6 / GS))
    dx = nchw_to_pm(acc0).clone()
    dx8 = torch.zeros((M, Cin), dtype=torch.uint8, device="cuda")
    ops.conv1x1_fp8(d, 1, g8, wq, ws, None, dx, add=dx, mask=nchw_to_pm(act), y8=dx8, q_scale=GS, flags=ops.EPI_ADD_BEFORE | ops.EPI_MASK)
    ref = bf16_round((TF.conv_transpose2d(gy, w.view(Cout, Cin, 1, 1)) + acc0) * (act > 0))
    got = pm_to_nchw(dx, N, H, W)
    bad = got != ref
    assert float(bad.float().mean()) < 1e-3, float(bad.float().mean())
    assert bool(((got - ref).abs() <= ref.abs() * 2.0 ** -7 + 1e-6).all())
    ab = (nchw_to_pm(act).float() > 0).cpu().numpy().reshape(M, Cin // 32, 32)
    abits = (ab.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32).T.copy()
    dx2 = nchw_to_pm(acc0).clone()
    ops.conv1x1_fp8(d, 1, g8, wq, ws, None, dx2, add=dx2, maskbits=torch.from_numpy(abits.view(np.int32)).cuda(), flags=ops.EPI_ADD_BEFORE)
    assert torch.equal(dx, dx2)
    dec = dx8.view(torch.float8_e5m2).float().cpu()
    wantq = (dx.float().cpu() * GS).clamp(-57344, 57344)
    assert bool(((dec - wantq).abs() <= wantq.abs() * 2.0 ** -3 * 1.01 + 2.0 ** -17 + wantq.abs() * 2.0 ** -8).all())


def test_fp8_dense_1x1_tolerance_on_random_data():
    """Stated tolerance of the one-byte 1x1 launches on random data: forward rel-L2 <= 6e-2 against the fp32 result of the same bf16
    inputs (e4m3 x e4m3), data gradient <= 1.2e-1 (e5m2 gradients keep 2 mantissa bits)."""
    ops = _ops()
    N, Cin, Cout, H, W = 2, 1024, 256, 20, 21
    g = torch.Generator().manual_seed(7)
    x = torch.relu(bf16_round(torch.randn(N, Cin, H, W, generator=g)))
    w = torch.randn(Cout, Cin, generator=g) / np.sqrt(Cin)
    geo = ops.single(N, H, W)
    d = ops.conv_desc(geo, geo, Cin, Cout, 1, 1, 1, 0)
    M = N * H * W
    xq = torch.empty((M * Cin,), dtype=torch.uint8, device="cuda")
    ops.quantize_fp8(nchw_to_pm(x), 1.0, xq)
    wq = torch.empty((Cout, 1, Cin), dtype=torch.uint8, device="cuda")
    ws = torch.empty((Cout,), dtype=torch.float32, device="cuda")
    ops.weight_pack_fp8(w.view(Cout, 1, Cin).contiguous().cuda(), None, Cout, 1, Cin, 1.0, wq, ws)
    y = torch.empty((M, Cout), dtype=torch.bfloat16, device="cuda")
    ops.conv1x1_fp8(d, 0, xq, wq, ws, None, y)
    rel = rel_l2(pm_to_nchw(y, N, H, W), TF.conv2d(x, w.view(Cout, Cin, 1, 1)))
    print("fp8 1x1 forward rel-L2:", rel)
    assert rel < 6e-2, rel
    GS = 4096.0
    gy = bf16_round(torch.randn(N, Cout, H, W, generator=g) * 1e-3)
    g8 = torch.empty((M * Cout,), dtype=torch.uint8, device="cuda")
    ops.quantize_bf8(nchw_to_pm(gy), GS, g8)
    wqt = torch.empty((Cin, 1, Cout), dtype=torch.uint8, device="cuda")
    wst = torch.empty((Cin,), dtype=torch.float32, device="cuda")
    ops.weight_pack_fp8_t(w.view(Cout, 1, Cin).contiguous().cuda(), None, Cout, 1, Cin, GS, wqt, wst)
    dx = torch.empty((M, Cin), dtype=torch.bfloat16, device="cuda")
    ops.conv1x1_fp8(d, 1, g8, wqt, wst, None, dx)
    reld = rel_l2(pm_to_nchw(dx, N, H, W), TF.conv_transpose2d(gy, w.view(Cout, Cin, 1, 1)))
    print("fp8 1x1 data-gradient rel-L2:", reld)
    assert reld < 1.2e-1, reld


R1X8_SHAPES = [
    # pixels (ragged against the 128-pixel tile), K, produced channels
    (2 * 37 * 53, 256, 256),          # two K steps, two channel tiles: the pixel rows stay resident (XRES)
    (1 * 41 * 29, 512, 544),          # four K steps, produced-channel tail (544 = 4 x 128 + 32), XRES
    (3 * 19 * 23, 1024, 128),         # eight K steps, one channel tile
    (1 * 30 * 17, 384, 1024),         # three K steps (no XRES), eight channel tiles
    (5 * 31 * 17, 128, 512),          # ONE K step per tile: every ring step closes a tile
]


@pytest.mark.parametrize("mode", ["fwd", "dgrad"])
@pytest.mark.parametrize("shape", R1X8_SHAPES)
def test_fp8_ring_1x1_kernel_is_bit_identical_to_the_dense_fp8_kernel(shape, mode):
    """conv1x1_ring_kernel's one-byte form (round 6; bd_conv_desc.route[0] = 5: every legal launch) against conv1x1_fp8_kernel (route[0] = 3) on
    random data, every epilogue the fp8 model issues: the bf16 result, the gate bits and the one-byte twin (to nearest and stochastically
    rounded) must be the same BITS -- same K order, same fp32 epilogue arithmetic."""
    ops = _ops()
    M, K, CO = shape
    g = torch.Generator(device="cuda").manual_seed(5 + M + K + CO)
    H, W = 1, M
    geo = ops.single(1, H, W)
    if mode == "fwd":
        d = ops.conv_desc(geo, geo, K, CO, 1, 1, 1, 0)
        x = torch.relu(torch.randn(M, K, generator=g, device="cuda")).to(torch.bfloat16)
        xq = torch.empty((M * K,), dtype=torch.uint8, device="cuda")
        ops.quantize_fp8(x, 1.0, xq)
        w = (torch.randn(CO, 1, K, generator=g, device="cuda") / np.sqrt(K)).contiguous()
        wq = torch.empty((CO, 1, K), dtype=torch.uint8, device="cuda")
        ws = torch.empty((CO,), dtype=torch.float32, device="cuda")
        ops.weight_pack_fp8(w, None, CO, 1, K, 1.0, wq, ws)
        bias = torch.randn(CO, generator=g, device="cuda")
        res = torch.randn(M, CO, generator=g, device="cuda").to(torch.bfloat16)
        variants = [dict(bias=None, add=None, flags=0, bits=False, twin=False),
                    dict(bias=bias, add=None, flags=ops.EPI_RELU, bits=True, twin=True),
                    dict(bias=bias, add=res, flags=ops.EPI_RELU | ops.EPI_ADD_BEFORE, bits=True, twin=True),
                    dict(bias=None, add=res, flags=ops.EPI_ADD_BEFORE, bits=False, twin=True)]
        for v in variants:
            outs = {}
            for route in (3, 5):
                ops.set_route(dense1x1=route)
                y = torch.full((M, CO), float("nan"), dtype=torch.bfloat16, device="cuda")
                yb = torch.full((CO // 32, M), -1, dtype=torch.int32, device="cuda") if v["bits"] else None
                y8 = torch.full((M, CO), 0x7f, dtype=torch.uint8, device="cuda") if v["twin"] else None
                ops.conv1x1_fp8(d, 0, xq, wq, ws, v["bias"], y, add=v["add"], bits=yb, y8=y8, q_scale=0.75, flags=v["flags"])
                name = ops.L().bd_conv_last_kernel().decode()
                assert name == ("conv1x1_ring_fp8_kernel" if route == 5 else "conv1x1_fp8_kernel"), (route, name)
                outs[route] = (y, yb, y8)
            ops.set_route(dense1x1=None)
            assert bool(torch.isfinite(outs[5][0].float()).all())
            for a, b, what in zip(outs[3], outs[5], ("y", "ybits", "twin")):
                assert (a is None and b is None) or torch.equal(a, b), (v["flags"], what)
    else:
        d = ops.conv_desc(geo, geo, CO, K, 1, 1, 1, 0)          # the data gradient contracts over Cout = K and produces Cin = CO channels
        GS = 2.0 ** 10
        gy = (torch.randn(M, K, generator=g, device="cuda") * 2.0 ** -9).to(torch.bfloat16)
        g8 = torch.empty((M * K,), dtype=torch.uint8, device="cuda")
        ops.quantize_bf8(gy, GS, g8)
        w = (torch.randn(K, 1, CO, generator=g, device="cuda") / np.sqrt(K)).contiguous()          # [Cout][1][Cin]
        wq = torch.empty((CO, 1, K), dtype=torch.uint8, device="cuda")
        ws = torch.empty((CO,), dtype=torch.float32, device="cuda")
        ops.weight_pack_fp8_t(w, None, K, 1, CO, GS, wq, ws)
        acc0 = (torch.randn(M, CO, generator=g, device="cuda") * 0.1).to(torch.bfloat16)
        gate = torch.randint(-2 ** 31, 2 ** 31 - 1, (CO // 32, M), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
        variants = [dict(acc=False, gate=False, twin=False, seed=0),
                    dict(acc=True, gate=True, twin=True, seed=0),
                    dict(acc=False, gate=True, twin=True, seed=0),
                    dict(acc=True, gate=True, twin=True, seed=12345)]
        for v in variants:
            outs = {}
            for route in (3, 5):
                ops.set_route(dense1x1=route)
                ops.fp8_set_stochastic_rounding(v["seed"])
                dx = acc0.clone() if v["acc"] else torch.full((M, CO), float("nan"), dtype=torch.bfloat16, device="cuda")
                dx8 = torch.full((M, CO), 0x7f, dtype=torch.uint8, device="cuda") if v["twin"] else None
                ops.conv1x1_fp8(d, 1, g8, wq, ws, None, dx, add=dx if v["acc"] else None, maskbits=gate if v["gate"] else None, y8=dx8, q_scale=GS,
                                flags=ops.EPI_ADD_BEFORE if v["acc"] else 0)
                name = ops.L().bd_conv_last_kernel().decode()
                assert name == ("conv1x1_ring_fp8_kernel" if route == 5 else "conv1x1_fp8_kernel"), (route, name)
                outs[route] = (dx, dx8)
            ops.set_route(dense1x1=None)
            ops.fp8_set_stochastic_rounding(0)
            assert bool(torch.isfinite(outs[5][0].float()).all())
            for a, b, what in zip(outs[3], outs[5], ("dx", "twin")):
                assert (a is None and b is None) or torch.equal(a, b), (v, what)


# ---- the 3x3 weight gradient on one-byte operands (csrc/conv_wgrad3x3_fp8.hip) -----------------------------------------------------------
WG_CASES = [
    # N, Cin, Cout, sizes
    (2, 64, 64, [(13, 21)]),
    (1, 256, 256, [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]),      # the shared-weight head over five pyramid levels
    (2, 80, 48, [(9, 17)]),                                           # channel tails on both sides (80 = 64 + 16, 48 < 64)
    (1, 256, 720, [(16, 32), (8, 16)]),                               # patch-aligned sizes, the class-score width
]


def _wgrad_fp8(ops, N, Cin, Cout, sizes, x_lv, g_lv, AS, GS, row_scale=None, accumulate=None):
    geo = ops.Geom(N, [h for h, _ in sizes], [w for _, w in sizes])
    d = ops.conv_desc(geo, geo, Cin, Cout, 3, 3, 1, 1)

    def pack(levels, C):
        t = torch.empty((N, geo.pix_per_img, C), dtype=torch.bfloat16)
        for (h, w_), o, xl in zip(sizes, geo.off, levels):
            t[:, o:o + h * w_] = xl.permute(0, 2, 3, 1).reshape(N, h * w_, C).to(torch.bfloat16)
        return t.reshape(-1, C).cuda()

    x, g = pack(x_lv, Cin), pack(g_lv, Cout)
    x8 = torch.empty((x.numel(),), dtype=torch.uint8, device="cuda")
    g8 = torch.empty((g.numel(),), dtype=torch.uint8, device="cuda")
    ops.quantize_fp8(x, AS, x8)
    ops.quantize_bf8(g, GS, g8)
    ws = torch.empty((ops.conv2d_wgrad_fp8_workspace_bytes(d) // 4 + 4,), dtype=torch.float32, device="cuda")
    dw = torch.full((Cout, 3, 3, Cin), 3.0, dtype=torch.float32, device="cuda") if accumulate is None else accumulate.clone()
    ops.conv2d_wgrad_fp8(d, x8, g8, 1.0 / (AS * GS), dw, ws, row_scale=row_scale, accumulate=accumulate is not None)
    return dw.cpu().permute(0, 3, 1, 2)           # OIHW


def _wgrad_ref(x_lv, g_lv, Cin, Cout):
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    tot = 0
    for xl, gl in zip(x_lv, g_lv):
        tot = tot + (TF.conv2d(xl.double(), w, padding=1) * gl.double()).sum()
    tot.backward()
    return w.grad.float()


@pytest.mark.parametrize("case", WG_CASES)
def test_fp8_wgrad3x3_is_exact_on_representable_inputs(case):
    """bd_conv2d_wgrad_fp8 on e4m3-valued activations and e5m2-valued gradients: every product and partial sum is exact in fp32, so the
    weight gradient equals the float64 reference exactly (proves the byte transposing reads, the k <-> pixel permutation, the tap
    shifts, halos, levels, channel tails and the split / reduce)."""
    ops = _ops()
    N, Cin, Cout, sizes = case
    g = torch.Generator().manual_seed(51 + Cin + Cout)
    xv = torch.tensor([0.0, 0.25, 0.5, 1.0, 1.5, -0.5, -1.0, 2.0, 3.0, -0.125])
    gv = torch.tensor([0.0, 0.25, 0.5, 1.0, -0.5, -1.0, 2.0, 0.125]) / 64.0
    x_lv = [xv[torch.randint(0, len(xv), (N, Cin, h, w), generator=g)] for h, w in sizes]
    g_lv = [gv[torch.randint(0, len(gv), (N, Cout, h, w), generator=g)] for h, w in sizes]
    got = _wgrad_fp8(ops, N, Cin, Cout, sizes, x_lv, g_lv, 1.0, 64.0)
    ref = _wgrad_ref(x_lv, g_lv, Cin, Cout)
    assert torch.equal(got, ref), float((got - ref).abs().max())
    # row scale (the folded FrozenBN factor) and accumulate
    rs = torch.rand(Cout, generator=g) + 0.5
    base = torch.randn(Cout, 3, 3, Cin, generator=g).cuda()
    got2 = _wgrad_fp8(ops, N, Cin, Cout, sizes, x_lv, g_lv, 1.0, 64.0, row_scale=rs.cuda(), accumulate=base)
    ref2 = ref * rs.view(-1, 1, 1, 1) + base.cpu().permute(0, 3, 1, 2)
    assert rel_l2(got2, ref2) < 1e-6


def test_fp8_wgrad3x3_tolerance_on_random_data():
    """Stated tolerance on random data: the weight gradient's rel-L2 against the fp64 result of the same bf16 tensors <= 8e-2 (measured
    5.7 %).  On independent random operands the sum itself is a random walk, so the operands' rounding errors (e5m2: 2 mantissa bits)
    do not average out relative to it: this is the per-product error, the worst case for a reduction."""
    ops = _ops()
    N, Cin, Cout, sizes = 2, 256, 256, [(25, 42), (13, 21)]
    g = torch.Generator().manual_seed(3)
    x_lv = [torch.relu(bf16_round(torch.randn(N, Cin, h, w, generator=g))) for h, w in sizes]
    g_lv = [bf16_round(torch.randn(N, Cout, h, w, generator=g) * 1e-3) for h, w in sizes]
    got = _wgrad_fp8(ops, N, Cin, Cout, sizes, x_lv, g_lv, 1.0, 4096.0)
    ref = _wgrad_ref(x_lv, g_lv, Cin, Cout)
    rel = rel_l2(got, ref)
    print("fp8 wgrad rel-L2:", rel)
    assert rel < 8e-2, rel


def test_absmax_and_delayed_gradient_scale():
    """bd_absmax_bf16 against torch (NaNs skipped, negative extremes, accumulation into the slot), and the delayed scaling built on it:
    on a model whose gradients are far below what the static scale resolves, the scale moves up by the probe's reading after
    FP8_AMAX_DELAY steps and every layer agrees on it."""
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = (torch.randn(1 << 16, device="cuda", generator=g) * 3e-4).to(torch.bfloat16)
    x[1234] = -0.0731
    x[77] = float("nan")
    out = torch.zeros(1, dtype=torch.float32, device="cuda")
    ops.absmax_bf16(x, out)
    want = float(torch.nan_to_num(x.float(), nan=0.0).abs().max())
    assert float(out) == want, (float(out), want)
    ops.absmax_bf16((x.float() * 0.5).to(torch.bfloat16), out)          # a smaller tensor does not lower the slot
    assert float(out) == want
    from basedet_amd.models import RetinaNet
    from tests.test_model_gpu import _setup
    cfg, params, batch = _setup("resnet50", 2, (128, 160))
    cfg.MODEL.WEIGHT_DTYPE = "fp8_e4m3"
    cfg.MODEL.FP8_DGRAD = True
    cfg.MODEL.FP8_AMAX_INTERVAL = 3
    cfg.MODEL.FP8_AMAX_DELAY = 1
    cfg.MODEL.FP8_AMAX_HISTORY = 1
    for mode in ("global", "group", "layer"):
        cfg.MODEL.FP8_SCALE_GROUPS = mode
        m = RetinaNet(cfg, params=params)
        assert m.fp8_scaler.delayed and all(c.grad_scale == 4096.0 for c in m.convs.values())
        for k in range(3):
            m(batch); m.backward()
            if k == 1:                                   # staged by the backward of step 1, NOT applied before the weight repack
                assert m.fp8_scaler.staged and all(c.grad_scale == 4096.0 for c in m.convs.values())
            m.repack_trainable()                         # what optimizer.step() does after the SGD launch
        torch.cuda.synchronize()
        assert len(m.fp8_scale_log) == 1 and m.fp8_scaler.staged is None
        t0, t1, amax, scale = m.fp8_scale_log[0]
        assert (t0, t1) == (0, 1) and amax > 0
        am = m.fp8_scaler.amax_host.numpy()
        keys = {}
        for i, c in enumerate(m.fp8_scaler.grad_layers):
            keys[m.fp8_scaler.scale_key(c)] = max(keys.get(m.fp8_scaler.scale_key(c), 0.0), float(am[i]))
        assert (len(keys) == 1) == (mode == "global") and (mode != "group" or set(keys) <= {"head", "fpn", "layer4", "layer3", "layer2"})
        for c in m.fp8_scaler.grad_layers:
            a = keys[m.fp8_scaler.scale_key(c)]
            if a > 0:                                    # every group's largest gradient lands in (2^14, 2^15] of e5m2's range
                t = m.fp8_scaler.amax_target         # 15 for one global scale, 12 (three binades of headroom) per group / layer
                assert t == (15.0 if mode == "global" else 12.0)
                assert 2.0 ** (t - 1) < a * c.grad_scale <= 2.0 ** t and np.log2(c.grad_scale) == np.floor(np.log2(c.grad_scale)), (mode, c.name)
        assert len({c.grad_scale for c in m.output.values()}) == 1        # the FPN output convolutions read ONE twin of dL/dP
        if mode == "global":
            assert all(c.grad_scale == scale for c in m.convs.values())
        else:
            assert len({c.grad_scale for c in m.fp8_scaler.grad_layers}) > 1    # the backbone's gradients are binades below the head's
        # the probe read what the fp8 data gradients consume: no larger than the largest gradient buffer of the step
        assert amax <= float(max(t.float().abs().max() for t in m._cur.g_tower[0] + m._cur.g_tower[1] + [m._cur.g_P])) * 1.0001 + 1e-30
        # a step with the new scales: finite gradients, cosine with the bf16-data-gradient run of the same forward
        m(batch); m.backward(); torch.cuda.synchronize()
        g = m.reference_grads()
        assert all(bool(torch.isfinite(v).all()) for v in g.values()), mode
    cfg.MODEL.pop("FP8_SCALE_GROUPS")


def test_e5m2_stochastic_rounding():
    """bd_conv_desc.sr_seed: (1) unbiased -- the mean of the dequantised values over many seeds approaches the input where
    round-to-nearest is off by up to an eighth; (2) every result is one of the two e5m2 neighbours of the value; (3) a function of (seed,
    element index) only: the same bytes twice, other bytes with another seed; (4) seed 0 restores round-to-nearest exactly."""
    ops = _ops()
    n = 1 << 14
    g = torch.Generator(device="cuda").manual_seed(9)
    x = (torch.rand(n, device="cuda", generator=g) * 3 + 0.6).to(torch.bfloat16)          # (0.6, 3.6): e5m2 steps of 1/8 .. 1/2
    q = torch.empty(n, dtype=torch.uint8, device="cuda")
    try:
        acc = torch.zeros(n, dtype=torch.float64, device="cuda")
        K = 256
        first = None
        for s in range(1, K + 1):
            ops.fp8_set_stochastic_rounding(s * 2654435761 | 1)
            ops.quantize_bf8(x, 1.0, q)
            v = q.view(torch.float8_e5m2).float()
            lo = x.float().to(torch.float8_e5m2)          # round to nearest: one of the two neighbours
            step = torch.where(x.float() < 1.0, 0.125, torch.where(x.float() < 2.0, 0.25, 0.5))
            assert bool(((v - x.float()).abs() < step).all())
            acc += v.double()
            if s == 1:
                first = q.clone()
                ops.quantize_bf8(x, 1.0, q)
                assert torch.equal(q, first)
            if s == 2:
                assert not torch.equal(q, first)
        mean = (acc / K).float()
        err_sr = float((mean - x.float()).abs().mean())
        ops.fp8_set_stochastic_rounding(0)
        ops.quantize_bf8(x, 1.0, q)
        rn = q.view(torch.float8_e5m2).float()
        assert torch.equal(q, x.float().to(torch.float8_e5m2).view(torch.uint8))
        err_rn = float((rn - x.float()).abs().mean())
        print(f"mean |error|: round-to-nearest {err_rn:.4f}, mean of {K} stochastic roundings {err_sr:.4f}")
        assert err_sr < 0.2 * err_rn, (err_sr, err_rn)
    finally:
        ops.fp8_set_stochastic_rounding(0)


@pytest.mark.parametrize("mode", ["fwd", "dgrad"])
def test_fp8_patch_kernel_large_ragged_grid_matches_the_generic_kernel(mode):
    """conv3x3_pp8_kernel on a grid of several rounds: 22 images x five pyramid levels x 264 produced channels = 4 224 tiles -- 16.5 per CU on an
    MI355X, a ragged second channel tile, a last tile that is mostly padding.  (Written for round 6's persistent rebuild of the kernel, where it
    caught an overflowing geometry table; the rebuild was removed -- profiles/r06_pp8_ab.txt -- the test stays.)  Exact-structure operands (every
    product and partial sum exact in fp32): the forward launch must agree with the generic per-tap fp8 kernel (bd_conv_desc.route[3] = generic) up
    to the tie direction of the bf16 store; the data gradient (which only the patch kernel serves) must be bit-identical over two launches and
    reproduce a float64 evaluation at sampled pixels."""
    ops = _ops()
    N, C, CO = 22, 256, 264
    sizes = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
    geo = ops.Geom(N, [h for h, _ in sizes], [w for _, w in sizes])
    g = torch.Generator(device="cuda").manual_seed(99)
    if mode == "fwd":
        d = ops.conv_desc(geo, geo, C, CO, 3, 3, 1, 1)
        vals = torch.tensor([0.0, 0.25, 0.5, 1.0, 1.5, -0.5, -1.0, 2.0, 3.0, -0.125], device="cuda")
        x = vals[torch.randint(0, len(vals), (geo.pixels, C), generator=g, device="cuda")].to(torch.bfloat16)
        wv = torch.tensor([0.0, 0.875, -0.875, 1.75, -3.5, 0.4375], device="cuda")
        w = wv[torch.randint(0, len(wv), (CO, 9, C), generator=g, device="cuda")].contiguous()
        w[:, 0, 0] = 7.0
        xq = torch.empty((x.numel(),), dtype=torch.uint8, device="cuda")
        ops.quantize_fp8(x, 1.0, xq)
        wq = torch.empty((CO, 9, C), dtype=torch.uint8, device="cuda")
        ws = torch.empty((CO,), dtype=torch.float32, device="cuda")
        ops.weight_pack_fp8(w, None, CO, 9, C, 1.0, wq, ws)
        bias = torch.randn(CO, generator=g, device="cuda")
        outs = {}
        for route in (1, 0, 1):
            ops.set_route(fp8_patch=route)
            y = torch.full((geo.pixels, CO), float("nan"), dtype=torch.bfloat16, device="cuda")
            ops.conv2d_fwd_fp8(d, xq, wq, ws, bias, y, flags=ops.EPI_RELU)
            name = ops.L().bd_conv_last_kernel().decode()
            assert (name == "conv3x3_pp8_kernel") == (route == 1), (route, name)
            outs.setdefault(route, []).append(y)
        ops.set_route(fp8_patch=None)
        a, b, gen = outs[1][0], outs[1][1], outs[0][0]
        assert torch.equal(a, b), "two launches of the patch kernel differ"
        assert bool(torch.isfinite(a.float()).all())
        diff = (a.float() - gen.float()).abs()
        assert float((diff > 0).float().mean()) < 1e-3
        assert bool((diff <= gen.float().abs() * 2.0 ** -7 + 1e-6).all()), float(diff.max())
        assert float(a.float().abs().max()) > 1.0
    else:
        d = ops.conv_desc(geo, geo, CO, C, 3, 3, 1, 1)          # the data gradient produces Cin = 264 channels from Cout = 256
        GS = 2.0 ** 12
        gv = torch.tensor([0.0, 1.0, -1.0, 1.5, 0.5, -0.75, 2.0, -3.0, 0.25], device="cuda") / GS
        gy = gv[torch.randint(0, len(gv), (geo.pixels, C), generator=g, device="cuda")].to(torch.bfloat16)
        wv = torch.tensor([0.0, 0.875, -0.875, 1.75, -3.5, 0.4375], device="cuda")
        w = wv[torch.randint(0, len(wv), (C, 9, CO), generator=g, device="cuda")].contiguous()          # [Cout][tap][Cin]
        w[0, 0, :] = 7.0
        g8 = torch.empty((gy.numel(),), dtype=torch.uint8, device="cuda")
        ops.quantize_bf8(gy, GS, g8)
        wq = torch.empty((CO, 9, C), dtype=torch.uint8, device="cuda")
        ws = torch.empty((CO,), dtype=torch.float32, device="cuda")
        ops.weight_pack_fp8_t(w, None, C, 9, CO, GS, wq, ws)
        outs = []
        for _ in range(2):
            dx = torch.full((geo.pixels, CO), float("nan"), dtype=torch.bfloat16, device="cuda")
            ops.conv2d_dgrad_fp8(d, g8, wq, ws, dx, q_scale=GS)
            assert ops.L().bd_conv_last_kernel().decode() == "conv3x3_pp8_kernel"
            outs.append(dx)
        assert torch.equal(outs[0], outs[1])
        assert bool(torch.isfinite(outs[0].float()).all())
        # float64 evaluation at sampled pixels of every level and of the first / last images: dx[n, y, x, ci] = sum g[n, y + 1 - r, x + 1 - s, co] w[co][r][s][ci]
        gyf, wf = gy.double().view(N, geo.pix_per_img, C), w.double().view(C, 3, 3, CO)
        rng = np.random.default_rng(4)
        for n in (0, N - 1, 7):
            for (h, wd), off in zip(sizes, geo.off):
                for _ in range(6):
                    yy, xx = int(rng.integers(0, h)), int(rng.integers(0, wd))
                    acc = torch.zeros(CO, dtype=torch.float64, device="cuda")
                    for r in range(3):
                        for s_ in range(3):
                            sy, sx = yy + 1 - r, xx + 1 - s_
                            if 0 <= sy < h and 0 <= sx < wd:
                                acc += gyf[n, off + sy * wd + sx] @ wf[:, r, s_, :]
                    got = outs[0].double().view(N, geo.pix_per_img, CO)[n, off + yy * wd + xx]
                    assert bool(((got - acc).abs() <= acc.abs() * 2.0 ** -7 + 1e-9).all()), (n, h, yy, xx, float((got - acc).abs().max()))
