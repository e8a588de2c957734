"""csrc/stem_bwd.hip: bd_maxpool3x3s2_bwd and bd_stem_conv7x7_wgrad, the two kernels MODEL.BACKBONE.FREEZE_AT = 0 adds to the step.

Max-pool backward: exact equality with `pool_bwd_ref`, a numpy restatement of the kernel's contract -- a stem pixel takes a window's
gradient iff it is the window's first maximum in row-major order (padding never wins); the taken gradients are summed in fp32 in row-major
window order, gated by stem_out > 0 and rounded to bf16 once.  The restatement is first checked on the CPU against torch.autograd of
TF.max_pool2d on tie-free inputs (integer-valued gradients: every fp32 sum is exact, whatever its order).

Stem weight gradient: rel-L2 <= 2e-3 against float64 from the same bf16 operands, the bound tests/test_conv_gpu.py applies to every bf16
weight gradient (fp32 accumulation of exact bf16 products).

Both kernels run with every operand, output and workspace between guards (tests/test_guard_gpu.py's Run: input guards hold zeros, NaNs and
+-max in turn, outputs start as a sentinel NaN); the three runs must agree bit for bit, which is also the reproducibility check."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import util as U
from tests.util import rel_l2

BF, F32 = torch.bfloat16, torch.float32
C = 64


def pool_bwd_ref(stem, g_pool):
    """stem (N, Hs, Ws, C), g_pool (N, Hq, Wq, C): float32 numpy arrays.  Returns (pool_out, fp32 sums before the gate, gated sums)."""
    N, Hs, Ws, Cn = stem.shape
    Hq, Wq = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    pool = np.zeros((N, Hq, Wq, Cn), np.float32)
    acc = np.zeros_like(stem, dtype=np.float32)
    for py in range(Hq):                  # row-major window order: a pixel's sum grows in the order the kernel documents
        for px in range(Wq):
            pos = [(2 * py - 1 + dy, 2 * px - 1 + dx) for dy in range(3) for dx in range(3)]
            pos = [(y, x) for y, x in pos if 0 <= y < Hs and 0 <= x < Ws]           # padding never wins
            best = np.full((N, Cn), -np.inf, np.float32)
            arg = np.full((N, Cn), -1, np.int64)
            for i, (y, x) in enumerate(pos):
                v = stem[:, y, x]
                upd = v > best                # strict: the FIRST maximum keeps the window
                best = np.where(upd, v, best)
                arg = np.where(upd, i, arg)
            pool[:, py, px] = best
            for i, (y, x) in enumerate(pos):
                acc[:, y, x] = acc[:, y, x] + np.where(arg == i, g_pool[:, py, px], np.float32(0))
    return pool, acc, np.where(stem > 0, acc, np.float32(0))


@pytest.mark.parametrize("N,Hs,Ws", [(2, 9, 11), (1, 8, 8), (1, 1, 1), (1, 2, 3)])
def test_restatement_matches_autograd_on_tie_free_inputs(N, Hs, Ws):
    g = torch.Generator().manual_seed(Hs * 31 + Ws)
    x = (torch.randperm(N * Hs * Ws * 4, generator=g).float() + 1).view(N, 4, Hs, Ws)        # distinct positive values: no ties, open gates
    x.requires_grad_(True)
    y = TF.max_pool2d(x, 3, 2, 1)
    gy = torch.randint(-8, 9, y.shape, generator=g).float()
    (gx,) = torch.autograd.grad(y, x, gy)
    pool, acc, gated = pool_bwd_ref(x.detach().permute(0, 2, 3, 1).numpy(), gy.permute(0, 2, 3, 1).numpy())
    assert np.array_equal(pool, y.detach().permute(0, 2, 3, 1).numpy())
    assert np.array_equal(acc, gx.permute(0, 2, 3, 1).numpy())
    assert np.array_equal(gated, acc)


def _pool_inputs(kind, N, Hs, Ws, seed):
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([0.0, 0.0, 0.5, 1.0, 1.0, 1.5, 2.0, 3.0])              # a handful of bf16 values, zero among them: ties and closed gates
    if kind == "ties":
        stem = vals[torch.randint(0, len(vals), (N, Hs, Ws, C), generator=g)]
    elif kind == "zeros":
        stem = torch.zeros(N, Hs, Ws, C)
    else:                 # the maximum of every window that can see them sits in the padding-adjacent rows and columns
        stem = vals[torch.randint(0, 4, (N, Hs, Ws, C), generator=g)]
        stem[:, 0], stem[:, -1], stem[:, :, 0], stem[:, :, -1] = 4.0, 5.0, 6.0, 7.0
    Hq, Wq = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    gp = torch.randn(N, Hq, Wq, C, generator=g).to(BF).float()
    return stem, gp


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ties", "zeros", "edges"])
@pytest.mark.parametrize("N,Hs,Ws", [(2, 9, 11), (1, 8, 8), (2, 35, 45), (1, 1, 1)])
def test_maxpool_bwd_equals_the_first_maximum_rule(N, Hs, Ws, kind):
    from basedet_amd import ops
    from tests.test_guard_gpu import Run, _same_bits
    stem, gp = _pool_inputs(kind, N, Hs, Ws, Hs * 131 + Ws)
    Hq, Wq = gp.shape[1:3]
    pool, _, want = pool_bwd_ref(stem.numpy(), gp.numpy())
    # the forward kernel's own output is what the step hands over: it must be the restatement's maximum
    pd = torch.empty((N * Hq * Wq, C), dtype=BF, device="cuda")
    ops.maxpool3x3s2_fwd(stem.to(BF).view(-1, C).cuda(), N, Hs, Ws, C, pd)
    assert torch.equal(pd.float().cpu().view(N, Hq, Wq, C), torch.from_numpy(pool))
    results = {}
    for fill in U.FILLS:
        r = Run(fill)
        GP, ST, PO = r.inp("g_pool", gp.to(BF).view(-1, C)), r.inp("stem_out", stem.to(BF).view(-1, C)), r.inp("pool_out", pd.cpu())
        gs = r.out("g_stem", N * Hs * Ws, C, BF)
        ops.maxpool3x3s2_bwd(GP, ST, PO, N, Hs, Ws, C, gs)
        results[fill] = r.finish()
    _same_bits(results, "maxpool3x3s2_bwd")
    got = results["zero"]["g_stem"].view(BF).float().cpu().view(N, Hs, Ws, C)
    assert torch.equal(got, torch.from_numpy(want).to(BF).float())
    if kind == "zeros":
        assert float(got.abs().max()) == 0


def _wgrad_case(N, H, W, seed, single_pixel=False):
    g = torch.Generator().manual_seed(seed)
    Hs, Ws = H // 2, W // 2
    xh = torch.zeros(N, H + 6, W + 8, 4)
    xh[:, 3:3 + H, 4:4 + W, :3] = torch.randn(N, H, W, 3, generator=g)
    xh[..., 3] = torch.randn(N, H + 6, W + 8, generator=g)          # the pad channel holds zeros in the step; whatever it holds is never read into the result
    xh = xh.to(BF)
    if single_pixel:
        gs = torch.zeros(N, Hs, Ws, 64)
        for n in range(N):
            y, x = int(torch.randint(0, Hs, (1,), generator=g)), int(torch.randint(0, Ws, (1,), generator=g))
            gs[n, y, x] = torch.randn(64, generator=g)
    else:
        gs = torch.randn(N, Hs, Ws, 64, generator=g)
    return xh, gs.to(BF)


def _wgrad_ref(xh, gs, H, W, row_scale):
    """float64, OHWI (64, 7, 7, 3): autograd of the 7x7 / stride 2 / pad 3 convolution the forward computes."""
    x = xh[:, 3:3 + H, 4:4 + W, :3].double().permute(0, 3, 1, 2)
    w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    (dw,) = torch.autograd.grad(TF.conv2d(x, w, stride=2, padding=3), w, gs.double().permute(0, 3, 1, 2))
    if row_scale is not None:
        dw = dw * row_scale.double().view(-1, 1, 1, 1)
    return dw.permute(0, 2, 3, 1).contiguous()


# (1, 70, 90): odd Hs, Ws, every tap meets the zero halo; (3, 32, 32): 16-pixel rows, so one 64-pixel K step spans four rows and the last
# step of an image runs into the next one
@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W,single,scaled", [(2, 64, 96, False, False), (1, 70, 90, False, True), (3, 32, 32, False, False),
                                                 (2, 64, 96, True, False), (1, 70, 90, True, True)])
def test_stem_wgrad_against_float64(N, H, W, single, scaled):
    from basedet_amd import ops
    from tests.test_guard_gpu import Run, _same_bits
    xh, gs = _wgrad_case(N, H, W, H * 17 + W + N, single)
    scale = (torch.rand(64, generator=torch.Generator().manual_seed(5)) + 0.5) if scaled else None
    ref = _wgrad_ref(xh, gs, H, W, scale)
    nbytes = ops.stem_conv7x7_wgrad_workspace_bytes(N, H, W)
    assert nbytes > 0
    results = {}
    for fill in U.FILLS:
        r = Run(fill)
        XH, GS = r.inp("x_halo", xh.view(-1, 4)), r.inp("g_stem", gs.view(-1, 64))
        SC = r.inp("row_scale", scale) if scaled else None
        dw, ws = r.out("dw", 64, 147, F32), r.ws("ws", nbytes)
        ops.stem_conv7x7_wgrad(N, H, W, XH, GS, dw, ws, row_scale=SC)
        results[fill] = r.finish()
    _same_bits(results, "stem_conv7x7_wgrad")
    got = results["zero"]["dw"].view(F32).cpu().view(64, 7, 7, 3)
    err = rel_l2(got, ref)
    print(f"stem wgrad N={N} H={H} W={W} single={single} scaled={scaled}: rel-L2 {err:.3e}")
    assert err < 2e-3
    if single:       # every tap on its own: a swapped ky / kx or a wrong stride moves whole taps
        tap = (got.double() - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
        assert float(tap.max()) < 2e-3


@pytest.mark.gpu
def test_stem_wgrad_accumulates_and_refuses_a_short_workspace():
    from basedet_amd import ops
    from basedet_amd._lib import BasedetHipError
    N, H, W = 1, 32, 64
    xh, gs = _wgrad_case(N, H, W, 9)
    ref = _wgrad_ref(xh, gs, H, W, None)
    ws = torch.empty((ops.stem_conv7x7_wgrad_workspace_bytes(N, H, W) // 4,), dtype=F32, device="cuda")
    dw = torch.ones((64, 7, 7, 3), dtype=F32, device="cuda")
    ops.stem_conv7x7_wgrad(N, H, W, xh.cuda(), gs.cuda(), dw, ws, accumulate=True)
    assert rel_l2(dw.cpu() - 1, ref) < 2e-3
    with pytest.raises(BasedetHipError):
        ops.stem_conv7x7_wgrad(N, H, W, xh.cuda(), gs.cuda(), dw, ws[:-1])
    with pytest.raises(BasedetHipError):
        ops.stem_conv7x7_wgrad(N, H + 1, W, xh.cuda(), gs.cuda(), dw, ws)
