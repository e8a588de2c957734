"""bd_resize_bilinear_normalize (csrc/image_resize.hip, ops.resize_bilinear_normalize) against the sampling rule evaluated in float64 on the
host: src = max(0, (dst + 0.5) * in / out - 0.5), neighbours floor(src) and min(floor(src) + 1, in - 1), then (x - mean) / std.
torch.nn.functional.interpolate on the float64 CPU tensor cross-checks the oracle itself.

The bound is derived, not measured: |kernel - oracle| <= half a bf16 ulp of |oracle| + 4 * 2^-24 * 255 / std.  Only the kernel's fp32
error can move a value across a bf16 rounding boundary; for values in [0, 255] one fp32 rounding is at most 2^-17, a blend costs the cast
of its fraction (255 * 2^-25) and two roundings (two FMAs), so 6 * 2^-17 after both passes; with mean 0 the subtraction is exact and the
division rounds once more: 7 * 2^-17 / std < 4 * 2^-24 * 255 / std = 7.97 * 2^-17 / std.  The bound cases therefore run with mean 0 (what
YOLOX passes); a non-zero mean is covered by the identity case, which is bit for bit.

Every operand of every launch lives between poisoned guards (tests/util.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from util import guarded

pytestmark = pytest.mark.gpu

N = 2
ZERO = (0.0, 0.0, 0.0)
BD_EINVAL = -1          # include/basedet_hip.h
STDS = ((1.0, 1.0, 1.0), (57.375, 57.12, 58.395))
# (H, W) -> (dst_h, dst_w) in (Hp, Wp)
SHAPES = [((5, 7), (8, 6), (32, 32)),            # mixed: up in y, down in x
          ((64, 64), (96, 96), (96, 96)),
          ((64, 64), (32, 32), (32, 32)),
          ((33, 47), (64, 96), (64, 96)),
          ((40, 40), (40, 40), (64, 64))]        # identity with a pad region


def _images(H, W, seed):
    """Uniform in [0, 255]; image 0 plane 1 is constant, image 1 plane 2 is zero but for a 255 in its last corner."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((N, 3, H, W), generator=g, dtype=torch.float64).mul(255).float()
    x[0, 1] = 200.0
    x[1, 2] = 0.0
    x[1, 2, H - 1, W - 1] = 255.0
    return x


def _taps(out, inp):
    src = np.maximum(0.0, (np.arange(out, dtype=np.float64) + 0.5) * inp / out - 0.5)
    i0 = np.floor(src).astype(np.int64)
    return i0, np.minimum(i0 + 1, inp - 1), src - i0


def oracle(x, dst_h, dst_w, mean, std):
    """float64 (N, 3, dst_h, dst_w): the rule of the module docstring, then the normalise."""
    x = x.double().numpy()
    y0, y1, fy = _taps(dst_h, x.shape[2])
    x0, x1, fx = _taps(dst_w, x.shape[3])
    top = x[:, :, y0][:, :, :, x0] * (1 - fx) + x[:, :, y0][:, :, :, x1] * fx
    bot = x[:, :, y1][:, :, :, x0] * (1 - fx) + x[:, :, y1][:, :, :, x1] * fx
    r = top * (1 - fy)[:, None] + bot * fy[:, None]
    return torch.from_numpy((r - np.asarray(mean).reshape(1, 3, 1, 1)) / np.asarray(std).reshape(1, 3, 1, 1))


def launch(x, dst, pad, mean, std):
    """-> (out bf16 (N, Hp + 6, Wp + 8, 4) on the host, bits of a second launch equal)."""
    from basedet_amd import ops
    (dh, dw), (Hp, Wp) = dst, pad
    xin, hx = guarded(x.numel(), None, torch.float32, "cuda", name="in")
    xin.copy_(x.reshape(-1))
    hx.snapshot()
    outs = []
    for _ in range(2):
        o, ho = guarded(N * (Hp + 6) * (Wp + 8), 4, torch.bfloat16, "cuda", name="x_halo")
        ops.resize_bilinear_normalize(xin.view(x.shape), dh, dw, Hp, Wp, mean, std, o.view(N, Hp + 6, Wp + 8, 4))
        torch.cuda.synchronize()
        ho.check()
        hx.assert_unchanged()
        outs.append(o.view(N, Hp + 6, Wp + 8, 4).cpu())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "two launches differ"
    return outs[0]


def bf16_half_ulp(v):
    """Half the spacing of bf16 at |v| (float64 tensor); the spacing of the smallest normal binade below it."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


@pytest.mark.parametrize("std", STDS, ids=["std1", "std57"])
@pytest.mark.parametrize("src,dst,pad", SHAPES, ids=[f"{s[0]}x{s[1]}to{d[0]}x{d[1]}" for s, d, _ in SHAPES])
def test_against_the_float64_rule(src, dst, pad, std):
    x = _images(*src, seed=src[0] * 100 + dst[0])
    want = oracle(x, *dst, ZERO, std)
    # the oracle against torch's own bilinear rule on the float64 tensor
    ref = TF.interpolate(x.double(), size=dst, mode="bilinear", align_corners=False) / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    assert float((want - ref).abs().max()) <= 1e-9 * 255
    out = launch(x, dst, pad, ZERO, std)
    (dh, dw), (Hp, Wp) = dst, pad
    got = out[:, 3:3 + dh, 4:4 + dw, :3].permute(0, 3, 1, 2).double()
    bound = bf16_half_ulp(want) + 4 * 2.0 ** -24 * 255 / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    err = (got - want).abs()
    print(f"max err / bound = {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    # the constant plane stays constant, to the bit
    assert torch.equal(got[0, 1], torch.full((dh, dw), 200.0 / std[1], dtype=torch.float32).to(torch.bfloat16).double())
    # halo, channel 3 and the pad region: exactly zero (mean 0)
    bits = out.view(torch.int16)
    inner = torch.zeros(out.shape[:3], dtype=torch.bool)
    inner[:, 3:3 + dh, 4:4 + dw] = True
    assert int((bits[~inner] != 0).sum()) == 0
    assert int((bits[..., 3] != 0).sum()) == 0


@pytest.mark.parametrize("mean,std", [(ZERO, STDS[0]), ((103.53, 116.28, 123.675), STDS[1])], ids=["yolox", "resnet"])
def test_identity_is_pad_normalize_bit_for_bit(mean, std):
    from basedet_amd import ops
    x = _images(40, 40, seed=7)
    out = launch(x, (40, 40), (64, 64), mean, std)
    ref = torch.empty((N, 70, 72, 4), dtype=torch.bfloat16, device="cuda")
    ops.pad_normalize(x.cuda(), 64, 64, mean, std, ref)
    assert torch.equal(out.view(torch.int16), ref.cpu().view(torch.int16))


def test_refusals():
    from basedet_amd import ops
    from basedet_amd._lib import BasedetHipError
    x = _images(8, 8, seed=1).cuda()
    out = torch.full((N, 38, 40, 4), 7.0, dtype=torch.bfloat16, device="cuda")
    before = out.clone()
    L = ops.L()
    m, s = ops.f32arr(ZERO), ops.f32arr(STDS[0])
    p = lambda t: t.data_ptr()
    ok = dict(inp=p(x), N=N, H=8, W=8, dh=16, dw=16, Hp=32, Wp=32, mean=m, std=s, out=p(out))
    bad = [dict(inp=None), dict(out=None), dict(mean=None), dict(std=None), dict(inp=p(x) + 2), dict(out=p(out) + 4), dict(N=0), dict(H=0),
           dict(W=-1), dict(dh=0), dict(dw=0), dict(dh=33), dict(dw=40), dict(Hp=48, dh=16), dict(Wp=40, dw=16), dict(Hp=0), dict(Wp=0)]
    for change in bad:
        a = dict(ok, **change)
        rc = L.bd_resize_bilinear_normalize(a["inp"], a["N"], a["H"], a["W"], a["dh"], a["dw"], a["Hp"], a["Wp"], a["mean"], a["std"], a["out"],
                                            None)
        assert rc == BD_EINVAL, change
    torch.cuda.synchronize()
    assert torch.equal(out, before), "a refused call wrote"
    with pytest.raises(BasedetHipError):
        ops.resize_bilinear_normalize(x, 64, 16, 32, 32, ZERO, STDS[0], out)
    ops.resize_bilinear_normalize(x, 16, 16, 32, 32, ZERO, STDS[0], out)          # and the valid call runs
    torch.cuda.synchronize()
    assert not torch.equal(out, before)
