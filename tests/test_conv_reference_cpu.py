"""The float64 reference of tests/util.py (conv_ref_fwd / conv_ref_dgrad / conv_ref_wgrad, decode_maskbits, bound_ratio) against
torch.nn.functional.conv2d and autograd in float64, on the pixel-major multi-level layout the kernels use: several levels at pixel offsets
inside one image (with rows between them that no level covers), stride 2 on odd sizes, 1x1 / 3x3 / 7x7, every epilogue flag, a maskbits
word layout [C/32][M], and the sparse strided data gradient.  The GPU audit (tests/test_conv_audit_gpu.py) trusts this reference."""
import pytest
import torch
import torch.nn.functional as TF

from basedet_amd import ops
from tests import util as U

BF = torch.bfloat16


def _bf(t):
    return t.to(BF)


def _layout(N, levels, C, gen, gap=3):
    """A pixel-major (N * ppi, C) bf16 buffer holding `levels` [(H, W)] per image with `gap` unused rows after each level, its Geom, and
    the per-level NCHW float64 views of its content."""
    off, o = [], 0
    for h, w in levels:
        off.append(o)
        o += h * w + gap
    geom = ops.Geom(N, [h for h, _ in levels], [w for _, w in levels], off, o)
    buf = _bf(torch.randn(N * o, C, generator=gen))
    return buf, geom


def _nchw(buf, geom, i):
    h, w, o = geom.H[i], geom.W[i], geom.off[i]
    return buf.view(geom.N, geom.pix_per_img, -1)[:, o:o + h * w].reshape(geom.N, h, w, -1).permute(0, 3, 1, 2).double()


def _pm(t, buf, geom, i):
    """Write NCHW t into level i of a float64 pixel-major buffer."""
    h, w, o = geom.H[i], geom.W[i], geom.off[i]
    buf.view(geom.N, geom.pix_per_img, -1)[:, o:o + h * w] = t.permute(0, 2, 3, 1).reshape(geom.N, h * w, -1)


def _out_geom(gin, R, stride, pad, gap=5):
    H = [(h + 2 * pad - R) // stride + 1 for h in gin.H]
    W = [(w + 2 * pad - R) // stride + 1 for w in gin.W]
    off, o = [], 0
    for h, w in zip(H, W):
        off.append(o)
        o += h * w + gap
    return ops.Geom(gin.N, H, W, off, o)


def _weights(Cout, R, Cin, gen):
    w = _bf(torch.randn(Cout, R * R, Cin, generator=gen) * 0.1)           # packed forward layout [Cout][RS][Cin]
    wd = w.permute(2, 1, 0).contiguous()                                   # dgrad layout [Cin][RS][Cout]
    oihw = w.double().view(Cout, R, R, Cin).permute(0, 3, 1, 2)
    return w, wd, oihw


def _covered(geom, C):
    m = torch.zeros(geom.N, geom.pix_per_img, C, dtype=torch.bool)
    for i in range(geom.nlev):
        m[:, geom.off[i]:geom.off[i] + geom.H[i] * geom.W[i]] = True
    return m.view(-1, C)


SHAPES = [  # N, Cin, Cout, R, stride, pad, levels
    (2, 16, 24, 3, 1, 1, [(7, 9), (4, 5), (1, 3)]),
    (2, 8, 16, 3, 2, 1, [(9, 11), (5, 6)]),
    (1, 32, 8, 1, 1, 0, [(6, 5), (3, 3)]),
    (2, 16, 32, 1, 2, 0, [(9, 7)]),
    (1, 8, 8, 7, 2, 3, [(13, 11)]),
    (3, 8, 16, 3, 2, 1, [(2, 3)]),
]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("flags", [0, U.EPI_RELU, U.EPI_ADD_BEFORE | U.EPI_RELU, U.EPI_ADD_AFTER])
def test_forward_reference(shape, flags):
    N, Cin, Cout, R, st, pad, levels = shape
    gen = torch.Generator().manual_seed(hash((N, Cin, Cout, R, st, flags)) & 0xFFFF)
    x, gin = _layout(N, levels, Cin, gen)
    gout = _out_geom(gin, R, st, pad)
    d = ops.conv_desc(gin, gout, Cin, Cout, R, R, st, pad)
    w, _, oihw = _weights(Cout, R, Cin, gen)
    bias = torch.randn(Cout, generator=gen)
    add = _bf(torch.randn(gout.pixels, Cout, generator=gen)) if flags & (U.EPI_ADD_BEFORE | U.EPI_ADD_AFTER) else None
    ref, S, exact = U.conv_ref_fwd(d, x, w, bias, add, flags)
    want = torch.full_like(ref, float("nan"))
    want_s = torch.full_like(ref, float("nan"))
    for i in range(gin.nlev):
        v = TF.conv2d(_nchw(x, gin, i), oihw, bias.double(), stride=st, padding=pad)
        s = TF.conv2d(_nchw(x, gin, i).abs(), oihw.abs(), bias.double().abs(), stride=st, padding=pad)
        if add is not None:
            a = _nchw(add, gout, i)
            if flags & U.EPI_ADD_BEFORE:
                v, s = v + a, s + a.abs()
        if flags & U.EPI_RELU:
            v = v.clamp_min(0)
        if add is not None and flags & U.EPI_ADD_AFTER:
            v, s = v + a, s + a.abs()
        _pm(v, want, gout, i)
        _pm(s, want_s, gout, i)
    cov = _covered(gout, Cout)
    assert torch.isnan(ref[~cov]).all() and not torch.isnan(ref[cov]).any()
    torch.testing.assert_close(ref[cov], want[cov], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(S[cov], want_s[cov], rtol=1e-12, atol=1e-12)
    if flags & U.EPI_RELU:
        assert exact[cov].any() and (ref[exact] == 0).all()
    else:
        assert not exact.any()
    # only some images
    r1, _, _ = U.conv_ref_fwd(d, x, w, bias, add, flags, images=[N - 1])
    rows = torch.zeros(N, gout.pix_per_img, dtype=torch.bool)
    rows[N - 1] = True
    rows = rows.view(-1)
    torch.testing.assert_close(r1[rows & cov[:, 0]], ref[rows & cov[:, 0]], rtol=0, atol=0)
    assert torch.isnan(r1[~rows]).all()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("flags", [0, U.EPI_MASK, U.EPI_ADD_BEFORE | U.EPI_MASK, U.EPI_ADD_AFTER | U.EPI_MASK, U.EPI_ADD_BEFORE])
def test_dgrad_reference(shape, flags):
    N, Cin, Cout, R, st, pad, levels = shape
    gen = torch.Generator().manual_seed(hash((N, Cin, Cout, R, st, flags, 1)) & 0xFFFF)
    x, gin = _layout(N, levels, Cin, gen)
    gout = _out_geom(gin, R, st, pad)
    d = ops.conv_desc(gin, gout, Cin, Cout, R, R, st, pad)
    _, wd, oihw = _weights(Cout, R, Cin, gen)
    g = _bf(torch.randn(gout.pixels, Cout, generator=gen))
    add = _bf(torch.randn(gin.pixels, Cin, generator=gen)) if flags & (U.EPI_ADD_BEFORE | U.EPI_ADD_AFTER) else None
    mask = x if flags & U.EPI_MASK else None                   # a signed activation: about half the gate closed
    ref, S, exact = U.conv_ref_dgrad(d, g, wd, add, mask, None, flags)
    want = torch.full_like(ref, float("nan"))
    for i in range(gin.nlev):
        xi = _nchw(x, gin, i).requires_grad_(True)
        TF.conv2d(xi, oihw, stride=st, padding=pad).backward(_nchw(g, gout, i))
        v = xi.grad
        if add is not None and flags & U.EPI_ADD_BEFORE:
            v = v + _nchw(add, gin, i)
        if mask is not None:
            v = v * (_nchw(mask, gin, i) > 0)
        if add is not None and flags & U.EPI_ADD_AFTER:
            v = v + _nchw(add, gin, i)
        _pm(v, want, gin, i)
    cov = _covered(gin, Cin)
    assert torch.isnan(ref[~cov]).all()
    torch.testing.assert_close(ref[cov], want[cov], rtol=1e-12, atol=1e-12)
    assert (S[cov] >= ref[cov].abs() - 1e-12).all()
    if mask is not None:
        closed = cov & ~(x.float() > 0)
        assert torch.equal(exact, closed)
        assert torch.equal(ref[closed], add.double()[closed] if flags & U.EPI_ADD_AFTER else torch.zeros_like(ref[closed]))


def test_maskbits_gate_and_sparse_dgrad():
    """maskbits as the dense 1x1 forward writes them ([C/32][M] words, bit b = channel 32 g + b) gate like the bf16 activation; EPI_SPARSE
    on a 1x1 / stride-2 shortcut leaves the 3 of 4 input pixels no tap reaches exactly as `add` (= dx) holds them."""
    gen = torch.Generator().manual_seed(11)
    N, C, H, W = 2, 64, 7, 9
    act = _bf(torch.randn(N * H * W, C, generator=gen))
    on = act.float() > 0
    words = torch.zeros(C // 32, N * H * W, dtype=torch.int64)
    for b in range(32):
        words |= on[:, b::32].t().to(torch.int64) << b
    bits = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    assert torch.equal(U.decode_maskbits(bits, C), on)
    # channel 31 of a word really is bit 31 (the sign bit of the int32 word)
    assert torch.equal(U.decode_maskbits(bits, C)[:, 31], on[:, 31]) and bool((bits < 0).any())
    gin = ops.single(N, H, W)
    gout = gin.conv_out(1, 2, 0)
    d = ops.conv_desc(gin, gout, C, 32, 1, 1, 2, 0)
    _, wd, oihw = _weights(32, 1, C, gen)
    g = _bf(torch.randn(gout.pixels, 32, generator=gen))
    dx0 = _bf(torch.randn(gin.pixels, C, generator=gen))
    fl = U.EPI_ADD_BEFORE | U.EPI_MASK
    r_bits, _, e_bits = U.conv_ref_dgrad(d, g, wd, dx0, None, bits, fl)
    r_mask, _, e_mask = U.conv_ref_dgrad(d, g, wd, dx0, act, None, fl)
    assert torch.equal(r_bits, r_mask) and torch.equal(e_bits, e_mask)
    r_sp, _, e_sp = U.conv_ref_dgrad(d, g, wd, dx0, act, None, fl | U.EPI_SPARSE)
    reached = torch.zeros(N, H, W, dtype=torch.bool)
    reached[:, ::2, ::2] = True
    reached = reached.view(-1)
    assert torch.equal(r_sp[reached], r_mask[reached])
    assert torch.equal(r_sp[~reached], dx0.double()[~reached]) and bool(e_sp[~reached].all())
    # the reached pixels of a masked 1x1 / stride-2 dgrad: (g W + dx0) * gate
    xi = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    TF.conv2d(xi, oihw, stride=2).backward(g.double().view(N, gout.H[0], gout.W[0], 32).permute(0, 3, 1, 2))
    v = (xi.grad.permute(0, 2, 3, 1).reshape(-1, C) + dx0.double()) * on
    torch.testing.assert_close(r_sp[reached], v[reached], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("accumulate", [False, True])
def test_wgrad_reference(shape, accumulate):
    N, Cin, Cout, R, st, pad, levels = shape
    gen = torch.Generator().manual_seed(hash((N, Cin, Cout, R, st, accumulate, 2)) & 0xFFFF)
    x, gin = _layout(N, levels, Cin, gen)
    gout = _out_geom(gin, R, st, pad)
    d = ops.conv_desc(gin, gout, Cin, Cout, R, R, st, pad)
    g = _bf(torch.randn(gout.pixels, Cout, generator=gen))
    rs = torch.rand(Cout, generator=gen) + 0.5
    dw0 = torch.randn(Cout, R, R, Cin, generator=gen) if accumulate else None
    db0 = torch.randn(Cout, generator=gen) if accumulate else None
    dw, sdw, db, sdb = U.conv_ref_wgrad(d, x, g, rs, dw0, True, db0)
    w = torch.zeros(Cout, Cin, R, R, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    for i in range(gin.nlev):
        TF.conv2d(_nchw(x, gin, i), w, b, stride=st, padding=pad).backward(_nchw(g, gout, i))
    want = w.grad.permute(0, 2, 3, 1) * rs.double().view(-1, 1, 1, 1)
    want_db = b.grad.clone()
    if accumulate:
        want, want_db = want + dw0.double(), want_db + db0.double()
    torch.testing.assert_close(dw, want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(db, want_db, rtol=1e-12, atol=1e-12)
    assert (sdw >= dw.abs() - 1e-12).all() and (sdb >= db.abs() - 1e-12).all()
    dw2, _, db2, _ = U.conv_ref_wgrad(d, x, g, None)
    assert db2 is None
    torch.testing.assert_close(dw2, w.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


def test_bound_ratio():
    ref = torch.tensor([1.0, -2.0, 0.0, float("nan"), 4.0], dtype=torch.float64)
    S = torch.tensor([2.0, 2.0, 1.0, 1.0, 4.0], dtype=torch.float64)
    got = torch.tensor([1.0 + 2 ** -8, -2.0, 2 ** -17, 7.0, 4.0])
    exact = torch.tensor([False, False, False, False, True])
    r = U.bound_ratio(got, ref, S, 2 ** -8, 2 ** -16, exact)
    assert r[0] == pytest.approx(2 ** -8 / (2 ** -8 + 2 ** -15)) and r[1] == 0 and r[2] == 0.5 and r[3] == 0 and r[4] == 0
    got[4] = 4.0 + 2 ** -6
    assert U.bound_ratio(got, ref, S, 2 ** -8, 2 ** -16, exact)[4] == float("inf")
