"""Guard-band tests: no launch reads or writes outside the rows it owns.

Every operand of every launch here -- activations, packed weights, bias, row_scale, residual / mask tensors, outputs, fp32 gradients,
statistics, workspaces -- lives between two guards inside one allocation the test owns (tests/util.py: guarded, gapped_geom); every
workspace has exactly the bytes its *_workspace_bytes function returns.  Each launch runs three times, with the guards and gaps of its
INPUTS holding zeros, quiet NaNs and +-max (the largest finite value, sign alternating: fmaxf drops a NaN, and 0 x NaN is NaN); outputs
and their guards start as a sentinel NaN.  After every run: output guards and gap rows still hold the sentinel, inputs (guards, gaps and
data) hold the bits they held, no sentinel is left in a row the launch owns, and the three runs agree bit for bit.  The zero-fill run is
then compared with a torch fp32 reference per level, at the tolerance of the entry point's own test.  Every launch uses a valid descriptor:
the guards only make a stray access visible.

Layout contract of each entry point, and the line that decides it:

  entry point                                   layout   decided by
  conv2d_fwd / _dgrad / _wgrad / _wgrad_bias    gapped   bd_conv_desc.in_off / out_off / *_pix_per_img (ops.conv_desc)
  ... their dense 1x1 kernels (conv1x1*.hip,    dense    conv_igemm.hip is_dense_1x1(), conv1x1.hip bd_conv1x1_s2_launch() and
      conv_wgrad1x1*.hip)                                conv_wgrad1x1_ring.hip bd_wgrad1x1r_eligible(): one level from offset 0 with
                                                         pix_per_img == H * W, else the launch goes to the generic kernels.  The 1x1
                                                         cases run both ways: dense (those kernels) and gapped (the generic ones)
  conv2d_fwd_gnstats, groupnorm_fwd_parts       dense    norm.hip level_of(): levels packed from offset 0 (the parts are indexed by it)
  conv1x1_thin_fwd / _bwd                       dense    (M, C) rows, no geometry argument
  bottleneck_fwd                                dense    (N, H, W) arguments only
  upsample2x_add_fwd / _bwd                     gapped   ppi / off arguments of both tensors (ops.upsample2x_add_fwd)
  colsum_bf16                                   gapped   n, ppi, off, cnt arguments (ops.colsum_bf16, geom=)
  maxpool3x3s2_fwd, stem_conv7x7_fwd,
  stem_pool_fwd, pad_normalize                  dense    (N, H, W) arguments only
  relu / add / relu_bwd / f32_to_bf16           dense    element count only
  groupnorm_fwd / _bwd                          dense    norm.hip level_of(): the kernels walk all N * pix_per_img rows
  fcos_offsets_fwd / _bwd                       dense    norm.hip level_of(): same walk
The dense entry points get outer guards only: forcing gaps on them would be an invalid descriptor, not a finding.

Exceptions to "no sentinel left in the rows the launch owns": none for the launches below (fcos_offsets_bwd writes its padding channels
5 .. 7 as zeros, conv1x1_thin_bwd writes the rows behind cout_real as zeros).

Findings: none.  Every launch below came back clean under all three fills, so no kernel or workspace formula was changed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import util as U
from tests.util import bf16_round, oihw_to_ohwi, pack_weights, rel_l2

pytestmark = pytest.mark.gpu

BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
TOL = 1e-2                               # tests/test_conv_gpu.py
LEVELS = [(9, 17), (5, 3), (1, 2)]       # one full 8x16 / 4x16 patch plus one overhanging row and column; smaller than a patch; two pixels


def _ops():
    from basedet_amd import ops
    return ops


def _last():
    return _ops().L().bd_conv_last_kernel().decode()


class Run:
    """The operands of launches made under one input fill.  inp: data the launch only reads (guards and gaps hold the fill; every bit
    must come back).  out: sentinel everywhere; `own` (row mask, default: the rows some level owns, all rows without gaps) must be
    written, every other row keeps its bits.  inout: as out, with data in place (accumulate targets, the lateral of upsample2x_add_fwd).
    ws: a workspace of exactly nbytes bytes (only its guards are checked)."""

    def __init__(self, fill):
        self.fill = fill
        self.ins, self.outs = [], []

    def inp(self, name, data, kind=None, fmt=None):
        rows, cols = (data.shape[0], None) if data.dim() == 1 else (data.shape[0], data.shape[1])
        t, h = U.guarded(rows, cols, data.dtype, "cuda", fill=self.fill, name=name, fmt=fmt)
        h.set(data)
        if kind is not None:
            h.set_gaps(kind)
        h.snapshot()
        self.ins.append(h)
        return t

    def out(self, name, rows, cols, dtype, kind=None, own=None, data=None):
        t, h = U.guarded(rows, cols, dtype, "cuda", name=name)
        if data is not None:
            h.set(data)
        if kind is not None:
            h.set_gaps(kind)
        if own is None:
            own = torch.ones(rows, dtype=torch.bool) if kind is None else kind == 0
        h.own = own.cuda()
        h.written = data is None
        h.snapshot()
        self.outs.append(h)
        return t

    def inout(self, name, data, kind=None, own=None):
        rows, cols = (data.shape[0], None) if data.dim() == 1 else (data.shape[0], data.shape[1])
        return self.out(name, rows, cols, data.dtype, kind, own, data=data)

    def ws(self, name, nbytes):
        t, h = U.guarded(max(int(nbytes), 1), None, U8, "cuda", name=name)
        t = t[:int(nbytes)]
        h.own, h.written = torch.ones(max(int(nbytes), 1), dtype=torch.bool, device="cuda"), False
        h.snapshot()
        self.outs.append(h)
        return t

    def finish(self):
        """Check everything since the last finish(); returns {name: bits of the rows the launch owns} of the outputs."""
        torch.cuda.synchronize()
        res = {}
        for h in self.ins:
            h.assert_unchanged()
        for h in self.outs:
            h.check()
            body = U.bits_of(h.t)
            snap = h._snap.view(2 * h.g + h.rows, h.cols)[h.g:h.g + h.rows].view_as(body)
            other = ~h.own
            if bool(other.any()):
                same = body[other] == snap[other]
                assert bool(same.all()), f"{h.name}: {int((~same).sum())} element(s) changed in rows the launch does not own"
            if h.name.startswith("ws"):
                continue
            got = h.t[h.own]
            if h.written:
                left = U.count_sentinel(got)
                assert left == 0, f"{h.name}: {left} element(s) of the rows the launch owns were not written"
            res[h.name] = U.bits_of(got).clone()
        self.outs = []
        return res


def _same_bits(results, what):
    """results: {fill: {name: bits}}: the three runs agree bit for bit."""
    base = results[U.FILLS[0]]
    for fill in U.FILLS[1:]:
        for name, bits in results[fill].items():
            diff = int((bits != base[name]).sum())
            assert diff == 0, f"{what}: {name} differs between the zero and the {fill} fill in {diff} element(s)"


def _lvl(t, geom, i):
    """Level i of a pixel-major CPU tensor (N * ppi, C) as fp32 NCHW."""
    h, w, o = geom.H[i], geom.W[i], geom.off[i]
    return t.view(geom.N, geom.pix_per_img, -1)[:, o:o + h * w].reshape(geom.N, h, w, -1).permute(0, 3, 1, 2).float()


def _owned_to_levels(bits_owned, dtype, geom, kind):
    """The owned rows a Run returned -> the full (N * ppi, C) CPU tensor with zeros in the gaps."""
    C = bits_owned.shape[1]
    full = torch.zeros(geom.pixels, C, dtype=dtype)
    own = torch.ones(geom.pixels, dtype=torch.bool) if kind is None else kind == 0
    full[own] = bits_owned.view(dtype).cpu()
    return full


# ---- a. descriptor-driven convolutions -------------------------------------------------------------------------------------------------
ROUTES = (0, 3, 3 | 64 | 512, 3 | 64 | 256)         # the patch3x3 words of tests/test_conv_gpu.py::test_conv_fwd_dgrad_wgrad
CONV_CASES = {
    # name: (N, levels, Cin, Cout, R, stride, pad, gapped, directions, extra dense-1x1 modes)
    "ml_256_256": (2, LEVELS, 256, 256, 3, 1, 1, True, "fdw", ()),
    "ml_200_136": (2, LEVELS, 200, 136, 3, 1, 1, True, "fdw", ()),          # K tails
    "ml_64_72": (2, LEVELS, 64, 72, 3, 1, 1, True, "fdw", ()),
    "ml_32_64": (2, LEVELS, 32, 64, 3, 1, 1, True, "fdw", ()),              # BK = 32
    "ml_256_40": (2, LEVELS, 256, 40, 3, 1, 1, True, "fdw", ()),
    "ml_256_720": (2, LEVELS, 256, 720, 3, 1, 1, True, "fdw", ()),
    "s2_128_128": (2, [(27, 31)], 128, 128, 3, 2, 1, True, "fdw", ()),      # stride 2 on odd sizes; gaps between the images
    # dense 1x1 modes 2 and 5 (256^2 tile, ring kernel everywhere): the only way to conv1x1_big_kernel / conv1x1_ring_kernel below 32 768 pixels
    "p1_64_256": (2, [(17, 23)], 64, 256, 1, 1, 0, False, "fdw", (2, 5)),
    "p1_2048_512": (2, [(5, 7)], 2048, 512, 1, 1, 0, False, "fdw", ()),
    "p1s2_256_512": (2, [(17, 19)], 256, 512, 1, 2, 0, False, "fw", ()),    # forward and wgrad only, as tests/test_conv_gpu.py
    # the same 1x1 shapes with a gap behind every image: the generic kernels' 1x1 path, and the image boundary on its own
    "p1_64_256_gap": (2, [(17, 23)], 64, 256, 1, 1, 0, True, "fdw", ()),
    "p1_2048_512_gap": (2, [(5, 7)], 2048, 512, 1, 1, 0, True, "fdw", ()),
    "p1s2_256_512_gap": (2, [(17, 19)], 256, 512, 1, 2, 0, True, "fw", ()),
}
# every bf16 name bd_note_kernel reports from bd_conv2d_fwd / _dgrad / _wgrad / _wgrad_bias
CONV_KERNELS = {"conv3x3_pp_kernel", "conv3x3_pp128_kernel", "conv3x3_patch_kernel", "conv_igemm_kernel<32>", "conv_igemm_kernel<64>",
                "conv1x1_dense_kernel", "conv1x1_big_kernel", "conv1x1_ring_kernel", "conv_wgrad3x3_ring_kernel", "conv_wgrad3x3_kernel",
                "conv_wgrad1x1_ring_kernel", "conv_wgrad1x1_kernel", "conv_wgrad_kernel"}
_SEEN = {}                               # case name -> {(direction, route words): kernel name}


def _conv_geoms(ops, N, levels, R, stride, pad, gapped):
    out_levels = [((h + 2 * pad - R) // stride + 1, (w + 2 * pad - R) // stride + 1) for h, w in levels]
    if gapped:
        gin, kin = U.gapped_geom(N, levels)
        gout, kout = U.gapped_geom(N, out_levels, gap=U.GUARD_MIN_ROWS + 5)        # other offsets than the input's
        return gin, kin, gout, kout
    return ops.Geom(N, [h for h, _ in levels], [w for _, w in levels]), None, ops.Geom(N, [h for h, _ in out_levels], [w for _, w in out_levels]), None


def _run_conv_case(name):
    if name in _SEEN:
        return _SEEN[name]
    ops = _ops()
    N, levels, Cin, Cout, R, stride, pad, gapped, dirs, dense_modes = CONV_CASES[name]
    gin, kin, gout, kout = _conv_geoms(ops, N, levels, R, stride, pad, gapped)
    d = ops.conv_desc(gin, gout, Cin, Cout, R, R, stride, pad)
    gen = torch.Generator().manual_seed(1234 + Cin + Cout + levels[0][0])
    rnd = lambda *s: bf16_round(torch.randn(*s, generator=gen))
    x, gy = rnd(gin.pixels, Cin).to(BF), rnd(gout.pixels, Cout).to(BF)
    res, addx, maskx = rnd(gout.pixels, Cout).to(BF), rnd(gin.pixels, Cin).to(BF), rnd(gin.pixels, Cin).to(BF)
    w = bf16_round(torch.randn(Cout, Cin, R, R, generator=gen) / np.sqrt(Cin * R * R))
    bias = torch.randn(Cout, generator=gen)
    scale = torch.rand(Cout, generator=gen) + 0.5
    dw0 = torch.randn(Cout * R * R, Cin, generator=gen)
    db0 = torch.randn(Cout, generator=gen)
    wf, wd = pack_weights(ops, w)
    wf, wd = wf.view(Cout * R * R, Cin).cpu(), wd.view(Cin * R * R, Cout).cpu()
    # ---- references, per level (torch CPU fp32 on the same bf16 operands)
    ref = {"fwd_epi": [], "fwd_plain": [], "dg_before": [], "dg_after": []}
    dw_ref, db_ref = torch.zeros(Cout, Cin, R, R), torch.zeros(Cout)
    for i in range(gin.nlev):
        xi = _lvl(x, gin, i).requires_grad_(True)
        wr = w.clone().requires_grad_(True)
        y = TF.conv2d(xi, wr, None, stride=stride, padding=pad)
        ref["fwd_plain"].append(y.detach())
        ref["fwd_epi"].append(TF.relu(y.detach() + bias.view(1, -1, 1, 1) + _lvl(res, gout, i)))
        gi = _lvl(gy, gout, i)
        y.backward(gi)
        a, m = _lvl(addx, gin, i), _lvl(maskx, gin, i) > 0
        ref["dg_before"].append((xi.grad + a) * m)
        ref["dg_after"].append(xi.grad * m + a)
        dw_ref += wr.grad
        db_ref += gi.sum((0, 2, 3))
    dw_ref = oihw_to_ohwi(dw_ref).reshape(Cout * R * R, Cin)
    scale_rows = scale.view(-1, 1).repeat(1, R * R).view(-1, 1)
    seen, results = {}, {}
    for fill in U.FILLS:
        r = Run(fill)
        X, G = r.inp("x", x, kin), r.inp("g", gy, kout)
        RES, ADD, MASK = r.inp("res", res, kout), r.inp("add", addx, kin), r.inp("mask", maskx, kin)
        WF, WD, B, RS = r.inp("wf", wf), r.inp("wd", wd), r.inp("bias", bias), r.inp("row_scale", scale)
        out = {}

        def fwd_dgrad(tag):
            if "f" in dirs:
                y = r.out("y", gout.pixels, Cout, BF, kout)
                ops.conv2d_fwd(d, X, WF, B, y, add=RES, flags=ops.EPI_RELU | ops.EPI_ADD_BEFORE)
                seen[("fwd",) + tag] = _last()
                out[("fwd_epi",) + tag] = r.finish()["y"]
                y = r.out("y", gout.pixels, Cout, BF, kout)
                ops.conv2d_fwd(d, X, WF, None, y)
                out[("fwd_plain",) + tag] = r.finish()["y"]
            if "d" in dirs:
                for key, fl in (("dg_before", ops.EPI_ADD_BEFORE | ops.EPI_MASK), ("dg_after", ops.EPI_ADD_AFTER | ops.EPI_MASK)):
                    dx = r.out("dx", gin.pixels, Cin, BF, kin)
                    ops.conv2d_dgrad(d, G, WD, dx, add=ADD, mask=MASK, flags=fl)
                    seen[("dgrad",) + tag] = _last()
                    out[(key,) + tag] = r.finish()["dx"]

        for p3 in ROUTES:
            ops.set_route(patch3x3=p3)
            fwd_dgrad((p3, None))
            if "w" in dirs:
                for tr in (0, 1):
                    ops.set_route(wgrad=tr)
                    tag = (p3, tr)
                    dw = r.out("dw", Cout * R * R, Cin, F32)
                    ws = r.ws("ws", ops.conv2d_wgrad_workspace_bytes(d))
                    ops.conv2d_wgrad(d, X, G, dw, ws)
                    seen[("wgrad",) + tag] = _last()
                    out[("dw",) + tag] = r.finish()["dw"]
                    dw = r.inout("dw", dw0)
                    ws = r.ws("ws", ops.conv2d_wgrad_workspace_bytes(d))
                    ops.conv2d_wgrad(d, X, G, dw, ws, row_scale=RS, accumulate=True)
                    out[("dw_acc",) + tag] = r.finish()["dw"]
                    dw, db = r.out("dw", Cout * R * R, Cin, F32), r.out("db", Cout, None, F32)
                    ws = r.ws("ws", ops.conv2d_wgrad_bias_workspace_bytes(d))
                    ops.conv2d_wgrad_bias(d, X, G, dw, db, ws)
                    seen[("wgrad_bias",) + tag] = _last()
                    o = r.finish()
                    out[("dwb",) + tag], out[("db",) + tag] = o["dw"], o["db"]
                    dw, db = r.inout("dw", dw0), r.inout("db", db0)
                    ws = r.ws("ws", ops.conv2d_wgrad_bias_workspace_bytes(d))
                    ops.conv2d_wgrad_bias(d, X, G, dw, db, ws, row_scale=RS, accumulate=True)
                    o = r.finish()
                    out[("dwb_acc",) + tag], out[("db_acc",) + tag] = o["dw"], o["db"]
                ops.set_route(wgrad=None)
        ops.set_route(patch3x3=None)
        for mode in dense_modes:
            ops.set_route(dense1x1=mode)
            fwd_dgrad(("dense1x1", mode))
        ops.set_route(dense1x1=None)
        r.finish()
        results[fill] = out
    ops.reset_route()
    _same_bits(results, name)
    # ---- the zero-fill run against the references
    for key, bits in results["zero"].items():
        what, tag = key[0], key[1:]
        if what in ref:
            geom, kind = (gout, kout) if what.startswith("fwd") else (gin, kin)
            full = _owned_to_levels(bits, BF, geom, kind)
            for i in range(geom.nlev):
                e = rel_l2(_lvl(full, geom, i), ref[what][i])
                assert e < TOL, f"{name} {key} level {i}: rel-L2 {e:.2e}"
        elif what in ("dw", "dwb"):
            assert rel_l2(bits.view(F32).cpu(), dw_ref) < 2e-3, (name, key)
        elif what in ("dw_acc", "dwb_acc"):
            assert rel_l2(bits.view(F32).cpu(), dw_ref * scale_rows + dw0) < 2e-3, (name, key)
        elif what == "db":
            assert rel_l2(bits.view(F32).cpu(), db_ref) < 1e-4, (name, key)
        elif what == "db_acc":
            assert rel_l2(bits.view(F32).cpu() - db0, db_ref) < 1e-4, (name, key)
    for k, v in sorted(seen.items(), key=str):
        print(f"[guard] {name} {k}: {v}")
    _SEEN[name] = seen
    return seen


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_launches_stay_inside_their_tensors(name):
    """bd_conv2d_fwd (bias + residual + ReLU, and plain), bd_conv2d_dgrad (add before / after + mask), bd_conv2d_wgrad and
    bd_conv2d_wgrad_bias (plain, and row_scale + accumulate) under every route word of test_conv_fwd_dgrad_wgrad."""
    _run_conv_case(name)


def test_conv_cases_reach_every_bf16_kernel():
    """The union of bd_conv_last_kernel() over the cases above names every bf16 kernel those four entry points can dispatch to."""
    got = set()
    for name in CONV_CASES:
        got |= set(_run_conv_case(name).values())
    assert got >= CONV_KERNELS, sorted(CONV_KERNELS - got)


def test_conv_gnstats_and_groupnorm_parts():
    """bd_conv2d_fwd_gnstats (part at exactly conv2d_fwd_gnstats_bytes) + bd_groupnorm_fwd_parts, N = 3 over LEVELS (dense contract):
    y equals bd_conv2d_fwd's bits and matches torch (TOL); z within 2e-3 of the separate bd_groupnorm_fwd (test_groupnorm_gpu.py)."""
    ops = _ops()
    C, N = 256, 3
    geom = ops.Geom(N, [h for h, _ in LEVELS], [w for _, w in LEVELS])
    d = ops.conv_desc(geom, geom, C, C, 3, 3, 1, 1)
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(geom.pixels, C, generator=gen).to(BF)
    w = bf16_round(torch.randn(C, C, 3, 3, generator=gen) / np.sqrt(9 * C))
    bias, gamma, beta = torch.randn(C, generator=gen) * 0.5, torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    wf, _ = pack_weights(ops, w)
    y0 = torch.empty((geom.pixels, C), dtype=BF, device="cuda")
    ops.conv2d_fwd(d, x.cuda(), wf, bias.cuda(), y0)
    st0 = torch.empty((N, geom.nlev, 32, 2), dtype=F32, device="cuda")
    z0 = torch.empty_like(y0)
    ws0 = torch.empty((ops.groupnorm_workspace_bytes(N, geom.nlev, C, geom.pix_per_img),), dtype=U8, device="cuda")
    ops.groupnorm_fwd(y0, gamma.cuda(), beta.cuda(), geom, C, 1e-5, True, st0, z0, ws0)
    results = {}
    for fill in U.FILLS:
        r = Run(fill)
        X, WF, B = r.inp("x", x), r.inp("wf", wf.view(C * 9, C).cpu()), r.inp("bias", bias)
        GA, BE = r.inp("gamma", gamma), r.inp("beta", beta)
        y = r.out("y", geom.pixels, C, BF)
        part = r.out("part", ops.conv2d_fwd_gnstats_bytes(d) // 4, None, F32)
        ops.conv2d_fwd_gnstats(d, X, WF, B, y, part)
        assert _last() == "conv3x3_pp_kernel"
        o = r.finish()
        Y, PART = r.inp("y_in", o["y"].view(BF)), r.inp("part_in", o["part"].view(F32))
        stats, z = r.out("stats", N * geom.nlev * 32 * 2, None, F32), r.out("z", geom.pixels, C, BF)
        ops.groupnorm_fwd_parts(d, Y, PART, GA, BE, 1e-5, True, stats, z)
        o.update(r.finish())
        results[fill] = o
    _same_bits(results, "gnstats")
    o = results["zero"]
    assert torch.equal(o["y"], U.bits_of(y0))
    yc = o["y"].view(BF).cpu()
    for i in range(geom.nlev):
        assert rel_l2(_lvl(yc, geom, i), TF.conv2d(_lvl(x, geom, i), w, bias, padding=1)) < TOL
    assert bool(torch.isfinite(o["part"].view(F32)).all())
    assert rel_l2(o["z"].view(BF).float().cpu(), z0.float().cpu()) < 2e-3
    s1, s0 = o["stats"].view(F32).view(N, geom.nlev, 32, 2), st0
    assert float(((s1[..., 0] - s0[..., 0]).abs() * s0[..., 1]).max()) < 2e-3
    assert float(((s1[..., 1] - s0[..., 1]).abs() / s0[..., 1]).max()) < 2e-3


def test_thin_1x1_forward_and_backward():
    """bd_conv1x1_thin_fwd / _bwd at M = 37 (tests/test_conv_gpu.py::test_thin_1x1_backward_in_one_pass: 3e-3 / 1e-5)."""
    ops = _ops()
    M, Cin, Cout, real = 37, 256, 16, 15
    rng = np.random.default_rng(M)
    x = np.maximum(rng.normal(0, 1, (M, Cin)), 0).astype(np.float32)
    g = rng.normal(0, 1, (M, Cout)).astype(np.float32)
    g[:, real:] = 0
    w = rng.normal(0, 0.05, (Cout, Cin)).astype(np.float32)
    w[real:] = 0
    bias = torch.from_numpy(rng.normal(0, 0.1, (Cout,)).astype(np.float32))
    xb, gb = torch.from_numpy(x).to(BF), torch.from_numpy(g).to(BF)
    wt = torch.from_numpy(w)
    results = {}
    for fill in U.FILLS:
        r = Run(fill)
        X, G, W, B = r.inp("x", xb), r.inp("g", gb), r.inp("w", wt), r.inp("bias", bias)
        y = r.out("y", M, Cout, BF)
        ops.conv1x1_thin_fwd(X, W, B, M, Cin, Cout, y)
        assert _last() == "conv1x1_thin_fwd_kernel"
        o = r.finish()
        dx, dw, db = r.out("dx", M, Cin, BF), r.out("dw", Cout, Cin, F32), r.out("db", Cout, None, F32)
        ws = r.ws("ws", ops.conv1x1_thin_bwd_workspace_bytes())
        ops.conv1x1_thin_bwd(X, G, W, M, Cin, Cout, dx, dw, db, real, ws)
        assert _last() == "conv1x1_thin_bwd_kernel"
        o.update(r.finish())
        results[fill] = o
    _same_bits(results, "thin")
    o = results["zero"]
    x64, g64, w64 = xb.double(), gb.double(), wt.to(BF).double()
    assert rel_l2(o["y"].view(BF).float().cpu(), x64 @ w64.t() + bias.double()) <= 3e-3
    assert rel_l2(o["dx"].view(BF).float().cpu(), (g64 @ w64) * (x64 > 0)) <= 3e-3
    assert rel_l2(o["dw"].view(F32).cpu(), g64.t() @ x64) <= 1e-5
    assert rel_l2(o["db"].view(F32).cpu(), g64.sum(0)) <= 1e-5
    assert bool((o["dw"].view(F32)[real:] == 0).all()) and bool((o["db"].view(F32)[real:] == 0).all())


@pytest.mark.parametrize("N,H,W,has_ds", [(1, 5, 3, True), (1, 5, 3, False), (2, 9, 17, True), (2, 9, 17, False)])
def test_bottleneck_fwd(N, H, W, has_ds):
    """bd_bottleneck_fwd against the fp32 restatement of tests/test_bottleneck_fused_gpu.py (rel-L2 5e-3)."""
    ops = _ops()
    cin, ch, cout = (64 if has_ds else 256), 64, 256
    assert ops.bottleneck_fwd_supported(N, H, W, cin, ch, cout, has_ds)
    g = torch.Generator().manual_seed(H * 1000 + W + int(has_ds))
    x = bf16_round(torch.randn(N, cin, H, W, generator=g).relu())
    w1 = torch.randn(ch, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5
    w2 = torch.randn(ch, ch, 3, 3, generator=g) * (2.0 / (9 * ch)) ** 0.5
    w3 = torch.randn(cout, ch, 1, 1, generator=g) * (1.0 / ch) ** 0.5
    wd = torch.randn(cout, cin, 1, 1, generator=g) * (1.0 / cin) ** 0.5
    bs = [torch.randn(c, generator=g) * 0.2 for c in (ch, ch, cout, cout)]
    packed = [pack_weights(ops, w)[0] for w in (w1, w2, w3, wd)]
    xp = x.permute(0, 2, 3, 1).reshape(N * H * W, cin).to(BF)
    results = {}
    for fill in U.FILLS:
        r = Run(fill)
        X = r.inp("x", xp)
        ws_ = [r.inp(f"w{i}", p.view(-1, p.shape[-1]).cpu()) for i, p in enumerate(packed)]
        bd_ = [r.inp(f"b{i}", b) for i, b in enumerate(bs)]
        y = r.out("y", N * H * W, cout, BF)
        ops.bottleneck_fwd(N, H, W, cin, ch, cout, X, ws_[0], bd_[0], ws_[1], bd_[1], ws_[2], bd_[2], ws_[3] if has_ds else None,
                           bd_[3] if has_ds else None, y)
        results[fill] = r.finish()
    _same_bits(results, "bottleneck")
    wq = [bf16_round(w) for w in (w1, w2, w3, wd)]
    t = bf16_round(TF.conv2d(x, wq[0], bs[0]).relu())
    t = bf16_round(TF.conv2d(t, wq[1], bs[1], padding=1).relu())
    want = (TF.conv2d(t, wq[2], bs[2]) + (TF.conv2d(x, wq[3], bs[3]) if has_ds else x)).relu()
    got = results["zero"]["y"].view(BF).float().cpu().reshape(N, H, W, cout).permute(0, 3, 1, 2)
    assert rel_l2(got, want) < 5e-3


def test_fpn_deconv():
    """bd_fpn_deconv_fwd / _dgrad (with the fused add) and bd_fpn_deconv_wgrad (stored and accumulated; workspace exactly
    fpn_deconv_wgrad_workspace_bytes) at (2, 7, 11, 128), the smallest ragged shape of tests/test_fpn_deconv_gpu.py: 1e-2 / 2e-3."""
    ops = _ops()
    N, H, W, C = 2, 7, 11, 128
    g = torch.Generator().manual_seed(H * 131 + W)
    x = bf16_round(torch.randn(N, C, H, W, generator=g))
    w = torch.randn(C, C, 4, 4, generator=g) * (2.0 / (16 * C)) ** 0.5
    add, dy = bf16_round(torch.randn(N, C, 2 * H, 2 * W, generator=g)), bf16_round(torch.randn(N, C, 2 * H, 2 * W, generator=g))
    addc = bf16_round(torch.randn(N, C, H, W, generator=g))
    dw0 = torch.randn(C * 16, C, generator=g)
    wf = torch.empty((4, C, 4, C), dtype=BF, device="cuda")
    wd = torch.empty((C, 16, C), dtype=BF, device="cuda")
    ops.fpn_deconv_pack(w.permute(0, 2, 3, 1).contiguous().cuda(), C, wf, wd)
    pm = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C).to(BF)
    wsb = ops.fpn_deconv_wgrad_workspace_bytes(N, H, W, C)
    results, names = {}, {}
    for fill in U.FILLS:
        r = Run(fill)
        X, DY, ADD, ADDC = r.inp("x", pm(x)), r.inp("dy", pm(dy)), r.inp("add", pm(add)), r.inp("addc", pm(addc))
        WF, WD = r.inp("wf", wf.view(-1, C).cpu()), r.inp("wd", wd.view(-1, C).cpu())
        ops.fpn_deconv_fwd(X, WF, r.out("y", N * 4 * H * W, C, BF), N, H, W, C, add=ADD)
        names["fwd"] = _last()
        o = r.finish()
        ops.fpn_deconv_dgrad(DY, WD, r.out("dx", N * H * W, C, BF), N, H, W, C, add=ADDC)
        names["dgrad"] = _last()
        o.update(r.finish())
        ops.fpn_deconv_wgrad(X, DY, r.out("dw", C * 16, C, F32), r.ws("ws", wsb), N, H, W, C, accumulate=False)
        names["wgrad"] = _last()
        o.update(r.finish())
        ops.fpn_deconv_wgrad(X, DY, r.inout("dw_acc", dw0), r.ws("ws", wsb), N, H, W, C, accumulate=True)
        o.update(r.finish())
        results[fill] = o
    print(f"[guard] fpn_deconv {names}")
    assert names == {"fwd": "fpn_deconv_kernel<fwd>", "dgrad": "fpn_deconv_kernel<dgrad>", "wgrad": "fpn_deconv_wgrad_kernel"}
    _same_bits(results, "fpn_deconv")
    o = results["zero"]
    xr, wr = x.clone().requires_grad_(True), bf16_round(w).requires_grad_(True)
    y = TF.conv_transpose2d(xr, wr, stride=2, padding=1)
    (y * dy).sum().backward()
    nchw = lambda t, h, w_: t.view(BF).float().cpu().view(N, h, w_, C).permute(0, 3, 1, 2)
    assert rel_l2(nchw(o["y"], 2 * H, 2 * W), y.detach() + add) < 1e-2
    assert rel_l2(nchw(o["dx"], H, W), xr.grad + addc) < 1e-2
    assert rel_l2(o["dw"].view(F32).cpu().view(C, 4, 4, C).permute(0, 3, 1, 2), wr.grad) < 2e-3
    assert rel_l2((o["dw_acc"].view(F32).cpu() - dw0).view(C, 4, 4, C).permute(0, 3, 1, 2), wr.grad) < 2e-3


# ---- c. pixel-major plumbing kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 256])
@pytest.mark.parametrize("H,W", [(5, 7), (1, 1)])
def test_upsample2x_add(H, W, C):
    """bd_upsample2x_add_fwd / _bwd: top and lateral are each the middle level of a gapped three-level tensor; the other two levels of
    both tensors must keep their bits.  5e-3 as tests/test_conv_gpu.py::test_upsample_add_fwd_bwd."""
    ops = _ops()
    N = 2
    gtop3, ktop = U.gapped_geom(N, [(3, 4), (H, W), (2, 2)])
    glat3, klat = U.gapped_geom(N, [(4, 3), (2 * H, 2 * W), (3, 3)], gap=U.GUARD_MIN_ROWS + 3)
    gtop, glat = gtop3.level(1), glat3.level(1)

    def own_of(g3, g1):
        m = torch.zeros(g3.N, g3.pix_per_img, dtype=torch.bool)
        m[:, g1.off[0]:g1.off[0] + g1.H[0] * g1.W[0]] = True
        return m.view(-1)
    own_top, own_lat = own_of(gtop3, gtop), own_of(glat3, glat)
    gen = torch.Generator().manual_seed(5 + C + H)
    top, lat = torch.randn(gtop3.pixels, C, generator=gen).to(BF), torch.randn(glat3.pixels, C, generator=gen).to(BF)
    dl, prev = torch.randn(glat3.pixels, C, generator=gen).to(BF), torch.randn(gtop3.pixels, C, generator=gen).to(BF)
    results = {}
    for fill in U.FILLS:
        r = Run(fill)
        T = r.inp("top", top, ktop)
        Lt = r.inout("lat", lat, klat, own_lat)            # updated in place: exempt from "inputs keep their bits" in its own level only
        ops.upsample2x_add_fwd(T, gtop, Lt, glat, C)
        o = r.finish()
        DL = r.inp("dlat", dl, klat)
        dt = r.inout("dtop_acc", prev, ktop, own_top)
        ops.upsample2x_add_bwd(DL, glat, dt, gtop, C, accumulate=True)
        o.update(r.finish())
        # accumulate off: the level is written, the other levels (data of other launches) keep their bits
        t_, h = U.guarded(gtop3.pixels, C, BF, "cuda", name="dtop")
        h.set(prev).set_gaps(ktop)
        U.bits_of(h.t)[own_top.cuda()] = U.fill_pattern(BF, "sentinel", C, "cuda").view(1, -1)
        h.own, h.written = own_top.cuda(), True
        h.snapshot()
        r.outs.append(h)
        ops.upsample2x_add_bwd(DL, glat, t_, gtop, C, accumulate=False)
        o.update(r.finish())
        results[fill] = o
    _same_bits(results, "upsample")
    o = {k: v.view(BF).float().cpu().view(N, -1, C) for k, v in results["zero"].items()}
    nchw = lambda t, h, w: t.reshape(N, h, w, C).permute(0, 3, 1, 2)
    tl = lambda t, g: t.view(N, g.pix_per_img, C)[:, g.off[0]:g.off[0] + g.H[0] * g.W[0]].float()
    topn = nchw(tl(top, gtop), H, W).clone().requires_grad_(True)
    up = TF.interpolate(topn, scale_factor=2, mode="bilinear", align_corners=False)
    assert rel_l2(nchw(o["lat"], 2 * H, 2 * W), nchw(tl(lat, glat), 2 * H, 2 * W) + up.detach()) < 5e-3
    up.backward(nchw(tl(dl, glat), 2 * H, 2 * W))
    assert rel_l2(nchw(o["dtop_acc"], H, W), nchw(tl(prev, gtop), H, W) + topn.grad) < 5e-3
    assert rel_l2(nchw(o["dtop"], H, W), topn.grad) < 5e-3


@pytest.mark.parametrize("N,H,W,C", [(1, 27, 19, 40), (1, 21, 37, 720), (2, 9, 17, 2056)])
def test_colsum(N, H, W, C):
    """bd_colsum_bf16 over the middle level of a gapped tensor: 513 x 40, 777 x 720, and a width above COLSUM_CHUNK (2048) over two
    images; workspace exactly colsum_workspace_bytes.  rtol 1e-4 / atol 1e-3 as test_elementwise_pack_colsum_sgd."""
    ops = _ops()
    g3, kind = U.gapped_geom(N, [(2, 3), (H, W), (1, 2)])
    lv = g3.level(1)
    gen = torch.Generator().manual_seed(9 + C)
    m = torch.randn(g3.pixels, C, generator=gen).to(BF)
    acc0 = torch.randn(C, generator=gen)
    results = {}
    for fill in U.FILLS:
        r = Run(fill)
        G = r.inp("g", m, kind)
        out, ws = r.out("out", C, None, F32), r.ws("ws", ops.colsum_workspace_bytes(C))
        ops.colsum_bf16(G, 0, C, out, ws, geom=lv)
        o = r.finish()
        out, ws = r.inout("out_acc", acc0), r.ws("ws", ops.colsum_workspace_bytes(C))
        ops.colsum_bf16(G, 0, C, out, ws, accumulate=True, geom=lv)
        o.update(r.finish())
        results[fill] = o
    _same_bits(results, "colsum")
    want = m.view(N, g3.pix_per_img, C)[:, lv.off[0]:lv.off[0] + H * W].float().sum((0, 1))
    assert torch.allclose(results["zero"]["out"].view(F32).cpu(), want, rtol=1e-4, atol=1e-3)
    assert torch.allclose(results["zero"]["out_acc"].view(F32).cpu(), want + acc0, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("H,W", [(7, 9), (8, 10), (1, 1), (2, 3)])
def test_maxpool_equals_torch(H, W):
    """bd_maxpool3x3s2_fwd == torch max_pool2d(3, 2, 1) at odd, even and tiny sizes.  The +-max fill is the one that matters: a window
    that reaches into the next image or past the tensor picks up +max (fmaxf would drop a NaN)."""
    ops = _ops()
    N, C = 2, 64
    Hq, Wq = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(H * 16 + W)).to(BF)
    xp = x.permute(0, 2, 3, 1).reshape(N * H * W, C).contiguous()
    results = {}
    for fill in U.FILLS:
        r = Run(fill)
        X, y = r.inp("x", xp), r.out("y", N * Hq * Wq, C, BF)
        ops.maxpool3x3s2_fwd(X, N, H, W, C, y)
        results[fill] = r.finish()
    _same_bits(results, "maxpool")
    got = results["zero"]["y"].view(BF).cpu().view(N, Hq, Wq, C).permute(0, 3, 1, 2)
    assert torch.equal(got.float(), TF.max_pool2d(x.float(), 3, 2, 1))


@pytest.mark.parametrize("N,Hp,Wp", [(2, 34, 58), (1, 32, 32)])
def test_stem_and_pad_normalize(N, Hp, Wp):
    """bd_pad_normalize (output guarded), bd_stem_conv7x7_fwd, bd_maxpool3x3s2_fwd behind it and bd_stem_pool_fwd: the halo input is
    guarded outside its own halo.  Equality / TOL as tests/test_conv_gpu.py::test_stem_conv_and_pad_normalize; the fused kernel equals
    the two launches bit for bit."""
    ops = _ops()
    H, W = Hp - 5, Wp - 9
    g = torch.Generator().manual_seed(Hp * 7 + Wp)
    img = torch.rand(N, 3, H, W, generator=g) * 255
    mean, std = [103.530, 116.280, 123.675], [57.375, 57.12, 58.395]
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.05
    scale, shift = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    wst = torch.empty((64, 7, 8, 4), dtype=BF, device="cuda")
    ops.stem_weight_pack(oihw_to_ohwi(w).cuda(), scale.cuda(), wst)
    rows = N * (Hp + 6) * (Wp + 8)
    Ho, Wo = Hp // 2, Wp // 2
    Hq, Wq = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    results = {}
    for fill in U.FILLS:
        r = Run(fill)
        IMG = r.inp("img", img.reshape(-1))
        xh = r.out("xh", rows, 4, BF)
        ops.pad_normalize(IMG.view(N, 3, H, W), Hp, Wp, mean, std, xh)
        o = r.finish()
        XH, WS, SH = r.inp("xh_in", o["xh"].view(BF)), r.inp("wst", wst.view(-1, 4).cpu()), r.inp("shift", shift)
        y = r.out("y", N * Ho * Wo, 64, BF)
        ops.stem_conv7x7_fwd(N, Hp, Wp, XH, WS, SH, y)
        o.update(r.finish())
        Y, p = r.inp("y_in", o["y"].view(BF)), r.out("p", N * Hq * Wq, 64, BF)
        ops.maxpool3x3s2_fwd(Y, N, Ho, Wo, 64, p)
        o.update(r.finish())
        pf = r.out("pf", N * Hq * Wq, 64, BF)
        ops.stem_pool_fwd(N, Hp, Wp, XH, WS, SH, pf)
        o.update(r.finish())
        results[fill] = o
    _same_bits(results, "stem")
    o = results["zero"]
    # data_to_input (pre_processing.py:11-19) at this padded size: pad with 0 first, then normalise in fp32
    xo = (TF.pad(img, (0, Wp - W, 0, Hp - H)) - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
    xh = o["xh"].view(BF).float().cpu().view(N, Hp + 6, Wp + 8, 4)
    assert torch.equal(xh[:, 3:3 + Hp, 4:4 + Wp, :3].permute(0, 3, 1, 2), bf16_round(xo))
    halo = xh.clone()
    halo[:, 3:3 + Hp, 4:4 + Wp, :3] = 0
    assert float(halo.abs().max()) == 0
    ref = TF.relu(TF.conv2d(bf16_round(xo), bf16_round(w * scale.view(-1, 1, 1, 1)), shift, stride=2, padding=3))
    got = o["y"].view(BF).float().cpu().view(N, Ho, Wo, 64).permute(0, 3, 1, 2)
    assert rel_l2(got, ref) < TOL
    assert torch.equal(o["p"].view(BF).float().cpu().view(N, Hq, Wq, 64).permute(0, 3, 1, 2), TF.max_pool2d(got, 3, 2, 1))
    assert torch.equal(o["pf"], o["p"])


@pytest.mark.parametrize("n", [8, 4104])
def test_elementwise(n):
    """bd_relu_bf16, bd_add_bf16, bd_relu_bwd_bf16, bd_f32_to_bf16 and bd_f32_to_bf16_add: equality with torch."""
    ops = _ops()
    g = torch.Generator().manual_seed(9 + n)
    a, b, c = (torch.randn(n, generator=g).to(BF) for _ in range(3))
    f = torch.randn(n, generator=g)
    results = {}
    for fill in U.FILLS:
        r = Run(fill)
        A, B, Cc, Fs = r.inp("a", a), r.inp("b", b), r.inp("c", c), r.inp("f", f)
        o = {}
        ops.relu_bf16(A, r.out("relu", n, None, BF)); o.update(r.finish())
        ops.add_bf16(A, B, r.out("add", n, None, BF)); o.update(r.finish())
        ops.relu_bwd_bf16(A, B, r.out("relu_bwd", n, None, BF), add=Cc); o.update(r.finish())
        ops.relu_bwd_bf16(A, B, r.out("relu_bwd_plain", n, None, BF)); o.update(r.finish())
        ops.f32_to_bf16(Fs, r.out("cvt", n, None, BF)); o.update(r.finish())
        ops.f32_to_bf16(Fs, r.inout("cvt_add", a), accumulate=True); o.update(r.finish())
        results[fill] = o
    _same_bits(results, "elementwise")
    o = {k: v.view(BF).float().cpu() for k, v in results["zero"].items()}
    af, bf_, cf = a.float(), b.float(), c.float()
    assert torch.equal(o["relu"], af.clamp(min=0))
    assert torch.equal(o["add"], bf16_round(af + bf_))
    assert torch.equal(o["relu_bwd"], bf16_round(af * (bf_ > 0) + cf))
    assert torch.equal(o["relu_bwd_plain"], af * (bf_ > 0))
    assert torch.equal(o["cvt"], bf16_round(f))
    assert torch.equal(o["cvt_add"], bf16_round(af + f))


def _gn_reference(y, dz, gamma, beta, geom):
    """torch group_norm(32) + ReLU and its autograd per (image, level); y, dz fp32 (pixels, C) on the CPU.  Returns (z, dy, dgamma, dbeta)."""
    N, C = geom.N, y.shape[1]
    yv, dzv = y.view(N, geom.pix_per_img, C), dz.view(N, geom.pix_per_img, C)
    z, dy = torch.zeros_like(yv), torch.zeros_like(yv)
    g, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    dg, db = torch.zeros(C), torch.zeros(C)
    for i in range(geom.nlev):
        o, n = geom.off[i], geom.H[i] * geom.W[i]
        x = yv[:, o:o + n].permute(0, 2, 1).contiguous().requires_grad_(True)
        out = TF.relu(TF.group_norm(x, 32, g, b, eps=1e-5))
        z[:, o:o + n] = out.detach().permute(0, 2, 1)
        gx, gg, gb = torch.autograd.grad(out, (x, g, b), dzv[:, o:o + n].permute(0, 2, 1).contiguous())
        dy[:, o:o + n] = gx.permute(0, 2, 1)
        dg += gg
        db += gb
    return z.reshape(-1, C), dy.reshape(-1, C), dg, db


@pytest.mark.parametrize("N,sizes", [(3, LEVELS), (1, [(3, 43)])])          # 129 pixels: one full 128-pixel slot plus one pixel
def test_groupnorm_fwd_bwd(N, sizes):
    """bd_groupnorm_fwd / _bwd (dense contract: outer guards only); workspace exactly groupnorm_workspace_bytes.  4e-3 / 6e-3 / 2e-3 as
    tests/test_groupnorm_gpu.py."""
    ops = _ops()
    C = 256
    geom = ops.Geom(N, [h for h, _ in sizes], [w for _, w in sizes])
    gen = torch.Generator().manual_seed(17 + N)
    y = (torch.randn(geom.pixels, C, generator=gen) * 1.5 + 0.3).to(BF)
    dz = torch.randn(geom.pixels, C, generator=gen).to(BF)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    dg0, db0 = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    wsb = ops.groupnorm_workspace_bytes(N, geom.nlev, C, geom.pix_per_img)
    results = {}
    for fill in U.FILLS:
        r = Run(fill)
        Y, DZ, GA, BE = r.inp("y", y), r.inp("dz", dz), r.inp("gamma", gamma), r.inp("beta", beta)
        stats, z = r.out("stats", N * geom.nlev * 32 * 2, None, F32), r.out("z", geom.pixels, C, BF)
        ops.groupnorm_fwd(Y, GA, BE, geom, C, 1e-5, True, stats, z, r.ws("ws", wsb))
        o = r.finish()
        ST = r.inp("stats_in", o["stats"].view(F32))
        dy, dg, db = r.out("dy", geom.pixels, C, BF), r.out("dgamma", C, None, F32), r.out("dbeta", C, None, F32)
        ops.groupnorm_bwd(DZ, Y, GA, BE, ST, geom, C, True, dy, dg, db, r.ws("ws", wsb))
        o.update(r.finish())
        dy, dg, db = r.out("dy2", geom.pixels, C, BF), r.inout("dgamma_acc", dg0), r.inout("dbeta_acc", db0)
        ops.groupnorm_bwd(DZ, Y, GA, BE, ST, geom, C, True, dy, dg, db, r.ws("ws", wsb), accumulate=True)
        o.update(r.finish())
        results[fill] = o
    _same_bits(results, "groupnorm")
    o = results["zero"]
    z_ref, dy_ref, dg_ref, db_ref = _gn_reference(y.float(), dz.float(), gamma, beta, geom)
    assert rel_l2(o["z"].view(BF).float().cpu(), z_ref) < 4e-3
    assert rel_l2(o["dy"].view(BF).float().cpu(), dy_ref) < 6e-3
    assert torch.equal(o["dy2"], o["dy"])
    assert rel_l2(o["dgamma"].view(F32).cpu(), dg_ref) < 2e-3 and rel_l2(o["dbeta"].view(F32).cpu(), db_ref) < 2e-3
    assert rel_l2(o["dgamma_acc"].view(F32).cpu() - dg0, dg_ref) < 2e-3 and rel_l2(o["dbeta_acc"].view(F32).cpu() - db0, db_ref) < 2e-3


def test_fcos_offsets_fwd_bwd():
    """bd_fcos_offsets_fwd / _bwd, N = 3 over LEVELS (dense contract).  <= 1 bf16 ulp as
    tests/test_losses_large_gpu.py::test_fcos_offsets_fwd_bwd_at_the_bench_batch; dscale within 2^-22 of the sum of |terms| (each term is
    rounded once to fp32, 2^-24, and a level of at most 459 points is summed through a tree of a few more roundings: the bench test's
    4e-8 is an average over 268 800 terms, not a bound for six)."""
    ops = _ops()
    N, strides = 3, [8, 16, 32]
    geom = ops.Geom(N, [h for h, _ in LEVELS], [w for _, w in LEVELS])
    P = geom.pixels
    gen = torch.Generator().manual_seed(17)
    raw = (torch.randn(P, 8, generator=gen) * 2).to(BF)
    raw[torch.rand(P, 8, generator=gen) < 0.05] = 0
    scales = torch.tensor([1.3, -0.7, 0.9])
    d_off, d_ctr = torch.randn(P, 4, generator=gen).to(BF), torch.randn(P, generator=gen).to(BF)
    results = {}
    for fill in U.FILLS:
        r = Run(fill)
        RAW, SC, DO, DC = r.inp("raw", raw), r.inp("scales", scales), r.inp("d_off", d_off), r.inp("d_ctr", d_ctr)
        out = r.out("out", P, 4, BF)
        ops.fcos_offsets_fwd(RAW, 8, SC, geom, strides, out)
        o = r.finish()
        d_raw, dscale = r.out("d_raw", P, 8, BF), r.out("dscale", 3, None, F32)
        ops.fcos_offsets_bwd(RAW, 8, SC, geom, strides, DO, DC, d_raw, dscale, r.ws("ws", ops.fcos_offsets_workspace_bytes()))
        o.update(r.finish())
        results[fill] = o
    _same_bits(results, "fcos_offsets")
    o = results["zero"]
    lvl = torch.zeros(geom.pix_per_img, dtype=torch.long)
    for i, off in enumerate(geom.off):
        lvl[off:] = i
    lvl = lvl.repeat(N)
    sc, st = scales.double()[lvl][:, None], torch.tensor(strides, dtype=torch.float64)[lvl][:, None]
    rr = raw[:, :4].double()
    assert int(U.bf16_ulps(o["out"].view(BF).cpu(), (rr * sc).clamp_min(0) * st).max()) <= 1
    on, go = (rr * sc) > 0, d_off.double()
    got = o["d_raw"].view(BF).cpu()
    assert int(U.bf16_ulps(got[:, :4].contiguous(), torch.where(on, go * st * sc, torch.zeros_like(go))).max()) <= 1
    assert torch.equal(U.bits_of(got[:, 4].contiguous()), U.bits_of(d_ctr)) and bool((U.bits_of(got[:, 5:].contiguous()) == 0).all())
    terms = torch.where(on, go * st * rr, torch.zeros_like(go)).sum(1)
    ds = torch.zeros(3, dtype=torch.float64).index_add_(0, lvl, terms)
    mag = torch.zeros(3, dtype=torch.float64).index_add_(0, lvl, terms.abs())
    assert float(((o["dscale"].view(F32).cpu().double() - ds).abs() / mag).max()) < 2.0 ** -22


# ---- b. fp8 path -----------------------------------------------------------------------------------------------------------------------
FP8_KERNELS = {"conv3x3_pp8_kernel", "conv_fp8_kernel", "conv_wgrad3x3_fp8_kernel", "conv1x1_fp8_kernel", "conv1x1_ring_fp8_kernel"}
_XV = torch.tensor([0.0, 0.25, 0.5, 1.0, 1.5, -0.5, -1.0, 2.0, 3.0, -0.125])          # e4m3 numbers
_WV = torch.tensor([0.0, 0.875, -0.875, 1.75, -3.5, 0.4375])                           # e4m3 numbers; with one 7 per channel the scale is 2^-6


def _pick(vals, gen, *shape):
    return vals[torch.randint(0, len(vals), shape, generator=gen)]


def _close_bf16(got, ref):
    """The structural bound of tests/test_fp8_gpu.py: exact fp32 sums, so only the bf16 store (ties aside) is left."""
    ref = bf16_round(ref)
    return float((got != ref).float().mean()) < 1e-3 and bool(((got - ref).abs() <= ref.abs() * 2.0 ** -7 + 1e-6).all())


def test_fp8_launches_stay_inside_their_tensors():
    """bd_quantize_fp8 / _bf8, bd_conv2d_fwd_fp8 (patch and generic kernel), bd_conv2d_dgrad_fp8, bd_conv2d_wgrad_fp8 and bd_conv1x1_fp8
    (both modes; dense 1x1 mode 5 reaches the ring form), each at one multi-level ragged case and one K-tail case from the smallest
    entries of CASES / DG_CASES / WG_CASES / D1_CASES of tests/test_fp8_gpu.py, on e4m3- / e5m2-valued operands (that file's structural
    bounds).  One-byte inputs take 0x7f, NaN in both formats, as their NaN fill, and the largest finite value of THEIR format as +-max (e4m3 0x7e,
    e5m2 0x7b); one-byte outputs start as 0xff."""
    ops = _ops()
    names = set()
    E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2

    # quantisers: dense contract (element count only, a multiple of 16)
    for n in (16, 4112):
        gen = torch.Generator().manual_seed(3 + n)
        x = (torch.randn(n, generator=gen) * 30).to(BF)
        x[:8] = torch.tensor([0.0, 448.0, -448.0, 1000.0, -1e4, 2.0 ** -9, 2.0 ** -10 * 1.5, 0.017], dtype=BF)
        results = {}
        for fill in U.FILLS:
            r = Run(fill)
            X = r.inp("x", x)
            ops.quantize_fp8(X, 0.5, r.out("q8", n, None, U8))
            o = r.finish()
            ops.quantize_bf8(X, 0.5, r.out("b8", n, None, U8))
            o.update(r.finish())
            results[fill] = o
        _same_bits(results, "quantize")
        assert torch.equal(results["zero"]["q8"].cpu(), (x.float() * 0.5).clamp(-448, 448).to(E4).view(U8))
        assert torch.equal(results["zero"]["b8"].cpu(), (x.float() * 0.5).clamp(-57344, 57344).to(E5).view(U8))

    def q8(t, scale, fmt):
        lim = 448 if fmt is E4 else 57344
        return (t.float() * scale).clamp(-lim, lim).to(fmt).view(U8)

    # 3x3 forward / data gradient / weight gradient on gapped geometries
    for N, Cin, Cout, sizes in ((2, 256, 256, [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]), (2, 80, 72, [(11, 9)])):
        gin, kin, gout, kout = _conv_geoms(ops, N, sizes, 3, 1, 1, True)
        d = ops.conv_desc(gin, gout, Cin, Cout, 3, 3, 1, 1)
        gen = torch.Generator().manual_seed(5 + Cin + Cout)
        x, res = _pick(_XV, gen, gin.pixels, Cin).to(BF), bf16_round(torch.randn(gout.pixels, Cout, generator=gen)).to(BF)
        w = _pick(_WV, gen, Cout, Cin, 3, 3)
        w[:, 0, 0, 0] = 7.0
        bias = torch.randn(Cout, generator=gen)
        wq = torch.empty((Cout, 9, Cin), dtype=U8, device="cuda")
        wsc = torch.empty((Cout,), dtype=F32, device="cuda")
        ops.weight_pack_fp8(w.permute(0, 2, 3, 1).contiguous().cuda(), None, Cout, 9, Cin, 1.0, wq, wsc)
        results = {}
        for fill in U.FILLS:
            r = Run(fill)
            XQ, RES = r.inp("xq", q8(x, 1.0, E4), kin), r.inp("res", res, kout)
            WQ, WS, B = r.inp("wq", wq.view(-1, Cin).cpu()), r.inp("wscale", wsc.cpu()), r.inp("bias", bias)
            o = {}
            for patch in (1, 0):
                ops.set_route(fp8_patch=patch)
                y, y8 = r.out(f"y{patch}", gout.pixels, Cout, BF, kout), r.out(f"y8{patch}", gout.pixels, Cout, U8, kout)
                ops.conv2d_fwd_fp8(d, XQ, WQ, WS, B, y, add=RES, flags=ops.EPI_RELU | ops.EPI_ADD_BEFORE, y8=y8, q_scale=0.5)
                names.add(_last())
                o.update(r.finish())
            ops.set_route(fp8_patch=None)
            results[fill] = o
        _same_bits(results, f"fwd_fp8 {Cin}->{Cout}")
        for patch in (1, 0):
            full = _owned_to_levels(results["zero"][f"y{patch}"], BF, gout, kout)
            for i in range(gin.nlev):
                ref = torch.relu(TF.conv2d(_lvl(x, gin, i), w, bias, padding=1) + _lvl(res, gout, i))
                assert _close_bf16(_lvl(full, gout, i), ref), (Cin, Cout, patch, i)
            dec = results["zero"][f"y8{patch}"].view(E4).float().cpu()
            want = (results["zero"][f"y{patch}"].view(BF).float().cpu() * 0.5).clamp(-448, 448)
            assert bool(((dec - want).abs() <= want.abs() * 2.0 ** -4 * 1.01 + 2.0 ** -10 + want.abs() * 2.0 ** -8).all())

    GS = 2.0 ** 12
    gv = torch.tensor([0.0, 1.0, -1.0, 1.5, 0.5, -0.75, 2.0, -3.0, 0.25]) / GS
    for N, Cin, Cout, sizes in ((1, 256, 720, [(12, 20), (6, 10), (3, 5)]), (2, 192, 80, [(9, 11)])):
        gin, kin, gout, kout = _conv_geoms(ops, N, sizes, 3, 1, 1, True)
        d = ops.conv_desc(gin, gout, Cin, Cout, 3, 3, 1, 1)
        assert ops.fp8_dgrad_ok(d)
        gen = torch.Generator().manual_seed(21 + Cin + Cout)
        g = _pick(gv, gen, gout.pixels, Cout).to(BF)
        w = _pick(_WV, gen, Cout, Cin, 3, 3)
        w[0, :, 0, 0] = 7.0
        add = bf16_round(torch.randn(gin.pixels, Cin, generator=gen) * 1e-4).to(BF)
        mask = torch.relu(torch.randn(gin.pixels, Cin, generator=gen)).to(BF)
        wq = torch.empty((Cin, 9, Cout), dtype=U8, device="cuda")
        wsc = torch.empty((Cin,), dtype=F32, device="cuda")
        ops.weight_pack_fp8_t(w.permute(0, 2, 3, 1).contiguous().cuda(), None, Cout, 9, Cin, GS, wq, wsc)
        results = {}
        for fill in U.FILLS:
            r = Run(fill)
            G8, ADD, MASK = r.inp("g8", q8(g, GS, E5), kout, fmt="e5m2"), r.inp("add", add, kin), r.inp("mask", mask, kin)
            WQ, WS = r.inp("wq", wq.view(-1, Cout).cpu()), r.inp("wscale", wsc.cpu())
            dx, dx8 = r.out("dx", gin.pixels, Cin, BF, kin), r.out("dx8", gin.pixels, Cin, U8, kin)
            ops.conv2d_dgrad_fp8(d, G8, WQ, WS, dx, add=ADD, mask=MASK, flags=ops.EPI_ADD_BEFORE | ops.EPI_MASK, dx8=dx8, q_scale=GS)
            names.add(_last())
            results[fill] = r.finish()
        _same_bits(results, f"dgrad_fp8 {Cin}<-{Cout}")
        full = _owned_to_levels(results["zero"]["dx"], BF, gin, kin)
        for i in range(gin.nlev):
            ref = (TF.conv_transpose2d(_lvl(g, gout, i), w, stride=1, padding=1) + _lvl(add, gin, i)) * (_lvl(mask, gin, i) > 0)
            got = _lvl(full, gin, i)
            refb = bf16_round(ref)
            assert float((got != refb).float().mean()) < 1e-3 and bool(((got - refb).abs() <= refb.abs() * 2.0 ** -7 + 1e-9).all()), (Cin, Cout, i)

    xg = torch.tensor([0.0, 0.25, 0.5, 1.0, -0.5, -1.0, 2.0, 0.125]) / 64.0
    for N, Cin, Cout, sizes in ((1, 256, 256, [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]), (2, 80, 48, [(9, 17)])):
        gin, kin, gout, kout = _conv_geoms(ops, N, sizes, 3, 1, 1, True)
        d = ops.conv_desc(gin, gout, Cin, Cout, 3, 3, 1, 1)
        gen = torch.Generator().manual_seed(51 + Cin + Cout)
        x, g = _pick(_XV, gen, gin.pixels, Cin).to(BF), _pick(xg, gen, gout.pixels, Cout).to(BF)
        rs, base = torch.rand(Cout, generator=gen) + 0.5, torch.randn(Cout * 9, Cin, generator=gen)
        wsb = ops.conv2d_wgrad_fp8_workspace_bytes(d)
        results = {}
        for fill in U.FILLS:
            r = Run(fill)
            X8, G8, RS = r.inp("x8", q8(x, 1.0, E4), kin), r.inp("g8", q8(g, 64.0, E5), kout, fmt="e5m2"), r.inp("row_scale", rs)
            ops.conv2d_wgrad_fp8(d, X8, G8, 1.0 / 64.0, r.out("dw", Cout * 9, Cin, F32), r.ws("ws", wsb))
            names.add(_last())
            o = r.finish()
            ops.conv2d_wgrad_fp8(d, X8, G8, 1.0 / 64.0, r.inout("dw_acc", base), r.ws("ws", wsb), row_scale=RS, accumulate=True)
            o.update(r.finish())
            results[fill] = o
        _same_bits(results, f"wgrad_fp8 {Cin}x{Cout}")
        wz = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
        tot = sum((TF.conv2d(_lvl(x, gin, i).double(), wz, padding=1) * _lvl(g, gout, i).double()).sum() for i in range(gin.nlev))
        tot.backward()
        ref = wz.grad.float().permute(0, 2, 3, 1).reshape(Cout * 9, Cin)
        assert torch.equal(results["zero"]["dw"].view(F32).cpu(), ref)
        assert rel_l2(results["zero"]["dw_acc"].view(F32).cpu(), ref * rs.view(-1, 1).repeat(1, 9).view(-1, 1) + base) < 1e-6

    # dense 1x1 launches on one-byte operands (dense contract: one level from offset 0)
    for N, Cin, Cout, H, W in ((2, 256, 128, 13, 17), (1, 128, 544, 9, 11)):
        for mode in (0, 1):
            ci, co = (Cin, Cout) if mode == 0 else (Cout, Cin)           # the data gradient's K is Cout
            if (co if mode else ci) % 128 or (ci if mode else co) % 32:
                continue
            geo = ops.single(N, H, W)
            d = ops.conv_desc(geo, geo, ci, co, 1, 1, 1, 0)
            assert ops.conv1x1_fp8_ok(d, mode)
            M = N * H * W
            gen = torch.Generator().manual_seed(31 + ci + co + mode)
            w = _pick(_WV, gen, co, ci)
            if mode == 0:
                w[:, 0] = 7.0
                src, scale, fmt = _pick(_XV, gen, M, ci).to(BF), 1.0, E4
            else:
                w[0, :] = 7.0
                src, scale, fmt = (_pick(_XV, gen, M, co) / 64.0).to(BF), 64.0, E5
            K, CO = (ci, co) if mode == 0 else (co, ci)
            wq = torch.empty((CO, 1, K), dtype=U8, device="cuda")
            wsc = torch.empty((CO,), dtype=F32, device="cuda")
            (ops.weight_pack_fp8 if mode == 0 else ops.weight_pack_fp8_t)(w.view(co, 1, ci).contiguous().cuda(), None, co, 1, ci, scale, wq, wsc)
            bias = torch.randn(CO, generator=gen) if mode == 0 else None
            add = bf16_round(torch.randn(M, CO, generator=gen) * 0.1).to(BF)
            act = torch.relu(torch.randn(M, CO, generator=gen)).to(BF)
            results = {}
            for fill in U.FILLS:
                r = Run(fill)
                SRC, WQ, WS, ADD = r.inp("src", q8(src, scale, fmt), fmt="e5m2" if mode else None), r.inp("wq", wq.view(CO, K).cpu()), r.inp("wscale", wsc.cpu()), r.inp("add", add)
                Bv = r.inp("bias", bias) if mode == 0 else None
                MASK = r.inp("mask", act) if mode == 1 else None
                o = {}
                for dense in (None, 5):
                    ops.set_route(dense1x1=dense)
                    y, y8 = r.out(f"y{dense}", M, CO, BF), r.out(f"y8{dense}", M, CO, U8)
                    if mode == 0:
                        ops.conv1x1_fp8(d, 0, SRC, WQ, WS, Bv, y, add=ADD, y8=y8, q_scale=0.5, flags=ops.EPI_RELU | ops.EPI_ADD_BEFORE)
                    else:
                        ops.conv1x1_fp8(d, 1, SRC, WQ, WS, None, y, add=ADD, mask=MASK, y8=y8, q_scale=scale, flags=ops.EPI_ADD_BEFORE | ops.EPI_MASK)
                    names.add(_last())
                    o.update(r.finish())
                ops.set_route(dense1x1=None)
                results[fill] = o
            _same_bits(results, f"conv1x1_fp8 mode {mode} {ci}->{co}")
            if mode == 0:
                ref = torch.relu(src.float() @ w.t() + bias + add.float())
            else:
                ref = (src.float() @ w + add.float()) * (act.float() > 0)
            for dense in (None, 5):
                assert _close_bf16(results["zero"][f"y{dense}"].view(BF).float().cpu(), ref), (mode, ci, co, dense)
    ops.reset_route()
    print(f"[guard] fp8 kernels reached: {sorted(names)}")
    assert names >= FP8_KERNELS, sorted(FP8_KERNELS - names)
