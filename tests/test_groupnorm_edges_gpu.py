"""csrc/norm.hip (bd_groupnorm_fwd / _bwd, and bd_conv2d_fwd_gnstats -> bd_groupnorm_fwd_parts) on ill-conditioned and degenerate groups against
the float64 oracle of tests/groupnorm_oracle.py, per element and for EVERY (image, level, group).

One launch carries nine data families, assigned by group (groupnorm_oracle.FAMILIES: ordinary; mean = +-100 sigma; mean 16 with sigma of one
bf16 step; constant; zero; gamma = 0 channels with beta = 0, < 0, > 0; one 2^10 among 2^-6 noise; var << eps), at the smallest shapes that
take each path of the kernels (groupnorm_oracle.SHAPES).  Every operand lives in a util.guarded allocation: inputs between NaN guards and
unchanged afterwards, outputs and the workspace (exactly groupnorm_workspace_bytes) between sentinel guards.

Bounds -- those of tests/test_conv_audit_gpu.py::test_groupnorm_fwd_bwd_on_the_bench_pyramid and Audit.groupnorm_fwd_parts, not retuned:
  mean within 2^-14 x the group's mean |y|; rstd within 2^-14 relative; z, dy: util.bound_ratio(.., 2^-8, 2^-14) <= 1 against S_z / S_dy;
  dgamma, dbeta within 2^-14 S.
The ReLU gate is the float64 one, except where |pre| is within z's tolerance (at most 1 % of a case, checked on the CPU in
tests/test_groupnorm_oracle_cpu.py): there it is the GPU's z > 0, and dy / dgamma / dbeta are recomputed under that gate, so the backward
must have used the gate the forward used.  The gamma = 0, beta = 0 channels are asserted exactly (z = +-0, gate closed).
Two launches agree bit for bit; accumulate=True lands within 2^-23 relative of prior + the plain run's value.

Measured on an MI355X, worst error / bound (each test prints the table per family and quantity):
  with the raw fp32 sums these kernels had (var = E[y^2] - mean^2): rstd 5 - 26 in families b, c, d at every shape but one_pixel, dy up to
  2.6, dgamma up to 2.9 (inf on a constant group, whose scale is 0); fused: rstd 171 (bias = +-100 sigma), 2 206 (dead), 3 814 (constant), z 3.0;
  with (count, mean, M2) partials (shifted accumulation, Chan's update): every ratio <= 0.98 (z, dy: their bf16 rounding), rstd <= 0.15.
"""
import functools

import pytest
import torch

from tests import groupnorm_oracle as O
from tests import util as U

pytestmark = pytest.mark.gpu
C, G = O.C, O.G
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
REL, ABS = 2.0 ** -8, 2.0 ** -14


def _in(data, dtype, name):
    rows, cols = (data.shape[0], None) if data.dim() == 1 else data.shape
    t, h = U.guarded(rows, cols, dtype, "cuda", fill="nan", name=name)
    h.set(data.to(dtype))
    h.snapshot()
    return t, h


def _out(rows, cols, dtype, name):
    return U.guarded(rows, cols, dtype, "cuda", fill="sentinel", name=name)


def _ratio(err, tol):
    """err / tol with 0 / 0 = 0 (a quantity that must be, and is, exact)."""
    return torch.where(err == 0, torch.zeros_like(err), err / tol)


def _bits(t):
    return U.bits_of(t.contiguous())


def _table(title, worst, keys):
    lines = [title, "  family " + " ".join(f"{k:>9}" for k in keys)]
    for f in sorted(next(iter(worst.values()))):
        lines.append(f"  {f:>6} " + " ".join(f"{worst[k][f]:9.3f}" for k in keys))
    print("\n" + "\n".join(lines))


def _per_family(ratio, fam_index, names):
    """worst ratio per family: ratio's last dimension runs over channels or groups, fam_index gives each one's family."""
    return {f: float(ratio[..., fam_index.to(ratio.device) == i].max()) for i, f in enumerate(names)}


@functools.lru_cache(maxsize=None)
def _run(name, relu):
    from basedet_amd import ops
    geom, y, dz, gamma, beta, tie = O.make_case(name)
    N, L, rows = geom.N, geom.nlev, geom.pixels
    (Y, hy), (DZ, hdz), (GA, hga), (BE, hbe) = _in(y, BF16, "y"), _in(dz, BF16, "dz"), _in(gamma, F32, "gamma"), _in(beta, F32, "beta")
    wsb = ops.groupnorm_workspace_bytes(N, L, C, geom.pix_per_img)
    gen = torch.Generator().manual_seed(99)
    prior_g, prior_b = torch.randn(C, generator=gen).cuda(), torch.randn(C, generator=gen).cuda()
    outs = []
    for rep in range(3):            # two plain runs, then accumulate=True onto random dgamma / dbeta
        stats, hs = _out(N * L * G, 2, F32, "stats")
        z, hz = _out(rows, C, BF16, "z")
        ws, hw = _out(wsb, None, U8, "forward workspace")
        ops.groupnorm_fwd(Y, GA, BE, geom, C, O.EPS, relu, stats, z, ws)
        torch.cuda.synchronize()
        dy, hdy = _out(rows, C, BF16, "dy")
        dg, hdg = _out(C, None, F32, "dgamma")
        db, hdb = _out(C, None, F32, "dbeta")
        ws2, hw2 = _out(wsb, None, U8, "backward workspace")
        if rep == 2:
            dg.copy_(prior_g), db.copy_(prior_b)
        ops.groupnorm_bwd(DZ, Y, GA, BE, stats, geom, C, relu, dy, dg, db, ws2, accumulate=rep == 2)
        torch.cuda.synchronize()
        for h in (hs, hz, hw, hdy, hdg, hdb, hw2):
            h.check()
        outs.append(dict(stats=stats.view(N, L, G, 2), z=z, dy=dy, dg=dg, db=db))
    for h in (hy, hdz, hga, hbe):
        h.assert_unchanged()
    return geom, (Y, DZ, GA, BE, tie.cuda()), outs, (prior_g, prior_b)


@pytest.mark.parametrize("name,relu", O.RUNS, ids=[f"{n}-{'relu' if r else 'linear'}" for n, r in O.RUNS])
def test_groupnorm_on_edge_families(name, relu):
    geom, (Y, DZ, GA, BE, tie), outs, (prior_g, prior_b) = _run(name, relu)
    o = outs[0]
    for k, v in o.items():
        assert bool(torch.isfinite(v.float()).all()), f"{k} has unwritten or non-finite elements"
    ref = O.oracle(Y, DZ, GA, BE, O.EPS, relu, geom)
    gfam = torch.tensor([g % len(O.FAMILIES) for g in range(G)])
    cfam = O.channel_family()
    worst = {}
    st = o["stats"].double()
    worst["mean"] = _per_family(_ratio((st[..., 0] - ref["mean"]).abs(), ABS * ref["mean_abs"]), gfam, O.FAMILIES)
    worst["rstd"] = _per_family(_ratio((st[..., 1] - ref["rstd"]).abs(), ABS * ref["rstd"]), gfam, O.FAMILIES)
    worst["z"] = _per_family(U.bound_ratio(o["z"], ref["z"], ref["S_z"], REL, ABS), cfam, O.FAMILIES)
    zf = o["z"].float()
    if relu:
        amb = O.ambiguous(ref)
        share = float((amb & ~tie.view(1, C)).double().mean())
        gate = torch.where(amb, zf > 0, ref["gate"])
        ref = O.oracle(Y, DZ, GA, BE, O.EPS, relu, geom, gate=gate)
    else:
        share, gate = 0.0, ref["gate"]
    worst["dy"] = _per_family(U.bound_ratio(o["dy"], ref["dy"], ref["S_dy"], REL, ABS), cfam, O.FAMILIES)
    worst["dgamma"] = _per_family(_ratio((o["dg"].double() - ref["dgamma"]).abs(), ABS * ref["S_dgamma"]), cfam, O.FAMILIES)
    worst["dbeta"] = _per_family(_ratio((o["db"].double() - ref["dbeta"]).abs(), ABS * ref["S_dbeta"]), cfam, O.FAMILIES)
    keys = ["mean", "rstd", "z", "dy", "dgamma", "dbeta"]
    _table(f"groupnorm {name} relu={relu}: worst error / bound per family (ambiguous gates: {share:.5f} of the case)", worst, keys)
    assert share <= 0.01, share
    for k in keys:
        for f, v in worst[k].items():
            assert v <= 1.0, (k, f, v)
    # ---- exact expectations --------------------------------------------------------------------------------------------------------
    act = (lambda t: t.clamp_min(0)) if relu else (lambda t: t)
    be_bits = _bits(act(BE).to(BF16))
    for g, f in enumerate(O.family_of_group()):
        c = slice(g * 8, g * 8 + 8)
        if f == "e":          # constant group: var = 0, z = bf16(relu(beta)) bit for bit
            assert torch.equal(_bits(o["z"][:, c]), be_bits[c].expand(o["z"].shape[0], 8)), "constant group: z != bf16(relu(beta))"
            assert bool((st[..., g, 0] == 3.0).all())
        if f == "f":
            assert bool((st[..., g, 0] == 0).all())
        if f == "g":
            z0 = _bits(o["z"][:, g * 8:g * 8 + 2])
            assert bool(((z0 & 0x7FFF) == 0).all()), "gamma = 0, beta = 0: z must be +-0"
            assert torch.equal(_bits(o["z"][:, g * 8 + 2:g * 8 + 6]), be_bits[g * 8 + 2:g * 8 + 6].expand(o["z"].shape[0], 4))
            if relu:
                assert not bool(gate[:, g * 8:g * 8 + 4].any()) and bool(gate[:, g * 8 + 4:g * 8 + 6].all())
    # ---- determinism, accumulate -----------------------------------------------------------------------------------------------------
    for k in ("stats", "z", "dy", "dg", "db"):
        assert torch.equal(_bits(outs[0][k]), _bits(outs[1][k])), f"{k} differs between two launches"
    for k in ("stats", "z", "dy"):
        assert torch.equal(_bits(outs[0][k]), _bits(outs[2][k])), f"{k} differs in the accumulate run"
    for got, prior, plain in ((outs[2]["dg"], prior_g, o["dg"]), (outs[2]["db"], prior_b, o["db"])):
        want = prior.double() + plain.double()
        assert bool(((got.double() - want).abs() <= 2.0 ** -23 * want.abs()).all())


# ---- statistics from the convolution's epilogue --------------------------------------------------------------------------------------------
FUSED_FAMILIES = ["ordinary", "bias+100s", "bias-100s", "dead", "constant", "zero"]


def test_groupnorm_statistics_from_the_convolution_epilogue_on_edge_groups():
    """bd_conv2d_fwd_gnstats + bd_groupnorm_fwd_parts, 256 -> 256, N = 2, levels 9x21, 3x4, 1x1 (patches overhang every level; two levels are
    smaller than a 4 x 16 patch).  Output group g is of family FUSED_FAMILIES[g % 6]: ordinary; bias = +-100 x the group's output sigma;
    bias about 5 with the weights scaled by 2^-10 (mean / sigma in the thousands); weights 0 with bias 5.03; weights and bias 0.  The
    statistics must be those of the UNROUNDED float64 convolution for every (image, level, group) (Audit.groupnorm_fwd_parts's bounds); z is
    bounded against the oracle on the GPU's bf16 y normalised with those reference statistics."""
    from basedet_amd import ops
    N, sizes = 2, [(9, 21), (3, 4), (1, 1)]
    geom = ops.Geom(N, [h for h, _ in sizes], [w for _, w in sizes])
    L, rows = geom.nlev, geom.pixels
    gen = torch.Generator().manual_seed(4200)
    x = torch.randn(rows, C, generator=gen).to(BF16)
    w = torch.randn(C, C, 3, 3, generator=gen) / (9 * C) ** 0.5
    bias = torch.randn(C, generator=gen) * 0.5
    gfam = torch.tensor([g % len(FUSED_FAMILIES) for g in range(G)])
    cfam = gfam.repeat_interleave(8)
    w[cfam == 3] *= 2.0 ** -10
    w[cfam >= 4] = 0.0
    bias[cfam == 3] = 5.0 + (torch.arange(C)[cfam == 3] // 8) * 2.0 ** -6
    bias[cfam == 4], bias[cfam == 5] = 5.03, 0.0
    gamma = (torch.randint(0, 2, (C,), generator=gen).float() * 2 - 1) * (0.5 + torch.rand(C, generator=gen))
    beta = torch.randn(C, generator=gen) * 0.3
    d = ops.conv_desc(geom, geom, C, C, 3, 3, 1, 1)
    wf, hwf = _out(C * 9, C, BF16, "w_fwd")
    wd = torch.empty((C * 9, C), dtype=BF16, device="cuda")
    ops.weight_pack(U.oihw_to_ohwi(w).cuda(), None, wf, wd, C, 9, C)
    torch.cuda.synchronize()
    hwf.check(), hwf.snapshot()
    X, hx = _in(x, BF16, "x")
    # bias = +-100 sigma: sigma of the group's response, float64, from the operands the kernel gets
    resp, _, _ = U.conv_ref_fwd(d, X, wf.view(C, 9, C))
    sigma = resp.view(rows, G, 8).permute(1, 0, 2).reshape(G, -1).std(1, correction=0).cpu()
    for g in range(G):
        if gfam[g] in (1, 2):
            bias[g * 8:g * 8 + 8] = (100.0 if gfam[g] == 1 else -100.0) * float(sigma[g])
    (B, hb), (GA, hga), (BE, hbe) = _in(bias, F32, "bias"), _in(gamma, F32, "gamma"), _in(beta, F32, "beta")
    y0 = torch.empty((rows, C), dtype=BF16, device="cuda")
    ops.conv2d_fwd(d, X, wf, B, y0)
    outs = []
    for rep in range(2):
        y, hy = _out(rows, C, BF16, "y")
        part, hp = _out(ops.conv2d_fwd_gnstats_bytes(d) // 4, None, F32, "part")
        ops.conv2d_fwd_gnstats(d, X, wf, B, y, part)
        assert ops.L().bd_conv_last_kernel().decode() == "conv3x3_pp_kernel"
        stats, hs = _out(N * L * G, 2, F32, "stats")
        z, hz = _out(rows, C, BF16, "z")
        ops.groupnorm_fwd_parts(d, y, part, GA, BE, O.EPS, True, stats, z)
        torch.cuda.synchronize()
        for h in (hy, hp, hs, hz):
            h.check()
        outs.append(dict(y=y, part=part, stats=stats.view(N, L, G, 2), z=z))
    for h in (hx, hwf, hb, hga, hbe):
        h.assert_unchanged()
    o = outs[0]
    assert torch.equal(_bits(o["y"]), _bits(y0)), "the fused launch's convolution output differs from bd_conv2d_fwd's"
    for k, v in o.items():
        assert bool(torch.isfinite(v.float()).all()), f"{k} has unwritten or non-finite elements"
    conv64, _, _ = U.conv_ref_fwd(d, X, wf.view(C, 9, C), B)
    by_level = O.oracle(conv64, None, GA, BE, O.EPS, True, geom)            # the statistics of the unrounded convolution
    st = o["stats"].double()
    worst = {}
    worst["mean"] = _per_family(_ratio((st[..., 0] - by_level["mean"]).abs(), ABS * by_level["mean_abs"]), gfam, FUSED_FAMILIES)
    worst["rstd"] = _per_family(_ratio((st[..., 1] - by_level["rstd"]).abs(), ABS * by_level["rstd"]), gfam, FUSED_FAMILIES)
    ref = O.oracle(o["y"], None, GA, BE, O.EPS, True, geom, stats=(by_level["mean"], by_level["var"]))
    worst["z"] = _per_family(U.bound_ratio(o["z"], ref["z"], ref["S_z"], REL, ABS), cfam, FUSED_FAMILIES)
    ms = (by_level["mean"].abs() / by_level["var"].sqrt().clamp_min(1e-300))[..., gfam == 3]
    _table(f"conv -> groupnorm, statistics from the epilogue (dead groups: |mean| / sigma up to {float(ms.max()):.0f}): worst error / bound",
           worst, ["mean", "rstd", "z"])
    assert float(ms.min()) > 1000
    for k, per in worst.items():
        for f, v in per.items():
            assert v <= 1.0, (k, f, v)
    const = (gfam == 4).cuda()
    assert bool((st[..., const, 0] == float(torch.tensor(5.03, dtype=F32))).all()) and bool((st[..., const, 1] == st[0, 0, 4, 1]).all())
    for k in ("y", "part", "stats", "z"):
        assert torch.equal(_bits(outs[0][k]), _bits(outs[1][k])), f"{k} differs between two launches"
