"""float64 restatement of GroupNorm(32, 256) (+ ReLU) as csrc/norm.hip computes it (bd_groupnorm_fwd / _bwd / _fwd_parts), per (image, level,
group), and the edge cases tests/test_groupnorm_edges_gpu.py and tests/test_groupnorm_oracle_cpu.py share.

y, dz (N * pix_per_img, 256): pixel-major, several pyramid levels per image (ops.Geom); a group is 8 consecutive channels, normalised over
the H_l W_l pixels of one level of one image.  With xhat = (y - mean) rstd, rstd = 1 / sqrt(var + eps) (biased variance):
    pre = xhat gamma + beta,  z = relu(pre) (or pre),  gate = pre > 0 (or every element; or the tensor passed in)
    d = dz gate,  dxh = d gamma,  dy = rstd (dxh - mean(dxh) - xhat mean(dxh xhat)),  dgamma = sum d xhat,  dbeta = sum d
The scales the kernels' errors are measured against are those of tests/test_conv_audit_gpu.py::test_groupnorm_fwd_bwd_on_the_bench_pyramid:
    S_z = |gamma| rstd (|y| + |mean|) + |beta|
    S_dy = rstd (|dxh| + mean|dxh| + |xhat| mean|dxh xhat|),  S_dgamma = sum |d xhat|,  S_dbeta = sum |d|,  mean_abs = mean |y|
Rows that no level owns are NaN in the per-element results."""
import math

import torch

C, G, CPG = 256, 32, 8
REL_BF16, ABS_STAT = 2.0 ** -8, 2.0 ** -14


def oracle(y, dz, gamma, beta, eps, relu, geom, gate=None, stats=None):
    """dict of float64 tensors on y's device.  mean, var, rstd, mean_abs: (N, L, 32); pre, z, dy, S_z, S_dy, gate: (N * pix_per_img, 256);
    dgamma, dbeta, S_dgamma, S_dbeta: (256,).  gate: bool (N * pix_per_img, 256) to use instead of pre > 0.  stats = (mean, var), each
    (N, L, 32): normalise with these instead of y's own (the statistics a producer took before it rounded y).  dz = None: forward only."""
    N, ppi, L, dev = geom.N, geom.pix_per_img, geom.nlev, y.device
    y64 = y.double().view(N, ppi, G, CPG)
    gm, bm = gamma.double().to(dev).view(1, 1, G, CPG), beta.double().to(dev).view(1, 1, G, CPG)
    nan = lambda: torch.full((N, ppi, G, CPG), float("nan"), dtype=torch.float64, device=dev)
    out = {k: torch.zeros((N, L, G), dtype=torch.float64, device=dev) for k in ("mean", "var", "rstd", "mean_abs")}
    out.update({k: nan() for k in ("pre", "z", "S_z")})
    out["gate"] = torch.zeros((N, ppi, G, CPG), dtype=torch.bool, device=dev)
    if dz is not None:
        dz64 = dz.double().view(N, ppi, G, CPG)
        out.update({k: nan() for k in ("dy", "S_dy")})
        out.update({k: torch.zeros(C, dtype=torch.float64, device=dev) for k in ("dgamma", "dbeta", "S_dgamma", "S_dbeta")})
    for li in range(L):
        sl = slice(geom.off[li], geom.off[li] + geom.H[li] * geom.W[li])
        yv = y64[:, sl]
        if stats is None:
            mu = yv.mean((1, 3), keepdim=True)
            var = yv.var((1, 3), correction=0, keepdim=True)
        else:
            mu, var = (s[:, li].double().to(dev).view(N, 1, G, 1) for s in stats)
        rstd = 1.0 / torch.sqrt(var + eps)
        out["mean"][:, li], out["var"][:, li], out["rstd"][:, li] = mu.view(N, G), var.view(N, G), rstd.view(N, G)
        out["mean_abs"][:, li] = yv.abs().mean((1, 3))
        xh = (yv - mu) * rstd
        pre = xh * gm + bm
        out["pre"][:, sl] = pre
        out["z"][:, sl] = pre.clamp_min(0) if relu else pre
        out["S_z"][:, sl] = gm.abs() * rstd * (yv.abs() + mu.abs()) + bm.abs()
        if gate is not None:
            on = gate.view(N, ppi, G, CPG)[:, sl]
        else:
            on = pre > 0 if relu else torch.ones_like(pre, dtype=torch.bool)
        out["gate"][:, sl] = on
        if dz is None:
            continue
        d = dz64[:, sl] * on
        dxh = d * gm
        m1 = dxh.mean((1, 3), keepdim=True)
        m2 = (dxh * xh).mean((1, 3), keepdim=True)
        out["dy"][:, sl] = rstd * (dxh - m1 - xh * m2)
        out["S_dy"][:, sl] = rstd * (dxh.abs() + dxh.abs().mean((1, 3), keepdim=True) + xh.abs() * (dxh * xh).abs().mean((1, 3), keepdim=True))
        out["dgamma"] += (d * xh).sum((0, 1)).reshape(C)
        out["S_dgamma"] += (d * xh).abs().sum((0, 1)).reshape(C)
        out["dbeta"] += d.sum((0, 1)).reshape(C)
        out["S_dbeta"] += d.abs().sum((0, 1)).reshape(C)
    for k in ("pre", "z", "S_z", "gate", "dy", "S_dy"):
        if k in out:
            out[k] = out[k].view(N * ppi, C)
    return out


def ambiguous(ref):
    """Elements whose ReLU gate the bound on z cannot decide: |pre| <= 2^-8 |pre| + 2^-14 S_z (rows no level owns: False)."""
    pre = ref["pre"]
    return torch.nan_to_num(pre.abs() - (REL_BF16 * pre.abs() + ABS_STAT * ref["S_z"]), nan=1.0) <= 0


# ---- the edge cases --------------------------------------------------------------------------------------------------------------------
# One launch carries every data family: group g holds family FAMILIES[g % 9].
#   a  randn 1.5 + 0.3                      b  mean = +100 sigma            c  mean = -100 sigma
#   d  mean 16, sigma 0.125 (one bf16 step)  e  3.0 everywhere               f  0 everywhere
#   g  data as a; channels 0 .. 5 of the group have gamma = 0 with beta = +0, -0, < 0, < 0, > 0, > 0
#   h  one element 2^10 per (image, level, group) among randn 2^-6           i  randn 2^-10 (var << eps)
# Every value is a bf16 number.  gamma = +-(0.5 .. 1.5), beta = +-(0.3 .. 0.7), signs drawn per channel: |beta| >= 0.2 |gamma| keeps pre away
# from 0 where the whole group sits on one xhat (e, f).  In b, c, d beta is placed (make_case) so that pre's zero lies between two bf16 values.
FAMILIES = "abcdefghi"
EPS = 1e-5
SHAPES = {            # name: (N, [(H, W)]) -- the smallest at which each path of norm.hip is taken
    "one_pixel": (2, [(1, 1)]),                                                      # a group is 8 numbers
    "short_levels": (3, [(1, 7), (3, 43), (16, 8), (1, 1)]),                          # 7 (< 8 pixel lanes), 129, 128 and 1 pixels
    "33_slots": (1, [(65, 64)]),                                                     # second trip of gn_stats_final_kernel, five of gn_bwd_final_body
    "8_levels": (2, [(9, 9), (5, 5), (3, 3), (2, 2), (1, 3), (1, 2), (1, 1), (1, 1)]),          # BD_MAX_SEGS levels
}
RUNS = [("one_pixel", True), ("short_levels", True), ("short_levels", False), ("33_slots", True), ("8_levels", True)]
SIGMA_BC = (1.0, 0.25, 3.0, 1.0)            # family b / c: sigma of the k-th group of the family


def family_of_group():
    return [FAMILIES[g % len(FAMILIES)] for g in range(G)]


def channel_family():
    """(256,) int64: index into FAMILIES of every channel."""
    return torch.tensor([g % len(FAMILIES) for g in range(G)]).repeat_interleave(CPG)


def make_geom(name):
    from basedet_amd import ops
    N, sizes = SHAPES[name]
    return ops.Geom(N, [h for h, _ in sizes], [w for _, w in sizes])


# one_pixel has 64 elements per family, so ONE ambiguous gate is 1.6 % of a family: its seed is the first from 4100 on with none in b, c, d
# (tests/test_groupnorm_oracle_cpu.py checks the condition for every case)
SEEDS = {"one_pixel": 4102, "short_levels": 4111, "33_slots": 4112, "8_levels": 4113}


def make_case(name, seed=None):
    """(geom, y, dz, gamma, beta, tie): y, dz float32 holding bf16 values (CPU); tie (256,) bool = the gamma = 0, beta = 0 channels."""
    geom = make_geom(name)
    N, ppi = geom.N, geom.pix_per_img
    gen = torch.Generator().manual_seed(SEEDS[name] if seed is None else seed)
    y = torch.zeros(N, ppi, G, CPG)
    for li in range(geom.nlev):
        n_px = geom.H[li] * geom.W[li]
        sl = slice(geom.off[li], geom.off[li] + n_px)
        for g, fam in enumerate(family_of_group()):
            r = torch.randn(N, n_px, CPG, generator=gen)
            if fam in "ag":
                v = r * 1.5 + 0.3
            elif fam in "bc":
                s = SIGMA_BC[g // len(FAMILIES)]
                v = (100.0 if fam == "b" else -100.0) * s + s * r
            elif fam == "d":
                v = 16.0 + 0.125 * r
            elif fam == "e":
                v = torch.full_like(r, 3.0)
            elif fam == "f":
                v = torch.zeros_like(r)
            elif fam == "h":
                v = r * 2.0 ** -6
                at = torch.randint(0, n_px * CPG, (N,), generator=gen)
                v.view(N, -1)[torch.arange(N), at] = 2.0 ** 10
            else:
                v = r * 2.0 ** -10
            y[:, sl, g] = v
    y = y.to(torch.bfloat16).float().view(N * ppi, C)
    dz = torch.randn(N * ppi, C, generator=gen).to(torch.bfloat16).float()
    sign = lambda: torch.randint(0, 2, (C,), generator=gen).float() * 2 - 1
    gamma = sign() * (0.5 + torch.rand(C, generator=gen))
    beta = sign() * (0.3 + 0.4 * torch.rand(C, generator=gen))
    tie = torch.zeros(C, dtype=torch.bool)
    for g, fam in enumerate(family_of_group()):
        if fam in "bcd":
            # sigma is about one bf16 step here, so xhat sits on a coarse lattice and a zero of pre that fell ON a lattice point would make a
            # fifth of the channel ambiguous: beta puts the zero half-way between two lattice points near the mean (nominal mean and sigma)
            m0, s0 = (16.0, 0.125) if fam == "d" else ((100.0 if fam == "b" else -100.0) * SIGMA_BC[g // len(FAMILIES)], SIGMA_BC[g // len(FAMILIES)])
            step = 2.0 ** (math.floor(math.log2(abs(m0))) - 7)
            # (d: above 16 only -- below it the bf16 step halves, and a half step of the upper lattice is a point of the lower one)
            k = torch.randint(0 if fam == "d" else -2, 2, (CPG,), generator=gen).float()
            c = slice(g * CPG, (g + 1) * CPG)
            beta[c] = -gamma[c] * step * (k + 0.5) / math.sqrt(s0 * s0 + step * step / 12)
        if fam == "g":
            c0 = g * CPG
            gamma[c0:c0 + 6] = 0.0
            beta[c0:c0 + 6] = torch.tensor([0.0, -0.0, -0.4, -0.25, 0.4, 0.25])
            tie[c0:c0 + 2] = True
    return geom, y, dz, gamma, beta, tie
