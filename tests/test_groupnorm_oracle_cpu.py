"""tests/groupnorm_oracle.py against torch.nn.functional.group_norm + autograd in float64, its closed forms on a constant group, and the
condition tests/test_groupnorm_edges_gpu.py puts on its inputs: few elements whose ReLU gate the bound on z cannot decide."""
import pytest
import torch
import torch.nn.functional as TF

from tests import groupnorm_oracle as O

C, G = O.C, O.G


def _torch_reference(y, dz, gamma, beta, geom, relu):
    N = geom.N
    yv, dzv = y.view(N, geom.pix_per_img, C), dz.view(N, geom.pix_per_img, C)
    z, dy = torch.zeros_like(yv), torch.zeros_like(yv)
    g, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    dg, db = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for i in range(geom.nlev):
        o, n = geom.off[i], geom.H[i] * geom.W[i]
        x = yv[:, o:o + n].permute(0, 2, 1).contiguous().requires_grad_(True)
        out = TF.group_norm(x, G, g, b, eps=O.EPS)
        if relu:
            out = TF.relu(out)
        z[:, o:o + n] = out.detach().permute(0, 2, 1)
        gx, gg, gb = torch.autograd.grad(out, (x, g, b), dzv[:, o:o + n].permute(0, 2, 1).contiguous())
        dy[:, o:o + n] = gx.permute(0, 2, 1)
        dg += gg
        db += gb
    return z.reshape(-1, C), dy.reshape(-1, C), dg, db


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("relu", [True, False])
def test_oracle_matches_torch_group_norm_in_float64(relu):
    from basedet_amd import ops
    geom = ops.Geom(3, [5, 3, 1], [7, 2, 1])
    gen = torch.Generator().manual_seed(5)
    y = torch.randn(geom.pixels, C, generator=gen, dtype=torch.float64) * 1.5 + 0.3
    dz = torch.randn(geom.pixels, C, generator=gen, dtype=torch.float64)
    gamma = torch.randn(C, generator=gen, dtype=torch.float64)
    beta = torch.randn(C, generator=gen, dtype=torch.float64) * 0.3
    r = O.oracle(y, dz, gamma, beta, O.EPS, relu, geom)
    z, dy, dg, db = _torch_reference(y, dz, gamma, beta, geom, relu)
    assert _rel(r["z"], z) <= 1e-12
    assert _rel(r["dy"], dy) <= 1e-10 and _rel(r["dgamma"], dg) <= 1e-10 and _rel(r["dbeta"], db) <= 1e-10
    # the statistics against the definition, and an explicit gate equal to the oracle's own changes nothing
    y0 = y.view(3, geom.pix_per_img, G, 8)[:, :35]
    assert _rel(r["mean"][:, 0], y0.mean((1, 3))) <= 1e-12 and _rel(r["var"][:, 0], y0.var((1, 3), correction=0)) <= 1e-12
    again = O.oracle(y, dz, gamma, beta, O.EPS, relu, geom, gate=r["gate"])
    assert torch.equal(again["dy"], r["dy"]) and torch.equal(again["dgamma"], r["dgamma"])


def test_oracle_closed_forms_on_a_constant_group():
    """var = 0 exactly and z = relu(beta) exactly.  dy is NOT 0 in general: with xhat = 0 it is (dxh - mean(dxh)) / sqrt(eps), which sums to 0
    over the group, and is 0 everywhere exactly when the ReLU closes the whole group (every beta of it <= 0)."""
    from basedet_amd import ops
    geom = ops.Geom(2, [3, 1], [5, 1])
    gen = torch.Generator().manual_seed(6)
    y = torch.full((geom.pixels, C), 3.0, dtype=torch.float64)
    dz = torch.randn(geom.pixels, C, generator=gen, dtype=torch.float64)
    gamma = torch.randn(C, generator=gen, dtype=torch.float64)
    beta = torch.randn(C, generator=gen, dtype=torch.float64)
    beta[:16] = -beta[:16].abs()            # groups 0 and 1: every gate closed
    r = O.oracle(y, dz, gamma, beta, O.EPS, True, geom)
    assert bool((r["var"] == 0).all()) and bool((r["mean"] == 3.0).all()) and bool((r["rstd"] == O.EPS ** -0.5).all())
    assert torch.equal(r["z"], beta.clamp_min(0).expand_as(r["z"]))
    assert bool((r["dy"][:, :16] == 0).all())
    N, ppi = geom.N, geom.pix_per_img
    on = (beta > 0).to(torch.float64)
    dxh = (dz * on * gamma).view(N, ppi, G, 8)
    for li in range(geom.nlev):
        sl = slice(geom.off[li], geom.off[li] + geom.H[li] * geom.W[li])
        want = (dxh[:, sl] - dxh[:, sl].mean((1, 3), keepdim=True)) * O.EPS ** -0.5
        got = r["dy"].view(N, ppi, G, 8)[:, sl]
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert float(got.sum((1, 3)).abs().max()) <= 1e-9 * float(got.abs().sum((1, 3)).max())


@pytest.mark.parametrize("name", list(O.SHAPES))
def test_few_ambiguous_gates_in_every_family_and_shape(name):
    """At most 1 % of a family's elements (and so of the case's) have |pre| within the tolerance of z; the gamma = 0, beta = 0 ties placed
    on purpose are not counted (the GPU test asserts them exactly)."""
    geom, y, dz, gamma, beta, tie = O.make_case(name)
    assert torch.equal(y, y.to(torch.bfloat16).float()) and torch.equal(dz, dz.to(torch.bfloat16).float())
    r = O.oracle(y, dz, gamma, beta, O.EPS, True, geom)
    amb = O.ambiguous(r) & ~tie.view(1, C)
    assert bool(O.ambiguous(r)[:, tie].all())
    fam = O.channel_family()
    shares = {f: float(amb[:, fam == i].double().mean()) for i, f in enumerate(O.FAMILIES)}
    print(name, {f: round(s, 5) for f, s in shares.items()})
    assert max(shares.values()) <= 0.01, shares
    # the families are what they claim
    st = {k: r[k].view(-1, G) for k in ("mean", "var")}
    for g, f in enumerate(O.family_of_group()):
        m, v = st["mean"][:, g], st["var"][:, g]
        if f in "ef":
            assert bool((v == 0).all()) and bool((m == (3.0 if f == "e" else 0.0)).all())
        if f in "bc" and name == "33_slots":
            assert bool((m.abs() / v.sqrt() > 90).all())
        if f == "i":
            assert bool((v < O.EPS / 4).all())
