"""The float64 oracle of the deformable convolution (tests/deform_conv_oracle.py) against torch and against values worked out by hand, and
the constructor checks of basedet.layers.DeformConvWithOff / ModulatedDeformConvWithOff (no GPU needed: they validate before touching it)."""
import pytest
import torch
import torch.nn.functional as TF

import deform_conv_oracle as O


def _rand(N, H, W, Cin, Cout, ld, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, 3, 3, Cin, generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    om = torch.randn(N, H, W, ld, generator=g, dtype=torch.float64)
    return x, om, w, b


@pytest.mark.parametrize("modulated", [False, True])
def test_zero_offsets_unit_mask_is_conv2d(modulated):
    x, om, w, b = _rand(2, 5, 7, 3, 4, 32, 0)
    om.zero_()
    om[..., 18:27] = 60.0              # sigmoid(60) = 1 - 9e-27: 1.0 in float64
    got = O.forward(x, om, w, b, modulated)
    want = TF.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, padding=1).permute(0, 2, 3, 1)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("modulated", [False, True])
def test_gradcheck_at_non_integer_positions(modulated):
    x, om, w, b = _rand(1, 4, 5, 2, 3, 32, 1)
    # offsets with fractional parts in [0.2, 0.8]: at least 0.2 away from every floor kink and from the -1 / H / W cut
    g = torch.Generator().manual_seed(2)
    frac = 0.2 + 0.6 * torch.rand(om[..., :18].shape, generator=g, dtype=torch.float64)
    om[..., :18] = torch.randint(-3, 3, frac.shape, generator=g).double() + frac
    leaves = [t.clone().requires_grad_(True) for t in (x, om, w, b)]
    assert torch.autograd.gradcheck(lambda *a: O.forward(*a, modulated), leaves, eps=1e-6, atol=1e-7, rtol=1e-6)


def _one_tap_problem(dy_off, dx_off, tap=4):
    """1 x 3 x 3 x 1 image x[y][x] = 10 y + x + 1, one output channel whose weight is 1 at `tap` only; every tap's offset = (dy_off, dx_off)."""
    x = (10.0 * torch.arange(3).view(3, 1) + torch.arange(3).view(1, 3) + 1.0).double().view(1, 3, 3, 1)
    w = torch.zeros(1, 9, 1, dtype=torch.float64)
    w[0, tap, 0] = 1.0
    om = torch.zeros(1, 3, 3, 24, dtype=torch.float64)
    om[..., 0:18:2] = dy_off
    om[..., 1:18:2] = dx_off
    return x, om, w.view(1, 3, 3, 1), torch.zeros(1, dtype=torch.float64)


def test_sample_at_exactly_minus_one_is_dead():
    # centre tap of output pixel (0, 1) with dy = -1: h = -1 exactly -> value 0 and gradient 0 (the rule is -1 < h, strictly)
    x, om, w, b = _one_tap_problem(-1.0, 0.0)
    dy = torch.zeros(1, 3, 3, 1, dtype=torch.float64)
    dy[0, 0, 1, 0] = 1.0
    r = O.oracle(x, om, w, b, dy, False)
    assert r["y"][0, 0, 1, 0] == 0.0
    assert torch.count_nonzero(r["d_x"]) == 0 and torch.count_nonzero(r["d_om"]) == 0 and r["d_w"][0, 1, 1, 0] == 0.0
    # one step inside (h = -0.5): half of row 0
    x, om, w, b = _one_tap_problem(-0.5, 0.0)
    r = O.oracle(x, om, w, b, dy, False)
    assert r["y"][0, 0, 1, 0] == 0.5 * 2.0
    assert r["d_om"][0, 0, 1, 8] == 2.0            # d/dh = x[0][1] - 0 (the row above the image is zero)


def test_integer_interior_coordinate_takes_right_hand_derivative():
    # centre tap of output pixel (1, 1), zero offset: h = w = 1 exactly.  value x[1][1] = 12; d/dh = x[2][1] - x[1][1] = 10 (right-hand;
    # the left-hand one, x[1][1] - x[0][1], is 10 as well here, so the image gets a kink: x[0][1] = 100)
    x, om, w, b = _one_tap_problem(0.0, 0.0)
    x[0, 0, 1, 0] = 100.0
    x[0, 1, 0, 0] = -50.0
    dy = torch.zeros(1, 3, 3, 1, dtype=torch.float64)
    dy[0, 1, 1, 0] = 1.0
    r = O.oracle(x, om, w, b, dy, False)
    assert r["y"][0, 1, 1, 0] == 12.0
    assert r["d_om"][0, 1, 1, 8] == 22.0 - 12.0     # x[2][1] - x[1][1], not 12 - 100
    assert r["d_om"][0, 1, 1, 9] == 13.0 - 12.0     # x[1][2] - x[1][1], not 12 + 50
    assert r["d_x"][0, 1, 1, 0] == 1.0 and r["d_x"].sum() == 1.0
    # at h = H - 1 the right-hand neighbour is the zero row below the image
    dy.zero_()
    dy[0, 2, 1, 0] = 1.0
    r = O.oracle(x, om, w, b, dy, False)
    assert r["d_om"][0, 2, 1, 8] == 0.0 - 22.0


def test_modulated_mask_gradient_is_for_the_logit():
    x, om, w, b = _one_tap_problem(0.0, 0.0)
    om = torch.cat([om, torch.zeros(1, 3, 3, 8, dtype=torch.float64)], -1)
    om[..., 18 + 4] = 0.5
    dy = torch.zeros(1, 3, 3, 1, dtype=torch.float64)
    dy[0, 1, 1, 0] = 1.0
    r = O.oracle(x, om, w, b, dy, True)
    m = torch.sigmoid(torch.tensor(0.5, dtype=torch.float64))
    assert torch.allclose(r["y"][0, 1, 1, 0], m * 12.0)
    assert torch.allclose(r["d_om"][0, 1, 1, 22], m * (1 - m) * 12.0)
    assert torch.count_nonzero(r["d_om"][..., 27:]) == 0


def test_s_bounds_the_result():
    x, om, w, b = _rand(2, 5, 6, 8, 8, 32, 3)
    dy = torch.randn(2, 5, 6, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    r = O.oracle(x, om, w, b, dy, True)
    for k in ("y", "d_x", "d_om", "d_w", "d_b"):
        assert bool((r[k].abs() <= r["S_" + k] * (1 + 1e-12) + 1e-300).all()), k


@pytest.mark.parametrize("name", ["DeformConvWithOff", "ModulatedDeformConvWithOff"])
@pytest.mark.parametrize("kw", [dict(kernel_size=5), dict(stride=2), dict(dilation=2), dict(deformable_groups=2), dict(in_channels=12)])
def test_layers_refuse_what_is_not_built(name, kw):
    import basedet.layers
    cls = getattr(basedet.layers, name)
    args = dict(in_channels=16, out_channels=8)
    args.update(kw)
    with pytest.raises(ValueError):
        cls(**args)
