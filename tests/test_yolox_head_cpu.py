"""CPU side of ConvBNSiLU / YOLOXHead: the float64 oracle against hand-worked values, the state names against the list written out from the
reference's constructor, the initial predictor biases, the refusals, and the new symbols."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import yolox_head_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"bd_bn_silu_fwd": 14, "bd_bn_silu_bwd_reduce": 18, "bd_bn_silu_bwd_apply": 20}          # name -> arguments


def test_silu_and_its_derivative_by_hand():
    """silu(u) = u / (1 + e^-u); silu'(u) = s (1 + u (1 - s)).  Values worked by hand from e = 2.718281828459045:
    s(1) = 1 / (1 + 1 / e) = 0.7310585786300049, s(-1) = 0.2689414213699951."""
    s1, sm1 = 0.7310585786300049, 0.2689414213699951
    want = {0.0: (0.0, 0.5), 1.0: (s1, s1 * (1 + sm1)), -1.0: (-sm1, sm1 * (1 - s1)),
            20.0: (20.0 / (1 + math.exp(-20.0)), 1.0 + 19.0 * math.exp(-20.0)),          # s = 1 - e^-20 + O(e^-40); s' = 1 + 19 e^-20 + O(e^-40)
            -20.0: (-20.0 * math.exp(-20.0), -19.0 * math.exp(-20.0)),                  # s = e^-20 (1 - e^-20 + ...)
            100.0: (100.0, 1.0), -100.0: (-100.0 * math.exp(-100.0), -99.0 * math.exp(-100.0))}
    for u, (z, dz) in want.items():
        assert np.isclose(float(O.silu(u)), z, rtol=1e-8, atol=0.0), u
        assert np.isclose(float(O.silu_grad(u)), dz, rtol=1e-8, atol=0.0), u
    assert np.all(np.isfinite(O.silu_grad(np.array([-745.0, -1e4, 1e4, 745.0]))))
    # the autograd path of the layer oracle agrees with the formula
    u = torch.tensor([0.0, 1.0, -1.0, 20.0, -20.0, 100.0, -100.0], dtype=torch.float64, requires_grad=True)
    (u * torch.sigmoid(u)).sum().backward()
    assert np.allclose(u.grad.numpy(), O.silu_grad(u.detach().numpy()), rtol=1e-12, atol=1e-300)


def test_oracle_constant_channel_and_statistics():
    """A constant channel: variance 0, xhat = 0, u = beta, z = silu(beta); the batch norm uses the BIASED
    variance and moves the running statistics with the unbiased one (momentum 0.03 in torch's convention)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1, 3, 4, generator=g, dtype=torch.float64)
    p = {"weight": torch.tensor([[[[2.0]]], [[[0.0]]]], dtype=torch.float64), "norm.weight": torch.tensor([1.5, -0.5], dtype=torch.float64),
         "norm.bias": torch.tensor([0.25, 0.75], dtype=torch.float64), "norm.running_mean": torch.tensor([1.0, 2.0], dtype=torch.float64),
         "norm.running_var": torch.tensor([3.0, 4.0], dtype=torch.float64)}
    q = {k: v.clone().requires_grad_("running" not in k) for k, v in p.items()}
    xr = x.clone().requires_grad_(True)
    stats = {}
    z = O.conv_bn_silu(xr, q, "", 1, stats=stats)
    y = 2.0 * x[:, 0]
    M = y.numel()
    mu, var = y.mean(), ((y - y.mean()) ** 2).sum() / M
    u = 1.5 * (y - mu) / torch.sqrt(var + O.EPS) + 0.25
    assert torch.allclose(z[:, 0], u * torch.sigmoid(u), rtol=1e-12, atol=0)
    assert torch.allclose(z[:, 1], torch.full_like(z[:, 1], float(O.silu(0.75))), rtol=1e-12, atol=0)
    assert np.isclose(float(stats["norm.running_mean"][0]), 0.97 * 1.0 + 0.03 * float(mu), rtol=1e-12)
    assert np.isclose(float(stats["norm.running_var"][0]), 0.97 * 3.0 + 0.03 * float(var) * M / (M - 1), rtol=1e-12)
    assert float(stats["norm.running_mean"][1]) == 0.97 * 2.0 and np.isclose(float(stats["norm.running_var"][1]), 0.97 * 4.0, rtol=1e-15)
    (z * torch.randn(z.shape, generator=g, dtype=torch.float64)).sum().backward()
    # the formula oracle of the kernels against the autograd oracle of the layer
    gz = torch.randn(M, 2, generator=g, dtype=torch.float64)
    yy = torch.stack([y.reshape(-1), torch.full((M,), 3.25, dtype=torch.float64)], 1).requires_grad_(True)
    gam, bet = torch.tensor([1.5, -0.5], dtype=torch.float64, requires_grad=True), torch.tensor([0.25, 0.75], dtype=torch.float64, requires_grad=True)
    m2, v2 = yy.mean(0), yy.var(0, unbiased=False)
    uu = gam * (yy - m2) / torch.sqrt(v2 + O.EPS) + bet
    ((uu * torch.sigmoid(uu)) * gz).sum().backward()
    inv = (1.0 / torch.sqrt(v2 + O.EPS)).detach().numpy()
    _, _, dg, db, gy = O.bn_silu_bwd(gz.numpy(), yy.detach().numpy(), m2.detach().numpy(), inv, gam.detach().numpy(), bet.detach().numpy())
    assert np.allclose(dg, gam.grad.numpy(), rtol=1e-9, atol=1e-12) and np.allclose(db, bet.grad.numpy(), rtol=1e-9, atol=1e-12)
    assert np.allclose(gy, yy.grad.numpy(), rtol=1e-7, atol=1e-10)


def test_faithful_switch_rounds_where_the_device_does():
    p = O.double_params(O.head_state(3))
    xs = [x.double() for x in O.head_inputs()]
    a, b = O.head(xs, p, True, False), O.head(xs, p, True, True)
    for la, lb in zip(a, b):
        for ta, tb in zip(la, lb):
            assert torch.equal(tb, tb.to(torch.bfloat16).double()) and not torch.equal(ta, ta.to(torch.bfloat16).double())
            assert float((ta - tb).abs().max()) < 0.1


def test_state_names_shapes_and_order():
    from basedet_amd.layers.yolox_head import head_param_shapes
    with open(os.path.join(ROOT, "tests", "golden", "yolox_head_state.json")) as f:
        gold = json.load(f)
    got = head_param_shapes(gold["num_classes"], gold["in_channels"], gold["mid_channels"])
    assert [[k, list(v)] for k, v in got.items()] == gold["state"]
    assert "stems.0.weight" in got and "cls_convs.1.0.norm.running_var" in got and "obj_preds.2.bias" in got


def test_initial_pred_biases_and_refusals():
    """The constructor's argument checks raise before the device is touched (no GPU here: anything later would raise something else)."""
    import basedet.layers as BL
    from basedet_amd.layers import yolox_head as Y
    assert BL.YOLOXHead is Y.YOLOXHead and BL.ConvBNSiLU is Y.ConvBNSiLU
    with pytest.raises(ValueError):
        Y.YOLOXHead(80, act="relu")
    with pytest.raises(ValueError):
        Y.YOLOXHead(80, depthwise=True)
    with pytest.raises(ValueError):
        Y.YOLOXHead(80, in_channels=[256, 500, 1024])
    with pytest.raises(ValueError):
        Y.YOLOXHead(80, mid_channels=100)
    with pytest.raises(ValueError):
        Y.YOLOXHead(0)
    for args in ((32, 32, 5), (32, 32, 3, 3), (12, 32, 3), (32, 20, 1), (0, 32, 1)):
        with pytest.raises(ValueError):
            Y.ConvBNSiLU(*args)
    assert (Y.BN_EPS, Y.BN_MOMENTUM) == (1e-3, 0.03) and abs((1 - 0.97) - Y.BN_MOMENTUM) < 1e-12
    # the initial biases: -log((1 - p) / p) for cls_preds and obj_preds (init_module), zero for reg_preds -- by hand for p = 0.01: -log(99)
    assert np.isclose(-math.log((1 - 0.01) / 0.01), -4.59511985013459, rtol=1e-14)
    src = open(os.path.join(ROOT, "basedet_amd", "layers", "yolox_head.py")).read()
    assert "bias_value = -math.log((1 - prior_prob) / prior_prob)" in src and 'cp._store.w["bias"][:K] = bias_value' in src \
        and 'rp._store.w["bias"][4] = bias_value' in src


def test_new_symbols_in_header_binding_and_abi():
    from basedet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "basedet_hip.h")).read()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.ABI_VERSION == 118
    src = open(os.path.join(ROOT, "basedet_amd", "csrc", "batchnorm.hip")).read()
    for name in ENTRIES:
        assert f'extern "C" int {name}(' in src
    from basedet_amd import ops
    assert all(hasattr(ops, n) for n in ("bn_silu_fwd", "bn_silu_bwd_reduce", "bn_silu_bwd_apply"))
    from basedet_amd.models import yolox
    assert callable(yolox.yolox_head_step)
