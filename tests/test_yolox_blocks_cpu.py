"""CPU side of the YOLOX feature extractor (basedet_amd/layers/yolox_blocks.py, csrc/yolox_neck.hip): the float64 oracle of
tests/yolox_blocks_oracle.py against hand-worked cases, the tie rule of bd_spp_bwd against the oracle it is compared with, the state
names against the list written out from the reference's constructors, the refusals, and the new symbols."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import yolox_blocks_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"bd_spp_fwd": 7, "bd_spp_bwd": 8, "bd_cat2_fwd": 11, "bd_cat2_bwd": 13, "bd_focus_fwd": 6}          # name -> arguments


def test_spp_on_a_3x3_plane_by_hand():
    """A 5x5 window reaches 2 away from its centre, so clipped to a 3x3 plane it is the whole plane, and so are the larger ones: all
    three pools of every pixel are the plane's maximum, 9.  The gradient of each of the 27 pooled values goes to the pixel holding 9;
    the identity block's stays where it is."""
    x = torch.tensor([[1., 5., 3.], [7., 9., 2.], [4., 8., 6.]], dtype=torch.float64).view(1, 1, 3, 3)
    cat = O.spp_cat(x)
    assert cat.shape == (1, 4, 3, 3) and torch.equal(cat[0, 0], x[0, 0])
    assert all(torch.equal(cat[0, i], torch.full((3, 3), 9., dtype=torch.float64)) for i in (1, 2, 3))
    g = torch.arange(1., 37., dtype=torch.float64).view(1, 4, 3, 3)
    d_x, abs_terms, count = O.spp_bwd_terms(x, g)
    want = g[0, 0].clone()
    want[1, 1] += g[0, 1:].sum()          # 10 + ... + 36 = 621
    assert float(g[0, 1:].sum()) == 621.0 and torch.equal(d_x[0, 0], want)
    assert torch.equal(count[0, 0], torch.tensor([[1., 1., 1.], [1., 28., 1.], [1., 1., 1.]], dtype=torch.float64))
    assert torch.equal(abs_terms, d_x)


def test_ties_go_to_the_first_pixel_of_the_window_in_row_major_order():
    """A constant 4 x 6 plane: every window is one big tie.  torch's float64 CPU max_pool2d autograd sends a window's gradient to the
    window's first in-image pixel in row-major order, (max(cy - r, 0), max(cx - r, 0)): the rule include/basedet_hip.h states for
    bd_spp_bwd, checked here against the very oracle the kernel is compared with."""
    H, W = 4, 6
    for k in (5, 9, 13):
        r = k // 2
        x = torch.full((1, 1, H, W), -0.2783203125, dtype=torch.float64, requires_grad=True)          # SiLU's plateau, a bf16 value
        g = torch.arange(1., H * W + 1., dtype=torch.float64).view(1, 1, H, W)
        (TF.max_pool2d(x, k, 1, r) * g).sum().backward()
        want = torch.zeros(H, W, dtype=torch.float64)
        for cy in range(H):
            for cx in range(W):
                want[max(cy - r, 0), max(cx - r, 0)] += g[0, 0, cy, cx]
        assert torch.equal(x.grad[0, 0], want), k
    # a tie between two distinct positions that is not the window's corner: the earlier one in row-major order wins
    x = torch.zeros((1, 1, 3, 3), dtype=torch.float64)
    x[0, 0, 0, 2] = x[0, 0, 1, 0] = 1.0
    x.requires_grad_(True)
    TF.max_pool2d(x, 5, 1, 2).sum().backward()
    assert float(x.grad[0, 0, 0, 2]) == 9.0 and float(x.grad[0, 0, 1, 0]) == 0.0


def test_focus_channel_order_on_a_2x2_image():
    """(top-left, bottom-left, top-right, bottom-right), 3 channels each (basic_block.py:25-31)."""
    x = torch.arange(12., dtype=torch.float64).view(1, 3, 2, 2)          # x[c][y][x] = 4 c + 2 y + x
    s = O.space_to_depth(x).view(-1)
    assert s.tolist() == [0., 4., 8., 2., 6., 10., 1., 5., 9., 3., 7., 11.]


def test_nearest_upsample_and_its_adjoint():
    x = torch.tensor([[1., 2.], [3., 4.]], dtype=torch.float64).view(1, 1, 2, 2).requires_grad_(True)
    u = O.upsample2x(x)
    assert u[0, 0].tolist() == [[1., 1., 2., 2.], [1., 1., 2., 2.], [3., 3., 4., 4.], [3., 3., 4., 4.]]
    g = torch.arange(16., dtype=torch.float64).view(1, 1, 4, 4)
    (u * g).sum().backward()
    assert x.grad[0, 0].tolist() == [[0. + 1 + 4 + 5, 2. + 3 + 6 + 7], [8. + 9 + 12 + 13, 10. + 11 + 14 + 15]]


def test_bottleneck_and_csp_oracle_wiring():
    """use_add adds the input; a CSPLayer's output depends on both of its branches; faithful outputs are bf16 values."""
    from basedet_amd.layers import yolox_blocks as B
    p = O.double_params(O.random_state(B.param_shapes(B.csp_convs(16, 16, 2)), 1))
    x = torch.randn(2, 16, 4, 5, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    pb = {k[4:]: v for k, v in p.items() if k.startswith("m.0.")}
    h = x[:, :8]
    a, b = O.bottleneck(h, pb, use_add=True), O.bottleneck(h, pb, use_add=False)
    assert torch.allclose(a - b, h, rtol=0, atol=1e-12)
    y = O.csp_layer(x, p, n=2)
    for name in ("conv1.weight", "conv2.weight", "m.1.conv2.weight"):
        q = dict(p)
        q[name] = p[name] * 1.5
        assert not torch.allclose(O.csp_layer(x, q, n=2), y)
    yf = O.csp_layer(x, p, n=2, faithful=True)
    assert torch.equal(yf, yf.to(torch.bfloat16).double()) and not torch.equal(y, y.to(torch.bfloat16).double())


def test_state_names_shapes_and_order():
    from basedet_amd.layers import yolox_blocks as B
    with open(os.path.join(ROOT, "tests", "golden", "yolox_fpn_state.json")) as f:
        gold = json.load(f)
    got = B.pafpn_param_shapes(gold["depth"], gold["width"], gold["in_channels"])
    assert [[k, list(v)] for k, v in got.items()] == gold["state"]
    for name in ("backbone.stem.conv.weight", "backbone.dark2.1.m.0.conv1.norm.running_var", "C3_p4.conv3.weight"):
        assert name in got
    assert got["backbone.stem.conv.weight"] == (32, 12, 3, 3) and got["backbone.dark5.1.conv2.weight"] == (512, 1024, 1, 1)
    # the test sizes of the GPU suite: every channel count a multiple of 8
    small = B.pafpn_param_shapes(0.33, 0.125)
    assert min(v[0] for v in small.values()) == 8 and all(v[0] % 8 == 0 for v in small.values())


def test_refusals_come_before_the_device():
    """No GPU here: anything that reached the device would raise something other than ValueError."""
    import basedet.layers as BL
    from basedet_amd.layers import yolox_blocks as B
    for name in B.__all__:
        assert getattr(BL, name) is getattr(B, name)
    for cls, args in ((B.Bottleneck, (16, 16)), (B.CSPLayer, (16, 16)), (B.CSPDarknet, (0.33, 0.5))):
        with pytest.raises(ValueError, match="depthwise"):
            cls(*args, depthwise=True)
        with pytest.raises(ValueError, match="activation"):
            cls(*args, activation="relu")
    for cls, args in ((B.Focus, (3, 16)), (B.SPPBottleneck, (16, 16))):
        with pytest.raises(ValueError, match="activation"):
            cls(*args, activation="lrelu")
    # channel counts that are no multiple of 8, wherever they arise
    for make in (lambda: B.Focus(3, 12), lambda: B.Focus(4, 16), lambda: B.SPPBottleneck(24, 16), lambda: B.SPPBottleneck(16, 12),
                 lambda: B.Bottleneck(16, 24, expansion=0.25), lambda: B.Bottleneck(12, 16), lambda: B.CSPLayer(16, 24),
                 lambda: B.CSPLayer(16, 16, expansion=0.25), lambda: B.CSPDarknet(0.33, 0.0625), lambda: B.SPPBottleneck(16, 16, (3, 5, 7))):
        with pytest.raises(ValueError):
            make()

    class Stub:          # a bottom_up that never touched the device
        out_features, channels = ("dark3", "dark4", "dark5"), {"dark3": 32, "dark4": 64, "dark5": 128}
    with pytest.raises(ValueError, match="depthwise"):
        B.YOLOPAFPN(Stub(), 0.33, 0.125, depthwise=True)
    with pytest.raises(ValueError):
        B.YOLOPAFPN(Stub(), 0.33, 0.25)          # widths that are not the bottom_up's
    with pytest.raises(ValueError):
        B.YOLOPAFPN(Stub(), 0.33, 0.125, in_features=("dark2", "dark3", "dark4"))
    # an input that is no multiple of 32: refused by the size check, before any launch
    fpn, dark = object.__new__(B.YOLOPAFPN), object.__new__(B.CSPDarknet)
    for m in (fpn, dark):
        with pytest.raises(ValueError, match="multiples of 32"):
            m.forward_pm(None, 1, 64, 80)
    with pytest.raises(ValueError, match="even"):
        object.__new__(B.Focus).forward_pm(torch.zeros((1, 9, 12, 4), dtype=torch.bfloat16), 1, 3, 4)


def test_new_symbols_in_library_header_binding_and_abi():
    from basedet_amd import _lib, build, ops
    assert "yolox_neck.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "basedet_hip.h")).read()
    src = open(os.path.join(ROOT, "basedet_amd", "csrc", "yolox_neck.hip")).read()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert f'extern "C" int {name}(' in src
    assert _lib.ABI_VERSION == 118
    assert all(hasattr(ops, n) for n in ("spp_fwd", "spp_bwd", "cat2_fwd", "cat2_bwd", "focus_fwd"))
    # the built library exports them (and load() refuses one that does not, by name)
    import ctypes
    raw = ctypes.CDLL(build.build(force=False, verbose=False))
    for name in ENTRIES:
        assert hasattr(raw, name), name
    assert int(_lib.load().bd_version()) == 118
    from basedet_amd.models import yolox
    assert callable(yolox.yolox_network_step) and "yolox_network_step" in yolox.__all__
