"""CPU side of the CenterNet neck / head: the float64 oracle against torch.autograd.gradcheck, the initialisation, the refusals, the
parameter names, the new symbols, and the learning rate of the GPU training test."""
import os
import re

import numpy as np
import pytest
import torch

import center_head_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["bd_center_head_out_fwd", "bd_center_head_out_bwd_workspace_bytes", "bd_center_head_out_bwd"]


def _tiny_params(channels, K, modulated, seed=0):
    from basedet_amd.layers import center_head as L
    g = torch.Generator().manual_seed(seed)
    shapes = dict(L.neck_param_shapes(channels, modulated))
    shapes.update(L.head_param_shapes(channels[-1], K))
    p = {k: 0.3 * torch.randn(s, generator=g, dtype=torch.float64) for k, s in shapes.items()}
    for k in p:
        if k.endswith("running_var") or ("_bn." in k and k.endswith(".weight")):
            p[k] = p[k].abs() + 0.5
    return p


@pytest.mark.parametrize("modulated", [False, True])
def test_neck_oracle_gradcheck(modulated):
    p = _tiny_params([2, 3], 2, modulated)
    names = [k for k in p if k.startswith("deconv") and "running" not in k]
    x = torch.randn(2, 2, 3, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).requires_grad_(True)

    def fn(x, *vals):
        q = dict(p)
        q.update(zip(names, vals))
        # (ReLU kinks and floor() of the sampling positions: gradcheck perturbs by 1e-6, the inputs stay clear of both)
        return O.neck(x, q, 1, modulated, True, False)
    assert torch.autograd.gradcheck(fn, (x, *[p[k].clone().requires_grad_(True) for k in names]), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_head_oracle_gradcheck():
    p = _tiny_params([2, 3], 2, True)
    names = [k for k in p if "_head." in k]
    x = torch.randn(1, 3, 3, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).requires_grad_(True)

    def fn(x, *vals):
        return torch.cat(O.head_raw(x, dict(zip(names, vals))), 1)
    assert torch.autograd.gradcheck(fn, (x, *[p[k].clone().requires_grad_(True) for k in names]), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_head_out_oracle_is_the_three_convolutions():
    g = torch.Generator().manual_seed(3)
    M, C, K = 11, 16, 5
    feat = torch.relu(torch.randn(M, 3 * C, generator=g)).to(torch.bfloat16).float()
    ws = [torch.randn(n, C, generator=g).to(torch.bfloat16).float() for n in (K, 2, 2)]
    bs = [torch.randn(n, generator=g) for n in (K, 2, 2)]
    gl, gw = torch.randn(M, K, generator=g), torch.randn(M, 4, generator=g)
    r = O.head_out(feat, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], gl, gw)
    pre = (torch.randn(M, 3 * C, generator=torch.Generator().manual_seed(3))).double()      # the same draw as feat, before the ReLU
    pre = pre.to(torch.bfloat16).double().requires_grad_(True)
    wd = [w.double().requires_grad_(True) for w in ws]
    bd = [b.double().requires_grad_(True) for b in bs]
    f = torch.relu(pre)
    outs = [f[:, i * C:(i + 1) * C] @ wd[i].t() + bd[i] for i in range(3)]
    assert torch.allclose(outs[0], r["logits"]) and torch.allclose(torch.cat(outs[1:], 1), r["wr"])
    loss = (outs[0] * gl.double()).sum() + (torch.cat(outs[1:], 1) * gw.double()).sum()
    grads = torch.autograd.grad(loss, [pre] + wd + bd)
    assert torch.allclose(grads[0], r["d_feat"])
    for i, n in enumerate(("cls", "wh", "reg")):
        assert torch.allclose(grads[1 + i], r["dw_" + n]) and torch.allclose(grads[4 + i], r["db_" + n])


def test_bilinear_init_by_hand():
    from basedet_amd.layers import center_head as L
    v = np.asarray([0.25, 0.75, 0.75, 0.25])          # f = 2, c = 0.75: 1 - |i / 2 - 0.75|
    hand = np.outer(v, v)
    assert hand[0, 0] == 0.0625 and hand[1, 2] == 0.5625
    np.testing.assert_array_equal(L.bilinear_stencil(4), hand)
    np.testing.assert_array_equal(O.bilinear_stencil(4).numpy(), hand)
    w = L.up_sample_init(64, np.random.default_rng(0))
    assert w.shape == (64, 64, 4, 4)
    for c in range(64):
        np.testing.assert_array_equal(w[c, 0], hand.astype(np.float32))
    rest = w[:, 1:]          # only [c, 0] gets the stencil: every other output channel keeps the N(0, sqrt(1 / (16 C))) draw
    assert not np.any(np.all(rest == hand.astype(np.float32), axis=(2, 3)))
    assert abs(rest.std() - (1.0 / (16 * 64)) ** 0.5) < 0.05 * (1.0 / (16 * 64)) ** 0.5 and abs(rest.mean()) < 1e-3


def test_unbuilt_configurations_raise_before_the_device():
    import basedet.layers as BL
    for kw in (dict(deconv_kernel=3), dict(deconv_kernel=4, deconv_stride=1), dict(deconv_kernel=4, deconv_pad=0),
               dict(deconv_kernel=4, deconv_out_pad=1)):
        with pytest.raises(ValueError, match="only"):
            BL.DeconvLayer(64, 64, **kw)
    with pytest.raises(ValueError, match="multiple of 64"):
        BL.DeconvLayer(64, 32, 4)
    with pytest.raises(ValueError, match="multiple of 64"):
        BL.CenternetDeconv([128, 64, 32], [4, 4], True)
    with pytest.raises(ValueError):
        BL.CenternetDeconv([128, 64, 64], [4, 2], False)
    with pytest.raises(ValueError):
        BL.CenterHead(24, 80)
    with pytest.raises(ValueError):
        BL.CenterHead(64, 0)
    with pytest.raises(ValueError):
        BL.CenterHead(128, 365)


def test_parameter_names():
    from basedet_amd.layers import center_head as L
    for modulated, off, dcn, k in ((True, "offset_mask_conv", "dcnv2", 27), (False, "offset_conv", "dcn", 18)):
        s = L.neck_param_shapes([128, 64, 64], modulated)
        want = []
        for i, cin in ((1, 128), (2, 64)):
            want += [f"deconv{i}.dcn.{off}.weight", f"deconv{i}.dcn.{off}.bias", f"deconv{i}.dcn.{dcn}.weight", f"deconv{i}.dcn.{dcn}.bias"]
            want += [f"deconv{i}.dcn_bn.{n}" for n in ("weight", "bias", "running_mean", "running_var")]
            want += [f"deconv{i}.up_sample.weight"]
            want += [f"deconv{i}.up_bn.{n}" for n in ("weight", "bias", "running_mean", "running_var")]
            assert s[f"deconv{i}.dcn.{off}.weight"] == (k, cin, 3, 3) and s[f"deconv{i}.dcn.{dcn}.weight"] == (64, cin, 3, 3)
            assert s[f"deconv{i}.up_sample.weight"] == (64, 64, 4, 4) and s[f"deconv{i}.up_bn.running_var"] == (64,)
        assert list(s) == want
    h = L.head_param_shapes(64, 80)
    assert list(h) == [f"{b}_head.{c}.{n}" for b in ("cls", "wh", "reg") for c in ("feat_conv", "out_conv") for n in ("weight", "bias")]
    assert h["cls_head.out_conv.weight"] == (80, 64, 1, 1) and h["wh_head.out_conv.bias"] == (2,) and h["reg_head.feat_conv.weight"] == (64, 64, 3, 3)
    import basedet.layers as BL
    assert all(hasattr(BL, n) for n in ("DeconvLayer", "CenternetDeconv", "SingleHead", "CenterHead"))
    sh = BL.SingleHead(64, 2)
    assert sh.shapes() == {"feat_conv.weight": (64, 64, 3, 3), "feat_conv.bias": (64,), "out_conv.weight": (2, 64, 1, 1), "out_conv.bias": (2,)}


def test_symbols_declared_bound_and_exported():
    from basedet_amd import _lib
    header = open(os.path.join(ROOT, "include", "basedet_hip.h")).read()
    build = open(os.path.join(ROOT, "basedet_amd", "build.py")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert '"center_head.hip"' in build and _lib.ABI_VERSION >= 116 and lib.bd_version() >= 116
    assert lib.bd_center_head_out_bwd_workspace_bytes(4096, 64, 80) > 0
    assert lib.bd_center_head_out_bwd_workspace_bytes(4096, 24, 80) == 0 and lib.bd_center_head_out_bwd_workspace_bytes(4096, 128, 365) == 0


def test_oracle_loss_falls_at_the_training_tests_learning_rate():
    """The float64 oracle, 20 plain SGD steps on the GPU test's batch (K = 3, DCNv1): the learning rate of that test is chosen here."""
    x, _, _, tgt = O.problem(3)
    q = O.init_params(3, False)
    losses = []
    for _ in range(O.TRAIN_STEPS):
        loss, g = O.loss_and_grads(x, q, tgt, False, False)
        losses.append(loss)
        for k in g:
            q[k] = (q[k].double() - O.TRAIN_LR * g[k]).float()
    assert all(np.isfinite(losses)) and np.mean(losses[-5:]) < np.mean(losses[:5]), losses
