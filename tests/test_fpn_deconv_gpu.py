"""MODEL.FPN.UPSAMPLE = "deconv" on the GPU: the csrc/fpn_deconv.hip kernels against torch-CPU fp32 conv_transpose2d and its autograd,
against the generic convolution kernels run on the same math (the fine -> coarse Conv2d(k4, s2, p1) view), and the training step of
a deconv RetinaNet / FCOS against an oracle whose FPN uses conv_transpose2d (fpn_backbone.py:92-103,131-138)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from util import bf16_round, nchw_to_pm, pm_to_nchw, rel_l2

pytestmark = pytest.mark.gpu

SHAPES = [(2, 25, 42, 256), (2, 50, 84, 256), (2, 7, 11, 128), (2, 1, 1, 256), (3, 1, 9, 128)]


def _operands(N, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = bf16_round(torch.randn(N, C, H, W, generator=g))
    w = torch.randn(C, C, 4, 4, generator=g) * (2.0 / (16 * C)) ** 0.5       # (C_coarse, C_fine, 4, 4): random, asymmetric
    add = bf16_round(torch.randn(N, C, 2 * H, 2 * W, generator=g))
    dy = bf16_round(torch.randn(N, C, 2 * H, 2 * W, generator=g))
    addc = bf16_round(torch.randn(N, C, H, W, generator=g))
    return x, w, add, dy, addc


def _packed(ops, w):
    C = w.shape[0]
    master = w.permute(0, 2, 3, 1).contiguous().cuda()                     # conv view OHWI [C_coarse][4][4][C_fine]
    wf = torch.empty((4, C, 4, C), dtype=torch.bfloat16, device="cuda")
    wd = torch.empty((C, 16, C), dtype=torch.bfloat16, device="cuda")
    ops.fpn_deconv_pack(master, C, wf, wd)
    return master, wf, wd


def _reference(x, w, add, dy, addc):
    wq = bf16_round(w)
    xr = x.clone().requires_grad_(True)
    wr = wq.clone().requires_grad_(True)
    y = TF.conv_transpose2d(xr, wr, stride=2, padding=1)
    (y * dy).sum().backward()
    return y.detach() + add, xr.grad + addc, wr.grad


@pytest.mark.parametrize("N,H,W,C", SHAPES)
def test_deconv_kernels_match_torch(N, H, W, C):
    from basedet_amd import ops
    x, w, add, dy, addc = _operands(N, H, W, C, seed=H * 131 + W)
    y_ref, dx_ref, dw_ref = _reference(x, w, add, dy, addc)
    master, wf, wd = _packed(ops, w)
    # forward with the fused lateral add, in place
    y = nchw_to_pm(add)
    ops.fpn_deconv_fwd(nchw_to_pm(x), wf, y, N, H, W, C, add=y)
    assert rel_l2(pm_to_nchw(y, N, 2 * H, 2 * W), y_ref) < 1e-2
    # data gradient accumulating in place
    dx = nchw_to_pm(addc)
    ops.fpn_deconv_dgrad(nchw_to_pm(dy), wd, dx, N, H, W, C, add=dx)
    assert rel_l2(pm_to_nchw(dx, N, H, W), dx_ref) < 1e-2
    # weight gradient, stored and accumulated, in the master's (conv view) layout
    ws = torch.empty((ops.fpn_deconv_wgrad_workspace_bytes(N, H, W, C) // 4 + 64,), dtype=torch.float32, device="cuda")
    dw = torch.full((C, 4, 4, C), 7.0, dtype=torch.float32, device="cuda")
    ops.fpn_deconv_wgrad(nchw_to_pm(x), nchw_to_pm(dy), dw, ws, N, H, W, C, accumulate=False)
    got = dw.cpu().permute(0, 3, 1, 2)
    assert rel_l2(got, dw_ref) < 2e-3
    ops.fpn_deconv_wgrad(nchw_to_pm(x), nchw_to_pm(dy), dw, ws, N, H, W, C, accumulate=True)
    assert rel_l2(dw.cpu().permute(0, 3, 1, 2), 2 * dw_ref) < 2e-3


def test_deconv_kernels_are_bitwise_repeatable():
    from basedet_amd import ops
    N, H, W, C = 2, 25, 42, 256
    x, w, add, dy, addc = _operands(N, H, W, C, seed=5)
    _, wf, wd = _packed(ops, w)
    xd, dyd, ad, acd = nchw_to_pm(x), nchw_to_pm(dy), nchw_to_pm(add), nchw_to_pm(addc)
    ws = torch.empty((ops.fpn_deconv_wgrad_workspace_bytes(N, H, W, C) // 4 + 64,), dtype=torch.float32, device="cuda")
    outs = []
    for _ in range(2):
        y = ops.fpn_deconv_fwd(xd, wf, torch.empty_like(ad), N, H, W, C, add=ad)
        dx = ops.fpn_deconv_dgrad(dyd, wd, torch.empty_like(acd), N, H, W, C, add=acd)
        dw = ops.fpn_deconv_wgrad(xd, dyd, torch.zeros((C, 4, 4, C), device="cuda"), ws, N, H, W, C)
        outs.append((y.clone(), dx.clone(), dw.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                           b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32))


def test_deconv_kernels_match_the_generic_convolution_kernels():
    """The same math through bd_conv2d_dgrad / bd_conv2d_fwd / bd_conv2d_wgrad on the conv view (4x4, stride 2, pad 1,
    Cin = fine, Cout = coarse): forward = the view's data gradient, data gradient = its forward, weight gradient = its weight gradient."""
    from basedet_amd import ops
    from util import pack_weights
    N, H, W, C = 2, 13, 21, 256
    x, w, add, dy, addc = _operands(N, H, W, C, seed=11)
    _, wf, wd = _packed(ops, w)
    gc, gf = ops.single(N, H, W), ops.single(N, 2 * H, 2 * W)
    d = ops.conv_desc(gf, gc, C, C, 4, 4, 2, 1)
    wfwd, wdg = pack_weights(ops, w)                 # w is the view's OIHW weight
    xd, dyd = nchw_to_pm(x), nchw_to_pm(dy)
    y_gen = ops.conv2d_dgrad(d, xd, wdg, torch.empty((N * 4 * H * W, C), dtype=torch.bfloat16, device="cuda"))
    y_ded = ops.fpn_deconv_fwd(xd, wf, torch.empty_like(y_gen), N, H, W, C)
    dx_gen = ops.conv2d_fwd(d, dyd, wfwd, None, torch.empty((N * H * W, C), dtype=torch.bfloat16, device="cuda"))
    dx_ded = ops.fpn_deconv_dgrad(dyd, wd, torch.empty_like(dx_gen), N, H, W, C)
    ws = torch.empty((max(ops.conv2d_wgrad_workspace_bytes(d), ops.fpn_deconv_wgrad_workspace_bytes(N, H, W, C)) // 4 + 64,),
                     dtype=torch.float32, device="cuda")
    dw_gen = ops.conv2d_wgrad(d, dyd, xd, torch.zeros((C, 4, 4, C), device="cuda"), ws).clone()
    dw_ded = ops.fpn_deconv_wgrad(xd, dyd, torch.zeros((C, 4, 4, C), device="cuda"), ws, N, H, W, C)
    assert rel_l2(y_ded.float().cpu(), y_gen.float().cpu()) < 1e-2
    assert rel_l2(dx_ded.float().cpu(), dx_gen.float().cpu()) < 1e-2
    assert rel_l2(dw_ded.cpu(), dw_gen.cpu()) < 1e-4


def test_deconv_refuses_bad_shapes():
    from basedet_amd import ops
    from basedet_amd._lib import BasedetHipError
    t = torch.zeros((2 * 4 * 4 * 96,), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(BasedetHipError):
        ops.fpn_deconv_fwd(t, t, t, 2, 2, 2, 96)


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
def _oracle_cls():
    from oracle.model import Oracle

    class DeconvOracle(Oracle):
        """FPN.forward with upsample = "deconv" (fpn_backbone.py:131-138); LastLevelP6P7 as in the base oracle."""

        def fpn(self, feats):
            names = self.arch.get("fpn_in", ["res3", "res4", "res5"])
            stages = [int(n[-1]) for n in names]
            x = [feats[n] for n in names[::-1]]
            st = stages[::-1]
            q, act = self._q, self._act
            prev = act(f"lat{st[0]}", self._conv(x[0], f"backbone.fpn_lateral{st[0]}"), False)
            results = [act(f"P{st[0]}", self._conv(prev, f"backbone.fpn_output{st[0]}", 1, 1), False)]
            for f, sc, s in zip(x[1:], st[:-1], st[1:]):
                td = TF.conv_transpose2d(prev, q(self.p[f"backbone.fpn_upsample{sc}.weight"]), stride=2, padding=1)
                prev = act(f"lat{s}", q(self._conv(f, f"backbone.fpn_lateral{s}")) + td, False)
                results.insert(0, act(f"P{s}", self._conv(prev, f"backbone.fpn_output{s}", 1, 1), False))
            top = stages[-1]
            p6 = act(f"P{top + 1}", self._conv(feats["res5"], "backbone.top_block.p6", 2, 1), False)
            p7 = act(f"P{top + 2}", self._conv(TF.relu(p6), "backbone.top_block.p7", 2, 1), False)
            return results + [p6, p7]
    return DeconvOracle


def _retinanet_setup(N, size):
    from basedet_amd.configs import retinanet_r18_config
    from basedet_amd.models import params as P
    from basedet_amd.utils import DummyLoader
    cfg = retinanet_r18_config()
    cfg.MODEL.BATCHSIZE = N
    cfg.MODEL.FPN.UPSAMPLE = "deconv"
    params = P.init_retinanet_params(cfg, 0)
    rng = np.random.default_rng(1)
    for k in list(params):
        if (".bn" in k or "downsample.1" in k) and k.endswith(".weight") and ".bn2." in k:
            params[k] = rng.uniform(0.15, 0.35, params[k].shape).astype(np.float32)
    batch = next(DummyLoader(N, size, seed=0))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    return cfg, params, batch


def _fcos_setup(N, size):
    from basedet_amd.configs import FCOSConfig
    from basedet_amd.models import params as P
    from basedet_amd.utils import DummyLoader
    cfg = FCOSConfig()
    cfg.MODEL.BATCHSIZE = N
    cfg.MODEL.FPN.UPSAMPLE = "deconv"
    params = P.init_fcos_params(cfg, seed=0, residual_gamma=0.25)
    params["head.bbox_pred.bias"] = np.full_like(params["head.bbox_pred.bias"], 0.5)
    batch = next(DummyLoader(N, size, seed=0))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    return cfg, params, batch


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))


@pytest.mark.parametrize("family", ["retinanet", "fcos"])
def test_deconv_training_step_matches_oracle(family):
    from basedet_amd.models import FCOS, RetinaNet, params as P
    cfg, params, batch = _retinanet_setup(2, (128, 160)) if family == "retinanet" else _fcos_setup(2, (96, 128))
    model = (RetinaNet if family == "retinanet" else FCOS)(cfg, params=params)
    names = P.trainable_names(params, cfg.MODEL.BACKBONE.FREEZE_AT)
    ups = ["backbone.fpn_upsample4.weight", "backbone.fpn_upsample5.weight"]
    assert all(n in names for n in ups) and sorted(names) == sorted(model.state_dict_trainable_names())
    Orc = _oracle_cls()
    losses_fn = "retinanet_losses" if family == "retinanet" else "fcos_losses"
    orc = Orc(params, P.oracle_arch(cfg), trainable=names)
    ref, aux = getattr(orc, losses_fn)(batch)
    ref_grads = orc.grads(ref["total_loss"])
    out = model(batch)
    assert np.array_equal(model._cur.labels.cpu().numpy(), aux["labels"])
    for k in ("cls_loss", "reg_loss", "total_loss"):
        got, want = float(out[k]), float(ref[k].detach())
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)
    model.backward()
    torch.cuda.synchronize()
    got = model.reference_grads()
    if family == "retinanet":        # (tests/test_model_gpu.py's bounds: the plain-oracle cosine is asserted for RetinaNet only)
        a = torch.cat([got[n].double().reshape(-1) for n in names])
        b = torch.cat([ref_grads[n].detach().double().reshape(-1) for n in names])
        assert _cos(a, b) > 0.99
    orc2 = Orc(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=model.debug_activations())
    l2, _ = getattr(orc2, losses_fn)(batch)
    g2 = orc2.grads(l2["total_loss"])
    bound = 1e-2 if family == "retinanet" else 2e-2
    for n in names:
        assert rel_l2(got[n], g2[n].detach()) < bound, (n, rel_l2(got[n], g2[n].detach()))
    for n in ups:
        assert _cos(got[n], g2[n].detach()) > 0.999, n
    # the same step again: bit-identical gradients
    first = {n: got[n].clone() for n in names}
    model(batch)
    model.backward()
    torch.cuda.synchronize()
    again = model.reference_grads()
    for n in names:
        assert torch.equal(first[n].view(torch.int32), again[n].view(torch.int32)), n
    # the checkpoint round trip keeps the reference's names and shapes
    sd = model.state_dict()
    for n in ups:
        assert sd[n].shape == params[n].shape and np.array_equal(sd[n], params[n])


def test_deconv_inference_runs():
    from basedet_amd.models import RetinaNet
    cfg, params, batch = _retinanet_setup(1, (128, 160))
    model = RetinaNet(cfg, params=params).eval()
    out = model({"data": batch["data"], "im_info": batch["im_info"]})
    assert set(out.keys()) == {"boxes", "box_scores", "box_labels"}
    assert torch.isfinite(model._plan(1, 128, 160).logits.float()).all()


def test_deconv_fp8_step_runs():
    """The deconv layers stay bf16 in the fp8 workload (they are not 3x3): one R101 step at a small size."""
    from basedet_amd.configs import RetinaNetConfig
    from basedet_amd.models import RetinaNet, params as P
    from basedet_amd.solver import DetSolver
    from basedet_amd.utils import DummyLoader
    cfg = RetinaNetConfig()
    cfg.MODEL.BACKBONE.NAME = "resnet101"
    cfg.MODEL.BATCHSIZE = 2
    cfg.MODEL.WEIGHT_DTYPE = "fp8_e4m3"
    cfg.MODEL.FPN.UPSAMPLE = "deconv"
    params = P.init_retinanet_params(cfg, 0, residual_gamma=0.25)
    batch = next(DummyLoader(2, (128, 160), seed=0))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    model = RetinaNet(cfg, params=params)
    assert not any(model.upsample[s].fp8 for s in model.upsample) and len(model.upsample) == 2
    solver = DetSolver.build(cfg, model)
    out = solver.minimize(model, batch)
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in out.values())
    assert torch.isfinite(model.upsample[5].gw).all() and float(model.upsample[5].gw.abs().sum()) > 0


def test_playground_config_with_deconv_builds_through_the_alias(tmp_path):
    import importlib.util
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import basedet  # noqa: F401
    path = tmp_path / "config.py"
    path.write_text("from basedet.configs import RetinaNetConfig\n\n\nclass Cfg(RetinaNetConfig):\n    def __init__(self, **kwargs):\n"
                    "        super().__init__(**kwargs)\n        self.MODEL.FPN.UPSAMPLE = \"deconv\"\n")
    spec = importlib.util.spec_from_file_location("playground_deconv_cfg", str(path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = mod.Cfg()
    from basedet.utils import registers
    import basedet.models  # noqa: F401
    model = registers.models.get(cfg.MODEL.NAME)(cfg)
    sd = model.state_dict()
    for s in (4, 5):
        assert sd[f"backbone.fpn_upsample{s}.weight"].shape == (256, 256, 4, 4)
    assert "backbone.fpn_upsample3.weight" not in sd
