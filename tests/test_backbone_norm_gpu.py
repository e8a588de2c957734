"""MODEL.BACKBONE.NORM = "BN" / "SyncBN" (FREEZE_AT = 0) on the GPU, at 2 x 128 x 160 on the fixtures of tests/test_model_gpu.py, against the
oracle subclass of tests/backbone_norm_oracle.py.

Per layer (every trainable parameter, gamma / beta of every backbone norm and conv1.weight included): the gradient against the sim_bf16
oracle on the stored activations, rel-L2 1e-2 (tests/test_fpn_norm_gpu.py's bound; a per-layer comparison, depth does not enter).

End to end against the fp32 oracle the project's bounds are 2e-2 (losses, activations) and 0.99 (whole-model gradient cosine); through ~20
(R18) / ~50 (R50) normalised layers they are kept where the distance of the sim_bf16 oracle from the fp32 oracle, measured on the CPU (the
code under test takes no part), leaves them a factor 2, and are twice that distance otherwise:

                     sim_bf16 oracle vs fp32 oracle (CPU)      bound                            GPU vs fp32 oracle (MI355X)
    R18  losses      cls 8.4e-5, reg 1.8e-5, total 2.4e-5      2e-2                             1.3e-4, 1.8e-6, 5.3e-5
         res3/4/5    1.14e-2 / 1.51e-2 / 1.93e-2               2.28e-2 / 3.02e-2 / 3.86e-2      1.13e-2 / 1.49e-2 / 1.90e-2
         cosine      0.99788 (1 - cos = 2.1e-3)                0.99                             0.99791
    R50  losses      cls 3.7e-4, reg 1.5e-4, total 6.3e-5      2e-2                             3.7e-4, 7.5e-5, 1.1e-4
         res3/4/5    1.81e-2 / 3.33e-2 / 5.21e-2               3.62e-2 / 6.66e-2 / 1.04e-1      1.82e-2 / 3.31e-2 / 5.18e-2
         cosine      0.97515 (1 - cos = 2.49e-2)               0.9503                           0.97336

Per parameter (bound 1e-2) the GPU's worst is 5.5e-3 (R18), 4.5e-3 (R50), 4.4e-3 (Faster R-CNN).  Also on file in DESIGN.md (4s)."""
import functools

import numpy as np
import pytest
import torch

from backbone_norm_oracle import backbone_norm_oracle_cls, randomise_backbone_norms
from fpn_norm_oracle import norm_oracle_cls, randomise_norms
from test_model_gpu import _frcnn_setup, _setup, check_faster_rcnn_step
from util import bits_of

pytestmark = pytest.mark.gpu

SIZE = (128, 160)
BU = "backbone.bottom_up"
E2E = {"resnet18": dict(res=(2.28e-2, 3.02e-2, 3.86e-2), cos=0.99), "resnet50": dict(res=(3.62e-2, 6.66e-2, 1.04e-1), cos=0.9503)}
NAMED = {"resnet18": (".bn1", ".layer2.1.bn2", ".layer3.0.bn2", ".layer2.0.downsample.1"),           # (R18's last norm of a branch is bn2)
         "resnet50": (".bn1", ".layer2.1.bn2", ".layer3.0.bn3", ".layer1.0.downsample.1")}


def _over(norm="BN", **fpn):
    return dict(MODEL=dict(BACKBONE=dict(FREEZE_AT=0, NORM=norm), **(dict(FPN=fpn) if fpn else {})))


def _retina(backbone="resnet18", norm="BN", seed=0):
    cfg, params, batch = _setup(backbone, 2, SIZE, seed=seed, overrides=_over(norm))
    return cfg, randomise_backbone_norms(params), batch


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))


def _res_keys(model):
    pl = model._cur
    return [model.blocks[pl.res[s]]["prefix"] + ".out" for s in (3, 4, 5)]


@pytest.mark.parametrize("backbone", ["resnet18", "resnet50"])
def test_retinanet_step_matches_oracle(backbone):
    from basedet_amd.models import RetinaNet, params as P
    cfg, params, batch = _retina(backbone)
    model = RetinaNet(cfg, params=params)
    names = P.trainable_names(params, 0, "BN")
    assert sorted(names) == sorted(model.state_dict_trainable_names())
    assert BU + ".bn1.weight" in names and BU + ".layer1.0.bn1.bias" in names and BU + ".bn1.running_mean" not in names
    out = model(batch)
    pl = model._cur
    Orc = backbone_norm_oracle_cls()
    acts = model.debug_activations()
    keys = _res_keys(model)
    rec = {"_compare": {k: acts[k] for k in keys}}
    orc = Orc(params, P.oracle_arch(cfg), trainable=names, record=rec)
    ref, aux = orc.retinanet_losses(batch)
    ref_grads = orc.grads(ref["total_loss"])
    assert np.array_equal(pl.labels.cpu().numpy(), aux["labels"])
    for k in ("cls_loss", "reg_loss", "total_loss"):
        got, want = float(out[k]), float(ref[k].detach())
        print(backbone, k, "rel", abs(got - want) / abs(want))
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)
    for k, bound in zip(keys, E2E[backbone]["res"]):
        print(backbone, k, "rel-L2", rec[k], "bound", bound)
        assert rec[k] < bound, (k, rec[k])
    model.backward()
    torch.cuda.synchronize()
    got = model.reference_grads()
    cos = _cos(torch.cat([got[n].double().reshape(-1) for n in names]), torch.cat([ref_grads[n].detach().double().reshape(-1) for n in names]))
    print(backbone, "whole-model gradient cosine", cos)
    assert cos > E2E[backbone]["cos"]
    # per layer: the sim_bf16 oracle on the stored activations (and the stored dL/dz of every backbone norm: tests/backbone_norm_oracle.py)
    orc2 = Orc(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=model.debug_activations())
    l2, _ = orc2.retinanet_losses(batch)
    g2 = orc2.grads(l2["total_loss"])
    print(backbone, "oracle's own dL/dz against the stored one, worst rel-L2", max(orc2.grad_check.items(), key=lambda t: t[1]))
    assert "g_stem_out" in orc2.grad_check and len(orc2.grad_check) == 1 + sum(len(b["convs"]) for b in model.blocks)
    assert all(v < 1e-2 for v in orc2.grad_check.values()), {k: v for k, v in orc2.grad_check.items() if not v < 1e-2}
    rels = {n: float((got[n].double().reshape(-1) - g2[n].detach().double().reshape(-1)).norm() / (g2[n].detach().double().norm() + 1e-30))
            for n in names}
    bad = {n: r for n, r in rels.items() if not r < 1e-2}
    print(backbone, "worst per-parameter rel-L2", max(rels.items(), key=lambda t: t[1]), "over 1e-2:", bad)
    assert not bad, bad
    for pre in NAMED[backbone]:
        for suffix in (".weight", ".bias"):
            n = BU + pre + suffix
            assert float(got[n].abs().sum()) > 0 and _cos(got[n], g2[n].detach()) > 0.999, n


def test_retinanet_deconv_fpn_step_matches_oracle():
    """MODEL.FPN.UPSAMPLE = "deconv" with BOTH norms live (tests/test_fpn_norm_gpu.py runs deconv under the FPN norm alone): the learned
    top-down path hands dL/d lat_s from the deconv's data gradient to the lateral norm's backward pass, and below it to the backbone
    norms.  Labels, losses (2e-2, fp32 oracle), then every trainable parameter -- the deconv weights and the lateral norms' gamma / beta
    among them -- against the sim_bf16 oracle on the stored activations, rel-L2 1e-2."""
    from basedet_amd.models import RetinaNet, params as P
    cfg, params, batch = _setup("resnet18", 2, SIZE, overrides=_over("BN", NORM="BN", UPSAMPLE="deconv"))
    params = randomise_backbone_norms(randomise_norms(params))
    model = RetinaNet(cfg, params=params)
    names = P.trainable_names(params, 0, "BN")
    assert sorted(names) == sorted(model.state_dict_trainable_names())
    ups = ["backbone.fpn_upsample4.weight", "backbone.fpn_upsample5.weight"]
    lats = [f"backbone.fpn_lateral{s}.norm.{k}" for s in (3, 4, 5) for k in ("weight", "bias")]
    assert all(n in names for n in ups + lats + [BU + ".bn1.weight"])
    Orc = backbone_norm_oracle_cls(norm_oracle_cls())
    ref, aux = Orc(params, P.oracle_arch(cfg), trainable=names).retinanet_losses(batch)
    out = model(batch)
    pl = model._cur
    assert np.array_equal(pl.labels.cpu().numpy(), aux["labels"])
    for k in ("cls_loss", "reg_loss", "total_loss"):
        got, want = float(out[k]), float(ref[k].detach())
        print("deconv + both norms", k, "rel", abs(got - want) / abs(want))
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)
    model.backward()
    torch.cuda.synchronize()
    got = model.reference_grads()
    acts = model.debug_activations()
    for s in model.fpn_stages:
        g = pl.blk[pl.res[s]].gout
        acts[f"g_lat{s}"] = pl.g_lat[s].float().cpu().view(pl.N, g.H[0], g.W[0], -1).permute(0, 3, 1, 2).contiguous()
    orc2 = Orc(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=acts)
    l2, _ = orc2.retinanet_losses(batch)
    g2 = orc2.grads(l2["total_loss"])
    assert len(orc2.grad_check) == 1 + sum(len(b["convs"]) for b in model.blocks) + len(model.fpn_stages)
    assert all(v < 1e-2 for v in orc2.grad_check.values()), {k: v for k, v in orc2.grad_check.items() if not v < 1e-2}
    rels = {n: float((got[n].double().reshape(-1) - g2[n].detach().double().reshape(-1)).norm() / (g2[n].detach().double().norm() + 1e-30))
            for n in names}
    bad = {n: r for n, r in rels.items() if not r < 1e-2}
    print("deconv + both norms: worst per-parameter rel-L2", max(rels.items(), key=lambda t: t[1]), "over 1e-2:", bad)
    assert not bad, bad
    for n in ups + lats:
        assert float(got[n].abs().sum()) > 0 and _cos(got[n], g2[n].detach()) > 0.999, n


class _Capture:
    """Keeps the last gradients both sides of check_faster_rcnn_step computed, for the tighter comparison below."""
    oracle = model = None


def test_faster_rcnn_step_matches_oracle(monkeypatch):
    """Faster R-CNN (p2-p5: res2 is tapped) with MODEL.FPN.NORM = "BN" as well, through tests/test_model_gpu.py's own step check (labels,
    proposals, samples, losses) with the oracle class swapped; then every parameter's gradient at 1e-2."""
    from basedet_amd.models import FasterRCNN, params as P
    Orc = backbone_norm_oracle_cls(norm_oracle_cls())

    class Cap(Orc):
        def grads(self, loss):
            _Capture.oracle = super().grads(loss)
            return _Capture.oracle
    real = FasterRCNN.reference_grads

    def grads(self):
        _Capture.model = real(self)
        return _Capture.model
    real_acts = FasterRCNN.debug_activations

    def acts_with_g_lat(self):
        """+ the stored dL/d lat_s the FPN-norm oracle takes (tests/fpn_norm_oracle.py: a lateral norm's dbeta is a border residue)."""
        out, pl = real_acts(self), self._cur
        for s in self.fpn_stages:
            g = pl.blk[pl.res[s]].gout
            out[f"g_lat{s}"] = pl.g_lat[s].float().cpu().view(pl.N, g.H[0], g.W[0], -1).permute(0, 3, 1, 2).contiguous()
        return out
    monkeypatch.setattr(FasterRCNN, "debug_activations", acts_with_g_lat)
    monkeypatch.setattr("oracle.model.Oracle", Cap)
    monkeypatch.setattr(FasterRCNN, "reference_grads", grads)
    monkeypatch.setattr(P, "trainable_names", functools.partial(P.trainable_names, backbone_norm="BN"))
    cfg, params, batch = _frcnn_setup(2, SIZE, overrides=_over("BN", NORM="BN"))
    params = randomise_backbone_norms(randomise_norms(params))
    assert BU + ".bn1.weight" in P.trainable_names(params, 0)
    check_faster_rcnn_step(cfg, params, batch)
    rels = {n: float((_Capture.model[n].double().reshape(-1) - r.detach().double().reshape(-1)).norm() / (r.detach().double().norm() + 1e-30))
            for n, r in _Capture.oracle.items()}
    bad = {n: r for n, r in rels.items() if not r < 1e-2}
    print("faster r-cnn worst per-parameter rel-L2", max(rels.items(), key=lambda t: t[1]), "over 1e-2:", bad)
    assert not bad, bad
    n = BU + ".layer1.0.bn1.weight"
    assert float(_Capture.model[n].abs().sum()) > 0 and _cos(_Capture.model[n], _Capture.oracle[n].detach()) > 0.999


def _norm_tensors(model, pl):
    """name -> stored pre-norm tensor (M, C) of the stem, one norm per layer and one downsample.1."""
    names = [BU + ".bn1"] + [blk["prefix"] + ".bn1" for blk in model.blocks if blk["prefix"].endswith(".0")]
    names.append(next(blk["prefix"] for blk in model.blocks if blk["ds"] is not None) + ".downsample.1")
    return {k: pl.norm_y[k] for k in names}


def test_norm_state_is_live_after_two_steps():
    """gamma, beta and the running statistics move; the running statistics follow the float64 recurrence over the float64 statistics of
    the stored bf16 pre-norm tensors, to tests/test_batchnorm_gpu.py's bounds (1e-5 (|mu| + sigma), 1e-4 relative)."""
    from basedet_amd.models import RetinaNet
    from basedet_amd.solver import DetSolver
    cfg, params, batch = _retina()
    model = RetinaNet(cfg, params=params)
    solver = DetSolver.build(cfg, model)
    run, scale = {}, {}
    for _ in range(2):
        solver.minimize(model, batch)
        torch.cuda.synchronize()
        for k, t in _norm_tensors(model, model._cur).items():
            y = t.double().cpu().numpy()
            M = y.shape[0]
            mu, var = y.mean(0), y.var(0)
            rm, rv = run.get(k, (params[k + ".running_mean"].astype(np.float64), params[k + ".running_var"].astype(np.float64)))
            run[k] = (0.9 * rm + 0.1 * mu, 0.9 * rv + 0.1 * var * M / (M - 1))
            scale[k] = np.abs(mu) + np.sqrt(var)
    sd = model.state_dict()
    assert len(run) == 6
    for k, (rm, rv) in run.items():
        assert np.all(np.abs(sd[k + ".running_mean"] - rm) <= 1e-5 * scale[k]), k
        assert np.all(np.abs(sd[k + ".running_var"] - rv) <= 1e-4 * rv), k
        for suffix in (".weight", ".bias", ".running_mean", ".running_var"):
            assert not np.array_equal(sd[k + suffix], params[k + suffix]), k + suffix


def _eval_logits(model, batch):
    model.eval()
    outs = model.inference_batch({"data": batch["data"], "im_info": batch["im_info"]})
    torch.cuda.synchronize()
    return model._plan(batch["data"].shape[0], *SIZE).logits.clone(), outs


def test_eval_is_the_frozen_model_and_train_comes_back():
    from basedet_amd.models import RetinaNet
    cfg, params, batch = _retina()
    model = RetinaNet(cfg, params=params)
    first = model(batch)
    logits, outs = _eval_logits(model, batch)
    cfg_f, _, _ = _setup("resnet18", 2, SIZE, overrides=dict(MODEL=dict(BACKBONE=dict(FREEZE_AT=0))))
    frozen = RetinaNet(cfg_f, params=model.state_dict())
    want, _ = _eval_logits(frozen, batch)
    assert torch.equal(bits_of(logits), bits_of(want))
    model.train()
    c = model.blocks[0]["convs"][0]
    assert c.row_scale is None and c.b is None and model.stem_scale is None
    again = model(batch)
    assert np.isfinite(float(again["total_loss"])) and float(again["total_loss"]) == float(first["total_loss"])      # (batch statistics: the moved running statistics do not enter)


def _two_steps_then(cfg, params, batch, reload):
    """One step, then `reload(model)` -> the model the second step runs on; returns the second step's losses."""
    from basedet_amd.models import RetinaNet
    from basedet_amd.solver import DetSolver
    model = RetinaNet(cfg, params=params)
    DetSolver.build(cfg, model).minimize(model, batch)
    model = reload(model)
    out = model(batch)
    torch.cuda.synchronize()
    return {k: float(v) for k, v in out.items()}


def test_state_dict_and_checkpoint_round_trips(tmp_path):
    from basedet_amd.models import RetinaNet
    from basedet_amd.utils.checkpoint import save_checkpoint
    cfg, params, batch = _retina()
    want = _two_steps_then(cfg, params, batch, lambda m: m)

    def through_state_dict(m):
        fresh = RetinaNet(cfg, seed=5)
        fresh.load_state_dict(m.state_dict())
        return fresh

    def through_checkpoint(m):
        path = str(tmp_path / "ckpt.pkl")
        save_checkpoint(path, m.state_dict())
        fresh = RetinaNet(cfg, seed=6)
        fresh.load_weights(path)
        return fresh
    assert _two_steps_then(cfg, params, batch, through_state_dict) == want
    assert _two_steps_then(cfg, params, batch, through_checkpoint) == want


def test_syncbn_at_world_one_is_bn_and_runs_repeat():
    from basedet_amd.models import RetinaNet
    res = []
    for norm in ("BN", "SyncBN", "BN"):
        cfg, params, batch = _retina(norm=norm)
        model = RetinaNet(cfg, params=params)
        out = model(batch)
        model.backward()
        torch.cuda.synchronize()
        res.append(({k: float(v) for k, v in out.items()}, model.arena.g.clone(), model.norms.running.clone()))
    for other in res[1:]:
        assert other[0] == res[0][0]
        assert torch.equal(bits_of(other[1]), bits_of(res[0][1])) and torch.equal(bits_of(other[2]), bits_of(res[0][2]))


def test_short_run_from_init():
    """30 SGD steps on the repeated batch from init_params (gamma 1, beta 0): the loss stays finite and ends below its first value;
    eval() then detects with finite boxes."""
    from basedet_amd.models import RetinaNet
    from basedet_amd.solver import DetSolver
    cfg, _, batch = _setup("resnet18", 2, SIZE, seed=3, overrides=_over())
    cfg.SOLVER.BASIC_LR = 0.005
    model = RetinaNet(cfg, seed=3)
    solver = DetSolver.build(cfg, model)
    losses = [float(solver.minimize(model, batch)["total_loss"]) for _ in range(30)]
    print("first", losses[0], "last", losses[-1])
    assert all(np.isfinite(v) for v in losses) and losses[-1] < losses[0]
    _, outs = _eval_logits(model, batch)
    assert len(outs) == 2
    for o in outs:
        assert bool(torch.isfinite(torch.as_tensor(o.boxes).float()).all())
