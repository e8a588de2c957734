"""MODEL.FPN.NORM = "BN" / "SyncBN" on the GPU: the training step of a normalised-FPN RetinaNet (resize and deconv top-down) and
Faster R-CNN against the oracle subclass of tests/fpn_norm_oracle.py -- with the tolerances of
tests/test_model_gpu.py (Faster R-CNN: through its own step check, the oracle class swapped) -- then liveness of gamma / beta / running statistics, the evaluation fold, the checkpoint round trip
and SyncBN at world size 1."""
import numpy as np
import pytest
import torch

from fpn_norm_oracle import norm_oracle_cls, randomise_norms as _randomise_norms
from test_model_gpu import _frcnn_setup, _setup, check_faster_rcnn_step
from util import bits_of

pytestmark = pytest.mark.gpu

SIZE = (128, 160)


def _retina(norm="BN", upsample="resize", N=2, seed=0):
    over = dict(MODEL=dict(FPN=dict(NORM=norm, UPSAMPLE=upsample)))
    cfg, params, batch = _setup("resnet18", N, SIZE, seed=seed, overrides=over)
    return cfg, _randomise_norms(params), batch


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))


def _nchw(t, N, H, W):
    return t.float().cpu().view(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("upsample", ["resize", "deconv"])
def test_retinanet_bn_step_matches_oracle(upsample):
    """Labels, losses (2e-2), lat{s} / P{s} against the fp32 oracle (2e-2, the bound of the logits), whole-model gradient cosine (0.99)
    and the gradient of EVERY trainable parameter -- gamma, beta, lateral / output / backbone weights -- against the oracle on the
    stored activations (rel-L2 1e-2): the bounds of tests/test_model_gpu.py::check_retinanet_step and tests/test_fpn_deconv_gpu.py.
    The oracle on the stored activations also takes the stored dL/d lat_s (tests/fpn_norm_oracle.py): its own gradient there is held to
    the same 1e-2 first, then both sides sum the same bf16 terms below it."""
    from basedet_amd.models import RetinaNet, params as P
    cfg, params, batch = _retina("BN", upsample)
    assert "backbone.fpn_lateral3.norm.weight" in params and "backbone.fpn_lateral3.bias" not in params
    model = RetinaNet(cfg, params=params)
    names = P.trainable_names(params, cfg.MODEL.BACKBONE.FREEZE_AT)
    assert sorted(names) == sorted(model.state_dict_trainable_names())
    out = model(batch)
    pl = model._cur
    Orc = norm_oracle_cls()
    rec = {"_compare": model.debug_activations()}
    orc = Orc(params, P.oracle_arch(cfg), trainable=names, record=rec)
    ref, aux = orc.retinanet_losses(batch)
    ref_grads = orc.grads(ref["total_loss"])
    for s in model.fpn_stages:
        assert rec[f"lat{s}"] < 2e-2 and rec[f"P{s}"] < 2e-2, (s, rec[f"lat{s}"], rec[f"P{s}"])
    assert np.array_equal(pl.labels.cpu().numpy(), aux["labels"])
    for k in ("cls_loss", "reg_loss", "total_loss"):
        got, want = float(out[k]), float(ref[k].detach())
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)
    model.backward()
    torch.cuda.synchronize()
    got = model.reference_grads()
    a = torch.cat([got[n].double().reshape(-1) for n in names])
    b = torch.cat([ref_grads[n].detach().double().reshape(-1) for n in names])
    assert _cos(a, b) > 0.99
    acts = model.debug_activations()
    for s in model.fpn_stages:
        g = pl.blk[pl.res[s]].gout
        acts[f"g_lat{s}"] = _nchw(pl.g_lat[s], pl.N, g.H[0], g.W[0])
    orc2 = Orc(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=acts)
    l2, _ = orc2.retinanet_losses(batch)
    g2 = orc2.grads(l2["total_loss"])
    assert sorted(orc2.grad_check) == [f"g_lat{s}" for s in model.fpn_stages]
    for k, rel in orc2.grad_check.items():
        assert rel < 1e-2, (k, rel)
    for n in names:
        r, g = g2[n].detach().double().reshape(-1), got[n].double().reshape(-1)
        rel = float((g - r).norm() / (r.norm() + 1e-30))
        assert rel < 1e-2, (n, rel)
    for n in ("backbone.fpn_output3.norm.weight", "backbone.fpn_output3.norm.bias", "backbone.fpn_lateral4.norm.weight",
              "backbone.fpn_lateral3.norm.bias"):
        assert float(got[n].abs().sum()) > 0 and _cos(got[n], g2[n].detach()) > 0.999, n


def test_faster_rcnn_bn_step_matches_oracle(monkeypatch):
    monkeypatch.setattr("oracle.model.Oracle", norm_oracle_cls())
    cfg, params, batch = _frcnn_setup(2, SIZE, overrides=dict(MODEL=dict(FPN=dict(NORM="BN"))))
    assert "backbone.fpn_output2.norm.running_var" in params
    params = _randomise_norms(params)
    check_faster_rcnn_step(cfg, params, batch)
    # lat{s} / P{s} of the training forward against the fp32 oracle
    from basedet_amd.models import FasterRCNN, params as P
    model = FasterRCNN(cfg, params=params)
    pl = model._plan(2, *SIZE)
    rng = np.random.default_rng(5)
    G = batch["gt_boxes"].shape[1]
    keys = dict(rpn_pos=rng.random((2, pl.A_total), dtype=np.float32), rpn_neg=rng.random((2, pl.A_total), dtype=np.float32),
                rcnn_fg=rng.random((2, pl.rois.shape[1] + G), dtype=np.float32), rcnn_bg=rng.random((2, pl.rois.shape[1] + G), dtype=np.float32))
    model(dict(batch, sample_keys=keys))
    acts = model.debug_activations()
    rec = {"_compare": {k: v for k, v in acts.items() if k.startswith(("lat", "P"))}}
    norm_oracle_cls()(params, P.oracle_arch(cfg), record=rec).faster_rcnn_losses(batch, keys)
    for s in model.fpn_stages:
        assert rec[f"lat{s}"] < 2e-2 and rec[f"P{s}"] < 2e-2, (s, rec[f"lat{s}"], rec[f"P{s}"])


def test_norm_state_is_live_after_two_steps():
    """After two SGD steps gamma, beta and the running statistics have moved, and the running statistics follow the float64 recurrence over the float64
    statistics of the very bf16 tensors the kernels read, to tests/test_batchnorm_gpu.py's bounds."""
    from basedet_amd.models import RetinaNet, params as P
    from basedet_amd.solver import DetSolver
    cfg, params, batch = _retina()
    model = RetinaNet(cfg, params=params)
    solver = DetSolver.build(cfg, model)
    run = {n.name: (params[n.name + ".running_mean"].astype(np.float64), params[n.name + ".running_var"].astype(np.float64))
           for n in model.norms if n.name.startswith("backbone.fpn_")}
    scale = {k: (np.zeros_like(v[0]), np.zeros_like(v[0])) for k, v in run.items()}
    for _ in range(2):
        solver.minimize(model, batch)
        torch.cuda.synchronize()
        pl = model._cur
        for kind in ("lateral", "output"):
            for s in model.fpn_stages:
                k = f"backbone.fpn_{kind}{s}.norm"
                y = pl.norm_y[k].double().cpu().numpy()
                M = y.shape[0]
                mu, var = y.mean(0), y.var(0)
                rm, rv = run[k]
                run[k] = (0.9 * rm + 0.1 * mu, 0.9 * rv + 0.1 * var * M / (M - 1))
                scale[k] = (np.abs(mu) + np.sqrt(var), None)
    sd = model.state_dict()
    for k, (rm, rv) in run.items():
        assert np.all(np.abs(sd[k + ".running_mean"] - rm) <= 1e-5 * scale[k][0]), k
        assert np.all(np.abs(sd[k + ".running_var"] - rv) <= 1e-4 * rv), k
        for suffix in (".weight", ".bias", ".running_mean", ".running_var"):
            assert not np.array_equal(sd[k + suffix], params[k + suffix]), k + suffix


def _eval_logits(model, batch):
    model.eval()
    outs = model.inference_batch({"data": batch["data"], "im_info": batch["im_info"]})
    torch.cuda.synchronize()
    pl = model._plan(batch["data"].shape[0], *SIZE)
    return pl.logits.clone(), outs


def test_eval_folds_the_running_statistics_and_round_trips():
    from basedet_amd.models import RetinaNet, params as P
    from oracle import box_ops
    import torch as T
    cfg, params, batch = _retina()
    model = RetinaNet(cfg, params=params)
    logits, outs = _eval_logits(model, batch)
    assert len(outs) == 2
    orc = norm_oracle_cls()(params, P.oracle_arch(cfg))
    orc.training = False
    a = orc.arch
    image = T.from_numpy(np.asarray(box_ops.data_to_input(batch["data"], a["img_mean"], a["img_std"]), np.float32))
    with T.no_grad():
        ref = orc.retinanet_forward(image)[0]
    got = logits.float().cpu().view(ref.shape)
    assert float((got - ref).norm() / ref.norm()) < 2e-2                       # test_model_gpu's bound for the logits
    # the round trip: state_dict() -> a fresh model (another seed) -> load_state_dict() -> the same bits
    sd = model.state_dict()
    fresh = RetinaNet(cfg, seed=5)
    fresh.load_state_dict(sd)
    again, _ = _eval_logits(fresh, batch)
    assert torch.equal(bits_of(again), bits_of(logits))
    # the fold is live: another running_var, other outputs
    sd2 = dict(sd)
    sd2["backbone.fpn_output3.norm.running_var"] = sd["backbone.fpn_output3.norm.running_var"] * 4
    fresh.load_state_dict(sd2)
    moved, _ = _eval_logits(fresh, batch)
    assert not torch.equal(bits_of(moved), bits_of(logits))
    # and training mode comes back to the batch statistics: a step after eval() still runs and reads no folded scale
    fresh.train()
    assert fresh.lateral[3].row_scale is None and fresh.lateral[3].b is None
    out = fresh(batch)
    assert np.isfinite(float(out["total_loss"]))


def test_syncbn_at_world_one_is_bn_bit_for_bit():
    from basedet_amd.models import RetinaNet
    res = []
    for norm in ("BN", "SyncBN"):
        cfg, params, batch = _retina(norm)
        model = RetinaNet(cfg, params=params)
        out = model(batch)
        model.backward()
        torch.cuda.synchronize()
        res.append((float(out["total_loss"]), model.arena.g.clone(), model.norms.running.clone(), model._cur.P.clone()))
    assert res[0][0] == res[1][0]
    for a, b in zip(res[0][1:], res[1][1:]):
        assert torch.equal(bits_of(a), bits_of(b))


def test_default_config_is_untouched():
    """NORM = None: no norm entry, the biases are back, and the plan is that of a config without the key."""
    from basedet_amd.models import RetinaNet
    cfg, params, batch = _setup("resnet18", 2, SIZE)
    model = RetinaNet(cfg, params=params)
    names = model.trainable_parameter_names()
    assert not any(".norm." in n for n in names) and "backbone.fpn_lateral3.bias" in names and not model.norms
    cfg2, params2, _ = _setup("resnet18", 2, SIZE)
    cfg2.MODEL.FPN.pop("NORM")
    other = RetinaNet(cfg2, params=params2)
    assert other.trainable_parameter_names() == names
    assert model.plan_bytes(model.reserve(2, *SIZE)) == other.plan_bytes(other.reserve(2, *SIZE))
    normed = RetinaNet(*_retina()[:1], params=_retina()[1])
    extra = normed.plan_bytes(normed.reserve(2, *SIZE)) - model.plan_bytes(model.reserve(2, *SIZE))
    assert extra > 0          # the pre-norm tensors and their gradients: four bf16 tensors per stage, and the reduction workspace
