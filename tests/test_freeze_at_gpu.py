"""MODEL.BACKBONE.FREEZE_AT = 0 end to end: the stem and layer1 train.  The fixtures and assertions are those of tests/test_model_gpu.py,
imported: their helpers compare every name of P.trainable_names(params, FREEZE_AT) against the oracle, so backbone.bottom_up.conv1.weight
(through bd_maxpool3x3s2_bwd and bd_stem_conv7x7_wgrad) and all of layer1 (through the data gradient that reaches the pool output) are
covered with nothing restated.  resnet18: BasicBlock, layer1.0's identity shortcut; resnet50: Bottleneck, layer1.0's downsample.0 path.

Two-step loss bound: tests/test_optim_gpu.py compares arena bits with a numpy restatement, never a loss with the oracle, so the bound here
is the one tests/test_model_gpu.py holds a HIP loss to against the fp32 oracle (2e-2 relative, bf16 activations): the second step's loss
is such a loss, on weights that both sides moved by their own first step."""
import numpy as np
import pytest
import torch

from tests import test_model_gpu as T

pytestmark = pytest.mark.gpu

FREEZE0 = dict(MODEL=dict(BACKBONE=dict(FREEZE_AT=0)))
R18 = dict(MODEL=dict(BACKBONE=dict(NAME="resnet18", OUT_FEATURE_CHANNELS=[128, 256, 512], FREEZE_AT=0), FPN=dict(TOP_BLOCK_IN_CHANNELS=512)))
STEM = "backbone.bottom_up.conv1.weight"


@pytest.mark.parametrize("backbone", ["resnet18", "resnet50"])
def test_retinanet_step_matches_oracle(backbone):
    T.check_retinanet_step(*T._setup(backbone, 2, (128, 160), overrides=FREEZE0))


def test_fcos_step_matches_oracle():
    T.check_fcos_step(*T.fcos_setup(overrides=R18))


def test_faster_rcnn_step_matches_oracle():
    T.check_faster_rcnn_step(*T._frcnn_setup(2, (128, 160), overrides=FREEZE0))


def test_two_sgd_steps_move_and_repack_the_stem():
    from basedet_amd import ops
    from basedet_amd.models import RetinaNet, params as P
    from basedet_amd.solver import DetSolver
    from oracle.model import Oracle
    cfg, params, batch = T._setup("resnet18", 2, (128, 160), seed=3, overrides=FREEZE0)
    cfg.SOLVER.BASIC_LR = 0.005                                    # lr 0.01 at batch 2, as test_minimize_runs_and_loss_decreases
    model = RetinaNet(cfg, params=params)
    solver = DetSolver.build(cfg, model)
    grp = solver.optimizer.param_groups[0]
    names = P.trainable_names(params, 0)
    orc = Oracle(params, P.oracle_arch(cfg), trainable=names)
    w0 = model.stem_w.clone()
    state, ref, got = {}, [], []
    for _ in range(2):
        loss, _ = orc.retinanet_losses(batch)
        ref.append(float(loss["total_loss"].detach()))
        state = orc.sgd_step(orc.grads(loss["total_loss"]), state, grp["lr"], grp["momentum"], grp["weight_decay"])
        got.append(float(solver.minimize(model, batch)["total_loss"]))
    torch.cuda.synchronize()
    for g, r in zip(got, ref):
        assert np.isfinite(g) and abs(g - r) / abs(r) < 2e-2, (got, ref)
    assert not torch.equal(model.stem_w, w0)
    want = torch.empty_like(model.stem_packed)
    ops.stem_weight_pack(model.stem_w, model.stem_scale, want)
    assert torch.equal(model.stem_packed, want)
    assert np.array_equal(model.state_dict()[STEM], model.stem_w.permute(0, 3, 1, 2).cpu().numpy())


@pytest.mark.parametrize("freeze_at", [0, 1, 2])
def test_optimizer_state_carries_the_stem_only_when_it_trains(freeze_at):
    from basedet_amd.layers.ema import ModelEMA
    from basedet_amd.models import RetinaNet, params as P
    from basedet_amd.solver import DetSolver
    cfg, params, batch = T._setup("resnet18", 2, (64, 64), overrides=dict(MODEL=dict(BACKBONE=dict(FREEZE_AT=freeze_at))))
    model = RetinaNet(cfg, params=params)
    solver = DetSolver.build(cfg, model)
    solver.minimize(model, batch)
    sd = solver.optimizer.state_dict()["momentum_buffer"]
    assert sorted(sd) == sorted(P.trainable_names(params, freeze_at))
    assert (STEM in sd) == (freeze_at == 0)
    if freeze_at == 0:
        assert sd[STEM].shape == (64, 3, 7, 7) and np.abs(sd[STEM]).max() > 0
        # the momentum is the first step's gradient plus the decay term, in the reference's layout
        g = model.reference_grads()[STEM].numpy()
        assert np.allclose(sd[STEM], g + cfg.SOLVER.WEIGHT_DECAY * params[STEM], rtol=1e-5, atol=1e-7)
        # round trips: optimizer state, EMA and a state_dict reload keep the moved stem
        ema = ModelEMA(model, 0.5, burnin_iter=0)
        assert np.array_equal(ema.state_dict()["model"][STEM], model.state_dict()[STEM])
        model2 = RetinaNet(cfg, params=model.state_dict())
        solver2 = DetSolver.build(cfg, model2)
        solver2.optimizer.load_state_dict(solver.optimizer.state_dict())
        assert torch.equal(model2.arena.v, model.arena.v) and torch.equal(model2.stem_packed, model.stem_packed)
