"""Host side of TRAINER.EMA (basedet_amd/layers/ema.py against basedet/layers/common/ema.py:10-93 and engine/trainer.py:63-72): the momentum
formula, the burn-in schedule, the counter, the trainer's wiring and the `--ema` switch.  No kernel runs here: `update` is overridden
to record the momentum it was called with."""
import types

import numpy as np
import pytest
import torch


def _arena_model():
    """A CPU ParamArena holding two reserved tensors, as tests/test_dist_cpu.py builds one."""
    from basedet_amd.models.engine import ParamArena

    class M:
        repacked = 0

        def repack_trainable(self):
            self.repacked += 1

    m = M()
    m.arena = ParamArena(torch.device("cpu"))
    m.arena.reserve("head.cls_score.weight", (5, 3, 3, 4))
    m.arena.reserve("head.cls_score.bias", (5,))
    m.arena.allocate()
    m.arena.w.copy_(torch.arange(m.arena.total, dtype=torch.float32))
    return m


def _recording_ema(model, **kw):
    from basedet_amd.layers import ModelEMA

    class Rec(ModelEMA):
        def __init__(self, *a, **k):
            self.calls, self.loaded = [], []
            super().__init__(*a, **k)

        def update(self, m):
            self.calls.append(m)

        def _load_model(self, values):
            self.loaded.append(values)

    return Rec(model, **kw)


def test_calculate_momentum():
    from basedet_amd.layers import calculate_momentum
    assert abs(calculate_momentum(5e-4, 90000, 1) - 0.9995) < 1e-12
    assert abs(calculate_momentum(5e-4, 90000, 10) - 0.995) < 1e-12
    assert calculate_momentum(1.0, 10, 1) == 0                       # 1 - 9000 clamps at 0


def test_exported_under_the_reference_module_path():
    import basedet.layers
    import basedet_amd.layers
    assert basedet.layers.ModelEMA is basedet_amd.layers.ModelEMA
    assert basedet.layers.calculate_momentum is basedet_amd.layers.calculate_momentum


def test_state_is_a_copy_of_the_arena():
    model = _arena_model()
    ema = _recording_ema(model, momentum=0.5)
    assert ema.e.shape == model.arena.w.shape and ema.e.dtype == torch.float32 and ema.e.device == model.arena.w.device
    assert torch.equal(ema.e, model.arena.w) and ema.e.data_ptr() != model.arena.w.data_ptr()
    assert (ema.momentum, ema.iters, ema.burnin_iter) == (0.5, 0, 2000)


def test_step_schedule():
    """ema.py:57-69 with burnin_iter = 3: iterations 1 and 2 do nothing, iteration 3 copies (m = 0) and averages, 4 .. 7 average."""
    ema = _recording_ema(_arena_model(), momentum=0.5, burnin_iter=3)
    for _ in range(7):
        ema.step()
    assert ema.calls == [0, 0.5, 0.5, 0.5, 0.5, 0.5]
    assert ema.iters == 7


def test_fused_steps_only_count():
    """SGD.step(ema=...) asks `fused_momentum()` before its launch: None up to and including the burn-in iteration (step() runs its own
    updates), the momentum after it -- and the step() that follows a fused launch only advances the counter."""
    ema = _recording_ema(_arena_model(), momentum=0.5, burnin_iter=3)
    asked = []
    for _ in range(6):
        asked.append(ema.fused_momentum())
        ema.step()
    assert asked == [None, None, None, 0.5, 0.5, 0.5]
    assert ema.calls == [0, 0.5] and ema.iters == 6
    ema.step()                                                       # a step nobody fused runs its own update again
    assert ema.calls == [0, 0.5, 0.5] and ema.iters == 7


def test_start_iter_and_load_state_dict():
    ema = _recording_ema(_arena_model(), momentum=0.5, start_iter=4, burnin_iter=3)
    assert ema.iters == 4
    ema.step()
    assert ema.iters == 5 and ema.calls == [0.5]
    ema.load_state_dict({"iter": 5, "model": {"k": 1}})
    assert ema.iters == 5 and ema.loaded == [{"k": 1}]
    ema.iters = 9
    ema.load_state_dict({"model": {}})                               # ema.py:84-86: no "iter" -> the counter stays
    assert ema.iters == 9
    ema.load_state_dict({"iter": 2, "model": {}})
    assert ema.iters == 2


def _trainer(**ema_cfg):
    from basedet_amd.configs import RetinaNetConfig
    from basedet_amd.engine import DetTrainer
    cfg = RetinaNetConfig()
    cfg.MODEL.BATCHSIZE = 16
    cfg.TRAINER.EMA.merge(ema_cfg)
    model = _arena_model()
    solver = types.SimpleNamespace(optimizer=types.SimpleNamespace(param_groups=[dict(lr=0.01)]), grad_scaler=None, grad_clip_fn=None)
    return cfg, DetTrainer(cfg, model, [], solver)


def test_trainer_momentum_from_config():
    from basedet_amd.layers import ModelEMA, calculate_momentum
    cfg, tr = _trainer(ENABLE=True, MOMENTUM=None, ALPHA=1e-3, UPDATE_PERIOD=4, BURNIN_ITER=7)
    max_iter = int(cfg.SOLVER.NUM_IMAGE_PER_EPOCH / 1 / 16)
    assert tr.enable_ema is True and isinstance(tr.ema, ModelEMA)
    assert tr.ema.momentum == calculate_momentum(1e-3, cfg.SOLVER.MAX_EPOCH * max_iter, 4)
    assert 0 < tr.ema.momentum < 1 and tr.ema.burnin_iter == 7 and tr.ema.iters == 0
    _, tr = _trainer(ENABLE=True, MOMENTUM=0.9)
    assert tr.ema.momentum == 0.9 and tr.ema.burnin_iter == 2000
    _, tr = _trainer(ENABLE=False)
    assert tr.enable_ema is False and not hasattr(tr, "ema")
    _, tr = _trainer()                                               # the default config: off
    assert tr.enable_ema is False


def test_trainer_hands_the_average_to_the_solver_and_steps_it():
    """trainer.py:98-100: minimize, then ema.step(); the solver receives the average so that SGD.step can fold the update in.  With
    EMA off the solver is called exactly as before (no `ema` argument)."""
    seen = []
    _, tr = _trainer(ENABLE=True, MOMENTUM=0.5, BURNIN_ITER=0)
    tr.solver.minimize = lambda model, inputs, **kw: seen.append(kw) or {"total_loss": 1.0}
    tr.ema.update = lambda m: seen.append(("update", m))
    assert tr.model_step({"x": 1}) == {"total_loss": 1.0}
    assert seen == [{"ema": tr.ema}, ("update", 0.5)] and tr.ema.iters == 1
    seen.clear()
    _, tr = _trainer(ENABLE=False)
    tr.solver.minimize = lambda model, inputs, **kw: seen.append(kw) or {}
    tr.model_step({"x": 1})
    assert seen == [{}]


def test_det_train_parser_sets_the_config_key():
    from basedet.tools.det_train import default_parser
    from basedet_amd.configs import RetinaNetConfig
    from basedet_amd.tools.det_train import apply_flags
    args = default_parser().parse_args(["-f", "cfg.py", "--ema"])
    assert args.ema is True
    cfg = apply_flags(RetinaNetConfig(), args)
    assert cfg.TRAINER.EMA.ENABLE is True and cfg.DATA.BUILDER_NAME != "DummyLoader"
    args = default_parser().parse_args(["-f", "cfg.py", "--synthetic"])
    assert args.ema is False
    cfg = apply_flags(RetinaNetConfig(), args)
    assert cfg.TRAINER.EMA.ENABLE is False and cfg.DATA.BUILDER_NAME == "DummyLoader"


def test_ema_coefficients_are_formed_in_double():
    """ema.py:80 casts `1 - m` after the subtraction in Python float64; float32(1) - float32(m) would differ for m = 0.9995."""
    from basedet_amd import ops
    m, om = ops.ema_coeffs(0.9995)
    assert np.float32(om) == np.float32(1 - 0.9995)
    assert np.float32(om) != np.float32(1) - np.float32(0.9995)
    assert ops.ema_coeffs(0) == (0.0, 1.0)
