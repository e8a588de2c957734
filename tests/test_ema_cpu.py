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


# ---- live batch norms: the running statistics are buffers outside the arena, averaged in a tensor of their own ---------------------------
NORM = "backbone.fpn_lateral3.norm"


def _normed_model():
    """_arena_model() plus one live norm of 4 channels (LiveNorms on the CPU) and the three model methods ModelEMA's state calls use."""
    from basedet_amd.models.live_norm import LiveNorms
    m = _arena_model()
    m.norms = LiveNorms(torch.device("cpu"))
    n = m.norms.add(NORM, 4)
    m.norms.allocate()
    m.norms.running.copy_(torch.arange(8, dtype=torch.float32) + 100)
    m.training = True
    m.frozen = np.full(3, 7.0, np.float32)
    m.bound = []

    def state_dict():
        return {"head.cls_score.weight": m.arena.w.numpy().copy(), NORM + ".running_mean": n.running_mean.numpy().copy(),
                NORM + ".running_var": n.running_var.numpy().copy(), "backbone.bottom_up.bn1.running_var": m.frozen.copy()}

    def bind(params):
        m.bound.append(params)
        m.arena.w.copy_(torch.from_numpy(params["head.cls_score.weight"]))
        n.running_mean.copy_(torch.from_numpy(params[NORM + ".running_mean"]))
        n.running_var.copy_(torch.from_numpy(params[NORM + ".running_var"]))

    m.state_dict, m._bind_params = state_dict, bind
    m.state_dict_trainable_names = lambda: ["head.cls_score.weight"]
    m.repack_weights = lambda: None
    return m


@pytest.fixture
def host_ops(monkeypatch):
    """bd_ema_update / bd_swap_f32 restated on the host, and a log of the tensors they were launched on."""
    from basedet_amd import ops
    log = []

    def ema_update(e, w, m):
        log.append(("ema_update", e.data_ptr(), m))
        e.copy_(e * np.float32(m) + np.float32(1 - m) * w)

    def swap_f32(a, b):
        log.append(("swap_f32", a.data_ptr(), b.data_ptr()))
        t = a.clone()
        a.copy_(b)
        b.copy_(t)

    monkeypatch.setattr(ops, "ema_update", ema_update)
    monkeypatch.setattr(ops, "swap_f32", swap_f32)
    return log


def test_buffer_average_exists_only_with_live_norms():
    from basedet_amd.layers import ModelEMA
    from basedet_amd.models.live_norm import LiveNorms
    model = _normed_model()
    ema = ModelEMA(model, momentum=0.5)
    assert torch.equal(ema.r, model.norms.running) and ema.r.data_ptr() != model.norms.running.data_ptr() and ema.r.dtype == torch.float32
    plain = _arena_model()
    assert ModelEMA(plain, momentum=0.5).r is None                   # no `norms` at all
    plain.norms = LiveNorms(torch.device("cpu"))
    plain.norms.allocate()
    assert ModelEMA(plain, momentum=0.5).r is None                   # an FPNDetector without a live norm: an empty LiveNorms


def test_buffers_are_averaged_on_every_updating_step_fused_or_not(host_ops):
    """burnin_iter = 2 and four steps, the last two fused into the optimizer launch: the buffers' average takes update(0) + update(m) at
    step 2 and update(m) at steps 3 and 4 -- on launches of its own in the fused steps too, where the arena's average is left to the
    optimizer.  m = 0.5 and small integers: the recurrence is exact in fp32."""
    from basedet_amd.layers import ModelEMA
    model = _normed_model()
    ema = ModelEMA(model, momentum=0.5, burnin_iter=2)
    e_ptr, r_ptr = ema.e.data_ptr(), ema.r.data_ptr()
    ref = model.norms.running.double().clone()
    for it in range(1, 5):
        model.norms.running.add_(8.0 * it)                           # the training forward moves the buffers
        fused = ema.fused_momentum()
        assert (fused is not None) == (it > 2)
        del host_ops[:]
        ema.step()
        x = model.norms.running.double()
        if it == 2:
            ref = 0.5 * x + 0.5 * x
        elif it > 2:
            ref = 0.5 * ref + 0.5 * x
        want = {1: [], 2: [("ema_update", e_ptr, 0), ("ema_update", r_ptr, 0), ("ema_update", e_ptr, 0.5), ("ema_update", r_ptr, 0.5)]}
        assert host_ops == want.get(it, [("ema_update", r_ptr, 0.5)]), it
        assert torch.equal(ema.r.double(), ref), it
    assert ema.iters == 4 and not torch.equal(ema.r, model.norms.running)


def test_a_model_without_live_norms_launches_what_it_launched(host_ops):
    from basedet_amd.layers import ModelEMA
    model = _arena_model()
    ema = ModelEMA(model, momentum=0.5, burnin_iter=1)
    e_ptr, w_ptr = ema.e.data_ptr(), model.arena.w.data_ptr()
    ema.step()
    assert ema.fused_momentum() == 0.5
    ema.step()
    with ema.applied():
        pass
    assert host_ops == [("ema_update", e_ptr, 0), ("ema_update", e_ptr, 0.5)] + [("swap_f32", e_ptr, w_ptr)] * 2
    assert model.repacked == 2


def test_applied_and_state_dict_swap_the_buffers_too(host_ops):
    from basedet_amd.layers import ModelEMA
    model = _normed_model()
    model.repack_trainable = lambda: None
    ema = ModelEMA(model, momentum=0.5)
    model.arena.w.add_(1000)
    model.norms.running.add_(1000)
    w, r, e0, r0 = model.arena.w.clone(), model.norms.running.clone(), ema.e.clone(), ema.r.clone()
    with ema.applied():
        assert torch.equal(model.arena.w, e0) and torch.equal(model.norms.running, r0)
        assert torch.equal(ema.e, w) and torch.equal(ema.r, r)
    assert torch.equal(model.arena.w, w) and torch.equal(model.norms.running, r) and torch.equal(ema.e, e0) and torch.equal(ema.r, r0)
    sd = ema.state_dict()["model"]
    assert np.array_equal(sd[NORM + ".running_mean"], r0[:4].numpy()) and np.array_equal(sd[NORM + ".running_var"], r0[4:].numpy())
    assert np.array_equal(sd["head.cls_score.weight"], e0.numpy())
    assert torch.equal(model.norms.running, r) and torch.equal(ema.r, r0)


def test_load_state_dict_restores_the_buffers_and_ignores_frozen_entries(host_ops):
    from basedet_amd.layers import ModelEMA
    model = _normed_model()
    ema = ModelEMA(model, momentum=0.5)
    w, r = model.arena.w.clone(), model.norms.running.clone()
    stored = {"head.cls_score.weight": np.full(model.arena.total, 2.0, np.float32), NORM + ".running_mean": np.full(4, 3.0, np.float32),
              NORM + ".running_var": np.full(4, 4.0, np.float32), "backbone.bottom_up.bn1.running_var": np.full(3, -1.0, np.float32)}
    ema.load_state_dict({"iter": 11, "model": stored})
    assert ema.iters == 11
    assert torch.equal(ema.e, torch.full_like(w, 2.0))
    assert torch.equal(ema.r, torch.tensor([3.0] * 4 + [4.0] * 4))
    assert torch.equal(model.arena.w, w) and torch.equal(model.norms.running, r)          # the live model is untouched
    assert np.array_equal(model.bound[-1]["backbone.bottom_up.bn1.running_var"], model.frozen)      # frozen: the model's own value


def test_ema_coefficients_are_formed_in_double():
    """ema.py:80 casts `1 - m` after the subtraction in Python float64; float32(1) - float32(m) would differ for m = 0.9995."""
    from basedet_amd import ops
    m, om = ops.ema_coeffs(0.9995)
    assert np.float32(om) == np.float32(1 - 0.9995)
    assert np.float32(om) != np.float32(1) - np.float32(0.9995)
    assert ops.ema_coeffs(0) == (0.0, 1.0)
