"""SOLVER.OPTIMIZER_NAME on the host: DetSolver.build's choice of optimizer and its ValueErrors, and the fp32 restatement of the three
rules (tests/optim_rules.py, which tests/test_optim_gpu.py holds the kernels to bit for bit) against torch.optim in float64.

The float64 comparison runs 10 steps from one w0 with a fresh gradient each step: 4096 elements, |g| in [0.1, 1] with random signs,
|w0| in [0.5, 2], lr = 1e-3, wd = 1e-2.  Bound: max|w32 - w64| <= 1e-5 * max|w64 - w0| + 2^-22 * max|w| -- about ten fp32 roundings per
element and step stay well inside it (the weight's own rounding, half an ulp of a value below 2 = 6e-8 per step, dominates), while a
wrong rule (no bias correction, coupled decay for decoupled) misses it by orders of magnitude.  torch's forms are algebraically the
kernel's: AdamW's p * (1 - lr * wd) - lr * d = p - lr * (d + wd * p)."""
import numpy as np
import pytest
import torch

from tests import optim_rules as R

N, STEPS, LR, WD, BETAS, EPS, MOMENTUM = 4096, 10, 1e-3, 1e-2, (0.9, 0.999), 1e-8, 0.9


class _FakeArena:
    def __init__(self, names_sizes):
        self.entries, off = [], 0
        for n, s in names_sizes:
            self.entries.append((n, (s,), off, s))
            off += (s + 63) // 64 * 64
        self.total = off
        self.w = torch.zeros(off); self.g = torch.zeros(off); self.v = torch.zeros(off)


class _FakeModel:
    def __init__(self):
        self.arena = _FakeArena([("backbone.bottom_up.layer2.0.conv1.weight", 100), ("backbone.fpn_lateral3.weight", 64),
                                 ("head.cls_score.weight", 200), ("head.cls_score.bias", 8)])


def _cfg(name=None, extra=None, mode=None):
    from basedet_amd.configs import RetinaNetConfig
    cfg = RetinaNetConfig()
    cfg.MODEL.BATCHSIZE = 16
    if name is not None:
        cfg.SOLVER.OPTIMIZER_NAME = name
    if extra is not None:
        cfg.SOLVER.EXTRA_OPT_ARGS = dict(extra)
    if mode is not None:
        cfg.SOLVER.REDUCE_MODE = mode
    return cfg


def _build(name=None, extra=None, mode=None):
    from basedet_amd.solver import DetSolver
    cfg = _cfg(name, extra, mode)
    return cfg, DetSolver.build(cfg, _FakeModel())


def test_build_selects_the_optimizer_by_name():
    from basedet_amd import solver as S
    cfg, s = _build()                                             # the config's defaults: SGD, momentum 0.9
    assert type(s.optimizer) is S.SGD and not s.optimizer.nesterov
    assert s.optimizer.param_groups[0] == dict(lr=cfg.SOLVER.BASIC_LR * 16, weight_decay=cfg.SOLVER.WEIGHT_DECAY, momentum=0.9)
    assert not hasattr(s.optimizer, "exp_avg_sq")                  # an SGD run allocates no second moment

    _, s = _build("SGD", dict(momentum=0.8, nesterov=True))
    assert type(s.optimizer) is S.SGD and s.optimizer.nesterov and s.optimizer.param_groups[0]["momentum"] == 0.8
    _, s = _build("SGD", {})
    assert s.optimizer.param_groups[0]["momentum"] == 0.0          # megengine.optimizer.SGD's default

    for name, cls in (("Adam", S.Adam), ("AdamW", S.AdamW)):
        cfg, s = _build(name, {})
        opt = s.optimizer
        assert type(opt) is cls and opt.decoupled == (name == "AdamW")
        assert opt.param_groups[0] == dict(lr=cfg.SOLVER.BASIC_LR * 16, weight_decay=cfg.SOLVER.WEIGHT_DECAY, betas=(0.9, 0.999), eps=1e-8)
        assert opt.exp_avg_sq.shape == (opt.model.arena.total,) and opt.exp_avg_sq.dtype == torch.float32
        assert not opt.exp_avg_sq.any() and opt.step_count == 0
        _, s = _build(name, dict(betas=(0.8, 0.99), eps=1e-6))
        assert type(s.optimizer) is cls and s.optimizer.param_groups[0]["betas"] == (0.8, 0.99)
        assert s.optimizer.param_groups[0]["eps"] == 1e-6


def test_reduce_mode_scaling_is_the_same_for_every_optimizer():
    """One process: MEAN and SUM both leave lr and wd alone (world = 1); the schedule object reads the Adam group like the SGD one."""
    from basedet_amd.solver import WarmupMultiStepLR
    for name, extra in (("SGD", dict(momentum=0.9)), ("AdamW", {})):
        for mode in ("MEAN", "SUM"):
            cfg, s = _build(name, extra, mode)
            g = s.optimizer.param_groups[0]
            assert g["lr"] == cfg.SOLVER.BASIC_LR * 16 and g["weight_decay"] == cfg.SOLVER.WEIGHT_DECAY
        sched = WarmupMultiStepLR(s.optimizer, cfg)
        sched.step(0)
        assert s.optimizer.param_groups[0]["lr"] == pytest.approx(cfg.SOLVER.BASIC_LR * 16 / cfg.SOLVER.WARM_ITERS)


@pytest.mark.parametrize("name,extra,match", [
    ("RMSprop", {}, r"OPTIMIZER_NAME = 'RMSprop'.*\['Adam', 'AdamW', 'SGD'\]"),
    ("adamw", {}, r"\['Adam', 'AdamW', 'SGD'\]"),
    ("SGD", dict(momentum=0.9, betas=(0.9, 0.999)), r"\['betas'\].*'SGD'.*\['momentum', 'nesterov'\]"),
    ("SGD", dict(dampening=0.1), r"\['dampening'\].*\['momentum', 'nesterov'\]"),
    ("AdamW", dict(momentum=0.9), r"\['momentum'\].*'AdamW'.*\['betas', 'eps'\]"),         # the config's own default EXTRA_OPT_ARGS
    ("Adam", dict(nesterov=True), r"\['nesterov'\].*'Adam'.*\['betas', 'eps'\]"),
    ("Adam", dict(amsgrad=True), r"\['amsgrad'\].*\['betas', 'eps'\]"),
    ("SGD", dict(nesterov=True), r"nesterov=True requires a momentum > 0"),
    ("SGD", dict(nesterov=True, momentum=0.0), r"nesterov=True requires a momentum > 0"),
    ("Adam", dict(betas=(0.9, 1.0)), r"betas"),
    ("AdamW", dict(eps=-1e-8), r"eps"),
])
def test_build_refuses_what_it_does_not_implement(name, extra, match):
    from basedet_amd.solver import DetSolver
    with pytest.raises(ValueError, match=match):
        DetSolver.build(_cfg(name, extra), _FakeModel())


def test_default_config_with_another_name_raises_instead_of_training_sgd():
    """OPTIMIZER_NAME = "AdamW" on top of the default EXTRA_OPT_ARGS (momentum = 0.9): the parent commit trained plain SGD here."""
    from basedet_amd.solver import DetSolver
    with pytest.raises(ValueError, match="momentum"):
        DetSolver.build(_cfg("AdamW"), _FakeModel())


# ---- the fp32 rules against float64 optimizers ---------------------------------------------------------------------------------------
def _problem():
    rng = np.random.default_rng(7)
    sign = lambda n: rng.choice(np.array([-1.0, 1.0]), n)             # noqa: E731
    w0 = (rng.uniform(0.5, 2.0, N) * sign(N)).astype(np.float32)
    gs = [(rng.uniform(0.1, 1.0, N) * sign(N)).astype(np.float32) for _ in range(STEPS)]
    return w0, gs


def _run32(kind, w0, gs):
    w, m, v = w0.copy(), np.zeros(N, np.float32), np.zeros(N, np.float32)
    for t, g in enumerate(gs, start=1):
        if kind == "nesterov":
            w, m = R.sgd_nesterov(w, m, g, LR, MOMENTUM, WD)
        else:
            w, m, v = R.adam(w, m, v, g, LR, BETAS, EPS, WD, t, decoupled=(kind == "adamw"))
    return w


def _run_torch64(kind, w0, gs):
    p = torch.nn.Parameter(torch.from_numpy(w0.astype(np.float64)))
    if kind == "nesterov":
        opt = torch.optim.SGD([p], lr=LR, momentum=MOMENTUM, weight_decay=WD, nesterov=True)
    else:
        cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
        opt = cls([p], lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    for g in gs:
        p.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
    return p.detach().numpy().copy()


def _run_megengine(kind, w0, gs):
    """The same steps through megengine.optimizer (fp32), or None where megengine is not installed."""
    try:
        import megengine as mge
        import megengine.optimizer as mopt
    except ImportError:
        return None
    p = mge.Parameter(w0.copy())
    if kind == "nesterov":
        opt = mopt.SGD([p], lr=LR, momentum=MOMENTUM, weight_decay=WD, nesterov=True)
    else:
        cls = mopt.AdamW if kind == "adamw" else mopt.Adam
        opt = cls([p], lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    for g in gs:
        p.grad = mge.tensor(g)
        opt.step()
    return p.numpy().copy()


@pytest.mark.parametrize("kind", ["adam", "adamw", "nesterov"])
def test_fp32_rule_matches_float64_optimizer(kind):
    w0, gs = _problem()
    w32 = _run32(kind, w0, gs)
    w64 = _run_torch64(kind, w0, gs)
    moved = float(np.abs(w64 - w0).max())
    bound = 1e-5 * moved + 2.0 ** -22 * float(np.abs(w64).max())
    err = float(np.abs(w32.astype(np.float64) - w64).max())
    print(f"{kind}: max|w32 - w64| = {err:.3e}, bound {bound:.3e}, max|w64 - w0| = {moved:.3e}")
    assert moved > 5e-3                                            # ten steps of about lr each
    assert err <= bound
    wm = _run_megengine(kind, w0, gs)
    if wm is not None:              # two fp32 runs, each within `bound` of the float64 one
        err_m = float(np.abs(w32.astype(np.float64) - wm.astype(np.float64)).max())
        print(f"{kind}: max|w32 - megengine| = {err_m:.3e}")
        assert err_m <= 2 * bound


@pytest.mark.parametrize("wrong", ["no bias correction", "coupled for decoupled", "plain momentum for nesterov"])
def test_bound_tells_a_wrong_rule_apart(wrong):
    """The bound above is not vacuous: each of these mistakes misses it by more than a factor of 30."""
    w0, gs = _problem()
    w, m, v = w0.copy(), np.zeros(N, np.float32), np.zeros(N, np.float32)
    if wrong == "plain momentum for nesterov":
        for g in gs:
            gg = g + np.float32(WD) * w
            m = np.float32(MOMENTUM) * m + gg
            w = w - np.float32(LR) * m
        w64 = _run_torch64("nesterov", w0, gs)
    elif wrong == "coupled for decoupled":
        w = _run32("adam", w0, gs)
        w64 = _run_torch64("adamw", w0, gs)
    else:
        for g in gs:
            w, m, v = R.adam(w, m, v, g, LR, BETAS, EPS, WD, 10 ** 9, decoupled=True)      # bc1 = bc2 = 1
        w64 = _run_torch64("adamw", w0, gs)
    bound = 1e-5 * float(np.abs(w64 - w0).max()) + 2.0 ** -22 * float(np.abs(w64).max())
    err = float(np.abs(w.astype(np.float64) - w64).max())
    print(f"{wrong}: error {err:.3e} against a bound of {bound:.3e}")
    assert err > 30 * bound


def test_ops_form_the_scalars_the_rule_uses():
    """ops.adam_coeffs (what the kernel receives) and the restatement's scalars are the same fp32 values, bias corrections included."""
    import ctypes as C
    from basedet_amd import ops
    for step in (1, 2, 1000, 10 ** 6):
        got = [C.c_float(x).value for x in ops.adam_coeffs(BETAS, step)]
        assert got == [float(x) for x in R.adam_scalars(BETAS, step)]
    assert ops.adam_coeffs((0.9, 0.999), 1)[4:] == (1 - 0.9, 1 - 0.999)


def test_state_dict_surface_exists_on_all_three():
    from basedet_amd import solver as S
    for cls in (S.SGD, S.Adam, S.AdamW):
        assert callable(getattr(cls, "state_dict")) and callable(getattr(cls, "load_state_dict"))
        assert callable(getattr(cls, "step")) and callable(getattr(cls, "clear_grad"))
