"""SOLVER.OPTIMIZER_NAME on the device: bd_adam_step, bd_adam_ema_step, bd_sgd_nesterov_step and bd_sgd_nesterov_ema_step (csrc/optim.hip)
bit for bit against the numpy fp32 restatement of tests/optim_rules.py (which tests/test_optim_cpu.py holds to float64 optimizers), their
argument checks, a guard-band launch, and Adam / AdamW / SGD through DetSolver.build on the smallest RetinaNet (R18, 2 x 64 x 64).

Every comparison is of BITS (uint32 views): optim.hip is built without FMA contraction and with IEEE division and square root, so each
operation of the rule is one fp32 rounding, which numpy's float32 arithmetic computes identically -- no tolerance is involved."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import optim_rules as R
from tests import util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BD_EINVAL = -1
LR, BETAS, EPS, WD, MOMENTUM, EMA_M = 1e-3, (0.9, 0.999), 1e-8, 1e-2, 0.9, 0.9995


def _full_pass():
    """Elements one pass of the capped grid covers: grid_for's cap (csrc/common.h) x 256 lanes x 4 elements."""
    src = open(os.path.join(ROOT, "basedet_amd", "csrc", "common.h")).read()
    m = re.search(r"int grid_for\(long long n, int block = (\d+), int cap = (\d+)\)", src)
    assert m, "grid_for not found in csrc/common.h"
    return int(m.group(2)) * int(m.group(1)) * 4


BIG = 2 ** 22 + 7                        # one element-quad past a full pass: the stride loop takes a second trip and ends in a scalar tail
SIZES = [1, 3, 4, 5, 1023, BIG]
# (w, m, v, g, e) planted at (k * 37) % n: all zeros (must stay +0); a denormal second moment under a gradient whose square underflows (w = 0: no decay joins it);
# a denormal second moment under a zero gradient; a denormal first moment and weight
SPECIALS = np.array([[0.0, 0.0, 0.0, 0.0, 0.0],
                     [0.0, 0.01, 1e-40, 1e-23, 0.5],
                     [-1.5, -0.02, 3e-42, 0.0, -1.0],
                     [2e-41, 1e-39, 0.01, 0.25, 1e-40]], np.float32)


def test_big_size_is_what_the_docstring_says():
    assert BIG == _full_pass() + 4 + 3


@functools.lru_cache(maxsize=None)
def _host(n):
    """(w, m, v, g, e) for a length, read-only: normal data, v >= 0, with the SPECIALS planted."""
    rng = np.random.default_rng(2000 + n % 9973)
    w, m, v, g, e = (rng.standard_normal(n).astype(np.float32) for _ in range(5))
    m *= np.float32(0.1)
    v = np.abs(v) * np.float32(0.01)
    pos = (np.arange(len(SPECIALS)) * 37) % n
    for k, p in enumerate(pos[:n]):
        w[p], m[p], v[p], g[p], e[p] = SPECIALS[k]
    for a in (w, m, v, g, e):
        a.setflags(write=False)
    return w, m, v, g, e


def _dev(a):
    return torch.from_numpy(a.copy()).cuda()


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(name, got, ref):
    diff = int((_bits(got) != _bits(ref)).sum())
    print(f"{name}: {diff} of {_bits(ref).size} elements differ from the numpy restatement")
    assert diff == 0, name


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_adam_step_bits(decoupled, n, step, grad_scale):
    """bd_adam_step and bd_adam_ema_step, one launch each on copies of the same inputs."""
    from basedet_amd import ops
    w, m, v, g, e = _host(n)
    rw, rm, rv = R.adam(w, m, v, g, LR, BETAS, EPS, WD, step, grad_scale, decoupled)
    re_ = R.ema(e, rw, EMA_M)
    w0, m0, v0, g0 = _dev(w), _dev(m), _dev(v), _dev(g)
    ops.adam_step(w0, m0, v0, g0, LR, BETAS, EPS, WD, step, grad_scale, decoupled)
    w1, m1, v1, g1, e1 = _dev(w), _dev(m), _dev(v), _dev(g), _dev(e)
    ops.adam_ema_step(w1, m1, v1, g1, e1, LR, BETAS, EPS, WD, step, grad_scale, decoupled, EMA_M)
    torch.cuda.synchronize()
    for name, plain, fused, ref in (("w", w0, w1, rw), ("m", m0, m1, rm), ("v", v0, v1, rv), ("g", g0, g1, g)):
        _same(f"n={n} plain {name}", plain, ref)
        _same(f"n={n} with ema {name}", fused, ref)
        assert np.array_equal(_bits(plain), _bits(fused)), name          # the two entries agree
    _same(f"n={n} e", e1, re_)
    assert np.isfinite(rw).all() and np.isfinite(rv).all()
    assert not np.array_equal(_bits(w0), _bits(w)) or n == 1           # the step did something (n = 1 is the all-zero element alone)
    assert all(int(_bits(t)[0]) == 0 for t in (w0, m0, v0, w1, m1, v1, e1))          # the all-zero element stays +0
    if n >= 3:
        p = 37 % n                                                       # the denormal second moment is still a nonzero denormal
        assert 0 < float(v0[p]) < np.finfo(np.float32).tiny and _bits(v0)[p] == _bits(rv)[p]


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("n", SIZES)
def test_sgd_nesterov_step_bits(n, grad_scale):
    """bd_sgd_nesterov_step and bd_sgd_nesterov_ema_step, one launch each on copies of the same inputs."""
    from basedet_amd import ops
    w, m, _, g, e = _host(n)
    rw, rv = R.sgd_nesterov(w, m, g, LR, MOMENTUM, WD, grad_scale)
    re_ = R.ema(e, rw, EMA_M)
    w0, v0, g0 = _dev(w), _dev(m), _dev(g)
    ops.sgd_nesterov_step(w0, v0, g0, LR, MOMENTUM, WD, grad_scale)
    w1, v1, g1, e1 = _dev(w), _dev(m), _dev(g), _dev(e)
    ops.sgd_nesterov_ema_step(w1, v1, g1, e1, LR, MOMENTUM, WD, grad_scale, EMA_M)
    torch.cuda.synchronize()
    for name, plain, fused, ref in (("w", w0, w1, rw), ("v", v0, v1, rv), ("g", g0, g1, g)):
        _same(f"n={n} plain {name}", plain, ref)
        _same(f"n={n} with ema {name}", fused, ref)
        assert np.array_equal(_bits(plain), _bits(fused)), name
    _same(f"n={n} e", e1, re_)
    assert not np.array_equal(_bits(w0), _bits(w)) or n == 1              # (n = 1 is the all-zero element alone)
    assert all(int(_bits(t)[0]) == 0 for t in (w0, v0, w1, v1, e1))


def test_bad_arguments_return_einval_and_launch_nothing():
    """Every refused call leaves the (poisoned) buffers alone.  All pointers are null or lie inside allocations of n + 4 elements, so
    even a library that launched would stay in bounds."""
    from basedet_amd import _lib
    lib = _lib.load()
    n = 64
    bufs = [torch.full((n + 4,), float(k + 1), device="cuda") for k in range(5)]
    for t in bufs:
        U.bits_of(t).copy_(U.fill_pattern(torch.float32, "sentinel", n + 4, "cuda"))
    w, m, v, g, e = bufs
    before = [t.clone() for t in bufs]
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off)         # noqa: E731
    null, st = C.c_void_p(0), _lib.stream_ptr()
    b1, b2 = 0.9, 0.999
    ok = dict(lr=LR, b1=b1, omb1=1 - b1, b2=b2, omb2=1 - b2, bc1=0.1, bc2=0.001, eps=EPS, wd=WD, gs=1.0)

    def sc(**kw):
        d = dict(ok, **kw)
        return [d[k] for k in ("lr", "b1", "omb1", "b2", "omb2", "bc1", "bc2", "eps", "wd", "gs")]

    def adam(pw=P(w), pm=P(m), pv=P(v), pg=P(g), nn=n, dec=1, **kw):
        return lib.bd_adam_step(pw, pm, pv, pg, nn, *sc(**kw), dec, st)

    def adam_e(pw=P(w), pm=P(m), pv=P(v), pg=P(g), pe=P(e), nn=n, dec=0, **kw):
        return lib.bd_adam_ema_step(pw, pm, pv, pg, pe, nn, *sc(**kw), dec, 0.5, 0.5, st)

    sgd = (LR, MOMENTUM, WD, 1.0)

    def nag(pw=P(w), pv=P(v), pg=P(g), nn=n):
        return lib.bd_sgd_nesterov_step(pw, pv, pg, nn, *sgd, st)

    def nag_e(pw=P(w), pv=P(v), pg=P(g), pe=P(e), nn=n):
        return lib.bd_sgd_nesterov_ema_step(pw, pv, pg, pe, nn, *sgd, 0.5, 0.5, st)

    calls = {}
    for tag, f in (("adam", adam), ("adam+ema", adam_e)):
        calls.update({
            f"{tag} negative n": lambda f=f: f(nn=-1),
            f"{tag} null w": lambda f=f: f(pw=null), f"{tag} null m": lambda f=f: f(pm=null),
            f"{tag} null v": lambda f=f: f(pv=null), f"{tag} null g": lambda f=f: f(pg=null),
            f"{tag} misaligned w": lambda f=f: f(pw=P(w, 1)), f"{tag} misaligned m": lambda f=f: f(pm=P(m, 2)),
            f"{tag} misaligned v": lambda f=f: f(pv=P(v, 3)), f"{tag} misaligned g": lambda f=f: f(pg=P(g, 1)),
            f"{tag} m aliases v": lambda f=f: f(pm=P(v)), f"{tag} m overlaps v": lambda f=f: f(pm=P(v, 4)),
            f"{tag} m aliases w": lambda f=f: f(pm=P(w)), f"{tag} m overlaps w": lambda f=f: f(pm=P(w, 4)),
            f"{tag} v aliases w": lambda f=f: f(pv=P(w)), f"{tag} v overlaps w": lambda f=f: f(pw=P(v, 4)),
            f"{tag} bc1 zero": lambda f=f: f(bc1=0.0), f"{tag} bc1 negative": lambda f=f: f(bc1=-0.1),
            f"{tag} bc2 zero": lambda f=f: f(bc2=0.0), f"{tag} bc2 negative": lambda f=f: f(bc2=-0.001),
            f"{tag} eps negative": lambda f=f: f(eps=-1e-8),
            f"{tag} beta1 negative": lambda f=f: f(b1=-0.1), f"{tag} beta1 one": lambda f=f: f(b1=1.0),
            f"{tag} beta2 negative": lambda f=f: f(b2=-0.1), f"{tag} beta2 above one": lambda f=f: f(b2=1.5),
        })
    calls.update({
        "adam+ema null e": lambda: adam_e(pe=null), "adam+ema misaligned e": lambda: adam_e(pe=P(e, 1)),
        "adam+ema e aliases w": lambda: adam_e(pe=P(w)), "adam+ema e overlaps w": lambda: adam_e(pe=P(w, 4)),
        "adam+ema e aliases m": lambda: adam_e(pe=P(m)), "adam+ema e overlaps m": lambda: adam_e(pe=P(m, 4)),
        "adam+ema e aliases v": lambda: adam_e(pe=P(v)), "adam+ema e overlaps v": lambda: adam_e(pe=P(v, 4)),
        "adam+ema e aliases g": lambda: adam_e(pe=P(g)), "adam+ema e overlaps g": lambda: adam_e(pe=P(g, 4)),
    })
    for tag, f in (("nesterov", nag), ("nesterov+ema", nag_e)):
        calls.update({
            f"{tag} negative n": lambda f=f: f(nn=-1),
            f"{tag} null w": lambda f=f: f(pw=null), f"{tag} null v": lambda f=f: f(pv=null), f"{tag} null g": lambda f=f: f(pg=null),
            f"{tag} misaligned w": lambda f=f: f(pw=P(w, 1)), f"{tag} misaligned v": lambda f=f: f(pv=P(v, 2)),
            f"{tag} misaligned g": lambda f=f: f(pg=P(g, 3)),
            f"{tag} v aliases w": lambda f=f: f(pv=P(w)), f"{tag} v overlaps w": lambda f=f: f(pv=P(w, 4)),
        })
    calls.update({
        "nesterov+ema null e": lambda: nag_e(pe=null), "nesterov+ema misaligned e": lambda: nag_e(pe=P(e, 1)),
        "nesterov+ema e aliases w": lambda: nag_e(pe=P(w)), "nesterov+ema e overlaps w": lambda: nag_e(pe=P(w, 4)),
        "nesterov+ema e aliases v": lambda: nag_e(pe=P(v)), "nesterov+ema e overlaps v": lambda: nag_e(pe=P(v, 4)),
        "nesterov+ema e aliases g": lambda: nag_e(pe=P(g)), "nesterov+ema e overlaps g": lambda: nag_e(pe=P(g, 4)),
    })
    for name, call in calls.items():
        assert call() == BD_EINVAL, name
        assert lib.bd_last_error_string(), name
    torch.cuda.synchronize()
    for t, b in zip(bufs, before):
        assert torch.equal(U.bits_of(t), U.bits_of(b))
    # n == 0 is a no-op that succeeds, whatever the pointers
    assert adam(null, null, null, null, nn=0) == 0 and adam_e(null, null, null, null, null, nn=0) == 0
    assert nag(null, null, null, nn=0) == 0 and nag_e(null, null, null, null, nn=0) == 0


def test_adam_ema_launch_stays_inside_its_buffers():
    """Guard bands (tests/util.py: guarded): n = 1023 -- 255 quads and a 3-element tail -- with every buffer inside a larger allocation whose
    bytes in front and behind hold a sentinel (256-byte aligned interiors).  The guards keep their bits; the interiors get the rule's."""
    from basedet_amd import ops
    n = 1023
    host = _host(n)
    hs = []
    for name, a in zip("wmvge", host):
        t, h = U.guarded(n, None, torch.float32, "cuda", name=name)
        h.set(torch.from_numpy(a.copy()))
        h.snapshot()
        assert t.data_ptr() % 16 == 0
        hs.append(h)
    w, m, v, g, e = (h.t for h in hs)
    ops.adam_ema_step(w, m, v, g, e, LR, BETAS, EPS, WD, 3, 0.5, True, EMA_M)
    torch.cuda.synchronize()
    for h in hs:
        h.check()                                                        # both guards of every buffer hold the sentinel
    hs[3].assert_unchanged()                                             # g: data included
    rw, rm, rv = R.adam(*host[:4], LR, BETAS, EPS, WD, 3, 0.5, True)
    for name, t, ref in (("w", w, rw), ("m", m, rm), ("v", v, rv), ("e", e, R.ema(host[4], rw, EMA_M))):
        _same(name, t, ref)


# ---- model level ------------------------------------------------------------------------------------------------------------------------
N_IMG, SIZE, K, A, STEPS, EMA_MODEL_M = 2, (64, 64), 3, 9, 3, 0.5


def _setup(optimizer, extra, ema=False):
    from basedet_amd.configs import retinanet_r18_config
    from basedet_amd.models import params as P
    from tests.test_class_count_gpu import _batch
    cfg = retinanet_r18_config()
    cfg.MODEL.BATCHSIZE = N_IMG
    cfg.DATA.NUM_CLASSES = K
    cfg.SOLVER.OPTIMIZER_NAME = optimizer
    cfg.SOLVER.EXTRA_OPT_ARGS = dict(extra)
    cfg.SOLVER.BASIC_LR = 1e-4 / N_IMG                                   # lr 1e-4: an Adam step moves every weight by about lr
    if ema:
        cfg.TRAINER.EMA.merge(dict(ENABLE=True, MOMENTUM=EMA_MODEL_M, BURNIN_ITER=1))     # step 1: burn-in copy; steps 2, 3: in the launch
    return cfg, P.init_retinanet_params(cfg, 0), _batch(N_IMG, SIZE, K)


def _pads(model, flat, name):
    """The pad rows (class slots K .. ld - 1 of every anchor) of cls_score's weight or bias inside an arena-shaped buffer."""
    _, shape, off, n = {e[0]: e for e in model.arena.entries}[name]
    t = flat[off:off + n].view(shape)
    ld = shape[0] // A
    assert ld > K
    return t.reshape((A, ld) + tuple(shape[1:]))[:, K:]


@pytest.fixture(scope="module")
def adamw():
    """Three DetTrainer.model_step calls under OPTIMIZER_NAME = "AdamW" with TRAINER.EMA (burn-in 1); arena.g, arena.w and both moments
    cloned after each.  Then the optimizer's state_dict, a fourth step, and the same fourth step on a fresh model + solver resumed from
    that state."""
    from basedet_amd.engine import DetTrainer
    from basedet_amd.models import RetinaNet
    from basedet_amd.solver import AdamW, DetSolver
    cfg, params, batch = _setup("AdamW", {}, ema=True)
    model = RetinaNet(cfg, params=params)
    solver = DetSolver.build(cfg, model)
    opt = solver.optimizer
    assert type(opt) is AdamW
    tr = DetTrainer(cfg, model, [], solver)
    out = dict(cfg=cfg, params=params, model=model, opt=opt, group=dict(opt.param_groups[0]))
    out["w0"], out["e0"] = model.arena.w.clone(), tr.ema.e.clone()
    snap = lambda: dict(g=model.arena.g.clone(), w=model.arena.w.clone(), m=model.arena.v.clone(), v=opt.exp_avg_sq.clone())   # noqa: E731
    out["after"] = []
    for _ in range(STEPS):
        losses = tr.model_step(batch)
        assert np.isfinite(float(losses["total_loss"]))
        out["after"].append(snap())
    out["e3"] = tr.ema.e.clone()
    torch.cuda.synchronize()

    out["sd"] = opt.state_dict()
    out["after_sd"] = snap()
    weights = model.state_dict()
    solver.minimize(model, batch)
    out["fourth"] = snap()

    cfg2, _, _ = _setup("AdamW", {})
    model2 = RetinaNet(cfg2, params=weights)
    solver2 = DetSolver.build(cfg2, model2)
    solver2.optimizer.load_state_dict(out["sd"])
    out["resumed_loaded"] = dict(w=model2.arena.w.clone(), m=model2.arena.v.clone(), v=solver2.optimizer.exp_avg_sq.clone())
    out["model2"], out["opt2"] = model2, solver2.optimizer
    solver2.minimize(model2, batch)
    out["resumed_fourth"] = dict(g=model2.arena.g.clone(), w=model2.arena.w.clone(), m=model2.arena.v.clone(),
                                 v=solver2.optimizer.exp_avg_sq.clone())
    torch.cuda.synchronize()
    return out


def test_adamw_moves_the_arena_as_the_rule_says(adamw):
    g = adamw["group"]
    assert g["betas"] == BETAS and g["eps"] == EPS and g["weight_decay"] > 0 and g["lr"] == pytest.approx(1e-4)
    w = adamw["w0"].cpu().numpy()
    m, v = np.zeros_like(w), np.zeros_like(w)
    for t, s in enumerate(adamw["after"], start=1):
        grad = s["g"].cpu().numpy()
        assert np.isfinite(grad).all() and (grad != 0).any()
        w, m, v = R.adam(w, m, v, grad, g["lr"], g["betas"], g["eps"], g["weight_decay"], t, 1.0, decoupled=True)
        for name, ref in (("w", w), ("m", m), ("v", v)):
            _same(f"step {t} arena {name}", s[name], ref)
    assert adamw["opt"].step_count == STEPS + 1
    assert not np.array_equal(_bits(w), _bits(adamw["w0"]))


def test_adamw_pad_rows_stay_zero(adamw):
    model = adamw["model"]
    for s in adamw["after"] + [adamw["fourth"]]:
        for name in ("head.cls_score.weight", "head.cls_score.bias"):
            for which in ("w", "m", "v", "g"):
                p = _pads(model, s[which], name)
                assert p.numel() > 0 and not (_bits(p) != 0).any(), (name, which)
    _, shape, off, n = {e[0]: e for e in model.arena.entries}["head.cls_score.weight"]
    assert bool((adamw["after"][-1]["v"][off:off + n] != 0).any())        # while the real rows have a second moment


def test_adamw_ema_follows_the_recurrence(adamw):
    """Burn-in 1: update(0) + update(0.5) after step 1 (separate launches), update(0.5) inside the AdamW launch at steps 2 and 3."""
    assert np.array_equal(_bits(adamw["e0"]), _bits(adamw["w0"]))
    e = adamw["w0"].cpu().numpy().copy()
    for it, s in enumerate(adamw["after"], start=1):
        w = s["w"].cpu().numpy()
        if it == 1:
            e = R.ema(e, w, 0)
        e = R.ema(e, w, EMA_MODEL_M)
    _same("ema.e", adamw["e3"], e)
    assert not np.array_equal(_bits(adamw["e3"]), _bits(adamw["after"][-1]["w"]))


def test_adamw_state_dict_resumes_with_the_same_bits(adamw):
    sd, model = adamw["sd"], adamw["model"]
    for k in ("w", "m", "v", "g"):                                        # reading the state leaves the run alone
        assert np.array_equal(_bits(adamw["after_sd"][k]), _bits(adamw["after"][-1][k])), k
    assert sd["step"] == STEPS and set(sd) == {"step", "exp_avg", "exp_avg_sq"}
    names = set(model.state_dict_trainable_names())
    for key in ("exp_avg", "exp_avg_sq"):
        assert set(sd[key]) == names
        for nme, arr in sd[key].items():                                  # the reference's shapes: cls_score without its pad rows
            assert tuple(arr.shape) == tuple(adamw["params"][nme].shape), (key, nme)
    assert sd["exp_avg_sq"]["head.cls_score.weight"].shape == (A * K, 256, 3, 3)
    assert all((a >= 0).all() for a in sd["exp_avg_sq"].values()) and any(a.any() for a in sd["exp_avg"].values())
    last, loaded = adamw["after"][-1], adamw["resumed_loaded"]
    for k in ("w", "m", "v"):                                             # the fresh solver holds the interrupted run's bits, pads as zeros
        assert np.array_equal(_bits(loaded[k]), _bits(last[k])), k
    for name in ("head.cls_score.weight", "head.cls_score.bias"):
        for k in ("m", "v"):
            assert not (_bits(_pads(adamw["model2"], loaded[k], name)) != 0).any()
    assert adamw["opt2"].step_count == STEPS + 1
    for k in ("g", "w", "m", "v"):
        diff = int((_bits(adamw["resumed_fourth"][k]) != _bits(adamw["fourth"][k])).sum())
        print(f"fourth step, {k}: {diff} elements differ between the resumed and the uninterrupted run")
        assert diff == 0, k
    assert not np.array_equal(_bits(adamw["fourth"]["w"]), _bits(last["w"]))


def test_adam_through_the_solver_is_the_coupled_rule():
    """OPTIMIZER_NAME = "Adam" with EXTRA_OPT_ARGS: one step, the coupled rule with the configured betas and eps."""
    from basedet_amd.models import RetinaNet
    from basedet_amd.solver import Adam, DetSolver
    cfg, params, batch = _setup("Adam", dict(betas=(0.8, 0.99), eps=1e-6))
    model = RetinaNet(cfg, params=params)
    solver = DetSolver.build(cfg, model)
    assert type(solver.optimizer) is Adam
    w0 = model.arena.w.cpu().numpy()
    solver.minimize(model, batch)
    torch.cuda.synchronize()
    g = solver.optimizer.param_groups[0]
    z = np.zeros_like(w0)
    w, m, v = R.adam(w0, z, z, model.arena.g.cpu().numpy(), g["lr"], (0.8, 0.99), 1e-6, g["weight_decay"], 1, 1.0, decoupled=False)
    _same("w", model.arena.w, w)
    _same("m", model.arena.v, m)
    _same("v", solver.optimizer.exp_avg_sq, v)


def test_sgd_by_name_is_the_parent_commits_sgd():
    """OPTIMIZER_NAME = "SGD" through DetSolver.build against SGD(model, lr, wd, momentum) built directly, the way the solver was built
    before it read the name: three steps, the same bits in w and v; and a state_dict round trip of the velocity."""
    from basedet_amd.models import RetinaNet
    from basedet_amd.solver import SGD, DetSolver, GradBuckets, Solver
    cfg, params, batch = _setup("SGD", dict(momentum=0.9))
    ma = RetinaNet(cfg, params=params)
    sa = DetSolver.build(cfg, ma)
    assert type(sa.optimizer) is SGD and not sa.optimizer.nesterov and not hasattr(sa.optimizer, "exp_avg_sq")
    mb = RetinaNet(cfg, params=params)
    s = cfg.SOLVER
    sb = Solver(SGD(mb, s.BASIC_LR * N_IMG, s.WEIGHT_DECAY, 0.9), GradBuckets(mb, "MEAN"))
    for _ in range(STEPS):
        sa.minimize(ma, batch)
        sb.minimize(mb, batch)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(ma.arena.w), _bits(mb.arena.w)) and np.array_equal(_bits(ma.arena.v), _bits(mb.arena.v))
    assert bool((ma.arena.v != 0).any())
    sd = sa.optimizer.state_dict()
    assert sd["step"] == STEPS and sd["momentum_buffer"]["head.cls_score.bias"].shape == (A * K,)
    v_before = mb.arena.v.clone()
    mb.arena.v.zero_()
    sb.optimizer.load_state_dict(sd)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(mb.arena.v), _bits(v_before)) and np.array_equal(_bits(mb.arena.w), _bits(ma.arena.w))


def test_nesterov_through_the_solver():
    """EXTRA_OPT_ARGS nesterov=True: one step is the look-ahead rule on the recorded gradient."""
    from basedet_amd.models import RetinaNet
    from basedet_amd.solver import DetSolver
    cfg, params, batch = _setup("SGD", dict(momentum=0.9, nesterov=True))
    model = RetinaNet(cfg, params=params)
    solver = DetSolver.build(cfg, model)
    assert solver.optimizer.nesterov
    w0 = model.arena.w.cpu().numpy()
    solver.minimize(model, batch)
    torch.cuda.synchronize()
    g = solver.optimizer.param_groups[0]
    w, v = R.sgd_nesterov(w0, np.zeros_like(w0), model.arena.g.cpu().numpy(), g["lr"], 0.9, g["weight_decay"], 1.0)
    _same("w", model.arena.w, w)
    _same("v", model.arena.v, v)
