"""TRAINER.EMA on the device: bd_ema_update, bd_sgd_momentum_ema_step and bd_swap_f32 (csrc/ema.hip) bit for bit against a numpy fp32
restatement of basedet/layers/common/ema.py:80, and ModelEMA / SGD.step(ema=...) / DetTrainer through six training steps of the small
RetinaNet-R18 configuration of tests/test_model_gpu.py.

Every comparison is of BITS (uint32 views): the update is two fp32 products and one fp32 sum, each rounded once, which numpy's float32
arithmetic computes identically -- no tolerance is involved.

One case cannot hold as the words "m = 0 reproduces w bit for bit" read: IEEE 754 gives (+0) + (-0) = +0, so where w is -0 and e * 0 is
+0 the mandated arithmetic (no special-cased copy) returns +0, as numpy does.  The m = 0 check therefore asks for w's bits everywhere
except at such elements, and for +0 there; the inputs hold both kinds of element."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BD_EINVAL = -1


def _full_pass():
    """Elements one pass of the capped grid covers: grid_for's cap (csrc/common.h) x 256 lanes x 4 elements."""
    src = open(os.path.join(ROOT, "basedet_amd", "csrc", "common.h")).read()
    m = re.search(r"int grid_for\(long long n, int block = (\d+), int cap = (\d+)\)", src)
    assert m, "grid_for not found in csrc/common.h"
    return int(m.group(2)) * int(m.group(1)) * 4


SIZES = [0, 1, 3, 4, 5, 255, 257, 2 ** 20 + 3, _full_pass() + 4 * 256 * 3 + 5]      # the last: a second trip through the loop + a tail
MOMENTA = [0, 0.5, 0.9995, 1]
SPECIALS_E = np.array([0.0, -0.0, 1e-40, -3e-42, 7.5, -0.0, 0.0], np.float32)
SPECIALS_W = np.array([-0.0, -0.0, -2e-41, 1.4e-45, 0.0, 0.0, 1e-39], np.float32)         # (e, w) zero pairs: (+0,-0) (-0,-0) (-0,+0) (+0,+0)


@functools.lru_cache(maxsize=None)
def _host(n):
    """(e, w, v, g) for a length, read-only; normal data with denormals and signed zeros in e and w."""
    rng = np.random.default_rng(1000 + n % 9973)
    e, w, v, g = (rng.standard_normal(n).astype(np.float32) for _ in range(4))
    pos = (np.arange(len(SPECIALS_E)) * 37) % max(n, 1)
    for k, p in enumerate(pos[: n]):
        e[p], w[p] = SPECIALS_E[k], SPECIALS_W[k]
    for a in (e, w, v, g):
        a.setflags(write=False)
    return e, w, v, g


def _dev(a):
    return torch.from_numpy(a.copy()).cuda()


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ema_ref(e, w, m):
    """ema.py:80 `v * mge.tensor(m) + mge.tensor(1 - m) * model_state` in numpy fp32: (e * f32(m)) + (f32(1 - m) * w)."""
    return (e * np.float32(m)) + (np.float32(1 - m) * w)


@pytest.mark.parametrize("m", MOMENTA)
@pytest.mark.parametrize("n", SIZES)
def test_ema_update_bits(n, m):
    from basedet_amd import ops
    e, w, _, _ = _host(n)
    de, dw = _dev(e), _dev(w)
    ops.ema_update(de, dw, m)
    torch.cuda.synchronize()
    got, ref = _bits(de), _bits(_ema_ref(e, w, m))
    print(f"n={n} m={m}: {int((got != ref).sum())} of {n} elements differ from the numpy restatement")
    assert np.array_equal(got, ref)
    assert np.array_equal(_bits(dw), _bits(w))                        # w is read only
    if m == 0 and n:
        wb = _bits(w)
        lost_sign = (wb == 0x80000000) & (_bits(e * np.float32(0)) == 0)        # (+0) + (-0) = +0: see the module docstring
        assert np.array_equal(got[~lost_sign], wb[~lost_sign])
        assert np.all(got[lost_sign] == 0)
        if n >= 255:
            assert lost_sign.sum() >= 1 and ((wb == 0x80000000) & ~lost_sign).sum() >= 1      # both kinds of -0 element are present


@pytest.mark.parametrize("n", SIZES)
def test_sgd_momentum_ema_step_bits(n):
    """w and v: the bits of bd_sgd_momentum_step on copies of the same inputs; e: bd_ema_update applied to that resulting w."""
    from basedet_amd import ops
    e, w, v, g = _host(n)
    lr, mom, wd, gs, m = 0.01, 0.9, 1e-4, 0.5, 0.9995
    w0, v0, g0 = _dev(w), _dev(v), _dev(g)
    if n:                  # (an empty torch tensor has a null pointer, which bd_sgd_momentum_step refuses even for n = 0: nothing to compare with)
        ops.sgd_momentum_step(w0, v0, g0, lr, mom, wd, gs)
    e0 = _dev(e)
    ops.ema_update(e0, w0, m)
    w1, v1, g1, e1 = _dev(w), _dev(v), _dev(g), _dev(e)
    ops.sgd_momentum_ema_step(w1, v1, g1, e1, lr, mom, wd, gs, m)
    torch.cuda.synchronize()
    for name, a, b in (("w", w1, w0), ("v", v1, v0), ("e", e1, e0), ("g", g1, g0)):
        diff = int((_bits(a) != _bits(b)).sum())
        print(f"n={n} {name}: {diff} of {n} elements differ")
        assert diff == 0, name
    assert np.array_equal(_bits(e1), _bits(_ema_ref(e, w0.cpu().numpy(), m)))
    if n:
        assert not np.array_equal(_bits(w1), _bits(w))               # the step did something


@pytest.mark.parametrize("n", [1, 5, 2 ** 20 + 3])
def test_swap_f32_exchanges_exactly(n):
    from basedet_amd import ops
    e, w, _, _ = _host(n)
    a, b = _dev(e), _dev(w)
    ops.swap_f32(a, b)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a), _bits(w)) and np.array_equal(_bits(b), _bits(e))


def test_bad_arguments_return_einval_and_launch_nothing():
    from basedet_amd import _lib
    lib = _lib.load()
    n = 64
    e, w, v, g = (_dev(a) for a in _host(n + 4))
    before = [t.clone() for t in (e, w, v, g)]
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off)         # noqa: E731
    null, st = C.c_void_p(0), _lib.stream_ptr()
    sgd = (0.01, 0.9, 1e-4, 0.5, 0.5, 0.5)
    calls = {
        "ema misaligned e": lambda: lib.bd_ema_update(P(e, 1), P(w), n, 0.5, 0.5, st),
        "ema misaligned w": lambda: lib.bd_ema_update(P(e), P(w, 1), n, 0.5, 0.5, st),
        "ema aliased": lambda: lib.bd_ema_update(P(e), P(e), n, 0.5, 0.5, st),
        "ema overlapping": lambda: lib.bd_ema_update(P(e), P(e, 4), n, 0.5, 0.5, st),
        "ema null e": lambda: lib.bd_ema_update(null, P(w), n, 0.5, 0.5, st),
        "ema null w": lambda: lib.bd_ema_update(P(e), null, n, 0.5, 0.5, st),
        "ema negative n": lambda: lib.bd_ema_update(P(e), P(w), -1, 0.5, 0.5, st),
        "fused misaligned e": lambda: lib.bd_sgd_momentum_ema_step(P(w), P(v), P(g), P(e, 1), n, *sgd, st),
        "fused misaligned w": lambda: lib.bd_sgd_momentum_ema_step(P(w, 1), P(v), P(g), P(e), n, *sgd, st),
        "fused aliased e/w": lambda: lib.bd_sgd_momentum_ema_step(P(w), P(v), P(g), P(w), n, *sgd, st),
        "fused overlapping e/w": lambda: lib.bd_sgd_momentum_ema_step(P(w), P(v), P(g), P(w, 4), n, *sgd, st),
        "fused null e": lambda: lib.bd_sgd_momentum_ema_step(P(w), P(v), P(g), null, n, *sgd, st),
        "fused null g": lambda: lib.bd_sgd_momentum_ema_step(P(w), P(v), null, P(e), n, *sgd, st),
        "swap misaligned": lambda: lib.bd_swap_f32(P(e, 1), P(w), n, st),
        "swap aliased": lambda: lib.bd_swap_f32(P(e), P(e), n, st),
        "swap overlapping": lambda: lib.bd_swap_f32(P(e), P(e, 4), n, st),
        "swap null": lambda: lib.bd_swap_f32(P(e), null, n, st),
    }
    for name, call in calls.items():
        assert call() == BD_EINVAL, name
        assert lib.bd_last_error_string(), name
    torch.cuda.synchronize()
    for t, b in zip((e, w, v, g), before):
        assert torch.equal(t, b)
    # n == 0 is a no-op that succeeds, whatever the pointers
    assert lib.bd_ema_update(null, null, 0, 0.5, 0.5, st) == 0
    assert lib.bd_sgd_momentum_ema_step(null, null, null, null, 0, *sgd, st) == 0
    assert lib.bd_swap_f32(null, null, 0, st) == 0


# ---- model level ------------------------------------------------------------------------------------------------------------------------
MOMENTUM, BURNIN, STEPS = 0.5, 3, 6


def _setup():
    """The smallest RetinaNet tests/test_model_gpu.py builds (R18, 2 x 128 x 160), with the prediction layers scaled as its inference
    test scales them so that scores straddle TEST.CLS_THRESHOLD and both models detect something."""
    from tests.test_model_gpu import _setup as base
    cfg, params, batch = base("resnet18", 2, (128, 160), seed=5)
    params["head.cls_score.bias"] = np.full_like(params["head.cls_score.bias"], -2.5)
    params["head.cls_score.weight"] = params["head.cls_score.weight"] * 8
    params["head.bbox_pred.weight"] = params["head.bbox_pred.weight"] * 8
    return cfg, params, batch


def _losses(d):
    return {k: float(v) for k, v in d.items()}


@pytest.fixture(scope="module")
def runs():
    """Run A: six DetTrainer.model_step calls with EMA on, arena.w cloned after each.  Run B, the twin: seven Solver.minimize steps
    with EMA off on the same parameters and batch."""
    from basedet_amd import ops
    from basedet_amd.engine import DetTrainer
    from basedet_amd.models import RetinaNet
    from basedet_amd.solver import DetSolver
    cfg, params, batch = _setup()
    out = dict(cfg=cfg, params=params, batch=batch)

    cfg_b, _, _ = _setup()
    mb = RetinaNet(cfg_b, params=params)
    sb = DetSolver.build(cfg_b, mb)
    out["b_losses"] = []
    for it in range(STEPS + 1):
        out["b_losses"].append(_losses(sb.minimize(mb, batch)))
        if it == STEPS - 1:
            out["b_w6"] = mb.arena.w.clone()
    torch.cuda.synchronize()

    cfg.TRAINER.EMA.merge(dict(ENABLE=True, MOMENTUM=MOMENTUM, BURNIN_ITER=BURNIN))
    ma = RetinaNet(cfg, params=params)
    sa = DetSolver.build(cfg, ma)
    tr = DetTrainer(cfg, ma, [], sa)
    counts = {"sgd_momentum_step": 0, "sgd_momentum_ema_step": 0, "ema_update": 0}
    orig = {k: getattr(ops, k) for k in counts}

    def counted(k):
        def f(*a, **kw):
            counts[k] += 1
            return orig[k](*a, **kw)
        return f

    for k in counts:
        setattr(ops, k, counted(k))
    try:
        out["w0"] = ma.arena.w.clone()
        out["e0"] = tr.ema.e.clone()
        out["a_losses"], out["w_after"] = [], []
        for _ in range(STEPS):
            out["a_losses"].append(_losses(tr.model_step(batch)))
            out["w_after"].append(ma.arena.w.clone())
        out["e6"] = tr.ema.e.clone()
        torch.cuda.synchronize()
    finally:
        for k in counts:
            setattr(ops, k, orig[k])
    out.update(model=ma, solver=sa, trainer=tr, ema=tr.ema, counts=dict(counts))
    return out


def test_model_ema_follows_the_reference_recurrence(runs):
    """ema.py:57-81 replayed in numpy fp32 over the weights after each step: nothing at iterations 1 and 2, update(0) + update(0.5) at 3,
    update(0.5) at 4 .. 6 -- of which the last three ran inside the SGD launch."""
    assert np.array_equal(_bits(runs["e0"]), _bits(runs["w0"]))
    e = runs["w0"].cpu().numpy().copy()
    for it, w in enumerate(runs["w_after"], start=1):
        w = w.cpu().numpy()
        if it < BURNIN:
            continue
        if it == BURNIN:
            e = _ema_ref(e, w, 0)
        e = _ema_ref(e, w, MOMENTUM)
    assert runs["counts"] == {"sgd_momentum_step": BURNIN, "sgd_momentum_ema_step": STEPS - BURNIN, "ema_update": 2}
    got = _bits(runs["e6"])
    diff = int((got != _bits(e)).sum())
    print(f"ema.e: {diff} of {e.size} elements differ from the replayed recurrence")
    assert diff == 0
    assert not np.array_equal(got, _bits(runs["w_after"][-1]))       # and it is an average, not the weights


def test_training_is_unchanged_by_ema(runs):
    """Losses of the six steps and the weights after them: the bits of the twin run with EMA off."""
    for it, (a, b) in enumerate(zip(runs["a_losses"], runs["b_losses"])):
        print(f"step {it + 1}: ema on {a}  ema off {b}")
    assert runs["a_losses"] == runs["b_losses"][:STEPS]
    assert np.array_equal(_bits(runs["w_after"][-1]), _bits(runs["b_w6"]))
    assert not np.array_equal(_bits(runs["w_after"][-1]), _bits(runs["w0"]))


def _detections(model, batch):
    outs = model({"data": batch["data"], "im_info": batch["im_info"]})
    torch.cuda.synchronize()
    return [(o["boxes"].cpu().numpy().copy(), o["box_scores"].cpu().numpy().copy(), o["box_labels"].cpu().numpy().copy()) for o in outs]


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for da, db in zip(a, b) for x, y in zip(da, db))


def test_state_dict_roundtrip(runs):
    from basedet_amd.layers import ModelEMA
    from basedet_amd.models import RetinaNet
    ema = runs["ema"]
    e_before = ema.e.clone()
    sd = ema.state_dict()
    assert np.array_equal(_bits(ema.e), _bits(e_before))             # reading the state leaves it alone
    own = runs["model"].state_dict()
    assert sd["iter"] == ema.iters and set(sd["model"]) == set(own)
    trainable = set(runs["model"].state_dict_trainable_names())
    for k, v in own.items():                                         # frozen entries: the model's own values
        if k not in trainable:
            assert np.array_equal(sd["model"][k], v), k
    assert any(not np.array_equal(sd["model"][k], own[k]) for k in trainable)
    other = RetinaNet(runs["cfg"], params=runs["params"])
    w_other = other.arena.w.clone()
    fresh = ModelEMA(other, momentum=0.25)
    fresh.load_state_dict(sd)
    torch.cuda.synchronize()
    assert fresh.iters == ema.iters
    assert np.array_equal(_bits(other.arena.w), _bits(w_other))      # the live weights of the receiving model are untouched
    for name, _, off, n in other.arena.entries:
        assert np.array_equal(_bits(fresh.e[off:off + n]), _bits(ema.e[off:off + n])), name
    fresh.load_state_dict({"model": sd["model"]})                    # ema.py:84-86: without "iter" the counter stays
    assert fresh.iters == ema.iters


def test_applied_evaluates_the_average_and_restores_training(runs):
    from basedet_amd.models import RetinaNet
    model, ema, batch = runs["model"], runs["ema"], runs["batch"]
    assert ema.iters == STEPS
    w_pre, e_pre = model.arena.w.clone(), ema.e.clone()
    packed = model.convs["head.cls_score"].w_fwd
    packed_pre = packed.clone()
    model.eval()
    live = _detections(model, batch)
    with ema.applied():
        assert np.array_equal(_bits(model.arena.w), _bits(e_pre))
        avg = _detections(model, batch)
    model.train()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(model.arena.w), _bits(w_pre)) and np.array_equal(_bits(ema.e), _bits(e_pre))
    assert torch.equal(packed, packed_pre)
    second = RetinaNet(runs["cfg"], params=ema.state_dict()["model"]).eval()
    ref = _detections(second, batch)
    print("detections per image: live", [len(d[1]) for d in live], "averaged", [len(d[1]) for d in avg])
    assert sum(len(d[1]) for d in avg) > 0
    assert _same(avg, ref)
    if _same(avg, live):                                             # vacuous at this size: then the weights themselves must differ
        i = [e[0] for e in model.arena.entries].index("head.cls_score.weight")
        _, _, off, n = model.arena.entries[i]
        assert not np.array_equal(_bits(w_pre[off:off + n]), _bits(e_pre[off:off + n]))
    # a seventh step continues the run as if nothing had happened
    seventh = _losses(runs["trainer"].model_step(batch))
    print("step 7: after applied()", seventh, " uninterrupted twin", runs["b_losses"][STEPS])
    assert seventh == runs["b_losses"][STEPS]


def test_applied_refuses_fp8_weights():
    from basedet_amd.layers import ModelEMA
    from basedet_amd.models import RetinaNet
    cfg, params, _ = _setup()
    cfg.MODEL.WEIGHT_DTYPE = "fp8_e4m3"
    model = RetinaNet(cfg, params=params)
    ema = ModelEMA(model, momentum=0.5)
    w = model.arena.w.clone()
    with pytest.raises(ValueError, match="WEIGHT_DTYPE"):
        with ema.applied():
            pass
    ema.update(0.5)                                                  # the fp32 masters are all update / step touch: any dtype
    torch.cuda.synchronize()
    assert torch.equal(model.arena.w, w)
