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


# ---- a model with live batch norms ------------------------------------------------------------------------------------------------------
# RetinaNet-R18, FREEZE_AT = 0, MODEL.BACKBONE.NORM = MODEL.FPN.NORM = "BN": every norm's running_mean / running_var is a buffer that
# moves with each training forward, outside the parameter arena.  ema.py:52-55 averages buffers like parameters.
N_MOMENTUM, N_BURNIN, N_STEPS = 0.5, 1, 3        # burn-in at the first step: update(0) + update(0.5) there, update(0.5) at steps 2 and 3
N_UPDATES = N_STEPS + 1
SIZE = (128, 160)


def _is_stat(k):
    return k.endswith((".running_mean", ".running_var"))


def _stats(sd):
    return {k: np.array(v, np.float32) for k, v in sd.items() if _is_stat(k)}


def _norm_setup():
    """cfg, params (gamma / beta / running statistics of every norm randomised: ignoring any of them moves the result) and three
    different batches; the second one's pixels are scaled by 0.6 so that its batch statistics stand apart from the others'."""
    from backbone_norm_oracle import randomise_backbone_norms
    from fpn_norm_oracle import randomise_norms
    from basedet_amd.utils import DummyLoader
    from tests.test_model_gpu import _setup as base
    over = dict(MODEL=dict(BACKBONE=dict(FREEZE_AT=0, NORM="BN"), FPN=dict(NORM="BN")))
    cfg, params, _ = base("resnet18", 2, SIZE, seed=5, overrides=over)
    params = randomise_backbone_norms(randomise_norms(params))
    params["head.cls_score.bias"] = np.full_like(params["head.cls_score.bias"], -2.5)
    params["head.cls_score.weight"] = params["head.cls_score.weight"] * 8
    batches = []
    for i, scale in enumerate((255.0, 0.6 * 255.0, 255.0)):
        b = next(DummyLoader(2, SIZE, seed=20 + i))
        b["data"] = (b["data"] * scale).astype(np.float32)
        batches.append(b)
    return cfg, params, batches


def _norm_run(cfg, params, batches, fused):
    """Three solver steps with a ModelEMA next to them.  fused: SGD.step(ema=...) folds the arena's update into its launch past the
    burn-in (what DetTrainer.model_step does); otherwise ema.step() runs its own launches."""
    from basedet_amd.layers import ModelEMA
    from basedet_amd.models import RetinaNet
    from basedet_amd.solver import DetSolver
    model = RetinaNet(cfg, params=params)
    solver = DetSolver.build(cfg, model)
    ema = ModelEMA(model, N_MOMENTUM, burnin_iter=N_BURNIN)
    run = dict(model=model, solver=solver, ema=ema, x0=_stats(model.state_dict()), x=[], losses=[])
    for b in batches:
        out = solver.minimize(model, b, ema=ema) if fused else solver.minimize(model, b)
        ema.step()
        torch.cuda.synchronize()
        run["losses"].append(_losses(out))
        run["x"].append(_stats(model.state_dict()))
    run["sd"] = ema.state_dict()
    return run


@pytest.fixture(scope="module")
def norm_runs():
    cfg, params, batches = _norm_setup()
    return dict(cfg=cfg, params=params, batches=batches, fused=_norm_run(cfg, params, batches, True),
                plain=_norm_run(cfg, params, batches, False))


def _eval_logits(model, batch):
    """The logits of inference_batch on `batch`, in whatever mode-independent state the caller arranged; the model must be in eval()."""
    assert not model.training
    model.inference_batch({"data": batch["data"], "im_info": batch["im_info"]})
    torch.cuda.synchronize()
    return model._plan(batch["data"].shape[0], *SIZE).logits.clone()


def _same_bits(a, b):
    from util import bits_of
    return a.shape == b.shape and bool(torch.equal(bits_of(a), bits_of(b)))


def test_live_norm_buffers_follow_the_float64_recurrence(norm_runs):
    """Every running_mean / running_var of ema.state_dict()["model"] against e = m e + (1 - m) x in float64 over the model's buffers
    recorded after each step, started from the buffers at construction, with the update(0) of the burn-in step (ema.py:57-69).

    Bound: one update is two fp32 products and one fp32 sum, three roundings of at most 2^-24 relative each on values no larger than
    max(|e|, |x|); after k = 4 updates that is 3 k 2^-24 max(|e|, |x|) -- asserted at 4 times that (the order of the roundings).  First
    the fixture: the float64 average must stand more than 1e-2 (rel-L2, from the recorded values alone) away from the model's current
    buffers, or the raw statistics would pass as the average."""
    run = norm_runs["fused"]
    got = _stats(run["sd"]["model"])
    names = sorted(run["x0"])
    assert names and sorted(got) == names and len(names) == 2 * len(run["model"].norms)
    e = {k: run["x0"][k].astype(np.float64) for k in names}
    scale = {k: np.abs(e[k]) for k in names}
    updates = 0
    for it, x in enumerate(run["x"], start=1):
        for m in ([0.0, N_MOMENTUM] if it == N_BURNIN else [N_MOMENTUM]):
            for k in names:
                xk = x[k].astype(np.float64)
                scale[k] = np.maximum(scale[k], np.maximum(np.abs(e[k]), np.abs(xk)))
                e[k] = m * e[k] + (1 - m) * xk
            updates += 1
    assert updates == N_UPDATES
    last = run["x"][-1]
    for kind in (".running_mean", ".running_var"):
        ks = [k for k in names if k.endswith(kind)]
        a, b = np.concatenate([e[k] for k in ks]), np.concatenate([last[k].astype(np.float64) for k in ks])
        away = float(np.linalg.norm(a - b) / np.linalg.norm(b))
        print(f"{kind}: float64 average vs the model's current buffers, rel-L2 {away:.3e}")
        assert away > 1e-2, (kind, away)
    bound = 4 * 3 * N_UPDATES * 2.0 ** -24
    worst, raw = ("", 0.0), 0
    for k in names:
        err = np.abs(got[k].astype(np.float64) - e[k]) / np.maximum(scale[k], 1e-300)
        if float(err.max()) > worst[1]:
            worst = (k, float(err.max()))
        raw += int(np.array_equal(got[k], last[k]))
    print(f"worst |ema - float64| / max(|e|, |x|) = {worst[1]:.3e} at {worst[0]} (bound {bound:.3e}); "
          f"{raw} of {len(names)} entries equal the model's own buffers")
    for k in names:
        assert np.all(np.abs(got[k].astype(np.float64) - e[k]) <= bound * scale[k]), k


def test_live_norm_fused_and_plain_updates_agree(norm_runs):
    """SGD.step(ema=...) + ema.step() against ema.step() on its own launches: the same training (losses, weights, buffers) and the same
    average, parameters and buffers, bit for bit."""
    f, p = norm_runs["fused"], norm_runs["plain"]
    assert f["losses"] == p["losses"]
    assert _same_bits(f["model"].arena.w, p["model"].arena.w) and _same_bits(f["model"].norms.running, p["model"].norms.running)
    assert f["sd"]["iter"] == p["sd"]["iter"] == N_STEPS and sorted(f["sd"]["model"]) == sorted(p["sd"]["model"])
    bad = [k for k, v in f["sd"]["model"].items() if not np.array_equal(_bits(v), _bits(p["sd"]["model"][k]))]
    assert not bad, bad[:8]
    assert any(_is_stat(k) for k in f["sd"]["model"])


@pytest.mark.parametrize("order", ["eval_inside", "eval_before"])
def test_live_norm_applied_is_the_averaged_model(norm_runs, order):
    """Eval logits inside applied() against those of a fresh model built from ema.state_dict()["model"]: the same weights through the
    same kernels, so anything but equal bits is a stale fold or a stale packed weight.  eval() is entered inside the block (the fold is
    made from what is in place) or before it (the repack on entry refolds).  The averaged buffers take part: the fresh model with the
    live model's own running statistics in their place computes other logits."""
    from basedet_amd.models import RetinaNet
    run, batch = norm_runs["fused"], norm_runs["batches"][0]
    model, ema = run["model"], run["ema"]
    w_pre, r_pre = model.arena.w.clone(), model.norms.running.clone()
    if order == "eval_before":
        model.eval()
    with ema.applied():
        model.eval()
        got = _eval_logits(model, batch)
    live = _eval_logits(model, batch)                                # after the exit, still in eval(): the live model again
    model.train()
    torch.cuda.synchronize()
    assert _same_bits(model.arena.w, w_pre) and _same_bits(model.norms.running, r_pre)
    sd = ema.state_dict()["model"]
    want = _eval_logits(RetinaNet(norm_runs["cfg"], params=sd).eval(), batch)
    assert bool(torch.isfinite(want.float()).all())
    assert _same_bits(got, want)
    own = RetinaNet(norm_runs["cfg"], params=model.state_dict()).eval()
    assert _same_bits(live, _eval_logits(own, batch))                # the fold on exit is the live model's
    assert not _same_bits(live, got)
    mixed = dict(sd)
    mixed.update(_stats(model.state_dict()))                         # averaged weights through the raw statistics of the last step
    assert not _same_bits(_eval_logits(RetinaNet(norm_runs["cfg"], params=mixed).eval(), batch), want)


def test_live_norm_applied_leaves_training_untouched(norm_runs):
    """One model evaluates through applied(), its twin (the same three steps, never inside applied()) does not: a fourth step on each
    gives the same losses, gradients, weights, running statistics and averages, bit for bit."""
    f, p, batch = norm_runs["fused"], norm_runs["plain"], norm_runs["batches"][1]
    with f["ema"].applied():
        f["model"].eval()
        _eval_logits(f["model"], batch)
    f["model"].train()
    outs = []
    for run in (f, p):
        model = run["model"]
        losses = _losses(run["solver"].minimize(model, batch, ema=run["ema"]))
        run["ema"].step()
        torch.cuda.synchronize()
        outs.append((losses, model.arena.g.clone(), model.arena.w.clone(), model.norms.running.clone(), run["ema"].state_dict()))
    (la, ga, wa, ra, sa), (lb, gb, wb, rb, sb) = outs
    print("step 4: after applied()", la, " twin", lb)
    assert la == lb
    assert _same_bits(ga, gb) and _same_bits(wa, wb) and _same_bits(ra, rb)
    assert sa["iter"] == sb["iter"]
    bad = [k for k, v in sa["model"].items() if not np.array_equal(_bits(v), _bits(sb["model"][k]))]
    assert not bad, bad[:8]


def test_live_norm_state_dict_roundtrip(norm_runs):
    """ema2.load_state_dict(ema.state_dict()) on a second model (the initial parameters): the averaged parameters and buffers and the
    eval logits under applied() come back bit for bit; the receiving model's own weights and buffers are untouched."""
    from basedet_amd.layers import ModelEMA
    from basedet_amd.models import RetinaNet
    run, batch = norm_runs["fused"], norm_runs["batches"][2]
    ema = run["ema"]
    sd = ema.state_dict()
    other = RetinaNet(norm_runs["cfg"], params=norm_runs["params"])
    w_other, r_other = other.arena.w.clone(), other.norms.running.clone()
    ema2 = ModelEMA(other, momentum=0.25)
    ema2.load_state_dict(sd)
    torch.cuda.synchronize()
    assert ema2.iters == ema.iters
    assert _same_bits(other.arena.w, w_other) and _same_bits(other.norms.running, r_other)
    sd2 = ema2.state_dict()["model"]
    assert sorted(sd2) == sorted(sd["model"])
    stats = [k for k in sd2 if _is_stat(k)]
    assert len(stats) == 2 * len(other.norms)
    bad = [k for k in stats if not np.array_equal(_bits(sd2[k]), _bits(sd["model"][k]))]
    assert not bad, ("buffers", bad[:8], len(bad))
    bad = [k for k in other.state_dict_trainable_names() if not np.array_equal(_bits(sd2[k]), _bits(sd["model"][k]))]
    assert not bad, ("parameters", bad[:8], len(bad))
    assert any(not np.array_equal(sd2[k], v) for k, v in _stats(other.state_dict()).items())      # and they are not the receiver's own
    logits = []
    for m, e in ((run["model"], ema), (other, ema2)):
        with e.applied():
            m.eval()
            logits.append(_eval_logits(m, batch))
        m.train()
    assert _same_bits(logits[0], logits[1])
