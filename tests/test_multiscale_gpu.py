"""Multi-scale training on the plan arena (FPNDetector: one device arena per model, every shape's per-step buffers carved from offset 0).

- memory bound: a model that stepped through six shapes holds at most 1.15 x what a fresh model that stepped through the largest one
  alone holds (per-shape constants are ~1 MB per shape at these sizes, <= 1 % of a batch-2 plan; the rest covers allocator rounding).
  With one full set of step buffers per shape this ratio is ~5.5.
- bit-identity across shape switches: losses, every parameter gradient and an interleaved inference() of a model that switches shapes
  equal those of fresh models that ran each step alone, for both orders (largest shape first: later shapes land on dirty memory;
  growing: the arena is replaced after shapes were bound).
- a recipe shape (2 x 736 x 1088: P5 23 x 34, P7 6 x 9) against the float oracle.
- fp8 (R101, stochastic rounding seeded per step: no bit-identity): finite losses and the memory bound over a shape sequence.

The loss values are compared too: the loss kernels of csrc/losses.hip sum their workgroups' partials in a fixed order (they used to add
them with a float atomicAdd, which made two fresh models running the same step differ by about one ulp)."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEM_SHAPES = [(512, 768), (576, 704), (640, 640), (704, 576), (768, 512), (544, 800)]     # similar areas, the largest last
MEM_BOUND = 1.15

# bit-identity shapes (H, W), multiples of 32: A and B have an odd P5 side (160 / 32 = 5), B is portrait, C is the largest
SHAPE_A, SHAPE_B, SHAPE_C, SHAPE_EVAL = (128, 160), (160, 96), (192, 224), (96, 128)
ORDERS = {"largest_first": [SHAPE_C, SHAPE_A, SHAPE_B, SHAPE_A], "growing": [SHAPE_A, SHAPE_B, SHAPE_C, SHAPE_A, SHAPE_B]}


def _cfg(kind, N, backbone=None):
    from basedet_amd import configs as C
    cfg = {"retinanet": C.RetinaNetConfig, "retinanet_deconv": C.RetinaNetConfig, "freeanchor": C.FreeAnchorConfig, "fcos": C.FCOSConfig,
           "atss": C.ATSSConfig, "ota": C.OTAConfig, "faster_rcnn": C.FasterRCNNConfig}[kind]()
    cfg.MODEL.BATCHSIZE = N
    if kind == "retinanet_deconv":
        cfg.MODEL.FPN.UPSAMPLE = "deconv"
    if backbone:
        cfg.MODEL.BACKBONE.NAME = backbone
    return cfg


def _params(kind, cfg):
    from basedet_amd.models import params as P
    if kind in ("fcos", "atss", "ota"):
        p = P.init_fcos_params(cfg, seed=0, residual_gamma=0.25)
        p["head.bbox_pred.bias"] = np.full_like(p["head.bbox_pred.bias"], 0.5)        # keep relu(bbox_pred * scale) alive
        return p
    if kind == "faster_rcnn":
        p = P.init_faster_rcnn_params(cfg, 0, residual_gamma=0.25)
        for k in ("rpn.rpn_cls_score.weight", "rpn.rpn_bbox_offsets.weight", "rcnn.pred_cls.weight", "rcnn.pred_delta.weight",
                  "rcnn.fc1.weight", "rcnn.fc2.weight", "rpn.rpn_conv.weight"):
            p[k] = (p[k] * 3).astype(np.float32)
        return p
    return P.init_retinanet_params(cfg, seed=0, residual_gamma=0.25)


def _model(kind, cfg, params):
    from basedet_amd import models as M
    cls = {"retinanet": M.RetinaNet, "retinanet_deconv": M.RetinaNet, "freeanchor": M.FreeAnchor, "fcos": M.FCOS, "atss": M.ATSS,
           "ota": M.OTA, "faster_rcnn": M.FasterRCNN}[kind]
    return cls(cfg, params=params)


def _batch(N, shape, seed):
    from basedet_amd.utils import DummyLoader
    b = next(DummyLoader(N, shape, seed=seed))
    b["data"] = (b["data"] * 255).astype(np.float32)
    return b


def _with_keys(model, batch, shape, seed):
    """Faster R-CNN: injected sampling keys (the same on every model that runs this step)."""
    N = batch["data"].shape[0]
    pl = model._plan(N, shape[0], shape[1])
    Gmax = batch["gt_boxes"].shape[1]
    rng = np.random.default_rng(seed)
    keys = dict(rpn_pos=rng.random((N, pl.A_total), dtype=np.float32), rpn_neg=rng.random((N, pl.A_total), dtype=np.float32),
                rcnn_fg=rng.random((N, pl.rois.shape[1] + Gmax), dtype=np.float32),
                rcnn_bg=rng.random((N, pl.rois.shape[1] + Gmax), dtype=np.float32))
    return dict(batch, sample_keys=keys)


def _step(model, kind, shape, N=2):
    seed = shape[0] * 1000 + shape[1]
    batch = _batch(N, shape, seed)
    if kind == "faster_rcnn":
        batch = _with_keys(model, batch, shape, seed + 1)
    out = model(batch)
    losses = {k: v.detach().clone().cpu() for k, v in out.items()}
    model.backward()
    torch.cuda.synchronize()
    return losses, model.reference_grads()


def _infer(model, shape):
    b = _batch(1, shape, 7)
    model.eval()
    out = model({"data": b["data"], "im_info": b["im_info"]})
    model.train()
    torch.cuda.synchronize()
    return {k: torch.as_tensor(v).detach().cpu().clone().as_subclass(torch.Tensor) for k, v in out.items()}


def _held_after(kind, cfg, params, shapes):
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    model = _model(kind, cfg, params)
    torch.cuda.synchronize()
    after_build = torch.cuda.memory_allocated()
    for s in shapes:
        out = model(_with_keys(model, _batch(2, s, 3), s, 4) if kind == "faster_rcnn" else _batch(2, s, 3))
        assert all(np.isfinite(float(v)) for v in out.values()), (kind, s, {k: float(v) for k, v in out.items()})
        model.backward()
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - after_build
    del model, out
    gc.collect()
    return held


@pytest.mark.parametrize("kind", ["retinanet", "fcos", "faster_rcnn"])
def test_multiscale_memory_bound(kind):
    """memory_allocated after the last of six shapes (largest last: the arena grows mid-sequence) minus its value after construction,
    against the same measurement for a fresh model that ran only the largest shape: <= 1.15 x."""
    cfg = _cfg(kind, 2)
    params = _params(kind, cfg)
    multi = _held_after(kind, cfg, params, MEM_SHAPES)
    single = _held_after(kind, cfg, params, MEM_SHAPES[-1:])
    ratio = multi / single
    print(f"[{kind}] held after six shapes {multi / 2**20:.1f} MiB, after the largest alone {single / 2**20:.1f} MiB: ratio {ratio:.4f}")
    assert ratio <= MEM_BOUND, (multi, single, ratio)


_REF = {}


def _reference(kind):
    """Per shape: the step of a fresh model with the same parameters (and the inference of a fresh eval model at SHAPE_EVAL)."""
    if kind not in _REF:
        cfg = _cfg(kind, 2)
        params = _params(kind, cfg)
        ref = {}
        for s in (SHAPE_A, SHAPE_B, SHAPE_C):
            m = _model(kind, cfg, params)
            ref[s] = _step(m, kind, s)
            del m
        m = _model(kind, cfg, params)
        ref["eval"] = _infer(m, SHAPE_EVAL)
        del m
        _REF.clear()
        _REF[kind] = (cfg, params, ref)
    return _REF[kind]


def _assert_equal(tag, got, want):
    assert sorted(got) == sorted(want), tag
    bad = [k for k in want if not torch.equal(got[k], want[k])]
    assert not bad, (tag, bad[:8], len(bad))


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("kind", ["retinanet", "freeanchor", "fcos", "atss", "ota", "faster_rcnn", "retinanet_deconv"])
def test_shape_switches_are_bit_identical(kind, order):
    """One model steps (forward + backward) through the shape sequence, with one inference at a fourth shape after the second step;
    every step's losses and reference_grads() and the inference outputs are torch.equal to a fresh model's.  RetinaNet runs with its
    default SPARSE_BOX_BWD (gradient-skipping box branch) on; retinanet_deconv has MODEL.FPN.UPSAMPLE = "deconv"."""
    cfg, params, ref = _reference(kind)
    if kind.startswith("retinanet"):
        assert cfg.MODEL.get("SPARSE_BOX_BWD", True)
    model = _model(kind, cfg, params)
    loss_steps = []
    for i, s in enumerate(ORDERS[order]):
        losses, grads = _step(model, kind, s)
        _assert_equal(f"{kind} {order} step {i} {s} grads", grads, ref[s][1])
        if i == 1:
            _assert_equal(f"{kind} {order} inference {SHAPE_EVAL}", _infer(model, SHAPE_EVAL), ref["eval"])
        loss_steps.append((f"{kind} {order} step {i} {s} losses", losses, ref[s][0]))
    assert model.arena_grows == (1 if order == "largest_first" else 2), model.arena_grows      # growing: once more when C arrives
    for tag, got, want in loss_steps:
        print(tag, {k: float(got[k] - want[k]) for k in want})
    for tag, got, want in loss_steps:
        _assert_equal(tag, got, want)


def test_reserve_grows_without_a_step():
    """model.reserve(N, H, W) sizes the arena for that shape: a later step at it and at every smaller shape grows nothing."""
    cfg = _cfg("retinanet", 2, "resnet18")
    cfg.MODEL.BACKBONE.OUT_FEATURE_CHANNELS = [128, 256, 512]
    cfg.MODEL.FPN.TOP_BLOCK_IN_CHANNELS = 512
    model = _model("retinanet", cfg, _params("retinanet", cfg))
    model.reserve(2, 250, 300)                   # padded 256 x 320
    grows, nbytes = model.arena_grows, model.arena_bytes
    assert grows == 1 and nbytes >= model.plan_bytes(model._plan(2, 256, 320))
    for s in ((256, 320), (128, 160), (160, 96)):
        _step(model, "retinanet", s)
    assert model.arena_grows == grows and model.arena_bytes == nbytes


def test_retinanet_r50_recipe_shape_matches_oracle():
    """One RetinaNet-R50 step at 2 x 736 x 1088 (a shape of the ShortestEdgeResize recipe: P5 23 x 34, P7 6 x 9 -- odd rows) against
    the float oracle, with the tolerances and helpers of the 800 x 1344 test."""
    from basedet_amd.models import RetinaNet, params as P
    from oracle.model import Oracle
    from tests.test_fullsize_parity_gpu import _check_forward_layers, _check_grads, _rel
    from tests.test_model_gpu import _setup
    N, size = 2, (736, 1088)
    cfg, params, batch = _setup("resnet50", N, size)
    model = RetinaNet(cfg, params=params)
    names = P.trainable_names(params, cfg.MODEL.BACKBONE.FREEZE_AT)
    orc = Oracle(params, P.oracle_arch(cfg), trainable=names)
    ref, aux = orc.retinanet_losses(batch)
    ref_grads = orc.grads(ref["total_loss"])
    out = model(batch)
    pl = model._cur
    assert pl.sizes[2] == (23, 34) and pl.sizes[4] == (6, 9)
    assert pl.labels.shape == (N, 9 * sum(h * w for h, w in pl.sizes))
    assert np.array_equal(pl.labels.cpu().numpy(), aux["labels"])
    assert int(pl.num_fg.item()) == aux["num_fg"]
    for k in ("cls_loss", "reg_loss", "total_loss"):
        got, want = float(out[k]), float(ref[k].detach())
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)
    K = cfg.DATA.NUM_CLASSES
    assert _rel(pl.logits.float().cpu().view(-1, K), aux["logits"].detach()) < 2e-2
    model.backward()
    torch.cuda.synchronize()
    got = model.reference_grads()
    acts = model.debug_activations()
    orc2 = Oracle(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=acts)
    l2, _ = orc2.retinanet_losses(batch)
    _check_grads(names, got, ref_grads, orc2.grads(l2["total_loss"]), "RetinaNet-R50 2x736x1088")
    _check_forward_layers(Oracle(params, P.oracle_arch(cfg), record={"_compare": acts}), batch, "retinanet_losses", "RetinaNet-R50 2x736x1088")


NORM_SEQ = [(128, 160), (96, 192), (128, 160)]       # A, B (landscape, another P5 side), A again: 2 x H x W each


def _normed_setup():
    """RetinaNet-R18 with live norms in backbone and FPN (FREEZE_AT = 0), every norm's parameters and running statistics randomised."""
    from backbone_norm_oracle import randomise_backbone_norms
    from fpn_norm_oracle import randomise_norms
    from tests.test_model_gpu import _setup
    over = dict(MODEL=dict(BACKBONE=dict(FREEZE_AT=0, NORM="BN"), FPN=dict(NORM="BN")))
    cfg, params, _ = _setup("resnet18", 2, NORM_SEQ[0], overrides=over)
    return cfg, randomise_backbone_norms(randomise_norms(params))


def _solver_step(model, solver, shape, seed):
    """One solver step; the losses as floats and clones of the gradients, the weights and the running statistics after it."""
    out = solver.minimize(model, _batch(2, shape, seed))
    torch.cuda.synchronize()
    return dict(losses={k: float(v) for k, v in out.items()}, g=model.arena.g.clone(), w=model.arena.w.clone(),
                running=model.norms.running.clone())


def test_live_norm_shape_switches_match_a_chain_of_single_shape_models():
    """A normalised model takes solver steps at A, B, A: each shape's plan has its own pre-norm tensors (pl.norm_y / pl.norm_gy) while the
    batch statistics, `sums` and the running statistics are the model's.  The chain: model 1 steps at A and hands its state_dict() and
    optimizer state to a fresh model 2, which steps at B, and so on -- every model sees one shape.  Losses, gradients, weights and
    norms.running after every step are equal bit for bit: a plan that read another plan's statistics or gate state would differ.  And
    the memory bound of this module for this config: the arena is what the larger of the two plans needs (rounded to 2 MiB, as
    PlanArena.grow rounds), which is the arena of the single-shape model of that shape."""
    from basedet_amd.models import RetinaNet
    from basedet_amd.solver import DetSolver
    from util import bits_of
    cfg, params = _normed_setup()
    multi = RetinaNet(cfg, params=params)
    assert len(multi.norms) > 20
    solver = DetSolver.build(cfg, multi)
    got = [_solver_step(multi, solver, s, 50 + i) for i, s in enumerate(NORM_SEQ)]
    assert len({id(multi._plan(2, *s)) for s in NORM_SEQ}) == 2
    want, single_arena, state, opt = [], [], params, None
    for i, s in enumerate(NORM_SEQ):
        m = RetinaNet(cfg, params=state)
        sv = DetSolver.build(cfg, m)
        if opt is not None:
            sv.optimizer.load_state_dict(opt)
        want.append(_solver_step(m, sv, s, 50 + i))
        assert len(m._plans) == 1
        single_arena.append(m.arena_bytes)
        state, opt = m.state_dict(), sv.optimizer.state_dict()
        del m, sv
    for i, (a, b) in enumerate(zip(got, want)):
        print(f"step {i} {NORM_SEQ[i]}: multi {a['losses']}  chain {b['losses']}")
        assert a["losses"] == b["losses"], i
        for k in ("g", "w", "running"):
            assert torch.equal(bits_of(a[k]), bits_of(b[k])), (i, k, int((bits_of(a[k]) != bits_of(b[k])).sum()))
    for k in ("w", "running"):                                       # every step moved the weights and the running statistics
        assert not torch.equal(got[0][k], got[1][k]) and not torch.equal(got[1][k], got[2][k])
    plans = [multi.plan_bytes(multi._plan(2, *s)) for s in NORM_SEQ[:2]]
    print(f"plan bytes A {plans[0]}, B {plans[1]}; arena {multi.arena_bytes}; single-shape arenas {single_arena}")
    assert multi.arena_bytes == -(-max(plans) // (2 << 20)) * (2 << 20)
    assert multi.arena_bytes == max(single_arena)


def test_fp8_r101_shape_sequence():
    """R101 with the fp8 defaults over [C, A, B, A] at batch 2: finite losses, and held memory <= 1.15 x that of a fresh fp8 model that
    ran only C (no bit-identity: the e5m2 stochastic rounding is seeded per step)."""
    from basedet_amd.configs import RetinaNetConfig
    from basedet_amd.models import params as P
    cfg = RetinaNetConfig()
    cfg.MODEL.BATCHSIZE = 2
    cfg.MODEL.BACKBONE.NAME = "resnet101"
    cfg.MODEL.WEIGHT_DTYPE = "fp8_e4m3"
    params = P.init_retinanet_params(cfg, seed=0, residual_gamma=0.2)
    seq = ORDERS["largest_first"]
    multi = _held_after("retinanet", cfg, params, seq)
    single = _held_after("retinanet", cfg, params, seq[:1])
    ratio = multi / single
    print(f"[fp8 R101] held after {seq}: {multi / 2**20:.1f} MiB, after {seq[0]} alone {single / 2**20:.1f} MiB: ratio {ratio:.4f}")
    assert ratio <= MEM_BOUND, (multi, single, ratio)
