"""The YOLOX detector on the device: the layers' adopt(), the model class against the stand-alone layers it is made of, YOLOXSolver against
the optimizer launch it slices, a short training run, inference against yolox_inference, the EMA swap and the gradient bucket.

No path here uses fp32 atomics (every forward output and everything the backward writes is bitwise reproducible), so a
stand-alone layer and its adopted twin, and the model and the stand-alone network step, are compared with torch.equal throughout: they
are the same kernels in the same order on other storage.  Sizes: DEPTH_FACTOR 0.33, WIDTH_FACTOR 0.25 (the narrowest width that keeps every
channel count a multiple of 8), 3 and 80 classes, N = 2, 64 x 64 and 96 x 64 inputs."""
import numpy as np
import pytest
import torch

import util

pytestmark = pytest.mark.gpu

DEPTH, WIDTH, N = 0.33, 0.25, 2
IN_CH, MID = (64, 128, 256), 64


def _cfg(K=3, size=(64, 64)):
    from basedet_amd.configs import YOLOXConfig
    cfg = YOLOXConfig()
    cfg.MODEL.DEPTH_FACTOR, cfg.MODEL.WIDTH_FACTOR, cfg.MODEL.BATCHSIZE = DEPTH, WIDTH, N
    cfg.DATA.NUM_CLASSES = K
    cfg.AUG.TRAIN_SETTING.INPUT_SIZE = tuple(size)
    return cfg


def _batch(H, W, K, seed=0, n=N):
    """A loader batch on the device: fp32 (n, 3, H, W) in [0, 255], three gts per image, im_info rows (H, W, H, W, num_gt)."""
    rng = np.random.default_rng(seed)
    data = torch.from_numpy(rng.uniform(0, 255, (n, 3, H, W)).astype(np.float32)).cuda()
    gt = np.zeros((n, 4, 5), np.float32)          # (one padding slot behind the three boxes)
    for i in range(n):
        for j in range(3):
            cx, cy, w, h = rng.uniform(16, W - 16), rng.uniform(16, H - 16), rng.uniform(12, 30), rng.uniform(12, 30)
            gt[i, j] = [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, 1 + (i + j) % K]
    info = torch.tensor([[H, W, H, W, 3]] * n, dtype=torch.float32)
    return {"data": data, "gt_boxes": torch.from_numpy(gt).cuda(), "im_info": info.cuda()}


def _standalone(K, state):
    """layers.YOLOPAFPN + layers.YOLOXHead loaded with the model's state."""
    import basedet.layers as BL
    fpn = BL.YOLOPAFPN(BL.CSPDarknet(DEPTH, WIDTH, seed=11), DEPTH, WIDTH, seed=12)
    head = BL.YOLOXHead(num_classes=K, in_channels=IN_CH, mid_channels=MID, seed=13)
    fpn.load_state_dict({k[len("backbone."):]: v for k, v in state.items() if k.startswith("backbone.")})
    head.load_state_dict({k[len("head."):]: v for k, v in state.items() if k.startswith("head.")})
    return fpn, head


def _same(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        assert torch.equal(torch.as_tensor(a[k]).cpu(), torch.as_tensor(b[k]).cpu()), f"{what}: {k}"


# ---- adopt(): a stand-alone layer and its twin on caller-provided storage ---------------------------------------------------------------------
def _adopt(layer):
    """Move `layer` onto flat storage like a model's arena; returns (w_flat, g_flat)."""
    shapes = layer.arena_shapes()
    w_flat, g_flat, w, g = util.flat_storage(shapes)
    if hasattr(layer, "_leaves"):
        layer.adopt(w, g, {n + ".norm": util.norm_record(c.cout) for n, c in layer._leaves() if c.NORMS})
    else:
        layer.adopt(w, g, util.norm_record(layer.cout))
    return w_flat, g_flat


def _layer_cases():
    import basedet.layers as BL
    from basedet_amd.layers.yolox_head import ConvBNSiLU
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    feats = [r(N, c, 64 // s, 96 // s) for c, s in zip((32, 64, 128), (8, 16, 32))]
    return {
        "ConvBNSiLU": (lambda: ConvBNSiLU(16, 24, 3, 2, seed=1), r(N, 16, 9, 11), lambda y: 0.1 * torch.randn_like(y)),
        "Focus": (lambda: BL.Focus(3, 16, 3, seed=2), r(N, 3, 16, 20), lambda y: 0.1 * torch.randn_like(y)),
        "CSPLayer": (lambda: BL.CSPLayer(16, 16, 2, seed=3), r(N, 16, 7, 9), lambda y: 0.1 * torch.randn_like(y)),
        "YOLOPAFPN": (lambda: BL.YOLOPAFPN(BL.CSPDarknet(DEPTH, 0.125, seed=4), DEPTH, 0.125, seed=5), r(N, 3, 64, 96),
                      lambda y: [0.1 * torch.randn_like(t) for t in y]),
        "YOLOXHead": (lambda: BL.YOLOXHead(num_classes=3, in_channels=(32, 64, 128), mid_channels=32, seed=6), feats,
                      lambda y: [[0.1 * torch.randn_like(t) for t in lst] for lst in y]),
    }


@pytest.mark.parametrize("name", ["ConvBNSiLU", "Focus", "CSPLayer", "YOLOPAFPN", "YOLOXHead"])
def test_adopted_twin_equals_the_standalone_layer(name):
    make, x, grad_of = _layer_cases()[name]
    a, b = make(), make()
    state = {k: v + 0.01 for k, v in a.state_dict().items()}          # not the constructor's values: the load has to carry them
    state = {k: (v.abs() + 0.5 if k.endswith("running_var") else v) for k, v in state.items()}
    a.load_state_dict(state)
    w_flat, g_flat = _adopt(b)
    ptrs = {k: v.data_ptr() for k, v in b.params().items()}
    b.load_state_dict(state)          # copies in place: the masters stay where adopt() put them
    after = b.params()
    assert {k: v.data_ptr() for k, v in after.items()} == ptrs
    assert all(util.lies_inside(v, w_flat) for k, v in after.items() if "norm." not in k)
    _same(a.state_dict(), b.state_dict(), "state after load")
    ya, yb = a(x), b(x)
    torch.manual_seed(0)
    dy = grad_of(ya)
    da = a.backward(*dy) if name == "YOLOXHead" else a.backward(dy)
    db = b.backward(*dy) if name == "YOLOXHead" else b.backward(dy)
    flat = lambda t: [] if t is None else [t] if torch.is_tensor(t) else [u for v in t for u in flat(v)]
    for u, v in zip(flat(ya) + flat(da), flat(yb) + flat(db)):
        assert torch.equal(u, v)
    assert len(flat(ya)) == len(flat(yb)) and len(flat(da)) == len(flat(db))
    _same(a.grads(), b.grads(), "grads")
    _same(a.state_dict(), b.state_dict(), "running statistics after the step")
    # the adopted layer's weight gradients were written into the caller's storage (it started at NaN)
    assert bool(torch.isfinite(g_flat).any()) and not bool(torch.isnan(b.grads()[next(iter(b.grads()))]).any())


# ---- the model against the stand-alone network step --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model3():
    from basedet_amd.models import YOLOX
    return YOLOX(_cfg(3))


@pytest.mark.parametrize("K,size,target", [(3, (64, 64), (64, 64)), (80, (96, 64), (96, 64)), (3, (64, 64), (96, 64)), (80, (96, 64), (64, 64))],
                         ids=["K3-64x64", "K80-96x64", "K3-64x64-to-96x64", "K80-96x64-to-64x64"])
def test_training_step_equals_network_step(K, size, target, model3):
    from basedet_amd import ops
    from basedet_amd.models import YOLOX
    from basedet_amd.models.yolox import yolox_network_step
    model = model3 if K == 3 else YOLOX(_cfg(K, target))
    model.train()
    model.target_size = target
    fpn, head = _standalone(K, model.state_dict())
    batch = _batch(*size, K, seed=K + size[0])
    before = {k: v.clone() for k, v in batch.items()}
    losses = model(batch)
    model.backward()
    _same(batch, before, "the caller's batch")
    (H, W), (h, w) = size, target
    halo = torch.empty((N, h + 6, w + 8, 4), dtype=torch.bfloat16, device="cuda")
    gt = batch["gt_boxes"].clone()
    if size == target:
        ops.pad_normalize(batch["data"], h, w, (0, 0, 0), (1, 1, 1), halo)
    else:
        ops.resize_bilinear_normalize(batch["data"], h, w, h, w, (0, 0, 0), (1, 1, 1), halo)
        gt[..., 0:4:2] *= w / W
        gt[..., 1:4:2] *= h / H
    assert torch.equal(model._cur["x_halo"], halo) and torch.equal(model._cur["gt_boxes"], gt)
    num_gt = batch["im_info"][:, -1].to(torch.int32)
    parts, assigned = yolox_network_step(fpn, head, halo, N, h, w, gt, num_gt, (8, 16, 32), False)
    assert torch.equal(model._cur["parts"], parts) and float(assigned[2]) > 0
    assert all(torch.equal(a, b) for a, b in zip(model._cur["assigned"], assigned))
    want = {"total_loss": parts.sum(), "iou_loss": parts[0], "obj_loss": parts[1], "cls_loss": parts[2], "l1_loss": parts[3]}
    assert set(losses) == set(want) and all(torch.equal(losses[k], want[k]) for k in want)
    ref = {"backbone." + k: v for k, v in fpn.grads().items()}
    ref.update({"head." + k: v for k, v in head.grads().items()})
    _same(model.reference_grads(), ref, "gradients")
    assert list(ref) == model.reference_grads_names()
    st = model.state_dict()
    _same({k: st[k] for k in st if "running_" in k},
          {**{"backbone." + k: v for k, v in fpn.state_dict().items() if "running_" in k},
           **{"head." + k: v for k, v in head.state_dict().items() if "running_" in k}}, "running statistics")


def test_arena_layout_state_round_trip_and_names(model3):
    m = model3
    a = m.arena
    assert m.decay_end % 64 == 0 and 0 < m.decay_end < a.total
    for name, shape, off, n in a.entries:
        assert off % 64 == 0
        assert (len(shape) == 4 and off + n <= m.decay_end) or (len(shape) == 1 and off >= m.decay_end), name
    first_1d = [e[0] for e in a.entries if len(e[1]) == 1]
    assert first_1d[0] == "backbone.backbone.stem.conv.norm.weight" and first_1d[-1].endswith(".bias") and "preds" in first_1d[-1]
    assert [e[0] for e in a.entries][0] == "backbone.backbone.stem.conv.weight"
    orig = m.state_dict()
    g = torch.Generator().manual_seed(1)
    st = {k: (torch.rand(v.shape, generator=g) + 0.5).numpy() for k, v in m.state_dict().items()}
    w_ptr, ptrs = a.w.data_ptr(), [c._store.w["weight"].data_ptr() for _, c in m._norm_layers()]
    m.load_state_dict(st)
    assert a.w.data_ptr() == w_ptr and [c._store.w["weight"].data_ptr() for _, c in m._norm_layers()] == ptrs
    assert all(util.lies_inside(c._store.w["weight"], a.w) and util.lies_inside(c.norm.p["weight"], a.w) for _, c in m._norm_layers())
    assert all(util.lies_inside(p._store.w["weight"], a.w) and util.lies_inside(p._store.w["bias"], a.w)
               and util.lies_inside(p._store.g["weight"], a.g) for p in m.head.cls_preds + m.head.regobj_preds)
    assert all(util.lies_inside(c.norm.p["running_var"], m.norms.running) for _, c in m._norm_layers())
    back = m.state_dict()
    assert list(back) == list(st) and all(np.array_equal(back[k], st[k]) for k in st)
    from basedet_amd.models import YOLOX
    assert {k: tuple(v.shape) for k, v in back.items()} == YOLOX.param_shapes(m.cfg)
    names = [k for k in st if "running_" not in k]
    assert m.reference_grads_names() == names == m.state_dict_trainable_names()
    # the pad rows of the padded predictors and Focus's pad columns came back as zeros
    assert int(util.bits_of(m.head.cls_preds[0]._store.w["weight"][3:]).abs().max()) == 0 and int(util.bits_of(m.head.regobj_preds[0]._store.w["bias"][5:]).abs().max()) == 0
    assert int(util.bits_of(m.backbone.backbone.stem.conv._store.w["weight"][..., 12:]).abs().max()) == 0
    with pytest.raises(KeyError):
        m._bind_params({k: v for k, v in st.items() if k != "head.stems.0.weight"})
    m.load_state_dict(orig)          # (the module's model goes on to the other tests with the weights it was built with)


# ---- the solver ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
def test_solver_step_decays_the_convolution_weights_only(with_ema):
    from basedet_amd import ops
    from basedet_amd.layers.ema import ModelEMA
    from basedet_amd.models import YOLOX
    from basedet_amd.utils.registry import registers
    cfg = _cfg(3)
    m = YOLOX(cfg)
    solver = registers.solvers.get("YOLOXSolver").build(cfg, m)
    opt, a, cut = solver.optimizer, m.arena, m.decay_end
    assert len(opt.param_groups) == 2 and opt.param_groups[0]["weight_decay"] == cfg.SOLVER.WEIGHT_DECAY and opt.param_groups[1]["weight_decay"] == 0
    lr, mom, wd = cfg.SOLVER.BASIC_LR * N, cfg.SOLVER.MOMENTUM, cfg.SOLVER.WEIGHT_DECAY
    assert opt.param_groups[0]["lr"] == opt.param_groups[1]["lr"] == lr and opt.nesterov
    g = torch.Generator(device="cuda").manual_seed(5)
    a.g.copy_(torch.randn(a.total, generator=g, device="cuda"))
    a.v.copy_(torch.randn(a.total, generator=g, device="cuda"))
    rec = next(iter(m.norms))          # a norm gamma of 1 with zero gradient and zero momentum: any decay would move it
    assert bool((rec.gamma == 1).all())
    rec.g_gamma.zero_()
    off = [e[2] for e in a.entries if e[0] == rec.name + ".weight"][0]
    a.v[off:off + rec.C].zero_()
    ema = ModelEMA(m, 0.9, burnin_iter=0) if with_ema else None
    if ema is not None:
        ema.e.mul_(0.5)
    w, v, e = a.w.clone(), a.v.clone(), (ema.e.clone() if ema is not None else None)
    w0, v0 = w.clone(), v.clone()
    for lo, hi, decay in ((0, cut, wd), (cut, a.total, 0.0)):
        sl = [t[lo:hi].clone() for t in (w, v, a.g)]          # the launch on copies of the slices
        if ema is None:
            ops.sgd_nesterov_step(*sl, lr, mom, decay, 1.0)
        else:
            es = e[lo:hi].clone()
            ops.sgd_nesterov_ema_step(*sl, es, lr, mom, decay, 1.0, 0.9)
            e[lo:hi] = es
        w[lo:hi], v[lo:hi] = sl[0], sl[1]
    opt.step(ema=ema) if ema is not None else opt.step()
    assert torch.equal(a.w[:cut], w[:cut]) and torch.equal(a.w[cut:], w[cut:]) and torch.equal(a.v, v)
    assert bool((rec.gamma == 1).all())
    if ema is not None:
        assert torch.equal(ema.e, e) and ema._fused
    # the decay did reach the weights: the same launch without it gives other bits there
    sl = [t[:cut].clone() for t in (w0, v0, a.g)]
    ops.sgd_nesterov_step(*sl, lr, mom, 0.0, 1.0)
    assert not torch.equal(a.w[:cut], sl[0])
    sd = opt.state_dict()
    assert sd["step"] == 1 and set(sd["momentum_buffer"]) == set(m.state_dict_trainable_names())


class _StubComm:
    """A one-rank communicator that reduces nothing: records what GradBuckets hands it."""
    world, rank, stream = 1, 0, None

    def __init__(self):
        self.calls = []

    def allreduce_async(self, t, producers, op="sum"):
        self.calls.append((t.data_ptr(), t.numel(), op))

    def wait(self, stream=None):
        self.calls.append("wait")


def test_training_run_descends_through_a_size_change_and_the_all_bucket():
    """Twenty Solver.minimize steps at lr 0.01 on one fixed 64 x 64 batch; target_size goes from 64 to 96 at step 10.  The gradient
    bucket "all" goes through GradBuckets with a recording one-rank communicator (the RCCL one needs an env:// store of its own
    process: tests/test_dist_gpu.py starts those; the bucket's RCCL leg is not run here)."""
    from basedet_amd.models import YOLOX
    from basedet_amd.solver import GradBuckets, YOLOXSolver
    cfg = _cfg(3)
    m = YOLOX(cfg, seed=1)
    m.use_l1 = True
    solver = YOLOXSolver.build(cfg, m)
    comm = _StubComm()
    solver.buckets = GradBuckets(m, "MEAN", comm=comm)
    assert solver.buckets.ranges == {"all": (0, m.arena.total)}
    for g in solver.optimizer.param_groups:
        g["lr"] = 0.01
    batch = _batch(64, 64, 3, seed=2)
    losses = []
    for step in range(20):
        if step == 10:
            m.target_size = (96, 96)
        out = solver.minimize(m, batch)
        losses.append(float(out["total_loss"]))
        assert bool(torch.isfinite(m.arena.g).all()) and bool(torch.isfinite(m.arena.w).all())
    print("total loss, step 1 .. 20:", " ".join(f"{v:.4f}" for v in losses))
    assert comm.calls == [(m.arena.g.data_ptr(), m.arena.total, "sum"), "wait"] * 20
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert m._cur["H"] == 96 and (N, 64, 64) in m._halo and (N, 96, 96) in m._halo
    assert int(util.bits_of(m.backbone.backbone.stem.conv._store.w["weight"][..., 12:]).abs().max()) == 0          # Focus's pad columns stayed zero
    assert int(util.bits_of(m.head.cls_preds[0]._store.w["weight"][3:]).abs().max()) == 0


# ---- inference -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_inference_batch_equals_yolox_inference(B, model3):
    from basedet_amd.models.yolox import _unpack, yolox_inference
    m = model3
    m.train()
    x = _batch(64, 96, 3, seed=B, n=B)["data"]
    with pytest.raises(AssertionError):
        m.inference_batch({"data": x})
    m.eval()
    assert m.cfg.TEST.CLS_THRESHOLD == 0.001          # low enough for the prior-probability biases of random weights (score ~ 0.01)
    outs = m.inference_batch({"data": x})
    cur = m._cur
    logits, offsets, objs = _unpack(cur["cls"], cur["box_obj"], B, 3, cur["sizes"], torch.float32)
    ref = yolox_inference([t.contiguous() for t in logits], [t.contiguous() for t in offsets], [t.contiguous() for t in objs],
                          cur["img_info"], m.cfg)
    assert len(outs) == len(ref) == B and any(o["boxes"].shape[0] > 0 for o in outs)
    for o, r in zip(outs, ref):
        for k in ("boxes", "box_scores", "box_labels"):
            assert torch.equal(torch.as_tensor(o[k]).as_subclass(torch.Tensor), torch.as_tensor(r[k]).as_subclass(torch.Tensor)), k
    again = m.inference_batch({"data": x})          # the cached scratch: same results, in new tensors
    assert all(torch.equal(torch.as_tensor(p["box_scores"]), torch.as_tensor(q["box_scores"])) for p, q in zip(outs, again))
    assert len(m._post) >= 1
    one = m.inference({"data": x})
    assert (isinstance(one, dict) and B == 1) or (isinstance(one, list) and len(one) == B)
    # a host batch takes the bd_h2d_submit route and gives the same detections
    host = m.inference_batch({"data": x.cpu().numpy()})
    assert all(torch.equal(torch.as_tensor(p["box_scores"]), torch.as_tensor(q["box_scores"])) for p, q in zip(outs, host))
    thr = m.cfg.TEST.CLS_THRESHOLD
    try:
        m.cfg.TEST.CLS_THRESHOLD = 0.99
        empty = m.inference_batch({"data": x})
    finally:
        m.cfg.TEST.CLS_THRESHOLD = thr
    assert all(tuple(o["boxes"].shape) == (0,) and tuple(o["box_labels"].shape) == (0,) for o in empty)
    m.train()


def test_ema_swap_leaves_the_weights_bit_identical(model3):
    from basedet_amd.layers.ema import ModelEMA
    m = model3
    m.train()
    ema = ModelEMA(m, 0.999, burnin_iter=0)
    ema.e.mul_(0.75)
    ema.r.add_(0.125)
    w, run, e = m.arena.w.clone(), m.norms.running.clone(), ema.e.clone()
    x = _batch(64, 64, 3, seed=9)["data"]
    m.eval()
    own = m.inference_batch({"data": x})
    with ema.applied() as avg:
        assert avg is m and torch.equal(m.arena.w, e)
        swapped = m.inference_batch({"data": x})
    back = m.inference_batch({"data": x})
    m.train()
    assert torch.equal(m.arena.w, w) and torch.equal(m.norms.running, run) and torch.equal(ema.e, e)
    key = lambda outs: [torch.as_tensor(o["box_scores"]).cpu() for o in outs]
    assert all(torch.equal(p, q) for p, q in zip(key(own), key(back)))
    assert not all(p.shape == q.shape and torch.equal(p, q) for p, q in zip(key(own), key(swapped)))
    sd = ema.state_dict()
    assert set(sd["model"]) == set(m.state_dict())
    ema.load_state_dict(sd)
    assert torch.equal(ema.e, e) and torch.equal(m.arena.w, w)
