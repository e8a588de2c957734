"""The CenterNet detector on the device: the seams between trunk, neck, head and losses, the trunk shared with the FPN detectors, the neck's
and head's parameters in the model's arena, the optimizer / EMA / clip / bucket path, a short training run, inference and the
bd_centernet_boxes_to_image kernel.

Shapes (the smallest at which the seams can still go wrong):
  A: resnet18, DECONV_CHANNEL [512, 64, 64, 64], K = 3, TENSOR_DIM 8, N = 2, input 64 x 96 -> OUTPUT_SIZE (16, 24), res5 2 x 3;
  B: resnet50, [2048, 64, 64, 64], K = 80, N = 1, 64 x 64, MODULATE_DEFORM False.
Ground truth: an image without boxes (A's image 0; B has one image, its empty batch runs in test_reproducible_losses), a box whose centre
lands on the map's last row and column, two boxes of one centre, one slot of label 0 (class -1)."""
import functools

import numpy as np
import pytest
import torch

import util
from util import guarded

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _cfg(shape, norm="BN", freeze_at=0):
    from basedet_amd.configs import CenterNetConfig
    cfg = CenterNetConfig()
    bb = dict(NORM=norm, FREEZE_AT=freeze_at)
    if shape == "A":
        cfg.merge(dict(MODEL=dict(BATCHSIZE=2, WEIGHTS=None, BACKBONE=dict(bb, NAME="resnet18"),
                                  HEAD=dict(DECONV_CHANNEL=[512, 64, 64, 64], IN_CHANNELS=64, TENSOR_DIM=8), OUTPUT_SIZE=(16, 24)),
                       DATA=dict(NUM_CLASSES=3)))
    else:
        cfg.merge(dict(MODEL=dict(BATCHSIZE=1, WEIGHTS=None, BACKBONE=bb,
                                  HEAD=dict(DECONV_CHANNEL=[2048, 64, 64, 64], MODULATE_DEFORM=False, TENSOR_DIM=8), OUTPUT_SIZE=(16, 16))))
    return cfg


def _batch(shape, seed=0, empty=False):
    N, H, W = (2, 64, 96) if shape == "A" else (1, 64, 64)
    K = 3 if shape == "A" else 80
    rng = np.random.default_rng(seed)
    data = rng.uniform(0, 255, (N, 3, H, W)).astype(np.float32)
    # last row and column of the stride-4 map; two boxes of one centre; a slot of label 0
    boxes = np.asarray([[W - 8, H - 8, W, H, 1], [24, 12, 40, 28, 2], [28, 16, 36, 24, K], [8, 8, 24, 20, 0]], np.float32)
    gt = np.zeros((N, 4, 5), np.float32)
    info = np.asarray([[H, W, H, W, 0]] * N, np.float32)
    if not empty:
        gt[N - 1] = boxes
        info[N - 1, 4] = 4
    return dict(data=data, gt_boxes=gt, im_info=info)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """One training forward and backward of a fresh model on the shared batch; everything the tests read is cloned."""
    from basedet_amd.models import CenterNet
    torch.manual_seed(0)
    model = CenterNet(_cfg(shape))
    batch = _batch(shape)
    losses = model(batch)
    phases = []
    model.backward(on_bucket_ready=lambda p, s: phases.append(p))
    torch.cuda.synchronize()
    pl = model._cur
    return dict(model=model, batch=batch, pl=pl, phases=phases, losses={k: v.clone() for k, v in losses.items()},
                grads=model.reference_grads(), state=model.state_dict(), res5=pl.blk[-1].out.clone(), g_out=pl.blk[-1].g_out.clone(),
                neck_dx=pl.neck_dx.clone(), logits=pl.logits.clone(), wr=pl.wr.clone(), d_logits=pl.d_logits.clone(), d_wr=pl.d_wr.clone(),
                tgt={k: v.clone() for k, v in pl.tgt.items()})


@pytest.mark.parametrize("shape", ["A", "B"])
def test_seams_are_exact(shape):
    from basedet_amd import ops
    c = _case(shape)
    model, pl, t = c["model"], c["pl"], c["tgt"]
    m = model.cfg.MODEL
    first, last = model.neck.layers()[0][1], model.neck.layers()[-1][1]
    assert first.stages["x"].data_ptr() == pl.blk[-1].out.data_ptr() and _same(first.stages["x"], c["res5"]), "the neck must read res5's stored output"
    assert model.head._saved[0].data_ptr() == last.stages["up_bn"].data_ptr() and _same(model.head._saved[0], last.stages["up_bn"])
    assert c["res5"].dtype == BF and tuple(c["res5"].shape) == (pl.N * pl.H5 * pl.W5, m.HEAD.DECONV_CHANNEL[0])
    assert (pl.Ho, pl.Wo) == tuple(m.OUTPUT_SIZE)
    N, K, T, M = pl.N, model.num_classes, m.HEAD.TENSOR_DIM, pl.N * pl.Ho * pl.Wo
    z = lambda: torch.zeros(1, dtype=F32, device="cuda")
    l_cls, l_wh, l_reg = z(), z(), z()
    ops.centernet_focal_fwd_bwd(c["logits"], t["score_map"], M, K, model.cls_ld, t["num_pos"], m.LOSS.CLS_WEIGHT, 1.0, l_cls,
                                torch.empty_like(c["logits"]))
    ops.centernet_l1_fwd_bwd(c["wr"], 8, 0, t["index"], t["reg_mask"], t["wh"], N, pl.Ho, pl.Wo, T, m.LOSS.WH_WEIGHT, 1.0, l_wh,
                             torch.empty_like(c["wr"]))
    ops.centernet_l1_fwd_bwd(c["wr"], 8, 2, t["index"], t["reg_mask"], t["reg"], N, pl.Ho, pl.Wo, T, m.LOSS.REG_WEIGHT, 1.0, l_reg,
                             torch.empty_like(c["wr"]))
    L = c["losses"]
    assert set(L) == {"total_loss", "loss_cls", "loss_box_wh", "loss_center_reg"} and all(v.is_cuda for v in L.values())
    assert _same(L["loss_cls"].reshape(1), l_cls) and _same(L["loss_box_wh"].reshape(1), l_wh) and _same(L["loss_center_reg"].reshape(1), l_reg)
    assert _same(L["total_loss"].reshape(1), (l_cls + l_wh) + l_reg)
    assert all(bool(torch.isfinite(v)) for v in L.values())
    # the targets saw the (H, W) = OUTPUT_SIZE map: the corner box's index is the last cell, the duplicate centre appears twice
    idx = t["index"][N - 1].cpu().tolist()
    assert idx[0] == pl.Ho * pl.Wo - 1 and idx[1] == idx[2] == 5 * pl.Wo + 8 and t["reg_mask"][N - 1].cpu().tolist() == [1, 1, 1, 1] + [0] * (T - 4)
    # res5's gradient in the trunk's convention
    want = ops.relu_bwd_bf16(c["neck_dx"], c["res5"], torch.empty_like(c["res5"]))
    assert _same(c["g_out"], want)
    assert _same(c["g_out"], torch.where(c["res5"] > 0, c["neck_dx"], torch.zeros_like(c["neck_dx"])))       # (+0 where the gate is closed)
    assert c["phases"] == ["head", "layer4", "layer3", "layer2", "layer1", "conv1"]


def _fcos_like(norm):
    from basedet_amd.configs import FCOSConfig
    cfg = FCOSConfig()
    cfg.merge(dict(MODEL=dict(BATCHSIZE=2, BACKBONE=dict(NAME="resnet18", OUT_FEATURE_CHANNELS=[128, 256, 512], NORM=norm, FREEZE_AT=0),
                              FPN=dict(TOP_BLOCK_IN_CHANNELS=512)), DATA=dict(NUM_CLASSES=3)))
    return cfg


@pytest.mark.parametrize("norm", ["FrozenBN", "BN"])
def test_trunk_is_the_fpn_detectors_trunk(norm):
    """An FCOS of the same backbone and norm at FREEZE_AT = 0 with the same weights: every backbone block output is bitwise equal.  Then
    (FrozenBN) both trunks' res5 g_out are seeded with one tensor and only the trunk's backward loop (FPNDetector._trunk_backward) runs:
    the backbone gradients are equal.  FCOS's loop accumulates onto the laterals' gradients of res3 / res4; those buffers are zeroed
    first, so its sums carry an extra `+ 0`: equality is by value (torch.equal: a -0 and a +0 compare equal), every other bit is pinned."""
    from basedet_amd.models import FCOS, CenterNet, params as P
    fcfg = _fcos_like(norm)
    fp = P.init_fcos_params(fcfg, seed=3, residual_gamma=0.2)
    fcos = FCOS(fcfg, params=fp)
    cn = CenterNet(_cfg("A", norm))
    state = cn.state_dict()
    state.update({k.replace("backbone.bottom_up.", "backbone."): v for k, v in fp.items() if k.startswith("backbone.bottom_up.")})
    cn.load_state_dict(state)
    batch = _batch("A", seed=5)
    fcos(batch), cn(batch)
    torch.cuda.synchronize()
    fpl, cpl = fcos._cur, cn._cur
    assert len(fpl.blk) == len(cpl.blk) == 8
    for i, (a, b) in enumerate(zip(fpl.blk, cpl.blk)):
        assert _same(a.out, b.out), f"block {i}"
    assert not hasattr(cpl, "P") and not hasattr(cpl, "g_P") and not hasattr(cpl, "lat") and not hasattr(cpl, "pyr")
    if norm != "FrozenBN":
        return
    g = (torch.randn(cpl.blk[-1].out.shape, generator=torch.Generator().manual_seed(1)) * 0.01).to(BF).cuda()
    g = g * (cpl.blk[-1].out > 0)
    grads = []
    for model in (fcos, cn):
        pl = model._cur
        for s in model.fpn_stages:
            pl.blk[pl.res[s]].g_out.zero_()
        pl.blk[-1].g_out.copy_(g)
        model._begin_wgrads()
        model._trunk_backward(pl, pl.wgrad_ws, pl.colsum_ws, None, ())
        model._join_wgrads()
        torch.cuda.synchronize()
        grads.append(model.reference_grads())
    n = 0
    for k, v in grads[1].items():
        if k.startswith("backbone."):
            assert torch.equal(v, grads[0][k.replace("backbone.", "backbone.bottom_up.")]), k
            n += 1
    assert n == 20 and bool(grads[1]["backbone.conv1.weight"].abs().sum() > 0)


def test_neck_and_head_gradients_in_the_arena():
    """reference_grads() of the neck and head against the standalone layers (which own their tensors) fed the model's res5 output and the
    model's loss gradients: the same launches.  Bitwise for the head and for everything upstream (in backward order) of the first
    bd_deform_conv_bwd_data -- deconv3's up_bn, up_sample, dcn_bn and its deformable convolution's own weight and bias.  Downstream of
    that launch's fp32 atomics bits are not claimed.  The bound there: two runs of bd_deform_conv_bwd_data differ in the
    order of an fp32 sum, by at most 2^-16 of the sum of the terms' magnitudes (the ACC term of tests/test_center_head_gpu.py), and
    d_x is that sum rounded to bf16, half a step being 2^-9: an element lands on the other side of a rounding boundary with probability
    at most 2^-16 / 2^-9 = 2^-7, and then moves by one step, 2^-8 relative.  The rel-L2 distance of d_x between two runs is therefore at
    most 2^-8 * sqrt(2^-7) = 2^-11.5, and every gradient downstream is linear in it; with the same allowance for each of the two later
    bd_deform_conv_bwd_data launches (deconv2, deconv1) the bound is 3 * 2^-11.5 < 2^-9.9, taken as 2^-10."""
    import basedet.layers as BL
    c = _case("A")
    model, pl = c["model"], c["pl"]
    h = model.cfg.MODEL.HEAD
    neck = BL.CenternetDeconv(list(h.DECONV_CHANNEL), list(h.DECONV_KERNEL), bool(h.MODULATE_DEFORM))
    head = BL.CenterHead(h.IN_CHANNELS, model.num_classes, h.CLS_PRIOR_PROB)
    # the state BEFORE the forward moved the running statistics does not matter for gradients: batch statistics are used
    neck.load_state_dict({k[9:]: v for k, v in c["state"].items() if k.startswith("upsample.")})
    head.load_state_dict({k[5:]: v for k, v in c["state"].items() if k.startswith("head.")})
    f = neck.forward_pm(c["res5"], pl.N, pl.H5, pl.W5)
    logits, wr = head.forward_pm(f, pl.N, pl.Ho, pl.Wo)
    assert _same(logits, c["logits"]) and _same(wr, c["wr"])
    dx = neck.backward_pm(head.backward_pm(c["d_logits"], c["d_wr"]))
    torch.cuda.synchronize()
    ref = {**{"upsample." + k: v.cpu() for k, v in neck.grads().items()}, **{"head." + k: v.cpu() for k, v in head.grads().items()}}
    got = c["grads"]
    names = [k for k in model.state_dict_trainable_names() if not k.startswith("backbone.")]
    assert set(names) == set(ref)
    dcn = "dcnv2" if h.MODULATE_DEFORM else "dcn"
    exact = lambda k: k.startswith("head.") or (k.startswith("upsample.deconv3.") and ("offset" not in k))
    for k in names:
        assert got[k].shape == ref[k].shape, k
        if exact(k):
            assert _same(got[k], ref[k]), k
        else:
            if k.endswith(f".dcn.{dcn}.bias"):
                # a bias in front of a training-mode batch norm: its true gradient is 0, the value is rounding noise of a sum of the bf16
                # gradient g (tests/test_center_head_gpu.py::test_end_to_end_wiring): |d_bias| <= (2^-8 + 2^-16) sum |g|, both runs
                g = getattr(model.neck, k.split(".")[1]).stage_grads["dcn"]
                bound = (2.0 ** -8 + 2.0 ** -16) * g.double().abs().sum(0).cpu()
                assert bool((got[k].double().abs() <= bound).all()) and bool((ref[k].double().abs() <= bound).all()), k
                continue
            d = util.rel_l2(got[k], ref[k])
            print(f"{k}: rel-L2 between two runs {d:.3e}")
            assert d <= 2.0 ** -10, k
    assert f"upsample.deconv3.dcn.{dcn}.weight" in ref
    # the arena holds them: every gradient view lies inside arena.g, nothing was allocated beside it
    lo, hi = model.arena.g.data_ptr(), model.arena.g.data_ptr() + 4 * model.arena.g.numel()
    held = list(model.head._store.g.values())
    for _, l in model.neck.layers():
        held += [*l._store.g.values(), *l.dcn._store.g.values(), *l.dcn_bn.g.values(), *l.up_bn.g.values()]
    assert len(held) == 8 + 3 * (1 + 4 + 2 + 2)
    for t in held:
        assert lo <= t.data_ptr() < hi


def test_optimizer_ema_clip_and_buckets_see_every_parameter():
    from basedet_amd.layers import ModelEMA
    from basedet_amd.models import CenterNet
    from basedet_amd.solver import DetSolver, GradBuckets, GradClip
    cfg = _cfg("A")
    model = CenterNet(cfg)
    batch, nxt = _batch("A"), _batch("A", seed=7)
    solver = DetSolver.build(cfg, model)
    before = model.state_dict()
    solver.minimize(model, batch)
    after = model.state_dict()
    names = model.state_dict_trainable_names()
    assert len(names) == len(set(names)) and set(names) <= set(after)
    same = [k for k in names if np.array_equal(before[k], after[k])]
    assert not same, f"masters the step did not change: {same}"
    assert not np.array_equal(before["upsample.deconv1.up_bn.running_mean"], after["upsample.deconv1.up_bn.running_mean"])
    fresh = CenterNet(cfg)
    fresh.load_state_dict(after)
    a, b = model(nxt), fresh(nxt)
    for k in a:
        assert _same(a[k].reshape(1), b[k].reshape(1)), f"{k}: the packed operands were not rebuilt from the masters"
    # optimizer state round trip
    opt = solver.optimizer
    sd = opt.state_dict()
    assert set(sd["momentum_buffer"]) == set(names)
    v0 = model.arena.v.clone()
    w0 = model.arena.w.clone()
    model.arena.v.zero_()
    opt.load_state_dict(sd)
    assert torch.equal(model.arena.v, v0) and torch.equal(model.arena.w, w0)
    # clip by norm over the whole arena
    model.backward()
    norm = float(model.arena.g.double().norm())
    clip = GradClip(model, "norm", max_norm=norm / 4)
    clip()
    assert abs(float(clip.last_norm) - norm) <= 1e-4 * norm
    assert abs(float(model.arena.g.double().norm()) - norm / 4) <= 1e-3 * norm / 4
    # one step with the EMA past its burn-in: the average and the buffer average move
    ema = ModelEMA(model, 0.5, burnin_iter=0)
    e0, r0 = ema.e.clone(), ema.r.clone()
    for _ in range(2):
        solver.minimize(model, batch, ema=ema)
        ema.step()
    assert not torch.equal(ema.e, e0) and not torch.equal(ema.r, r0) and bool(torch.isfinite(ema.e).all())
    assert ema.e.shape == model.arena.w.shape and ema.r.shape == model.norms.running.shape
    # buckets: a partition of the gradient arena in backward order
    ranges = GradBuckets(model)._ranges()
    assert set(ranges) == {"head", "layer4", "layer3", "layer2", "layer1", "conv1"}
    spans = sorted(ranges.values())
    assert spans[0][0] == 0 and spans[-1][1] == model.arena.g.numel()
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    for name, _, off, n in model.arena.entries:
        assert sum(lo <= off and off + n <= hi for lo, hi in spans) == 1, name


def test_it_learns():
    """The criterion of tests/test_center_head_gpu.py::test_short_training_run (TRAIN_STEPS steps on one fixed batch, every loss finite,
    the mean of the last five below the mean of the first five) through DetSolver at the config's learning rate scaled to the batch."""
    import center_head_oracle as O
    from basedet_amd.models import CenterNet
    from basedet_amd.solver import DetSolver
    cfg = _cfg("A")
    model = CenterNet(cfg)
    solver = DetSolver.build(cfg, model)
    assert abs(solver.optimizer.param_groups[0]["lr"] - cfg.SOLVER.BASIC_LR * 2) < 1e-12
    batch = _batch("A")
    r0 = model.norms.running.clone()
    vals = []
    for _ in range(O.TRAIN_STEPS):          # (the losses are views of the plan's loss buffer: read each step's before the next step)
        vals.append({k: float(v) for k, v in solver.minimize(model, batch).items()})
    total = [v["total_loss"] for v in vals]
    print("losses:", " ".join(f"{v:.3f}" for v in total))
    assert all(np.isfinite(x) for v in vals for x in v.values())
    assert np.mean(total[-5:]) < np.mean(total[:5])
    r1 = model.norms.running.clone()
    neck_lo = r1.numel() - 2 * sum(n.C for n in model._neck_norms.values())
    assert not torch.equal(r0[:neck_lo], r1[:neck_lo]) and not torch.equal(r0[neck_lo:], r1[neck_lo:]), "trunk and neck statistics move in train()"
    model.eval()
    model.inference(dict(data=batch["data"][:1]))
    torch.cuda.synchronize()
    assert torch.equal(model.norms.running, r1), "an eval() forward must not touch the running statistics"
    model.train()


def test_inference():
    from basedet_amd import ops
    from basedet_amd.models import CenterNet
    from basedet_amd.models.centernet import CenterNetDecoder
    model = CenterNet(_cfg("A"))
    batch = _batch("A")
    for _ in range(3):                      # running statistics away from their initial values
        model(batch)
    model.eval()
    info = np.asarray([[64, 96, 100, 150], [64, 96, 51, 77]], np.float32)
    outs = model.inference_batch(dict(data=batch["data"], im_info=info))
    pl = model._cur
    logits, wr = pl.logits.clone(), pl.wr.clone()
    singles = [model.inference(dict(data=batch["data"][i:i + 1], im_info=info[i:i + 1])) for i in range(2)]
    K, k = 3, 100
    assert len(outs) == 2
    for o, s in zip(outs, singles):
        b, sb = o.boxes.as_subclass(torch.Tensor), s.boxes.as_subclass(torch.Tensor)
        assert _same(b, sb) and _same(o.box_scores, s.box_scores) and torch.equal(o.box_labels, s.box_labels)
        assert tuple(b.shape) == (k, 4) and o.box_labels.dtype == torch.int32 and o.box_scores.dtype == F32
        assert int(o.box_labels.min()) >= 0 and int(o.box_labels.max()) < K
        assert bool((o.box_scores[:-1] >= o.box_scores[1:]).all())
    f = lambda *s: torch.empty(s, dtype=F32, device="cuda")
    boxes, scores, classes = f(2, k, 4), f(2, k), torch.empty((2, k), dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.centernet_decode_workspace_bytes(2, K, 16, 24), dtype=torch.uint8, device="cuda")
    ops.centernet_decode(logits, 8, wr, 8, 0, wr, 8, 2, 2, K, 16, 24, k, boxes, scores, classes, ws)
    # a device im_info is not read back: the same map in closed form on the device, held to the same bound
    outs_dev = model.inference_batch(dict(data=batch["data"], im_info=torch.from_numpy(info).cuda()))
    for tag, res in (("host im_info", outs), ("device im_info", outs_dev)):
        for i, o in enumerate(res):
            assert _same(o.box_scores, scores[i]) and torch.equal(o.box_labels, classes[i])
            _check_boxes(o, boxes[i], info[i], f"{tag}, image {i}")
    # without im_info: pre_process's default row, the padded and the given size (60 x 90 pads to 64 x 96)
    o = model.inference(dict(data=np.ascontiguousarray(batch["data"][:1, :, :60, :90])))
    ops.centernet_decode(model._cur.logits, 8, model._cur.wr, 8, 0, model._cur.wr, 8, 2, 1, K, 16, 24, k, boxes[:1], scores[:1], classes[:1], ws)
    _check_boxes(o, boxes[0], np.asarray([64, 96, 60, 90], np.float32), "no im_info")


def _check_boxes(o, raw, info_row, what, ds=4):
    """The Container's boxes against CenterNetDecoder.transform_boxes (float64, host) on the decoded map boxes `raw`, within
    4 * 2^-24 * (|a x| + |b y| + |c|) per coordinate."""
    from basedet_amd.models.centernet import CenterNetDecoder
    row = np.asarray(info_row, np.float64)[:4][::-1]
    args = (row[:2] // 2, row[-2:], row[-2:] // ds)
    raw = raw.cpu().numpy().astype(np.float64)
    want = CenterNetDecoder.transform_boxes(raw, *args)
    tr = np.abs(CenterNetDecoder.affine_matrix(*args))
    pts = np.abs(raw.reshape(-1, 2))
    bound = (4 * 2.0 ** -24 * (pts @ tr[:, :2].T + tr[:, 2])).reshape(-1, 4)
    err = np.abs(o.boxes.as_subclass(torch.Tensor).cpu().numpy().astype(np.float64) - want)
    print(f"{what}: worst error / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), what


class _Repeat:
    def __init__(self, batch):
        self.batch = batch

    def __iter__(self):
        while True:
            yield self.batch


def test_train_checkpoint_reload_and_evaluate(tmp_path):
    """The path a training run takes to its evaluation: DetTrainer steps with the EMA on, a checkpoint of the model and one of the
    average written to disk, each loaded into a fresh model, and the test-time pipeline of the config (TEST.AUG.VALUE: TestTimeCenterPad)
    on an image whose padded size, 64 x 64, is NOT the training shape (OUTPUT_SIZE describes the targets only).  The reloaded models
    give the trained model's bits -- for the average, the bits of the model inside ModelEMA.applied() in eval(): swap, folded trunk
    norms and the neck's precomputed 1 / std together.  Then inference_batch with a device im_info through the COCO evaluator."""
    from basedet_amd import ops
    from basedet_amd.data.transforms import build_transform
    from basedet_amd.engine import DetTrainer
    from basedet_amd.evaluators.selfcheck import evaluate_batch
    from basedet_amd.models import CenterNet
    from basedet_amd.solver import DetSolver
    from basedet_amd.utils.checkpoint import save_checkpoint
    cfg = _cfg("A")
    cfg.merge(dict(TRAINER=dict(EMA=dict(ENABLE=True, MOMENTUM=0.5, BURNIN_ITER=1))))
    model = CenterNet(cfg)
    trainer = DetTrainer(cfg, model, _Repeat(_batch("A")), DetSolver.build(cfg, model))
    meter = trainer.train(max_iters=4, log=None)
    assert all(np.isfinite(v) for v in meter.values())
    save_checkpoint(str(tmp_path / "model.pkl"), model.state_dict(), iter=4)
    save_checkpoint(str(tmp_path / "ema.pkl"), trainer.ema.state_dict()["model"], iter=4)

    rng = np.random.default_rng(11)
    raw = rng.integers(0, 256, (40, 50, 3)).astype(np.uint8)
    image, info = build_transform(cfg.TEST.AUG.VALUE, mode="test")(raw)
    assert image.shape == (1, 3, 64, 64) and info.tolist() == [[64, 64, 40, 50]]
    inputs = dict(data=image, im_info=info)

    def run(m):
        o = m.inference(inputs)
        return o.boxes.as_subclass(torch.Tensor).clone(), o.box_scores.clone(), o.box_labels.clone()

    model.eval()
    own = run(model)
    pl = model._cur
    assert (pl.Ho, pl.Wo) == (16, 16) != tuple(cfg.MODEL.OUTPUT_SIZE)
    # the centred pad: a map cell is 4 pixels, the image starts (64 - 50) / 2 = 7 and (64 - 40) / 2 = 12 pixels into the canvas
    assert torch.allclose(model._post[(1, 16, 16)]["aff"].cpu(), torch.tensor([[4.0, 0.0, -7.0, 0.0, 4.0, -12.0]]), rtol=0, atol=1e-5)
    k, K = 100, 3
    f = lambda *s: torch.empty(s, dtype=F32, device="cuda")
    boxes, scores, classes = f(1, k, 4), f(1, k), torch.empty((1, k), dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.centernet_decode_workspace_bytes(1, K, 16, 16), dtype=torch.uint8, device="cuda")
    ops.centernet_decode(pl.logits, 8, pl.wr, 8, 0, pl.wr, 8, 2, 1, K, 16, 16, k, boxes, scores, classes, ws)
    assert tuple(own[0].shape) == (k, 4) and _same(own[1], scores[0]) and torch.equal(own[2], classes[0])
    with trainer.ema.applied():
        averaged = run(model)
    assert not _same(averaged[1], own[1]), "the average differs from the live weights after four steps"
    assert all(_same(a, b) for a, b in zip(run(model), own)), "leaving applied() puts the live weights and statistics back"
    for path, want in (("model.pkl", own), ("ema.pkl", averaged)):
        fresh = CenterNet(cfg)
        fresh.load_weights(str(tmp_path / path), strict=True)
        fresh.eval()
        got = run(fresh)
        assert all(_same(a, b) for a, b in zip(got, want)), path
    # the evaluator on a collated batch with a device im_info (evaluate_batch switches to eval() and back)
    host = dict(data=image, gt_boxes=np.asarray([[[12, 16, 40, 44, 2], [30, 20, 50, 50, 1]]], np.float32),
                im_info=np.asarray([[64, 64, 40, 50, 2]], np.float32))
    dev = {k_: torch.from_numpy(v).cuda() for k_, v in host.items()}
    fresh.train()
    stats, ndet = evaluate_batch(fresh, cfg, host, dev)
    assert fresh.training and ndet == 100
    assert all(k_ in stats and np.isfinite(stats[k_]) and -1.0 <= stats[k_] <= 1.0 for k_ in ("AP", "AP50", "AP75", "AR100"))


def test_load_backbone_only_classification_checkpoint():
    """MODEL.WEIGHTS in the reference's config is a classification checkpoint of the bare ResNet (conv1, bn1, layerL.B.*, fc):
    load_weights(strict=False) matches it by suffix, leaves fc unused and the neck and head as they were."""
    from basedet_amd.models import CenterNet, params as P
    model = CenterNet(_cfg("A"))
    before = model.state_dict()
    ckpt = {}
    P.init_resnet(ckpt, np.random.default_rng(9), "resnet18", prefix="net")
    ckpt = {k[4:]: (v + 0.25).astype(np.float32) for k, v in ckpt.items()}
    ckpt["fc.weight"], ckpt["fc.bias"] = np.zeros((1000, 512), np.float32), np.zeros(1000, np.float32)
    model.load_weights({"state_dict": ckpt}, strict=False)
    after = model.state_dict()
    assert set(after) == set(before)
    for k, v in after.items():
        if k.startswith("backbone."):
            assert np.array_equal(v, ckpt[k[9:]]), k
        else:
            assert np.array_equal(v, before[k]), k
    losses = model(_batch("A"))
    assert bool(torch.isfinite(losses["total_loss"]))


AFFINES = dict(identity=[1, 0, 0, 0, 1, 0], offset=[1, 0, 3.25, 0, 1, -7.5], scale4=[4, 0, -11.3, 0, 4, -2.7], mixed=[3.9, 0.1, 17, -0.2, 4.1, 5])


@pytest.mark.parametrize("kind", list(AFFINES))
@pytest.mark.parametrize("B,k", [(b, k) for b in (1, 3) for k in (1, 100, 2048)])
def test_boxes_to_image_kernel(B, k, kind):
    """bd_centernet_boxes_to_image alone: guarded operands, two launches bit for bit, the bound of the issue against float64 (three fp32
    roundings of the fma chain and the rounding of the coefficients: 4 * 2^-24 * (|a x| + |b y| + |c|) per coordinate)."""
    from basedet_amd import ops
    g = torch.Generator().manual_seed(B * 10000 + k)
    H, W = 128, 160
    ctr = torch.rand(B, k, 2, generator=g) * torch.tensor([W, H])
    half = torch.rand(B, k, 2, generator=g) * 20
    boxes = torch.cat([ctr - half, ctr + half], -1)
    boxes[:, -1] = torch.tensor([W - 1.0, H - 1.0, float(W), float(H)])          # a box at the map's far corner
    aff = torch.tensor(AFFINES[kind], dtype=F32).repeat(B, 1) + torch.arange(B).view(B, 1) * torch.tensor([0, 0, 1.5, 0, 0, -2.25])
    scores = torch.rand(B, k, generator=g)
    classes = torch.randint(0, 80, (B, k), generator=g, dtype=torch.int32)
    ins = []
    for data, cols, dt, name in ((boxes.view(B * k, 4), 4, F32, "boxes"), (aff, 6, F32, "affine"), (scores.view(-1), None, F32, "scores"),
                                 (classes.view(-1), None, torch.int32, "classes")):
        # (util.guarded has fills for float formats: an int32 tensor is the int32 view of a guarded fp32 interior)
        t, h = guarded(data.shape[0], cols, F32, "cuda", fill="nan", name=name)
        t = t.view(dt)
        t.copy_(data.to(dt))
        h.snapshot()
        ins.append((t, h))
    runs = []
    for _ in range(2):
        outs = [guarded(B * k, 4, F32, "cuda", name="boxes_out"), guarded(B * k, None, F32, "cuda", name="scores_out"),
                guarded(B * k, None, F32, "cuda", name="labels_out")]
        outs[2] = (outs[2][0].view(torch.int32), outs[2][1])
        ops.centernet_boxes_to_image(ins[0][0], ins[1][0], ins[2][0], ins[3][0], B, k, *[t for t, _ in outs])
        torch.cuda.synchronize()
        for _, h in outs:
            h.check()
        runs.append([t.cpu().clone() for t, _ in outs])
    for _, h in ins:
        h.assert_unchanged()
    assert all(_same(a, b) for a, b in zip(*runs))
    ob, osc, ol = runs[0]
    assert _same(osc, scores.view(-1)) and torch.equal(ol, classes.view(-1))
    m = aff.double().view(B, 1, 2, 3)
    pts = boxes.double().view(B, k, 2, 2)                                         # [corner][x, y]
    want = torch.einsum("bkcj,bkij->bkci", pts, m[..., :2].expand(B, k, 2, 2)) + m[..., 2].view(B, 1, 1, 2)
    S = torch.einsum("bkcj,bkij->bkci", pts.abs(), m[..., :2].abs().expand(B, k, 2, 2)) + m[..., 2].abs().view(B, 1, 1, 2)
    err = (ob.double().view(B, k, 2, 2) - want).abs()
    assert bool((err <= 4 * 2.0 ** -24 * S).all()), float((err / (4 * 2.0 ** -24 * S)).max())
    if kind == "identity" and B == 1:
        assert _same(ob.view(-1), boxes.view(-1))


def test_boxes_to_image_refuses_bad_arguments():
    from basedet_amd import ops
    from basedet_amd._lib import BasedetHipError
    f = lambda *s: torch.full(s, 7.0, dtype=F32, device="cuda")
    boxes, aff, sc, cl = f(4, 4), f(1, 6), f(4), torch.zeros(4, dtype=torch.int32, device="cuda")
    ob, osc, ol = f(4, 4), f(4), torch.full((4,), 7, dtype=torch.int32, device="cuda")
    for args in ((boxes, aff, sc, cl, 0, 4, ob, osc, ol), (boxes, aff, sc, cl, 1, 0, ob, osc, ol), (boxes, aff, sc, cl, -1, 4, ob, osc, ol),
                 (None, aff, sc, cl, 1, 4, ob, osc, ol), (boxes, None, sc, cl, 1, 4, ob, osc, ol), (boxes, aff, sc, cl, 1, 4, None, osc, ol),
                 (boxes, aff, sc, cl, 1, 4, ob, osc, None)):
        with pytest.raises(BasedetHipError, match="centernet_boxes_to_image"):
            ops.centernet_boxes_to_image(*args)
    torch.cuda.synchronize()
    assert bool((ob == 7).all()) and bool((osc == 7).all()) and bool((ol == 7).all()), "a refused call must not launch"


@pytest.mark.parametrize("shape", ["A", "B"])
def test_reproducible_losses(shape):
    """Two forward passes of one batch give the same loss bits (gradients downstream of bd_deform_conv_bwd_data: no bits claimed,
    fp32 atomics).  A batch without a single box gives finite losses and no positive."""
    c = _case(shape)
    model = c["model"]
    a = {k: v.clone() for k, v in model(c["batch"]).items()}
    b = {k: v.clone() for k, v in model(c["batch"]).items()}
    for k in a:
        assert _same(a[k].reshape(1), b[k].reshape(1)) and _same(a[k].reshape(1), c["losses"][k].reshape(1)), k
    e = model(_batch(shape, empty=True))
    assert all(bool(torch.isfinite(v)) for v in e.values()) and float(e["loss_box_wh"]) == 0.0 and float(e["loss_center_reg"]) == 0.0
    assert float(model._cur.tgt["num_pos"]) == 0.0
    model(c["batch"])                       # (the shared case's stored tensors hold its own batch again)
