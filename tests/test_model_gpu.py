"""End-to-end GPU parity of the RetinaNet training step (forward losses, target assignment, parameter gradients,
SGD update) against the torch-CPU fp32 oracle (oracle/model.py) on the same parameters and the same batch.

Tolerances (bf16 activations/weights on the HIP side, fp32 oracle): losses and logits 2e-2 relative; labels /
matched anchors bit-exact; parameter gradients: cosine >= 0.99 against the plain fp32 oracle, and rel-L2 <= 1e-2
per parameter against the oracle evaluated on the same stored activations (identical ReLU gates)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _setup(backbone, N, size, seed=0, overrides=None):
    from basedet_amd.configs import RetinaNetConfig, retinanet_r18_config
    from basedet_amd.models import params as P
    from basedet_amd.utils import DummyLoader
    cfg = retinanet_r18_config() if backbone == "resnet18" else RetinaNetConfig()
    cfg.MODEL.BATCHSIZE = N
    if overrides:
        cfg.merge(overrides)
    params = P.init_retinanet_params(cfg, seed)
    rng = np.random.default_rng(seed + 1)
    for k in list(params):                       # non-trivial FrozenBN statistics
        if k.endswith("running_var"):
            params[k] = rng.uniform(0.5, 1.5, params[k].shape).astype(np.float32)
        elif k.endswith("running_mean"):
            params[k] = rng.normal(0, 0.1, params[k].shape).astype(np.float32)
        elif (".bn" in k or "downsample.1" in k) and k.endswith(".weight"):
            # last BN of every residual branch is damped so that random-init activations stay O(1-10) at res5
            last = (".bn3." in k) or (backbone in ("resnet18", "resnet34") and ".bn2." in k)
            lo, hi = (0.15, 0.35) if last else (0.7, 1.3)
            params[k] = rng.uniform(lo, hi, params[k].shape).astype(np.float32)
        elif (".bn" in k or "downsample.1" in k) and k.endswith(".bias"):
            params[k] = rng.normal(0, 0.1, params[k].shape).astype(np.float32)
    batch = next(DummyLoader(N, size, seed=seed))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    return cfg, params, batch


def _grad_of(model, name, like, cache={}):
    key = id(model)
    if cache.get("key") != key:
        cache.clear(); cache["key"] = key; cache["g"] = model.reference_grads()
    return cache["g"][name].double().reshape(-1)


# ("resnet18", 2, (512, 512)) is BASELINE config C1 at its own size (RetinaNet-R18-FPN, 2 x 512x512: the reference's CPU-runnable
# plumbing configuration, which bench.py's cpu_baseline leg times on the oracle): the HIP step against the oracle on C1's workload
@pytest.mark.parametrize("backbone,N,size", [("resnet18", 2, (128, 160)), ("resnet50", 3, (96, 128)), ("resnet18", 2, (512, 512))])
def test_training_step_matches_oracle(backbone, N, size):
    check_retinanet_step(*_setup(backbone, N, size))


def check_retinanet_step(cfg, params, batch):
    """One RetinaNet training step against the oracle: the assertions of test_training_step_matches_oracle, for any config (also
    imported by test_config_keys_gpu.py)."""
    from basedet_amd.models import RetinaNet, params as P
    from basedet_amd.solver import DetSolver
    from oracle.model import Oracle
    N = cfg.MODEL.BATCHSIZE
    model = RetinaNet(cfg, params=params)
    names = P.trainable_names(params, cfg.MODEL.BACKBONE.FREEZE_AT)
    assert sorted(names) == sorted(model.state_dict_trainable_names())

    # ---- (1) forward vs the plain fp32 oracle -------------------------------------------------------------
    orc = Oracle(params, P.oracle_arch(cfg), trainable=names)
    ref_losses, aux = orc.retinanet_losses(batch)
    ref_grads = orc.grads(ref_losses["total_loss"])
    losses = model(batch)
    pl = model._cur
    assert np.array_equal(pl.labels.cpu().numpy(), aux["labels"])            # target assignment: bit-exact
    assert int(pl.num_fg.item()) == aux["num_fg"]
    for k in ("cls_loss", "reg_loss", "total_loss"):
        got, ref = float(losses[k]), float(ref_losses[k].detach())
        assert abs(got - ref) / abs(ref) < 2e-2, (k, got, ref)               # bf16 tolerance (observed ~1e-5)
    K = cfg.DATA.NUM_CLASSES
    got_logits = pl.logits.float().cpu().view(-1, K)
    ref_logits = aux["logits"].detach()
    assert float((got_logits - ref_logits).norm() / ref_logits.norm()) < 2e-2

    model.backward()
    torch.cuda.synchronize()
    _grad_of.__defaults__[0].clear()
    # ---- (2) gradients vs the fp32 oracle: loose (bf16 forward differences flip ReLU gates) ------------------
    a = torch.cat([_grad_of(model, n, ref_grads[n]) for n in names])
    b = torch.cat([ref_grads[n].detach().double().reshape(-1) for n in names])
    assert float(torch.dot(a, b) / (a.norm() * b.norm())) > 0.99
    # ---- (3) gradients vs the oracle evaluated on the SAME stored activations: tight ------------------------
    # (the backward pass is then the same linear map on both sides; only bf16 rounding of gradient tensors differs)
    orc2 = Oracle(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=model.debug_activations())
    l2, _ = orc2.retinanet_losses(batch)
    g2 = orc2.grads(l2["total_loss"])
    for n in names:
        r = g2[n].detach().double().reshape(-1)
        g = _grad_of(model, n, g2[n])
        rel = float((g - r).norm() / (r.norm() + 1e-30))
        assert rel < 1e-2, (n, rel)

    # ---- (4) one optimizer step (solver/default_solver.py:96-114) -------------------------------------------
    solver = DetSolver.build(cfg, model)
    lr = solver.optimizer.param_groups[0]["lr"]
    assert abs(lr - cfg.SOLVER.BASIC_LR * N) < 1e-12
    w_before = model.arena.w.clone()
    solver.optimizer.step()
    state = orc2.sgd_step(g2, {}, lr, 0.9, cfg.SOLVER.WEIGHT_DECAY)
    delta_ref, delta_got = [], []
    for name in names:
        idx = [e[0] for e in model.arena.entries].index(name)
        _, shape, off, n = model.arena.entries[idx]
        d = (model.arena.view("w", idx) - w_before[off: off + n].view(shape)).cpu()
        if d.ndim == 4:
            d = d.permute(0, 3, 1, 2)
        d = d[: state[name].shape[0]]
        delta_got.append(d.reshape(-1).double()); delta_ref.append((-lr * state[name]).reshape(-1).double())
    a, b = torch.cat(delta_got), torch.cat(delta_ref)
    assert float((a - b).norm() / b.norm()) < 1e-2


def test_minimize_runs_and_loss_decreases():
    """Solver.minimize protocol (engine/trainer.py:98): a few steps on a fixed batch reduce the loss."""
    from basedet_amd.models import RetinaNet
    from basedet_amd.solver import DetSolver
    cfg, params, batch = _setup("resnet18", 2, (128, 160), seed=3)
    model = RetinaNet(cfg, params=params)
    solver = DetSolver.build(cfg, model)
    solver.optimizer.param_groups[0]["lr"] = 0.01
    first = None
    for it in range(8):
        out = solver.minimize(model, batch)
        v = float(out["total_loss"])
        assert np.isfinite(v)
        first = v if first is None else first
    assert v < first, (first, v)


def _level_split(t, sizes, per_pixel):
    out, o = [], 0
    for (h, w) in sizes:
        n = h * w * per_pixel
        out.append(t[o:o + n]); o += n
    return out


def test_retinanet_inference_matches_oracle():
    """retinanet.py:172-209 on the HIP kernels (scores, per-level top-k, decode, NMS, rescale) against the numpy restatement
    evaluated on the same bf16 logits / offsets."""
    check_retinanet_inference()


def check_retinanet_inference(overrides=None):
    """The assertions of test_retinanet_inference_matches_oracle under a config override (also imported by test_config_keys_gpu.py)."""
    from basedet_amd.models import RetinaNet, params as P
    from oracle import rcnn_ops as orc
    from oracle.model import Oracle
    cfg, params, batch = _setup("resnet18", 1, (128, 160), seed=5, overrides=overrides)
    params["head.cls_score.bias"] = np.full_like(params["head.cls_score.bias"], -2.5)      # scores around the 0.05 threshold
    params["head.cls_score.weight"] = params["head.cls_score.weight"] * 8
    params["head.bbox_pred.weight"] = params["head.bbox_pred.weight"] * 8
    batch["im_info"][0, 2:4] = (100, 141)                                                    # a rescale different from 1
    model = RetinaNet(cfg, params=params).eval()
    out = model({"data": batch["data"], "im_info": batch["im_info"]})
    assert set(out.keys()) == {"boxes", "box_scores", "box_labels"}
    pl = model._plan(1, 128, 160)
    K, A = model.num_classes, model.num_anchors
    logits = pl.logits.float().cpu().numpy().reshape(-1)
    offs = pl.offsets.float().cpu().numpy()[:, : A * 4].reshape(-1, 4)
    boxes_all = Oracle(params, P.oracle_arch(cfg)).retinanet_decode(pl.anchors.cpu().numpy(), offs)      # MODEL.BOX_REG (identity by default)
    sc_l = _level_split(orc.sigmoid(logits), pl.sizes, A * K)
    bx_l = _level_split(boxes_all, pl.sizes, A)
    rb, rs, rl = orc.detect_postprocess(sc_l, bx_l, K, batch["im_info"][0], cfg.TEST.CLS_THRESHOLD, cfg.TEST.IOU_THRESHOLD,
                                        cfg.TEST.MAX_BOXES_PER_IMAGE)
    assert len(rs) > 10
    assert out["boxes"].shape[0] == len(rs)
    assert np.array_equal(out["box_labels"].cpu().numpy(), rl)
    np.testing.assert_allclose(out["box_scores"].cpu().numpy(), rs, rtol=1e-5)
    np.testing.assert_allclose(out["boxes"].float().cpu().numpy(), rb, rtol=1e-5, atol=1e-3)


def test_fcos_inference_matches_oracle():
    from basedet_amd.configs import FCOSConfig
    from basedet_amd.models import FCOS, params as P
    from basedet_amd.utils import DummyLoader
    from oracle import box_ops as ob, rcnn_ops as orc
    cfg = FCOSConfig()
    cfg.MODEL.BATCHSIZE = 1
    params = P.init_fcos_params(cfg, seed=0, residual_gamma=0.25)
    params["head.cls_score.bias"] = np.full_like(params["head.cls_score.bias"], -1.0)
    params["head.cls_score.weight"] = params["head.cls_score.weight"] * 8
    params["head.bbox_pred.bias"] = np.full_like(params["head.bbox_pred.bias"], 1.5)
    batch = next(DummyLoader(1, (128, 160), seed=0))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    model = FCOS(cfg, params=params).eval()
    out = model({"data": batch["data"], "im_info": batch["im_info"]})
    pl = model._plan(1, 128, 160)
    K = model.num_classes
    logits = pl.logits.float().cpu().numpy()
    ctr = pl.raw.float().cpu().numpy()[:, 4:5]
    scores = np.sqrt(orc.sigmoid(logits) * orc.sigmoid(ctr)).astype(np.float32).reshape(-1)
    boxes_all = ob.point_decode(pl.points.cpu().numpy(), pl.offsets.float().cpu().numpy())
    rb, rs, rl = orc.detect_postprocess(_level_split(scores, pl.sizes, K), _level_split(boxes_all, pl.sizes, 1), K, batch["im_info"][0],
                                        cfg.TEST.CLS_THRESHOLD, cfg.TEST.IOU_THRESHOLD, cfg.TEST.MAX_BOXES_PER_IMAGE)
    assert len(rs) > 10
    assert out["boxes"].shape[0] == len(rs)
    assert np.array_equal(out["box_labels"].cpu().numpy(), rl)
    np.testing.assert_allclose(out["box_scores"].cpu().numpy(), rs, rtol=1e-5)
    np.testing.assert_allclose(out["boxes"].float().cpu().numpy(), rb, rtol=1e-5, atol=1e-3)


def test_faster_rcnn_inference_matches_oracle():
    """faster_rcnn.py:98-131: proposals (test top-k) -> box head on every proposal -> softmax / per-class decode -> threshold
    -> NMS; the oracle restates the post-processing on the box-head outputs of the HIP run."""
    check_faster_rcnn_inference()


def check_faster_rcnn_inference(overrides=None):
    """The assertions of test_faster_rcnn_inference_matches_oracle under a config override (also imported by test_config_keys_gpu.py)."""
    from basedet_amd.models import FasterRCNN
    from oracle import box_ops as ob, rcnn_ops as orc
    cfg, params, batch = _frcnn_setup(1, (128, 160), seed=2, overrides=overrides)
    params["rcnn.pred_cls.weight"] = params["rcnn.pred_cls.weight"] * 5      # confident but unsaturated softmax scores
    model = FasterRCNN(cfg, params=params).eval()
    out = model({"data": batch["data"], "im_info": batch["im_info"]})
    pl = model._cur
    K = model.num_classes
    R = pl.rois.shape[1]
    nr = int(pl.num_rois[0].item())
    assert 0 < nr <= R
    raw = pl.inf["raw"].float().cpu().numpy()
    rois = pl.rois[0].cpu().numpy()
    lg = raw[:nr, : K + 1].astype(np.float32)
    e = np.exp(lg - lg.max(axis=1, keepdims=True)).astype(np.float32)
    scores = (e / e.sum(axis=1, keepdims=True))[:, 1:].astype(np.float32)
    deltas = raw[:nr, K + 1: K + 1 + 4 * K].reshape(nr * K, 4)
    boxes = ob.box_decode(np.repeat(rois[:nr], K, axis=0), deltas, cfg.MODEL.RCNN_BOX_REG.MEAN, cfg.MODEL.RCNN_BOX_REG.STD)
    rb, rs, rl = orc.detect_postprocess([scores.reshape(-1)], [boxes], K, batch["im_info"][0], cfg.TEST.CLS_THRESHOLD,
                                        cfg.TEST.IOU_THRESHOLD, cfg.TEST.MAX_BOXES_PER_IMAGE, topk=2048)
    assert len(rs) > 5
    assert out["boxes"].shape[0] == len(rs)
    assert np.array_equal(out["box_labels"].cpu().numpy(), rl)
    np.testing.assert_allclose(out["box_scores"].cpu().numpy(), rs, rtol=1e-4)
    np.testing.assert_allclose(out["boxes"].float().cpu().numpy(), rb, rtol=1e-4, atol=1e-2)


def test_fcos_training_step_matches_oracle():
    """FCOS (models/det/fcos.py): GroupNorm towers, per-level scales, centre-ness; point target assignment bit-exact,
    losses within bf16 tolerance, gradients tight against the oracle evaluated on the same stored activations."""
    check_fcos_step(*fcos_setup())


def fcos_setup(overrides=None):
    """The FCOS fixture of test_fcos_training_step_matches_oracle; `overrides` is merged into the config before the parameters are drawn."""
    from basedet_amd.configs import FCOSConfig
    from basedet_amd.models import params as P
    from basedet_amd.utils import DummyLoader
    N, size = 2, (128, 160)
    cfg = FCOSConfig()
    cfg.MODEL.BATCHSIZE = N
    if overrides:
        cfg.merge(overrides)
    params = P.init_fcos_params(cfg, seed=0, residual_gamma=0.25)
    rng = np.random.default_rng(7)
    for k in list(params):
        if k.startswith("head.") and (k.endswith(".1.weight") or k.endswith(".4.weight") or k.endswith(".7.weight") or k.endswith(".10.weight")):
            params[k] = rng.uniform(0.7, 1.3, params[k].shape).astype(np.float32)       # GroupNorm gamma
        if k == "head.scales":
            params[k] = rng.uniform(0.8, 1.2, params[k].shape).astype(np.float32)
        if k in ("head.bbox_pred.bias",):
            params[k] = np.full_like(params[k], 0.5)                                     # keep relu(bbox_pred * scale) alive
    batch = next(DummyLoader(N, size, seed=0))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    return cfg, params, batch


def check_fcos_step(cfg, params, batch):
    """The assertions of test_fcos_training_step_matches_oracle, for any FCOS config (also imported by test_config_keys_gpu.py)."""
    from basedet_amd.models import FCOS, params as P
    from oracle.model import Oracle
    model = FCOS(cfg, params=params)
    names = P.trainable_names(params, cfg.MODEL.BACKBONE.FREEZE_AT)
    assert sorted(names) == sorted(model.state_dict_trainable_names())
    orc = Oracle(params, P.oracle_arch(cfg), trainable=names)
    ref, aux = orc.fcos_losses(batch)
    out = model(batch)
    pl = model._cur
    assert np.array_equal(pl.labels.cpu().numpy(), aux["labels"])
    assert np.array_equal(pl.gt_offsets.cpu().numpy(), aux["gt_offsets"])
    st = pl.stats.cpu().numpy()
    assert st[0] == aux["num_fg"] and abs(st[1] - aux["sum_ctr"]) / aux["sum_ctr"] < 1e-5
    for k in ("cls_loss", "reg_loss", "ctr_loss", "total_loss"):
        got, want = float(out[k]), float(ref[k].detach())
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)
    model.backward()
    torch.cuda.synchronize()
    orc2 = Oracle(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=model.debug_activations())
    l2, _ = orc2.fcos_losses(batch)
    g2 = orc2.grads(l2["total_loss"])
    got = model.reference_grads()
    for n in names:
        r = g2[n].detach().double().reshape(-1)
        g = got[n].double().reshape(-1)
        rel = float((g - r).norm() / (r.norm() + 1e-30))
        assert rel < 2e-2, (n, rel)


def _frcnn_setup(N, size, seed=0, pool=(7, 7), overrides=None):
    from basedet_amd.configs import FasterRCNNConfig
    from basedet_amd.models import params as P
    from basedet_amd.utils import DummyLoader
    cfg = FasterRCNNConfig()
    cfg.merge(dict(MODEL=dict(BATCHSIZE=N, BACKBONE=dict(NAME="resnet18", OUT_FEATURE_CHANNELS=[64, 128, 256, 512]),
                              FPN=dict(TOP_BLOCK_IN_CHANNELS=512),
                              RPN=dict(TRAIN_PREV_NMS_TOPK=300, TRAIN_POST_NMS_TOPK=120, TEST_PREV_NMS_TOPK=300, TEST_POST_NMS_TOPK=120,
                                       NUM_SAMPLE_ANCHORS=64),
                              RCNN=dict(NUM_ROIS=48), ROI_POOLER=dict(SIZE=tuple(pool)))))
    if overrides:
        cfg.merge(overrides)
    params = P.init_faster_rcnn_params(cfg, seed, residual_gamma=0.25)
    rng = np.random.default_rng(seed + 11)
    # larger head weights than the N(0, 0.01) init so that scores / deltas are not all ~0 (non-trivial top-k, NMS, sampling)
    for k in ("rpn.rpn_cls_score.weight", "rpn.rpn_bbox_offsets.weight", "rcnn.pred_cls.weight", "rcnn.pred_delta.weight",
              "rcnn.fc1.weight", "rcnn.fc2.weight", "rpn.rpn_conv.weight"):
        params[k] = (params[k] * 3).astype(np.float32)
    batch = next(DummyLoader(N, size, seed=seed))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    return cfg, params, batch


@pytest.mark.parametrize("pool", [(7, 7), (14, 14), (5, 3)])
def test_faster_rcnn_training_step_matches_oracle(pool):
    """Faster R-CNN (models/det/faster_rcnn.py): RPN targets bit-exact with the same sampling keys; proposals, sampled RoIs,
    labels and the four losses against the oracle evaluated on the stored activations of the HIP run (so that the discrete
    proposal / sample selection sees identical scores); parameter gradients rel-L2 <= 2e-2 per parameter.
    ROI_POOLER.SIZE other than the configured 7 x 7 (the reference's roi_pool takes any, roi_pool.py:35-78): RoIAlign's backward then
    leaves the tiled 7 x 7 kernel for the general fp32 scatter -- chosen per plan, no flag."""
    check_faster_rcnn_step(*_frcnn_setup(2, (128, 160), pool=pool))


def check_faster_rcnn_step(cfg, params, batch):
    """The assertions of test_faster_rcnn_training_step_matches_oracle, for any Faster R-CNN config at 2 x 128 x 160 (also imported by
    test_config_keys_gpu.py)."""
    from basedet_amd.models import FasterRCNN, params as P
    from oracle.model import Oracle
    N, size = 2, (128, 160)
    pool = tuple(cfg.MODEL.ROI_POOLER.SIZE)
    model = FasterRCNN(cfg, params=params)
    assert model.deterministic_roi_bwd is True
    names = P.trainable_names(params, cfg.MODEL.BACKBONE.FREEZE_AT)
    assert sorted(names) == sorted(model.state_dict_trainable_names())
    pl = model._plan(N, size[0], size[1])
    assert pl.roi_bwd_tiled == (pool == (7, 7))
    Gmax = batch["gt_boxes"].shape[1]
    rng = np.random.default_rng(5)
    keys = dict(rpn_pos=rng.random((N, pl.A_total), dtype=np.float32), rpn_neg=rng.random((N, pl.A_total), dtype=np.float32),
                rcnn_fg=rng.random((N, pl.rois.shape[1] + Gmax), dtype=np.float32),
                rcnn_bg=rng.random((N, pl.rois.shape[1] + Gmax), dtype=np.float32))
    batch = dict(batch, sample_keys=keys)
    out = model(batch)
    model.backward()
    torch.cuda.synchronize()
    dbg = model.debug_samples()

    # (1) plain fp32 oracle: RPN targets are independent of the network output -> bit-exact; RPN losses within bf16 tolerance
    orc = Oracle(params, P.oracle_arch(cfg), trainable=names)
    ref, aux = orc.faster_rcnn_losses(batch, keys)
    assert np.array_equal(dbg["rpn_labels"], aux["rpn_labels"])
    for k in ("rpn_cls_loss", "rpn_reg_loss"):
        got, want = float(out[k]), float(ref[k].detach())
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)

    # (2) oracle on the stored activations of the HIP run: identical scores -> identical proposals and samples
    acts = model.debug_activations()
    valid = dbg["s_labels"].reshape(-1) >= 0
    ch = cfg.MODEL.FPN.OUT_CHANNELS
    pooled = acts.pop("pooled")[valid]
    nb = pool[0] * pool[1]
    acts["pooled"] = pooled.reshape(-1, nb, ch).permute(0, 2, 1).reshape(-1, ch * nb).contiguous()
    for k in ("fc1", "fc2", "rcnn_raw"):
        acts[k] = acts[k][valid].contiguous()
    orc2 = Oracle(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=acts)
    l2, aux2 = orc2.faster_rcnn_losses(batch, keys)
    for n in range(N):
        m = int(dbg["num_rois"][n])
        assert m == len(aux2["rois"][n])
        np.testing.assert_allclose(dbg["rois"][n, :m], aux2["rois"][n], rtol=1e-5, atol=1e-3)
    assert int(valid.sum()) == len(aux2["s_labels"])
    assert np.array_equal(dbg["s_labels"].reshape(-1)[valid], aux2["s_labels"])
    np.testing.assert_allclose(dbg["s_rois"].reshape(-1, 4)[valid], aux2["s_rois"], rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(dbg["s_targets"].reshape(-1, 4)[valid], aux2["s_targets"], rtol=1e-3, atol=1e-3)
    assert (aux2["s_labels"] > 0).sum() >= N                    # the gt boxes themselves are foreground candidates
    for k in ("rpn_cls_loss", "rpn_reg_loss", "rcnn_cls_loss", "rcnn_reg_loss", "total_loss"):
        got, want = float(out[k]), float(l2[k].detach())
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)
    g2 = orc2.grads(l2["total_loss"])
    got = model.reference_grads()
    for n in names:
        r = g2[n].detach().double().reshape(-1)
        g = got[n].double().reshape(-1)
        rel = float((g - r).norm() / (r.norm() + 1e-30))
        assert rel < 2e-2, (n, rel)


def test_faster_rcnn_minimize_runs():
    from basedet_amd.models import FasterRCNN
    from basedet_amd.solver import DetSolver
    cfg, params, batch = _frcnn_setup(2, (128, 160), seed=3)
    model = FasterRCNN(cfg, params=params)
    solver = DetSolver.build(cfg, model)
    solver.optimizer.param_groups[0]["lr"] = 0.0005         # the sampled anchors / RoIs change every step: keep the steps small
    first = None
    for it in range(10):
        out = solver.minimize(model, batch)
        v = float(out["total_loss"])
        assert np.isfinite(v)
        first = v if first is None else first
    assert v < first, (first, v)


def test_faster_rcnn_roi_backward_variants_agree():
    """RoIAlign backward variants inside the model (dL/dP already holds the RPN head's gradient when the RoI contributions arrive):
    the tiled fixed-order sum (the default since round 5) and the general fp32 atomic scatter (the default of rounds 2-4, now the
    fallback for poolers other than 7 x 7) must give the same parameter gradients for one step with identical sampling keys -- per
    parameter rel-L2 <= 2e-2 against the deterministic variant (observed: <= 3e-3)."""
    from basedet_amd.models import FasterRCNN
    grads = {}
    for name in ("det", "fp32"):
        cfg, params, batch = _frcnn_setup(2, (128, 160), seed=3)
        model = FasterRCNN(cfg, params=params)
        assert model.deterministic_roi_bwd is True           # the default is the tiled fixed-order sum
        model.deterministic_roi_bwd = name == "det"
        pl = model._plan(2, 128, 160)
        rng = np.random.default_rng(9)
        Gmax = batch["gt_boxes"].shape[1]
        keys = dict(rpn_pos=rng.random((2, pl.A_total), dtype=np.float32), rpn_neg=rng.random((2, pl.A_total), dtype=np.float32),
                    rcnn_fg=rng.random((2, pl.rois.shape[1] + Gmax), dtype=np.float32),
                    rcnn_bg=rng.random((2, pl.rois.shape[1] + Gmax), dtype=np.float32))
        model(dict(batch, sample_keys=keys))
        model.backward()
        torch.cuda.synchronize()
        grads[name] = model.reference_grads()
    worst = {}
    for name in ("fp32",):
        w = 0.0
        for n, r in grads["det"].items():
            g = grads[name][n].double().reshape(-1)
            r = r.double().reshape(-1)
            w = max(w, float((g - r).norm() / (r.norm() + 1e-30)))
        worst[name] = w
    print("worst per-parameter gradient rel-L2 vs the deterministic RoIAlign backward:", worst)
    assert worst["fp32"] < 2e-2, worst


def test_all_empty_batch_is_all_background():
    """A batch in which no image has an annotation (the pad collator then yields gt_boxes of shape (N, 0, 5)): every anchor / point is
    background, the regression losses are zero and the step runs (the oracle defines this case the same way)."""
    from basedet_amd.configs import FCOSConfig
    from basedet_amd.models import FCOS, RetinaNet, params as P
    from basedet_amd.solver import DetSolver
    cfg, params, batch = _setup("resnet18", 2, (128, 160))
    empty = dict(data=batch["data"], gt_boxes=np.zeros((2, 0, 5), np.float32), im_info=batch["im_info"].copy())
    empty["im_info"][:, 4] = 0
    model = RetinaNet(cfg, params=params)
    out = DetSolver.build(cfg, model).minimize(model, empty)
    assert int((model._cur.labels > 0).sum()) == 0 and int((model._cur.labels == 0).sum()) == model._cur.labels.numel()
    assert float(out["reg_loss"]) == 0.0 and np.isfinite(float(out["cls_loss"])) and float(out["cls_loss"]) > 0
    fc = FCOSConfig()
    fc.merge(dict(MODEL=dict(BATCHSIZE=2, BACKBONE=dict(NAME="resnet18", OUT_FEATURE_CHANNELS=[128, 256, 512]), FPN=dict(TOP_BLOCK_IN_CHANNELS=512))))
    fm = FCOS(fc, params=P.init_fcos_params(fc, seed=0))
    out = DetSolver.build(fc, fm).minimize(fm, empty)
    assert int((fm._cur.labels > 0).sum()) == 0
    assert float(out["reg_loss"]) == 0.0 and float(out["ctr_loss"]) == 0.0 and np.isfinite(float(out["total_loss"]))


def test_state_dict_roundtrip_and_load_weights(tmp_path):
    """state_dict() returns the reference layouts bit-exactly (incl. the permuted fc1 columns and the fused predictors of
    Faster R-CNN); load_weights (models/base_net.py:83-89) of a saved checkpoint reproduces the losses."""
    from basedet_amd.models import FasterRCNN, RetinaNet
    from basedet_amd.utils import save_checkpoint
    cfg, params, batch = _frcnn_setup(1, (128, 160), seed=4)
    m = FasterRCNN(cfg, params=params)
    sd = m.state_dict()
    for k, v in params.items():
        assert np.array_equal(sd[k], v), k
    cfg, params, batch = _setup("resnet18", 2, (128, 160), seed=6)
    a = RetinaNet(cfg, params=params)
    ref = {k: float(v) for k, v in a(batch).items()}
    path = tmp_path / "ck.pkl"
    save_checkpoint(path, a.state_dict())
    b = RetinaNet(cfg, seed=9)
    assert abs(float(b(batch)["total_loss"]) - ref["total_loss"]) > 1e-3
    b.load_weights(str(path))
    got = {k: float(v) for k, v in b(batch).items()}
    for k in ref:                     # loss sums are block-atomic fp32 adds: equal up to summation order
        assert abs(got[k] - ref[k]) <= 1e-5 * abs(ref[k]), (k, got[k], ref[k])


def test_inference_without_detections_returns_empty():
    """retinanet.py:185-186 / post_processing.py:59-61: nothing above TEST.CLS_THRESHOLD -> empty container."""
    from basedet_amd.models import RetinaNet
    cfg, params, batch = _setup("resnet18", 1, (128, 160), seed=5)        # prior-probability bias: every score ~ 0.01
    model = RetinaNet(cfg, params=params).eval()
    out = model({"data": batch["data"], "im_info": batch["im_info"]})
    assert out["boxes"].numel() == 0 and out["box_scores"].numel() == 0 and out["box_labels"].numel() == 0


def test_atss_training_step_matches_oracle():
    """ATSS (models/det/atss.py) = the FCOS network with the adaptive sample selection: assignment bit-exact, losses within bf16
    tolerance, gradients tight against the oracle evaluated on the same stored activations."""
    check_atss_step(*atss_setup())


def atss_setup(overrides=None):
    """The ATSS fixture of test_atss_training_step_matches_oracle; `overrides` is merged into the config before the parameters are drawn."""
    from basedet_amd.configs import ATSSConfig
    from basedet_amd.models import params as P
    from basedet_amd.utils import DummyLoader
    N, size = 2, (128, 160)
    cfg = ATSSConfig()
    cfg.MODEL.BATCHSIZE = N
    if overrides:
        cfg.merge(overrides)
    params = P.init_fcos_params(cfg, seed=0, residual_gamma=0.25)
    params["head.bbox_pred.bias"] = np.full_like(params["head.bbox_pred.bias"], 0.5)
    batch = next(DummyLoader(N, size, seed=0))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    return cfg, params, batch


def check_atss_step(cfg, params, batch):
    """The assertions of test_atss_training_step_matches_oracle, for any ATSS config (also imported by test_config_keys_gpu.py)."""
    from basedet_amd.models import ATSS, params as P
    from oracle.model import Oracle
    model = ATSS(cfg, params=params)
    names = P.trainable_names(params, cfg.MODEL.BACKBONE.FREEZE_AT)
    orc = Oracle(params, P.oracle_arch(cfg), trainable=names)
    ref, aux = orc.fcos_losses(batch)
    out = model(batch)
    pl = model._cur
    assert np.array_equal(pl.labels.cpu().numpy(), aux["labels"])
    assert np.array_equal(pl.gt_offsets.cpu().numpy(), aux["gt_offsets"])
    assert aux["num_fg"] > 10 and pl.stats.cpu().numpy()[0] == aux["num_fg"]
    for k in ("cls_loss", "reg_loss", "ctr_loss", "total_loss"):
        got, want = float(out[k]), float(ref[k].detach())
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)
    model.backward()
    torch.cuda.synchronize()
    orc2 = Oracle(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=model.debug_activations())
    l2, _ = orc2.fcos_losses(batch)
    g2 = orc2.grads(l2["total_loss"])
    got = model.reference_grads()
    for n in names:
        r = g2[n].detach().double().reshape(-1)
        g = got[n].double().reshape(-1)
        rel = float((g - r).norm() / (r.norm() + 1e-30))
        assert rel < 2e-2, (n, rel)


def test_ragged_batch_through_collator_matches_oracle():
    """Images of different sizes -> DetectionPadCollator (pad to the batch maximum with 0) -> pre_process (pad to x32 with the
    normalised value of 0, pre_processing.py:11-49) -> RetinaNet losses: same targets and losses as the oracle on the same dict."""
    from basedet_amd.data import DetectionPadCollator
    from basedet_amd.models import RetinaNet, params as P
    from oracle.model import Oracle
    cfg, params, _ = _setup("resnet18", 2, (128, 160))
    rng = np.random.default_rng(9)
    samples = []
    for (h, w, nb) in ((100, 150, 3), (120, 130, 1)):
        img = rng.uniform(0, 255, (3, h, w)).astype(np.float32)
        x1 = rng.uniform(0, w * 0.5, nb); y1 = rng.uniform(0, h * 0.5, nb)
        boxes = np.stack([x1, y1, x1 + rng.uniform(20, w * 0.45, nb), y1 + rng.uniform(20, h * 0.45, nb)], 1)
        samples.append((img, boxes, rng.integers(1, 81, nb), (2 * h, 2 * w)))
    batch = DetectionPadCollator().apply(samples)
    assert batch["data"].shape == (2, 3, 120, 150) and batch["gt_boxes"].shape == (2, 3, 5)
    model = RetinaNet(cfg, params=params)
    names = P.trainable_names(params, cfg.MODEL.BACKBONE.FREEZE_AT)
    ref, aux = Oracle(params, P.oracle_arch(cfg), trainable=names).retinanet_losses(batch)
    out = model(batch)
    pl = model._cur
    assert (pl.Hp, pl.Wp) == (128, 160)
    assert np.array_equal(pl.labels.cpu().numpy(), aux["labels"])
    for k in ("cls_loss", "reg_loss", "total_loss"):
        got, want = float(out[k]), float(ref[k].detach())
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)
