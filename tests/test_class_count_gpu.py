"""The one-stage detectors at class counts that are no multiple of 8 (DATA.NUM_CLASSES = 1, 13, 365, ...): one class stride
cls_ld = round_up(K, 8) per anchor, pad slots that no loss, selection or gradient ever sees.

Kernels alone (focal loss with a row stride, the column sum past 2048 channels, score selection on padded logits), then one training
step per model against the oracle at K = 13 / 365, the zero-pad invariant over three optimizer steps, and inference.  Tolerances are
those of the tests these follow (tests/test_boxops_gpu.py, tests/test_conv_gpu.py, tests/test_model_gpu.py, tests/test_ota_gpu.py,
tests/test_freeanchor_gpu.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ld(K):
    return (K + 7) // 8 * 8


# ---- 1. focal kernels ---------------------------------------------------------------------------------------------------------------
def _focal_problem(rows, K, seed):
    rng = np.random.default_rng(seed)
    ld = _ld(K)
    x = torch.from_numpy(rng.normal(0, 3, (rows, ld)).astype(np.float32)).to(torch.bfloat16)      # pad slots hold noise, not zeros:
    labels = rng.integers(1, K + 1, rows).astype(np.int32)                                        # a kernel that reads them shows
    u = rng.uniform(size=rows)
    labels[u < 0.5] = 0                         # background
    labels[u < 0.1] = -1                        # ignored
    # the four kinds of row the issue names, whatever the draw gave: ignored, background, positive in the tail vector, in a full vector
    forced = [-1, 0, K, 1]
    for i, v in enumerate(forced[: rows] if rows >= 4 else [K]):
        labels[i] = v
    return x, labels


@pytest.mark.parametrize("gamma", [2.0, 1.5])
@pytest.mark.parametrize("rows", [1, 257, 4099])
@pytest.mark.parametrize("K", [1, 3, 13, 365])
def test_focal_with_row_stride(K, rows, gamma):
    from basedet_amd import ops
    from oracle import box_ops as ob
    alpha = 0.25
    ld = _ld(K)
    x, labels = _focal_problem(rows, K, seed=K * 7 + rows)
    nfg = int((labels > 0).sum())
    norm = torch.tensor([nfg], dtype=torch.int32, device="cuda")
    xd, ld_dev = x.cuda(), torch.from_numpy(labels).cuda()
    loss = torch.zeros((1,), dtype=torch.float32, device="cuda")
    dl = torch.full((rows, ld), 7.0, dtype=torch.bfloat16, device="cuda")
    ops.focal_loss_fwd_bwd(xd, ld_dev, rows, K, alpha, gamma, norm, 1.0, loss, dl, ld=ld)
    torch.cuda.synchronize()
    xf = x.float().numpy().astype(np.float64)[:, :K]
    t = np.zeros((rows, K)); fg = labels > 0
    t[fg, labels[fg] - 1] = 1
    valid = labels >= 0
    ref_loss = ob.sigmoid_focal_loss(xf[valid], t[valid], alpha, gamma).sum() / max(1, nfg)
    got_loss = float(loss.item())
    print(f"K={K} rows={rows} gamma={gamma}: loss {got_loss} ref {ref_loss}")
    if valid.any():
        assert abs(got_loss - ref_loss) / ref_loss < 2e-3
    else:
        assert got_loss == 0.0
    got = dl.float().cpu().numpy()
    ref_grad = ob.sigmoid_focal_loss_grad(xf, t, alpha, gamma) * valid[:, None] / max(1, nfg)
    assert np.allclose(got[:, :K], ref_grad, rtol=2e-2, atol=1e-7)
    assert np.all(got[~valid] == 0)
    # every pad slot of the gradient is exactly +0
    assert not dl.view(torch.int16)[:, K:].any()
    # the real slots carry the bits of the existing entry point run with K = cls_ld on the same padded buffer (labels 1..K are valid there)
    loss2 = torch.zeros((1,), dtype=torch.float32, device="cuda")
    dl2 = torch.empty((rows, ld), dtype=torch.bfloat16, device="cuda")
    ops.focal_loss_fwd_bwd(xd, ld_dev, rows, ld, alpha, gamma, norm, 1.0, loss2, dl2)
    assert torch.equal(dl.view(torch.int16)[:, :K], dl2.view(torch.int16)[:, :K])


@pytest.mark.parametrize("gamma,general", [(2.0, False), (2.0, True), (1.5, False)])
def test_focal_stride_equal_to_k_is_the_old_entry(gamma, general):
    from basedet_amd import ops
    K, rows = 80, 4099
    x, labels = _focal_problem(rows, K, seed=3)
    norm = torch.tensor([int((labels > 0).sum())], dtype=torch.int32, device="cuda")
    xd, lab = x.cuda(), torch.from_numpy(labels).cuda()
    out = []
    for ld in (None, K):
        loss = torch.zeros((1,), dtype=torch.float32, device="cuda")
        dl = torch.empty((rows, K), dtype=torch.bfloat16, device="cuda")
        ops.focal_loss_fwd_bwd(xd, lab, rows, K, 0.25, gamma, norm, 1.0, loss, dl, general=general, ld=ld)
        out.append((loss, dl))
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32))
    assert torch.equal(out[0][1].view(torch.int16), out[1][1].view(torch.int16))


def test_old_focal_entry_still_refuses_other_k():
    from basedet_amd import _lib, ops
    x = torch.zeros((4, 13), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.BasedetHipError):
        ops.focal_loss_fwd_bwd(x, torch.zeros(4, dtype=torch.int32, device="cuda"), 4, 13, 0.25, 2.0, torch.ones(1, dtype=torch.int32, device="cuda"),
                               1.0, torch.zeros(1, device="cuda"), torch.empty_like(x))


# ---- 2. column sum ------------------------------------------------------------------------------------------------------------------
def _colsum_input(rows, C):
    g = torch.Generator().manual_seed(1000 + C)
    return torch.randn(rows, C, generator=g).to(torch.bfloat16)


@pytest.mark.parametrize("C", [2048, 2056, 3312])
def test_colsum_past_2048_channels(C):
    """Against a float64 sum with the tolerance of tests/test_conv_gpu.py::test_elementwise_pack_colsum_sgd.  C = 2048 runs as ONE chunk with
    the row stride equal to C -- the launch the code before the chunked walk made -- and the same 2048 columns as the first chunk of a
    3312-wide tensor (row stride 3312, second chunk beside it) must give the same bits: chunking moves nothing within a column."""
    from basedet_amd import ops
    rows = 5000
    m = _colsum_input(rows, C)
    out = torch.zeros(C, device="cuda")
    ws = torch.empty((ops.colsum_workspace_bytes(C) // 4,), dtype=torch.float32, device="cuda")
    ops.colsum_bf16(m.cuda(), rows, C, out, ws)
    ref = m.double().sum(0)
    err = float((out.cpu().double() - ref).abs().max())
    print(f"C={C}: max abs error {err}")
    assert torch.allclose(out.cpu().double(), ref, rtol=1e-4, atol=1e-3)
    # accumulate, and the per-level form (N images x cnt rows at an offset into each image) -- for C > 2048 across the chunk boundary,
    # the second chunk with a row stride (C) that is not its width
    out2 = out.clone()
    ops.colsum_bf16(m.cuda(), rows, C, out2, ws, accumulate=True)
    assert torch.equal(out2, out + out)
    pyr = ops.Geom(2, [40, 20], [50, 25])                   # 2 images x (2000 + 500) rows = the 5000 rows of m
    assert pyr.pixels == rows
    for lv in range(2):
        g1 = pyr.level(lv)
        out3 = torch.full((C,), 3.0, device="cuda")
        ops.colsum_bf16(m.cuda(), rows, C, out3, ws, geom=g1)
        n = g1.H[0] * g1.W[0]
        ref3 = m.view(2, pyr.pix_per_img, C)[:, g1.off[0]: g1.off[0] + n].double().sum((0, 1))
        assert torch.allclose(out3.cpu().double(), ref3, rtol=1e-4, atol=1e-3), lv
    if C == 2048:
        wide = torch.cat([m, _colsum_input(rows, 3312)[:, 2048:]], 1).contiguous()
        outw = torch.zeros(3312, device="cuda")
        wsw = torch.empty((ops.colsum_workspace_bytes(3312) // 4,), dtype=torch.float32, device="cuda")
        ops.colsum_bf16(wide.cuda(), rows, 3312, outw, wsw)
        assert torch.equal(outw[:2048].view(torch.int32), out.view(torch.int32))


# ---- 3. score selection on padded logits --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ctr", [False, True])
@pytest.mark.parametrize("K", [1, 13, 365])
def test_det_select_and_scores_on_padded_logits(K, with_ctr):
    from basedet_amd import ops
    B, seg_rows, k, thr = 2, [45, 18, 7], 64, 0.05
    rows, ld = sum(seg_rows), _ld(K)
    starts = [0, seg_rows[0], seg_rows[0] + seg_rows[1]]
    g = torch.Generator().manual_seed(K)
    compact = (torch.randn((B, rows, K), generator=g) * 2 - 1).to(torch.bfloat16)
    compact[:, ::3, 0] = 0                      # real logits equal to 0: a real 0.5 score beside the pads' 0.5
    compact[:, 1::5, K - 1] = 0
    compact[1, 40:50] = 0                       # whole rows of ties across a level boundary
    padded = torch.zeros((B, rows, ld), dtype=torch.bfloat16)
    padded[:, :, :K] = compact
    ctr = torch.randn((B, rows, 8), generator=g).to(torch.bfloat16).cuda() if with_ctr else None
    kw = dict(ctr=ctr, ctr_ld=8, ctr_off=4) if with_ctr else {}
    res = []
    for lg, stride in ((compact.contiguous().cuda(), None), (padded.cuda(), ld)):
        idx = torch.full((B, 3, k), -7, dtype=torch.int32, device="cuda")
        sc = torch.full((B, 3, k), -7.0, dtype=torch.float32, device="cuda")
        cnt = torch.full((B, 3), -7, dtype=torch.int32, device="cuda")
        ws = torch.full((ops.det_select_workspace_bytes(B, 3, rows, K, k),), 0xA5, dtype=torch.uint8, device="cuda")
        ops.det_select(lg, B, rows, K, starts, seg_rows, k, thr, idx, sc, cnt, ws, ld=stride, **kw)
        scores = torch.empty((B, rows * K), dtype=torch.float32, device="cuda")
        for b in range(B):
            ops.det_scores(lg[b], rows, K, scores[b], ld=stride, **({} if ctr is None else dict(ctr=ctr[b], ctr_ld=8, ctr_off=4)))
        torch.cuda.synchronize()
        res.append((idx, sc, cnt, scores))
    (i0, s0, c0, f0), (i1, s1, c1, f1) = res
    assert int(c0.sum()) > 0
    assert torch.equal(c0, c1), (c0.tolist(), c1.tolist())
    assert torch.equal(i0, i1)
    assert torch.equal(s0.view(torch.int32), s1.view(torch.int32))
    assert torch.equal(f0.view(torch.int32), f1.view(torch.int32))
    assert int(i1.max()) < max(seg_rows) * K


# ---- 4. one training step per model -------------------------------------------------------------------------------------------------
def _set_classes(batch, K):
    """The dummy annotations with classes in 1..K, class K (the tail vector's last real slot) and class 1 among them."""
    gt = batch["gt_boxes"].copy()
    for n in range(gt.shape[0]):
        for g in range(int(batch["im_info"][n, 4])):
            gt[n, g, 4] = K - (g * 5) % K if g % 2 == 0 else 1 + (g * 3) % K
    batch["gt_boxes"] = gt
    return batch


def _batch(N, size, K, seed=0):
    from basedet_amd.utils import DummyLoader
    batch = next(DummyLoader(N, size, seed=seed))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    return _set_classes(batch, K)


def _check_reference_shapes(model, params, names):
    """Exported weights and gradients keep the reference's shapes, (A*K, ...) for the class predictor."""
    sd, gr = model.state_dict(), model.reference_grads()
    for n in names:
        assert tuple(sd[n].shape) == tuple(params[n].shape), (n, sd[n].shape, params[n].shape)
        assert tuple(gr[n].shape) == tuple(params[n].shape), (n, gr[n].shape, params[n].shape)
    for n in ("head.cls_score.weight", "head.cls_score.bias"):
        assert np.array_equal(sd[n], params[n])                 # bind -> export is exact (fp32 masters)


def _check_grads(model, g2, names, tol):
    got = model.reference_grads()
    for n in names:
        r = g2[n].detach().double().reshape(-1)
        g = got[n].double().reshape(-1)
        rel = float((g - r).norm() / (r.norm() + 1e-30))
        assert rel < tol, (n, rel)


@pytest.mark.parametrize("K", [13, 365])
def test_retinanet_step_matches_oracle(K):
    """tests/test_model_gpu.py::test_training_step_matches_oracle at NUM_CLASSES = 13 and 365 (cls_score: 9 x 16 = 144 and 9 x 368 = 3312
    channels, the latter past the old 2048-channel limit of the bias gradient)."""
    from basedet_amd.configs import retinanet_r18_config
    from basedet_amd.models import RetinaNet, params as P
    from oracle.model import Oracle
    N, size = 2, (128, 160)
    cfg = retinanet_r18_config()
    cfg.MODEL.BATCHSIZE = N
    cfg.DATA.NUM_CLASSES = K
    params = P.init_retinanet_params(cfg, 0)
    batch = _batch(N, size, K)
    model = RetinaNet(cfg, params=params)
    assert model.cls_score.cout == 9 * _ld(K) and model._plan(N, *size).logits.shape[1] == 9 * _ld(K)
    names = P.trainable_names(params, cfg.MODEL.BACKBONE.FREEZE_AT)
    assert sorted(names) == sorted(model.state_dict_trainable_names())
    orc = Oracle(params, P.oracle_arch(cfg), trainable=names)
    ref_losses, aux = orc.retinanet_losses(batch)
    ref_grads = orc.grads(ref_losses["total_loss"])
    losses = model(batch)
    pl = model._cur
    assert np.array_equal(pl.labels.cpu().numpy(), aux["labels"])            # target assignment: bit-exact
    assert int(pl.num_fg.item()) == aux["num_fg"]
    assert (aux["labels"] == K).any()                                         # a positive in the tail vector
    for k in ("cls_loss", "reg_loss", "total_loss"):
        got, ref = float(losses[k]), float(ref_losses[k].detach())
        assert abs(got - ref) / abs(ref) < 2e-2, (k, got, ref)
    got_logits = model.cls_score.real_logits(pl.logits.float().cpu()).reshape(-1, K)
    ref_logits = aux["logits"].detach()
    assert float((got_logits - ref_logits).norm() / ref_logits.norm()) < 2e-2
    model.backward()
    torch.cuda.synchronize()
    got = model.reference_grads()
    a = torch.cat([got[n].double().reshape(-1) for n in names])
    b = torch.cat([ref_grads[n].detach().double().reshape(-1) for n in names])
    assert float(torch.dot(a, b) / (a.norm() * b.norm())) > 0.99
    orc2 = Oracle(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=model.debug_activations())
    l2, _ = orc2.retinanet_losses(batch)
    _check_grads(model, orc2.grads(l2["total_loss"]), names, 1e-2)
    _check_reference_shapes(model, params, names)
    assert tuple(params["head.cls_score.weight"].shape) == (9 * K, 256, 3, 3)


def _fcos_family(cls_name, cfg_name, K, matching=None):
    from basedet_amd import configs, models
    from basedet_amd.models import params as P
    N, size = 2, (128, 160)
    cfg = getattr(configs, cfg_name)()
    cfg.MODEL.BATCHSIZE = N
    cfg.DATA.NUM_CLASSES = K
    if matching:
        cfg.MODEL.MATCHING = matching
    params = P.init_fcos_params(cfg, seed=0, residual_gamma=0.25)
    params["head.bbox_pred.bias"] = np.full_like(params["head.bbox_pred.bias"], 0.5)
    batch = _batch(N, size, K)
    model = getattr(models, cls_name)(cfg, params=params)
    assert model.cls_score.cout == _ld(K) and tuple(params["head.cls_score.weight"].shape) == (K, 256, 3, 3)
    names = P.trainable_names(params, cfg.MODEL.BACKBONE.FREEZE_AT)
    return cfg, params, batch, model, names


@pytest.mark.parametrize("family", ["FCOS", "ATSS"])
def test_fcos_atss_step_matches_oracle(family):
    """tests/test_model_gpu.py::test_fcos_training_step_matches_oracle / test_atss_training_step_matches_oracle at NUM_CLASSES = 13."""
    from basedet_amd.models import params as P
    from oracle.model import Oracle
    K = 13
    cfg, params, batch, model, names = _fcos_family(family, family + "Config", K)
    orc = Oracle(params, P.oracle_arch(cfg), trainable=names)
    ref, aux = orc.fcos_losses(batch)
    out = model(batch)
    pl = model._cur
    assert np.array_equal(pl.labels.cpu().numpy(), aux["labels"])
    assert np.array_equal(pl.gt_offsets.cpu().numpy(), aux["gt_offsets"])
    st = pl.stats.cpu().numpy()
    assert st[0] == aux["num_fg"] and aux["num_fg"] > 10 and abs(st[1] - aux["sum_ctr"]) / aux["sum_ctr"] < 1e-5
    for k in ("cls_loss", "reg_loss", "ctr_loss", "total_loss"):
        got, want = float(out[k]), float(ref[k].detach())
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)
    model.backward()
    torch.cuda.synchronize()
    orc2 = Oracle(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=model.debug_activations())
    l2, _ = orc2.fcos_losses(batch)
    _check_grads(model, orc2.grads(l2["total_loss"]), names, 2e-2)
    _check_reference_shapes(model, params, names)


def test_ota_topk_step_matches_oracle():
    """tests/test_ota_gpu.py::test_ota_training_step_matches_oracle at NUM_CLASSES = 13."""
    from basedet_amd.models import params as P
    from oracle.model import Oracle
    K = 13
    cfg, params, batch, model, names = _fcos_family("OTA", "OTAConfig", K)
    orc = Oracle(params, P.oracle_arch(cfg), trainable=names)
    ref, aux = orc.ota_losses(batch)
    out = model(batch)
    pl = model._cur
    lab = pl.labels.cpu().numpy()
    nfg = int((aux["labels"] > 0).sum())
    assert nfg >= 5
    agree = (lab == aux["labels"]).mean()
    assert agree > 0.995, agree
    assert abs(int((lab > 0).sum()) - nfg) <= max(2, nfg // 5)
    for k in ("loss_cls", "loss_offsets", "loss_ious", "total_loss"):
        got, want = float(out[k]), float(ref[k].detach())
        assert abs(got - want) / abs(want) < 0.1, (k, got, want)
    model.backward()
    torch.cuda.synchronize()
    forced = (lab, pl.gt_offsets.cpu().numpy(), pl.gt_ctr.cpu().numpy())
    orc2 = Oracle(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=model.debug_activations())
    l2, _ = orc2.ota_losses(batch, forced=forced)
    for k in ("loss_cls", "loss_offsets", "loss_ious", "total_loss"):
        got, want = float(out[k]), float(l2[k].detach())
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)
    _check_grads(model, orc2.grads(l2["total_loss"]), names, 2e-2)
    _check_reference_shapes(model, params, names)


def test_ota_sinkhorn_step_matches_oracle():
    """MATCHING = "sinkhorn" at NUM_CLASSES = 13: the device's assignment handed to the oracle on the stored activations (as the top-k
    test's second half); the assignment itself against oracle.box_ops.ota_ground_truth on the device's own bf16 predictions."""
    from basedet_amd.models import params as P
    from oracle import box_ops
    from oracle.model import Oracle
    K = 13
    cfg, params, batch, model, names = _fcos_family("OTA", "OTAConfig", K, matching="sinkhorn")
    out = model(batch)
    pl = model._cur
    lab = pl.labels.cpu().numpy()
    N, P_ = lab.shape
    logits = pl.logits.float().cpu().numpy().reshape(N, P_, _ld(K))[:, :, :K]
    pred = pl.offsets.float().cpu().numpy().reshape(N, P_, 4)
    pts = []
    o = 0
    allp = pl.points.cpu().numpy()
    for (h, w) in pl.sizes:
        pts.append(allp[o:o + h * w]); o += h * w
    num = batch["im_info"][:, 4].astype(np.int32)
    lab_o, _, _, aux = box_ops.ota_ground_truth(pts, model.strides, logits, pred, batch["gt_boxes"], num, 0.25, 2.0, 1.5, 2.5, 10,
                                                matching="sinkhorn")
    nfg = int((lab_o > 0).sum())
    assert nfg >= 5
    diff = np.argwhere(lab != lab_o)
    assert len(diff) <= max(1, nfg // 20), (len(diff), nfg)
    model.backward()
    torch.cuda.synchronize()
    forced = (lab, pl.gt_offsets.cpu().numpy(), pl.gt_ctr.cpu().numpy())
    orc2 = Oracle(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=model.debug_activations())
    l2, _ = orc2.ota_losses(batch, forced=forced)
    for k in ("loss_cls", "loss_offsets", "loss_ious", "total_loss"):
        got, want = float(out[k]), float(l2[k].detach())
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)
    _check_grads(model, orc2.grads(l2["total_loss"]), names, 2e-2)
    _check_reference_shapes(model, params, names)


def test_freeanchor_step_matches_oracle():
    """tests/test_freeanchor_gpu.py::test_freeanchor_training_step_matches_oracle at NUM_CLASSES = 13."""
    from basedet_amd.configs import FreeAnchorConfig
    from basedet_amd.models import FreeAnchor, params as P
    from oracle.model import Oracle
    N, size, K = 2, (128, 160), 13
    cfg = FreeAnchorConfig()
    cfg.merge(dict(MODEL=dict(BACKBONE=dict(NAME="resnet18", OUT_FEATURE_CHANNELS=[128, 256, 512]), FPN=dict(TOP_BLOCK_IN_CHANNELS=512))))
    cfg.MODEL.BATCHSIZE = N
    cfg.DATA.NUM_CLASSES = K
    params = P.init_retinanet_params(cfg, seed=0)
    batch = _batch(N, size, K)
    model = FreeAnchor(cfg, params=params)
    names = P.trainable_names(params, cfg.MODEL.BACKBONE.FREEZE_AT)
    orc = Oracle(params, P.oracle_arch(cfg), trainable=names)
    ref, _ = orc.freeanchor_losses(batch)
    out = model(batch)
    for k in ("pos_loss", "neg_loss", "total_loss"):
        got, want = float(out[k]), float(ref[k].detach())
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)
    pl = model._cur
    assert not pl.d_logits.view(-1, _ld(K)).view(torch.int16)[:, K:].any()         # pad slots of the gradient: exactly +0
    model.backward()
    torch.cuda.synchronize()
    orc2 = Oracle(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=model.debug_activations())
    l2, _ = orc2.freeanchor_losses(batch)
    _check_grads(model, orc2.grads(l2["total_loss"]), names, 2e-2)
    _check_reference_shapes(model, params, names)


def test_freeanchor_refuses_more_classes_than_its_lds_tile_when_built():
    from basedet_amd.configs import FreeAnchorConfig
    from basedet_amd.models import FreeAnchor
    cfg = FreeAnchorConfig()
    cfg.DATA.NUM_CLASSES = 365
    with pytest.raises(ValueError, match="NUM_CLASSES = 365"):
        FreeAnchor(cfg)


# ---- 5. pads stay zero --------------------------------------------------------------------------------------------------------------
def test_pad_rows_stay_zero():
    """Three solver.minimize steps of RetinaNet at K = 13 with momentum, weight decay and TRAINER.EMA: every pad row of cls_score's weight,
    bias, gradient and momentum, and of the EMA's copy, is exactly 0; the real rows moved."""
    from basedet_amd.configs import retinanet_r18_config
    from basedet_amd.engine import DetTrainer
    from basedet_amd.models import RetinaNet, params as P
    from basedet_amd.solver import DetSolver
    N, size, K, A = 2, (128, 160), 13, 9
    ld = _ld(K)
    cfg = retinanet_r18_config()
    cfg.MODEL.BATCHSIZE = N
    cfg.DATA.NUM_CLASSES = K
    cfg.TRAINER.EMA.merge(dict(ENABLE=True, MOMENTUM=0.5, BURNIN_ITER=1))     # step 1: burn-in copy; steps 2, 3: inside the SGD launch
    params = P.init_retinanet_params(cfg, 0)
    batch = _batch(N, size, K)
    model = RetinaNet(cfg, params=params)
    solver = DetSolver.build(cfg, model)
    group = solver.optimizer.param_groups[0]
    assert group["momentum"] > 0 and group["weight_decay"] > 0
    tr = DetTrainer(cfg, model, [], solver)                                   # its model_step is solver.minimize(model, batch, ema=tr.ema)
    ema = tr.ema
    assert ema is not None
    c = model.cls_score
    w0 = c.w.clone()
    entries = {e[0]: e for e in model.arena.entries}

    def pads(flat, name):
        _, shape, off, n = entries[name]
        t = flat[off:off + n].view(shape)
        return t.reshape((A, ld) + tuple(shape[1:]))[:, K:]

    for _ in range(3):
        out = tr.model_step(batch)
        assert np.isfinite(float(out["total_loss"]))
        torch.cuda.synchronize()
        for name in ("head.cls_score.weight", "head.cls_score.bias"):
            for which, flat in (("w", model.arena.w), ("g", model.arena.g), ("v", model.arena.v), ("ema", ema.e)):
                p = pads(flat, name)
                assert p.numel() > 0 and not (p != 0).any(), (name, which)
    assert not torch.equal(c.w, w0)
    with ema.applied():
        sd = model.state_dict()
    assert sd["head.cls_score.weight"].shape == (A * K, 256, 3, 3) and sd["head.cls_score.bias"].shape == (A * K,)


# ---- 6. inference -------------------------------------------------------------------------------------------------------------------
def _level_split(t, sizes, per_pixel):
    out, o = [], 0
    for (h, w) in sizes:
        n = h * w * per_pixel
        out.append(t[o:o + n]); o += n
    return out


def test_retinanet_inference_k13():
    """tests/test_model_gpu.py::test_retinanet_inference_matches_oracle at NUM_CLASSES = 13: the pad slots' 0.5 scores never surface."""
    from basedet_amd.configs import retinanet_r18_config
    from basedet_amd.models import RetinaNet, params as P
    from oracle import box_ops as ob, rcnn_ops as orc
    K = 13
    cfg = retinanet_r18_config()
    cfg.MODEL.BATCHSIZE = 1
    cfg.DATA.NUM_CLASSES = K
    params = P.init_retinanet_params(cfg, 5)
    params["head.cls_score.bias"] = np.full_like(params["head.cls_score.bias"], -2.5)      # scores around the 0.05 threshold
    params["head.cls_score.weight"] = params["head.cls_score.weight"] * 8
    params["head.bbox_pred.weight"] = params["head.bbox_pred.weight"] * 8
    batch = _batch(1, (128, 160), K, seed=5)
    batch["im_info"][0, 2:4] = (100, 141)
    model = RetinaNet(cfg, params=params).eval()
    out = model({"data": batch["data"], "im_info": batch["im_info"]})
    pl = model._plan(1, 128, 160)
    A = model.num_anchors
    logits = model.cls_score.real_logits(pl.logits.float().cpu()).numpy().reshape(-1)
    offs = pl.offsets.float().cpu().numpy()[:, : A * 4].reshape(-1, 4)
    boxes_all = ob.box_decode(pl.anchors.cpu().numpy(), offs)
    rb, rs, rl = orc.detect_postprocess(_level_split(orc.sigmoid(logits), pl.sizes, A * K), _level_split(boxes_all, pl.sizes, A), K,
                                        batch["im_info"][0], cfg.TEST.CLS_THRESHOLD, cfg.TEST.IOU_THRESHOLD, cfg.TEST.MAX_BOXES_PER_IMAGE)
    assert len(rs) > 10
    assert out["boxes"].shape[0] == len(rs)
    labels = out["box_labels"].cpu().numpy()
    assert labels.max() < K and labels.min() >= 0
    assert np.array_equal(labels, rl)
    np.testing.assert_allclose(out["box_scores"].cpu().numpy(), rs, rtol=1e-5)
    np.testing.assert_allclose(out["boxes"].float().cpu().numpy(), rb, rtol=1e-5, atol=1e-3)


def test_fcos_inference_k13():
    """tests/test_model_gpu.py::test_fcos_inference_matches_oracle at NUM_CLASSES = 13."""
    from basedet_amd.configs import FCOSConfig
    from basedet_amd.models import FCOS, params as P
    from oracle import box_ops as ob, rcnn_ops as orc
    K = 13
    cfg = FCOSConfig()
    cfg.MODEL.BATCHSIZE = 1
    cfg.DATA.NUM_CLASSES = K
    params = P.init_fcos_params(cfg, seed=0, residual_gamma=0.25)
    params["head.cls_score.bias"] = np.full_like(params["head.cls_score.bias"], -1.0)
    params["head.cls_score.weight"] = params["head.cls_score.weight"] * 8
    params["head.bbox_pred.bias"] = np.full_like(params["head.bbox_pred.bias"], 1.5)
    batch = _batch(1, (128, 160), K)
    model = FCOS(cfg, params=params).eval()
    out = model({"data": batch["data"], "im_info": batch["im_info"]})
    pl = model._plan(1, 128, 160)
    logits = pl.logits.float().cpu().numpy()[:, :K]
    ctr = pl.raw.float().cpu().numpy()[:, 4:5]
    scores = np.sqrt(orc.sigmoid(logits) * orc.sigmoid(ctr)).astype(np.float32).reshape(-1)
    boxes_all = ob.point_decode(pl.points.cpu().numpy(), pl.offsets.float().cpu().numpy())
    rb, rs, rl = orc.detect_postprocess(_level_split(scores, pl.sizes, K), _level_split(boxes_all, pl.sizes, 1), K, batch["im_info"][0],
                                        cfg.TEST.CLS_THRESHOLD, cfg.TEST.IOU_THRESHOLD, cfg.TEST.MAX_BOXES_PER_IMAGE)
    assert len(rs) > 10
    assert out["boxes"].shape[0] == len(rs)
    labels = out["box_labels"].cpu().numpy()
    assert labels.max() < K and labels.min() >= 0
    assert np.array_equal(labels, rl)
    np.testing.assert_allclose(out["box_scores"].cpu().numpy(), rs, rtol=1e-5)
    np.testing.assert_allclose(out["boxes"].float().cpu().numpy(), rb, rtol=1e-5, atol=1e-3)


# ---- 7. Faster R-CNN already takes any class count ----------------------------------------------------------------------------------
def test_faster_rcnn_step_k13():
    """tests/test_model_gpu.py::test_faster_rcnn_training_step_matches_oracle (7 x 7 pooling) at NUM_CLASSES = 13: pins what worked before the
    one-stage heads took a class stride."""
    from basedet_amd.configs import FasterRCNNConfig
    from basedet_amd.models import FasterRCNN, params as P
    from oracle.model import Oracle
    N, size, K = 2, (128, 160), 13
    cfg = FasterRCNNConfig()
    cfg.merge(dict(MODEL=dict(BATCHSIZE=N, BACKBONE=dict(NAME="resnet18", OUT_FEATURE_CHANNELS=[64, 128, 256, 512]),
                              FPN=dict(TOP_BLOCK_IN_CHANNELS=512),
                              RPN=dict(TRAIN_PREV_NMS_TOPK=300, TRAIN_POST_NMS_TOPK=120, TEST_PREV_NMS_TOPK=300, TEST_POST_NMS_TOPK=120,
                                       NUM_SAMPLE_ANCHORS=64),
                              RCNN=dict(NUM_ROIS=48), ROI_POOLER=dict(SIZE=(7, 7)))))
    cfg.DATA.NUM_CLASSES = K
    params = P.init_faster_rcnn_params(cfg, 0, residual_gamma=0.25)
    for k in ("rpn.rpn_cls_score.weight", "rpn.rpn_bbox_offsets.weight", "rcnn.pred_cls.weight", "rcnn.pred_delta.weight",
              "rcnn.fc1.weight", "rcnn.fc2.weight", "rpn.rpn_conv.weight"):
        params[k] = (params[k] * 3).astype(np.float32)
    batch = _batch(N, size, K)
    model = FasterRCNN(cfg, params=params)
    names = P.trainable_names(params, cfg.MODEL.BACKBONE.FREEZE_AT)
    pl = model._plan(N, size[0], size[1])
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
    acts = model.debug_activations()
    valid = dbg["s_labels"].reshape(-1) >= 0
    ch = cfg.MODEL.FPN.OUT_CHANNELS
    pooled = acts.pop("pooled")[valid]
    acts["pooled"] = pooled.reshape(-1, 49, ch).permute(0, 2, 1).reshape(-1, ch * 49).contiguous()
    for k in ("fc1", "fc2", "rcnn_raw"):
        acts[k] = acts[k][valid].contiguous()
    orc2 = Oracle(params, P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=acts)
    l2, aux2 = orc2.faster_rcnn_losses(batch, keys)
    assert np.array_equal(dbg["s_labels"].reshape(-1)[valid], aux2["s_labels"])
    assert (aux2["s_labels"] > 0).sum() >= N and aux2["s_labels"].max() <= K
    for k in ("rpn_cls_loss", "rpn_reg_loss", "rcnn_cls_loss", "rcnn_reg_loss", "total_loss"):
        got, want = float(out[k]), float(l2[k].detach())
        assert abs(got - want) / abs(want) < 2e-2, (k, got, want)
    _check_grads(model, orc2.grads(l2["total_loss"]), names, 2e-2)
