"""Inference on a batch: N = 3 images of 128x160 through ONE launch chain (bd_det_select or bd_segment_topk(B = N) ->
bd_det_candidates(B = N) -> bd_nms_batched(B = N) -> bd_det_finalize(B = N)) against

  * the single-image chain (det_scores -> segment_topk -> det_candidates -> nms_batched -> det_finalize, B = 1) run on each image's slice
    of the SAME batched plan's logits / offsets / RoIs: boxes, scores and labels bit-identical.  The network ran once, at batch 3, for
    both sides, so batch-size-dependent kernel routing inside it cannot enter the comparison;
  * oracle/rcnn_ops.py detect_postprocess per image on the device's own scores and decoded boxes, with the comparison of
    tests/test_fullsize_inference_gpu.py's _compare: labels and order exact, boxes and scores at that file's tolerances
    (rtol 1e-5 / atol 1e-3 for the one-stage heads, 1e-4 / 1e-2 for the RCNN head).

Models and parameters are those of tests/test_model_gpu.py's inference tests; the classification bias is shifted by bisection on a
first forward (the recipe of test_fullsize_inference_gpu.py) so that a fixed fraction of the items clears TEST.CLS_THRESHOLD.
Every image has its own im_info: one is shrunk, one enlarged, one anisotropic, so rescale and clipping differ per image."""
import numpy as np
import pytest
import torch

from oracle import box_ops as ob
from oracle import rcnn_ops as orc

pytestmark = pytest.mark.gpu
SIZE = (128, 160)
N = 3
IM_INFO = np.asarray([[128, 160, 96, 120, 0], [128, 160, 192, 240, 0], [128, 160, 100, 141, 0]], np.float32)


def _shift_for_fraction(frac_of, target):
    lo, hi = -30.0, 30.0
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if frac_of(mid) < target else (lo, mid)
    return 0.5 * (lo + hi)


def _level_split(a, rows):
    out, o = [], 0
    for r in rows:
        out.append(a[o:o + r]); o += r
    return out


def _data(seed, n=N):
    from basedet_amd.utils import DummyLoader
    b = next(DummyLoader(n, SIZE, seed=seed))
    return (b["data"] * 255).astype(np.float32)


def _single_image_chain(cfg, scores, lvl_rows, K, mode, info_row, k, anchors=None, offsets=None, off_ld=4, A=1, mean=(0, 0, 0, 0),
                        std=(1, 1, 1, 1), item_boxes=None):
    """FPNDetector._detect as it was for one image: one launch chain of B = 1 per image."""
    from basedet_amd import ops
    t = cfg.TEST
    Ln = len(lvl_rows)
    row_off = [0]
    for r in lvl_rows[:-1]:
        row_off.append(row_off[-1] + r)
    i32 = dict(dtype=torch.int32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    tk_idx = torch.empty((Ln, k), **i32); tk_sc = torch.empty((Ln, k), **f32); tk_cnt = torch.empty((Ln,), **i32)
    ops.segment_topk(scores, 1, 0, 1, 1, 0, [r * K for r in row_off], [r * K for r in lvl_rows], k, tk_idx, tk_sc, tk_cnt,
                     min_score=t.CLS_THRESHOLD)
    C = Ln * k
    boxes = torch.empty((C, 4), **f32); sc = torch.empty((1, C), **f32); labels = torch.empty((1, C), **i32)
    ops.det_candidates(mode, tk_idx, tk_sc, tk_cnt, 1, Ln, k, row_off, K, anchors, offsets, 0, off_ld, A, mean, std, item_boxes, 0, boxes, sc,
                       labels)
    max_out = t.MAX_BOXES_PER_IMAGE
    keep = torch.empty((1, max_out), **i32); num = torch.zeros((1,), **i32)
    ws = torch.empty((ops.nms_batched_workspace_bytes(1, C),), dtype=torch.uint8, device="cuda")
    ops.nms_batched(boxes, sc, labels, t.IOU_THRESHOLD, max_out, keep, num, ws)
    ob_ = torch.empty((max_out, 4), **f32); osc = torch.empty((max_out,), **f32); ol = torch.empty((max_out,), **i32)
    ops.det_finalize(boxes, sc, labels, keep, num, max_out, info_row.contiguous(), ob_, osc, ol)
    n = int(num.item())
    return ob_[:n], osc[:n], ol[:n], tk_cnt.cpu().numpy()


def _assert_same_bits(out, ref, what):
    rb, rs, rl, _ = ref
    n = rs.shape[0]
    assert out["box_scores"].numel() == n, (what, out["box_scores"].numel(), n)
    if n == 0:
        assert out["boxes"].numel() == 0 and out["box_labels"].numel() == 0
        return
    assert torch.equal(out["box_labels"], rl), what
    assert torch.equal(out["box_scores"].view(torch.int32), rs.view(torch.int32)), what
    assert torch.equal(torch.as_tensor(out["boxes"]).float().view(torch.int32), rb.view(torch.int32)), what


def _compare_oracle(out, sc_l, bx_l, K, cfg, k, tol, im_info):
    """_compare of tests/test_fullsize_inference_gpu.py with the image's own im_info."""
    t = cfg.TEST
    rb, rs, rl = orc.detect_postprocess(sc_l, bx_l, K, np.asarray(im_info, np.float32), t.CLS_THRESHOLD, t.IOU_THRESHOLD,
                                        t.MAX_BOXES_PER_IMAGE, topk=k)
    assert out["box_scores"].numel() == len(rs)
    if len(rs) == 0:
        return 0
    assert np.array_equal(out["box_labels"].cpu().numpy(), rl)
    np.testing.assert_allclose(out["box_scores"].cpu().numpy(), rs, rtol=tol[0])
    np.testing.assert_allclose(torch.as_tensor(out["boxes"]).float().cpu().numpy(), rb, rtol=tol[0], atol=tol[1])
    return len(rs)


# ---- the three models: one batched run each, shared by the bitwise and the oracle test ----------------------------------------------
_RUNS = {}


def _retinanet_params(seed=5, overrides=None):
    from tests.test_model_gpu import _setup
    cfg, params, _ = _setup("resnet18", N, SIZE, seed=seed, overrides=overrides)
    params["head.cls_score.weight"] = params["head.cls_score.weight"] * 8
    params["head.bbox_pred.weight"] = params["head.bbox_pred.weight"] * 8
    return cfg, params


def _run_retinanet(name="retinanet", overrides=None):
    if name in _RUNS:
        return _RUNS[name]
    from basedet_amd import ops
    from basedet_amd.models import RetinaNet
    cfg, params = _retinanet_params(overrides=overrides)
    batch = {"data": _data(5), "im_info": IM_INFO}
    thr = cfg.TEST.CLS_THRESHOLD
    model = RetinaNet(cfg, params=params).eval()
    model(batch)
    logits = model._plan(N, *SIZE).logits.float().reshape(-1)
    d = _shift_for_fraction(lambda s: float((torch.sigmoid(logits + s) > thr).float().mean()), 2e-2)
    params["head.cls_score.bias"] = params["head.cls_score.bias"] + np.float32(d)
    model = RetinaNet(cfg, params=params).eval()
    outs = model(batch)
    pl = model._plan(N, *SIZE)
    K, A = model.num_classes, model.num_anchors
    rows = pl.pyr.pix_per_img * A
    lvl_rows = [h * w * A for h, w in pl.sizes]
    assert lvl_rows == [2880, 720, 180, 54, 18]
    info = torch.from_numpy(IM_INFO).cuda()
    m = cfg.MODEL.BOX_REG
    per = []
    for i in range(N):
        lg = pl.logits.view(N, rows, K)[i]
        offs = pl.offsets.view(N, pl.pyr.pix_per_img, -1)[i]
        scores = torch.empty((rows * K,), dtype=torch.float32, device="cuda")
        ops.det_scores(lg, rows, K, scores)
        ref = _single_image_chain(cfg, scores, lvl_rows, K, 0, info[i], 1000, anchors=pl.anchors, offsets=offs, off_ld=model.box_ld, A=A,
                                  mean=m.MEAN, std=m.STD)
        deltas = offs[:, : A * 4].float().reshape(-1, 4).contiguous()
        boxes = ops.box_decode(pl.anchors, deltas, m.MEAN, m.STD).cpu().numpy()
        np.testing.assert_allclose(boxes, ob.box_decode(pl.anchors.cpu().numpy(), deltas.cpu().numpy(), m.MEAN, m.STD), rtol=1e-5, atol=1e-3)
        per.append(dict(ref=ref, sc_l=_level_split(scores.cpu().numpy(), [r * K for r in lvl_rows]), bx_l=_level_split(boxes, lvl_rows)))
    _RUNS[name] = (cfg, K, outs, per, 1000, (1e-5, 1e-3))
    return _RUNS[name]


def _fcos_params():
    from basedet_amd.configs import FCOSConfig
    from basedet_amd.models import params as P
    cfg = FCOSConfig()
    cfg.MODEL.BATCHSIZE = N
    params = P.init_fcos_params(cfg, seed=0, residual_gamma=0.25)
    params["head.cls_score.weight"] = params["head.cls_score.weight"] * 8
    params["head.bbox_pred.bias"] = np.full_like(params["head.bbox_pred.bias"], 1.5)
    return cfg, params


def _run_fcos():
    if "fcos" in _RUNS:
        return _RUNS["fcos"]
    from basedet_amd import ops
    from basedet_amd.models import FCOS
    cfg, params = _fcos_params()
    batch = {"data": _data(0), "im_info": IM_INFO}
    thr = cfg.TEST.CLS_THRESHOLD
    model = FCOS(cfg, params=params).eval()
    model(batch)
    pl = model._plan(N, *SIZE)
    logits, ctr = pl.logits.float(), torch.sigmoid(pl.raw[:, 4:5].float())
    d = _shift_for_fraction(lambda s: float((torch.sqrt(torch.sigmoid(logits + s) * ctr) > thr).float().mean()), 5e-2)
    params["head.cls_score.bias"] = params["head.cls_score.bias"] + np.float32(d)
    model = FCOS(cfg, params=params).eval()
    outs = model(batch)
    pl = model._plan(N, *SIZE)
    K = model.num_classes
    rows = pl.pyr.pix_per_img
    lvl_rows = [h * w for h, w in pl.sizes]
    assert lvl_rows == [320, 80, 20, 6, 2]
    info = torch.from_numpy(IM_INFO).cuda()
    per = []
    for i in range(N):
        lg = pl.logits.view(N, rows, K)[i]
        raw = pl.raw.view(N, rows, 8)[i]
        offs = pl.offsets.view(N, rows, 4)[i]
        scores = torch.empty((rows * K,), dtype=torch.float32, device="cuda")
        ops.det_scores(lg, rows, K, scores, ctr=raw, ctr_ld=8, ctr_off=4)
        ref = _single_image_chain(cfg, scores, lvl_rows, K, 1, info[i], 1000, anchors=pl.points, offsets=offs, off_ld=4, A=1)
        boxes = ob.point_decode(pl.points.cpu().numpy(), offs.float().cpu().numpy())
        per.append(dict(ref=ref, sc_l=_level_split(scores.cpu().numpy(), [r * K for r in lvl_rows]), bx_l=_level_split(boxes, lvl_rows)))
    _RUNS["fcos"] = (cfg, K, outs, per, 1000, (1e-5, 1e-3))
    return _RUNS["fcos"]


def _run_faster_rcnn():
    if "faster_rcnn" in _RUNS:
        return _RUNS["faster_rcnn"]
    from basedet_amd.models import FasterRCNN
    from tests.test_model_gpu import _frcnn_setup
    cfg, params, _ = _frcnn_setup(N, SIZE, seed=2)
    params["rcnn.pred_cls.weight"] = params["rcnn.pred_cls.weight"] * 5
    batch = {"data": _data(2), "im_info": IM_INFO}
    thr = cfg.TEST.CLS_THRESHOLD
    model = FasterRCNN(cfg, params=params).eval()
    model(batch)
    pl = model._cur
    K = model.num_classes
    R = pl.rois.shape[1]
    nrs = pl.num_rois.cpu().numpy()
    lg = torch.cat([pl.inf["raw"][i * R: i * R + int(nrs[i]), : K + 1] for i in range(N)]).double()

    def frac(s):            # background logit lowered by s
        x = lg.clone(); x[:, 0] -= s
        return float((torch.softmax(x, 1)[:, 1:] > thr).double().mean())
    d = _shift_for_fraction(frac, 0.05)
    params["rcnn.pred_cls.bias"] = params["rcnn.pred_cls.bias"].copy()
    params["rcnn.pred_cls.bias"][0] -= np.float32(d)
    model = FasterRCNN(cfg, params=params).eval()
    outs = model(batch)
    pl = model._cur
    assert pl.inf["raw"].shape[0] == N * R and pl.inf["scores"].numel() == N * R * K
    info = torch.from_numpy(IM_INFO).cuda()
    nrs = pl.num_rois.cpu().numpy()
    m = cfg.MODEL.RCNN_BOX_REG
    per = []
    for i in range(N):
        nr = int(nrs[i])
        assert 0 < nr <= R
        scores = pl.inf["scores"].view(N, R * K)[i]
        boxes = pl.inf["boxes"].view(N, R * K, 4)[i]
        ref = _single_image_chain(cfg, scores, [R], K, 2, info[i], 2048, item_boxes=boxes)
        raw = pl.inf["raw"].view(N, R, -1)[i].float().cpu().numpy()
        rois = pl.rois[i].cpu().numpy()
        dec = ob.box_decode(np.repeat(rois[:nr], K, axis=0), raw[:nr, K + 1: K + 1 + 4 * K].reshape(nr * K, 4), m.MEAN, m.STD)
        np.testing.assert_allclose(boxes.cpu().numpy()[: nr * K], dec, rtol=1e-5, atol=1e-3)
        sc = scores.cpu().numpy()
        assert np.all(sc[nr * K:] == -np.inf)
        per.append(dict(ref=ref, sc_l=[sc], bx_l=[boxes.cpu().numpy()]))
    _RUNS["faster_rcnn"] = (cfg, K, outs, per, 2048, (1e-4, 1e-2))
    return _RUNS["faster_rcnn"]


_RUNNERS = {"retinanet": _run_retinanet, "fcos": _run_fcos, "faster_rcnn": _run_faster_rcnn}


@pytest.mark.parametrize("name", ["retinanet", "fcos", "faster_rcnn"])
def test_batched_chain_is_bit_identical_to_the_single_image_ops(name):
    cfg, K, outs, per, k, _ = _RUNNERS[name]()
    assert isinstance(outs, list) and len(outs) == N
    counts = []
    for i in range(N):
        _assert_same_bits(outs[i], per[i]["ref"], f"{name} image {i}")
        counts.append((per[i]["ref"][3].tolist(), int(per[i]["ref"][1].shape[0])))
    print(f"{name} 3x128x160: (candidates per level, detections) per image {counts}")
    assert all(n > 10 for _, n in counts), "trivially few detections"
    if name != "faster_rcnn":      # (120 RoIs x 80 classes at 5 % are ~480 items: the 2048 cut cannot occur at this size; it is the full-size test's regime)
        assert any(max(c) == k for c, _ in counts), "no level is cut at its top-k"
        assert any(0 < min(x for x in c if x) < k for c, _ in counts), "every level is cut"
    # per-image im_info: identical candidates would still come out differently scaled -- the clip bound of every image is its own
    for i in range(N):
        b = torch.as_tensor(outs[i]["boxes"]).float()
        assert float(b[:, 0::2].max()) <= IM_INFO[i, 3] and float(b[:, 1::2].max()) <= IM_INFO[i, 2]


@pytest.mark.parametrize("name", ["retinanet", "fcos", "faster_rcnn"])
def test_batched_inference_matches_oracle_per_image(name):
    cfg, K, outs, per, k, tol = _RUNNERS[name]()
    for i in range(N):
        n = _compare_oracle(outs[i], per[i]["sc_l"], per[i]["bx_l"], K, cfg, k, tol, IM_INFO[i, :4])
        assert n > 10


@pytest.mark.parametrize("coder", ["A", "B"])
def test_batched_retinanet_decodes_with_box_reg(coder):
    """MODEL.BOX_REG with a non-zero mean (A) and with four different stds (B) through bd_det_candidates at B = 3: three images, bit-identical
    to the single-image operators under the same coder and, per image, the oracle's detections (box_decode with that mean and std)."""
    from tests import config_key_cases as C
    cfg, K, outs, per, k, tol = _run_retinanet("retinanet_coder_" + coder, dict(MODEL=dict(BOX_REG=dict(A=C.CODER_A, B=C.CODER_B)[coder])))
    assert list(cfg.MODEL.BOX_REG.STD) == list(dict(A=C.BOX_CODER_A, B=C.BOX_CODER_B)[coder][1])
    for i in range(N):
        _assert_same_bits(outs[i], per[i]["ref"], f"coder {coder} image {i}")
        assert _compare_oracle(outs[i], per[i]["sc_l"], per[i]["bx_l"], K, cfg, k, tol, IM_INFO[i, :4]) > 10


def test_an_image_without_detections_between_two_with():
    """The classification bias is placed between the highest logit of the image that has the lowest one and the next image's: that image
    comes out as the empty Container, its neighbours as the single-image operators give them."""
    from basedet_amd import ops
    from basedet_amd.models import RetinaNet
    cfg, params = _retinanet_params()
    data = _data(5)
    data[1] = data[1] * 0.05 + 110.0           # a flat grey image in the middle: its logits spread far less
    batch = {"data": data, "im_info": IM_INFO}
    thr = cfg.TEST.CLS_THRESHOLD
    model = RetinaNet(cfg, params=params).eval()
    model(batch)
    pl = model._plan(N, *SIZE)
    K, A = model.num_classes, model.num_anchors
    rows = pl.pyr.pix_per_img * A
    mx = pl.logits.float().view(N, -1).max(dim=1).values.cpu().numpy()
    order = np.argsort(mx)
    e = int(order[0])
    gap = float(mx[order[1]] - mx[e])
    # the shifted maxima land near logit(0.05) = -2.94, where a bf16 step is 2^-6: half the gap must be a few such steps, so that the
    # rounding of the shifted logits cannot move either maximum across the threshold (the counts are asserted below in any case)
    assert 0.5 * gap >= 4 * 2.0 ** -6, f"per-image maxima {mx.tolist()} too close for a bf16-safe cut"
    x_thr = float(np.log(thr / (1 - thr)))
    params["head.cls_score.bias"] = params["head.cls_score.bias"] + np.float32(x_thr - (mx[e] + 0.5 * gap))
    model = RetinaNet(cfg, params=params).eval()
    outs = model(batch)
    assert isinstance(outs, list) and len(outs) == N
    pl = model._plan(N, *SIZE)
    info = torch.from_numpy(IM_INFO).cuda()
    m = cfg.MODEL.BOX_REG
    lvl_rows = [h * w * A for h, w in pl.sizes]
    for i in range(N):
        scores = torch.empty((rows * K,), dtype=torch.float32, device="cuda")
        ops.det_scores(pl.logits.view(N, rows, K)[i], rows, K, scores)
        above = int((scores > thr).sum())
        ref = _single_image_chain(cfg, scores, lvl_rows, K, 0, info[i], 1000, anchors=pl.anchors,
                                  offsets=pl.offsets.view(N, pl.pyr.pix_per_img, -1)[i], off_ld=model.box_ld, A=A, mean=m.MEAN, std=m.STD)
        _assert_same_bits(outs[i], ref, f"image {i}")
        if i == e:
            assert above == 0
            o = outs[i]
            assert o["boxes"].numel() == 0 and o["box_scores"].numel() == 0 and o["box_labels"].numel() == 0
            assert not o["boxes"].is_cuda          # the same empty Container as single-image inference returns
        else:
            assert above > 0 and outs[i]["box_scores"].numel() > 0


def test_return_types():
    """inference on one image: a Container; inference_batch on it: a one-element list with the same tensors; on three: a list."""
    from basedet_amd.models import RetinaNet
    from basedet_amd.structures import Container
    cfg, params = _retinanet_params()
    params["head.cls_score.bias"] = np.full_like(params["head.cls_score.bias"], -2.5)
    data = _data(5)
    model = RetinaNet(cfg, params=params).eval()
    one = {"data": data[:1], "im_info": IM_INFO[:1]}
    out = model.inference(one)
    assert isinstance(out, Container) and not isinstance(out, list)
    assert out["box_scores"].numel() > 0
    lst = model.inference_batch(one)
    assert isinstance(lst, list) and len(lst) == 1 and isinstance(lst[0], Container)
    for key in ("boxes", "box_scores", "box_labels"):
        assert torch.equal(torch.as_tensor(lst[0][key]), torch.as_tensor(out[key])), key
    assert out["box_scores"].data_ptr() != lst[0]["box_scores"].data_ptr(), "a later call must not overwrite an earlier result"
    three = model.inference({"data": data, "im_info": IM_INFO})
    assert isinstance(three, list) and len(three) == N and all(isinstance(o, Container) for o in three)
    assert len(model._det_scratch) == 2            # one scratch set per (N, L, k), reused by the repeated calls


@pytest.mark.parametrize("name", ["ATSS", "FreeAnchor"])
def test_inherited_heads_take_batches(name):
    """ATSS inherits FCOS's inference, FreeAnchor RetinaNet's: a batch of three gives three Containers equal to inference_batch's."""
    from basedet_amd import configs, models
    from basedet_amd.models import params as P
    if name == "ATSS":
        cfg = configs.ATSSConfig()
        cfg.MODEL.BATCHSIZE = N
        params = P.init_fcos_params(cfg, seed=0, residual_gamma=0.25)
        params["head.cls_score.bias"] = np.full_like(params["head.cls_score.bias"], -1.0)
        params["head.cls_score.weight"] = params["head.cls_score.weight"] * 8
        params["head.bbox_pred.bias"] = np.full_like(params["head.bbox_pred.bias"], 1.5)
    else:
        cfg = configs.FreeAnchorConfig()
        cfg.MODEL.BATCHSIZE = N
        params = P.init_retinanet_params(cfg, seed=0, residual_gamma=0.25)
        params["head.cls_score.bias"] = np.full_like(params["head.cls_score.bias"], -2.5)
        params["head.cls_score.weight"] = params["head.cls_score.weight"] * 8
    model = getattr(models, name)(cfg, params=params).eval()
    outs = model({"data": _data(0), "im_info": IM_INFO})
    assert isinstance(outs, list) and len(outs) == N
    assert sum(o["box_scores"].numel() for o in outs) > 0
    again = model.inference_batch({"data": _data(0), "im_info": IM_INFO})
    for a, b in zip(outs, again):
        assert torch.equal(torch.as_tensor(a["box_scores"]), torch.as_tensor(b["box_scores"]))
