"""csrc/yolox.hip against tests/yolox_oracle.py: SimOTA assignment, the four losses with gradients, the inference decode and the Python
surface.  Operands live in guarded() allocations (tests/util.py) whose guards are checked; every launch runs twice and must repeat its
bits."""
import math

import numpy as np
import pytest
import torch

import util as U
import yolox_oracle as O
from basedet_amd import ops

pytestmark = pytest.mark.gpu
BF, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8


def _in(data, name, fill="nan"):
    """A guarded device copy of data; int32 data travels in a float32 allocation of the same bits (guarded() knows float formats)."""
    data = data.contiguous()
    rows, cols = (data.shape[0], None) if data.dim() == 1 else (data.shape[0], int(np.prod(data.shape[1:])))
    is_int = data.dtype == I32
    t, h = U.guarded(rows, cols, F32 if is_int else data.dtype, "cuda", fill=fill, name=name)
    if is_int:
        U.bits_of(h.t).copy_(data.view_as(h.t))
        t = h.t.view(I32)
    else:
        h.set(data)
    return t, h.snapshot()


def _out(rows, cols, dtype, name):
    t, h = U.guarded(rows, cols, F32 if dtype == I32 else dtype, "cuda", name=name)
    return (t.view(I32) if dtype == I32 else t), h


def _twice(launch, outs, ins):
    """Run launch() twice on sentinel-filled outputs: the guards hold, the inputs come back unchanged, the two results have the same bits."""
    res = []
    for _ in range(2):
        for t, h in outs:
            U.bits_of(h.t).copy_(U.fill_pattern(h.dtype, "sentinel", h.t.numel(), "cuda").view_as(U.bits_of(h.t)))
        launch()
        torch.cuda.synchronize()
        for _, h in outs:
            h.check()
        for h in ins:
            h.assert_unchanged()
        res.append([U.bits_of(t).clone() for t, _ in outs])
    for a, b in zip(*res):
        assert torch.equal(a, b), "the launch is not reproducible"


def _operands(prob):
    """Guarded device operands of a problem: (dict of tensors, [input handles])."""
    N, P = prob["cls"].shape[:2]
    t, hs = {}, []
    for name, data in (("cls", torch.from_numpy(prob["cls"]).to(BF).reshape(N * P, -1)),
                       ("box_obj", torch.from_numpy(prob["box_obj"]).to(BF).reshape(N * P, 8)),
                       ("points", torch.from_numpy(prob["pts"])), ("gt", torch.from_numpy(prob["gt"]).reshape(N, -1))):
        t[name], h = _in(data, name)
        hs.append(h)
    t["num"], h = _in(torch.from_numpy(prob["num"]), "num_gt", fill="zero")
    hs.append(h)
    t["gt"] = t["gt"].view(N, -1, 5)
    return t, hs


def _assign(prob):
    N, P = prob["cls"].shape[:2]
    t, hs = _operands(prob)
    outs = [_out(N * P, None, I32, "matched"), _out(N * P, None, F32, "iou_t"), _out(1, None, F32, "stats")]
    (matched, _), (iou_t, _), (stats, _) = outs
    ws = torch.empty(ops.yolox_assign_workspace_bytes(N, P), dtype=U8, device="cuda")
    _twice(lambda: ops.yolox_assign_into(t["cls"], prob["K"], t["box_obj"], t["points"], prob["lvl_start"], prob["strides"], t["gt"], t["num"],
                                         matched.view(N, P), iou_t.view(N, P), stats, ws), outs, hs)
    return matched.view(N, P).cpu().numpy().astype(np.int64), iou_t.view(N, P).cpu().numpy(), float(stats[0])


def _check_assignment(prob, ref, got, name):
    m_o, u_o, aux = ref
    m, u, nfg_dev = got
    G = np.minimum(np.maximum(prob["num"], 0), prob["gt"].shape[1])
    assert ((m >= -1) & (m < G[:, None])).all()
    assert nfg_dev == (m >= 0).sum()
    assert (u[m < 0] == 0).all() and np.isfinite(u).all()
    nfg, cap, diff = O.compare(prob, ref, m)
    print(f"assign {name}: foreground {nfg}, differing {len(diff)} (cap {cap}) {diff}")
    assert len(diff) <= cap, (len(diff), cap)
    assert all(e is not None for _, _, e in diff), diff
    same = (m == m_o) & (m_o >= 0)
    if same.any():
        err = np.abs(u.astype(np.float64) - u_o)[same].max()
        print(f"assign {name}: iou_t max err 2^{math.log2(max(err, 1e-30)):.1f}")
        assert err <= 2.0 ** -12


@pytest.mark.parametrize("shape", O.SHAPES)
def test_assign(shape):
    prob = O.problem(shape)
    assert prob["pts"].shape[0] == {64: 84, 96: 315, 256: 1344, 640: 8400}[shape[1]]
    _check_assignment(prob, O.reference(shape), _assign(prob), shape)


def test_assign_edge_gts():
    prob = O.edge_problem()
    ref = O.reference("edge")
    got = _assign(prob)
    _check_assignment(prob, ref, got, "edge")
    assert (got[0][1] == -1).all()                                   # the image whose only gt has no candidate
    assert not (got[0][0] == 3).any()                                # the duplicate never beats the lower index


def test_assign_all_empty():
    prob = O.empty_problem()
    m, u, nfg = _assign(prob)
    assert (m == -1).all() and (u == 0).all() and nfg == 0


def test_assign_extremes():
    """Logits of +-20 / +-40 and raw w / h of +-8: every output finite, every foreground point a candidate, every index valid."""
    prob = O.extremes_problem()
    m, u, nfg = _assign(prob)
    assert np.isfinite(u).all() and (u >= 0).all() and (u <= 1).all()
    G = prob["num"]
    assert ((m >= -1) & (m < G[:, None])).all() and nfg == (m >= 0).sum() > 0
    for n in range(m.shape[0]):
        g = int(G[n])
        if g == 0:
            assert (m[n] == -1).all()
            continue
        in_box, in_ctr = O.in_tests(prob["pts"], prob["stride"], prob["gt"][n, :g])
        assert (in_box | in_ctr).any(0)[m[n] >= 0].all()


def _loss(prob, matched, iou_t, nf, use_l1):
    N, P = prob["cls"].shape[:2]
    K = prob["K"]
    t, hs = _operands(prob)
    mt, hm = _in(torch.from_numpy(matched.astype(np.int32)).reshape(-1), "matched", fill="zero")
    ut, hu = _in(torch.from_numpy(iou_t.astype(np.float32)).reshape(-1), "iou_t")
    st, hst = _in(torch.tensor([float(nf)]), "stats")
    outs = [_out(4, None, F32, "loss_out"), _out(N * P, t["cls"].shape[1], BF, "d_cls"), _out(N * P, 8, BF, "d_box_obj")]
    (loss, _), (d_cls, _), (d_box, _) = outs
    ws = torch.empty(ops.yolox_loss_workspace_bytes(), dtype=U8, device="cuda")
    _twice(lambda: ops.yolox_loss_fwd_bwd_into(t["cls"], K, t["box_obj"], t["points"], prob["lvl_start"], prob["strides"], t["gt"],
                                               mt.view(N, P), ut.view(N, P), st, use_l1, 1.0, loss, d_cls, d_box, ws),
           outs, hs[:4] + [hm, hu, hst])
    return loss.cpu().numpy(), d_cls.view(N, P, -1), d_box.view(N, P, 8)


NF = 4.0            # a small constant normaliser: the gradients stay above the atol of the comparison


@pytest.mark.parametrize("use_l1", [False, True])
@pytest.mark.parametrize("shape", O.SHAPES)
def test_loss(shape, use_l1):
    prob = O.problem(shape)
    K = prob["K"]
    m_o, u_o, _ = O.reference(shape)
    ref_loss, ref_dc, ref_db = O.losses(prob, m_o, u_o, NF, use_l1)
    loss, d_cls, d_box = _loss(prob, m_o, u_o, NF, use_l1)
    for j, name in enumerate(("iou", "obj", "cls", "l1")):
        if name == "l1" and not use_l1:
            assert loss[j] == 0
            continue
        rel = abs(float(loss[j]) - ref_loss[j]) / abs(ref_loss[j])
        print(f"loss {shape} l1={use_l1} {name}: {loss[j]:.6f} vs {ref_loss[j]:.6f}, rel err 2^{math.log2(max(rel, 1e-30)):.1f}")
        assert rel <= 2.0 ** -16, (name, float(loss[j]), ref_loss[j])
    assert np.allclose(d_cls[..., :K].float().cpu().numpy(), ref_dc, rtol=3e-2, atol=2e-6)
    assert np.allclose(d_box[..., :5].float().cpu().numpy(), ref_db, rtol=3e-2, atol=2e-6)
    bg = torch.from_numpy(m_o < 0).cuda()
    assert int((U.bits_of(d_cls)[bg] != 0).sum()) == 0                # background rows: exactly +0
    assert int((U.bits_of(d_cls)[..., K:] != 0).sum()) == 0 and int((U.bits_of(d_box)[..., 5:] != 0).sum()) == 0
    assert int((U.bits_of(d_box)[bg][:, :4] != 0).sum()) == 0


def test_loss_all_empty():
    """Every num_gt == 0: the obj loss alone, with nf == 1."""
    prob = O.empty_problem()
    m_o, u_o, _ = O.reference("empty")
    ref_loss, ref_dc, ref_db = O.losses(prob, m_o, u_o, 0.0, True)
    loss, d_cls, d_box = _loss(prob, m_o, u_o, 0.0, True)
    assert loss[0] == 0 and loss[2] == 0 and loss[3] == 0
    assert abs(float(loss[1]) - ref_loss[1]) / ref_loss[1] <= 2.0 ** -16
    assert int((U.bits_of(d_cls) != 0).sum()) == 0
    assert np.allclose(d_box[..., :5].float().cpu().numpy(), ref_db, rtol=3e-2, atol=2e-6)


# ---- inference --------------------------------------------------------------------------------------------------------------------------
CAND_CASES = [(1, 96, 160, 3, 0.001), (3, 96, 160, 3, 0.001), (1, 256, 256, 80, 0.5), (3, 256, 256, 80, 0.5)]
TOPK = 1000


def _select_ref(prob, thr):
    sc = O.scores(prob)
    assert np.abs(sc - thr).min() > 1e-6                              # no score sits on the threshold
    sel = O.select(prob, thr, TOPK)
    K = prob["K"]
    assert all(len(idx) < TOPK or len(prob["pts"]) * K <= TOPK for lv in sel for idx, _ in lv)
    return sel


@pytest.mark.parametrize("B,H,W,K,thr", CAND_CASES)
def test_candidates(B, H, W, K, thr):
    prob = O.inference_problem(B, H, W, K)
    sel = _select_ref(prob, thr)
    P, L = prob["pts"].shape[0], len(prob["sizes"])
    t, hs = _operands(prob)
    lvl_rows = [h * w for h, w in prob["sizes"]]
    i32, f32 = dict(dtype=I32, device="cuda"), dict(dtype=F32, device="cuda")
    tk_idx, tk_sc, tk_cnt = torch.empty((B, L, TOPK), **i32), torch.empty((B, L, TOPK), **f32), torch.empty((B, L), **i32)
    ws = torch.empty(ops.det_select_workspace_bytes(B, L, P, K, TOPK), dtype=U8, device="cuda")
    ops.det_select(t["cls"], B, P, K, prob["lvl_start"][:-1], lvl_rows, TOPK, thr, tk_idx, tk_sc, tk_cnt, ws, ctr=t["box_obj"], ctr_ld=8,
                   ctr_off=4, ld=O.ld_of(K))
    outs = [_out(B * L * TOPK, 4, F32, "boxes"), _out(B * L * TOPK, None, F32, "scores"), _out(B * L * TOPK, None, I32, "labels")]
    (boxes, _), (scores, _), (labels, _) = outs
    _twice(lambda: ops.yolox_candidates_into(tk_idx, tk_sc, tk_cnt, K, t["points"], prob["lvl_start"], prob["strides"], t["box_obj"],
                                             boxes.view(B, L * TOPK, 4), scores.view(B, L * TOPK), labels.view(B, L * TOPK)), outs, hs[:3])
    idx, cnt = tk_idx.cpu().numpy(), tk_cnt.cpu().numpy()
    bx, sc, lab = boxes.view(B, L, TOPK, 4).cpu().numpy(), scores.view(B, L, TOPK).cpu().numpy(), labels.view(B, L, TOPK).cpu().numpy()
    want_boxes = O.boxes_xyxy(prob)
    total = 0
    for b in range(B):
        for l in range(L):
            c = int(cnt[b, l])
            want_idx, want_sc = sel[b][l]
            assert c == len(want_idx) and sorted(idx[b, l, :c].tolist()) == sorted(want_idx.tolist())
            rows = prob["lvl_start"][l] + idx[b, l, :c] // K
            np.testing.assert_array_equal(lab[b, l, :c], idx[b, l, :c] % K)
            np.testing.assert_allclose(bx[b, l, :c], want_boxes[b, rows], rtol=2.0 ** -8, atol=2.0 ** -8)
            np.testing.assert_array_equal(sc[b, l, :c], tk_sc[b, l, :c].cpu().numpy())
            assert (sc[b, l, c:] == -np.inf).all() and (bx[b, l, c:] == 0).all() and (lab[b, l, c:] == 0).all()
            total += c
    assert total >= 20 * B


def _nchw_lists(prob):
    N, K = prob["cls"].shape[0], prob["K"]
    lg, of, ob = [], [], []
    for (h, w), a, b in zip(prob["sizes"], prob["lvl_start"][:-1], prob["lvl_start"][1:]):
        lg.append(torch.from_numpy(prob["cls"][:, a:b, :K]).float().reshape(N, h, w, K).permute(0, 3, 1, 2).contiguous().cuda())
        of.append(torch.from_numpy(prob["box_obj"][:, a:b, :4]).float().reshape(N, h, w, 4).permute(0, 3, 1, 2).contiguous().cuda())
        ob.append(torch.from_numpy(prob["box_obj"][:, a:b, 4:5]).float().reshape(N, h, w, 1).permute(0, 3, 1, 2).contiguous().cuda())
    return lg, of, ob


@pytest.mark.parametrize("H,W,K,thr", [(96, 160, 3, 0.001), (256, 256, 80, 0.5)])
def test_inference_end_to_end(H, W, K, thr):
    """yolox_inference against the oracle's threshold and decode followed by the project's NMS reference (oracle/box_ops.py) and the
    rescale + clip of post_processing; the B = 3 result equals three B = 1 calls bit for bit."""
    from basedet.configs import YOLOXConfig
    from basedet.models.yolox import yolox_inference
    from oracle import box_ops
    B = 3
    prob = O.inference_problem(B, H, W, K)
    sel = _select_ref(prob, thr)
    cfg = YOLOXConfig()
    cfg.TEST.CLS_THRESHOLD = thr
    lg, of, ob = _nchw_lists(prob)
    info = torch.tensor([[H, W, H * 1.5, W * 1.25]] * B, dtype=F32, device="cuda")
    outs = yolox_inference(lg, of, ob, info, cfg)
    want_boxes = O.boxes_xyxy(prob)
    for b in range(B):
        rows = np.concatenate([prob["lvl_start"][l] + sel[b][l][0] // K for l in range(3)])
        labs = np.concatenate([sel[b][l][0] % K for l in range(3)])
        scs = np.concatenate([sel[b][l][1] for l in range(3)]).astype(np.float32)
        cb = want_boxes[b, rows].astype(np.float32)
        keep = box_ops.batched_nms(cb, scs, labs, cfg.TEST.IOU_THRESHOLD, cfg.TEST.MAX_BOXES_PER_IMAGE)
        fb = cb[keep].astype(np.float64) * np.array([1.25, 1.5, 1.25, 1.5])
        fb = np.clip(fb, 0, np.array([W * 1.25, H * 1.5, W * 1.25, H * 1.5]))
        got = outs[b]
        assert len(keep) >= 3 and len(got.box_scores) == len(keep)
        np.testing.assert_array_equal(got.box_labels.cpu().numpy(), labs[keep])
        np.testing.assert_allclose(got.box_scores.cpu().numpy(), scs[keep], rtol=1e-6, atol=1e-7)
        gb = got.boxes._raw().cpu().numpy()
        np.testing.assert_allclose(gb, fb, rtol=2.0 ** -8, atol=2.0 ** -8)
        one = yolox_inference([x[b:b + 1].contiguous() for x in lg], [x[b:b + 1].contiguous() for x in of],
                              [x[b:b + 1].contiguous() for x in ob], info[b:b + 1].contiguous(), cfg)[0]
        ob1 = one.boxes._raw().cpu().numpy()
        assert np.array_equal(U.bits_of(torch.from_numpy(gb)).numpy(), U.bits_of(torch.from_numpy(ob1)).numpy())
        assert torch.equal(one.box_scores, got.box_scores) and torch.equal(one.box_labels, got.box_labels)


def test_python_surface_matches_the_entries():
    """yolox_losses on the reference's NCHW lists equals the entry-level result bit for bit, and backward() delivers the kernel's
    gradients; yolox_assignments is the entry; FastPointGenerator on the device equals its host grid."""
    from basedet.layers import FastPointGenerator
    from basedet.models.yolox import pack_head_outputs, yolox_assignments, yolox_losses
    shape = O.SHAPES[1]
    prob = O.problem(shape)
    N, P, K = prob["cls"].shape[0], prob["pts"].shape[0], prob["K"]
    lg, of, ob = _nchw_lists(prob)
    gen = FastPointGenerator(prob["strides"])
    pts = gen(lg)
    for a, b in zip(pts, gen.grid(prob["sizes"])):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    cls, box_obj, sizes = pack_head_outputs(lg, of, ob)
    assert sizes == prob["sizes"]
    np.testing.assert_array_equal(cls.float().cpu().numpy().reshape(N, P, -1)[..., :K], prob["cls"][..., :K])
    np.testing.assert_array_equal(box_obj.float().cpu().numpy().reshape(N, P, 8)[..., :5], prob["box_obj"][..., :5])
    gt, num = torch.from_numpy(prob["gt"]).cuda(), torch.from_numpy(prob["num"]).cuda()
    matched, iou_t, stats = yolox_assignments(cls, box_obj, pts, prob["strides"], gt, num, K=K)
    m_o = O.reference(shape)[0]
    assert (matched.cpu().numpy() == m_o).mean() > 0.99 and float(stats[0]) == int((matched >= 0).sum())
    loss4, d_cls, d_box = ops.yolox_loss_fwd_bwd(cls, K, box_obj, torch.cat(pts), prob["lvl_start"], prob["strides"], gt, matched, iou_t, stats,
                                                 use_l1=True)
    for x in lg + of + ob:
        x.requires_grad_(True)
    out = yolox_losses(lg, of, ob, gt, num, prob["strides"], use_l1=True)
    assert set(out) == {"total_loss", "iou_loss", "l1_loss", "obj_loss", "cls_loss"}
    for key, j in (("iou_loss", 0), ("obj_loss", 1), ("cls_loss", 2), ("l1_loss", 3)):
        assert float(out[key]) == float(loss4[j]) > 0
    assert float(out["total_loss"].detach()) == float(loss4.sum())
    assert float(yolox_losses(lg, of, ob, gt, num, prob["strides"])["l1_loss"]) == 0
    (out["total_loss"] * 2.0).backward()
    dc, db = d_cls.view(N, P, -1).float(), d_box.view(N, P, 8).float()
    for l, (h, w) in enumerate(prob["sizes"]):
        a, b = prob["lvl_start"][l], prob["lvl_start"][l + 1]
        assert torch.equal(lg[l].grad, 2.0 * dc[:, a:b, :K].reshape(N, h, w, K).permute(0, 3, 1, 2))
        assert torch.equal(of[l].grad, 2.0 * db[:, a:b, :4].reshape(N, h, w, 4).permute(0, 3, 1, 2))
        assert torch.equal(ob[l].grad, 2.0 * db[:, a:b, 4:5].reshape(N, h, w, 1).permute(0, 3, 1, 2))
    assert float(lg[0].grad.abs().sum()) > 0 and float(of[0].grad.abs().sum()) > 0


def test_entries_refuse_bad_arguments():
    """BD_EINVAL before any launch: ld not round_up(K, 8), L out of range, a short workspace, a null pointer."""
    from basedet_amd._lib import BasedetHipError
    prob = O.problem(O.SHAPES[0])
    N, P, K = 1, prob["pts"].shape[0], 1
    dev = "cuda"
    cls, box_obj = torch.zeros((N * P, 8), dtype=BF, device=dev), torch.zeros((N * P, 8), dtype=BF, device=dev)
    pts = torch.from_numpy(prob["pts"]).to(dev)
    gt, num = torch.from_numpy(prob["gt"]).to(dev), torch.from_numpy(prob["num"]).to(dev)
    matched, iou_t = torch.full((N, P), -7, dtype=I32, device=dev), torch.full((N, P), -7.0, dtype=F32, device=dev)
    stats = torch.full((1,), -7.0, dtype=F32, device=dev)
    ws = torch.empty(ops.yolox_assign_workspace_bytes(N, P), dtype=U8, device=dev)
    lws = torch.empty(ops.yolox_loss_workspace_bytes(), dtype=U8, device=dev)
    loss, d_cls, d_box = torch.full((4,), -7.0, dtype=F32, device=dev), torch.empty_like(cls), torch.empty_like(box_obj)
    start, strides = prob["lvl_start"], prob["strides"]

    def assign(cls_=cls, K_=K, start_=start, strides_=strides, ws_=ws, matched_=matched):
        ops.yolox_assign_into(cls_, K_, box_obj, pts, start_, strides_, gt, num, matched_, iou_t, stats, ws_)

    def lossf(cls_=cls, K_=K, start_=start, strides_=strides, ws_=lws, d_cls_=d_cls):
        ops.yolox_loss_fwd_bwd_into(cls_, K_, box_obj, pts, start_, strides_, gt, matched, iou_t, stats, False, 1.0, loss, d_cls_, d_box, ws_)
    wide = torch.zeros((N * P, 12), dtype=BF, device=dev)
    nine = [0] + [P] * 9
    for fn in (assign, lossf):
        for kw in (dict(cls_=wide, K_=9), dict(K_=9), dict(start_=nine, strides_=[8] * 9), dict(start_=[0], strides_=[]), dict(ws_=ws[:64])):
            with pytest.raises(BasedetHipError):
                fn(**kw)
    with pytest.raises(BasedetHipError):
        assign(matched_=None)
    with pytest.raises(BasedetHipError):
        lossf(d_cls_=None)
    tk = torch.zeros((1, 3, 4), dtype=I32, device=dev)
    with pytest.raises(BasedetHipError):
        ops.yolox_candidates_into(tk, tk.float(), torch.zeros((1, 3), dtype=I32, device=dev), K, pts, start, strides, None,
                                  torch.empty((1, 12, 4), device=dev), torch.empty((1, 12), device=dev), torch.empty((1, 12), dtype=I32, device=dev))
    tk9 = torch.zeros((1, 9, 4), dtype=I32, device=dev)
    with pytest.raises(BasedetHipError):
        ops.yolox_candidates_into(tk9, tk9.float(), torch.zeros((1, 9), dtype=I32, device=dev), K, pts, nine, [8] * 9, box_obj,
                                  torch.empty((1, 36, 4), device=dev), torch.empty((1, 36), device=dev), torch.empty((1, 36), dtype=I32, device=dev))
    torch.cuda.synchronize()
    assert (matched == -7).all() and (iou_t == -7).all() and float(stats[0]) == -7 and (loss == -7).all()      # nothing was launched
