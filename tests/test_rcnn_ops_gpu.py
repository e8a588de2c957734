"""GPU parity of the Faster R-CNN operators (csrc/rcnn_ops.hip, csrc/nms.hip, RPN / RCNN losses) against oracle/rcnn_ops.py.
Index-valued outputs (top-k order, NMS survivors, sampled labels / RoIs) are compared bit-exactly; RoIAlign within one
bf16 ulp; the losses against a float64 restatement with the tolerance written at each assert."""
import numpy as np
import pytest
import torch

from oracle import box_ops as ob
from oracle import rcnn_ops as orc
from tests.config_key_cases import BOX_CODER_0 as CODER_0, BOX_CODER_A as CODER_A, BOX_CODER_B as CODER_B

pytestmark = pytest.mark.gpu

STRIDES = [4, 8, 16, 32, 64]


def _ops():
    from basedet_amd import ops
    return ops


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def _geom(N, sizes):
    from basedet_amd.ops import Geom
    return Geom(N, [s[0] for s in sizes], [s[1] for s in sizes])


def _rand_boxes(rng, n, W, H, min_size=2.0, max_size=300.0):
    cx = rng.uniform(0, W, n); cy = rng.uniform(0, H, n)
    w = rng.uniform(min_size, max_size, n); h = rng.uniform(min_size, max_size, n)
    b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    b[:, 0::2] = np.clip(b[:, 0::2], 0, W); b[:, 1::2] = np.clip(b[:, 1::2], 0, H)
    return b.astype(np.float32)


def _gt(rng, N, Gmax, W, H):
    gt = np.zeros((N, Gmax, 5), np.float32)
    num = rng.integers(1, Gmax + 1, N).astype(np.int32)
    for n in range(N):
        b = _rand_boxes(rng, num[n], W, H, 20, 250)
        gt[n, : num[n], :4] = b
        gt[n, : num[n], 4] = rng.integers(1, 81, num[n])
    return gt, num


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_segment_topk(dtype):
    ops = _ops()
    rng = np.random.default_rng(0)
    B, A, ldc, coff, k = 3, 3, 16, 1, 2000
    rows = [5000, 900, 300, 40]              # 15000, 2700, 900, 120 items
    starts = np.concatenate([[0], np.cumsum(rows)[:-1]]).astype(np.int32)
    ppi = int(sum(rows))
    raw = rng.normal(0, 1, (B, ppi, ldc)).astype(np.float32)
    if dtype == "bf16":
        t = _bf16(raw)
        raw = t.float().numpy()
        dev = t.cuda()
    else:
        raw = np.round(raw * 64) / 64        # plenty of ties
        dev = _dev(raw)
    out_idx = torch.empty((B, len(rows), k), dtype=torch.int32, device="cuda")
    out_sc = torch.empty((B, len(rows), k), dtype=torch.float32, device="cuda")
    out_cnt = torch.empty((B, len(rows)), dtype=torch.int32, device="cuda")
    for min_score in (None, 0.5):
        ops.segment_topk(dev, B, ppi * ldc, A, ldc, coff, starts.tolist(), rows, k, out_idx, out_sc, out_cnt, min_score=min_score)
        gi, gs, gc = out_idx.cpu().numpy(), out_sc.cpu().numpy(), out_cnt.cpu().numpy()
        for b in range(B):
            for s, (st, r) in enumerate(zip(starts, rows)):
                sc = raw[b, st:st + r, coff:coff + A].reshape(-1)
                ri, rs = orc.topk_desc(sc, k, min_score)
                assert gc[b, s] == len(ri)
                assert np.array_equal(gi[b, s, : len(ri)], ri)
                assert np.array_equal(gs[b, s, : len(ri)], rs)
                assert np.all(gi[b, s, len(ri):] == -1)


def test_nms_batched():
    ops = _ops()
    rng = np.random.default_rng(1)
    B, C = 3, 3000
    boxes = np.stack([_rand_boxes(rng, C, 1344, 800, 8, 200) for _ in range(B)])
    # clustered boxes so that a large fraction is suppressed
    boxes[:, 1000:2000] = boxes[:, :1000] + rng.normal(0, 3, (B, 1000, 4)).astype(np.float32)
    scores = rng.uniform(0, 1, (B, C)).astype(np.float32)
    scores = np.round(scores * 512) / 512
    scores[1, 100:400] = -np.inf
    idxs = rng.integers(0, 5, (B, C)).astype(np.int32)
    for max_out in (1000, 0, 17):
        cap = max_out if max_out > 0 else C
        keep = torch.full((B, cap), -1, dtype=torch.int32, device="cuda")
        num = torch.zeros((B,), dtype=torch.int32, device="cuda")
        ws = torch.empty((ops.nms_batched_workspace_bytes(B, C),), dtype=torch.uint8, device="cuda")
        ops.nms_batched(_dev(boxes), _dev(scores), _dev(idxs), 0.7, max_out, keep, num, ws)
        gk, gn = keep.cpu().numpy(), num.cpu().numpy()
        for b in range(B):
            valid = np.nonzero(scores[b] > -np.inf)[0]
            ref = ob.batched_nms(boxes[b][valid], scores[b][valid], idxs[b][valid], 0.7, max_out if max_out > 0 else None)
            ref = valid[ref]
            assert gn[b] == len(ref)
            assert np.array_equal(gk[b, : gn[b]], ref)


def _nms_batched_one(ops, boxes, scores, idxs, thr, max_output):
    """ops.nms_batched on one problem: its keep list"""
    n = len(scores)
    keep = torch.full((1, max_output or n), -1, dtype=torch.int32, device="cuda")
    num = torch.zeros((1,), dtype=torch.int32, device="cuda")
    ws = torch.empty((ops.nms_batched_workspace_bytes(1, n),), dtype=torch.uint8, device="cuda")
    ops.nms_batched(_dev(boxes[None]), _dev(scores[None]), _dev(idxs[None]), thr, max_output or 0, keep, num, ws)
    return keep.cpu().numpy()[0, : int(num.item())]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 700])
def test_nms_public_entries_agree(n):
    """bd_batched_nms (one problem, every item present) and bd_nms_batched with B = 1 run the same kernels: on finite scores both return
    the oracle's keep list.  The sizes are the chunk boundaries of the 64-wide tiles and the one-word case; scores rounded to 1/512 tie."""
    ops = _ops()
    rng = np.random.default_rng(100 + n)
    boxes = _rand_boxes(rng, n, 1344, 800, 40, 200)
    scores = (np.round(rng.uniform(0, 1, n) * 512) / 512).astype(np.float32)
    idxs = rng.integers(0, 5, n).astype(np.int32)
    h = n // 2                                # clustered, a cluster in one class: about half of the boxes is suppressed
    boxes[h:2 * h] = boxes[:h] + rng.normal(0, 2, (h, 4)).astype(np.float32)
    idxs[h:2 * h] = idxs[:h]
    for max_output in (None, 1, 17):
        ref = ob.batched_nms(boxes, scores, idxs, 0.7, max_output)
        if max_output is None and n == 700:
            assert 0.4 * n < len(ref) < 0.7 * n          # (the clusters do suppress)
        one = ops.batched_nms(_dev(boxes), _dev(scores), _dev(idxs), 0.7, max_output).cpu().numpy()
        many = _nms_batched_one(ops, boxes, scores, idxs, 0.7, max_output)
        assert np.array_equal(one, many)
        assert np.array_equal(one, ref)
        assert np.array_equal(many, ref)


def test_nms_absent_against_present():
    """A score of -inf: bd_batched_nms treats the item as present (it sorts last, takes part in the shift step's maximum and is kept unless
    suppressed, as the oracle's and the reference's batched_nms), bd_nms_batched as absent (out of the maximum, never kept).  Items 10..19
    lie far from every other box and from each other; item 13 has the largest coordinate of the set."""
    ops = _ops()
    rng = np.random.default_rng(7)
    n = 130
    boxes = _rand_boxes(rng, n, 1344, 800, 40, 200)
    scores = (np.round(rng.uniform(0, 1, n) * 512) / 512).astype(np.float32)
    idxs = rng.integers(0, 5, n).astype(np.int32)
    boxes[65:125] = boxes[:60] + rng.normal(0, 2, (60, 4)).astype(np.float32)
    idxs[65:125] = idxs[:60]
    for q, i in enumerate(range(10, 20)):
        x = 3000.0 + 150.0 * q
        boxes[i] = [x, x, x + 100.0, x + (2000.0 if i == 13 else 100.0)]
    scores[10:20] = -np.inf
    assert boxes.max() == boxes[13, 3] and boxes[13, 3] > boxes[np.isfinite(scores)].max()
    for max_output in (None, 17):
        ref = ob.batched_nms(boxes, scores, idxs, 0.7, max_output)
        got = ops.batched_nms(_dev(boxes), _dev(scores), _dev(idxs), 0.7, max_output).cpu().numpy()
        assert np.array_equal(got, ref)
        if max_output is None:
            assert np.array_equal(ref[-10:], np.arange(10, 20))          # present: kept, at the end, in index order
        valid = np.nonzero(np.isfinite(scores))[0]
        ref_v = valid[ob.batched_nms(boxes[valid], scores[valid], idxs[valid], 0.7, max_output)]
        got_v = _nms_batched_one(ops, boxes, scores, idxs, 0.7, max_output)
        assert np.array_equal(got_v, ref_v)


def _pyramid_inputs(rng, N, sizes, A, ldc):
    ppi = sum(h * w for h, w in sizes)
    raw = np.zeros((N, ppi, ldc), np.float32)
    raw[:, :, :A] = rng.normal(0, 2, (N, ppi, A))
    raw[:, :, A:5 * A] = rng.normal(0, 0.5, (N, ppi, 4 * A))
    t = _bf16(raw)
    return t.float().numpy(), t.cuda().reshape(N * ppi, ldc).contiguous(), ppi


def _anchors(sizes):
    scales = [[x] for x in [32, 64, 128, 256, 512]]
    ratios = [[0.5, 1, 2]]
    return ob.default_anchors(sizes, STRIDES, scales, ratios, 0.5)


@pytest.mark.parametrize("pre_k,post_k,per_level,ties", [(500, 300, 1, 0), (500, 300, 0, 0), (2000, 1000, 1, 0), (2000, 120, 1, 0),
                                                         (2000, 1000, 1, 1), (700, 64, 1, 1), (64, 40, 1, 0), (65, 40, 1, 1)])
def test_rpn_proposals(pre_k, post_k, per_level, ties):
    """per_level = 1 (round 5, default): the batched NMS level by level + a merge into the joint order; 0: one problem per image (rounds
    1-4).  Both against the oracle's joint batched_nms; (2000, 1000): the configured sizes (every level of this pyramid below pre_k keeps
    all its anchors); (2000, 120): the per-level cap and the merge cut the lists; ties = 1: five images whose scores take 17 distinct
    values only -- the merge's tie rule (lower level first, then candidate index) decides most of the joint order.  pre_k = 64 / 65: levels
    of exactly one 64-box word and of one word plus one box, beside the 45-anchor coarsest level below one word."""
    ops = _ops()
    rng = np.random.default_rng(2)
    N, A, ldc = (5 if ties else 2), 3, 16
    sizes = [(48, 80), (24, 40), (12, 20), (6, 10), (3, 5)]
    H, W = 192, 320
    raw, raw_dev, ppi = _pyramid_inputs(rng, N, sizes, A, ldc)
    if ties:
        raw[:, :, :A] = np.round(raw[:, :, :A] * 2) / 2          # multiples of 0.5 in about [-4, 4]: exact in bf16
        raw_dev = _bf16(raw).cuda().reshape(N * ppi, ldc).contiguous()
    anchors = _anchors(sizes)
    anc_all = np.concatenate(anchors, 0)
    im_info = np.array([[H, W, H, W, 3], [180, 300, 180, 300, 2]] + [[H, W, H, W, 1]] * (N - 2), np.float32)
    geom = _geom(N, sizes)
    rois = torch.empty((N, post_k, 4), dtype=torch.float32, device="cuda")
    num = torch.empty((N,), dtype=torch.int32, device="cuda")
    ws = torch.empty((ops.rpn_proposals_workspace_bytes(N, [h * w for h, w in sizes], A, pre_k, post_k),), dtype=torch.uint8, device="cuda")
    # RPN.NMS_THRESHOLD 0.7 (the default) with the identity coder; on the smaller problems also 0.5 and 0.9 under the two other coders
    # (RPN_BOX_REG: std < 1 shrinks the decoded shifts, std 2 on dw doubles them)
    combos = [(0.7, CODER_0)] + ([(0.5, CODER_A), (0.9, CODER_B)] if pre_k <= 700 else [])
    for thr, (mean, std) in combos:
        mean, std = list(mean), list(std)
        ops.rpn_proposals(raw_dev, ldc, A, 0, A, geom, _dev(anc_all), _dev(im_info), mean, std, pre_k, thr, post_k, rois, num, ws,
                          joint_nms=not per_level)
        gr, gn = rois.cpu().numpy(), num.cpu().numpy()
        if per_level:            # ... and the joint form gives the same proposals bit for bit
            rois0, num0 = torch.empty_like(rois), torch.empty_like(num)
            ops.rpn_proposals(raw_dev, ldc, A, 0, A, geom, _dev(anc_all), _dev(im_info), mean, std, pre_k, thr, post_k, rois0, num0, ws,
                              joint_nms=True)
            assert torch.equal(num, num0) and torch.equal(rois, rois0)
        for n in range(N):
            sc, of = [], []
            o = 0
            for (h, w) in sizes:
                blk = raw[n, o:o + h * w]
                sc.append(blk[:, :A].reshape(-1))
                of.append(blk[:, A:5 * A].reshape(-1, 4))
                o += h * w
            ref_rois, _, _ = orc.rpn_proposals(sc, of, anchors, im_info[n, :2], pre_k, post_k, thr, mean, std)
            assert gn[n] == len(ref_rois), (thr, n)
            # decode uses expf on the device and np.exp in the oracle: boxes within a few ulp, selection identical
            np.testing.assert_allclose(gr[n, : gn[n]], ref_rois, rtol=1e-5, atol=1e-3)
            assert np.all(gr[n, gn[n]:] == 0)


def test_rpn_targets_and_sampling():
    ops = _ops()
    rng = np.random.default_rng(3)
    N, Gmax = 3, 12
    sizes = [(48, 80), (24, 40), (12, 20), (6, 10), (3, 5)]
    anchors = np.concatenate(_anchors(sizes), 0)
    A = anchors.shape[0]
    gt, num_gt = _gt(rng, N, Gmax, 320, 192)
    num_gt[2] = 0
    kp = rng.random((N, A), dtype=np.float32)
    kn = rng.random((N, A), dtype=np.float32)
    kn = (np.round(kn * 4096) / 4096).astype(np.float32)          # force key ties
    labels = torch.empty((N, A), dtype=torch.int32, device="cuda")
    match = torch.empty((N, A), dtype=torch.int32, device="cuda")
    offs = torch.empty((N, A, 4), dtype=torch.float32, device="cuda")
    nfg = torch.zeros((1,), dtype=torch.int32, device="cuda")
    nvalid = torch.zeros((1,), dtype=torch.int32, device="cuda")
    ws = torch.empty((N * Gmax,), dtype=torch.float32, device="cuda")
    # (256, 64) and (64, 64): RPN.POSITIVE_ANCHOR_RATIO 0.25 and 1.0, under the non-identity coders (RPN_BOX_REG)
    for num_total, num_pos, (mean, std) in ((256, 128, CODER_0), (64, 8, CODER_0), (256, 64, CODER_A), (64, 64, CODER_B)):
        ops.rpn_assign_encode(_dev(anchors), _dev(gt), _dev(num_gt), 0.3, 0.7, True, list(mean), list(std), labels, match, offs, nfg, ws)
        ops.sample_labels(labels, _dev(kp), _dev(kn), num_pos, num_total, nvalid)
        ref_l, ref_o = orc.rpn_ground_truth(anchors, gt, num_gt, kp, kn, (0.3, 0.7), (0, -1, 1), True, num_total, num_pos, mean, std)
        gl = labels.cpu().numpy()
        assert np.array_equal(gl, ref_l)
        assert int(nvalid.item()) == int((ref_l >= 0).sum())
        fg = ref_l > 0
        np.testing.assert_allclose(offs.cpu().numpy()[fg], ref_o[fg], rtol=2e-6, atol=2e-6)
        assert (gl == 1).sum(axis=1).max() <= num_pos and (gl >= 0).sum(axis=1).max() <= num_total


def _ref_sample(labels, kp, kn, num_pos, num_total):
    """sampling.py:7-30 as applied by rpn.py:229-232: keep the num_pos smallest positive keys, then the (num_total - kept) smallest negative
    keys; ties go to the lowest index; the rest become -1."""
    out = labels.copy()
    for n in range(labels.shape[0]):
        pos = np.flatnonzero(labels[n] == 1)
        if len(pos) > num_pos:
            order = pos[np.lexsort((pos, kp[n, pos]))]
            out[n, order[max(num_pos, 0):]] = -1
        kept = min(len(pos), num_pos)
        neg = np.flatnonzero(labels[n] == 0)
        lim = num_total - kept
        if len(neg) > lim:
            order = neg[np.lexsort((neg, kn[n, neg]))]
            out[n, order[max(lim, 0):]] = -1
    return out


@pytest.mark.parametrize("case", ["uniform", "ties", "all_equal", "few_values", "no_negatives_left", "full_size"])
def test_sample_labels_selection_forms(case):
    """bd_sample_labels against a direct restatement of the rule at 20 000 and at C4's 268 569 anchors: uniform keys, heavy ties (lowest index
    wins), degenerate keys (one / three distinct values) and a sample the positives fill alone.  (Round 3 also measured a two-sweep form of the
    kernel -- 0.66 -> ~0.25 ms -- against these cases; the launch sits on a side stream and the step did not move, so it was not kept.)"""
    ops = _ops()
    rng = np.random.default_rng(17)
    N, A = (2, 268569) if case == "full_size" else (3, 20000)
    labels = rng.choice(np.array([-1, 0, 1], np.int32), size=(N, A), p=[0.1, 0.85, 0.05]).astype(np.int32)
    kp = rng.random((N, A), dtype=np.float32)
    kn = rng.random((N, A), dtype=np.float32)
    num_pos, num_total = 128, 256
    if case == "ties":
        kn = (np.round(kn * 512) / 512).astype(np.float32); kp = (np.round(kp * 64) / 64).astype(np.float32)
    elif case == "all_equal":
        kn[:] = 0.5; kp[:] = 0.25
    elif case == "few_values":
        kn = rng.choice(np.array([0.125, 0.126, 0.5], np.float32), size=(N, A)).astype(np.float32)
    elif case == "no_negatives_left":
        num_pos, num_total = 200, 200                      # the positives fill the sample: every negative goes
    lab = torch.from_numpy(labels).cuda()
    nvalid = torch.zeros((1,), dtype=torch.int32, device="cuda")
    ops.sample_labels(lab, _dev(kp), _dev(kn), num_pos, num_total, nvalid)
    ref = _ref_sample(labels, kp, kn, num_pos, num_total)
    assert np.array_equal(lab.cpu().numpy(), ref)
    assert int(nvalid.item()) == int((ref >= 0).sum())


def test_rcnn_sample_targets():
    ops = _ops()
    rng = np.random.default_rng(4)
    N, Gmax, post_k = 4, 10, 600
    gt, num_gt = _gt(rng, N, Gmax, 640, 480)
    num_gt[3] = 0
    rois = np.zeros((N, post_k, 4), np.float32)
    num_rois = np.array([600, 350, 40, 500], np.int32)
    for n in range(N):
        b = _rand_boxes(rng, num_rois[n], 640, 480, 10, 300)
        g = int(num_gt[n])
        if g:   # jittered copies of the gts so that there are many foreground candidates
            rep = gt[n, rng.integers(0, g, num_rois[n] // 2), :4] + rng.normal(0, 6, (num_rois[n] // 2, 4)).astype(np.float32)
            b[: len(rep)] = rep
        rois[n, : num_rois[n]] = b
    key_ld = post_k + Gmax
    kf = rng.random((N, key_ld), dtype=np.float32)
    kb = rng.random((N, key_ld), dtype=np.float32)
    kb = (np.round(kb * 256) / 256).astype(np.float32)             # force key ties
    std = [0.1, 0.1, 0.2, 0.2]
    # RCNN.FG_THRESHOLD / BG_THRESHOLD_HIGH / BG_THRESHOLD_LOW 0.6 / 0.4 / 0.1: a gap between the bands and a floor under the background
    # band; FG_RATIO 0 and 1 (num_fg_max = 0 and = num_samples); RCNN_BOX_REG with a non-zero mean and with four different stds
    for num_samples, fg_ratio, (fg_t, bg_hi, bg_lo), (mean, std) in ((512, 0.5, (0.5, 0.5, 0.0), ((0, 0, 0, 0), std)),
                                                                      (64, 0.25, (0.5, 0.5, 0.0), ((0, 0, 0, 0), std)),
                                                                      (64, 0.0, (0.6, 0.4, 0.1), CODER_A), (64, 1.0, (0.6, 0.4, 0.1), CODER_B),
                                                                      (512, 0.5, (0.6, 0.4, 0.1), CODER_A)):
        nfg = int(num_samples * fg_ratio)
        o_rois = torch.empty((N, num_samples, 4), dtype=torch.float32, device="cuda")
        o_lab = torch.empty((N, num_samples), dtype=torch.int32, device="cuda")
        o_tgt = torch.empty((N, num_samples, 4), dtype=torch.float32, device="cuda")
        o_cnt = torch.empty((N,), dtype=torch.int32, device="cuda")
        tot = torch.zeros((1,), dtype=torch.int32, device="cuda")
        ops.rcnn_sample_targets(_dev(rois), _dev(num_rois), _dev(gt), _dev(num_gt), _dev(kf), _dev(kb), num_samples, nfg, fg_t, bg_hi, bg_lo,
                                list(mean), list(std), o_rois, o_lab, o_tgt, o_cnt, tot)
        total = 0
        for n in range(N):
            rr, rl, rt = orc.rcnn_ground_truth(rois[n, : num_rois[n]], gt[n, : num_gt[n]], kf[n], kb[n], num_samples, fg_ratio,
                                               fg_t, bg_hi, bg_lo, mean, std)
            m = len(rl)
            total += m
            assert int(o_cnt[n].item()) == m
            assert np.array_equal(o_lab[n].cpu().numpy()[:m], rl)
            assert np.all(o_lab[n].cpu().numpy()[m:] == -1)
            assert np.array_equal(o_rois[n].cpu().numpy()[:m], rr)
            np.testing.assert_allclose(o_tgt[n].cpu().numpy()[:m], rt, rtol=2e-5, atol=2e-5)
        assert int(tot.item()) == total


def test_roi_align_reference_known_answer(golden_dir):
    """The reference's own RoIAlign vectors on bd_roi_align_fwd (tests/layers/test_roi_pool.py:32-45: the 4x4 matrix on the 5x5
    arange map; :64-75: the same RoI on the 2x bilinearly upsampled map at half the stride gives the same output).  One level,
    PH = PW = 4, the single channel replicated over 8 (16-byte channel groups).  Every value is exact in bf16."""
    import os
    import torch.nn.functional as TF
    ops = _ops()
    k = np.load(os.path.join(golden_dir, "reference_kat.npz"))
    C = 8

    def run(feat_nchw, stride, rois):
        _, _, h, w = feat_nchw.shape
        f = np.repeat(feat_nchw.transpose(0, 2, 3, 1), C, axis=3).reshape(h * w, C)
        geom = _geom(1, [(h, w)])
        out = torch.empty((1, 16, C), dtype=torch.bfloat16, device="cuda")
        ops.roi_align_fwd(_bf16(f).cuda(), geom, 1, [stride], C, _dev(rois), _dev(np.ones(1, np.int32)), 1, (4, 4), 2, out)
        o = out.float().cpu().numpy()
        assert np.all(o == o[..., :1]), "replicated channels differ"
        return o[0, :, 0].reshape(4, 4)

    feat, rois = k["roi_feat"], k["roi_rois"][:, 1:].copy()
    got = run(feat, 1, rois)
    assert np.array_equal(got.astype(np.float64), k["roi_align_4x4"]), got
    # scale invariance: integer strides only in the ABI, so the pair (stride 1, stride 1/2) becomes (stride 2, stride 1) with the
    # RoI given in 2x image coordinates
    f2 = TF.interpolate(torch.from_numpy(feat), scale_factor=2, mode="bilinear", align_corners=False).numpy()
    assert np.array_equal(run(feat, 2, rois * 2), got)
    assert np.array_equal(run(f2, 1, rois * 2), got)


def test_roi_align_bwd_scatter_full_size():
    """The GENERAL form of Faster R-CNN's RoIAlign backward (bd_roi_align_bwd: fp32 atomics, any pooled size) at BASELINE config C4's
    sizes: 256 channels, 512 RoIs per image, P2..P5 of an 800x1344 input (2 images) -- against the float64 adjoint of the oracle, with
    the configured 7 x 7 bins and with 14 x 14 and 5 x 3 ones (the shapes the tiled default does not take)."""
    ops = _ops()
    rng = np.random.default_rng(11)
    N, C, rpi = 2, 256, 512
    sizes = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    nlev = 4
    geom = _geom(N, sizes)
    ppi = geom.pix_per_img
    rois = np.concatenate([_rand_boxes(rng, rpi, 1344, 800, 8, 700) for _ in range(N)], 0)
    labels = np.ones(N * rpi, np.int32)
    labels[rng.integers(0, N * rpi, 40)] = -1                      # empty sample slots
    bidx = np.repeat(np.arange(N), rpi)
    gout = _bf16(rng.normal(0, 1, (N * rpi, 49, C)).astype(np.float32))
    g_in = gout.float().numpy().copy()
    g_in[labels < 0] = 0
    shapes = [(N, h, w, C) for h, w in sizes[:nlev]]
    refg = orc.roi_align_backward(g_in, shapes, rois, bidx, STRIDES[:nlev], 7, 7, 2)
    assert len(set(orc.assign_roi_levels(rois, STRIDES[:nlev]).tolist())) == 4
    # fp32 scatter
    gfeat = torch.zeros((N * ppi, C), dtype=torch.float32, device="cuda")
    ops.roi_align_bwd(gout.cuda(), geom, nlev, STRIDES, C, _dev(rois), _dev(labels), rpi, (7, 7), 2, gfeat)
    gg = gfeat.cpu().numpy().reshape(N, ppi, C)
    o = 0
    for l, (h, w) in enumerate(sizes[:nlev]):
        np.testing.assert_allclose(gg[:, o:o + h * w].reshape(N, h, w, C), refg[l], rtol=2e-4, atol=2e-4)
        o += h * w
    assert np.all(gg[:, o:] == 0)
    for PH, PW in ((14, 14), (5, 3)):
        gout2 = _bf16(rng.normal(0, 1, (N * rpi, PH * PW, C)).astype(np.float32))
        g2 = gout2.float().numpy().copy()
        g2[labels < 0] = 0
        ref2 = orc.roi_align_backward(g2, shapes, rois, bidx, STRIDES[:nlev], PH, PW, 2)
        gfeat.zero_()
        ops.roi_align_bwd(gout2.cuda(), geom, nlev, STRIDES, C, _dev(rois), _dev(labels), rpi, (PH, PW), 2, gfeat)
        gg = gfeat.cpu().numpy().reshape(N, ppi, C)
        o = 0
        for l, (h, w) in enumerate(sizes[:nlev]):
            np.testing.assert_allclose(gg[:, o:o + h * w].reshape(N, h, w, C), ref2[l], rtol=2e-4, atol=3e-4)
            o += h * w


def test_roi_align_bwd_tiles_full_size():
    """The training default since round 5 (bd_roi_align_bwd_bf16: per-tile RoI lists in slot order, sums in registers) at C4's sizes --
    256 channels, 512 RoIs per image, P2..P5 of an 800x1344 input -- against the float64 adjoint of the oracle: written into a buffer full
    of garbage (every pixel must be written), and added to an existing gradient (one bf16 rounding of the total; pixels no sample reaches
    keep their bits).  The RoI set carries what stresses the tile lists: footprints hundreds of pixels long and two pixels high, the whole
    image, zero-area and out-of-image boxes, empty slots.  Two launches give identical bits."""
    ops = _ops()
    rng = np.random.default_rng(12)
    N, C, rpi = 2, 256, 512
    sizes = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    nlev = 4
    geom = _geom(N, sizes)
    ppi = geom.pix_per_img
    rois = np.concatenate([_rand_boxes(rng, rpi, 1344, 800, 8, 700) for _ in range(N)], 0)
    rois[0] = [0, 0, 1344, 800]                  # the whole image (P5: every tile of the level)
    rois[1] = [0, 100, 1344, 109]                # 1344 x 9: sqrt(area) = 110 -> P2, a footprint 336 pixels long and 2-3 high
    rois[2] = [40, 0, 52, 800]                   # 12 x 800 -> P2, 200 pixels high
    rois[3] = [0, 300, 1344, 337]                # 1344 x 37 -> P3, 168 pixels long
    rois[4] = [500, 500, 500, 620]               # zero area
    rois[5] = [-300, -200, -20, -10]             # outside the image
    rois[6] = [1300, 760, 1500, 900]             # hanging over the bottom-right corner
    rois[rpi + 7] = [3, 3, 11, 9]                # smaller than one bin per pixel: every bin of a row lands on the same pixels
    labels = np.ones(N * rpi, np.int32)
    labels[rng.integers(8, N * rpi, 40)] = -1    # empty sample slots
    bidx = np.repeat(np.arange(N), rpi)
    gout = _bf16(rng.normal(0, 1, (N * rpi, 49, C)).astype(np.float32))
    g_in = gout.float().numpy().copy()
    g_in[labels < 0] = 0
    shapes = [(N, h, w, C) for h, w in sizes[:nlev]]
    refg = orc.roi_align_backward(g_in, shapes, rois, bidx, STRIDES[:nlev], 7, 7, 2)
    ws = torch.empty((ops.roi_align_bwd_bf16_workspace_bytes(geom, rpi),), dtype=torch.uint8, device="cuda")
    out = torch.full((N * ppi, C), 3.0, dtype=torch.bfloat16, device="cuda")
    ops.roi_align_bwd_bf16(gout.cuda(), geom, nlev, STRIDES, C, _dev(rois), _dev(labels), rpi, (7, 7), 2, out, ws)
    out2 = torch.full((N * ppi, C), -5.0, dtype=torch.bfloat16, device="cuda")
    ops.roi_align_bwd_bf16(gout.cuda(), geom, nlev, STRIDES, C, _dev(rois), _dev(labels), rpi, (7, 7), 2, out2, ws)
    assert torch.equal(out, out2)
    base = _bf16(rng.normal(0, 0.5, (N * ppi, C)).astype(np.float32))
    acc = base.clone().cuda()
    ops.roi_align_bwd_bf16(gout.cuda(), geom, nlev, STRIDES, C, _dev(rois), _dev(labels), rpi, (7, 7), 2, acc, ws, accumulate=True)
    g1 = out.float().cpu().numpy().reshape(N, ppi, C)
    g2 = acc.float().cpu().numpy().reshape(N, ppi, C)
    b = base.float().numpy().reshape(N, ppi, C)
    o = n_untouched = 0
    for l, (h, w) in enumerate(sizes[:nlev]):
        sl = slice(o, o + h * w)
        ref_l = refg[l].reshape(N, h * w, C)
        # an fp32 sum stored as bf16: half an ulp per element (2^-9 relative), rel-L2 ~1.1e-3
        np.testing.assert_allclose(g1[:, sl], ref_l, rtol=2 ** -8, atol=2e-3)
        assert np.linalg.norm(g1[:, sl] - ref_l) <= 2e-3 * np.linalg.norm(ref_l), l
        np.testing.assert_allclose(g2[:, sl], ref_l + b[:, sl], rtol=2 ** -8, atol=4e-3)
        untouched = (ref_l == 0).all(-1)
        n_untouched += int(untouched.sum())
        assert np.array_equal(g2[:, sl][untouched], b[:, sl][untouched])
        o += h * w
    assert n_untouched > 1000
    assert np.all(g1[:, o:] == 0) and np.array_equal(g2[:, o:], b[:, o:])


def test_roi_align_bwd_tiles_long_lists():
    """Tile lists far beyond one 64-RoI staging chunk: all 512 RoIs of an image are slivers stacked on the same rows of P2 / P3 (every
    tile of those rows lists hundreds of them, each RoI touches ~44 tiles) -- the chunked list staging of roi_align_bwd_tile_kernel and
    the list capacity (sized so that it cannot overflow) against the float64 adjoint."""
    ops = _ops()
    rng = np.random.default_rng(21)
    N, C, rpi = 1, 64, 512
    sizes = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    nlev = 4
    geom = _geom(N, sizes)
    ppi = geom.pix_per_img
    y0 = rng.uniform(100, 140, rpi).astype(np.float32)
    hh = rng.uniform(6, 9, rpi).astype(np.float32)
    rois = np.stack([rng.uniform(0, 20, rpi), y0, rng.uniform(1300, 1344, rpi), y0 + hh], 1).astype(np.float32)
    rois[256:, 3] = rois[256:, 1] + rng.uniform(10, 30, 256).astype(np.float32)      # sqrt(area) >= 112: P3
    labels = np.ones(N * rpi, np.int32)
    bidx = np.zeros(rpi, np.int64)
    lev = orc.assign_roi_levels(rois, STRIDES[:nlev])
    assert (lev == 0).sum() > 100 and (lev == 1).sum() > 100
    gout = _bf16(rng.normal(0, 1, (N * rpi, 49, C)).astype(np.float32))
    refg = orc.roi_align_backward(gout.float().numpy(), [(N, h, w, C) for h, w in sizes[:nlev]], rois, bidx, STRIDES[:nlev], 7, 7, 2)
    ws = torch.empty((ops.roi_align_bwd_bf16_workspace_bytes(geom, rpi),), dtype=torch.uint8, device="cuda")
    out = torch.full((N * ppi, C), 3.0, dtype=torch.bfloat16, device="cuda")
    ops.roi_align_bwd_bf16(gout.cuda(), geom, nlev, STRIDES, C, _dev(rois), _dev(labels), rpi, (7, 7), 2, out, ws)
    g1 = out.float().cpu().numpy().reshape(N, ppi, C)
    o = 0
    for l, (h, w) in enumerate(sizes[:nlev]):
        ref_l = refg[l].reshape(N, h * w, C)
        if np.abs(ref_l).max() > 0:
            assert np.linalg.norm(g1[:, o:o + h * w] - ref_l) <= 2e-3 * np.linalg.norm(ref_l), l
        else:
            assert np.all(g1[:, o:o + h * w] == 0)
        o += h * w
    assert np.all(g1[:, o:] == 0)


def test_roi_align_fwd_bwd():
    ops = _ops()
    rng = np.random.default_rng(5)
    N, C = 2, 64
    sizes = [(48, 80), (24, 40), (12, 20), (6, 10), (3, 5)]
    nlev = 4
    geom = _geom(N, sizes)
    ppi = geom.pix_per_img
    feat = _bf16(rng.normal(0, 1, (N, ppi, C)).astype(np.float32))
    feats = []
    o = 0
    for (h, w) in sizes[:nlev]:
        feats.append(feat.float().numpy()[:, o:o + h * w].reshape(N, h, w, C))
        o += h * w
    rpi = 24
    rois = np.concatenate([_rand_boxes(rng, rpi, 320, 192, 4, 400) for _ in range(N)], 0)
    rois[3] = [10, 10, 10, 30]            # zero area
    rois[5] = [-20, -30, 500, 400]        # far outside the image
    labels = np.ones(N * rpi, np.int32)
    labels[7] = -1
    bidx = np.repeat(np.arange(N), rpi)
    out = torch.empty((N * rpi, 49, C), dtype=torch.bfloat16, device="cuda")
    ops.roi_align_fwd(feat.cuda().reshape(N * ppi, C), geom, nlev, STRIDES, C, _dev(rois), _dev(labels), rpi, (7, 7), 2, out)
    ref = orc.roi_align(feats, rois, bidx, STRIDES[:nlev], 7, 7, 2)
    ref[7] = 0
    got = out.float().cpu().numpy()
    # one bf16 ulp (2^-8 relative) on top of the fp32 accumulation-order difference
    np.testing.assert_allclose(got, ref, rtol=2 ** -7, atol=1e-3)
    levels = orc.assign_roi_levels(rois, STRIDES[:nlev])
    assert len(set(levels.tolist())) >= 3
    # backward: adjoint
    gout = _bf16(rng.normal(0, 1, (N * rpi, 49, C)).astype(np.float32))
    gfeat = torch.zeros((N * ppi, C), dtype=torch.float32, device="cuda")
    ops.roi_align_bwd(gout.cuda(), geom, nlev, STRIDES, C, _dev(rois), _dev(labels), rpi, (7, 7), 2, gfeat)
    g_in = gout.float().numpy().copy()
    g_in[7] = 0
    refg = orc.roi_align_backward(g_in, [f.shape for f in feats], rois, bidx, STRIDES[:nlev], 7, 7, 2)
    gg = gfeat.cpu().numpy().reshape(N, ppi, C)
    o = 0
    for l, (h, w) in enumerate(sizes[:nlev]):
        np.testing.assert_allclose(gg[:, o:o + h * w].reshape(N, h, w, C), refg[l], rtol=1e-4, atol=1e-4)
        o += h * w
    assert np.all(gg[:, o:] == 0)
    # deterministic gather variant: bf16 output over the whole pyramid, bitwise reproducible
    gbf = torch.full((N * ppi, C), 7.0, dtype=torch.bfloat16, device="cuda")
    ws = torch.empty((ops.roi_align_bwd_bf16_workspace_bytes(geom, rpi),), dtype=torch.uint8, device="cuda")
    ops.roi_align_bwd_bf16(gout.cuda(), geom, nlev, STRIDES, C, _dev(rois), _dev(labels), rpi, (7, 7), 2, gbf, ws)
    g1 = gbf.float().cpu().numpy().reshape(N, ppi, C)
    o = 0
    for l, (h, w) in enumerate(sizes[:nlev]):
        np.testing.assert_allclose(g1[:, o:o + h * w].reshape(N, h, w, C), refg[l], rtol=2 ** -7, atol=1e-3)
        o += h * w
    assert np.all(g1[:, o:] == 0)
    gbf2 = torch.empty_like(gbf)
    ops.roi_align_bwd_bf16(gout.cuda(), geom, nlev, STRIDES, C, _dev(rois), _dev(labels), rpi, (7, 7), 2, gbf2, ws)
    assert torch.equal(gbf, gbf2)
    # accumulating form: added to what the buffer holds (one bf16 rounding of the total), pixels no sample reaches untouched
    base = _bf16(rng.normal(0, 1, (N * ppi, C)).astype(np.float32))
    gacc = base.cuda().clone()
    ops.roi_align_bwd_bf16(gout.cuda(), geom, nlev, STRIDES, C, _dev(rois), _dev(labels), rpi, (7, 7), 2, gacc, ws, accumulate=True)
    ga = gacc.float().cpu().numpy().reshape(N, ppi, C)
    bb = base.float().numpy().reshape(N, ppi, C)
    o = 0
    for l, (h, w) in enumerate(sizes[:nlev]):
        np.testing.assert_allclose(ga[:, o:o + h * w].reshape(N, h, w, C), refg[l] + bb[:, o:o + h * w].reshape(N, h, w, C), rtol=2 ** -7, atol=2e-3)
        untouched = (refg[l] == 0).all(-1)
        assert np.array_equal(ga[:, o:o + h * w].reshape(N, h, w, C)[untouched], bb[:, o:o + h * w].reshape(N, h, w, C)[untouched])
        o += h * w
    assert np.array_equal(ga[:, o:], bb[:, o:])


def test_subsample_and_convert():
    ops = _ops()
    rng = np.random.default_rng(6)
    N, C = 2, 32
    sizes = [(13, 21), (7, 11)]
    geom = _geom(N, sizes)
    ppi = geom.pix_per_img
    buf = _bf16(rng.normal(0, 1, (N, ppi, C)).astype(np.float32))
    dev = buf.cuda().reshape(N * ppi, C).contiguous()
    ops.subsample2x_fwd(dev, geom.level(0), dev, geom.level(1), C)
    got = dev.float().cpu().numpy().reshape(N, ppi, C)
    src = buf.float().numpy()[:, : 13 * 21].reshape(N, 13, 21, C)
    assert np.array_equal(got[:, 13 * 21:].reshape(N, 7, 11, C), src[:, ::2, ::2])
    g = _bf16(rng.normal(0, 1, (N, ppi, C)).astype(np.float32))
    gdev = g.cuda().reshape(N * ppi, C).contiguous()
    ops.subsample2x_bwd_add(gdev, geom.level(1), gdev, geom.level(0), C)
    gg = gdev.float().cpu().numpy().reshape(N, ppi, C)
    g0 = g.float().numpy()
    exp = g0[:, : 13 * 21].reshape(N, 13, 21, C).copy()
    exp[:, ::2, ::2] = (torch.from_numpy(exp[:, ::2, ::2] + g0[:, 13 * 21:].reshape(N, 7, 11, C)).to(torch.bfloat16).float().numpy())
    assert np.array_equal(gg[:, : 13 * 21].reshape(N, 13, 21, C), exp)
    x = torch.randn(4096, device="cuda")
    y = torch.empty(4096, dtype=torch.bfloat16, device="cuda")
    ops.f32_to_bf16(x, y)
    assert torch.equal(y, x.to(torch.bfloat16))
    # accumulating form (the fp32 RoIAlign-backward pyramid joins the RPN head's dL/dP): dst = bf16(float(dst) + src), one rounding
    base = torch.randn(4096, device="cuda").to(torch.bfloat16)
    y2 = base.clone()
    ops.f32_to_bf16(x, y2, accumulate=True)
    assert torch.equal(y2, (base.float() + x).to(torch.bfloat16))


def test_rpn_loss():
    ops = _ops()
    rng = np.random.default_rng(7)
    rows, A, ldc = 5000, 3, 16
    raw = _bf16(rng.normal(0, 2, (rows, ldc)).astype(np.float32))
    labels = rng.choice([-1, 0, 1], size=rows * A, p=[0.9, 0.07, 0.03]).astype(np.int32)
    targets = rng.normal(0, 1, (rows * A, 4)).astype(np.float32)
    nv = torch.tensor([int((labels >= 0).sum())], dtype=torch.int32, device="cuda")
    for beta in (0.0, 0.5):
        loss = torch.zeros((2,), dtype=torch.float32, device="cuda")
        draw = torch.zeros((rows, ldc), dtype=torch.bfloat16, device="cuda")
        ops.rpn_loss_fwd_bwd(raw.cuda(), ldc, A, 0, A, _dev(labels), _dev(targets), rows, beta, nv, loss, draw)
        r = raw.float().numpy()
        logits = r[:, :A].reshape(-1)
        offs = r[:, A:5 * A].reshape(-1, 4)
        cls, box = orc.rpn_losses(logits, offs, labels, targets, beta)
        got = loss.cpu().numpy()
        assert abs(got[0] - cls) <= 1e-4 * abs(cls) + 1e-6
        assert abs(got[1] - box) <= 1e-4 * abs(box) + 1e-6
        # gradient: torch autograd on the same formula (fp64), compared at bf16 resolution
        x = torch.tensor(r, dtype=torch.float64, requires_grad=True)
        lab = torch.from_numpy(labels)
        lg = x[:, :A].reshape(-1); of = x[:, A:5 * A].reshape(-1, 4)
        valid = lab >= 0; fg = lab > 0
        t = lab[valid].double()
        ls = torch.nn.functional.logsigmoid
        l_cls = (-(t * ls(lg[valid]) + (1 - t) * ls(-lg[valid]))).sum() / max(int(valid.sum()), 1)
        d = of[fg] - torch.from_numpy(targets).double()[fg]
        l_box = (d.abs() if beta < 1e-5 else torch.where(d.abs() < beta, 0.5 * d * d / beta, d.abs() - 0.5 * beta)).sum() / max(int(valid.sum()), 1)
        (l_cls + l_box).backward()
        ref_g = x.grad.float().numpy()
        ref_g[:, 5 * A:] = 0
        np.testing.assert_allclose(draw.float().cpu().numpy(), ref_g, rtol=2 ** -7, atol=1e-7)


def test_rcnn_loss():
    ops = _ops()
    rng = np.random.default_rng(8)
    R, K = 700, 80
    ld = 408
    box_off = K + 1
    raw = _bf16(rng.normal(0, 1.5, (R, ld)).astype(np.float32))
    labels = rng.integers(-1, K + 1, R).astype(np.int32)
    labels[rng.random(R) < 0.5] = 0
    targets = rng.normal(0, 1, (R, 4)).astype(np.float32)
    ns = torch.tensor([int((labels >= 0).sum())], dtype=torch.int32, device="cuda")
    for beta in (0.0, 1.0):
        loss = torch.zeros((2,), dtype=torch.float32, device="cuda")
        draw = torch.empty((R, ld), dtype=torch.bfloat16, device="cuda")
        ops.rcnn_loss_fwd_bwd(raw.cuda(), ld, K, box_off, _dev(labels), _dev(targets), R, beta, ns, loss, draw)
        r = raw.float().numpy()
        v = labels >= 0
        cls, box = orc.rcnn_losses(r[v, : K + 1], r[v, box_off: box_off + 4 * K].reshape(-1, K, 4), labels[v], targets[v], beta)
        got = loss.cpu().numpy()
        assert abs(got[0] - cls) <= 1e-4 * abs(cls) + 1e-6
        assert abs(got[1] - box) <= 1e-4 * abs(box) + 1e-6
        x = torch.tensor(r, dtype=torch.float64, requires_grad=True)
        lab = torch.from_numpy(labels).long()
        vm = lab >= 0
        nsamp = max(int(vm.sum()), 1)
        l_cls = torch.nn.functional.cross_entropy(x[vm, : K + 1], lab[vm], reduction="sum") / nsamp
        fg = lab > 0
        d = x[:, box_off: box_off + 4 * K].reshape(R, K, 4)[fg, lab[fg] - 1] - torch.from_numpy(targets).double()[fg]
        l_box = (d.abs() if beta < 1e-5 else torch.where(d.abs() < beta, 0.5 * d * d / beta, d.abs() - 0.5 * beta)).sum() / nsamp
        (l_cls + l_box).backward()
        np.testing.assert_allclose(draw.float().cpu().numpy(), x.grad.float().numpy(), rtol=2 ** -7, atol=1e-7)


def test_empty_and_degenerate_inputs():
    """Edge cases: nothing above the score threshold, no valid NMS candidate, an image without proposals or ground truth."""
    ops = _ops()
    B, C, k = 2, 128, 64
    scores = torch.full((B, C), -3.0, device="cuda")
    idx = torch.empty((B, 1, k), dtype=torch.int32, device="cuda")
    sc = torch.empty((B, 1, k), dtype=torch.float32, device="cuda")
    cnt = torch.full((B, 1), -1, dtype=torch.int32, device="cuda")
    ops.segment_topk(scores, B, C, 1, 1, 0, [0], [C], k, idx, sc, cnt, min_score=0.05)
    assert cnt.cpu().tolist() == [[0], [0]] and bool((idx == -1).all())
    boxes = torch.rand((B, C, 4), device="cuda")
    neg = torch.full((B, C), float("-inf"), device="cuda")
    keep = torch.full((B, 10), -1, dtype=torch.int32, device="cuda")
    num = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty((ops.nms_batched_workspace_bytes(B, C),), dtype=torch.uint8, device="cuda")
    ops.nms_batched(boxes, neg, None, 0.5, 10, keep, num, ws)
    assert num.cpu().tolist() == [0, 0]
    # RoI sampling: image 0 has neither proposals nor gts, image 1 has gts only
    N, Gmax, post_k, S = 2, 4, 16, 8
    rois = torch.zeros((N, post_k, 4), device="cuda")
    num_rois = torch.zeros((N,), dtype=torch.int32, device="cuda")
    gt = torch.zeros((N, Gmax, 5), device="cuda")
    gt[1, 0] = torch.tensor([10., 10., 50., 60., 7.])
    gt[1, 1] = torch.tensor([30., 20., 90., 80., 2.])
    num_gt = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    keys = torch.rand((N, post_k + Gmax), device="cuda")
    o_rois = torch.empty((N, S, 4), device="cuda"); o_lab = torch.empty((N, S), dtype=torch.int32, device="cuda")
    o_tgt = torch.empty((N, S, 4), device="cuda"); o_cnt = torch.empty((N,), dtype=torch.int32, device="cuda")
    tot = torch.zeros((1,), dtype=torch.int32, device="cuda")
    ops.rcnn_sample_targets(rois, num_rois, gt, num_gt, keys, keys, S, 4, 0.5, 0.5, 0.0, [0, 0, 0, 0], [0.1, 0.1, 0.2, 0.2],
                            o_rois, o_lab, o_tgt, o_cnt, tot)
    assert o_cnt.cpu().tolist() == [0, 2] and int(tot.item()) == 2
    assert o_lab.cpu().tolist()[0] == [-1] * S and o_lab.cpu().tolist()[1][:2] == [7, 2]
    assert torch.equal(o_rois[1, :2], gt[1, :2, :4]) and float(o_tgt[1, :2].abs().max()) == 0.0
    # the losses of an all-empty RoI batch are zero with zero gradients
    R, K, ld = 8, 80, 408
    raw = torch.randn((R, ld), device="cuda").to(torch.bfloat16)
    loss = torch.zeros((2,), device="cuda"); draw = torch.ones((R, ld), dtype=torch.bfloat16, device="cuda")
    ops.rcnn_loss_fwd_bwd(raw, ld, K, K + 1, torch.full((R,), -1, dtype=torch.int32, device="cuda"), torch.zeros((R, 4), device="cuda"), R,
                          0.0, torch.zeros((1,), dtype=torch.int32, device="cuda"), loss, draw)
    assert loss.cpu().tolist() == [0.0, 0.0] and not bool(draw.float().any())
