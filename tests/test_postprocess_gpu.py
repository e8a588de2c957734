"""The inference post-processing kernels one at a time (csrc/postprocess.hip det_scores / det_candidates / det_finalize /
rcnn_predict, csrc/rcnn_ops.hip segment_topk, csrc/nms.hip nms_batched) in the call forms and at the sizes of 800x1344 inference, against
float64 torch or the numpy oracle: oracle/rcnn_ops.py topk_desc (:44-53) and detect_postprocess (:294-318), oracle/box_ops.py
box_decode (:203-215), point_decode (:225-230), batched_nms (:598-609), box_scale / box_clip (:142-162).

Indices, labels and keep lists are compared bit-exactly; fp32 scores in units of the fp32 spacing (util.f32_ulps); decoded boxes
with the box_decode tolerance of test_boxops_gpu.py (rtol 1e-5, atol 1e-3)."""
import numpy as np
import pytest
import torch

from oracle import box_ops as ob
from oracle import rcnn_ops as orc
from util import f32_ulps

pytestmark = pytest.mark.gpu

SIZES = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]        # 800x1344, strides 8..128
STRIDES = [8, 16, 32, 64, 128]
SCALES = [[x, x * 2 ** (1.0 / 3), x * 2 ** (2.0 / 3)] for x in [32, 64, 128, 256, 512]]
RATIOS = [[0.5, 1, 2]]
from tests.config_key_cases import BOX_CODER_A, BOX_CODER_B  # noqa: E402

MEAN, STD = (0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2)
CODERS = ((MEAN, STD), BOX_CODER_A, BOX_CODER_B)      # further coders for the kernels that decode


def _ops():
    from basedet_amd import ops
    return ops


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _row_off(rows):
    return [int(v) for v in np.concatenate([[0], np.cumsum(rows)[:-1]])]


# ---- det_scores ----------------------------------------------------------------------------------------------------
def test_det_scores_sigmoid_and_fcos_forms():
    """sigmoid at RetinaNet's 201 600 anchors x 80 classes (16.1M scores: 7.7 passes of the 8192 x 256 grid) and FCOS's
    sqrt(sigmoid(cls) * sigmoid(ctr)) at 22 400 points x 80 with the centre-ness read from channel 4 of 8-channel rows."""
    ops = _ops()
    gen = _gen(1)
    rows, K = 201600, 80
    logits = (torch.randn((rows, K), generator=gen, device="cuda") * 4 - 2).to(torch.bfloat16)
    scores = torch.full((rows * K,), float("nan"), dtype=torch.float32, device="cuda")
    ops.det_scores(logits, rows, K, scores)
    u = f32_ulps(scores, torch.sigmoid(logits.double().reshape(-1)))
    worst = float(u.max())
    print(f"det_scores sigmoid: max {worst:.2f} fp32 ulp")
    assert worst <= 2                   # observed 1.98 (expf, one add, one division)

    rows = 22400
    logits = (torch.randn((rows, K), generator=gen, device="cuda") * 4 - 2).to(torch.bfloat16)
    raw = (torch.randn((rows, 8), generator=gen, device="cuda") * 3).to(torch.bfloat16)
    scores = torch.full((rows * K,), float("nan"), dtype=torch.float32, device="cuda")
    ops.det_scores(logits, rows, K, scores, ctr=raw, ctr_ld=8, ctr_off=4)
    ref = torch.sqrt(torch.sigmoid(logits.double()) * torch.sigmoid(raw[:, 4:5].double())).reshape(-1)
    worst = float(f32_ulps(scores, ref).max())
    print(f"det_scores fcos: max {worst:.2f} fp32 ulp")
    assert worst <= 3                   # observed 2.12 (two sigmoids, a product and a square root)


# ---- segment_topk --------------------------------------------------------------------------------------------------
def test_segment_topk_inference_form():
    """The inference call (fpn_base.py _detect): fp32 scores, A = 1, ldc = 1, seg_start = row_off * K, k = 1000, min_score 0.05,
    one segment per FCOS/RetinaNet level.  Scores are fp32 sigmoids of bf16 logits, so equal scores come in groups and the cut at
    rank 1000 falls inside one.  Levels: P3 (151 200 x 80 = 12.1M items) cut at k; P4 with fewer than k items above the threshold;
    P5 with none; P6, P7 cut at k."""
    ops = _ops()
    gen = _gen(2)
    K, k, thr = 80, 1000, 0.05
    lvl_rows = [151200, 37800, 9450, 2457, 693]                # RetinaNet's anchors per level at 800x1344 (9 per pixel)
    mu_sd = [(-6.0, 1.2), (-7.0, 1.0), (-9.0, 0.5), (-3.0, 1.0), (-3.0, 1.0)]
    # logits on a 1/16 grid (exact in bf16): ~100 items share each score value near P3's cut
    parts = [(torch.round((torch.randn((r * K,), generator=gen, device="cuda") * sd + mu) * 16) / 16).to(torch.bfloat16)
             for r, (mu, sd) in zip(lvl_rows, mu_sd)]
    scores = torch.sigmoid(torch.cat(parts).float())
    row_off = _row_off(lvl_rows)
    L = len(lvl_rows)
    idx = torch.full((L, k), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((L, k), float("nan"), dtype=torch.float32, device="cuda")
    cnt = torch.full((L,), -7, dtype=torch.int32, device="cuda")
    ops.segment_topk(scores, 1, 0, 1, 1, 0, [r * K for r in row_off], [r * K for r in lvl_rows], k, idx, sc, cnt, min_score=thr)
    s_np = scores.cpu().numpy()
    gi, gs, gc = idx.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy()
    passing = []
    for l, (o, r) in enumerate(zip(row_off, lvl_rows)):
        lv = s_np[o * K:(o + r) * K]
        ri, rs = orc.topk_desc(lv, k, thr)
        passing.append(int((lv > np.float32(thr)).sum()))
        assert gc[l] == len(ri), l
        assert np.array_equal(gi[l, : len(ri)], ri), l
        assert np.array_equal(gs[l, : len(ri)].view(np.uint32), rs.view(np.uint32)), l
        assert np.all(gi[l, len(ri):] == -1) and np.all(gs[l, len(ri):] == 0), l
        if l == 0:                                              # the cut splits a group of equal scores
            above = np.sort(lv[lv > np.float32(thr)])[::-1]
            assert above[k - 1] == above[k], "the k-th and (k+1)-th scores of P3 should tie"
    print(f"segment_topk: items above the threshold per level {passing}, kept {gc.tolist()}")
    assert passing[0] > k and 0 < passing[1] < k and passing[2] == 0 and passing[3] > k


def test_segment_topk_refuses_a_segment_of_2_pow_24_items():
    """Item indices travel through fp32 keys and the radix histogram counts in 24 bits: the entry point must refuse such a segment
    before any launch and leave the outputs alone."""
    from basedet_amd._lib import BasedetHipError
    ops = _ops()
    scores = torch.zeros((16,), dtype=torch.float32, device="cuda")
    idx = torch.full((1, 8), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((1, 8), 5.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(BasedetHipError, match="too long"):
        ops.segment_topk(scores, 1, 0, 1, 1, 0, [0], [1 << 24], 8, idx, sc, cnt, min_score=0.05)
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((sc == 5.0).all()) and int(cnt.item()) == -7


# ---- det_candidates -------------------------------------------------------------------------------------------------
def _fake_topk(rng, lvl_items, k, cnts):
    """segment_topk-shaped outputs: per level `cnt` distinct item indices with descending scores, then -1 / 0 padding."""
    L = len(lvl_items)
    idx = np.full((L, k), -1, np.int32)
    sc = np.zeros((L, k), np.float32)
    for l, (n, c) in enumerate(zip(lvl_items, cnts)):
        idx[l, :c] = rng.choice(n, c, replace=False)
        sc[l, :c] = np.sort(rng.uniform(0.05, 1, c).astype(np.float32))[::-1]
    return idx, sc, np.asarray(cnts, np.int32)


def _check_candidates(boxes, scores, labels, tk_idx, tk_sc, tk_cnt, K, ref_box_of, exact):
    L, k = tk_idx.shape
    boxes, scores, labels = boxes.cpu().numpy().reshape(L, k, 4), scores.cpu().numpy().reshape(L, k), labels.cpu().numpy().reshape(L, k)
    for l in range(L):
        c = int(tk_cnt[l])
        assert np.array_equal(labels[l, :c], tk_idx[l, :c] % K)
        assert np.array_equal(scores[l, :c], tk_sc[l, :c])
        ref = ref_box_of(l, tk_idx[l, :c]) if c else np.zeros((0, 4), np.float32)
        if exact:
            assert np.array_equal(boxes[l, :c], ref), l
        else:
            np.testing.assert_allclose(boxes[l, :c], ref, rtol=1e-5, atol=1e-3)
        assert np.all(scores[l, c:] == -np.inf) and np.all(labels[l, c:] == 0) and np.all(boxes[l, c:] == 0), l


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_det_candidates(mode):
    """mode 0: RetinaNet anchors (A = 9, offsets in 40-channel rows); mode 1: FCOS points (off_ld = 4); mode 2: RCNN per-item boxes
    (one level of R x K items, k = 2048).  Some levels hold fewer than k candidates, one holds none."""
    ops = _ops()
    rng = np.random.default_rng(10 + mode)
    K = 80
    if mode == 2:
        R, k = 1000, 2048
        lvl_rows, A, off_ld = [R], 1, 4
        cnts = [1333]
        item_boxes = ob.box_decode(np.repeat(rng.uniform(0, 700, (R, 4)).astype(np.float32), K, 0),
                                   rng.normal(0, 0.5, (R * K, 4)).astype(np.float32), MEAN, STD)
        anchors = offsets_np = None
    else:
        k = 1000
        A, off_ld = (9, 40) if mode == 0 else (1, 4)
        lvl_rows = [h * w * A for h, w in SIZES]
        cnts = [1000, 1000, 437, 0, 12]
        pix = sum(h * w for h, w in SIZES)
        if mode == 0:
            anchors = np.concatenate(ob.default_anchors(SIZES, STRIDES, SCALES, RATIOS, 0.5))
            off = rng.normal(0, 0.7, (pix, off_ld)).astype(np.float32)
        else:
            anchors = np.concatenate(ob.point_anchors(SIZES, STRIDES, 0.5, 1))
            off = rng.uniform(0, 300, (pix, off_ld)).astype(np.float32)
        offsets = torch.from_numpy(off).to(torch.bfloat16)
        offsets_np = offsets.float().numpy()
        item_boxes = None
    row_off = _row_off(lvl_rows)
    L = len(lvl_rows)
    tk_idx, tk_sc, tk_cnt = _fake_topk(rng, [r * K for r in lvl_rows], k, cnts)
    boxes = torch.full((L * k, 4), 7.0, device="cuda")
    scores = torch.full((1, L * k), 7.0, device="cuda")
    labels = torch.full((1, L * k), 7, dtype=torch.int32, device="cuda")
    for mean, std in (CODERS if mode == 0 else CODERS[:1]):          # mode 0 is the one that decodes with a box coder (MODEL.BOX_REG)
        boxes.fill_(7.0); scores.fill_(7.0); labels.fill_(7)
        ops.det_candidates(mode, _dev(tk_idx), _dev(tk_sc), _dev(tk_cnt), 1, L, k, row_off, K,
                           _dev(anchors) if anchors is not None else None, offsets.cuda() if offsets_np is not None else None, 0, off_ld, A,
                           mean, std, _dev(item_boxes) if item_boxes is not None else None, 0, boxes, scores, labels)

        def ref_box(l, idx):
            row = row_off[l] + idx // K
            if mode == 2:
                return item_boxes[row * K + idx % K]
            d = offsets_np[row // A][np.arange(len(row))[:, None], (row % A)[:, None] * 4 + np.arange(4)[None]]
            if mode == 0:
                return ob.box_decode(anchors[row], d, mean, std)
            return ob.point_decode(anchors[row], d)

        _check_candidates(boxes, scores, labels, tk_idx, tk_sc, tk_cnt, K, ref_box, exact=mode != 0)


# ---- nms_batched ----------------------------------------------------------------------------------------------------
def _clustered_boxes(rng, n, W=1344, H=800):
    centres = rng.uniform(0, 1, (max(n // 12, 1), 2)) * [W, H]
    c = centres[rng.integers(0, len(centres), n)] + rng.normal(0, 12, (n, 2))
    wh = rng.uniform(16, 260, (n, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)


def _nms_case(boxes, scores, labels, max_out, thr=0.5):
    ops = _ops()
    B, C = scores.shape
    cap = max_out if max_out > 0 else C
    keep = torch.full((B, cap), -7, dtype=torch.int32, device="cuda")
    num = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty((ops.nms_batched_workspace_bytes(B, C),), dtype=torch.uint8, device="cuda")
    ops.nms_batched(_dev(boxes), _dev(scores), _dev(labels), thr, max_out, keep, num, ws)
    gk, gn = keep.cpu().numpy(), num.cpu().numpy()
    refs = []
    for b in range(B):
        valid = np.nonzero(scores[b] > -np.inf)[0]
        ref = valid[ob.batched_nms(boxes[b][valid], scores[b][valid], labels[b][valid], thr, max_out if max_out > 0 else None)]
        assert gn[b] == len(ref), b
        assert np.array_equal(gk[b, : gn[b]], ref), b
        refs.append(ref)
    return refs


def test_nms_batched_one_stage_candidate_list():
    """B = 1, C = 5 x 1000: the candidate list of a one-stage detector, per level the top-k in descending order followed by its
    -inf padding slots (fewer than k on three levels), 80 labels, IoU 0.5, max_out = 100 -- the 100th survivor falls inside a
    64-box chunk of the sorted list, not on its edge."""
    rng = np.random.default_rng(20)
    k, L = 1000, 5
    cnts = [1000, 1000, 618, 97, 0]
    boxes = np.zeros((1, L * k, 4), np.float32)
    scores = np.full((1, L * k), -np.inf, np.float32)
    labels = np.zeros((1, L * k), np.int32)
    for l, c in enumerate(cnts):
        boxes[0, l * k: l * k + c] = _clustered_boxes(rng, c)
        scores[0, l * k: l * k + c] = np.sort(np.round(rng.uniform(0.05, 1, c) * 256) / 256).astype(np.float32)[::-1]   # ties
        labels[0, l * k: l * k + c] = rng.integers(0, 80, c)
    full = _nms_case(boxes, scores, labels, 0)[0]
    assert len(full) > 100
    ref = _nms_case(boxes, scores, labels, 100)[0]
    valid = np.nonzero(scores[0] > -np.inf)[0]
    order = valid[np.argsort(-scores[0][valid], kind="stable")]
    rank = int(np.nonzero(order == ref[-1])[0][0])
    print(f"nms_batched C=5000: {len(full)} survivors without a cap; the 100th at sorted rank {rank} (position {rank % 64} of its chunk)")
    assert rank % 64 not in (0, 63)


def test_nms_batched_at_the_lds_limit():
    """C = 16 384 (NMSB_MAX), two problems, with and without max_out; -inf slots scattered through the list."""
    rng = np.random.default_rng(21)
    B, C = 2, 16384
    boxes = np.stack([_clustered_boxes(rng, C) for _ in range(B)])
    scores = (np.round(rng.uniform(0, 1, (B, C)) * 1024) / 1024).astype(np.float32)
    scores[rng.uniform(size=(B, C)) < 0.1] = -np.inf
    labels = rng.integers(0, 80, (B, C)).astype(np.int32)
    for max_out in (0, 100):
        refs = _nms_case(boxes, scores, labels, max_out)
        print(f"nms_batched C=16384 max_out={max_out}: survivors {[len(r) for r in refs]}")


# ---- det_finalize ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_keep", [0, 37, 100])
def test_det_finalize(num_keep):
    """Gather the NMS survivors, rescale anisotropically (800x1344 -> 533x1111) and clip: boxes cross all four borders.  Slots past
    num_keep are label -1, score 0, box 0.  The arithmetic is one fp32 multiply and a clamp: bit-exact against box_scale / box_clip."""
    ops = _ops()
    rng = np.random.default_rng(30 + num_keep)
    C, max_out = 5000, 100
    xy = rng.uniform(-150, 1400, (C, 2)) * [1, 800 / 1344]
    wh = rng.uniform(10, 400, (C, 2))
    boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    scores = rng.uniform(0, 1, C).astype(np.float32)
    labels = rng.integers(0, 80, C).astype(np.int32)
    keep = np.full((1, max_out), -1, np.int32)
    keep[0, :num_keep] = rng.choice(C, num_keep, replace=False)
    info = np.array([800, 1344, 533, 1111], np.float32)
    ob_, os_, ol_ = (torch.full((max_out, 4), 7.0, device="cuda"), torch.full((max_out,), 7.0, device="cuda"),
                     torch.full((max_out,), 7, dtype=torch.int32, device="cuda"))
    ops.det_finalize(_dev(boxes), _dev(scores)[None], _dev(labels)[None], _dev(keep), _dev(np.array([num_keep], np.int32)), max_out,
                     _dev(info), ob_, os_, ol_)
    gb, gs, gl = ob_.cpu().numpy(), os_.cpu().numpy(), ol_.cpu().numpy()
    kk = keep[0, :num_keep]
    ref = ob.box_clip(ob.box_scale(boxes[kk], (np.float32(info[2] / info[0]), np.float32(info[3] / info[1]))), info[2:4])
    assert np.array_equal(gb[:num_keep], ref)
    assert np.array_equal(gs[:num_keep], scores[kk]) and np.array_equal(gl[:num_keep], labels[kk])
    assert np.all(gb[num_keep:] == 0) and np.all(gs[num_keep:] == 0) and np.all(gl[num_keep:] == -1)
    if num_keep == max_out:                 # every border clips at least one box
        assert (ref[:, 0] == 0).any() and (ref[:, 1] == 0).any() and (ref[:, 2] == info[3]).any() and (ref[:, 3] == info[2]).any()


# ---- rcnn_predict ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 20, 80, 365])
def test_rcnn_predict(K):
    """Softmax over K + 1 logits (1 to 6 passes of the 64 lanes), background dropped, and the per-class decode of every RoI; R = 3 x 333
    (not a multiple of the kernel's 4 rows per block), image 1 with 120 RoIs and image 2 with none (their rows score -inf), and a row
    pitch with 8 padding channels."""
    ops = _ops()
    rng = np.random.default_rng(40 + K)
    per_img, nimg = 333, 3
    R = per_img * nimg
    ld = (K + 1 + 4 * K + 7) // 8 * 8 + 8
    raw = torch.from_numpy(rng.normal(0, 2.5, (R, ld)).astype(np.float32)).to(torch.bfloat16)
    xy = rng.uniform(0, 1200, (R, 2)); wh = rng.uniform(4, 300, (R, 2))
    rois = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    num_rois = np.array([per_img, 120, 0], np.int32)
    scores = torch.full((R * K,), float("nan"), device="cuda")
    boxes = torch.full((R * K, 4), float("nan"), device="cuda")
    deltas = raw.float().numpy()[:, K + 1: K + 1 + 4 * K].reshape(R * K, 4)
    for mean, std in CODERS[1:]:                     # MODEL.RCNN_BOX_REG other than the configured one (checked last, with the scores)
        ops.rcnn_predict(raw.cuda(), ld, K, K + 1, _dev(rois), _dev(num_rois), per_img, mean, std, scores, boxes)
        np.testing.assert_allclose(boxes.cpu().numpy(), ob.box_decode(np.repeat(rois, K, 0), deltas, mean, std), rtol=1e-5, atol=1e-3)
        scores.fill_(float("nan")); boxes.fill_(float("nan"))
    ops.rcnn_predict(raw.cuda(), ld, K, K + 1, _dev(rois), _dev(num_rois), per_img, MEAN, STD, scores, boxes)
    r = raw.double()
    p64 = torch.softmax(r[:, : K + 1], 1)[:, 1:].reshape(-1)
    got = scores.cpu().double()
    valid = torch.from_numpy(np.repeat((np.arange(R) % per_img) < num_rois[np.arange(R) // per_img], K))
    assert bool(torch.isneginf(got[~valid]).all())
    rel = float(((got[valid] - p64[valid]).abs() / p64[valid]).max())
    print(f"rcnn_predict K={K}: softmax max rel err {rel:.2e}")
    assert rel < 1e-6                   # observed 2.8e-7 (K = 365)
    deltas = raw.float().numpy()[:, K + 1: K + 1 + 4 * K].reshape(R * K, 4)
    ref = ob.box_decode(np.repeat(rois, K, 0), deltas, MEAN, STD)
    np.testing.assert_allclose(boxes.cpu().numpy(), ref, rtol=1e-5, atol=1e-3)
