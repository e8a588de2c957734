"""bd_det_select (csrc/det_select.hip: scores + per-level top-k straight from the bf16 logits, B images x L levels) against the two
launches it replaces, bd_det_scores -> bd_segment_topk(min_score): item indices, score BITS and counts must be equal -- the selection
is a total order on (score, item index), so there is no tolerance to choose.

Shapes: the 128x160 pyramid x 9 anchors (rows 2880 / 720 / 180 / 54 / 18, K = 80): the first level spans several of the kernel's
65536-item chunks and -- 230 400 items on at most 65 536 bf16 values -- is full of exactly equal scores; the last level (1440 items)
is shorter than k.  Regimes per case are asserted from the reference's counts, not assumed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RETINA_ROWS = [2880, 720, 180, 54, 18]
FCOS_ROWS = [320, 80, 20, 6, 2]


def _reference(logits, B, rows, K, seg_rows, k, thr, ctr=None, ctr_ld=1, ctr_off=0):
    from basedet_amd import ops
    dev = logits.device
    scores = torch.empty((B, rows * K), dtype=torch.float32, device=dev)
    lg = logits.view(B, rows, K)
    for b in range(B):
        ops.det_scores(lg[b], rows, K, scores[b], ctr=None if ctr is None else ctr.view(B, rows, ctr_ld)[b], ctr_ld=ctr_ld, ctr_off=ctr_off)
    starts = np.concatenate([[0], np.cumsum(seg_rows)[:-1]]).tolist() if len(seg_rows) > 1 else [0]
    L = len(seg_rows)
    idx = torch.empty((B, L, k), dtype=torch.int32, device=dev)
    sc = torch.empty((B, L, k), dtype=torch.float32, device=dev)
    cnt = torch.empty((B, L), dtype=torch.int32, device=dev)
    ops.segment_topk(scores, B, rows * K, 1, 1, 0, [s * K for s in starts], [r * K for r in seg_rows], k, idx, sc, cnt, min_score=thr)
    return idx, sc, cnt, starts


def _check(logits, B, rows, K, seg_rows, k, thr, ctr=None, ctr_ld=1, ctr_off=0, seg_start=None):
    """Runs both forms and requires equal bits; returns the counts [B][L] (host)."""
    from basedet_amd import ops
    dev = logits.device
    ridx, rsc, rcnt, starts = _reference(logits, B, rows, K, seg_rows, k, thr, ctr, ctr_ld, ctr_off)
    L = len(seg_rows)
    idx = torch.full((B, L, k), -7, dtype=torch.int32, device=dev)
    sc = torch.full((B, L, k), -7.0, dtype=torch.float32, device=dev)
    cnt = torch.full((B, L), -7, dtype=torch.int32, device=dev)
    nbytes = ops.det_select_workspace_bytes(B, L, rows, K, k)
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)          # the entry must not rely on a cleared workspace
    ops.det_select(logits, B, rows, K, starts, seg_rows, k, thr, idx, sc, cnt, ws, ctr=ctr, ctr_ld=ctr_ld, ctr_off=ctr_off)
    torch.cuda.synchronize()
    assert torch.equal(cnt, rcnt), (cnt.tolist(), rcnt.tolist())
    assert torch.equal(idx, ridx)
    assert torch.equal(sc.view(torch.int32), rsc.view(torch.int32))
    # second call on the used workspace: same answer
    ops.det_select(logits, B, rows, K, starts, seg_rows, k, thr, idx, sc, cnt, ws, ctr=ctr, ctr_ld=ctr_ld, ctr_off=ctr_off)
    assert torch.equal(idx, ridx) and torch.equal(cnt, rcnt)
    return rcnt.cpu().numpy()


def _logits(B, seg_rows, K, mean, std, seed, level_shift=None):
    g = torch.Generator().manual_seed(seed)
    rows = sum(seg_rows)
    x = torch.randn((B, rows, K), generator=g) * std + mean
    if level_shift:
        o = 0
        for r, d in zip(seg_rows, level_shift):
            x[:, o:o + r] += d
            o += r
    return x.to(torch.bfloat16).cuda().contiguous()


@pytest.mark.parametrize("k", [1000, 2048])
@pytest.mark.parametrize("head", ["retina", "fcos"])
def test_threshold_cuts_one_level_and_not_another(head, k):
    """TEST.CLS_THRESHOLD = 0.05 on logits around -4.5 (about 6 % above the threshold: sigmoid(x) > 0.05 <=> x > -2.94)."""
    seg_rows = RETINA_ROWS if head == "retina" else FCOS_ROWS
    B, K = 3, 80
    lg = _logits(B, seg_rows, K, -4.5 if head == "retina" else -1.0, 1.0, seed=1)
    ctr = None
    if head == "fcos":         # sqrt(sigmoid(x) * sigmoid(c)) > 0.05: centerness in columns 4 of 8
        ctr = (torch.randn((B, sum(seg_rows), 8), generator=torch.Generator().manual_seed(2)) - 1.0).to(torch.bfloat16).cuda()
    cnt = _check(lg, B, sum(seg_rows), K, seg_rows, k, 0.05, ctr=ctr, ctr_ld=8, ctr_off=4)
    print(f"{head} k={k} thr=0.05: counts {cnt.tolist()}")
    if head == "retina":
        assert (cnt[:, 0] == k).all(), "the first level is not cut at k"
    assert ((cnt > 0) & (cnt < k)).any(), "no level keeps fewer than k items"
    if head == "fcos":
        assert (cnt.max(axis=1) > 100).all()


@pytest.mark.parametrize("k", [1000, 2048])
@pytest.mark.parametrize("head", ["retina", "fcos"])
def test_every_item_survives(head, k):
    """min_score = 0: sigmoid > 0 for every finite logit, so all items compete; levels shorter than k come out whole."""
    seg_rows = RETINA_ROWS if head == "retina" else FCOS_ROWS
    B, K = 3, 80
    lg = _logits(B, seg_rows, K, -4.5, 1.0, seed=3)
    ctr = None
    if head == "fcos":
        ctr = torch.randn((B, sum(seg_rows), 8), generator=torch.Generator().manual_seed(4)).to(torch.bfloat16).cuda()
    cnt = _check(lg, B, sum(seg_rows), K, seg_rows, k, 0.0, ctr=ctr, ctr_ld=8, ctr_off=4)
    want = [min(k, r * K) for r in seg_rows]
    assert (cnt == np.asarray(want)[None]).all(), (cnt.tolist(), want)


@pytest.mark.parametrize("k", [1000, 2048])
@pytest.mark.parametrize("head", ["retina", "fcos"])
def test_empty_segments(head, k):
    """0.999 on one image: two levels pushed far below it hold nothing (cnt = 0, every idx -1), the others a few items."""
    seg_rows = RETINA_ROWS if head == "retina" else FCOS_ROWS
    K = 80
    lg = _logits(1, seg_rows, K, 0.0, 3.0 if head == "retina" else 5.0, seed=5, level_shift=[0, 0, -40, 0, -40])
    ctr = None
    if head == "fcos":
        ctr = (torch.randn((1, sum(seg_rows), 8), generator=torch.Generator().manual_seed(6)) + 12.0).to(torch.bfloat16).cuda()
    cnt = _check(lg, 1, sum(seg_rows), K, seg_rows, k, 0.999, ctr=ctr, ctr_ld=8, ctr_off=4)
    print(f"{head} k={k} thr=0.999: counts {cnt.tolist()}")
    assert cnt[0, 2] == 0 and cnt[0, 4] == 0
    assert cnt[0, 0] > 0 and cnt[0, 1] > 0


@pytest.mark.parametrize("thr", [0.0, 0.05])
@pytest.mark.parametrize("k", [1000, 2048])
def test_heavy_ties_need_the_index_digits(k, thr):
    """Seventeen distinct logits: every score is shared by ~13 500 items of the first level, far more than the sort holds, so the
    selection has to run through the lower score digits into the item-index digits to cut a tie group by index."""
    seg_rows = RETINA_ROWS
    B, K = 2, 80
    g = torch.Generator().manual_seed(7)
    x = (torch.randint(0, 17, (B, sum(seg_rows), K), generator=g).float() * 0.25 - 3.0).to(torch.bfloat16).cuda()
    cnt = _check(x, B, sum(seg_rows), K, seg_rows, k, thr)
    assert (cnt[:, 0] == k).all()


@pytest.mark.parametrize("with_ctr", [False, True])
def test_sizes_off_the_vector_and_the_wave(with_ctr):
    """K = 7, rows 37 / 5 / 1: 301 items per image -- no multiple of 8 (the 16-byte load) or 64; images and levels start at odd
    byte offsets, the last vector of every level is partial."""
    seg_rows = [37, 5, 1]
    B, K = 3, 7
    lg = _logits(B, seg_rows, K, -1.0, 2.0, seed=8)
    ctr = None
    if with_ctr:
        ctr = torch.randn((B, sum(seg_rows), 3), generator=torch.Generator().manual_seed(9)).to(torch.bfloat16).cuda()
    for k in (5, 64, 300):
        for thr in (0.0, 0.05, 0.6):
            _check(lg, B, sum(seg_rows), K, seg_rows, k, thr, ctr=ctr, ctr_ld=3, ctr_off=2)


def test_workspace_is_a_fraction_of_the_score_tensor():
    """Batch 16 of RetinaNet at 800x1344 (201 600 anchors x 80 classes): the workspace must stay below 2 % of the fp32 scores it avoids,
    and must not grow with the number of items."""
    from basedet_amd import ops
    ws = ops.det_select_workspace_bytes(16, 5, 201600, 80, 1000)
    assert ws * 50 < 16 * 201600 * 80 * 4
    assert ws == ops.det_select_workspace_bytes(16, 5, 3852, 80, 2048)


def test_refuses_bad_arguments():
    from basedet_amd import _lib, ops
    lg = _logits(1, [4], 8, 0.0, 1.0, seed=0)
    idx = torch.empty((1, 1, 4096), dtype=torch.int32, device="cuda")
    sc = torch.empty((1, 1, 4096), dtype=torch.float32, device="cuda")
    cnt = torch.empty((1, 1), dtype=torch.int32, device="cuda")
    ws = torch.empty((ops.det_select_workspace_bytes(1, 1, 4, 8, 8),), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.BasedetHipError):
        ops.det_select(lg, 1, 4, 8, [0], [4], 4096, 0.05, idx, sc, cnt, ws)           # k > 2048
    with pytest.raises(_lib.BasedetHipError):
        ops.det_select(lg, 1, 4, 8, [2], [4], 8, 0.05, idx, sc, cnt, ws)              # segment past the rows
    with pytest.raises(_lib.BasedetHipError):
        ops.det_select(lg, 1, 4, 8, [0], [4], 8, 0.05, idx, sc, cnt, ws[:1024])       # workspace too small
