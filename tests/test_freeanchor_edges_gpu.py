"""FreeAnchor bag-loss kernels (csrc/freeanchor.hip) at the trained class count, at the launcher's limits and on the branches random
inputs never reach, against the float64 form of the oracle (oracle/freeanchor.py, dtype=torch.float64: float64 arithmetic on the fp32
selections, so kernel and oracle pick the same anchors).

Measures (`_check`).  Losses: 1e-4 relative.  Gradients, with REL = 2^-8 (one bf16 rounding, REL_BF16 of tests/audit.py):
  * per element             |got - ref| <= REL |ref| + ABS
  * rel-L2 over a set of n  ||got - ref|| <= REL ||ref|| + ABS sqrt(n)      (what the per-element bound sums to)
    - d_offsets: every (image, gt) bag over its own anchors, and the union of an image's bags;
    - d_logits: the bag entries (anchor in a bag, that gt's class), and all other entries (negative-loss gradient only);
  * d_offsets is exactly zero outside the bags and in the padding columns.
ABS is the fp32-ordering term: 8 x frac x max |ref| of the tensor, where frac is the largest deviation of the FP32 oracle from the
float64 oracle on the same inputs, as a fraction of max |ref|.  Each case measures its own frac on the CPU before it asserts (and
prints it).  Measured when the cases were written: d_logits 1.2e-7 .. 4.5e-7 of max |ref| on every case but the confident bag, where it
is 6.7e-6 (p = 0.9997: 1 - p keeps 12 of fp32's 24 bits); d_offsets 7.4e-8 .. 3.6e-7.  With the margin of 8, ABS is about 1e-6 .. 4e-6
of the largest gradient (5e-5 on the confident bag): the margin covers the kernel's other summation order (bag members by ascending anchor
index, the oracle's by descending IoU) and its exp / log / reciprocal instructions, one ulp each.  One bf16 rounding alone reaches 0.99
of the per-element bound on tensors of this size, so a result that is rounded twice (a sum kept in bf16) does not pass.

Out of range: a bag member with logit +30 has p == 1 in fp32, w = 1 / (1 - p) divides by zero and the original model's formula gives
NaN -- not a property of this port, so the confident bag stops at logit +8."""
import functools

import numpy as np
import pytest
import torch

from tests.test_freeanchor_gpu import _problem

pytestmark = pytest.mark.gpu

REL = 2.0 ** -8
MARGIN = 8.0
STD = (0.1, 0.1, 0.2, 0.2)
T1 = 0.6
FLT_MIN = float(np.finfo(np.float32).tiny)


# ---- problems ----------------------------------------------------------------------------------------------------------------------------
def _anchors(sizes=((16, 20), (8, 10), (4, 5)), strides=(8, 16, 32)):
    return _problem(0, N=1, K=1, sizes=sizes, strides=strides)[0]


def _predictions(rng, anchors, gt, num, K):
    """As _problem: offsets = the encoded best-matching gt, shrunk and with noise; logits from N(-2, 1.5)."""
    from oracle import box_ops
    N, A = gt.shape[0], anchors.shape[0]
    offsets = np.zeros((N, A, 4), np.float32)
    for n in range(N):
        best = box_ops.box_iou(gt[n, :max(1, num[n]), :4], anchors).argmax(0)
        tgt = box_ops.box_encode(anchors, gt[n, best, :4], (0, 0, 0, 0), STD)
        offsets[n] = np.clip(tgt, -8, 8) * rng.uniform(0.6, 1.0, (A, 1)).astype(np.float32) + rng.normal(0, 0.3, (A, 4)).astype(np.float32)
    logits = rng.normal(-2.0, 1.5, (N, A, K)).astype(np.float32)
    return logits, offsets


def _boxes(rng, g, K, lo=(20, 20), hi=(140, 108), size=(16, 90), classes=None):
    cx, cy = rng.uniform(lo[0], hi[0], g), rng.uniform(lo[1], hi[1], g)
    w, h = rng.uniform(size[0], size[1], g), rng.uniform(size[0], size[1], g)
    out = np.zeros((g, 5), np.float32)
    out[:, 0] = np.clip(cx - w / 2, 0, 160); out[:, 1] = np.clip(cy - h / 2, 0, 128)
    out[:, 2] = np.clip(cx + w / 2, 0, 160); out[:, 3] = np.clip(cy + h / 2, 0, 128)
    out[:, 4] = rng.integers(1, (classes or K) + 1, g)
    return out


def _case(anchors, gt, num, logits, offsets, bucket=50, beta=0.0, apix=9, ld=40):
    """The operands as the kernel reads them (bf16) plus the launch parameters."""
    return dict(anchors=anchors, gt=gt, num=np.asarray(num, np.int32), lg=torch.from_numpy(logits).to(torch.bfloat16),
                of=torch.from_numpy(offsets).to(torch.bfloat16), bucket=bucket, beta=beta, apix=apix, ld=ld)


@functools.lru_cache(maxsize=None)
def _many_boxes(nums=(40, 17), K=80, seed=11):
    """Gmax = 40, boxes drawn in the middle third of the image and from 8 classes: bags overlap, also within one class."""
    rng = np.random.default_rng(seed)
    anchors = _anchors()
    gt = np.zeros((len(nums), 40, 5), np.float32)
    for n, g in enumerate(nums):
        gt[n, :g] = _boxes(rng, g, K, lo=(50, 40), hi=(110, 88), size=(24, 80), classes=8)
    logits, offsets = _predictions(rng, anchors, gt, nums, K)
    return _case(anchors, gt, nums, logits, offsets)


# ---- oracle and launch -------------------------------------------------------------------------------------------------------------------
def _oracle(c, dtype):
    from oracle import freeanchor
    lt = c["lg"].to(dtype).clone().requires_grad_(True)
    ot = c["of"].to(dtype).clone().requires_grad_(True)
    aux = []
    pos, neg = freeanchor.bag_losses(lt, ot, c["anchors"], c["gt"], c["num"], std=STD, iou_thresh=T1, bucket=c["bucket"],
                                     beta=c["beta"], reg_weight=0.75, alpha=0.25, gamma=2.0, dtype=dtype, aux=aux)
    (pos + neg).backward()
    d_of = ot.grad if ot.grad is not None else torch.zeros_like(ot)              # no box in any image: offsets are not in the graph
    return dict(pos=float(pos.detach()), neg=float(neg.detach()), d_lg=lt.grad.double(), d_of=d_of.double(), aux=aux)


def _launch(c, K=None, bucket=None, fill=None):
    """One bd_freeanchor_loss_fwd_bwd into fresh buffers; returns (loss (2,) float64 numpy, d_logits (N, A, K), d_offsets (N, A, 4),
    padding columns of d_offsets), all on the CPU.  fill: the three output buffers to use instead (validation tests)."""
    from basedet_amd import ops
    dev = "cuda"
    N, A, Kc = c["lg"].shape
    K = Kc if K is None else K
    bucket = c["bucket"] if bucket is None else bucket
    apix, ld = c["apix"], c["ld"]
    off_dev = torch.zeros((N * (A // apix), ld), dtype=torch.bfloat16, device=dev)
    off_dev[:, :apix * 4] = c["of"].reshape(N * (A // apix), apix * 4).to(dev)
    lg_dev = c["lg"].reshape(N * A, Kc).to(dev)
    if fill is None:
        d_lg, d_of = torch.full_like(lg_dev, 7.0), torch.full_like(off_dev, 7.0)
        loss = torch.zeros(2, dtype=torch.float32, device=dev)
    else:
        d_lg, d_of, loss = fill
    ws = torch.empty(ops.freeanchor_workspace_bytes(N, c["gt"].shape[1], bucket, A), dtype=torch.uint8, device=dev)
    ops.freeanchor_loss_fwd_bwd(lg_dev, off_dev, ld, apix, torch.from_numpy(c["anchors"]).to(dev), K, torch.from_numpy(c["gt"]).to(dev),
                                torch.from_numpy(c["num"]).to(dev), (0, 0, 0, 0), STD, T1, bucket, c["beta"], 0.75, 0.25, 2.0,
                                loss, d_lg, d_of, ws)
    torch.cuda.synchronize()
    g_o = d_of.float().cpu()
    return (loss.cpu().numpy().astype(np.float64), d_lg.float().cpu().reshape(N, A, K).double(),
            g_o[:, :apix * 4].reshape(N, A, 4).double(), g_o[:, apix * 4:])


def _membership(c, ref):
    """(bags, in_bag (N, A) bool, entry (N, A, K) bool): bags = [(image, gt, anchor indices)]."""
    N, A, K = c["lg"].shape
    in_bag = torch.zeros((N, A), dtype=torch.bool)
    entry = torch.zeros((N, A, K), dtype=torch.bool)
    bags = []
    for n, rec in enumerate(ref["aux"]):
        for g in range(int(c["num"][n])):
            idx = torch.from_numpy(rec["order"][g].astype(np.int64))
            bags.append((n, g, idx))
            in_bag[n, idx] = True
            entry[n, idx, int(rec["labels"][g])] = True
    return bags, in_bag, entry


def _check(c, ref=None, got=None):
    """Every measure of the module docstring; prints each figure as err / bound before asserting them all.  Returns (ref, got)."""
    ref = _oracle(c, torch.float64) if ref is None else ref
    assert np.isfinite(ref["pos"]) and np.isfinite(ref["neg"]) and bool(torch.isfinite(ref["d_lg"]).all()) \
        and bool(torch.isfinite(ref["d_of"]).all()), "the reference is not finite on this input"
    r32 = _oracle(c, torch.float32)
    got = _launch(c) if got is None else got
    loss, g_l, g_o, pad = got
    r_l, r_o = ref["d_lg"], ref["d_of"]
    fig = {}
    scale_l, scale_o = float(r_l.abs().max()), float(r_o.abs().max())
    frac_l = float((r32["d_lg"] - r_l).abs().max()) / scale_l
    frac_o = float((r32["d_of"] - r_o).abs().max()) / scale_o if scale_o > 0 else 0.0
    abs_l, abs_o = MARGIN * frac_l * scale_l, MARGIN * frac_o * scale_o
    print(f"fp32 oracle vs float64 oracle: d_logits {frac_l:.3e}, d_offsets {frac_o:.3e} of the tensor's max |ref|")
    for name, g, r in (("pos", loss[0], ref["pos"]), ("neg", loss[1], ref["neg"])):
        fig["loss " + name] = abs(g - r) / (1e-4 * abs(r)) if r != 0 else (0.0 if g == 0 else float("inf"))

    def l2(name, g, r, abs_):
        bound = REL * float(r.norm()) + abs_ * float(np.sqrt(r.numel()))
        err = float((g - r).norm())
        fig[name] = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))

    def elem(name, g, r, abs_):
        err, bound = (g - r).abs(), REL * r.abs() + abs_
        fig[name] = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max()) if r.numel() else 0.0

    bags, in_bag, entry = _membership(c, ref)
    worst = 0.0
    for n, g, idx in bags:
        l2("tmp", g_o[n, idx], r_o[n, idx], abs_o)
        worst = max(worst, fig.pop("tmp"))
    fig["d_offsets rel-L2, worst bag"] = worst
    for n in range(c["lg"].shape[0]):
        l2(f"d_offsets rel-L2, union of image {n}", g_o[n][in_bag[n]], r_o[n][in_bag[n]], abs_o)
    l2("d_logits rel-L2, bag entries", g_l[entry], r_l[entry], abs_l)
    l2("d_logits rel-L2, other entries", g_l[~entry], r_l[~entry], abs_l)
    elem("d_logits per element, bag entries", g_l[entry], r_l[entry], abs_l)
    elem("d_logits per element, other entries", g_l[~entry], r_l[~entry], abs_l)
    elem("d_offsets per element", g_o, r_o, abs_o)
    for k, v in fig.items():
        print(f"{k}: {v:.4f} of its bound")
    assert bool((pad == 0).all()), "padding columns of d_offsets"
    assert bool((g_o[~in_bag] == 0).all()), "d_offsets outside every bag"
    assert bool(((r_o.abs().sum(-1) == 0) == (g_o.abs().sum(-1) == 0)).all()), "zero pattern of d_offsets"
    bad = {k: v for k, v in fig.items() if not v <= 1.0}
    assert not bad, bad
    ref["abs_lg"], ref["abs_of"] = abs_l, abs_o
    return ref, got


# ---- K and bucket grid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,bucket", [(80, 50), (128, 50), (80, 1), (80, 64)])
def test_class_count_and_bucket_grid(K, bucket):
    """The trained class count (a 40 KB LDS tile), the largest K the launcher takes (64 KB), and both ends of the bucket range."""
    anchors, gt, num, logits, offsets = _problem(20 + K + bucket, K=K)
    assert int(gt[..., 4].max()) > 16 and int(num.max()) == 6                     # classes beyond the K = 16 of the other file
    _check(_case(anchors, gt, num, logits, offsets, bucket=bucket))


@pytest.mark.parametrize("K,bucket", [(129, 50), (80, 65)])
def test_refused_launch_writes_nothing(K, bucket):
    anchors, gt, num, logits, offsets = _problem(5, K=K)
    c = _case(anchors, gt, num, logits, offsets, bucket=bucket)
    N, A, _ = logits.shape
    d_lg = torch.empty((N * A, K), dtype=torch.bfloat16, device="cuda")
    d_of = torch.empty((N * (A // 9), 40), dtype=torch.bfloat16, device="cuda")
    loss = torch.empty(2, dtype=torch.float32, device="cuda")
    d_lg.view(torch.int16).fill_(0x7fc1); d_of.view(torch.int16).fill_(0x7fc1); loss.view(torch.int32).fill_(0x7fc00001)
    with pytest.raises(RuntimeError):
        _launch(c, fill=(d_lg, d_of, loss))
    torch.cuda.synchronize()
    assert bool((d_lg.view(torch.int16) == 0x7fc1).all()) and bool((d_of.view(torch.int16) == 0x7fc1).all())
    assert bool((loss.view(torch.int32) == 0x7fc00001).all())
    K1 = min(K, 128)                                                               # and the neighbour inside the limits runs
    _launch(_case(anchors, gt, num, logits[..., :K1], offsets, bucket=min(bucket, 64)), fill=(d_lg[:, :K1].contiguous(), d_of, loss))
    assert not bool((d_of.view(torch.int16) == 0x7fc1).any()) and not bool((loss.view(torch.int32) == 0x7fc00001).any())


# ---- fewer candidates than the bucket ----------------------------------------------------------------------------------------------------
def test_bucket_larger_than_anchor_count():
    """A one-level 2 x 2 pyramid has 36 anchors, bucket 50: fa_gt_kernel's radix select reports take_all (fewer than `bucket` valid
    keys), falls back from the positive-IoU candidates to all anchors, and the bag is all 36 anchors -- min(bucket, A) of the oracle.
    The normaliser of the negative loss keeps `bucket` in both."""
    anchors = _anchors(sizes=((2, 2),), strides=(32,))
    assert anchors.shape[0] == 36
    rng = np.random.default_rng(3)
    gt = np.zeros((2, 2, 5), np.float32)
    gt[0, 0] = [4, 6, 60, 58, 3]; gt[0, 1] = [0, 0, 2.5, 2.5, 7]; gt[1, 0] = [10, 20, 50, 64, 1]
    num = [2, 1]
    logits, offsets = _predictions(rng, anchors, gt, num, 16)
    c = _case(anchors, gt, num, logits, offsets, bucket=50, ld=36)
    ref = _oracle(c, torch.float64)
    mq = ref["aux"][0]["mq"]
    assert ref["aux"][0]["order"].shape == (2, 36)
    assert int((mq[0] > 0).sum()) == 36 and 0 < int((mq[1] > 0).sum()) < 36          # with and without the fall-back to zero-IoU anchors
    _check(c, ref=ref)


def test_fewer_overlapping_anchors_than_bucket():
    """2880 anchors of one level, bucket 50, small boxes just beyond two corners of the image (an anchor spans four strides: inside the
    image more than 64 anchors touch any box) that 21 and 33 anchors touch: the second selection pass over all anchors fills the bag
    with zero-IoU anchors, lowest index first (the tie rule at IoU 0)."""
    anchors = _anchors(sizes=((16, 20),), strides=(8,))
    rng = np.random.default_rng(4)
    gt = np.zeros((2, 2, 5), np.float32)
    gt[0, 0] = [170, 134, 176, 140, 2]; gt[0, 1] = [30, 30, 110, 100, 5]; gt[1, 0] = [-12, -10, -6, -4, 2]
    num = [2, 1]
    logits, offsets = _predictions(rng, anchors, gt, num, 16)
    c = _case(anchors, gt, num, logits, offsets, bucket=50)
    ref = _oracle(c, torch.float64)
    for n, g in ((0, 0), (1, 0)):
        mq, order = ref["aux"][n]["mq"][g], ref["aux"][n]["order"][g]
        npos = int((mq > 0).sum())
        assert 0 < npos < 50 and anchors.shape[0] - npos > 50 - npos                 # zero-IoU ties cross the bucket boundary
        zeros = np.nonzero(mq == 0)[0]
        assert (order[npos:] == zeros[:50 - npos]).all()
    _check(c, ref=ref)


# ---- many boxes --------------------------------------------------------------------------------------------------------------------------
def test_many_overlapping_boxes():
    c = _many_boxes()
    ref = _oracle(c, torch.float64)
    for n in range(2):
        cnt = np.bincount(ref["aux"][n]["order"].reshape(-1), minlength=c["anchors"].shape[0])
        assert (cnt >= 2).sum() >= 0.25 * (cnt >= 1).sum() and (cnt >= 3).any(), "bags do not overlap enough"
    lab, order = ref["aux"][0]["labels"], ref["aux"][0]["order"]
    assert any(lab[a] == lab[b] and np.intersect1d(order[a], order[b]).size for a in range(40) for b in range(a)), \
        "no two bags of one class share an anchor"
    _check(c, ref=ref)


def test_many_boxes_and_an_image_without():
    c = _many_boxes(nums=(40, 0, 17))
    ref, (loss, g_l, g_o, pad) = _check(c)
    assert ref["aux"][1] == {} and bool((g_o[1] == 0).all())


def test_no_boxes_at_all():
    c = _many_boxes(nums=(0, 0))
    ref, (loss, g_l, g_o, pad) = _check(c)
    assert ref["pos"] == 0.0 and loss[0] == 0.0 and bool((g_o == 0).all())
    # neg normalised by max(1, 0 * bucket) = 1: the plain sum of q^2 * -log(1 - q) over all logits, times 1 - alpha
    q = torch.sigmoid(c["lg"].double())
    want = 0.75 * float((q * q * -torch.log1p(-q)).sum())
    assert abs(ref["neg"] - want) <= 1e-12 * want and abs(loss[1] - want) <= 1e-4 * want


def test_same_bits_twice():
    """The header of freeanchor.hip promises fixed-order reductions: two launches into fresh buffers give the same bits."""
    c = _many_boxes()
    a, b = _launch(c), _launch(c)
    assert float(np.abs(a[0]).min()) > 0 and float(a[2].abs().max()) > 0
    assert np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ---- the later gt wins per (anchor, class) -------------------------------------------------------------------------------------------------
def test_later_gt_wins_shared_anchor_and_class():
    """Three boxes of one class a few pixels apart, predictions aimed at the middle one.  On anchors whose prediction overlaps several of
    them the LAST gt with a non-zero box probability stands (oracle: indexed assignment at `nonzero`; kernel: 64-bit atomicMax on
    (gt index, value)), whether its value is smaller than an earlier one -- which separates it from 'largest wins' -- or an even later
    gt's value is exactly 0 -- which separates it from 'highest index wins'."""
    rng = np.random.default_rng(7)
    anchors = _anchors()
    K, cls = 80, 37
    gt = np.zeros((2, 6, 5), np.float32)
    gt[0, 0] = [40, 30, 100, 90, cls]; gt[0, 1] = [44, 33, 104, 93, cls]; gt[0, 2] = [49, 37, 109, 97, cls]
    gt[0, 3] = [100, 20, 150, 70, 5]
    gt[1, :3] = _boxes(rng, 3, K)
    num = [4, 3]
    logits, offsets = _predictions(rng, anchors, gt, num, K)
    from oracle import box_ops
    near = box_ops.box_iou(gt[0, 1:2, :4], anchors)[0] > 0.2                      # aim these at the middle box, loosely
    tgt = box_ops.box_encode(anchors, np.repeat(gt[0, 1:2, :4], anchors.shape[0], 0), (0, 0, 0, 0), STD)
    offsets[0][near] = (tgt + rng.normal(0, 0.25, tgt.shape).astype(np.float32))[near]
    c = _case(anchors, gt, num, logits, offsets)
    ref = _oracle(c, torch.float64)
    gp = ref["aux"][0]["gp"]
    earlier = np.maximum(gp[0], gp[1])
    smaller = np.nonzero((gp[2] != 0) & (gp[2] < earlier))[0]                     # (a) last < earlier, both non-zero
    absent = np.nonzero((gp[2] == 0) & (earlier != 0))[0]                         # (b) last exactly 0, an earlier one is not
    both = np.nonzero((gp[2] == 0) & (gp[1] != 0) & (gp[0] > gp[1]))[0]           # and there the middle one stands, not the largest
    assert smaller.size >= 5 and absent.size >= 5 and both.size >= 1, (smaller.size, absent.size, both.size)
    assert bool((gp[1][smaller] > gp[2][smaller]).any()), "the middle box never has the largest value"
    _, (loss, g_l, g_o, pad) = _check(c, ref=ref)
    # per element on exactly those anchors at that class; the gradients of 'largest wins' / 'highest index wins' differ from the
    # reference there by far more than the bound (asserted, so the comparison cannot pass vacuously)
    sel = torch.from_numpy(np.concatenate([smaller, absent]))
    r, g = ref["d_lg"][0, sel, cls - 1], g_l[0, sel, cls - 1]
    n_fg = float(sum(num)) * 50

    def neg_grad(bp):
        s = torch.sigmoid(c["lg"][0, sel, cls - 1].double())
        q = s * (1 - bp)
        return 0.75 / n_fg * (2 * q * -torch.log1p(-q) + q * q / (1 - q)) * s * (1 - s) * (1 - bp)
    wrong = neg_grad(torch.from_numpy(np.concatenate([earlier[smaller], np.zeros(absent.size)])).double())
    right = neg_grad(torch.from_numpy(np.concatenate([gp[2][smaller], np.where(gp[1] != 0, gp[1], gp[0])[absent]])).double())
    bound = REL * r.abs() + ref["abs_lg"]
    assert int(((wrong - right).abs() > 4 * bound).sum()) >= 5, "the wrong rules would pass on these inputs"
    assert bool(((g - r).abs() <= bound).all()), float(((g - r).abs() / bound).max())


# ---- ties at the bucket boundary -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bucket", [3, 48, 64])
def test_ties_across_the_bucket_boundary(bucket):
    """Square boxes centred on an anchor centre of each level: the ratio 0.5 and ratio 2 anchors of one location, and the locations
    mirrored about the centre, have the same IoU in fp32.  At these buckets the k-th and (k+1)-th largest IoU of every box are equal, and
    the bag takes the lowest anchor index."""
    rng = np.random.default_rng(9)
    anchors = _anchors()

    def sq(cx, cy, s, cls):
        return [cx - s / 2, cy - s / 2, cx + s / 2, cy + s / 2, cls]
    gt = np.zeros((2, 3, 5), np.float32)
    gt[0] = [sq(8 * 7 + 4, 8 * 6 + 4, 40, 3), sq(16 * 4 + 8, 16 * 3 + 8, 80, 9), sq(32 * 2 + 16, 32 * 2 + 16, 120, 3)]
    gt[1, :2] = [sq(16 * 6 + 8, 16 * 4 + 8, 80, 1), sq(8 * 12 + 4, 8 * 9 + 4, 40, 16)]
    num = [3, 2]
    logits, offsets = _predictions(rng, anchors, gt, num, 16)
    c = _case(anchors, gt, num, logits, offsets, bucket=bucket)
    ref = _oracle(c, torch.float64)
    for n in range(2):
        for g in range(num[n]):
            mq, order = ref["aux"][n]["mq"][g], ref["aux"][n]["order"][g]
            s = -np.sort(-mq)
            assert s[bucket - 1] == s[bucket] and s[bucket] > 0, (n, g, "no tie at the boundary")
            tied = np.nonzero(mq == s[bucket])[0]
            taken = np.intersect1d(order, tied)
            assert 0 < taken.size < tied.size and taken.max() < np.setdiff1d(tied, order).min()
    _, (loss, g_l, g_o, pad) = _check(c, ref=ref)
    _, in_bag, _ = _membership(c, ref)
    assert bool(((ref["d_of"].abs().sum(-1) != 0) == in_bag).all())               # every member has a gradient: the pattern is the bag
    assert bool(((g_o.abs().sum(-1) != 0) == in_bag).all())


# ---- saturation ----------------------------------------------------------------------------------------------------------------------------
def _saturation_base(seed):
    rng = np.random.default_rng(seed)
    anchors = _anchors()
    K = 80
    gt = np.zeros((2, 6, 5), np.float32)
    gt[0, :4] = _boxes(rng, 4, K, size=(30, 80))
    gt[1, :3] = _boxes(rng, 3, K, size=(30, 80))
    num = [4, 3]
    logits, offsets = _predictions(rng, anchors, gt, num, K)
    return anchors, gt, num, logits, offsets


def test_confident_bag_member():
    """One bag member with logit +8 and offsets equal to the encoded gt: p = 0.9997, its weight 1 / (1 - p) is about 3000 and 1 - p keeps
    half of fp32's bits.  (Logit +30: see the module docstring.)"""
    from oracle import box_ops
    anchors, gt, num, logits, offsets = _saturation_base(13)
    c0 = _case(anchors, gt, num, logits, offsets)
    order = _oracle(c0, torch.float32)["aux"][0]["order"]
    a, cls = int(order[1][0]), int(gt[0, 1, 4]) - 1
    logits[0, a, cls] = 8.0
    offsets[0, a] = box_ops.box_encode(anchors[a:a + 1], gt[0, 1:2, :4], (0, 0, 0, 0), STD)[0]
    c = _case(anchors, gt, num, logits, offsets, beta=0.11)
    ref = _oracle(c, torch.float64)
    tgt = box_ops.box_encode(anchors[a:a + 1], gt[0, 1:2, :4], (0, 0, 0, 0), STD)[0]
    d = np.abs(c["of"][0, a].double().numpy() - tgt)                              # what bf16 storage leaves of offsets - target
    reg = 0.75 * float(np.where(d < 0.11, 0.5 * d * d / 0.11, d - 0.055).sum())
    p = float(torch.sigmoid(torch.tensor(8.0, dtype=torch.float64))) * np.exp(-reg)
    assert float(c["lg"][0, a, cls]) == 8.0 and 0.999 < p < 1.0, p
    _check(c, ref=ref)


def test_underflowed_bag():
    """Every member of one bag has logit -120 at the gt's class: sigmoid is 0 in fp32 (7.7e-53 in float64, below FLT_MIN as well), the
    bag's probability is clamped by safelog, its loss is -log(FLT_MIN) and nothing flows back through the clamp."""
    anchors, gt, num, logits, offsets = _saturation_base(14)
    gt[0, 2, 4] = 77                                                               # a class no other box of the image has
    assert (gt[0, [0, 1, 3], 4] != 77).all()
    c0 = _case(anchors, gt, num, logits, offsets)
    members = _oracle(c0, torch.float32)["aux"][0]["order"][2]
    logits[0, members, 76] = -120.0
    c = _case(anchors, gt, num, logits, offsets)
    assert bool((torch.sigmoid(c["lg"][0, torch.from_numpy(members), 76].float()) == 0).all())
    ref = _oracle(c, torch.float64)
    _, (loss, g_l, g_o, pad) = _check(c, ref=ref)
    # the loss of that bag, and exact zeros: d_logits of its entries (the negative part is 0 as well: q = 0), d_offsets of the anchors
    # that are in no other bag
    others = ref["pos"] - 0.25 * -np.log(FLT_MIN) / 7
    assert others > 0 and abs(loss[0] - ref["pos"]) <= 1e-4 * others               # tighter than 1e-4 of the total
    m = torch.from_numpy(members)
    assert float(ref["d_lg"][0, m, 76].abs().max()) < 1e-100 and bool((g_l[0, m, 76] == 0).all())         # float64: q^2 = 6e-105, not 0
    rest = np.setdiff1d(members, np.concatenate([ref["aux"][0]["order"][g] for g in (0, 1, 3)]))
    assert rest.size > 0
    assert bool((ref["d_of"][0, torch.from_numpy(rest)] == 0).all()) and bool((g_o[0, torch.from_numpy(rest)] == 0).all())


def test_box_prob_one_and_threshold_fallback():
    """(a) At a gt's arg-max prediction the rescaled IoU is exactly 1: q = 0, and with that anchor outside every bag of the class both
    the negative loss term and d_logits are exactly 0.  (b) A gt none of whose predictions reaches IoU 0.6 takes t2 = t1 + 1e-7 and
    gives no box probability at all."""
    from oracle import box_ops
    anchors, gt, num, logits, offsets = _saturation_base(15)
    gt[0, 3] = [70, 4, 82, 124, 60]                                                # (b) 12 x 120: no anchor shape comes close
    best = box_ops.box_iou(gt[0, :4, :4], anchors).argmax(0)
    offsets[0][best == 3] = 0                                                      # and its anchors predict themselves
    c0 = _case(anchors, gt, num, logits, offsets)
    aux0 = _oracle(c0, torch.float32)["aux"]
    picks = []
    for n, g in ((0, 0), (0, 1), (1, 0)):                                          # (a) an anchor outside the bag predicts the gt exactly
        mq, order = aux0[n]["mq"][g], aux0[n]["order"]
        cand = [a for a in np.argsort(-mq, kind="stable")[50:] if not any(a in o for o in order)]
        a = int(cand[0])
        assert mq[a] > 0.1
        offsets[n, a] = box_ops.box_encode(anchors[a:a + 1], gt[n, g:g + 1, :4], (0, 0, 0, 0), STD)[0]
        picks.append((n, g, a))
    c = _case(anchors, gt, num, logits, offsets)
    ref = _oracle(c, torch.float64)
    _, (loss, g_l, g_o, pad) = _check(c, ref=ref)
    _, in_bag, _ = _membership(c, ref)
    for n, g, a in picks:
        rec = ref["aux"][n]
        cls = int(rec["labels"][g])
        assert int(rec["ov"][g].argmax()) == a and rec["gp"][g][a] == 1.0 and not bool(in_bag[n, a])
        later = [h for h in range(g + 1, int(num[n])) if rec["labels"][h] == cls]
        assert all(rec["gp"][h][a] == 0 for h in later)
        assert float(ref["d_lg"][n, a, cls]) == 0.0 and float(g_l[n, a, cls]) == 0.0
    rec = ref["aux"][0]
    assert float(rec["ov"][3].max()) < T1 and rec["t2"][3, 0] == np.float32(np.float32(T1) + np.float32(1e-7))
    assert not rec["gp"][3].any()
