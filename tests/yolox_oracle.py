"""Numpy / torch float64 statement of YOLOX behind the head's last convolutions (SimOTA assignment, the four losses, the inference
decode), written from the description of bd_yolox_* in include/basedet_hip.h, plus the problems the YOLOX tests share.  Inputs are bf16
values held in float64.  The gt is xyxy everywhere; both IoUs are between the gt box and the decoded prediction.

assign(prob) is the literal form: the class cost is summed over the K one-hot columns, everything in float64.
assign(prob, dtype=np.float32, reassoc=True) rounds every intermediate to float32 and forms the class cost as
(S_bg - bce0(s_c)) + bce1(s_c), as the kernel does: the CPU tests use it to show that the shared problems do not rest on a rounding."""
import functools

import numpy as np
import torch

STRIDES = (8, 16, 32)
LOG_FLOOR = 1e-30
# (N, input H, input W, K, Gmax) of the assignment and loss tests
SHAPES = [(1, 64, 64, 1, 1), (2, 96, 160, 3, 7), (3, 256, 256, 20, 40), (2, 640, 640, 80, 120)]
SEEDS = {SHAPES[0]: 3, SHAPES[1]: 1, SHAPES[2]: 2, SHAPES[3]: 5}


def bf16(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def ld_of(K):
    return (K + 7) // 8 * 8


def level_sizes(H, W, strides=STRIDES):
    return [(H // s, W // s) for s in strides]


def points(sizes, strides=STRIDES):
    """Per level (col * stride, row * stride), row-major; -> (points (P, 2) float32, lvl_start, stride per point)."""
    pts, st, start = [], [], [0]
    for (h, w), s in zip(sizes, strides):
        ys, xs = np.divmod(np.arange(h * w), w)
        pts.append(np.stack([xs * s, ys * s], 1))
        st.append(np.full(h * w, s))
        start.append(start[-1] + h * w)
    return np.concatenate(pts).astype(np.float32), start, np.concatenate(st).astype(np.float64)


def decode(raw, pts, stride):
    """raw (..., P, 4) -> xc, yc, w, h (yolox.py:162-164)."""
    raw = np.asarray(raw, np.float64)
    return np.stack([raw[..., 0] * stride + pts[:, 0], raw[..., 1] * stride + pts[:, 1], stride * np.exp(raw[..., 2]),
                     stride * np.exp(raw[..., 3])], -1)


def _sig(x):
    e = np.exp(-np.abs(x))
    inv = 1.0 / (1.0 + e)
    return np.where(x >= 0, inv, e * inv), np.where(x >= 0, e * inv, inv), np.minimum(x, 0) - np.log1p(e)       # p, q, log p


def in_tests(pts, stride, gt):
    """(in_box, in_centre) (G, P): get_in_boxes_info, both tests strict."""
    px, py = pts[None, :, 0].astype(np.float64), pts[None, :, 1].astype(np.float64)
    x1, y1, x2, y2 = (gt[:, i, None].astype(np.float64) for i in range(4))
    in_box = np.minimum(np.minimum(px - x1, py - y1), np.minimum(x2 - px, y2 - py)) > 0
    cx, cy, r = (x1 + x2) / 2, (y1 + y2) / 2, 2.5 * stride[None, :]
    in_ctr = np.minimum(np.minimum(px - (cx - r), py - (cy - r)), np.minimum((cx + r) - px, (cy + r) - py)) > 0
    return in_box, in_ctr


def _image_assign(cls, box_obj, pts, stride, gt, K, dtype, reassoc):
    """One image: matched (P,), iou_t (P,), aux."""
    P = pts.shape[0]
    matched, iou_t = np.full(P, -1, np.int64), np.zeros(P, np.float64)
    G = gt.shape[0]
    aux = dict(cand=np.zeros(0, np.int64), G=G)
    if G == 0:
        return matched, iou_t, aux
    f = lambda a: np.asarray(a, dtype)
    in_box, in_ctr = in_tests(pts, stride, gt)
    cand = np.nonzero((in_box | in_ctr).any(0))[0]
    aux.update(cand=cand, in_box=in_box[:, cand], in_ctr=in_ctr[:, cand])
    if cand.size == 0:
        return matched, iou_t, aux
    # point-relative coordinates: IoU is translation invariant, and this is where the kernel rounds
    p = pts[cand].astype(np.float64)
    raw = box_obj[cand, :4].astype(np.float64)
    s = stride[cand]
    dec = np.stack([f(raw[:, 0] * s), f(raw[:, 1] * s), f(s * f(np.exp(f(raw[:, 2])))), f(s * f(np.exp(f(raw[:, 3]))))], 1)
    iou = np.zeros((G, cand.size), dtype)
    for g in range(G):
        rel = gt[g, :4].astype(np.float64)[None, :] - np.concatenate([p, p], 1)
        iou[g] = _iou_rows(f(rel), dec, dtype)
    pc, qc, lpc = (f(v) for v in _sig(f(cls[cand, :K].astype(np.float64))))
    po, qo, lpo = (f(v) for v in _sig(f(box_obj[cand, 4].astype(np.float64))))
    sk = f(np.sqrt(f(pc * po[:, None])))
    u = f(f(qc + qo[:, None]) - f(qc * qo[:, None]))
    bce0 = f(-np.log(np.maximum(f(u / f(1 + sk)), dtype(LOG_FLOOR))))
    bce1 = f(-0.5 * f(lpc + lpo[:, None]))
    lab = gt[:, 4].astype(np.int64) - 1
    cost = np.zeros((G, cand.size), dtype)
    if reassoc:
        sbg = np.zeros(cand.size, dtype)
        for k in range(K):
            sbg = f(sbg + bce0[:, k])
    for g in range(G):
        c = lab[g]
        if reassoc:
            cc = f(f(sbg - bce0[:, c]) + bce1[:, c]) if 0 <= c < K else sbg
        else:
            row = bce0.copy()
            if 0 <= c < K:
                row[:, c] = bce1[:, c]
            cc = row.sum(1)
        pen = np.where(in_box[g, cand] & in_ctr[g, cand], 0.0, 1e5).astype(dtype)
        cost[g] = f(f(cc + f(3 * f(-np.log(f(iou[g] + dtype(1e-8)))))) + pen)
    # dynamic k: the min(10, C) largest IoUs, summed largest first
    top = -np.sort(-iou, axis=1, kind="stable")[:, :min(10, cand.size)]
    sums = np.zeros(G, dtype)
    for v in top.T:
        sums = f(sums + v)
    dyn = np.maximum(1, sums.astype(np.int64))
    sel = np.zeros((G, cand.size), bool)
    for g in range(G):
        sel[g, np.argsort(cost[g], kind="stable")[:dyn[g]]] = True
    n_sel = sel.sum(0)
    m = np.where(n_sel > 0, np.argmax(sel, 0), -1)
    multi = n_sel > 1
    m[multi] = np.argmin(cost[:, multi], 0)              # over ALL gts; first minimum
    fg = m >= 0
    matched[cand[fg]] = m[fg]
    iou_t[cand[fg]] = iou[m[fg], np.nonzero(fg)[0]]
    aux.update(cost=cost, iou=iou, dyn=dyn, sums=sums, sel=sel)
    return matched, iou_t, aux


def _iou_rows(rel_gt, dec, dtype):
    """IoU of one gt against C predictions, the gt given relative to each point: rel_gt (C, 4), dec (C, 4) = dx, dy, w, h."""
    f = lambda a: np.asarray(a, dtype)
    hw, hh = f(dec[:, 2] / 2), f(dec[:, 3] / 2)
    tlx, tly = np.maximum(rel_gt[:, 0], f(dec[:, 0] - hw)), np.maximum(rel_gt[:, 1], f(dec[:, 1] - hh))
    brx, bry = np.minimum(rel_gt[:, 2], f(dec[:, 0] + hw)), np.minimum(rel_gt[:, 3], f(dec[:, 1] + hh))
    ai = np.where((tlx < brx) & (tly < bry), f(f(brx - tlx) * f(bry - tly)), 0).astype(dtype)
    ag, ap = f(f(rel_gt[:, 2] - rel_gt[:, 0]) * f(rel_gt[:, 3] - rel_gt[:, 1])), f(dec[:, 2] * dec[:, 3])
    with np.errstate(divide="ignore", invalid="ignore"):
        v = f(ai / f(f(ag + ap) - ai))
    return np.where(v > 0, v, 0).astype(dtype)


def assign(prob, dtype=np.float64, reassoc=False):
    """-> matched (N, P) int64 (-1 = background), iou_t (N, P) float64, aux per image."""
    N, P = prob["cls"].shape[:2]
    matched, iou_t, aux = np.zeros((N, P), np.int64), np.zeros((N, P)), []
    for n in range(N):
        G = int(min(max(prob["num"][n], 0), prob["gt"].shape[1]))
        m, u, a = _image_assign(prob["cls"][n], prob["box_obj"][n], prob["pts"], prob["stride"], prob["gt"][n, :G], prob["K"], dtype, reassoc)
        matched[n], iou_t[n] = m, u
        aux.append(a)
    return matched, iou_t, aux


def cost_tol(c):
    """How far two evaluations of one cost may lie apart: 1e-4 relative below the 1e5 penalty, two float32 spacings (2^-6) above it."""
    c = abs(float(c))
    return 1e-4 * c if c < 1e5 else 2.0 ** -6


def compare(prob, ref, matched_x):
    """(foreground count of the oracle, cap on differing points, [(image, point, excuse)]) for another evaluation of the same problem.
    Excuses -- a: a gt that takes the point on one side only has its cost within cost_tol of its k-th or (k+1)-th smallest cost;
    b: the two smallest costs of the point's column are within cost_tol; c: the top-10 IoU sum of such a gt is within 1e-4 of an integer."""
    matched_o, _, aux = ref
    nfg = int((matched_o >= 0).sum())
    out = []
    for n, p in np.argwhere(matched_x != matched_o):
        a = aux[n]
        excuse = None
        where = np.nonzero(a["cand"] == p)[0]
        if where.size:
            j = int(where[0])
            cost, sel, dyn, sums = a["cost"], a["sel"], a["dyn"], a["sums"]
            theirs = int(matched_x[n, p])
            one_sided = ([theirs] if theirs >= 0 and not sel[theirs, j] else []) + [g for g in np.nonzero(sel[:, j])[0] if g != theirs]
            srt = np.sort(cost, axis=1)
            for g in one_sided:
                kth = [srt[g, dyn[g] - 1]] + ([srt[g, dyn[g]]] if dyn[g] < cost.shape[1] else [])
                if min(abs(float(cost[g, j]) - float(t)) for t in kth) <= cost_tol(cost[g, j]):
                    excuse = "a"
            if excuse is None and cost.shape[0] >= 2:
                two = np.sort(cost[:, j])[:2]
                if float(two[1]) - float(two[0]) <= cost_tol(two[0]):
                    excuse = "b"
            if excuse is None and any(abs(float(sums[g]) - round(float(sums[g]))) <= 1e-4 for g in one_sided):
                excuse = "c"
        out.append((int(n), int(p), excuse))
    return nfg, max(1, int(0.005 * nfg)), out


# ---- losses -----------------------------------------------------------------------------------------------------------------------------
def losses(prob, matched, iou_t, nf, use_l1):
    """float64 autograd: (loss4 = 5 * iou, obj, cls, l1; d_cls (N, P, K); d_box_obj (N, P, 5)) of the sum of the four.  A matched entry
    outside 0 .. Gmax - 1 is background, as in the kernel."""
    K = prob["K"]
    cls = torch.tensor(prob["cls"][..., :K], dtype=torch.float64, requires_grad=True)
    bo = torch.tensor(prob["box_obj"][..., :5], dtype=torch.float64, requires_grad=True)
    pts = torch.tensor(prob["pts"], dtype=torch.float64)
    st = torch.tensor(prob["stride"], dtype=torch.float64)
    gt = torch.tensor(prob["gt"], dtype=torch.float64)
    m = torch.tensor(matched)
    fg = (m >= 0) & (m < gt.shape[1])
    nf = max(float(nf), 1.0)
    n_idx = torch.nonzero(fg)[:, 0]
    g = gt[n_idx, m[fg]]                                   # (F, 5)
    raw = bo[..., :4][fg]
    p, s = pts.expand(fg.shape[0], -1, -1)[fg], st.expand(fg.shape[0], -1)[fg]
    xc, yc = raw[:, 0] * s + p[:, 0], raw[:, 1] * s + p[:, 1]
    w, h = s * torch.exp(raw[:, 2]), s * torch.exp(raw[:, 3])
    x1, y1, x2, y2 = xc - w / 2, yc - h / 2, xc + w / 2, yc + h / 2
    iw = torch.clamp(torch.minimum(x2, g[:, 2]) - torch.maximum(x1, g[:, 0]), min=0)
    ih = torch.clamp(torch.minimum(y2, g[:, 3]) - torch.maximum(y1, g[:, 1]), min=0)
    inter = iw * ih
    union = (x2 - x1) * (y2 - y1) + (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) - inter
    iou = torch.clamp(inter / union, min=0)
    l_iou = 5 * (1 - iou ** 2).sum() / nf
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    l_obj = bce(bo[..., 4], fg.double(), reduction="sum") / nf
    tgt = torch.zeros((int(fg.sum()), K), dtype=torch.float64)
    lab = g[:, 4].long() - 1
    ok = (lab >= 0) & (lab < K)
    tgt[torch.nonzero(ok)[:, 0], lab[ok]] = torch.tensor(iou_t, dtype=torch.float64)[fg][ok]
    l_cls = bce(cls[fg], tgt, reduction="sum") / nf
    if use_l1:
        t = torch.stack([((g[:, 0] + g[:, 2]) / 2 - p[:, 0]) / s, ((g[:, 1] + g[:, 3]) / 2 - p[:, 1]) / s,
                         torch.log((g[:, 2] - g[:, 0]) / s + 1e-8), torch.log((g[:, 3] - g[:, 1]) / s + 1e-8)], 1)
        l_l1 = (raw - t).abs().sum() / nf
    else:
        l_l1 = torch.zeros((), dtype=torch.float64)
    total = l_iou + l_obj + l_cls + l_l1
    total.backward()
    return (np.array([float(v.detach()) for v in (l_iou, l_obj, l_cls, l_l1)]), cls.grad.numpy(), bo.grad.numpy())


# ---- inference --------------------------------------------------------------------------------------------------------------------------
def scores(prob):
    """sqrt(sigmoid(cls) sigmoid(obj)) (N, P, K), float64."""
    K = prob["K"]
    pc, _, _ = _sig(prob["cls"][..., :K].astype(np.float64))
    po, _, _ = _sig(prob["box_obj"][..., 4].astype(np.float64))
    return np.sqrt(pc * po[..., None])


def boxes_xyxy(prob):
    d = decode(prob["box_obj"][..., :4], prob["pts"].astype(np.float64), prob["stride"])
    return np.stack([d[..., 0] - d[..., 2] / 2, d[..., 1] - d[..., 3] / 2, d[..., 0] + d[..., 2] / 2, d[..., 1] + d[..., 3] / 2], -1)


def select(prob, thr, k):
    """Per image and level the items (point - level start) * K + class with score > thr, best k: score descending, index ascending."""
    sc = scores(prob)
    out = []
    for n in range(sc.shape[0]):
        lv = []
        for l in range(len(prob["lvl_start"]) - 1):
            s = sc[n, prob["lvl_start"][l]:prob["lvl_start"][l + 1]].reshape(-1)
            idx = np.nonzero(s > thr)[0]
            idx = idx[np.argsort(-s[idx], kind="stable")][:k]
            lv.append((idx, s[idx]))
        out.append(lv)
    return out


# ---- problems ---------------------------------------------------------------------------------------------------------------------------
def _base(N, H, W, K, Gmax, rng):
    sizes = level_sizes(H, W)
    pts, lvl_start, stride = points(sizes)
    P = pts.shape[0]
    return dict(N=N, H=H, W=W, K=K, sizes=sizes, pts=pts, lvl_start=lvl_start, stride=stride, strides=list(STRIDES),
                gt=np.zeros((N, Gmax, 5), np.float32), num=np.zeros(N, np.int32),
                cls=rng.normal(-2.0, 1.5, (N, P, ld_of(K))), box_obj=rng.normal(0, 0.6, (N, P, 8)))


def _finish(prob, rng, near=0.5):
    """Predictions: a share `near` of the points regress towards a random gt of their image (noisy), the others stay random; pad slots
    hold values that would show if they were read; everything rounded to bf16; gt rows >= num_gt hold NaN / 1e30."""
    N, P = prob["cls"].shape[:2]
    K, pts, st = prob["K"], prob["pts"].astype(np.float64), prob["stride"]
    for n in range(N):
        G = int(prob["num"][n])
        prob["gt"][n, G:] = np.where(rng.random((prob["gt"].shape[1] - G, 5)) < 0.5, np.nan, 1e30)
        if G == 0:
            continue
        g = prob["gt"][n, rng.integers(0, G, P), :4].astype(np.float64)
        sel = rng.random(P) < near
        w, h = np.maximum(g[:, 2] - g[:, 0], 1.0), np.maximum(g[:, 3] - g[:, 1], 1.0)
        tgt = np.stack([((g[:, 0] + g[:, 2]) / 2 - pts[:, 0]) / st, ((g[:, 1] + g[:, 3]) / 2 - pts[:, 1]) / st, np.log(w / st), np.log(h / st)], 1)
        tgt += rng.normal(0, 0.15, tgt.shape)
        prob["box_obj"][n, sel, :4] = np.clip(tgt[sel], -8, 8)
    prob["cls"][..., K:] = 3.0
    prob["box_obj"][..., 5:] = 3.0
    prob["cls"], prob["box_obj"] = bf16(prob["cls"]).astype(np.float64), bf16(prob["box_obj"]).astype(np.float64)
    return prob


def _rand_gts(rng, G, H, W, K, lo=6.0, hi=None):
    hi = hi or max(min(H, W) * 0.6, lo + 1)
    cx, cy = rng.uniform(0, W, G), rng.uniform(0, H, G)
    w, h = lo * (hi / lo) ** rng.random(G), lo * (hi / lo) ** rng.random(G)
    b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    out = np.zeros((G, 5), np.float32)
    out[:, :4] = np.round(b * 4) / 4                       # quarter pixels: the candidate tests are exact in float32
    out[:, 4] = rng.integers(1, K + 1, G)
    return out


@functools.lru_cache(maxsize=None)
def problem(shape):
    """The shared assignment / loss problem of one SHAPES entry.  Every batch with N > 1 holds an image without gts (image 1)."""
    N, H, W, K, Gmax = shape
    rng = np.random.default_rng(SEEDS[shape])
    prob = _base(N, H, W, K, Gmax, rng)
    for n in range(N):
        G = 0 if (N > 1 and n == 1) else (Gmax if n == 0 else int(rng.integers(1, Gmax + 1)))
        prob["num"][n] = G
        prob["gt"][n, :G] = _rand_gts(rng, G, H, W, K)
    if Gmax >= 7:                                         # image 0: a 4 px gt between the points of every level (centre test only) ...
        prob["gt"][0, 0] = [18.0, 18.0, 22.0, 22.0, 1]
        a, b, side = round(W * 0.1), round(H * 0.1), round(min(H, W) * 0.5)
        prob["gt"][0, 1] = [a, b, a + side, b + side, K]  # ... and a large one
    return _finish(prob, rng)


@functools.lru_cache(maxsize=None)
def edge_problem():
    """96 x 160, K = 3: image 0 holds a zero-area gt, a gt wholly outside the image, two identical gts and a gt covering the image;
    image 1's only gt lies outside the image (no candidate); image 2 is ordinary."""
    N, H, W, K, Gmax = 3, 96, 160, 3, 7
    rng = np.random.default_rng(11)
    prob = _base(N, H, W, K, Gmax, rng)
    prob["num"][:] = [7, 1, 4]
    prob["gt"][0, :7] = [[40, 20, 40, 70, 1], [W + 100, H + 100, W + 180, H + 150, 2], [30.25, 12.5, 90.75, 60.5, 3],
                         [30.25, 12.5, 90.75, 60.5, 3], [0, 0, W, H, 1], [100, 40, 140, 80, 2], [8, 50, 52, 90, 1]]
    prob["gt"][1, 0] = [W + 100, H + 100, W + 180, H + 150, 1]
    prob["gt"][2, :4] = _rand_gts(rng, 4, H, W, K)
    return _finish(prob, rng)


@functools.lru_cache(maxsize=None)
def empty_problem():
    N, H, W, K, Gmax = 2, 96, 160, 3, 4
    rng = np.random.default_rng(12)
    return _finish(_base(N, H, W, K, Gmax, rng), rng)


@functools.lru_cache(maxsize=None)
def extremes_problem():
    """Logits of +-20 and +-40, raw w / h of +-8 spread over the points of the 96 x 160 problem."""
    shape = SHAPES[1]
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in problem(shape).items()}
    P, K = p["cls"].shape[1], p["K"]
    vals = np.array([20.0, -20.0, 40.0, -40.0])
    idx = np.arange(P)
    p["cls"][:, :, :K] = vals[(idx[None, :, None] + np.arange(K)[None, None, :]) % 4]
    p["box_obj"][:, :, 4] = vals[(idx // 4) % 4][None, :]
    p["box_obj"][:, :, 2] = np.where(idx % 3 == 0, 8.0, np.where(idx % 3 == 1, -8.0, p["box_obj"][:, :, 2]))
    p["box_obj"][:, :, 3] = np.where(idx % 5 == 0, -8.0, np.where(idx % 5 == 1, 8.0, p["box_obj"][:, :, 3]))
    return p


@functools.lru_cache(maxsize=None)
def reference(name):
    """assign() of a shared problem, computed once: name = a SHAPES entry, "edge" or "empty"."""
    prob = edge_problem() if name == "edge" else empty_problem() if name == "empty" else problem(name)
    return assign(prob)


@functools.lru_cache(maxsize=None)
def inference_problem(B, H, W, K, seed=21):
    rng = np.random.default_rng(seed + B + K)
    prob = _base(B, H, W, K, 1, rng)
    prob["cls"] = rng.normal(-5.0, 2.0, prob["cls"].shape)
    prob["box_obj"][..., 4] = rng.normal(0.0, 2.0, prob["box_obj"].shape[:2])
    prob["box_obj"][..., 2:4] = rng.normal(1.0, 0.5, prob["box_obj"].shape[:2] + (2,))
    return _finish(prob, rng)


# ---- problems past the loss kernel's grid cap, on the kinks of the IoU loss and on exact cost ties (tests/test_yolox_edges_gpu.py) -------
BIG_SHAPE = (3, 640, 640, 365, 40)


@functools.lru_cache(maxsize=None)
def big_loss_problem():
    """(prob, matched, iou_t) at BIG_SHAPE: 3 x 8400 rows of 46 vectors.  The assignment is drawn, not computed: about 2 % of the points
    are foreground with a valid gt index of their image and an iou_t in (0, 1) that float32 holds exactly."""
    N, H, W, K, Gmax = BIG_SHAPE
    rng = np.random.default_rng(31)
    prob = _base(N, H, W, K, Gmax, rng)
    for n, G in enumerate((Gmax, 17, 1)):
        prob["num"][n] = G
        prob["gt"][n, :G] = _rand_gts(rng, G, H, W, K)
    prob = _finish(prob, rng)
    P = prob["pts"].shape[0]
    fg = rng.random((N, P)) < 0.02
    matched = np.where(fg, rng.integers(0, prob["num"][:, None], (N, P)), -1).astype(np.int64)
    iou_t = np.where(fg, rng.uniform(0.02, 0.98, (N, P)).astype(np.float32), np.float32(0)).astype(np.float64)
    return prob, matched, iou_t


KINK_CASES = ("equal", "edge_x1", "edge_y1", "edge_x2", "edge_y2", "two_edges", "disjoint", "inside", "label_0", "label_K+1", "zero_area")


@functools.lru_cache(maxsize=None)
def kink_problem():
    """One image, one level of 12 x 12 points at stride 8, K = 3, one gt per foreground point.  Foreground rows have raw w = h = 0 (the
    decoded box is 8 x 8) and raw dx, dy in eighths; gts lie on quarter pixels: every coordinate is exact in float32 and float64, in the
    image frame and relative to the point.  With (X1, Y1, X2, Y2) the decoded prediction, prob["cases"] names the point of
      equal       gt = prediction: all four min / max tie, iou = 1;
      edge_x1, edge_y1, edge_x2, edge_y2   gt shares exactly that edge with the prediction, the other three differ, the overlap is positive;
      two_edges   gt shares x1 and y2;
      disjoint    gt and prediction do not meet: q = 0, iou loss 1, no box gradient from the IoU term;
      inside      the prediction lies strictly inside its gt;
      label_0, label_K+1   an overlapping gt whose label matches no class column: every class column is a background term;
      zero_area   a gt with x1 = x2 and y1 = y2 inside the prediction: the L1 target is log(0 + 1e-8).
    prob["bg_gmax"] is a background row whose matched entry is Gmax; every other row has matched = -1.  prob["matched"], prob["iou_t"]
    (1, P) go with it."""
    K, S, side = 3, 8, 12
    rng = np.random.default_rng(41)
    sizes = [(side, side)]
    pts, lvl_start, stride = points(sizes, (S,))
    P, G = side * side, len(KINK_CASES)
    cls, box_obj = rng.normal(-2.0, 1.5, (1, P, 8)), rng.normal(0, 0.6, (1, P, 8))
    cls[..., K:], box_obj[..., 5:] = 3.0, 3.0
    # name -> (raw dx, raw dy, what is added to (X1, Y1, X2, Y2), label)
    spec = {"equal": (0.25, -0.125, (0, 0, 0, 0), 1), "edge_x1": (0, 0.125, (0, -1.25, 2.5, -1.75), 2),
            "edge_y1": (-0.125, 0, (1.5, 0, 3.25, 2), 3), "edge_x2": (0.375, 0.25, (-2.25, 0.75, 0, 1.5), 1),
            "edge_y2": (0, -0.25, (-1.5, -3, -2.75, 0), 2), "two_edges": (0.125, 0.125, (0, -2.5, 1.25, 0), 3),
            "disjoint": (0, 0, (11.25, 9.5, 13.25, 9.75), 1), "inside": (-0.25, 0.125, (-2.5, -1.25, 3.75, 0.5), 2),
            "label_0": (0.125, 0, (-1.25, 1.5, 2.25, 2.75), 0), "label_K+1": (0, -0.125, (1.75, -2.25, 3.5, 1.25), K + 1)}
    gt = np.zeros((1, G, 5), np.float32)
    matched, iou_t, cases = np.full((1, P), -1, np.int64), np.zeros((1, P)), {}
    for i, name in enumerate(KINK_CASES):
        p = (1 + 3 * (i // 5)) * side + 1 + 2 * (i % 5)
        dx, dy, add, lab = spec.get(name, (0, 0.125, None, 2))
        cx, cy = pts[p, 0] + S * dx, pts[p, 1] + S * dy
        box = np.array([cx - 4, cy - 4, cx + 4, cy + 4]) + add if add is not None else np.array([cx + 1.25, cy - 0.75, cx + 1.25, cy - 0.75])
        gt[0, i] = list(box) + [lab]
        box_obj[0, p, :4] = [dx, dy, 0, 0]
        matched[0, p], iou_t[0, p], cases[name] = i, (i + 1) / 16, p
    matched[0, 0] = G
    return dict(N=1, H=side * S, W=side * S, K=K, sizes=sizes, pts=pts, lvl_start=lvl_start, stride=stride, strides=[S], gt=gt,
                num=np.array([G], np.int32), cls=bf16(cls).astype(np.float64), box_obj=bf16(box_obj).astype(np.float64), matched=matched,
                iou_t=iou_t, cases=cases, bg_gmax=0)


@functools.lru_cache(maxsize=None)
def tie_problem():
    """Two 256 x 256 images, K = 3, P = 1344: the workgroup of a gt walks the points in two chunks, [0, 1024) = the stride-8 level and
    [1024, 1344).  Every class logit is -2, every obj logit 0.5, every raw box 0: the prediction of a point is the stride x stride box
    around it, IoUs are quotients of small integers, and the cost of a (gt, point) pair depends on that IoU and on the two inside tests
    alone -- equal IoUs are equal costs, bit for bit, in float32 and float64.  Image 0:
      gt 0  128 x 128 around the stride-8 point (176, 176): 225 + 49 + 16 points inside, IoU 1/256, 1/64 or 1/16; the 16 stride-32 points
            tie at the top-10 cut and at the cost cut (k = 1);
      gt 1  16 x 8 around (32, 32): the stride-8 point 132 (its 8 x 8 box inside the gt) and the stride-16 point 1058 (its box around the
            gt) both have IoU 1/2 and no penalty: with k = 1 the k-th and (k+1)-th cheapest candidates tie across the two chunks;
      gt 2  a zero-area gt: every IoU is 0, so its top-10 IoUs are all equal and every candidate of the image costs the same.
    Image 1: a gt outside the image with 8 candidates (fewer than the 10 the dynamic k reads).  Rows >= num_gt hold NaN."""
    N, H, W, K, Gmax = 2, 256, 256, 3, 4
    sizes = level_sizes(H, W)
    pts, lvl_start, stride = points(sizes)
    P = pts.shape[0]
    cls, box_obj = np.full((N, P, 8), -2.0), np.zeros((N, P, 8))
    cls[..., K:], box_obj[..., 4], box_obj[..., 5:] = 3.0, 0.5, 3.0
    gt = np.full((N, Gmax, 5), np.nan, np.float32)
    gt[0, :3] = [[112, 112, 240, 240, 1], [24, 28, 40, 36, 2], [40.5, 200.5, 40.5, 200.5, 3]]
    gt[1, 0] = [-30, -30, -14, -14, 1]
    return dict(N=N, H=H, W=W, K=K, sizes=sizes, pts=pts, lvl_start=lvl_start, stride=stride, strides=list(STRIDES), gt=gt,
                num=np.array([3, 1], np.int32), cls=cls, box_obj=box_obj)
