"""Forward skip of the box tower (bd_fwd_live_maps, bd_conv_desc.fwd_map / fwd_clean, MODEL.SPARSE_BOX_FWD): the tower's forward
convolutions compute only the 4 x 16 patches within reach of a foreground anchor and leave +0 everywhere else.  The dense route is the
oracle and there is no tolerance: flags and lists equal a numpy dilation, live patches equal the dense launch's bits, dead patches are +0,
and a training step gives the same losses, gradients and dL/dP.

Kernel level on a small pyramid, 2 images x levels (13, 21), (7, 11), (4, 6), (2, 3), (1, 2): ragged widths, a height below the patch
height, level / image boundaries adjacent in memory.  Step level: RetinaNet-R50 at 2 x 128 x 160."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LEVELS = [(13, 21), (7, 11), (4, 6), (2, 3), (1, 2)]
N, C, A, DEPTHS = 2, 256, 3, 4
NAN16 = 0x7FC1
HDR = 8


def _geo():
    from basedet_amd import ops
    g = ops.Geom(N, [h for h, _ in LEVELS], [w for _, w in LEVELS])
    return g, ops.conv_desc(g, g, C, C, 3, 3, 1, 1)


def _patches():
    """(image, level, patch row, patch column) of every 4 x 16 patch, in the library's order."""
    return [(n, l, by, bx) for n in range(N) for l, (H, W) in enumerate(LEVELS) for by in range(-(-H // 4)) for bx in range(-(-W // 16))]


def _labels(fg):
    """int32 (N, pixels * A) labels from per-(image, level) boolean foreground masks: one anchor of a foreground pixel is positive (which
    one varies with the pixel), the others are background (0) or ignored (-1)."""
    g, _ = _geo()
    lab = np.zeros((N, g.pix_per_img, A), np.int32)
    lab[:, ::3, 1] = -1
    for n in range(N):
        for l, (H, W) in enumerate(LEVELS):
            ys, xs = np.nonzero(fg[n][l])
            for y, x in zip(ys, xs):
                lab[n, g.off[l] + y * W + x, (y + x) % A] = 1 + (y * 7 + x) % 80
    return torch.from_numpy(lab.reshape(N, -1)).cuda()


def _dilate(m):
    H, W = m.shape
    p = np.zeros((H + 2, W + 2), bool)
    p[1:-1, 1:-1] = m
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def _expected(fg):
    """flags[k - 1] (bool per patch) and the pixel sets after k = 1 .. DEPTHS dilations inside each image and level."""
    cur = [[fg[n][l].copy() for l in range(len(LEVELS))] for n in range(N)]
    flags, pix = [], []
    for _ in range(DEPTHS):
        cur = [[_dilate(m) for m in img] for img in cur]
        flags.append(np.array([cur[n][l][4 * by:4 * by + 4, 16 * bx:16 * bx + 16].any() for n, l, by, bx in _patches()]))
        pix.append(cur)
    return flags, pix


def _empty():
    return [[np.zeros(hw, bool) for hw in LEVELS] for _ in range(N)]


def _fg_edges():
    """Image 0: all four corners, one pixel on each border and the last pixel of every level; image 1: isolated interior pixels, the first and
    the last pixel of the image."""
    fg = _empty()
    H, W = LEVELS[0]
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 9), (H - 1, 5), (6, 0), (4, W - 1)):
        fg[0][0][y, x] = True
    for l, (h, w) in enumerate(LEVELS):
        fg[0][l][h - 1, w - 1] = True
    fg[1][0][5, 10] = fg[1][0][8, 16] = fg[1][1][3, 5] = True
    fg[1][0][0, 0] = fg[1][4][0, 1] = True
    return fg


def _fg_sparse():
    """A few isolated pixels: at depth 1 most patches are dead."""
    fg = _empty()
    fg[0][0][1, 2] = fg[1][0][11, 19] = fg[1][1][0, 10] = True
    return fg


def _fg_moved():
    fg = _empty()
    fg[0][0][12, 20] = fg[0][2][0, 0] = fg[1][3][1, 1] = True
    return fg


def _fg_full_and_empty():
    """Image 0 all background, image 1 every pixel foreground."""
    fg = _empty()
    fg[1] = [np.ones(hw, bool) for hw in LEVELS]
    return fg


FG = {"edges": _fg_edges, "sparse": _fg_sparse, "full_and_empty": _fg_full_and_empty, "background": _empty}


def _new_maps():
    from basedet_amd import ops
    _, d = _geo()
    ints = (ops.fwd_live_map_bytes(d) + 3) // 4
    assert ints == HDR + 3 * len(_patches())
    return [torch.full((ints,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(DEPTHS)]      # (garbage: reset clears what matters)


def _read(m):
    """(flags, current list, previous list) of a map."""
    P4 = len(_patches())
    v = m.cpu().numpy()
    cur = v[0] & 1
    lists = [v[HDR + P4 * (1 + k): HDR + P4 * (1 + k) + max(int(v[2 + k]), 0)] for k in range(2)]
    return v[HDR:HDR + P4], lists[cur], lists[cur ^ 1]


@pytest.mark.parametrize("name", list(FG))
def test_maps_equal_numpy_dilation(name):
    from basedet_amd import ops
    _, d = _geo()
    fg = FG[name]()
    want, _ = _expected(fg)
    maps = _new_maps()
    ops.fwd_live_maps(d, _labels(fg), A, maps, reset=True)
    torch.cuda.synchronize()
    first = []
    for k in range(DEPTHS):
        live, cur, prev = _read(maps[k])
        assert np.array_equal(live != 0, want[k]), (name, k + 1)
        assert np.array_equal(cur, np.nonzero(want[k])[0]), (name, k + 1)
        assert len(prev) == 0
        first.append(cur.copy())
    if name == "edges":
        assert not want[0].all() and want[0].any()           # the case can tell "equal" from "superset"
    # a second call without reset writes the other list and keeps the first as the previous one
    fg2 = _fg_moved()
    want2, _ = _expected(fg2)
    ops.fwd_live_maps(d, _labels(fg2), A, maps, reset=False)
    torch.cuda.synchronize()
    for k in range(DEPTHS):
        live, cur, prev = _read(maps[k])
        assert np.array_equal(live != 0, want2[k]) and np.array_equal(cur, np.nonzero(want2[k])[0]) and np.array_equal(prev, first[k])
        assert int(maps[0][1]) == 0                          # the finished-workgroup counter is back at 0


class _Conv:
    """Operands of the sparse-against-dense comparison (made once, never modified)."""

    def __init__(self):
        from basedet_amd import ops
        self.ops = ops
        self.geo, self.d = _geo()
        self.P = N * self.geo.pix_per_img
        gen = torch.Generator(device="cuda").manual_seed(5)
        self.x = torch.randn((self.P, C), device="cuda", generator=gen).to(torch.bfloat16)
        self.w = (torch.randn((C, 9, C), device="cuda", generator=gen) * 0.05).to(torch.bfloat16)
        self.b = torch.randn((C,), device="cuda", generator=gen)
        self.dense = torch.empty((self.P, C), dtype=torch.bfloat16, device="cuda")
        ops.conv2d_fwd(self.d, self.x, self.w, self.b, self.dense, flags=ops.EPI_RELU)
        torch.cuda.synchronize()
        assert bool((self.dense.view(torch.int16) != 0).view(self.P, C).any(1).all())      # no dense pixel is all +0: a dead patch shows

    def patch_mask(self, flags):
        """bool per pixel (P,): inside a patch whose flag is set."""
        m = np.zeros((N, self.geo.pix_per_img), bool)
        for f, (n, l, by, bx) in zip(flags, _patches()):
            if f:
                H, W = LEVELS[l]
                t = np.zeros((H, W), bool)
                t[4 * by:4 * by + 4, 16 * bx:16 * bx + 16] = True
                m[n, self.geo.off[l]:self.geo.off[l] + H * W] |= t.reshape(-1)
        return torch.from_numpy(m.reshape(-1)).cuda()

    def check(self, y, flags, what):
        live = self.patch_mask(flags)
        yb, db = y.view(torch.int16), self.dense.view(torch.int16)
        assert torch.equal(yb[live], db[live]), (what, "live patches differ from the dense launch")
        assert int((yb[~live] != 0).sum()) == 0, (what, "dead patches are not +0")


_CONV = []


@pytest.fixture(scope="module")
def conv():
    if not _CONV:
        _CONV.append(_Conv())
    return _CONV[0]


@pytest.mark.parametrize("name", list(FG))
def test_sparse_forward_equals_dense(conv, name):
    """Every depth's map on a NaN-filled output without the promise; with the promise only the previous list's patches may be touched, so
    the same call on a buffer that is +0 outside that list gives the same picture; then a list that shrank and moved, with the promise."""
    ops, d = conv.ops, conv.d
    fg = FG[name]()
    want, _ = _expected(fg)
    maps = _new_maps()
    ops.fwd_live_maps(d, _labels(fg), A, maps, reset=True)
    ys = []
    for k in range(DEPTHS):
        y = torch.full((conv.P, C), NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        ops.conv2d_fwd(ops.fwd_map_desc(d, maps[k]), conv.x, conv.w, conv.b, y, flags=ops.EPI_RELU)
        from basedet_amd import _lib
        assert _lib.load().bd_conv_last_kernel().decode() == "conv3x3_pp_kernel"
        torch.cuda.synchronize()
        conv.check(y, want[k], (name, "no promise", k + 1))
        ys.append(y)
    # the same batch again (the lists repeat), promise given: nothing dead may be rewritten -- NaN planted in a patch that was dead before
    # and is dead now must survive (the promise is what allows leaving it), everything else as before
    ops.fwd_live_maps(d, _labels(fg), A, maps, reset=False)
    for k in range(DEPTHS):
        dead = np.nonzero(~want[k])[0]
        y = ys[k]
        if len(dead):
            n, l, by, bx = _patches()[dead[0]]
            planted = (n * conv.geo.pix_per_img + conv.geo.off[l] + 4 * by * LEVELS[l][1] + 16 * bx)
            y.view(torch.int16)[planted] = NAN16
        ops.conv2d_fwd(ops.fwd_map_desc(d, maps[k], clean=True), conv.x, conv.w, conv.b, y, flags=ops.EPI_RELU)
        torch.cuda.synchronize()
        if len(dead):
            assert bool((y.view(torch.int16)[planted] == NAN16).all()), (name, "the promise was not used", k + 1)
            y.view(torch.int16)[planted] = 0
        conv.check(y, want[k], (name, "promise, same list", k + 1))
    # a list that shrank and moved, promise given: the patches that were live and are dead now are cleared
    fg2 = _fg_moved()
    want2, _ = _expected(fg2)
    ops.fwd_live_maps(d, _labels(fg2), A, maps, reset=False)
    for k in range(DEPTHS):
        ops.conv2d_fwd(ops.fwd_map_desc(d, maps[k], clean=True), conv.x, conv.w, conv.b, ys[k], flags=ops.EPI_RELU)
        torch.cuda.synchronize()
        conv.check(ys[k], want2[k], (name, "promise, moved list", k + 1))


def test_refusals(conv):
    """A forward call with a map that the sparse instance cannot honour is an error, not a dense launch."""
    from basedet_amd._lib import BasedetHipError
    ops, d = conv.ops, conv.d
    maps = _new_maps()
    y = torch.zeros((conv.P, C), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(BasedetHipError):          # residual operand
        ops.conv2d_fwd(ops.fwd_map_desc(d, maps[0]), conv.x, conv.w, conv.b, y, add=conv.dense, flags=ops.EPI_ADD_BEFORE)
    with pytest.raises(BasedetHipError):          # map too small
        ops.conv2d_fwd(ops.fwd_map_desc(d, maps[0][:16]), conv.x, conv.w, conv.b, y, flags=ops.EPI_RELU)
    d40 = ops.conv_desc(conv.geo, conv.geo, C, 40, 3, 3, 1, 1)
    with pytest.raises(BasedetHipError):          # 40 output channels: not the 256-channel tile
        ops.conv2d_fwd(ops.fwd_map_desc(d40, maps[0]), conv.x, conv.w[:40].contiguous(), conv.b[:40].contiguous(),
                       torch.zeros((conv.P, 40), dtype=torch.bfloat16, device="cuda"), flags=0)
    with pytest.raises(BasedetHipError):          # labels of another size
        ops.fwd_live_maps(d, torch.zeros((N, 7), dtype=torch.int32, device="cuda"), A, maps, reset=True)
    torch.cuda.synchronize()
    assert int((y.view(torch.int16) != 0).sum()) == 0          # nothing was launched


# ---- one training step -------------------------------------------------------------------------------------------------------------------
SIZE = (128, 160)


def _batch(kind):
    rng = np.random.default_rng({"boxes": 1, "background": 2, "many": 3}[kind])
    G = {"boxes": 5, "background": 4, "many": 100}[kind]
    num = {"boxes": (5, 3), "background": (0, 0), "many": (100, 100)}[kind]
    gt = np.zeros((2, G, 5), np.float32)
    for n in range(2):
        for k in range(num[n]):
            w, h = rng.uniform(8, 90), rng.uniform(8, 90)
            x1, y1 = rng.uniform(0, SIZE[1] - w), rng.uniform(0, SIZE[0] - h)
            gt[n, k] = (x1, y1, x1 + w, y1 + h, rng.integers(1, 81))
    info = np.array([[*SIZE, 612., 612., num[0]], [*SIZE, 500., 375., num[1]]], np.float32)
    data = (rng.random((2, 3, *SIZE)) * 255).astype(np.float32)
    return {"data": data, "gt_boxes": gt, "im_info": info}


_MODELS = []


@pytest.fixture(scope="module")
def models():
    """RetinaNet-R50 with MODEL.SPARSE_BOX_FWD = 1 and = 0 on the same parameters (made once; no optimizer step: the weights stay equal)."""
    if not _MODELS:
        from basedet_amd.models import RetinaNet
        from tests.test_model_gpu import _setup
        out = []
        for on in (1, 0):
            cfg, params, _ = _setup("resnet50", 2, SIZE)
            cfg.MODEL.SPARSE_BOX_FWD = on
            out.append(RetinaNet(cfg, params=params))
        _MODELS.append(tuple(out))
    return _MODELS[0]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("kind", ["boxes", "background", "many", "boxes"], ids=["boxes", "background", "many", "boxes_again"])
def test_retinanet_step_same_bits(models, kind):
    """Losses, every reference gradient and dL/dP of a step with the skip equal those without, bit for bit; debug_activations() then shows
    the dense box tower.  The cases run on the same two models one after the other: from the second on the promise is given."""
    m_on, m_off = models
    assert m_on.sparse_box_fwd and not m_off.sparse_box_fwd
    batch = _batch(kind)
    res = []
    for m in (m_on, m_off):
        losses = m({k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()})
        skipped = m._cur.fwd_skipped
        m.backward()
        torch.cuda.synchronize()
        res.append((losses, m.reference_grads(), m._cur.g_P.clone(), skipped))
    (l1, g1, p1, s1), (l0, g0, p0, s0) = res
    assert s1 and not s0                                    # the skip was really on / off
    for k in l0:
        assert torch.equal(_bits(l1[k].float().reshape(1)), _bits(l0[k].float().reshape(1))), (kind, k, float(l1[k]), float(l0[k]))
    assert g1.keys() == g0.keys()
    for k in g0:
        assert torch.equal(_bits(g1[k].float()), _bits(g0[k].float())), (kind, k)
        assert bool(torch.isfinite(g1[k]).all()), (kind, k)
    assert torch.equal(_bits(p1), _bits(p0)), (kind, "g_P")
    if kind == "boxes":
        lab = m_on._cur.labels
        assert 0 < int((lab > 0).sum()) < lab.numel() // 4          # a sparse foreground: the skip has something to skip
    a1, a0 = m_on.debug_activations(), m_off.debug_activations()
    assert not m_on._cur.fwd_skipped and m_on._cur.fwd_epoch is None          # the promise is withdrawn
    names = [k for k in a0 if k.startswith("box") or k.startswith("offs_")]
    assert len(names) == 5 * 5
    for k in names:
        assert torch.equal(_bits(a1[k]), _bits(a0[k])), (kind, k)


def test_promise_is_given_on_consecutive_steps(models):
    """Two steps without debug_activations() in between: the second carries the promise (the arena's epoch stood), and gives the dense bits."""
    m_on, m_off = models
    for kind in ("many", "boxes"):
        batch = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in _batch(kind).items()}
        for m in (m_on, m_off):
            m(batch)
            m.backward()
    torch.cuda.synchronize()
    pl = m_on._cur
    assert pl.fwd_skipped and pl.fwd_epoch == m_on.plan_arena.epoch
    assert any(key[2] for c in m_on.box_tower for key in c._fwd_map_cache)          # a descriptor with fwd_clean was used
    g1, g0 = m_on.reference_grads(), m_off.reference_grads()
    for k in g0:
        assert torch.equal(_bits(g1[k].float()), _bits(g0[k].float())), k
    assert torch.equal(_bits(pl.g_P), _bits(m_off._cur.g_P))


def test_freeanchor_and_fp8_keep_the_skip_off():
    from basedet_amd.configs import FreeAnchorConfig, RetinaNetConfig
    from basedet_amd.models import FreeAnchor, RetinaNet, params as P
    cfg = FreeAnchorConfig()
    cfg.MODEL.BATCHSIZE = 2
    assert cfg.MODEL.get("SPARSE_BOX_FWD", True)
    fa = FreeAnchor(cfg, params=P.init_retinanet_params(cfg, seed=0))
    assert not fa.sparse_box_fwd
    del fa
    cfg = RetinaNetConfig()
    cfg.MODEL.BATCHSIZE = 2
    cfg.MODEL.WEIGHT_DTYPE = "fp8_e4m3"
    m8 = RetinaNet(cfg, params=P.init_retinanet_params(cfg, seed=0))
    assert not m8.sparse_box_fwd
    del m8
    cfg = RetinaNetConfig()
    cfg.MODEL.BATCHSIZE = 2
    cfg.MODEL.SPARSE_BOX_BWD = 0
    mb = RetinaNet(cfg, params=P.init_retinanet_params(cfg, seed=0))
    assert not mb.sparse_box_fwd
    del mb
    torch.cuda.empty_cache()
