"""Gradient skip (bd_conv_desc.gskip, MODEL.SPARSE_BOX_BWD): the box branch's data and weight gradients computed only where a nonzero
gradient reaches must give the SAME BITS as the dense launches.

Kernel level, at the head descriptor (16 images, the five 800 x 1344 pyramid levels, 256 -> 256 and 256 -> 40 channels): sparse g masks
(single pixels at level corners, patches across level and image boundaries, all zero, all live, random), data gradients compared as int16
with dx pre-filled with a NaN pattern (an unwritten dead patch shows), in-place accumulation left untouched where dead, weight and bias
gradients compared as int32, and a too-small or missing scratch refused.  Step level: RetinaNet-R50 with the hint on and off gives the
same gradient arena bit for bit and the same losses (bench batch, batch 2, no gt, 100 gt per image, FreeAnchor), and two hinted runs the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SIZE = (800, 1344)
LEVELS = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
NAN16 = 0x7FC1


def _pyr(N):
    from basedet_amd import ops
    return ops.Geom(N, [h for h, _ in LEVELS], [w for _, w in LEVELS])


def _live_pixels(kind, g, rng):
    """bool [N, pixels per image]: where g may be nonzero."""
    N, ppi = g.N, g.pix_per_img
    m = np.zeros((N, ppi), bool)
    if kind == "full":
        m[:] = True
    elif kind == "corners":                         # single pixels at the corners of every level, a few images
        for n in (0, 7, 15):
            for (H, W), o in zip(LEVELS, g.off):
                for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
                    m[n, o + y * W + x] = True
    elif kind == "boundary":                        # blocks across patch, level and image boundaries
        for n in (0, 1, 8):
            for (H, W), o in zip(LEVELS, g.off):
                v = m[n, o:o + H * W].reshape(H, W)
                v[3:5, 15:17] = True                 # 4 x 16 patch corner (pp) and an 8 x 8 patch edge (ring)
                v[H - 2:, W - 3:] = True             # bottom-right of the level: next pixels belong to the next level / image
                v[:2, :2] = True
                v[H // 2, :] = True                  # one full row
    elif kind == "random":                          # ~1 % of the pixels, 3 x 3 blobs
        for n in range(N):
            for (H, W), o in zip(LEVELS, g.off):
                v = m[n, o:o + H * W].reshape(H, W)
                k = max(1, H * W // 900)
                ys, xs = rng.integers(0, H, k), rng.integers(0, W, k)
                for y, x in zip(ys, xs):
                    v[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = True
    else:
        assert kind == "zero"
    return torch.from_numpy(m)


def _operands(C, kind, seed, N=16):
    rng = np.random.default_rng(seed)
    g = _pyr(N)
    live = _live_pixels(kind, g, rng).cuda()
    t = torch.randn((N, g.pix_per_img, C), device="cuda").to(torch.bfloat16)
    t = torch.where(live[:, :, None], t, torch.zeros((), dtype=torch.bfloat16, device="cuda"))
    return g, t.reshape(N * g.pix_per_img, C).contiguous()


def _descs(ops, geo, cin, cout):
    d = ops.conv_desc(geo, geo, cin, cout, 3, 3, 1, 1)
    nb = ops.conv2d_dgrad_gskip_bytes(d)
    assert nb > 0
    scratch = torch.empty((nb + 3) // 4, dtype=torch.int32, device="cuda")
    return d, ops.gskip_desc(d, scratch), scratch


KINDS = ["corners", "boundary", "zero", "full", "random"]


@pytest.mark.parametrize("cout", [256, 40])
@pytest.mark.parametrize("kind", KINDS)
def test_dgrad_bits(kind, cout):
    from basedet_amd import ops
    geo, g = _operands(cout, kind, seed=1)
    d, hd, _ = _descs(ops, geo, 256, cout)
    P = geo.N * geo.pix_per_img
    w = (torch.randn((256, 9, cout), device="cuda") * 0.05).to(torch.bfloat16)
    act = torch.randn((P, 256), device="cuda").to(torch.bfloat16)          # ReLU gate operand (> 0 keeps)
    base = torch.randn((P, 256), device="cuda").to(torch.bfloat16)
    # overwrite and gated overwrite: dead patches must be written (+0) -- a NaN pattern shows any that are not
    for flags, mask in ((0, None), (ops.EPI_MASK, act)):
        out = []
        for desc in (d, hd):
            dx = torch.full((P, 256), NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
            ops.conv2d_dgrad(desc, g, w, dx, mask=mask, flags=flags)
            out.append(dx)
        torch.cuda.synchronize()
        assert torch.equal(out[0].view(torch.int16), out[1].view(torch.int16)), (kind, cout, flags)
    # accumulate in place (the box tower's first conv into g_P): dead patches keep what dx holds
    out = []
    for desc in (d, hd):
        dx = base.clone()
        ops.conv2d_dgrad(desc, g, w, dx, add=dx, flags=ops.EPI_ADD_BEFORE)
        out.append(dx)
    torch.cuda.synchronize()
    assert torch.equal(out[0].view(torch.int16), out[1].view(torch.int16)), (kind, cout, "in place")
    if kind == "zero":
        assert torch.equal(out[1].view(torch.int16), base.view(torch.int16))


@pytest.mark.parametrize("cout", [256, 40])
@pytest.mark.parametrize("kind", KINDS)
def test_wgrad_bits(kind, cout):
    from basedet_amd import ops
    geo, g = _operands(cout, kind, seed=2)
    d, hd, _ = _descs(ops, geo, 256, cout)
    x = torch.randn((geo.N * geo.pix_per_img, 256), device="cuda").to(torch.bfloat16)
    res = []
    for desc in (d, hd):
        ws = torch.empty((ops.conv2d_wgrad_bias_workspace_bytes(desc) // 4 + 64,), dtype=torch.float32, device="cuda")
        dw = torch.full((cout, 3, 3, 256), 7.0, device="cuda")
        db = torch.full((cout,), 7.0, device="cuda")
        ops.conv2d_wgrad_bias(desc, x, g, dw, db, ws)
        res.append((dw, db))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)), (kind, cout)
    assert torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32)), (kind, cout)
    if cout == 256:
        assert ops.conv2d_wgrad_bias_workspace_bytes(hd) > ops.conv2d_wgrad_bias_workspace_bytes(d)     # the ring walk's flags


def test_too_small_scratch_is_refused():
    from basedet_amd import ops
    from basedet_amd._lib import BasedetHipError
    geo, g = _operands(256, "corners", seed=3)
    d, hd, scratch = _descs(ops, geo, 256, 256)
    w = torch.zeros((256, 9, 256), dtype=torch.bfloat16, device="cuda")
    dx = torch.empty((geo.N * geo.pix_per_img, 256), dtype=torch.bfloat16, device="cuda")
    small = ops.gskip_desc(d)
    small.gskip_ws, small.gskip_ws_bytes = scratch.data_ptr(), ops.conv2d_dgrad_gskip_bytes(d) - 4
    with pytest.raises(BasedetHipError):
        ops.conv2d_dgrad(small, g, w, dx)
    with pytest.raises(BasedetHipError):
        ops.conv2d_dgrad(ops.gskip_desc(d), g, w, dx)          # no scratch at all
    torch.cuda.synchronize()


# ---- step level ------------------------------------------------------------------------------------------------------------------
def _step(make, batch):
    model = make()
    loss = model({k: (v if isinstance(v, dict) else torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in batch.items()})
    model.backward()
    torch.cuda.synchronize()
    arena = model.arena.g.clone()
    losses = {k: float(v) for k, v in loss.items()}
    del model
    torch.cuda.empty_cache()
    return arena, losses


def _check_on_off(cls, cfg, params, batch):
    def make(on):
        def f():
            cfg.MODEL.SPARSE_BOX_BWD = on
            return cls(cfg, params=params)
        return f
    a0, l0 = _step(make(0), batch)
    a1, l1 = _step(make(1), batch)
    a2, l2 = _step(make(1), batch)
    # (the loss scalars are summed with float atomics in the forward pass, before any backward launch: equal to fp32 summation order)
    for k in l0:
        assert abs(l1[k] - l0[k]) <= 1e-5 * abs(l0[k]) and abs(l2[k] - l0[k]) <= 1e-5 * abs(l0[k]), (k, l0[k], l1[k], l2[k])
    assert torch.equal(a0.view(torch.int32), a1.view(torch.int32)), int((a0 != a1).sum())
    assert torch.equal(a1.view(torch.int32), a2.view(torch.int32))


def _retina(N):
    from tests.test_model_gpu import _setup
    return _setup("resnet50", N, SIZE)


@pytest.mark.parametrize("N", [16, 2])
def test_retinanet_step_same_bits(N):
    from basedet_amd.models import RetinaNet
    cfg, params, batch = _retina(N)
    _check_on_off(RetinaNet, cfg, params, batch)


def test_retinanet_step_no_gt():
    from basedet_amd.models import RetinaNet
    cfg, params, batch = _retina(2)
    batch["im_info"] = batch["im_info"].copy()
    batch["im_info"][:, 4] = 0
    _check_on_off(RetinaNet, cfg, params, batch)


def test_retinanet_step_dense_gt():
    from basedet_amd.models import RetinaNet
    cfg, params, batch = _retina(2)
    rng = np.random.default_rng(5)
    G = 100
    gt = np.zeros((2, G, 5), np.float32)
    x0, y0 = rng.uniform(0, SIZE[1] - 40, (2, G)), rng.uniform(0, SIZE[0] - 40, (2, G))
    w, h = rng.uniform(16, 300, (2, G)), rng.uniform(16, 300, (2, G))
    gt[..., 0], gt[..., 1] = x0, y0
    gt[..., 2], gt[..., 3] = np.minimum(x0 + w, SIZE[1]), np.minimum(y0 + h, SIZE[0])
    gt[..., 4] = rng.integers(1, 81, (2, G))
    batch["gt_boxes"] = gt
    batch["im_info"] = batch["im_info"].copy()
    batch["im_info"][:, 4] = G
    _check_on_off(RetinaNet, cfg, params, batch)


def test_freeanchor_step_same_bits():
    from basedet_amd.configs import FreeAnchorConfig
    from basedet_amd.models import FreeAnchor, params as P
    from basedet_amd.utils import DummyLoader
    cfg = FreeAnchorConfig()
    cfg.MODEL.BATCHSIZE = 2
    params = P.init_retinanet_params(cfg, seed=0)
    batch = next(DummyLoader(2, SIZE, seed=0))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    _check_on_off(FreeAnchor, cfg, params, batch)
