"""Per-element audit of every convolution launch of a bench-size training step (16 x 800 x 1344) against float64.

The model runs one forward + backward pass with the entry points of basedet_amd.ops wrapped (the SGD update that ends a training step
is left out: it launches no convolution, and the gradient arena it would read is compared bit for bit instead): each wrapper clones what the launch updates in
place, calls the kernel, synchronises, reads bd_conv_last_kernel(), recomputes the launch in float64 from ITS OWN operands (the packed bf16
weights the kernel received, tests/util.py) and checks every element; the kernel's output stays in place, so the step goes on with real
data.  Rows of an output buffer that the launch's levels do not cover must come back bit for bit as they were.

Bounds (derived, not tuned; S = the same operation on |operands|):
  * bf16 outputs (forward, data gradient, stem, fused blocks): the kernel rounds an fp32 value v to bf16, |bf16(v) - v| <= 2^-9 |v|, and
    |v - ref| <= delta, the fp32 accumulation error.  tol = 2^-8 |ref| + abs S with abs computed from the launch's own K (tests/audit.py,
    abs_bf16): two fp32 roundings of at most 2^-24 S per 32-product MFMA step plus three epilogue adds, never below 2^-16.  That is 2^-16
    for every launch of these steps (K <= 2 304: at most 147 roundings) EXCEPT res5's three 3x3 512 -> 512 convolutions, forward and data
    gradient (K = 4 608: 291 roundings, 1.73e-5 S -- 14 % above the 2^-16 this file used for them before the term followed K).  Those six
    launches have K > 4 096 and are therefore also repeated with the K-edge probe (input kept in the first and last column of every
    256-column block).  A tap missing from a 2 304-term sum moves the result by about S / 2 304 >> 2^-16 S.  A kernel the MFMA table does
    not know would be counted with 16-product steps (looser); the test asserts that none is.
  * elements that are exactly representable (a closed ReLU / mask gate: 0 or the bf16 `add`; a ReLU input below -2^-16 S; pixels a
    sparse strided data gradient must not touch) are compared for equality.
  * fp32 outputs (weight and bias gradients, column sums): a bound per launch from the kernel's own plan (tests/audit.py fp32_roundings, which
    mirrors the split plans of conv_wgrad3x3_ring.hip, conv_wgrad3x3.hip, conv_wgrad1x1_ring.hip, conv_wgrad1x1.hip and the column-sum
    pass of image_ops.hip).  A workgroup accumulates its pixel range in fp32 MFMA accumulators; each MFMA step sums K exact bf16 products
    and adds them to the accumulator: two roundings of at most 2^-24 S.  (One rounding per step is not enough: for the 720-channel
    cls_score bias on the ring kernel, 1 224 steps + 10 partials would allow 7.4e-5 S, and 1.0e-4 S is observed -- the 720 focal
    gradients are nearly one-signed, so the rounding errors add up.)  Then the fixed-order reduce adds the `splits` partials, the row
    scale and an accumulate add one rounding each.  tol = roundings x 2^-24 S, never looser than 2^-12 S.  The column-sum pass is plain
    fp32 adds: rows per thread + rows in flight + 1 024 / 32 + 32 partials + levels.
    Observed worst err / S on an MI355X (RetinaNet-R50 step, B = 16): weight gradients 8.6e-6 (conv_wgrad3x3_ring_kernel), 6.6e-7
    (conv_wgrad1x1_ring_kernel), 3.8e-7 (conv_wgrad3x3_kernel), 2.4e-7 (conv_wgrad1x1_kernel); bias gradients 1.0e-4 (ring kernel,
    cls_score).  The worst err / tol of each kernel is in the printed table.
  * A per-element bound cannot see a weight-gradient kernel drop a few pixels of a 268 800-pixel sum (one 64-pixel patch moves a weight
    by ~1e-5 S).  So every weight-gradient launch is repeated on the same descriptor (same kernel, same split plan) with g kept only at
    the first and the last pixel of every level of every image -- the pixels where a split, a patch row or a tail starts and ends -- and
    zero elsewhere: a pixel the kernel skips there costs about 1 / (2 N levels) of S, against a bound of ~1e-4 S.
  * upsample2x_add: the bilinear weights 0.75 / 0.25 are exact, <= 16 products and one add in fp32: tol = 2^-8 |ref| + 2^-19 S.

Every image of the batch is audited (the float64 references of a whole RetinaNet step take about 5 s on an MI355X).
"""
import collections
import time

import numpy as np
import pytest
import torch

from tests import util as U
from tests.audit import Audit, REL_BF16

pytestmark = pytest.mark.gpu
SIZE = (800, 1344)
B = 16


# ---- the models ------------------------------------------------------------------------------------------------------------------------
def _dev(batch):
    return {k: ({kk: torch.from_numpy(vv).cuda() for kk, vv in v.items()} if isinstance(v, dict)
                else torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in batch.items()}


def _make(name):
    if name == "retinanet":
        from basedet_amd.models import RetinaNet
        from tests.test_model_gpu import _setup
        cfg, params, batch = _setup("resnet50", B, SIZE)
        return (lambda: RetinaNet(cfg, params=params)), batch
    from basedet_amd.configs import FCOSConfig
    from basedet_amd.models import FCOS, params as P
    from basedet_amd.utils import DummyLoader
    cfg = FCOSConfig()
    cfg.MODEL.BATCHSIZE = B
    params = P.init_fcos_params(cfg, seed=0, residual_gamma=0.25)
    batch = next(DummyLoader(B, SIZE, seed=0))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    return (lambda: FCOS(cfg, params=params)), batch


# what the RetinaNet-R50 step dispatches (tests/test_conv_gpu.py pins the same names for its descriptors)
PINNED = {("conv3x3_pp_kernel", "fwd"), ("conv3x3_pp_kernel", "dgrad"), ("conv_wgrad3x3_ring_kernel", "wgrad"),
          ("conv1x1_ring_kernel", "fwd"), ("conv1x1_ring_kernel", "dgrad"), ("conv_wgrad1x1_ring_kernel", "wgrad"),
          ("conv_igemm_kernel<32>", "fwd"), ("conv_igemm_kernel<32>", "dgrad"), ("conv_wgrad3x3_kernel", "wgrad"),
          ("conv_wgrad1x1_kernel", "wgrad")}


@pytest.fixture(scope="module", params=["retinanet", "fcos"])
def audited_step(request):
    from basedet_amd import ops
    make, batch = _make(request.param)
    # the same step without wrappers first: the audited step must leave the gradient arena bit for bit as it is
    model = make()
    model.async_wgrad = False
    model(_dev(batch))
    model.backward()
    torch.cuda.synchronize()
    arena_plain = model.arena.g.clone()
    del model
    torch.cuda.empty_cache()
    model = make()
    model.async_wgrad = False
    t0 = time.time()
    with Audit(ops) as au:
        model(_dev(batch))
        model.backward()
        torch.cuda.synchronize()
    dt = time.time() - t0
    print("\n" + au.table(f"{request.param} B={B} {SIZE[0]}x{SIZE[1]} training step ({dt:.1f} s)"))
    yield request.param, model, au, arena_plain
    del model
    torch.cuda.empty_cache()


def test_every_element_within_bound(audited_step):
    name, model, au, _ = audited_step
    assert not au.bad, "\n".join(au.bad[:20])
    assert au.stats
    assert not au.unknown, au.unknown            # every dispatched kernel is in the MFMA / weight-gradient plan tables: no loosened row


def test_dispatched_kernels_and_launch_counts(audited_step):
    """Every conv launch went through an audited wrapper (C ABI calls == audited calls), and their number follows the model's own layer
    list: one forward per layer outside a fused block, one weight gradient per trainable layer."""
    name, model, au, _ = audited_step
    abi = au.abi
    for s in ("bd_conv2d_wgrad_queued", "bd_conv2d_fwd_fp8_ex", "bd_conv2d_dgrad_fp8", "bd_conv1x1_fp8", "bd_conv2d_wgrad_fp8",
              "bd_conv1x1_thin_fwd", "bd_conv1x1_thin_bwd", "bd_stem_conv7x7_fwd"):
        assert abi[s] == 0, (s, abi[s])                   # none of these is on the bf16 RetinaNet / FCOS step with the default config
    c = au.calls
    assert abi["bd_conv2d_fwd"] + abi["bd_conv2d_fwd_bits"] + abi["bd_conv2d_fwd_ex"] == c["conv2d_fwd"]
    assert abi["bd_conv2d_dgrad"] + abi["bd_conv2d_dgrad_bits"] + abi["bd_conv2d_dgrad_ex"] == c["conv2d_dgrad"]
    assert abi["bd_conv2d_wgrad"] + abi["bd_conv2d_wgrad_bias"] == c["conv2d_wgrad"] + c["conv2d_wgrad_bias"]
    for n in ("stem_pool_fwd", "bottleneck_fwd", "conv2d_fwd_gnstats", "colsum_bf16", "upsample2x_add_fwd", "upsample2x_add_bwd"):
        assert abi["bd_" + n] == c[n], n
    convs = list(model.convs.values())
    fused = [blk for blk, b in zip(model.blocks, model._cur.blk) if getattr(b, "fused", False)]
    in_fused = sum(len(blk["convs"]) + (blk["ds"] is not None) for blk in fused)
    assert c["bottleneck_fwd"] == len(fused) and c["stem_pool_fwd"] == 1
    assert c["conv2d_fwd"] + c["conv2d_fwd_gnstats"] == len(convs) - in_fused
    assert c["conv2d_wgrad"] + c["conv2d_wgrad_bias"] == sum(1 for cv in convs if cv.trainable)
    assert model.wgrads.queue is None                      # WGRAD_QUEUE = "layer": no deferred reduce on this step
    if name == "retinanet":
        assert c["upsample2x_add_fwd"] == 2 and c["upsample2x_add_bwd"] == 2
        audited = set(au.stats)
        missing = {k for k in PINNED if k not in audited}
        assert not missing, missing
        dense = {k for (k, p) in au.stats if p == "fwd" and k in ("conv1x1_dense_kernel", "conv1x1_gemm_kernel")}
        assert dense, sorted(au.stats)
    else:
        assert c["conv2d_fwd_gnstats"] == 8 and ("groupnorm_fwd_parts", "stats") in au.stats


def test_relu_bits_and_fused_blocks(audited_step):
    """Forward launches that wrote gate bits wrote (y > 0) of their own y; the data gradients that read them were audited with the gate
    decoded from the bits; each fused frozen res2 block equals its separate launches bit for bit at batch 16."""
    name, model, au, _ = audited_step
    assert au.bits_checked > 0 and au.bits_read > 0, (au.bits_checked, au.bits_read)
    assert len(au.fused) == 3 and all(same for _, same in au.fused), au.fused


def test_audit_leaves_the_step_unchanged(audited_step):
    name, model, au, arena_plain = audited_step
    assert torch.equal(model.arena.g, arena_plain), int((model.arena.g != arena_plain).sum())


def test_inference_forward_audited():
    """The inference forward (one image, RetinaNet-R50 at 800 x 1344) through the same wrappers."""
    from basedet_amd import ops
    make, batch = _make("retinanet")
    one = {k: ({kk: vv[:1] for kk, vv in v.items()} if isinstance(v, dict) else v[:1]) for k, v in batch.items()}
    model = make().eval()
    model.async_wgrad = False
    with Audit(ops) as au:
        model(one)
        torch.cuda.synchronize()
    print("\n" + au.table("retinanet inference 1x800x1344"))
    assert not au.bad, "\n".join(au.bad[:20])
    assert au.calls["conv2d_dgrad"] == 0 and au.calls["conv2d_fwd"] > 0 and au.calls["stem_pool_fwd"] == 1


def test_groupnorm_fwd_bwd_on_the_bench_pyramid():
    """bd_groupnorm_fwd / bd_groupnorm_bwd (GroupNorm(32, 256) + ReLU) over 16 images of the bench pyramid (100x168 .. 7x11) against
    float64 from the same bf16 inputs.  S_z = |gamma| rstd (|y| + |mean|) + |beta|; the statistics are fp32 sums over <= 134 400
    elements in a two-stage fixed-order reduce (128-pixel slots), so the relative error of mean and rstd stays below 2^-14 (< 2^10
    roundings): z within 2^-8 |z| + 2^-14 S_z.  The backward's gate is z > 0 of the forward's own output (the kernel recomputes it with
    the forward's arithmetic); dy within 2^-8 |dy| + 2^-14 S_dy, dgamma / dbeta (fp32 sums over the batch) within 2^-14 S."""
    from basedet_amd import ops
    from basedet_amd.models.fcos import GN_EPS
    gen = torch.Generator().manual_seed(21)
    C, G = 256, 32
    pyr = ops.Geom(B, [100, 50, 25, 13, 7], [168, 84, 42, 21, 11])
    y = (torch.randn(pyr.pixels, C, generator=gen) * 2 + 0.3).to(torch.bfloat16).cuda()
    dz = torch.randn(pyr.pixels, C, generator=gen).to(torch.bfloat16).cuda()
    gamma = (torch.rand(C, generator=gen) + 0.5).cuda()
    beta = (torch.randn(C, generator=gen) * 0.2).cuda()
    stats = torch.empty((B, pyr.nlev, G, 2), dtype=torch.float32, device="cuda")
    z = torch.empty_like(y)
    dy = torch.empty_like(y)
    dgamma = torch.full((C,), 0.5, dtype=torch.float32, device="cuda")
    dbeta = torch.full((C,), -0.5, dtype=torch.float32, device="cuda")
    ws = torch.empty((ops.groupnorm_workspace_bytes(B, pyr.nlev, C, pyr.pix_per_img) // 4 + 16,), dtype=torch.float32, device="cuda")
    ops.groupnorm_fwd(y, gamma, beta, pyr, C, GN_EPS, True, stats, z, ws)
    ops.groupnorm_bwd(dz, y, gamma, beta, stats, pyr, C, True, dy, dgamma, dbeta, ws, accumulate=True)
    torch.cuda.synchronize()
    g64, b64 = gamma.double(), beta.double()
    worst = collections.defaultdict(float)
    dg, sdg = 0.5 + torch.zeros(C, dtype=torch.float64, device="cuda"), 0.5 + torch.zeros(C, dtype=torch.float64, device="cuda")
    db, sdb = -0.5 + torch.zeros_like(dg), 0.5 + torch.zeros_like(dg)
    for li in range(pyr.nlev):
        n_px = pyr.H[li] * pyr.W[li]
        lv = lambda t: t.view(B, pyr.pix_per_img, C)[:, pyr.off[li]:pyr.off[li] + n_px]
        yv = lv(y).double().view(B, n_px, G, 8)
        mu = yv.mean((1, 3), keepdim=True)
        rstd = 1.0 / torch.sqrt(yv.var((1, 3), correction=0, keepdim=True) + GN_EPS)
        xh = (yv - mu) * rstd
        gm, bm = g64.view(1, 1, G, 8), b64.view(1, 1, G, 8)
        pre = xh * gm + bm
        zr = pre.clamp_min(0)
        Sz = gm.abs() * rstd * (yv.abs() + mu.abs()) + bm.abs()
        zg = lv(z).view(B, n_px, G, 8)
        worst["z"] = max(worst["z"], float(U.bound_ratio(zg, zr, Sz, REL_BF16, 2.0 ** -14).max()))
        st = stats[:, li].double()
        worst["mean"] = max(worst["mean"], float(((st[..., 0] - mu.view(B, G)).abs() / (2.0 ** -14 * yv.abs().mean((1, 3)))).max()))
        worst["rstd"] = max(worst["rstd"], float(((st[..., 1] - rstd.view(B, G)).abs() / (2.0 ** -14 * rstd.view(B, G))).max()))
        gate = zg.float() > 0
        d = lv(dz).double().view(B, n_px, G, 8) * gate
        dxh = d * gm
        m1 = dxh.mean((1, 3), keepdim=True)
        m2 = (dxh * xh).mean((1, 3), keepdim=True)
        ref = rstd * (dxh - m1 - xh * m2)
        Sdy = rstd * (dxh.abs() + dxh.abs().mean((1, 3), keepdim=True) + xh.abs() * (dxh * xh).abs().mean((1, 3), keepdim=True))
        worst["dy"] = max(worst["dy"], float(U.bound_ratio(lv(dy).view(B, n_px, G, 8), ref, Sdy, REL_BF16, 2.0 ** -14).max()))
        dg = dg + (d * xh).sum((0, 1)).reshape(C)
        sdg = sdg + (d * xh).abs().sum((0, 1)).reshape(C)
        db = db + d.sum((0, 1)).reshape(C)
        sdb = sdb + d.abs().sum((0, 1)).reshape(C)
    worst["dgamma"] = float(((dgamma.double() - dg).abs() / (2.0 ** -14 * sdg)).max())
    worst["dbeta"] = float(((dbeta.double() - db).abs() / (2.0 ** -14 * sdb)).max())
    print("\ngroupnorm 16 x pyramid x 256, worst err/tol:", dict(worst))
    for k, v in worst.items():
        assert v <= 1.0, (k, v)
