"""Per-element audit of EVERY launch of a Faster R-CNN R50-FPN training step at the bench batch (16 x 800 x 1344, BASELINE config C4)
against float64, with the machinery of tests/audit.py (see tests/test_conv_audit_gpu.py for the protocol and the convolution bounds).

What this step runs that no other configuration reaches, and how each launch is bounded (derived, not tuned; S = the same operation on
|operands|, every reference computed from the launch's OWN operands, one image and one level at a time):
  * bf16 outputs of a K-long sum (forward, data gradient): tol = 2^-8 |ref| + abs_bf16(K) S with abs_bf16 = (2 x MFMA steps + 3) x 2^-24,
    never below 2^-16: two fp32 roundings per 32-product MFMA step of the dispatched kernel (audit.MFMA_K) and three epilogue adds.  It
    is 2^-16 up to 126 steps (K <= 4 032), 291 x 2^-24 = 1.73e-5 for res5's 3x3 512 -> 512 convolutions (K = 4 608, forward and data
    gradient) and 787 x 2^-24 = 4.7e-5 for rcnn.fc1 (K = 12 544), close to the weight S / 12 544 = 8.0e-5 of one product.  So every
    launch with K > 4 096 -- forward (K over Cin) or data gradient (K over Cout) -- is repeated on the same descriptor with the K-side
    operand kept only in columns c % 256 in {0, 255} (for fc1 the first and last channel of each of the 49 pooled positions after the
    in_chw permutation): a column dropped there costs about S / 98.
  * thin 1x1 layer (rpn.pred, 256 -> 15 + 1 channels over M = 1 432 368 pixels).  Forward: K = 256, 2^-16.  Backward, dx: 16 exact bf16
    products in ONE MFMA step: 2^-8 |ref| + 2^-16 S, exact zeros where the input is zero.  dW / db: the roundings of the kernel's own plan
    (audit.thin_bwd_roundings: ceil(groups / grid) = 350 FMAs per lane, 4 shuffle adds, ceil(grid / 8) = 32 reduce adds, 3 lane adds)
    x 2^-24 S = 2.3e-5 S; rows 15 of dW / db are exact zeros.  A 16-pixel group skipped at a pipeline hand-over moves dW by ~1e-5 S, so
    the launch is repeated with g kept only at the first and last pixel of every level of every image (160 pixels: a lost one costs
    S / 160).
  * RoIAlign forward (8 192 RoIs x 49 bins x 256 channels on P2..P5): 2^-8 |ref| + 34 x 2^-24 S (16 products, 16 adds, the 1/4 scale)
    + roi_weight_err(level) x F.  The bilinear weights come from fp32 sample coordinates: nine roundings of values of at most
    max(H, W) + 1 per axis (audit.roi_coord_err; roi_weight_err = 2 x that + 3 x 2^-24: 3.6e-4 on P2, 4.6e-5 on P5); F is the unweighted
    mean of |feat| over each sample's four corners -- over the 4 x 4 pixels around its cell only where the coordinate is within
    roi_coord_err of a cell edge and may land in the neighbouring cell.  Empty slots: exact zeros.
  * RoIAlign backward, tiled: g_P = bf16(g_P + adjoint): 2^-8 |ref| + (2 cnt + 4) x 2^-24 S (cnt = the (sample, corner) terms the
    reference counts for that pixel; capped at 2^-12) + roi_weight_err(level) x G (G: |g| / 4 of the samples within reach of the pixel).
    Scatter route (fp32 atomics): the same with a 2^-24 relative term, sum order free, no bit identity.
  * A RoI's level is evaluated in float64 and in float32; where they differ either result passes.  The count must stay <= 1 / 1 000.
  * subsample2x_fwd: bit-equal copy; subsample2x_bwd_add / f32_to_bf16(_add): 2^-8 |ref| + 2^-24 S; pixels off the even grid keep their
    bits.  upsample2x_add: as in the convolution audit.
  * rcnn_loss_fwd_bwd: see Audit.rcnn_loss_fwd_bwd; padding columns and empty rows are exact zeros.
  * fp32 outputs (weight / bias gradients): audit.fp32_roundings from each kernel's split plan + the edge probe, as in the convolution
    audit.  The FC layers are "1 x 8 192 x 1" descriptors: at most 8 192 / 16 MFMA steps in one chain (6.1e-5 S).
No launch may fall into an unknown-kernel row of those tables (au.unknown is empty).

OBSERVED on an MI355X (one audited step: 271 audited launches, 8.4 s wall, 7.2 s of it float64 references; 0 level-ambiguous RoIs of
16 384 sampled).  Worst err / tol and err / S per (kernel, pass):
  conv1x1_dense_kernel       fwd 0.992 / 3.7e-3   dgrad 0.991 / 3.3e-3   kprobe (fc1) 0.963 / 1.6e-3
  conv1x1_ring_kernel        fwd 0.991 / 3.3e-3   dgrad 0.991 / 3.5e-3
  conv3x3_pp_kernel          fwd 0.972 / 8.6e-4   dgrad 0.986 / 2.1e-3   kprobe (res5, K = 4 608) 0.990 / 3.9e-3
  conv3x3_patch_kernel       fwd 0.977 / 1.0e-3   dgrad 0.982 / 1.5e-3   conv3x3_pp128_kernel fwd 0.981 / 1.2e-3
  conv_igemm_kernel<32>      fwd 0.968 / 8.6e-4   dgrad 0.988 / 2.6e-3   kprobe 0.991 / 3.6e-3
  conv1x1_thin_fwd_kernel    fwd 0.982 / 1.7e-3
  conv1x1_thin_bwd_kernel    dx 0.985 / 3.9e-3    dW, db 0.0054 / 1.3e-7 (bound 2.3e-5 S)
  conv_wgrad1x1_ring_kernel  wgrad 0.042 / 2.6e-6   bias 0.0048 / 3.0e-7   probe 0.014 / 2.7e-7
  conv_wgrad1x1_kernel       wgrad 0.030 / 4.9e-7   probe 0.011 / 2.2e-7
  conv_wgrad3x3_ring_kernel  wgrad 0.039 / 4.5e-7   bias 0.0022 / 1.1e-7   probe 0.016 / 2.4e-7
  conv_wgrad3x3_kernel       wgrad 0.025 / 5.2e-7   probe 0.0094 / 2.2e-7
  roi_align_fwd_kernel       0.800 / 3.9e-3       roi_align_bwd_tile_kernel 0.928 (err / S is not meaningful where the weights vanish)
  rcnn_loss_kernel           grad 0.995 / 3.9e-3  cls 0.0098 / 4.9e-8   box 0.0050 / 2.5e-8
  stem_pool_kernel 0.984   subsample fwd bit-equal, bwd 0.996   upsample2x_add fwd / bwd 0.996
(The bf16 ratios sit just below 1 by construction: half a bf16 step is 2^-8 of a value just above a power of two.)
"""
import time

import numpy as np
import pytest
import torch

from tests.audit import Audit, CONV_ABI

pytestmark = pytest.mark.gpu
SIZE = (800, 1344)
B = 16
PYR_H, PYR_W = [200, 100, 50, 25, 13], [336, 168, 84, 42, 21]          # P2 .. P6 of an 800 x 1344 input: 89 523 pixels per image

# C ABI launches the step reaches that are NOT audited here, and the test that covers each at full size
NOT_AUDITED = {
    "bd_rpn_assign_encode": "test_model_gpu / test_fullsize_parity_gpu (RPN targets bit-exact against the oracle at 800 x 1344), test_assign_edges_gpu",
    "bd_sample_labels": "test_bench_batch_gpu::test_faster_rcnn_bench_batch_equals_tiled_batch2 (rpn_labels bit for bit at batch 16)",
    "bd_rpn_proposals": "test_bench_batch_gpu::test_faster_rcnn_bench_batch_equals_tiled_batch2 (rois / num_rois bit for bit at batch 16)",
    "bd_rcnn_sample_targets": "test_bench_batch_gpu::test_faster_rcnn_bench_batch_equals_tiled_batch2 (s_rois / s_labels / s_targets)",
    "bd_rpn_loss_fwd_bwd": "test_losses_large_gpu::test_rpn_loss_past_the_grid_cap",
    "bd_pad_normalize": "test_fullsize_parity_gpu (input of the full-size forward against the oracle)",
    "bd_pad_normalize_nchw": "test_fullsize_parity_gpu",
    "bd_anchors_generate": "test_fullsize_gpu::test_anchor_grid_invariants_full_size, test_boxops_gpu::test_anchors_bit_exact",
    "bd_weight_pack": "test_conv_gpu::test_elementwise_pack_colsum_sgd (the packed bf16 copies against torch), test_conv_gpu::test_conv_fwd_dgrad_wgrad",
    "bd_weight_pack_multi": "test_fullsize_parity_gpu (the packed weights of the full-size step)",
    "bd_stem_weight_pack": "test_fullsize_parity_gpu",
    "bd_rcnn_predict": "test_postprocess_gpu::test_rcnn_predict",
    "bd_segment_topk": "test_postprocess_gpu::test_segment_topk_inference_form",
    "bd_det_candidates": "test_postprocess_gpu::test_det_candidates",
    "bd_nms_batched": "test_postprocess_gpu::test_nms_batched_one_stage_candidate_list",
    "bd_det_finalize": "test_postprocess_gpu::test_det_finalize",
}

# kernels the C4 step dispatches for the shapes no other configuration runs: (pass, Cin, Cout, R, rows of the first level, levels) -> kernel
R_TRAIN = B * 512
P2 = B * 200 * 336
DENSE, RING, PP = "conv1x1_dense_kernel", "conv1x1_ring_kernel", "conv3x3_pp_kernel"
W1R, W3R = "conv_wgrad1x1_ring_kernel", "conv_wgrad3x3_ring_kernel"
PINNED = {
    ("fwd", 12544, 1024, 1, R_TRAIN, 1): DENSE, ("dgrad", 12544, 1024, 1, R_TRAIN, 1): DENSE, ("wgrad", 12544, 1024, 1, R_TRAIN, 1): W1R,     # rcnn.fc1
    ("fwd", 1024, 1024, 1, R_TRAIN, 1): DENSE, ("dgrad", 1024, 1024, 1, R_TRAIN, 1): DENSE, ("wgrad", 1024, 1024, 1, R_TRAIN, 1): W1R,        # rcnn.fc2
    ("fwd", 1024, 408, 1, R_TRAIN, 1): DENSE, ("dgrad", 1024, 408, 1, R_TRAIN, 1): DENSE, ("wgrad", 1024, 408, 1, R_TRAIN, 1): W1R,           # rcnn.pred
    ("fwd", 256, 256, 1, P2, 1): RING, ("wgrad", 256, 256, 1, P2, 1): W1R,          # P2 lateral (its input, res2, is frozen: no data gradient)
    ("fwd", 256, 256, 3, P2, 1): PP, ("dgrad", 256, 256, 3, P2, 1): PP, ("wgrad", 256, 256, 3, P2, 1): W3R,                                 # P2 output
    ("fwd", 256, 256, 3, P2, 5): PP, ("dgrad", 256, 256, 3, P2, 5): PP, ("wgrad", 256, 256, 3, P2, 5): W3R,                                 # rpn_conv, P2 .. P6
}


def _dev(batch):
    return {k: ({kk: torch.from_numpy(np.ascontiguousarray(vv)).cuda() for kk, vv in v.items()} if isinstance(v, dict)
                else torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in batch.items()}


def _setup(batch_size, pool=None):
    from basedet_amd.configs import FasterRCNNConfig
    from basedet_amd.models import FasterRCNN, params as P
    from basedet_amd.utils import DummyLoader
    cfg = FasterRCNNConfig()
    cfg.MODEL.BATCHSIZE = batch_size
    if pool is not None:
        cfg.MODEL.ROI_POOLER.SIZE = pool
    params = P.init_faster_rcnn_params(cfg, 0, residual_gamma=0.25)
    for k in ("rpn.rpn_cls_score.weight", "rpn.rpn_bbox_offsets.weight", "rcnn.pred_cls.weight", "rcnn.pred_delta.weight",
              "rcnn.fc1.weight", "rcnn.fc2.weight", "rpn.rpn_conv.weight"):
        params[k] = (params[k] * 3).astype(np.float32)        # (as the bench-batch parity test: top-k, NMS and sampling become non-trivial)
    batch = next(DummyLoader(batch_size, SIZE, seed=0))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    Gmax = batch["gt_boxes"].shape[1]
    A_total, R = 3 * sum(h * w for h, w in zip(PYR_H, PYR_W)), cfg.MODEL.RPN.TRAIN_POST_NMS_TOPK
    rng = np.random.default_rng(5)
    batch["sample_keys"] = dict(rpn_pos=rng.random((batch_size, A_total), dtype=np.float32), rpn_neg=rng.random((batch_size, A_total), dtype=np.float32),
                                rcnn_fg=rng.random((batch_size, R + Gmax), dtype=np.float32), rcnn_bg=rng.random((batch_size, R + Gmax), dtype=np.float32))
    return (lambda: FasterRCNN(cfg, params=params)), batch


def _step(model, batch):
    model(_dev(batch))
    model.backward()
    torch.cuda.synchronize()


KEEP = ("g_P", "s_rois", "s_labels")


@pytest.fixture(scope="module")
def audited_step():
    from basedet_amd import ops
    make, batch = _setup(B)
    model = make()
    model.async_wgrad = False
    _step(model, batch)
    plain = {"arena": model.arena.g.clone(), **{k: getattr(model._cur, k).clone() for k in KEEP}}
    del model
    torch.cuda.empty_cache()
    model = make()
    model.async_wgrad = False
    t0 = time.time()
    with Audit(ops) as au:
        au.thin_geom = ops.Geom(B, PYR_H, PYR_W)
        _step(model, batch)
    dt = time.time() - t0
    print("\n" + au.table(f"Faster R-CNN R50-FPN B={B} {SIZE[0]}x{SIZE[1]} training step ({dt:.1f} s)"))
    print(f"  level-ambiguous RoIs: {au.ambiguous} of {au.rois_seen}")
    for k, v in sorted(au.dispatch.items(), key=str):
        print(f"  dispatch {k} -> {v}")
    print("  reached:", dict(au.reached))
    yield model, au, plain
    del model
    torch.cuda.empty_cache()


def test_every_element_within_bound(audited_step):
    model, au, _ = audited_step
    assert not au.bad, "\n".join(au.bad[:20])
    assert au.stats
    assert not au.unknown, au.unknown                     # no launch fell into a table's unknown-kernel row
    assert au.rois_seen > B * 256 and au.ambiguous * 1000 <= au.rois_seen, (au.ambiguous, au.rois_seen)


def test_launch_accounting(audited_step):
    """C ABI calls == audited calls for every wrapped entry point; the counts follow the model's layer list; every launch symbol the step
    reaches is audited or named in NOT_AUDITED."""
    model, au, _ = audited_step
    abi, c = au.abi, au.calls
    for s in ("bd_conv2d_wgrad_queued", "bd_conv2d_fwd_fp8_ex", "bd_conv2d_dgrad_fp8", "bd_conv1x1_fp8", "bd_conv2d_wgrad_fp8", "bd_stem_conv7x7_fwd",
              "bd_roi_align_bwd", "bd_f32_to_bf16", "bd_f32_to_bf16_add", "bd_conv2d_fwd_gnstats"):
        assert abi[s] == 0, (s, abi[s])                   # not on the bf16 step with the default config (tiled RoIAlign backward)
    assert abi["bd_conv2d_fwd"] + abi["bd_conv2d_fwd_bits"] + abi["bd_conv2d_fwd_ex"] == c["conv2d_fwd"]
    assert abi["bd_conv2d_dgrad"] + abi["bd_conv2d_dgrad_bits"] + abi["bd_conv2d_dgrad_ex"] == c["conv2d_dgrad"]
    assert abi["bd_conv2d_wgrad"] + abi["bd_conv2d_wgrad_bias"] == c["conv2d_wgrad"] + c["conv2d_wgrad_bias"]
    for n in ("stem_pool_fwd", "bottleneck_fwd", "colsum_bf16", "upsample2x_add_fwd", "upsample2x_add_bwd", "conv1x1_thin_fwd", "conv1x1_thin_bwd",
              "roi_align_fwd", "roi_align_bwd_bf16", "subsample2x_fwd", "subsample2x_bwd_add", "rcnn_loss_fwd_bwd"):
        assert abi["bd_" + n] == c[n], n
    convs = list(model.convs.values())
    fused = [blk for blk, b in zip(model.blocks, model._cur.blk) if getattr(b, "fused", False)]
    in_fused = sum(len(blk["convs"]) + (blk["ds"] is not None) for blk in fused)
    assert c["bottleneck_fwd"] == len(fused) and c["stem_pool_fwd"] == 1
    # the RPN prediction layer runs on the thin kernels: one forward and one weight gradient fewer on the generic entry points
    assert c["conv1x1_thin_fwd"] == 1 and c["conv1x1_thin_bwd"] == 1
    assert c["conv2d_fwd"] == len(convs) - in_fused - 1
    assert c["conv2d_wgrad"] + c["conv2d_wgrad_bias"] == sum(1 for cv in convs if cv.trainable) - 1
    assert model.wgrads.queue is None
    assert c["roi_align_fwd"] == 1 and c["roi_align_bwd_bf16"] == 1 and c["roi_align_bwd"] == 0 and c["f32_to_bf16"] == 0
    assert c["subsample2x_fwd"] == 1 and c["subsample2x_bwd_add"] == 1 and c["rcnn_loss_fwd_bwd"] == 1
    assert c["upsample2x_add_fwd"] == 3 and c["upsample2x_add_bwd"] == 3
    unplaced = {s for s, n in au.reached.items() if n and s not in CONV_ABI and s not in NOT_AUDITED}
    assert not unplaced, unplaced
    for s in ("bd_rpn_assign_encode", "bd_sample_labels", "bd_rpn_proposals", "bd_rcnn_sample_targets", "bd_rpn_loss_fwd_bwd", "bd_anchors_generate"):
        assert au.reached[s] > 0, s
    assert au.reached["bd_pad_normalize"] + au.reached["bd_pad_normalize_nchw"] > 0
    pyr = model._cur.pyr
    assert (pyr.H, pyr.W, pyr.pixels) == (PYR_H, PYR_W, B * 89523)


def test_dispatch(audited_step):
    """The thin launches ran conv1x1_thin_fwd_kernel / conv1x1_thin_bwd_kernel; the kernels of the FC layers (all three directions) and of
    the P2-level convolutions are pinned by name."""
    model, au, _ = audited_step
    assert ("conv1x1_thin_fwd_kernel", "fwd") in au.stats and ("conv1x1_thin_bwd_kernel", "dgrad") in au.stats
    assert ("conv1x1_thin_bwd_kernel", "wgrad") in au.stats and ("conv1x1_thin_bwd_kernel", "probe") in au.stats
    assert any(p == "kprobe" for _, p in au.stats)         # rcnn.fc1's K-edge probe ran
    for key, kern in PINNED.items():
        assert key in au.dispatch, (key, sorted(au.dispatch, key=str))
        assert au.dispatch[key] == kern, (key, au.dispatch[key], kern)
    assert ("dgrad", 256, 256, 1, P2, 1) not in au.dispatch


def test_audit_leaves_the_step_unchanged(audited_step):
    """Also the bit-reproducibility of the C4 step at batch 16: two models, two runs, the same gradient arena, dL/dP and RoI samples."""
    model, au, plain = audited_step
    assert torch.equal(model.arena.g, plain["arena"]), int((model.arena.g != plain["arena"]).sum())
    for k in KEEP:
        a, b = getattr(model._cur, k), plain[k]
        same = torch.equal(a.view(torch.int16), b.view(torch.int16)) if a.dtype == torch.bfloat16 else torch.equal(a, b)
        assert same, k


def test_inference_forward_audited():
    """One image through FasterRCNN.inference under the same wrappers: no data-gradient launch, the 1 000-row FC launches and the RoIAlign
    forward over every proposal slot within bound."""
    from basedet_amd import ops
    make, batch = _setup(B)
    one = {k: v[:1] for k, v in batch.items() if not isinstance(v, dict)}
    model = make().eval()
    model.async_wgrad = False
    with Audit(ops) as au:
        model(one)
        torch.cuda.synchronize()
    print("\n" + au.table("Faster R-CNN inference 1x800x1344"))
    print(f"  level-ambiguous RoIs: {au.ambiguous} of {au.rois_seen}")
    assert not au.bad, "\n".join(au.bad[:20])
    assert not au.unknown, au.unknown
    c = au.calls
    assert c["conv2d_dgrad"] == 0 and c["conv2d_wgrad"] + c["conv2d_wgrad_bias"] == 0 and c["conv1x1_thin_bwd"] == 0 and c["roi_align_bwd_bf16"] == 0
    assert c["conv2d_fwd"] > 0 and c["stem_pool_fwd"] == 1 and c["roi_align_fwd"] == 1 and c["subsample2x_fwd"] == 1
    for s in ("bd_conv2d_wgrad_queued", "bd_conv2d_fwd_fp8_ex", "bd_conv2d_dgrad_fp8", "bd_conv1x1_fp8", "bd_conv2d_wgrad_fp8", "bd_stem_conv7x7_fwd",
              "bd_conv2d_fwd_gnstats", "bd_roi_align_bwd", "bd_f32_to_bf16", "bd_f32_to_bf16_add", "bd_rcnn_loss_fwd_bwd", "bd_subsample2x_bwd_add"):
        assert au.abi[s] == 0, (s, au.abi[s])
    assert au.abi["bd_conv2d_fwd"] + au.abi["bd_conv2d_fwd_bits"] + au.abi["bd_conv2d_fwd_ex"] == c["conv2d_fwd"]
    assert au.rois_seen == 1000 and au.ambiguous * 1000 <= au.rois_seen
    fc = {k: v for k, v in au.dispatch.items() if k[0] == "fwd" and k[4] == 1000}
    assert {(k[1], k[2]) for k in fc} == {(12544, 1024), (1024, 1024), (1024, 408)}, fc
    assert any(p == "kprobe" for _, p in au.stats)
    unplaced = {s for s, n in au.reached.items() if n and s not in CONV_ABI and s not in NOT_AUDITED}
    assert not unplaced, unplaced


def test_scatter_route_audited():
    """Batch 2 with ROI_POOLER.SIZE = (14, 14): the plan takes bd_roi_align_bwd (fp32 atomics) + bd_f32_to_bf16(_add), through the same
    wrappers.  The atomics leave the order of the sums free: the bound uses the contribution count, no bit identity is asserted."""
    from basedet_amd import ops
    make, batch = _setup(2, pool=(14, 14))
    model = make()
    model.async_wgrad = False
    with Audit(ops) as au:
        au.thin_geom = ops.Geom(2, PYR_H, PYR_W)
        _step(model, batch)
    print("\n" + au.table("Faster R-CNN B=2, 14 x 14 pooler (scatter route)"))
    assert not au.bad, "\n".join(au.bad[:20])
    assert not au.unknown, au.unknown
    assert not model._cur.roi_bwd_tiled
    c = au.calls
    assert c["roi_align_bwd"] == 1 and c["f32_to_bf16"] == 1 and c["roi_align_bwd_bf16"] == 0 and c["roi_align_fwd"] == 1
    assert au.abi["bd_roi_align_bwd"] == 1 and au.abi["bd_f32_to_bf16"] + au.abi["bd_f32_to_bf16_add"] == 1
    assert ("roi_align_bwd_kernel", "bwd") in au.stats and au.ambiguous * 1000 <= au.rois_seen
