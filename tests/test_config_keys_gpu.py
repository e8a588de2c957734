"""Every detector at non-default values of the config keys it reads: one training step against the oracle per key, then all keys at once.

Fixture and assertions are those of tests/test_model_gpu.py (resnet18, 2 x 128 x 160, bf16; check_retinanet_step, check_fcos_step,
check_atss_step, check_faster_rcnn_step, check_*_inference): nothing is restated or loosened here.  tests/test_config_keys_cpu.py shows on
the CPU that every case's fixture feels its key by >= 10 x what these comparisons tolerate, and asserts the refusals.

Time: the module is to stay within the time of tests/test_model_gpu.py, so a key gets a case of its own only where nothing else tells its
kernel apart: config_key_cases.KERNEL_LEVEL names every per-key case left out and what covers it ("(all)" below = the family's "all keys
together" step, which test_config_keys_cpu.py shows, leaving one key out at a time, to feel every key it moves).

Regression targets and tolerances: every RetinaNet / RPN bound is relative, so BOX_REG.STD < 1 (targets x 1/std) needs no change.  The one
absolute term that depends on a coder is the 1e-3 of the s_targets comparison (RoI coordinates at 1e-3 px, divided by RCNN_BOX_REG.STD =
(0.1, 0.1, 0.2, 0.2)); the RCNN_BOX_REG case uses LARGER stds, so the reference target shrinks and the term is kept as it is.

INVENTORY -- the MODEL.* / TEST.* keys the reference's model code reads (models/det/{retinanet,free_anchor,fcos,atss,ota,faster_rcnn,rpn}.py,
layers/head/*.py) for the six detectors; "K:" = kernel / host code of ours that consumes it, "T:" = the test that moves it, "R:" = refused
(ValueError from check_config, asserted by test_config_keys_cpu.py::test_unimplemented_value_is_refused) with the accepted values.

All six
  BACKBONE.NAME, OUT_FEATURES, OUT_FEATURE_CHANNELS   K: FPNDetector._build_layers.  T: test_model_gpu (resnet18 / resnet50), test_r101_gpu
  BACKBONE.IMG_MEAN, IMG_STD    K: bd stem normalisation (pre_process).  T: test_raw_input_gpu, test_layers_gpu
  BACKBONE.NORM                 K: LiveNorms / bd_bn_* under every backbone convolution and the stem ("BN"; "SyncBN" at world size 1 is "BN").
                                T: test_backbone_norm_gpu (RetinaNet R18 / R50, Faster R-CNN), test_live_norm_families_gpu (FCOS, ATSS, OTA,
                                FreeAnchor), test_fpn_norm_gpu (deconv), test_multiscale_gpu, test_ema_gpu.  R: any value but "FrozenBN" / "BN" /
                                "SyncBN"; a live norm with FREEZE_AT >= 1, with fp8 weights, "SyncBN" at world size > 1
  BACKBONE.FREEZE_AT            K: trainable set (0 trains the 7x7 stem, 1 freezes it, >= 2 freezes layer1 too).  T: test_stem_bwd_gpu.
                                R: not an integer >= 0; >= 1 under a live BACKBONE.NORM
  FPN.NORM                      K: LiveNorms / bd_bn_* under every lateral and output convolution.  T: test_fpn_norm_gpu and the modules named
                                at BACKBONE.NORM.  R: any value but None / "BN" / "SyncBN"; a live norm with fp8 weights, "SyncBN" at world
                                size > 1 (all: test_config_keys_cpu::test_unimplemented_value_is_refused, test_live_norm_values_are_accepted)
  FPN.UPSAMPLE                  K: DeconvLayer.  T: test_fpn_deconv_gpu; R: other than "resize" / "deconv" (not read by Faster R-CNN, as in the reference)
  FPN.STRIDES, OUT_FEATURES, OUT_CHANNELS, TOP_BLOCK_IN_CHANNELS, TOP_BLOCK_IN_FEATURE
                                K: pyramid geometry.  Out of scope here: they define the network's shape, not a parameter of a kernel; the
                                fixtures fix them.  FCOS family R: FPN.OUT_CHANNELS != 256 (GroupNorm kernel: 32 groups x 8 channels)
  DATA.NUM_CLASSES              T: test_class_count_gpu / _cpu
  TEST.IOU_THRESHOLD, TEST.CLS_THRESHOLD, TEST.MAX_BOXES_PER_IMAGE
                                K: det_select / nms_batched / det_finalize (FPNDetector._detect).  T: test_batched_inference_gpu and
                                test_fullsize_inference_gpu move them; test_postprocess_gpu at kernel level.  Not duplicated here.
RetinaNet (and FreeAnchor, which shares network, anchors and coder)
  BOX_REG.MEAN, BOX_REG.STD     K: bd_retina_assign_encode (encode), bd_det_candidates mode 0 (decode),
                                bd_freeanchor_loss_fwd_bwd (decode and encode).
                                T: test_retinanet_key[BOX_REG], (all), test_retinanet_inference_box_reg; kernel level, coders A and B:
                                test_assign_edges_gpu (assign_encode), test_boxops_gpu (box_encode / box_decode), test_postprocess_gpu
                                (det_candidates), test_batched_inference_gpu::test_batched_retinanet_decodes_with_box_reg (the batched
                                decode, three images), test_freeanchor_gpu::test_freeanchor_losses_and_gradients (the bag-loss kernel)
  MATCHER.THRESHOLDS            K: bd_retina_assign_encode.  T: test_retinanet_key (all), test_assign_edges_gpu; R: not two ascending values
  MATCHER.ALLOW_LOW_QUALITY     K: bd_retina_assign_encode.  T: test_retinanet_key[MATCHER.ALLOW_LOW_QUALITY]
  MATCHER.LABELS                R: [0, -1, 1] only (hard-wired in the assign kernels).  FreeAnchor never calls the matcher: any value
  LOSSES.FOCAL_LOSS_ALPHA, FOCAL_LOSS_GAMMA   K: bd_focal_loss_fwd_bwd (gamma != 2: the general kernel).  T: test_retinanet_key (all), test_boxops_gpu
  LOSSES.SMOOTH_L1_BETA, REG_LOSS_WEIGHT      K: bd_smooth_l1_fwd_bwd.  T: test_retinanet_key[LOSSES.REG_LOSS_WEIGHT], (all), test_boxops_gpu
  HEAD.NUM_CONVS, HEAD.CLS_PRIOR_PROB         K: RetinaNet._build_head / init_retina_head.  T: test_retinanet_key[HEAD.CLS_PRIOR_PROB], (all)
  HEAD.WITH_NORM                R: True only (test_fpn_variants_cpu)
  ANCHOR.SCALES, ANCHOR.RATIOS  K: _build_base_anchors, bd_anchors_generate, head width A.  T: test_retinanet_key (all) (A = 4; default 9); R: per-level scale lists of unequal length, a list count other than 1 or the
                                level count, more than one ratio list
  ANCHOR.OFFSET                 K: bd_anchors_generate.  T: test_retinanet_key[ANCHOR.OFFSET]
  BUCKET.BOX_IOU_THRESH, BUCKET.BUCKET_SIZE (FreeAnchor)   K: bd_freeanchor_loss_fwd_bwd.  T: test_freeanchor_gpu, test_freeanchor_edges_gpu.
                                Neither they nor BOX_REG are moved through a FreeAnchor MODEL here (no FreeAnchor training-step helper
                                among the four this module imports): free_anchor.py's hand-over of m.BOX_REG to the kernel is left uncovered.
FCOS
  ANCHOR.NUM_ANCHORS            R: 1 only
  ANCHOR.OFFSET                 K: bd_points_generate.  T: test_fcos_key[ANCHOR.OFFSET]
  HEAD.NUM_CONVS, CLS_PRIOR_PROB               K: FCOS._build_head / init_point_head.  T: test_fcos_key[HEAD.CLS_PRIOR_PROB], (all)
  HEAD.CENTER_SAMPLING_RADIUS   K: bd_fcos_assign (<= 0: inside the box).  T: test_fcos_key (all), test_assign_edges_gpu (0, 0.5)
  HEAD.OBJECT_SIZES_OF_INTEREST K: bd_fcos_assign.  T: test_fcos_key (all), test_assign_edges_gpu (overlapping, empty); R: not one pair per level
  LOSSES.FOCAL_LOSS_ALPHA, FOCAL_LOSS_GAMMA, REG_LOSS_WEIGHT   K: bd_focal_loss_fwd_bwd, bd_iou_ltrb_fwd_bwd.  T: test_fcos_key[LOSSES.REG_LOSS_WEIGHT], (all)
  LOSSES.IOU_LOSS_TYPE          T: test_iou_loss_types_gpu (all four); R: any other string
  BOX_REG.*                     carried by the config as in the reference; the reference's FCOS never reads it (PointCoder): ignored by both
ATSS = FCOS's keys without the two assignment keys, plus
  ANCHOR.TOPK                   K: bd_atss_assign.  T: test_atss_key (all: 16 > the 6 and 2 points of the coarsest levels), test_boxops_gpu (1, 9, 13);
                                R: outside 1..16 (the kernel's candidate list)
  ANCHOR.SCALE                  K: bd_atss_assign.  T: test_atss_key (all), test_boxops_gpu (4, 8)
OTA = FCOS's network keys, plus
  MATCHING                      T: test_ota_gpu (topk, sinkhorn); other values: assertion
  HEAD.NORM_REG_TARGETS, WITH_NORM, SHARE_PARAM   accepted: True only (assertion in OTA.__init__)
  HEAD.COST_REG_WEIGHTS, HEAD.CANDIDATE_K      K: bd_ota_assign.  T: kernel level only (test_ota_gpu, test_ota_edges_gpu at the defaults 1.5 / 10).
                                NOT moved: OTA's model step is compared as a set (99.5 % of the labels, losses at 0.1), which a per-key
                                case cannot be held to at ten times the tolerance; left uncovered.
Faster R-CNN
  ANCHOR.SCALES, RATIOS, OFFSET K: as RetinaNet (RPN head width A).  T: test_faster_rcnn_key[ANCHOR.OFFSET], (all) (A = 4; default 3); R: as RetinaNet
  MATCHER.THRESHOLDS, ALLOW_LOW_QUALITY, LABELS   K: bd_rpn_assign_encode.  T: test_faster_rcnn_key[MATCHER.ALLOW_LOW_QUALITY], (all); R: as RetinaNet
  RPN_BOX_REG.MEAN, STD         K: bd_rpn_assign_encode (encode), bd_rpn_proposals (decode).  T: test_faster_rcnn_key (all); kernel level:
                                test_assign_edges_gpu, test_rcnn_ops_gpu
  RCNN_BOX_REG.MEAN, STD        K: bd_rcnn_sample_targets (encode), bd_rcnn_predict (decode).  T: test_faster_rcnn_key (all),
                                test_faster_rcnn_inference_box_reg; kernel level: test_rcnn_ops_gpu, test_postprocess_gpu
  LOSSES.RPN_SMOOTH_L1_BETA, RCNN_SMOOTH_L1_BETA   K: bd_rpn_loss_fwd_bwd, bd_rcnn_loss_fwd_bwd.  T: test_faster_rcnn_key (all), test_rcnn_ops_gpu
  RPN.CHANNELS                  K: rpn_conv width; network shape, fixed by the fixture
  RPN.NUM_SAMPLE_ANCHORS        T: the fixture itself (64, default 256)
  RPN.POSITIVE_ANCHOR_RATIO     K: bd_sample_labels.  T: test_faster_rcnn_key (all), test_rcnn_ops_gpu
  RPN.NMS_THRESHOLD             K: bd_rpn_proposals.  T: test_faster_rcnn_key (all), test_rcnn_ops_gpu
  RPN.TRAIN_/TEST_PREV_NMS_TOPK, TRAIN_/TEST_POST_NMS_TOPK   T: the fixture (300 / 120); R: TEST_POST_NMS_TOPK != TRAIN_POST_NMS_TOPK
  RCNN.NUM_ROIS                 T: the fixture (48, default 512)
  RCNN.FG_RATIO                 K: bd_rcnn_sample_targets.  T: test_faster_rcnn_key (all), test_rcnn_ops_gpu
  RCNN.FG_THRESHOLD, BG_THRESHOLD_HIGH, BG_THRESHOLD_LOW   K: bd_rcnn_sample_targets.  T: test_faster_rcnn_key (all), test_rcnn_ops_gpu (0.6 / 0.4 / 0.1)
  RCNN.IN_FEATURES, RCNN.STRIDES               R: other than the finest FPN levels in order
  ROI_POOLER.METHOD, ROI_POOLER.SIZE           T: test_roi_pool_model_gpu, test_model_gpu (three sizes); R: METHOD not roi_align / roi_pool
"""
import pytest

from tests import config_key_cases as C
from tests import test_model_gpu as T

pytestmark = pytest.mark.gpu

ALL = "all keys together"


def _override(family, case):
    return C.all_together(family) if case == ALL else C.model_override(next(c for c in C.CASES[family] if c[0] == case))


@pytest.mark.parametrize("case", C.gpu_case_ids("retinanet") + [ALL])
def test_retinanet_key(case):
    T.check_retinanet_step(*T._setup("resnet18", 2, (128, 160), overrides=_override("retinanet", case)))


@pytest.mark.parametrize("case", C.gpu_case_ids("fcos") + [ALL])
def test_fcos_key(case):
    T.check_fcos_step(*T.fcos_setup(_override("fcos", case)))


@pytest.mark.parametrize("case", C.gpu_case_ids("atss") + [ALL])
def test_atss_key(case):
    T.check_atss_step(*T.atss_setup(_override("atss", case)))


@pytest.mark.parametrize("case", C.gpu_case_ids("faster_rcnn") + [ALL])
def test_faster_rcnn_key(case):
    T.check_faster_rcnn_step(*T._frcnn_setup(2, (128, 160), overrides=_override("faster_rcnn", case)))


def test_retinanet_inference_box_reg():
    """RetinaNet.inference decodes with BoxCoder(MODEL.BOX_REG): detections against the oracle's, as test_retinanet_inference_matches_oracle."""
    T.check_retinanet_inference(dict(MODEL=dict(BOX_REG=C.CODER_A)))


def test_faster_rcnn_inference_box_reg():
    """Detections decoded with RCNN_BOX_REG (bd_rcnn_predict), as test_faster_rcnn_inference_matches_oracle.  (The helper takes the proposals
    from the HIP run, so RPN_BOX_REG at inference is not its business: bd_rpn_proposals is the training step's kernel too, checked under
    coders A and B by test_rcnn_ops_gpu::test_rpn_proposals and through the config by test_faster_rcnn_key[all keys together].)"""
    T.check_faster_rcnn_inference(dict(MODEL=dict(RCNN_BOX_REG=dict(MEAN=[0.1, -0.2, 0.05, -0.1], STD=[0.2, 0.1, 0.4, 0.3]))))
