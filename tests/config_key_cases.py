"""The per-key cases shared by test_config_keys_gpu.py (HIP step against the oracle) and test_config_keys_cpu.py (the oracle at the default
against the oracle at the changed value: the fixture must feel the key).

CASES[family] is a list of (id, MODEL override, witness).  The witness names what the GPU comparison would catch if the key were ignored:
  * a loss name      -- compared at 2e-2 relative on the GPU; the CPU test wants it to move by >= 10 x 2e-2;
  * "labels" / "rpn_labels" / "s_labels" / "rois" (the proposals of every image, stacked) -- compared exactly (or at 1e-3) on the GPU; the CPU test wants >= 10
    entries to move (by >= 10 x 1e-3 for the float ones);
  * "params"         -- the key changes the parameter table (names or shapes): a model that ignored it could not bind the parameters.
"""
import copy

# box coders (structures/boxcoder.py) as (mean, std), shared with the kernel-level tests: the identity, a non-zero mean with the usual
# stds, and four different stds (a swapped component shows)
BOX_CODER_0 = ((0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0))
BOX_CODER_A = ((0.1, -0.2, 0.05, -0.1), (0.1, 0.1, 0.2, 0.2))
BOX_CODER_B = ((0.0, 0.0, 0.0, 0.0), (0.5, 0.25, 2.0, 1.0))
CODER_A = dict(MEAN=list(BOX_CODER_A[0]), STD=list(BOX_CODER_A[1]))
CODER_B = dict(MEAN=list(BOX_CODER_B[0]), STD=list(BOX_CODER_B[1]))
TWO_SCALES = [[x, x * 2 ** 0.5] for x in [32, 64, 128, 256, 512]]                # A = 2 x 3 = 6 (RetinaNet default 9)
SOI_OVERLAP = [[-1, 96], [48, 160], [96, 320], [256, 512], [512, float("inf")]]  # overlapping ranges: a box is "cared" on two levels
SOI_EMPTY = [[-1, 64], [64, 64], [64, 256], [256, 512], [512, float("inf")]]     # level 1 cares about max(ltrb) == 64 only

CASES = {
    "retinanet": [
        ("BOX_REG", dict(BOX_REG=CODER_A), "reg_loss"),
        ("BOX_REG.STD4", dict(BOX_REG=CODER_B), "reg_loss"),
        ("MATCHER.THRESHOLDS", dict(MATCHER=dict(THRESHOLDS=[0.3, 0.6])), "labels"),
        ("MATCHER.ALLOW_LOW_QUALITY", dict(MATCHER=dict(ALLOW_LOW_QUALITY=False)), "labels"),
        ("LOSSES.SMOOTH_L1_BETA", dict(LOSSES=dict(SMOOTH_L1_BETA=1.0)), "reg_loss"),
        ("LOSSES.REG_LOSS_WEIGHT", dict(LOSSES=dict(REG_LOSS_WEIGHT=0.5)), "reg_loss"),
        ("LOSSES.FOCAL_LOSS_ALPHA", dict(LOSSES=dict(FOCAL_LOSS_ALPHA=0.5)), "cls_loss"),
        ("LOSSES.FOCAL_LOSS_GAMMA", dict(LOSSES=dict(FOCAL_LOSS_GAMMA=0.5)), "cls_loss"),      # the `general` focal kernel
        ("HEAD.NUM_CONVS", dict(HEAD=dict(NUM_CONVS=2)), "params"),
        ("HEAD.CLS_PRIOR_PROB", dict(HEAD=dict(CLS_PRIOR_PROB=0.2)), "cls_loss"),
        ("ANCHOR.SCALES", dict(ANCHOR=dict(SCALES=TWO_SCALES)), "params"),
        ("ANCHOR.RATIOS", dict(ANCHOR=dict(RATIOS=[[0.5, 2.0]])), "params"),
        ("ANCHOR.OFFSET", dict(ANCHOR=dict(OFFSET=0.0)), "labels"),
    ],
    "fcos": [
        ("LOSSES.FOCAL_LOSS_ALPHA", dict(LOSSES=dict(FOCAL_LOSS_ALPHA=0.5)), "cls_loss"),
        ("LOSSES.FOCAL_LOSS_GAMMA", dict(LOSSES=dict(FOCAL_LOSS_GAMMA=0.5)), "cls_loss"),
        ("LOSSES.REG_LOSS_WEIGHT", dict(LOSSES=dict(REG_LOSS_WEIGHT=2.0)), "reg_loss"),
        ("HEAD.CENTER_SAMPLING_RADIUS=0", dict(HEAD=dict(CENTER_SAMPLING_RADIUS=0.0)), "labels"),      # the in-box branch
        ("HEAD.CENTER_SAMPLING_RADIUS=0.5", dict(HEAD=dict(CENTER_SAMPLING_RADIUS=0.5)), "labels"),
        ("HEAD.OBJECT_SIZES_OF_INTEREST.overlap", dict(HEAD=dict(OBJECT_SIZES_OF_INTEREST=SOI_OVERLAP)), "labels"),
        ("HEAD.OBJECT_SIZES_OF_INTEREST.empty", dict(HEAD=dict(OBJECT_SIZES_OF_INTEREST=SOI_EMPTY)), "labels"),
        ("HEAD.NUM_CONVS", dict(HEAD=dict(NUM_CONVS=2)), "params"),
        ("HEAD.CLS_PRIOR_PROB", dict(HEAD=dict(CLS_PRIOR_PROB=0.2)), "cls_loss"),
        ("ANCHOR.OFFSET", dict(ANCHOR=dict(OFFSET=0.0)), "labels"),
    ],
    "atss": [
        ("ANCHOR.TOPK=3", dict(ANCHOR=dict(TOPK=3)), "labels"),
        ("ANCHOR.TOPK=16", dict(ANCHOR=dict(TOPK=16)), "labels"),            # the kernel's limit; more than the 6 and 2 points of the two coarsest levels
        ("ANCHOR.SCALE", dict(ANCHOR=dict(SCALE=4)), "labels"),
    ],
    "faster_rcnn": [
        ("LOSSES.RPN_SMOOTH_L1_BETA", dict(LOSSES=dict(RPN_SMOOTH_L1_BETA=1.0)), "rpn_reg_loss"),
        ("LOSSES.RCNN_SMOOTH_L1_BETA", dict(LOSSES=dict(RCNN_SMOOTH_L1_BETA=3.0)), "rcnn_reg_loss"),
        ("MATCHER.THRESHOLDS", dict(MATCHER=dict(THRESHOLDS=[0.2, 0.5])), "rpn_labels"),
        ("MATCHER.ALLOW_LOW_QUALITY", dict(MATCHER=dict(ALLOW_LOW_QUALITY=False)), "rpn_labels"),
        ("ANCHOR.RATIOS", dict(ANCHOR=dict(RATIOS=[[0.5, 2.0]])), "params"),                         # A = 2 (default 3)
        ("ANCHOR.SCALES", dict(ANCHOR=dict(SCALES=[[x, 1.5 * x] for x in [32, 64, 128, 256, 512]])), "params"),   # A = 6
        ("ANCHOR.OFFSET", dict(ANCHOR=dict(OFFSET=0.0)), "rpn_labels"),
        ("RPN.POSITIVE_ANCHOR_RATIO", dict(RPN=dict(POSITIVE_ANCHOR_RATIO=0.125)), "rpn_labels"),
        ("RPN.NMS_THRESHOLD", dict(RPN=dict(NMS_THRESHOLD=0.4)), "rois"),
        ("RCNN.FG_RATIO", dict(RCNN=dict(FG_RATIO=0.0625)), "s_labels"),
        ("RCNN.THRESHOLDS", dict(RCNN=dict(FG_THRESHOLD=0.6, BG_THRESHOLD_HIGH=0.4, BG_THRESHOLD_LOW=0.1)), "s_labels"),
        ("RPN_BOX_REG", dict(RPN_BOX_REG=CODER_A), "rpn_reg_loss"),
        # larger stds than the default (0.1, 0.1, 0.2, 0.2): the targets shrink, so the absolute 1e-3 of the s_targets comparison stays inside
        # its derivation (RoI coordinates at 1e-3 px, divided by std)
        ("RCNN_BOX_REG", dict(RCNN_BOX_REG=dict(MEAN=[0.1, -0.2, 0.05, -0.1], STD=[0.2, 0.1, 0.4, 0.3])), "rcnn_reg_loss"),
    ],
}


# Per-key cases left out of the GPU module to keep it within the time of tests/test_model_gpu.py.  Either the kernel that consumes the key
# is already told apart at non-default values by a kernel-level test (named on the right), or the key changes the parameter table, which
# no step can bind by halves.  The family's all-keys-together step carries every one of these values from the config to its kernel, and
# test_config_keys_cpu.py shows (leave one out) that this step feels each of them.
KERNEL_LEVEL = {
    "retinanet": {"BOX_REG.STD4": "test_assign_edges_gpu (coder B)", "MATCHER.THRESHOLDS": "test_assign_edges_gpu (0.3 / 0.6, 0.3 / 0.7)",
                  "LOSSES.SMOOTH_L1_BETA": "test_boxops_gpu::test_focal_and_l1_losses (0.11)",
                  "LOSSES.FOCAL_LOSS_ALPHA": "test_boxops_gpu::test_focal_and_l1_losses (-1)",
                  "LOSSES.FOCAL_LOSS_GAMMA": "test_boxops_gpu::test_focal_and_l1_losses (1.5)", "ANCHOR.RATIOS": "parameter table (A)", "ANCHOR.SCALES": "parameter table (A)",
                  "HEAD.NUM_CONVS": "parameter table"},
    "fcos": {"HEAD.NUM_CONVS": "parameter table", "LOSSES.FOCAL_LOSS_ALPHA": "test_boxops_gpu::test_focal_and_l1_losses", "LOSSES.FOCAL_LOSS_GAMMA": "test_boxops_gpu::test_focal_and_l1_losses",
             "HEAD.CENTER_SAMPLING_RADIUS=0": "test_assign_edges_gpu", "HEAD.CENTER_SAMPLING_RADIUS=0.5": "test_assign_edges_gpu",
             "HEAD.OBJECT_SIZES_OF_INTEREST.overlap": "test_assign_edges_gpu", "HEAD.OBJECT_SIZES_OF_INTEREST.empty": "test_assign_edges_gpu"},
    "atss": {"ANCHOR.TOPK=3": "test_boxops_gpu::test_atss_assign_bit_exact", "ANCHOR.TOPK=16": "test_boxops_gpu::test_atss_assign_bit_exact",
             "ANCHOR.SCALE": "test_boxops_gpu::test_atss_assign_bit_exact"},
    "faster_rcnn": {"LOSSES.RPN_SMOOTH_L1_BETA": "test_rcnn_ops_gpu::test_rpn_loss (0.5)", "LOSSES.RCNN_SMOOTH_L1_BETA": "test_rcnn_ops_gpu::test_rcnn_loss (1.0)",
                    "MATCHER.THRESHOLDS": "test_assign_edges_gpu (retina_assign_encode shares the matcher code)",
                    "ANCHOR.SCALES": "parameter table (A)", "ANCHOR.RATIOS": "parameter table (A)",
                    "RPN.POSITIVE_ANCHOR_RATIO": "test_rcnn_ops_gpu::test_rpn_targets_and_sampling (0.25, 1.0)",
                    "RPN.NMS_THRESHOLD": "test_rcnn_ops_gpu::test_rpn_proposals (0.5, 0.9)", "RCNN.FG_RATIO": "test_rcnn_ops_gpu::test_rcnn_sample_targets (0, 1)",
                    "RCNN.THRESHOLDS": "test_rcnn_ops_gpu::test_rcnn_sample_targets (0.6 / 0.4 / 0.1)",
                    "RPN_BOX_REG": "test_rcnn_ops_gpu::test_rpn_proposals, test_rpn_targets_and_sampling (coders A, B)",
                    "RCNN_BOX_REG": "test_rcnn_ops_gpu::test_rcnn_sample_targets, test_postprocess_gpu::test_rcnn_predict (coders A, B)"},
}


def model_override(case):
    return dict(MODEL=copy.deepcopy(case[1]))


# Where a key has two cases, the one that stays out of the all-keys-together step
ALL_SKIP = {"BOX_REG.STD4", "HEAD.CENTER_SAMPLING_RADIUS=0.5", "HEAD.OBJECT_SIZES_OF_INTEREST.empty", "ANCHOR.TOPK=3"}


def all_together(family, without=None):
    """Every key of the family moved at once; `without` names one case whose key stays at its default (the leave-one-out of
    test_config_keys_cpu.py: the all-together fixture has to feel every single key)."""
    out = {}

    def merge(dst, src):
        for k, v in src.items():
            if isinstance(v, dict) and isinstance(dst.get(k), dict):
                merge(dst[k], v)
            else:
                dst[k] = copy.deepcopy(v)

    for name, ov, _ in CASES[family]:
        if name not in ALL_SKIP and name != without:
            merge(out, ov)
    return dict(MODEL=out)


def all_together_ids(family):
    return [c[0] for c in CASES[family] if c[0] not in ALL_SKIP]


def gpu_case_ids(family):
    return [c[0] for c in CASES[family] if c[0] not in KERNEL_LEVEL[family]]
