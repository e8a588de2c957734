"""The fixtures of test_config_keys_gpu.py can feel every key they move, and the constructors refuse what the HIP path does not implement.

For every per-key case (tests/config_key_cases.py) the ORACLE runs at the default and at the changed value on the GPU test's own batch, and
the quantity the GPU test compares has to move by at least ten times what that comparison tolerates -- otherwise a HIP path that ignored
the key would pass.  This is a condition on the inputs (no HIP code runs here); the ratios are printed (pytest -s)."""
import numpy as np
import pytest

from tests import config_key_cases as C

LOSS_TOL = 2e-2          # every loss comparison of tests/test_model_gpu.py's training-step checks: 2e-2 relative
FLOAT_TOL = 1e-3         # proposals are compared at 1e-3 px
MIN_RATIO = 10.0
_default = {}


def _fixture(family, overrides=None):
    from tests import test_model_gpu as T
    if family == "retinanet":
        return T._setup("resnet18", 2, (128, 160), overrides=overrides)
    if family == "fcos":
        return T.fcos_setup(overrides)
    if family == "atss":
        return T.atss_setup(overrides)
    return T._frcnn_setup(2, (128, 160), overrides=overrides)


def _oracle_run(family, overrides=None):
    """Losses and target tensors of the plain fp32 oracle, and the parameter table's shapes."""
    from basedet_amd.models import params as P
    from oracle.model import Oracle
    cfg, params, batch = _fixture(family, overrides)
    orc = Oracle(params, P.oracle_arch(cfg))
    if family == "retinanet":
        losses, aux = orc.retinanet_losses(batch)
    elif family in ("fcos", "atss"):
        losses, aux = orc.fcos_losses(batch)
    else:
        A = len(cfg.MODEL.ANCHOR.SCALES[0]) * len(cfg.MODEL.ANCHOR.RATIOS[0])
        a_total = A * sum(-(-128 // s) * -(-160 // s) for s in cfg.MODEL.FPN.STRIDES)
        width = cfg.MODEL.RPN.TRAIN_POST_NMS_TOPK + batch["gt_boxes"].shape[1]
        rng = np.random.default_rng(5)                       # the draws of check_faster_rcnn_step
        keys = dict(rpn_pos=rng.random((2, a_total), dtype=np.float32), rpn_neg=rng.random((2, a_total), dtype=np.float32),
                    rcnn_fg=rng.random((2, width), dtype=np.float32), rcnn_bg=rng.random((2, width), dtype=np.float32))
        losses, aux = orc.faster_rcnn_losses(batch, keys)
        aux["rois"] = np.concatenate(aux["rois"], 0)
    out = {k: float(v.detach()) for k, v in losses.items()}
    for k in ("labels", "rpn_labels", "s_labels", "rois"):
        if k in aux:
            out[k] = np.asarray(aux[k])
    out["params"] = {k: v.shape for k, v in params.items()}
    return out


def _movement(ref, got, witness):
    """(figure, what it measures).  A loss: relative movement / the 2e-2 the GPU comparison allows.  A tensor compared exactly (labels)
    or at 1e-3 (proposals): the NUMBER of entries that move (by >= 10 x 1e-3 for the floats) -- one would fail the GPU comparison, ten
    are asked for.  A changed parameter table or another number of proposals / samples cannot be bound or compared at all: inf."""
    if witness == "params":
        return (float("inf") if ref["params"] != got["params"] else 0.0), "parameter table differs"
    a, b = ref[witness], got[witness]
    if isinstance(a, float):
        return abs(b - a) / abs(a) / LOSS_TOL, "x the 2e-2 relative tolerance"
    if a.shape != b.shape:
        return float("inf"), "another number of rows"
    if a.dtype.kind == "f":
        fin = np.isfinite(a) & np.isfinite(b)
        return float((np.abs(a - b)[fin] > MIN_RATIO * FLOAT_TOL).sum()), "entries moved by >= 10 x 1e-3 (1 fails the comparison)"
    return float((a != b).sum()), "entries changed (1 fails the exact comparison)"


def _best_movement(ref, got):
    """The compared quantity that moves most, for the leave-one-out of the all-together fixtures."""
    names = ["params"] + [k for k in ref if k != "params"]
    return max(((*_movement(ref, got, k), k) for k in names), key=lambda t: t[0])


@pytest.mark.parametrize("family,case", [(f, c) for f in C.CASES for c in C.CASES[f]], ids=[f"{f}-{c[0]}" for f in C.CASES for c in C.CASES[f]])
def test_fixture_feels_the_key(family, case):
    if family not in _default:
        _default[family] = _oracle_run(family)
    got = _oracle_run(family, C.model_override(case))
    ratio, unit = _movement(_default[family], got, case[2])
    print(f"{family} {case[0]}: {case[2]}: {ratio:.3g} {unit}")
    assert ratio >= MIN_RATIO, (family, case[0], case[2], ratio)


_all = {}


@pytest.mark.parametrize("family,name", [(f, n) for f in C.CASES for n in C.all_together_ids(f)],
                         ids=[f"{f}-{n}" for f in C.CASES for n in C.all_together_ids(f)])
def test_all_together_fixture_feels_each_key(family, name):
    """Leave one out: the all-keys-together step with this key back at its default differs from the step with every key moved, in a quantity
    the GPU test compares, by ten times the tolerance -- so that step alone would notice this key being ignored."""
    if family not in _all:
        _all[family] = _oracle_run(family, C.all_together(family))
    got = _oracle_run(family, C.all_together(family, without=name))
    ratio, unit, witness = _best_movement(_all[family], got)
    print(f"{family} all-together without {name}: {witness}: {ratio:.3g} {unit}")
    assert ratio >= MIN_RATIO, (family, name, witness, ratio)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _cfg(name):
    from basedet_amd import configs as K
    return dict(RetinaNet=K.retinanet_r18_config, FreeAnchor=K.FreeAnchorConfig, FCOS=K.FCOSConfig, ATSS=K.ATSSConfig, OTA=K.OTAConfig,
                FasterRCNN=K.FasterRCNNConfig)[name]()


def _model_cls(name):
    from basedet_amd import models as M
    return getattr(M, name)


@pytest.mark.parametrize("name", ["RetinaNet", "FreeAnchor", "FCOS", "ATSS", "OTA", "FasterRCNN"])
def test_default_config_is_accepted(name):
    _model_cls(name).check_config(_cfg(name))


REFUSED = [
    ("RetinaNet", dict(MATCHER=dict(LABELS=[0, 1, 1])), "MODEL.MATCHER.LABELS"),
    ("RetinaNet", dict(MATCHER=dict(LABELS=[-1, 0, 1])), "MODEL.MATCHER.LABELS"),
    ("FasterRCNN", dict(MATCHER=dict(LABELS=[0, 0, 1])), "MODEL.MATCHER.LABELS"),
    ("RetinaNet", dict(MATCHER=dict(THRESHOLDS=[0.5])), "MODEL.MATCHER.THRESHOLDS"),
    ("FasterRCNN", dict(MATCHER=dict(THRESHOLDS=[0.3, 0.5, 0.7])), "MODEL.MATCHER.THRESHOLDS"),
    ("RetinaNet", dict(ANCHOR=dict(SCALES=[[32, 40], [64], [128], [256], [512]])), "MODEL.ANCHOR.SCALES"),
    ("RetinaNet", dict(ANCHOR=dict(SCALES=[[32], [64]])), "MODEL.ANCHOR.SCALES"),
    ("FasterRCNN", dict(ANCHOR=dict(SCALES=[[32], [64], [128], [256], [512, 640]])), "MODEL.ANCHOR.SCALES"),
    ("RetinaNet", dict(ANCHOR=dict(RATIOS=[[0.5, 1, 2]] * 5)), "MODEL.ANCHOR.RATIOS"),
    ("FasterRCNN", dict(ANCHOR=dict(RATIOS=[[0.5, 1, 2], [1]])), "MODEL.ANCHOR.RATIOS"),
    ("FreeAnchor", dict(ANCHOR=dict(RATIOS=[[0.5, 1, 2], [1]])), "MODEL.ANCHOR.RATIOS"),
    ("FCOS", dict(ANCHOR=dict(NUM_ANCHORS=2)), "MODEL.ANCHOR.NUM_ANCHORS"),
    ("FCOS", dict(FPN=dict(OUT_CHANNELS=128)), "MODEL.FPN.OUT_CHANNELS"),
    ("FCOS", dict(HEAD=dict(OBJECT_SIZES_OF_INTEREST=[[-1, 64], [64, float("inf")]])), "MODEL.HEAD.OBJECT_SIZES_OF_INTEREST"),
    ("ATSS", dict(ANCHOR=dict(TOPK=17)), "MODEL.ANCHOR.TOPK"),
    ("ATSS", dict(ANCHOR=dict(TOPK=0)), "MODEL.ANCHOR.TOPK"),
    ("FasterRCNN", dict(RCNN=dict(IN_FEATURES=["p3", "p4", "p5"], STRIDES=[8, 16, 32])), "MODEL.RCNN.IN_FEATURES"),
    ("FasterRCNN", dict(RPN=dict(TEST_POST_NMS_TOPK=500)), "MODEL.RPN.TEST_POST_NMS_TOPK"),
    ("FasterRCNN", dict(ROI_POOLER=dict(METHOD="roi_warp")), "MODEL.ROI_POOLER.METHOD"),
    # live norms (FPNDetector.check_config): a value that is no norm of the reference's, a backbone norm above frozen convolutions,
    # fp8 weights under either key, a FREEZE_AT that is no stage count
    ("RetinaNet", dict(BACKBONE=dict(NORM="GN", FREEZE_AT=0)), "MODEL.BACKBONE.NORM"),
    ("FCOS", dict(BACKBONE=dict(NORM=None, FREEZE_AT=0)), "MODEL.BACKBONE.NORM"),
    ("RetinaNet", dict(BACKBONE=dict(NORM="BN", FREEZE_AT=1)), "MODEL.BACKBONE.NORM"),
    ("FasterRCNN", dict(BACKBONE=dict(NORM="SyncBN", FREEZE_AT=2)), "MODEL.BACKBONE.NORM"),
    ("RetinaNet", dict(WEIGHT_DTYPE="fp8_e4m3", BACKBONE=dict(NORM="BN", FREEZE_AT=0)), "MODEL.BACKBONE.NORM"),
    ("RetinaNet", dict(WEIGHT_DTYPE="fp8_e4m3", FPN=dict(NORM="BN")), "MODEL.FPN.NORM"),
    ("OTA", dict(FPN=dict(NORM="GN")), "MODEL.FPN.NORM"),
    ("FasterRCNN", dict(FPN=dict(NORM="FrozenBN")), "MODEL.FPN.NORM"),
    ("RetinaNet", dict(BACKBONE=dict(FREEZE_AT=-1)), "MODEL.BACKBONE.FREEZE_AT"),
    ("ATSS", dict(BACKBONE=dict(FREEZE_AT=True)), "MODEL.BACKBONE.FREEZE_AT"),
]

LIVE_NORMS = [dict(BACKBONE=dict(NORM="BN", FREEZE_AT=0)), dict(BACKBONE=dict(NORM="SyncBN", FREEZE_AT=0)), dict(FPN=dict(NORM="BN")),
              dict(FPN=dict(NORM="SyncBN")), dict(BACKBONE=dict(NORM="BN", FREEZE_AT=0), FPN=dict(NORM="BN")),
              dict(BACKBONE=dict(NORM="FrozenBN", FREEZE_AT=0)), dict(BACKBONE=dict(NORM="FrozenBN", FREEZE_AT=1), FPN=dict(NORM=None))]


@pytest.mark.parametrize("name", ["RetinaNet", "FreeAnchor", "FCOS", "ATSS", "OTA", "FasterRCNN"])
@pytest.mark.parametrize("override", LIVE_NORMS, ids=[str(i) for i in range(len(LIVE_NORMS))])
def test_live_norm_values_are_accepted(name, override):
    """MODEL.BACKBONE.NORM / MODEL.FPN.NORM = "BN", and "SyncBN" at world size 1 (this process), by every detector; the backbone norm at
    FREEZE_AT = 0 only."""
    from basedet_amd import comm
    assert comm.world_size() == 1
    cfg = _cfg(name)
    cfg.merge(dict(MODEL=override))
    _model_cls(name).check_config(cfg)


@pytest.mark.parametrize("name,override,key", REFUSED, ids=[f"{n}-{k}-{i}" for i, (n, _, k) in enumerate(REFUSED)])
def test_unimplemented_value_is_refused(name, override, key):
    cfg = _cfg(name)
    cfg.merge(dict(MODEL=override))
    with pytest.raises(ValueError, match=key.replace(".", r"\.") + r" = .* is not supported"):
        _model_cls(name).check_config(cfg)


def test_freeanchor_does_not_read_the_matcher():
    """free_anchor.py:20-142 never calls the matcher RetinaNet's constructor builds: any MATCHER.LABELS trains the same network."""
    cfg = _cfg("FreeAnchor")
    cfg.merge(dict(MODEL=dict(MATCHER=dict(LABELS=[0, 1, 1]))))
    _model_cls("FreeAnchor").check_config(cfg)
