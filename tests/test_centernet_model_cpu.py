"""The CenterNet detector without a device: CenterNetConfig against the reference's values (tests/golden/centernet_cfg.json, transcribed
from configs/det_model/centernet_cfg.py), the registry, every check_config refusal, TestTimeCenterPad, the unbuilt transforms and the
parameter names and shapes (tests/golden/centernet_names.json, written from the reference's module tree: models/cls/resnet.py,
layers/head/center_head.py, layers/blocks/deformable.py)."""
import json
import math
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _cfg(shape="A", **model):
    from basedet_amd.configs import CenterNetConfig
    cfg = CenterNetConfig()
    if shape == "A":
        cfg.merge(dict(MODEL=dict(BATCHSIZE=2, WEIGHTS=None, BACKBONE=dict(NAME="resnet18"),
                                  HEAD=dict(DECONV_CHANNEL=[512, 64, 64, 64], IN_CHANNELS=64, TENSOR_DIM=8), OUTPUT_SIZE=(16, 24)),
                       DATA=dict(NUM_CLASSES=3)))
    elif shape == "B":
        cfg.merge(dict(MODEL=dict(BATCHSIZE=1, WEIGHTS=None, HEAD=dict(DECONV_CHANNEL=[2048, 64, 64, 64], MODULATE_DEFORM=False, TENSOR_DIM=8),
                                  OUTPUT_SIZE=(16, 16))))
    cfg.merge(dict(MODEL=model))
    return cfg


def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def test_config_equals_reference_key_for_key():
    from basedet_amd.configs import CenterNetConfig
    want = json.load(open(os.path.join(GOLD, "centernet_cfg.json")))
    cfg = CenterNetConfig()

    def walk(w, have, path):
        for k, v in w.items():
            assert k in have, f"{path}{k} is missing"
            if isinstance(v, dict):
                walk(v, have[k], f"{path}{k}.")
            else:
                assert _plain(have[k]) == v, f"{path}{k}: {have[k]!r} != {v!r}"
    walk(want, cfg, "")
    assert set(cfg.MODEL.HEAD) == set(want["MODEL"]["HEAD"]) and set(cfg.MODEL.LOSS) == set(want["MODEL"]["LOSS"])


def test_registry_resolves_centernet():
    from basedet_amd import models
    from basedet_amd.utils.registry import registers
    assert registers.models.get("CenterNet") is models.CenterNet


@pytest.mark.parametrize("change,key", [
    (dict(WEIGHT_DTYPE="fp8_e4m3"), "MODEL.WEIGHT_DTYPE"),
    (dict(HEAD=dict(DECONV_CHANNEL=[256, 64, 64, 64])), "DECONV_CHANNEL[0]"),
    (dict(HEAD=dict(IN_CHANNELS=128)), "MODEL.HEAD.IN_CHANNELS"),
    (dict(HEAD=dict(DOWN_SCALE=8)), "MODEL.HEAD.DOWN_SCALE"),
    (dict(BACKBONE=dict(NAME="vgg16")), "MODEL.BACKBONE.NAME"),
    (dict(BACKBONE=dict(NORM="GN")), "MODEL.BACKBONE.NORM"),
    (dict(BACKBONE=dict(NORM="BN", FREEZE_AT=2)), "MODEL.BACKBONE.FREEZE_AT"),
    (dict(OUTPUT_SIZE=(16,)), "MODEL.OUTPUT_SIZE"),
    (dict(HEAD=dict(DECONV_KERNEL=[4, 3, 4])), "DECONV_KERNEL"),
])
def test_check_config_refuses(change, key):
    from basedet_amd.models import CenterNet
    with pytest.raises(ValueError) as e:
        CenterNet.check_config(_cfg("A", **change))
    assert key in str(e.value)


def test_check_config_accepts():
    from basedet_amd.models import CenterNet
    CenterNet.check_config(_cfg("A"))
    CenterNet.check_config(_cfg("B"))
    CenterNet.check_config(_cfg("A", BACKBONE=dict(NORM="SyncBN")))
    for fa in (0, 1, 2, 3):
        CenterNet.check_config(_cfg("A", BACKBONE=dict(NORM="FrozenBN", FREEZE_AT=fa)))
    CenterNet.check_config(_cfg("A", HEAD=dict(MODULATE_DEFORM=False)))


def test_check_batch_refuses_output_size_and_gt_slots():
    from basedet_amd.models import CenterNet
    cfg = _cfg("A")
    CenterNet.check_batch(cfg, (64, 96), 8)
    CenterNet.check_batch(cfg, (60, 90), 8)              # pads to 64 x 96
    with pytest.raises(ValueError, match="MODEL.OUTPUT_SIZE"):
        CenterNet.check_batch(cfg, (96, 64), 4)          # (H, W) swapped
    with pytest.raises(ValueError, match="MODEL.HEAD.TENSOR_DIM"):
        CenterNet.check_batch(cfg, (64, 96), 9)


@pytest.mark.parametrize("h,w", [(37, 53), (1, 1), (31, 33), (32, 64), (64, 96), (95, 32)])
def test_test_time_center_pad(h, w):
    from basedet_amd.data.transforms import TestTimeCenterPad
    img = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, 3)).astype(np.uint8)
    th, tw = (h | 31) + 1, (w | 31) + 1
    assert th % 32 == 0 and th > h and tw > w                     # a multiple of 32 grows too
    ph, pw = math.ceil((th - h) / 2), math.ceil((tw - w) / 2)
    want = np.zeros((th, tw, 3))
    want[ph:h + ph, pw:w + pw] = img
    got = TestTimeCenterPad().apply(img)
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)


def test_test_aug_builds_and_train_aug_names_center_affine():
    from basedet_amd.configs import CenterNetConfig
    from basedet_amd.data.transforms import build_transform
    cfg = CenterNetConfig()
    t = build_transform(cfg.TEST.AUG.VALUE, mode="test")
    img, info = t(np.zeros((40, 50, 3), np.uint8))
    assert img.shape == (1, 3, 64, 64) and img.dtype == np.float32
    with pytest.raises(ValueError, match="CenterAffine"):
        build_transform(cfg.AUG.TRAIN_VALUE, mode="train")


@pytest.mark.parametrize("shape", ["A", "B"])
def test_parameter_names_and_shapes(shape):
    from basedet_amd.models import CenterNet
    want = {k: tuple(v) for k, v in json.load(open(os.path.join(GOLD, "centernet_names.json")))[shape]}
    got = CenterNet.param_shapes(_cfg(shape))
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:5]
    assert got == want
    assert not any("bottom_up" in k or ".fc." in k for k in got)


def test_grad_bucket_names():
    """GradBuckets' phase of a name: the neck belongs to the head's bucket, the bare ResNet's names to their layer."""
    from basedet_amd.solver import GradBuckets

    class Arena:
        entries = [("backbone.conv1.weight", (64,), 0, 64), ("backbone.bn1.weight", (64,), 64, 64), ("backbone.layer1.0.conv1.weight", (64,), 128, 64),
                   ("backbone.layer4.1.bn2.bias", (64,), 192, 60), ("upsample.deconv1.dcn.dcn.weight", (64,), 256, 64),
                   ("head.feat_conv.weight", (64,), 320, 10)]

    class Model:
        arena = Arena()
    b = GradBuckets.__new__(GradBuckets)
    b.model = Model()
    assert b._ranges() == {"conv1": (0, 128), "layer1": (128, 192), "layer4": (192, 256), "head": (256, 384)}
