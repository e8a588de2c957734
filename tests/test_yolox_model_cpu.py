"""CPU side of the YOLOX detector (models/yolox.py YOLOX, solver YOLOXSolver / YoloxLR / SyncSizeHook, bd_resize_bilinear_normalize): the
registries, the parameter names against the two golden state fixtures, the refusals of check_config by key, the schedule against values
worked out from the reference's formula (tests/golden/yolox_lr.json), and the new symbol."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gold(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def _cfg(depth=0.33, width=0.5, **model):
    from basedet_amd.configs import YOLOXConfig
    cfg = YOLOXConfig()
    cfg.MODEL.DEPTH_FACTOR, cfg.MODEL.WIDTH_FACTOR = depth, width
    for k, v in model.items():
        cfg.MODEL[k] = v
    return cfg


def test_registries_resolve():
    from basedet_amd import models, solver  # noqa: F401
    from basedet_amd.utils.registry import registers
    assert registers.models.get("YOLOX") is models.YOLOX
    assert registers.solvers.get("YOLOXSolver") is solver.YOLOXSolver
    assert "YOLOX" in models.yolox.__all__


def test_param_shapes_are_the_golden_states_under_their_prefixes():
    """backbone.* at (0.33, 0.5) is yolox_fpn_state.json entry for entry, in order.  yolox_head_state.json was written at width 1.0
    (mid_channels 256): head.* has its names in its order at any width, its shapes at width 1.0, and at 0.5 every channel count halved
    (the predictors' row counts -- K, 4, 1 -- stay)."""
    from basedet_amd.models import YOLOX
    fpn, head = _gold("yolox_fpn_state.json"), _gold("yolox_head_state.json")
    assert (fpn["depth"], fpn["width"]) == (0.33, 0.5)
    got = YOLOX.param_shapes(_cfg(0.33, 0.5))
    back = [[k, list(v)] for k, v in got.items() if k.startswith("backbone.")]
    assert back == [["backbone." + k, v] for k, v in fpn["state"]]
    hd = [[k, list(v)] for k, v in got.items() if k.startswith("head.")]
    assert [k for k, _ in hd] == ["head." + k for k, _ in head["state"]]
    assert len(got) == len(back) + len(hd)
    full = YOLOX.param_shapes(_cfg(0.33, 1.0))
    assert [[k, list(v)] for k, v in full.items() if k.startswith("head.")] == [["head." + k, v] for k, v in head["state"]]
    rows = {"cls_preds": 80, "reg_preds": 4, "obj_preds": 1}
    for (k, v), (_, w) in zip(hd, head["state"]):
        keep = rows.get(k.split(".")[1])
        want = [c if i >= 2 or (i == 0 and keep is not None) else c // 2 for i, c in enumerate(w)]          # (out, in, kh, kw) or (C,)
        assert v == want, k
    assert got["backbone.backbone.stem.conv.weight"] == (32, 12, 3, 3) and got["head.cls_preds.2.weight"] == (80, 128, 1, 1)


def test_check_config_names_the_key():
    from basedet_amd.models import YOLOX
    YOLOX.check_config(_cfg())
    for key, change in (("MODEL.DEPTHWISE", dict(DEPTHWISE=True)), ("MODEL.ACTIVATION", dict(ACTIVATION="relu")),
                        ("MODEL.WEIGHT_DTYPE", dict(WEIGHT_DTYPE="fp8"))):
        with pytest.raises(ValueError, match=re.escape(key)):
            YOLOX.check_config(_cfg(**change))
    cfg = _cfg()
    cfg.MODEL.BACKBONE.NAME = "darknet53"
    with pytest.raises(ValueError, match=r"MODEL\.BACKBONE\.NAME"):
        YOLOX.check_config(cfg)
    for size in ((640, 630), (0, 640), (4096, 4096)):
        cfg = _cfg()
        cfg.AUG.TRAIN_SETTING.INPUT_SIZE = size
        with pytest.raises(ValueError, match=r"AUG\.TRAIN_SETTING\.INPUT_SIZE"):
            YOLOX.check_config(cfg)
    with pytest.raises(ValueError, match=r"WIDTH_FACTOR"):          # channel counts that are no multiple of 8
        YOLOX.check_config(_cfg(0.33, 0.0625))
    # the constructor checks before it touches the device (there is none here)
    with pytest.raises(ValueError, match=r"MODEL\.DEPTHWISE"):
        YOLOX(_cfg(DEPTHWISE=True))
    # target_size: multiples of 32, at most 64 x 64 cells at stride 32
    m = object.__new__(YOLOX)
    m.target_size = [96, 64]
    assert m.target_size == (96, 64)
    for bad in ((100, 64), (2080, 2080), (64,), 64):
        with pytest.raises(ValueError, match="target_size"):
            m.target_size = bad
    assert m.target_size == (96, 64)


def test_yolox_lr_matches_the_formula_fixture():
    from basedet_amd.solver import YoloxLR
    g = _gold("yolox_lr.json")
    assert "not recorded from a run" in g["note"]
    cfg = _cfg()
    s = cfg.SOLVER
    s.MIN_LR_RATIO, s.WARM_EPOCH, s.MAX_EPOCH, s.NUM_IMAGE_PER_EPOCH = g["min_lr_ratio"], g["warm_epoch"], g["max_epoch"], g["num_image_per_epoch"]
    cfg.MODEL.BATCHSIZE, cfg.AUG.TRAIN_SETTING.NO_AUG_EPOCH = g["batchsize"], g["no_aug_epoch"]

    class Opt:
        param_groups = [dict(lr=g["lr"], weight_decay=5e-4), dict(lr=g["lr"], weight_decay=0.0)]
    sched = YoloxLR(Opt, cfg)
    assert sched.max_iter == g["max_iter"] and len(g["points"]) >= 12
    assert {p["phase"] for p in g["points"]} == {"warmup", "cosine", "no_aug"}
    for p in g["points"]:
        got = sched.lr_at(p["epoch"], p["iter"])
        assert abs(got - p["lr"]) <= 1e-12 * abs(p["lr"]), (p, got)
    sched.step(3, 900)
    assert Opt.param_groups[0]["lr"] == Opt.param_groups[1]["lr"] == sched.lr_at(3, 900)          # both groups follow one rate


def test_trainer_picks_the_schedule_by_hook_list():
    """HOOKS.BUILDER_NAME == "YOLOXHookList" selects YoloxLR and the size hook (off when MULTISCALE_RANGE is empty); seeded draws repeat."""
    from basedet_amd.solver import SyncSizeHook

    class Model:
        training, device, target_size = True, None, (640, 640)
    cfg = _cfg()
    a, b = (SyncSizeHook.build(cfg, Model(), seed=3) for _ in range(2))
    assert a.sizes == [32 * x for x in range(14, 27)] and a.change_iter == 10
    draws = []
    for hook in (a, b):
        seen = []
        for it in range(1, 61):
            hook.before_iter(1, it, 1000)
            seen.append(hook.model.target_size)
        draws.append(seen)
    assert draws[0] == draws[1] and seen[8] == (640, 640) and len(set(seen)) > 2
    assert all(s[0] == s[1] and s[0] in a.sizes for s in seen[9:])
    cfg.AUG.TRAIN_SETTING.MULTISCALE_RANGE = ()
    assert SyncSizeHook.build(cfg, Model()) is None


def test_new_symbol_in_library_header_binding_and_abi():
    from basedet_amd import _lib, build, ops
    name, nargs = "bd_resize_bilinear_normalize", 12
    hdr = open(os.path.join(ROOT, "include", "basedet_hip.h")).read()
    src = open(os.path.join(ROOT, "basedet_amd", "csrc", "image_resize.hip")).read()
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == nargs
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert f'extern "C" int {name}(' in src and hasattr(ops, "resize_bilinear_normalize")
    assert _lib.ABI_VERSION == 118
    import ctypes
    raw = ctypes.CDLL(build.build(force=False, verbose=False))
    assert hasattr(raw, name)
    assert int(_lib.load().bd_version()) == 118
