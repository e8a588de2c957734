"""MODEL.BACKBONE.FREEZE_AT = 0, 1, 2 on the CPU: check_config, the parameter table and the parameter arena's trainable set
(solver/default_solver.py:83-94 drops bottom_up.conv1 at >= 1 and bottom_up.layer1 at >= 2).  No kernel runs and the HIP library is
never loaded: the packed bf16 copies, the only thing construction launches kernels for, are skipped."""
import numpy as np
import pytest

MODELS = [("RetinaNet", "init_retinanet_params"), ("FCOS", "init_fcos_params"), ("FasterRCNN", "init_faster_rcnn_params")]


def _build(model, init, freeze_at, monkeypatch, backbone=None):
    import basedet_amd.models as M
    from basedet_amd import _lib, configs, ops
    from basedet_amd.models import params as P
    from basedet_amd.models.fpn_base import FPNDetector

    def no_library(*a, **k):
        raise AssertionError("the HIP library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(ops, "L", no_library)
    monkeypatch.setattr(FPNDetector, "repack_weights", lambda self: None)
    cfg = getattr(configs, model + "Config")()
    cfg.MODEL.BACKBONE.FREEZE_AT = freeze_at
    if backbone == "resnet18":
        chans = [64 * 2 ** (int(f[-1]) - 2) for f in cfg.MODEL.BACKBONE.OUT_FEATURES]              # res2 .. res5 of a BasicBlock net
        cfg.merge(dict(MODEL=dict(BACKBONE=dict(NAME="resnet18", OUT_FEATURE_CHANNELS=chans), FPN=dict(TOP_BLOCK_IN_CHANNELS=512))))
    params = getattr(P, init)(cfg, 0)
    return cfg, params, getattr(M, model)(cfg, params=params, device="cpu")


@pytest.mark.parametrize("freeze_at", [0, 1, 2])
@pytest.mark.parametrize("model,init", MODELS)
def test_arena_holds_exactly_the_trainable_names(model, init, freeze_at, monkeypatch):
    from basedet_amd.models import params as P
    cfg, params, m = _build(model, init, freeze_at, monkeypatch)
    names = P.trainable_names(params, freeze_at)
    stem = "backbone.bottom_up.conv1.weight"
    assert (stem in names) == (freeze_at == 0)
    assert any("bottom_up.layer1." in n for n in names) == (freeze_at <= 1)
    assert sorted(m.state_dict_trainable_names()) == sorted(names)
    # every arena entry belongs to one reference parameter (fused predictors hold several): the stem's is its own, OHWI like every master
    arena = {e[0]: e[1] for e in m.arena.entries}
    assert (stem in arena) == (freeze_at == 0)
    if freeze_at == 0:
        assert arena[stem] == (64, 7, 7, 3) and m.arena.entries[0][0] == stem
        assert m.stem_w.data_ptr() == m.arena.view("w", 0).data_ptr()
    assert not any("bottom_up.layer1." in k for k in arena) == (freeze_at >= 2)
    # state_dict: the reference's names and shapes at every value, conv1.weight included
    sd = m.state_dict()
    assert set(sd) == set(params)
    for k, v in params.items():
        assert sd[k].shape == v.shape and np.array_equal(sd[k], v), k
    # FUSE_STEM_POOL is ignored while the stem trains; layer1 leaves the fused frozen-block launch as soon as it trains
    assert m.fuse_stem_pool == (freeze_at >= 1)
    assert all(b["trainable"] == (b["layer"] > 1 or freeze_at <= 1) for b in m.blocks)


@pytest.mark.parametrize("model,init", MODELS)
def test_resnet18_table(model, init, monkeypatch):
    """BasicBlock backbones: layer1.0 has no downsample convolution (the identity shortcut carries the gradient to the pool output)."""
    from basedet_amd.models import params as P
    cfg, params, m = _build(model, init, 0, monkeypatch, backbone="resnet18")
    assert sorted(m.state_dict_trainable_names()) == sorted(P.trainable_names(params, 0))
    assert m.blocks[0]["kind"] == "basic" and m.blocks[0]["ds"] is None


@pytest.mark.parametrize("bad", [-1, 1.5, "0", None, True])
def test_check_config_refuses_what_is_not_a_count(bad, monkeypatch):
    import basedet_amd.models as M
    from basedet_amd import _lib, configs, ops

    def no_library(*a, **k):
        raise AssertionError("the HIP library was reached before the config check")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(ops, "L", no_library)
    cfg = configs.RetinaNetConfig()
    cfg.MODEL.BACKBONE.FREEZE_AT = bad
    with pytest.raises(ValueError) as ei:
        M.RetinaNet(cfg, params={}, device="cpu")
    assert "MODEL.BACKBONE.FREEZE_AT" in str(ei.value)


@pytest.mark.parametrize("freeze_at", [0, 1, 2, 5])
def test_check_config_accepts(freeze_at):
    from basedet_amd import configs
    from basedet_amd.models.fpn_base import FPNDetector
    cfg = configs.RetinaNetConfig()
    cfg.MODEL.BACKBONE.FREEZE_AT = freeze_at
    FPNDetector.check_config(cfg)
