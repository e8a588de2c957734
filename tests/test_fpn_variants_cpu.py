"""MODEL.FPN.UPSAMPLE = "deconv" parameters (fpn_backbone.py:92-103) and the loud refusal of the config variants this build does not
implement (CPU: no kernel runs, the HIP library is never loaded)."""
import math
import numpy as np
import pytest


def _cfgs():
    from basedet_amd.configs import FCOSConfig, RetinaNetConfig, retinanet_r18_config
    return {"retinanet": (RetinaNetConfig, "init_retinanet_params"), "retinanet_r18": (retinanet_r18_config, "init_retinanet_params"),
            "fcos": (FCOSConfig, "init_fcos_params")}


@pytest.mark.parametrize("name", ["retinanet", "retinanet_r18", "fcos"])
@pytest.mark.parametrize("seed", [0, 3])
def test_deconv_config_adds_exactly_the_two_upsample_weights(name, seed):
    from basedet_amd.models import params as P
    make, init = _cfgs()[name]
    base = getattr(P, init)(make(), seed)
    cfg = make()
    cfg.MODEL.FPN.UPSAMPLE = "deconv"
    got = getattr(P, init)(cfg, seed)
    extra = sorted(set(got) - set(base))
    assert extra == ["backbone.fpn_upsample4.weight", "backbone.fpn_upsample5.weight"]
    assert set(base) <= set(got)
    for k in base:
        assert np.array_equal(base[k], got[k]), k
    C = cfg.MODEL.FPN.OUT_CHANNELS
    want = math.sqrt(2.0 / (16 * C))
    for k in extra:
        w = got[k]
        assert w.shape == (C, C, 4, 4) and w.dtype == np.float32
        assert abs(float(w.std()) - want) / want < 0.05, (k, float(w.std()), want)
    names = P.trainable_names(got, cfg.MODEL.BACKBONE.FREEZE_AT)
    assert all(k in names for k in extra)
    assert P.oracle_arch(cfg)["upsample"] == "deconv"
    assert "upsample" not in P.oracle_arch(make())


@pytest.mark.parametrize("name", ["retinanet", "fcos"])
def test_resize_config_is_unchanged(name):
    """UPSAMPLE = "resize" (explicit) gives the dict of a config without the key, bit for bit."""
    from basedet_amd.models import params as P
    make, init = _cfgs()[name]
    a = getattr(P, init)(make(), 1)
    cfg = make()
    cfg.MODEL.FPN.UPSAMPLE = "resize"
    b = getattr(P, init)(cfg, 1)
    assert list(a) == list(b)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not any("fpn_upsample" in k for k in b)


def test_faster_rcnn_ignores_the_upsample_key():
    """faster_rcnn.py:30-36 builds its FPN without `upsample`."""
    from basedet_amd.configs import FasterRCNNConfig
    from basedet_amd.models import params as P
    a = P.init_faster_rcnn_params(FasterRCNNConfig(), 0)
    cfg = FasterRCNNConfig()
    cfg.MODEL.FPN.UPSAMPLE = "deconv"
    b = P.init_faster_rcnn_params(cfg, 0)
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert "upsample" not in P.oracle_arch(cfg)


def _refused(model_cls, cfg, key, monkeypatch):
    """The check comes before any allocation or library call: loading the HIP library would raise something else."""
    from basedet_amd import _lib, ops

    def no_library(*a, **k):
        raise AssertionError("the HIP library was reached before the config check")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(ops, "L", no_library)
    with pytest.raises(ValueError) as ei:
        model_cls(cfg, params={}, device="cpu")
    assert key in str(ei.value)


@pytest.mark.parametrize("model", ["RetinaNet", "FCOS", "FreeAnchor", "ATSS", "OTA", "FasterRCNN"])
def test_unbuilt_norms_are_refused(model, monkeypatch):
    import basedet_amd.models as M
    from basedet_amd import configs
    make = getattr(configs, model + "Config")
    cfg = make()
    cfg.MODEL.BACKBONE.NORM = "SyncBN"
    _refused(getattr(M, model), cfg, "MODEL.BACKBONE.NORM", monkeypatch)
    cfg = make()
    cfg.MODEL.FPN.NORM = "GN"
    _refused(getattr(M, model), cfg, "MODEL.FPN.NORM", monkeypatch)


@pytest.mark.parametrize("model", ["RetinaNet", "FCOS", "FreeAnchor", "ATSS", "OTA"])
def test_unknown_upsample_is_refused(model, monkeypatch):
    import basedet_amd.models as M
    from basedet_amd import configs
    cfg = getattr(configs, model + "Config")()
    cfg.MODEL.FPN.UPSAMPLE = "nearest"
    _refused(getattr(M, model), cfg, "MODEL.FPN.UPSAMPLE", monkeypatch)


@pytest.mark.parametrize("model", ["RetinaNet", "FreeAnchor"])
def test_retina_head_without_norm_is_refused(model, monkeypatch):
    """retina_head.py:54-61: WITH_NORM = False removes the tower ReLUs."""
    import basedet_amd.models as M
    from basedet_amd import configs
    cfg = getattr(configs, model + "Config")()
    cfg.MODEL.HEAD.WITH_NORM = False
    _refused(getattr(M, model), cfg, "MODEL.HEAD.WITH_NORM", monkeypatch)
