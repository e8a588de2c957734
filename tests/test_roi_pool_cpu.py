"""MODEL.ROI_POOLER.METHOD without a GPU: the accepted values, the error for any other, parameter shapes, and the ABI of RoI max pooling."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bd_roi_pool_fwd", "bd_roi_pool_bwd_bf16_workspace_bytes", "bd_roi_pool_bwd_bf16")


def _cfg(method):
    from basedet_amd.configs import FasterRCNNConfig
    cfg = FasterRCNNConfig()
    cfg.merge(dict(MODEL=dict(BACKBONE=dict(NAME="resnet18", OUT_FEATURE_CHANNELS=[64, 128, 256, 512]), FPN=dict(TOP_BLOCK_IN_CHANNELS=512),
                              ROI_POOLER=dict(METHOD=method))))
    return cfg


def test_default_is_roi_align():
    from basedet_amd.configs import FasterRCNNConfig
    assert FasterRCNNConfig().MODEL.ROI_POOLER.METHOD == "roi_align"


def test_roi_pool_builds_the_same_parameter_shapes():
    from basedet_amd.models import params as P
    a = P.init_faster_rcnn_params(_cfg("roi_align"), 0)
    b = P.init_faster_rcnn_params(_cfg("roi_pool"), 0)
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k


def test_accepted_methods():
    from basedet_amd.models.faster_rcnn import ROI_POOLER_METHODS, check_roi_pooler_method
    assert ROI_POOLER_METHODS == ("roi_align", "roi_pool")
    for m in ROI_POOLER_METHODS:
        assert check_roi_pooler_method(m) == m


@pytest.mark.parametrize("method", ["roi_pool_avg", "ROI_POOL", "", None])
def test_unknown_method_raises_naming_the_key(method):
    from basedet_amd.models.faster_rcnn import check_roi_pooler_method
    with pytest.raises(ValueError, match=r"MODEL\.ROI_POOLER\.METHOD = .* is not supported: use 'roi_align' or 'roi_pool'"):
        check_roi_pooler_method(method)


def test_model_construction_checks_the_method():
    """_build_head runs the check itself (the assert it replaces is gone)."""
    src = open(os.path.join(ROOT, "basedet_amd", "models", "faster_rcnn.py")).read()
    assert "check_roi_pooler_method(m.ROI_POOLER.METHOD)" in src
    assert not re.search(r"assert\s+m\.ROI_POOLER\.METHOD", src)


def test_abi_symbols_declared():
    from basedet_amd import _lib
    header = open(os.path.join(ROOT, "include", "basedet_hip.h")).read()
    lib_src = open(_lib.__file__).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", header), s
        assert f'"{s}"' in lib_src, s
    from basedet_amd import ops
    assert callable(ops.roi_pool_fwd) and callable(ops.roi_pool_bwd_bf16) and callable(ops.roi_pool_bwd_bf16_workspace_bytes)
