"""MODEL.LOSSES.IOU_LOSS_TYPE of the FCOS family (configs/det_model/fcos_cfg.py:34 -> layers.iou_loss(loss_type=...)): the config check
and the C ABI boundary of the training kernel, without a device."""
import os
import re

import pytest

TYPES = ("iou", "linear_iou", "giou", "square_iou")     # layers/losses/iou_loss.py:78


def _cases():
    from basedet_amd import configs, models
    return [(models.FCOS, configs.FCOSConfig), (models.ATSS, configs.ATSSConfig), (models.OTA, configs.OTAConfig)]


@pytest.mark.parametrize("which", range(3))
def test_check_config_accepts_the_four_types_and_refuses_the_rest(which):
    model, config = _cases()[which]
    for t in TYPES:
        cfg = config()
        cfg.MODEL.LOSSES.IOU_LOSS_TYPE = t
        model.check_config(cfg)
    for bad in ("ciou", None):
        cfg = config()
        cfg.MODEL.LOSSES.IOU_LOSS_TYPE = bad
        with pytest.raises(ValueError) as e:
            model.check_config(cfg)
        msg = str(e.value)
        assert "MODEL.LOSSES.IOU_LOSS_TYPE" in msg and repr(bad) in msg
        assert all(repr(t) in msg for t in TYPES), msg


def test_type_codes_are_those_of_the_c_abi():
    from basedet_amd import ops
    assert ops.IOU_LOSS_TYPES == {"iou": 0, "linear_iou": 1, "giou": 2, "square_iou": 3}      # as bd_iou_loss_ltrb documents them


def test_header_and_ctypes_table_carry_the_entry_point():
    from basedet_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "basedet_hip.h")).read()
    m = re.search(r"\bint\s+bd_iou_ltrb_fwd_bwd\s*\(([^)]*)\)", header)
    assert m, "bd_iou_ltrb_fwd_bwd is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 11 and args[5] == "int loss_type"
    ret, argtypes = _lib.SIGNATURES["bd_iou_ltrb_fwd_bwd"]
    assert len(argtypes) == 11


def test_loss_grid_cap_is_exported():
    """The block cap of the loss launchers, which the device tests size their largest launch by."""
    from basedet_amd import ops
    assert 1 <= ops.loss_grid_cap() <= 65536
