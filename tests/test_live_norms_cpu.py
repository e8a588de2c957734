"""LiveNorms (basedet_amd/models/live_norm.py) without a GPU: one owner of every live norm's buffers, in forward order, and a plan whose
byte count did not move when the per-plan pre-norm tensors moved into pl.norm_y / pl.norm_gy."""
import pytest
import torch

CASES = {"fpn": dict(FPN=dict(NORM="BN")), "backbone": dict(BACKBONE=dict(NORM="BN", FREEZE_AT=0)),
         "both": dict(FPN=dict(NORM="BN"), BACKBONE=dict(NORM="BN", FREEZE_AT=0)), "default": {}}
# FPNDetector.plan_bytes(model.reserve(2, 64, 96)) of RetinaNet-R18 at commit c18419c (pl.bn_y / b.ys / pl.stem_y)
PLAN_BYTES = {"fpn": 58720256, "backbone": 62914560, "both": 62914560, "default": 58720256}


def _model(case, monkeypatch):
    from basedet_amd.configs import retinanet_r18_config
    from basedet_amd.models import RetinaNet, params as P
    from basedet_amd.models.fpn_base import FPNDetector

    def no_anchor_launch(self, pl):         # (the one kernel launch of _plan; its output is not a plan-arena buffer)
        pl.A_total, pl.anchors = pl.pyr.pix_per_img * self.num_anchors, None
    monkeypatch.setattr(FPNDetector, "repack_weights", lambda self: None)
    monkeypatch.setattr(FPNDetector, "_plan_anchors", no_anchor_launch)
    cfg = retinanet_r18_config()
    cfg.merge(dict(MODEL=CASES[case]))
    return RetinaNet(cfg, params=P.init_retinanet_params(cfg, 0), device="cpu")


@pytest.mark.parametrize("case", sorted(CASES))
def test_one_owner_in_forward_order(case, monkeypatch):
    model = _model(case, monkeypatch)
    norms = list(model.norms)
    assert bool(model.norms) == (case != "default") and len(model.norms) == len(norms)
    total = sum(n.C for n in norms)
    assert model.norms.running.numel() == 2 * total and model.norms.stats.numel() == 2 * total and model.norms.sums.numel() == 3 * total
    # backbone first (the stem's bn1 leading, as in the forward pass), then the FPN: every lateral, every output convolution
    names = [n.name for n in norms]
    fpn = [f"backbone.fpn_{k}{s}.norm" for k in ("lateral", "output") for s in model.fpn_stages] if "FPN" in CASES[case] else []
    bb = names[:len(names) - len(fpn)]
    assert names[len(bb):] == fpn and all(n.startswith("backbone.bottom_up.") for n in bb)
    if "BACKBONE" in CASES[case]:
        convs = [c for c in model.convs.values() if c.name.startswith("backbone.bottom_up.")]
        assert bb == ["backbone.bottom_up.bn1"] + [c.norm.name for c in convs] and model.stem.norm is norms[0]
    else:
        assert bb == []
    # record i's views alias the flat tensors at its running offset
    o = 0
    for i, n in enumerate(norms):
        n.running_mean.fill_(i + 1.0)
        n.running_var.fill_(-(i + 1.0))
        n.inv_std.fill_(i + 0.5)
        n.sums[2].fill_(i + 0.25)
        assert torch.all(model.norms.running[2 * o: 2 * o + n.C] == i + 1.0) and torch.all(model.norms.running[2 * o + n.C: 2 * (o + n.C)] == -(i + 1.0))
        assert torch.all(model.norms.stats[2 * o + n.C: 2 * (o + n.C)] == i + 0.5)
        assert torch.all(model.norms.sums[3 * o + 2 * n.C: 3 * (o + n.C)] == i + 0.25)
        o += n.C
    assert o == total


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_bytes_are_the_parent_commits(case, monkeypatch):
    model = _model(case, monkeypatch)
    pl = model.reserve(2, 64, 96)
    assert model.plan_bytes(pl) == PLAN_BYTES[case]
    assert sorted(pl.norm_y) == sorted(pl.norm_gy) == sorted(n.name for n in model.norms)
    for n in model.norms:
        assert pl.norm_y[n.name].shape == pl.norm_gy[n.name].shape == (pl.norm_geo[n.name].pixels, n.C)
