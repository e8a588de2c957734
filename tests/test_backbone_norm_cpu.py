"""MODEL.BACKBONE.NORM = "BN" / "SyncBN" without a GPU: the config check (before the HIP library loads), the parameter and trainable-name
tables, and the self-checks of the oracle subclass the GPU tests compare against (tests/backbone_norm_oracle.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from backbone_norm_oracle import EPS, backbone_norm_oracle_cls, batch_norm, is_backbone_norm_key, randomise_backbone_norms

MODELS = {"RetinaNet": "init_retinanet_params", "FreeAnchor": "init_retinanet_params", "FCOS": "init_fcos_params",
          "ATSS": "init_fcos_params", "OTA": "init_fcos_params", "FasterRCNN": "init_faster_rcnn_params"}


def _cfg(model, norm="BN", freeze_at=0):
    from basedet_amd import configs
    cfg = getattr(configs, model + "Config")()
    cfg.MODEL.BACKBONE.NORM = norm
    cfg.MODEL.BACKBONE.FREEZE_AT = freeze_at
    return cfg


def _no_library(monkeypatch):
    from basedet_amd import _lib, ops

    def no_library(*a, **k):
        raise AssertionError("the HIP library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(ops, "L", no_library)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_accept_refuse_matrix(model, monkeypatch):
    import basedet_amd.models as M
    _no_library(monkeypatch)
    cls = getattr(M, model)
    for freeze_at in (0, 1, 2):
        cls.check_config(_cfg(model, "FrozenBN", freeze_at))
        for norm in ("BN", "SyncBN"):
            if freeze_at == 0:
                cls.check_config(_cfg(model, norm, 0))
                continue
            with pytest.raises(ValueError) as ei:
                cls(_cfg(model, norm, freeze_at), params={}, device="cpu")
            msg = str(ei.value)
            assert "MODEL.BACKBONE.NORM" in msg and "FREEZE_AT" in msg and "frozen" in msg, msg
        for norm in ("GN", "bn", "LN", None, True, ["BN"]):
            with pytest.raises(ValueError, match="MODEL.BACKBONE.NORM"):
                cls(_cfg(model, norm, freeze_at), params={}, device="cpu")
    cfg = _cfg(model, "BN")
    cfg.MODEL.WEIGHT_DTYPE = "fp8_e4m3"
    with pytest.raises(ValueError, match="MODEL.BACKBONE.NORM.*MODEL.WEIGHT_DTYPE"):
        cls(cfg, params={}, device="cpu")


@pytest.mark.parametrize("model", sorted(MODELS))
def test_syncbn_is_refused_at_world_size_two(model, monkeypatch):
    import basedet_amd.models as M
    from basedet_amd import comm

    class Ranks:
        rank = 0

        def __init__(self, world):
            self.world = world
    _no_library(monkeypatch)
    cls = getattr(M, model)
    monkeypatch.setattr(comm, "_active", Ranks(2))
    with pytest.raises(ValueError, match="MODEL.BACKBONE.NORM = 'SyncBN' at world size 2"):
        cls(_cfg(model, "SyncBN"), params={}, device="cpu")
    cls.check_config(_cfg(model, "BN"))
    monkeypatch.setattr(comm, "_active", Ranks(1))
    cls.check_config(_cfg(model, "SyncBN"))


@pytest.mark.parametrize("norm", ["BN", "SyncBN"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_parameter_and_trainable_tables(model, norm, monkeypatch):
    """Names and shapes are the FrozenBN table's; gamma / beta of every backbone norm are arena parameters right behind their convolution's
    weight, the running statistics are buffers of the state_dict only."""
    import basedet_amd.models as M
    from basedet_amd.models import params as P
    from basedet_amd.models.fpn_base import FPNDetector
    _no_library(monkeypatch)
    monkeypatch.setattr(FPNDetector, "repack_weights", lambda self: None)
    cfg = _cfg(model, norm)
    params = getattr(P, MODELS[model])(cfg, 0)
    frozen = getattr(P, MODELS[model])(_cfg(model, "FrozenBN"), 0)
    assert list(params) == list(frozen) and all(np.array_equal(params[k], frozen[k]) for k in params)
    assert P.backbone_norm(cfg) == norm and P.backbone_norm(_cfg(model, "FrozenBN")) is None
    names = P.trainable_names(params, 0, norm)
    bn = [k for k in params if is_backbone_norm_key(k)]
    assert len(bn) == 4 * 53 and "backbone.bottom_up.bn1.weight" in bn                   # resnet50: 1 + 16 * 3 + 4 norms
    assert all((k in names) == k.endswith((".weight", ".bias")) for k in bn)
    assert sorted(set(names) - set(P.trainable_names(params, 0))) == sorted(k for k in bn if k.endswith((".weight", ".bias")))
    m = getattr(M, model)(cfg, params=randomise_backbone_norms(dict(params)), device="cpu")
    assert sorted(m.state_dict_trainable_names()) == sorted(names)
    arena = [e[0] for e in m.arena.entries]
    assert arena[:3] == ["backbone.bottom_up.conv1.weight", "backbone.bottom_up.bn1.weight", "backbone.bottom_up.bn1.bias"]
    i = arena.index("backbone.bottom_up.layer2.0.downsample.0.weight")
    assert arena[i + 1: i + 3] == ["backbone.bottom_up.layer2.0.downsample.1.weight", "backbone.bottom_up.layer2.0.downsample.1.bias"]
    assert not any("running_" in k for k in arena)
    sd = m.state_dict()
    assert set(sd) == set(params)
    for k in bn:
        assert sd[k].shape == params[k].shape and not np.array_equal(sd[k], params[k]), k       # the randomised values came back
    # the stem's norm sits in the conv1 bucket of the gradient all-reduce
    from basedet_amd.solver import GradBuckets
    rng = GradBuckets._ranges(type("B", (), {"model": m})())
    assert "bn1" not in rng and rng["conv1"][0] == 0 and rng["conv1"][1] >= m.arena.entries[2][2] + 64


def _oracles(norm):
    from test_model_gpu import _setup
    from basedet_amd.models import params as P
    from oracle.model import Oracle
    cfg, params, batch = _setup("resnet18", 2, (128, 160), overrides=dict(MODEL=dict(BACKBONE=dict(FREEZE_AT=0, NORM=norm))))
    params = randomise_backbone_norms(params)
    cls = Oracle if norm == "FrozenBN" else backbone_norm_oracle_cls()
    losses, _ = cls(params, P.oracle_arch(cfg)).retinanet_losses(batch)
    return {k: float(v.detach()) for k, v in losses.items()}


def test_the_fixture_feels_the_key():
    """The GPU test's fixture under "BN" against "FrozenBN": a loss must move by >= 10 x the GPU test's loss bound (2e-2 relative), or the
    GPU test could pass with the key ignored.  The fixture's running variances are what makes it so (randomise_backbone_norms):
    total_loss 2.7732 (BN) vs 4.8106 (FrozenBN), the largest relative move of a loss is 0.54 (reg_loss)."""
    bn, frozen = _oracles("BN"), _oracles("FrozenBN")
    move = max(abs(bn[k] - frozen[k]) / abs(frozen[k]) for k in bn)
    print("losses", bn, frozen, "largest relative move", move)
    assert move >= 10 * 2e-2


def test_oracle_batch_norm_against_torch_float64():
    rng = np.random.default_rng(0)
    y = torch.from_numpy(rng.standard_normal((3, 16, 7, 9)) * rng.uniform(0.2, 3, (1, 16, 1, 1)) + rng.uniform(-2, 2, (1, 16, 1, 1)))
    g, b = torch.from_numpy(rng.uniform(-1.5, 1.5, 16)), torch.from_numpy(rng.standard_normal(16))
    rm, rv = torch.from_numpy(rng.standard_normal(16)), torch.from_numpy(rng.uniform(0.5, 2, 16))
    y1, g1, b1 = (t.clone().requires_grad_(True) for t in (y, g, b))
    z, rm1, rv1 = batch_norm(y1, g1, b1, rm, rv)
    y2, g2, b2 = (t.clone().requires_grad_(True) for t in (y, g, b))
    rm2, rv2 = rm.clone(), rv.clone()
    ref = TF.batch_norm(y2, rm2, rv2, g2, b2, training=True, momentum=0.1, eps=EPS)
    assert torch.allclose(z, ref, rtol=1e-12, atol=1e-12)
    assert torch.allclose(rm1, rm2, rtol=1e-12, atol=1e-12) and torch.allclose(rv1, rv2, rtol=1e-12, atol=1e-12)
    w = torch.from_numpy(rng.standard_normal(tuple(z.shape)))
    (z * w).sum().backward()
    (ref * w).sum().backward()
    for a, c in ((y1, y2), (g1, g2), (b1, b2)):
        assert torch.allclose(a.grad, c.grad, rtol=1e-10, atol=1e-10)


def test_oracle_eval_is_the_frozen_arithmetic():
    """training = False: the running statistics, i.e. the base class's FrozenBN forward, bit for bit."""
    from test_model_gpu import _setup
    from basedet_amd.models import params as P
    from oracle.model import Oracle
    cfg, params, batch = _setup("resnet18", 1, (64, 64), overrides=dict(MODEL=dict(BACKBONE=dict(FREEZE_AT=0, NORM="BN"))))
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((1, 3, 64, 64)).astype(np.float32))
    orc = backbone_norm_oracle_cls()(params, P.oracle_arch(cfg))
    orc.training = False
    with torch.no_grad():
        a, b = orc.backbone(x), Oracle(params, P.oracle_arch(cfg)).backbone(x)
        orc.training = True
        c = orc.backbone(x)
    assert all(torch.equal(a[k], b[k]) for k in b)
    assert not torch.equal(c["res5"], b["res5"])
    assert not torch.equal(orc.p["backbone.bottom_up.bn1.running_mean"], torch.from_numpy(params["backbone.bottom_up.bn1.running_mean"]))
