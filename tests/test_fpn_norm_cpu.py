"""MODEL.FPN.NORM = "BN" / "SyncBN" without a GPU: the parameter tables, the config check (before the HIP library loads) and the
self-checks of the oracle subclass the GPU tests compare against (tests/fpn_norm_oracle.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from fpn_norm_oracle import EPS, norm_oracle_cls

MODELS = {"RetinaNet": "init_retinanet_params", "FreeAnchor": "init_retinanet_params", "FCOS": "init_fcos_params",
          "ATSS": "init_fcos_params", "OTA": "init_fcos_params", "FasterRCNN": "init_faster_rcnn_params"}


def _cfg(model, norm="BN"):
    from basedet_amd import configs
    cfg = getattr(configs, model + "Config")()
    cfg.MODEL.FPN.NORM = norm
    return cfg


@pytest.mark.parametrize("model", sorted(MODELS))
def test_parameter_table_with_bn(model):
    from basedet_amd.models import params as P
    cfg = _cfg(model)
    base = getattr(P, MODELS[model])(_cfg(model, None), 3)
    got = getattr(P, MODELS[model])(cfg, 3)
    stages = [int(f[-1]) for f in cfg.MODEL.BACKBONE.OUT_FEATURES]
    C = cfg.MODEL.FPN.OUT_CHANNELS
    norm = [f"backbone.fpn_{k}{s}.norm.{e}" for k in ("lateral", "output") for s in stages
            for e in ("weight", "bias", "running_mean", "running_var")]
    bias = [f"backbone.fpn_{k}{s}.bias" for k in ("lateral", "output") for s in stages]
    assert sorted(set(got) - set(base)) == sorted(norm) and sorted(set(base) - set(got)) == sorted(bias)
    assert list(got)[-len(norm):] == norm                   # added after everything else
    for k in got:
        if k in base:
            assert np.array_equal(got[k], base[k]), k       # same seed, same draws
    for k in norm:
        assert got[k].shape == (C,) and got[k].dtype == np.float32
        assert np.all(got[k] == (1.0 if k.endswith(("norm.weight", "running_var")) else 0.0))
    assert not any("top_block" in k and "norm" in k for k in got)
    assert [k for k in base if "top_block" in k] == [k for k in got if "top_block" in k]
    names = P.trainable_names(got, cfg.MODEL.BACKBONE.FREEZE_AT)
    assert all((k in names) == k.endswith((".norm.weight", ".norm.bias")) for k in norm)
    assert P.oracle_arch(cfg)["fpn_norm"] == "BN" and "fpn_norm" not in P.oracle_arch(_cfg(model, None))


@pytest.mark.parametrize("model", sorted(MODELS))
def test_parameter_table_without_norm_is_unchanged(model):
    """NORM = None: the table of a config that never had the key (what the parent commit drew), array for array."""
    from basedet_amd import configs
    from basedet_amd.models import params as P
    plain = getattr(configs, model + "Config")()
    plain.MODEL.FPN.pop("NORM")
    a, b = getattr(P, MODELS[model])(plain, 1), getattr(P, MODELS[model])(_cfg(model, None), 1)
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert not any(".norm." in k for k in b) and "backbone.fpn_lateral3.bias" in b


def _no_library(monkeypatch):
    from basedet_amd import _lib, ops

    def no_library(*a, **k):
        raise AssertionError("the HIP library was reached before the config check")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(ops, "L", no_library)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_check_config(model, monkeypatch):
    import basedet_amd.models as M
    _no_library(monkeypatch)
    cls = getattr(M, model)
    for norm in ("BN", "SyncBN", None):
        cls.check_config(_cfg(model, norm))
    for norm in ("LN", "GN", "bn", True):
        with pytest.raises(ValueError, match="MODEL.FPN.NORM"):
            cls(_cfg(model, norm), params={}, device="cpu")
    cfg = _cfg(model, "BN")
    cfg.MODEL.WEIGHT_DTYPE = "fp8_e4m3"
    with pytest.raises(ValueError, match="MODEL.FPN.NORM.*MODEL.WEIGHT_DTYPE"):
        cls(cfg, params={}, device="cpu")
    cfg = _cfg(model, "BN")
    cfg.MODEL.BACKBONE.NORM = "SyncBN"
    with pytest.raises(ValueError, match="MODEL.BACKBONE.NORM"):
        cls(cfg, params={}, device="cpu")


@pytest.mark.parametrize("model", sorted(MODELS))
def test_syncbn_is_refused_at_world_size_two(model, monkeypatch):
    """The exchange of the batch statistics between ranks is not built: "SyncBN" under a communicator of two ranks is refused before the
    library loads, "BN" (per-rank statistics) and a one-rank communicator are not."""
    import basedet_amd.models as M
    from basedet_amd import comm

    class Ranks:
        rank = 0

        def __init__(self, world):
            self.world = world
    _no_library(monkeypatch)
    cls = getattr(M, model)
    monkeypatch.setattr(comm, "_active", Ranks(2))
    with pytest.raises(ValueError, match="MODEL.FPN.NORM = 'SyncBN' at world size 2"):
        cls(_cfg(model, "SyncBN"), params={}, device="cpu")
    cls.check_config(_cfg(model, "BN"))
    monkeypatch.setattr(comm, "_active", Ranks(1))
    cls.check_config(_cfg(model, "SyncBN"))


# ---- the oracle subclass -----------------------------------------------------------------------------------------------------------
def _oracle(training=True, seed=0, top="p6p7"):
    rng = np.random.default_rng(seed)
    C, cin = 16, {3: 8, 4: 12, 5: 20}
    p = {}
    for s, ci in cin.items():
        p[f"backbone.fpn_lateral{s}.weight"] = rng.standard_normal((C, ci, 1, 1)).astype(np.float32)
        p[f"backbone.fpn_output{s}.weight"] = (rng.standard_normal((C, C, 3, 3)) * 0.2).astype(np.float32)
        for k in ("lateral", "output"):
            n = f"backbone.fpn_{k}{s}.norm"
            p[n + ".weight"] = rng.uniform(-1.5, 1.5, C).astype(np.float32)
            p[n + ".bias"] = rng.standard_normal(C).astype(np.float32)
            p[n + ".running_mean"] = rng.standard_normal(C).astype(np.float32)
            p[n + ".running_var"] = rng.uniform(0.5, 2.0, C).astype(np.float32)
    p["backbone.top_block.p6.weight"] = rng.standard_normal((C, 20, 3, 3)).astype(np.float32)
    p["backbone.top_block.p6.bias"] = rng.standard_normal(C).astype(np.float32)
    p["backbone.top_block.p7.weight"] = rng.standard_normal((C, C, 3, 3)).astype(np.float32)
    p["backbone.top_block.p7.bias"] = rng.standard_normal(C).astype(np.float32)
    feats = {f"res{s}": torch.from_numpy(rng.standard_normal((2, ci, 32 >> (s - 3), 40 >> (s - 3))).astype(np.float32)) for s, ci in cin.items()}
    orc = norm_oracle_cls()(p, dict(fpn_in=["res3", "res4", "res5"], fpn_norm="BN", top_block=top))
    orc.training = training
    return orc, p, feats


def _bn(y, p, n, training):
    t = lambda k: torch.from_numpy(p[f"{n}.norm.{k}"]).clone()
    return TF.batch_norm(y, t("running_mean"), t("running_var"), t("weight"), t("bias"), training=training, momentum=0.1, eps=EPS)


@pytest.mark.parametrize("training", [True, False])
def test_oracle_fpn_is_batch_norm_composed_by_hand(training):
    """Training: torch.nn.functional.batch_norm on the batch; evaluation: on the running statistics (the fold equals the formula)."""
    orc, p, feats = _oracle(training)
    got = orc.fpn(feats)
    w = lambda n: torch.from_numpy(p[n + ".weight"])
    prev, want = None, {}
    for s in (5, 4, 3):
        lat = _bn(TF.conv2d(feats[f"res{s}"], w(f"backbone.fpn_lateral{s}")), p, f"backbone.fpn_lateral{s}", training)
        if prev is not None:
            lat = lat + TF.interpolate(prev, scale_factor=2, mode="bilinear", align_corners=False)
        want[s] = _bn(TF.conv2d(lat, w(f"backbone.fpn_output{s}"), padding=1), p, f"backbone.fpn_output{s}", training)
        prev = lat
    for i, s in enumerate((3, 4, 5)):
        assert torch.allclose(got[i], want[s], rtol=1e-4, atol=1e-4), s
    p6 = TF.conv2d(feats["res5"], w("backbone.top_block.p6"), torch.from_numpy(p["backbone.top_block.p6.bias"]), stride=2, padding=1)
    assert torch.allclose(got[3], p6, rtol=1e-5, atol=1e-5) and len(got) == 5          # top_block: no norm


def test_oracle_running_statistics_follow_the_float64_recurrence():
    orc, p, feats = _oracle(True, seed=2)
    n = "backbone.fpn_lateral5"
    rm, rv = p[n + ".norm.running_mean"].astype(np.float64), p[n + ".norm.running_var"].astype(np.float64)
    for step in range(2):
        f = {k: v * (1.0 + step) for k, v in feats.items()}
        orc.fpn(f)
        y = TF.conv2d(f["res5"], torch.from_numpy(p[n + ".weight"])).double().numpy()
        M = y.size // y.shape[1]
        rm = 0.9 * rm + 0.1 * y.mean((0, 2, 3))
        rv = 0.9 * rv + 0.1 * y.var((0, 2, 3)) * M / (M - 1)
    assert np.allclose(orc.p[n + ".norm.running_mean"].numpy(), rm, rtol=1e-5, atol=1e-6)
    assert np.allclose(orc.p[n + ".norm.running_var"].numpy(), rv, rtol=1e-5)


def test_oracle_pool_top_block_has_no_norm():
    orc, p, feats = _oracle(True, top="pool")
    got = orc.fpn(feats)
    assert len(got) == 4 and torch.equal(got[3], got[2][:, :, ::2, ::2])
