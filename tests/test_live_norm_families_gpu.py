"""FCOS, ATSS, OTA (top-k) and FreeAnchor under live batch norms (MODEL.BACKBONE.NORM = "BN", FREEZE_AT = 0, MODEL.FPN.NORM = "BN"): one
training step of each on the R18 fixture (2 x 128 x 160) against backbone_norm_oracle_cls(norm_oracle_cls()) composed over the family's
loss method, as tests/test_backbone_norm_gpu.py::test_faster_rcnn_step_matches_oracle composes it.  tests/test_backbone_norm_gpu.py and
tests/test_fpn_norm_gpu.py run RetinaNet and Faster R-CNN; these four families share the normalised backbone and FPN code but bring their
own heads (GroupNorm towers, per-level scales), assignments and losses behind it.

Bounds, the project's own: labels and assignments equal; losses 2e-2 against the fp32 oracle; every trainable parameter's gradient
rel-L2 1e-2 against the sim_bf16 oracle on the stored activations and the stored dL/dz of every norm; running statistics to
tests/test_backbone_norm_gpu.py::test_norm_state_is_live_after_two_steps's bounds.  OTA's assignment reads the network's own predictions,
bf16 here and fp32 in the oracle; on this fixture (13 foreground points) it is equal all the same and is asserted so, and the gradients
are then compared on the device's assignment forced into the oracle, as tests/test_ota_gpu.py does.

Whole-model gradient cosine against the fp32 oracle, by the rule of tests/test_backbone_norm_gpu.py: 0.99 where the distance of the
sim_bf16 oracle from the fp32 oracle, measured on the CPU (the code under test takes no part), leaves it a factor 2 -- 1 - cos <= 5e-3 --
and 1 - 2 (1 - cos) otherwise.  MEASURED below holds that CPU measurement per family.

On an MI355X (also in DESIGN.md, 4s): worst per-parameter rel-L2 (bound 1e-2) fcos 5.8e-3, atss 5.7e-3, ota 7.8e-3, freeanchor 4.8e-3;
whole-model cosine fcos 0.98317, atss 0.98303, ota 0.96897, freeanchor 0.98375; losses within 6.6e-4, 4.1e-4, 2.5e-3, 7.1e-4 of the
fp32 oracle's; running statistics 3.3e-8 (|mu| + sigma) and 1.7e-7 relative (bounds 1e-5 and 1e-4).

The ground-truth boxes of the three GIoU families sit 0.37 px off the pixel grid (fixture()).  On the loader's own boxes one OTA
foreground point predicted a top side of exactly 32.0 px against a target of 32.0: min / max have no derivative there, the kernel's
documented subgradient (0 to both sides) and autograd's (half to each) differ, and that one row of 13 moved the regression branch's
gradients by 4e-2 to 1e-1 and the CPU-measured ATSS distance from 9.6e-3 on one host to 4.7e-2 on another."""
import numpy as np
import pytest
import torch

from backbone_norm_oracle import backbone_norm_oracle_cls, randomise_backbone_norms
from fpn_norm_oracle import norm_oracle_cls, randomise_norms

pytestmark = pytest.mark.gpu

SIZE = (128, 160)
R18 = dict(BACKBONE=dict(NAME="resnet18", OUT_FEATURE_CHANNELS=[128, 256, 512], FREEZE_AT=0, NORM="BN"),
           FPN=dict(TOP_BLOCK_IN_CHANNELS=512, NORM="BN"))
FCOS_LOSSES = ("cls_loss", "reg_loss", "ctr_loss", "total_loss")
FAMILIES = {"fcos": ("FCOSConfig", "FCOS", "fcos_losses", FCOS_LOSSES), "atss": ("ATSSConfig", "ATSS", "fcos_losses", FCOS_LOSSES),
            "ota": ("OTAConfig", "OTA", "ota_losses", ("loss_cls", "loss_offsets", "loss_ious", "total_loss")),
            "freeanchor": ("FreeAnchorConfig", "FreeAnchor", "freeanchor_losses", ("pos_loss", "neg_loss", "total_loss"))}

# sim_bf16 oracle against fp32 oracle on the CPU, whole-model gradient: 1 - cosine (measure_oracle_distance below), the larger of the
# measurements on two hosts (fcos 1.606e-2 / 1.592e-2, atss 1.663e-2 / 1.618e-2, ota 3.202e-2 / 3.550e-2, freeanchor 1.648e-2 both).  None
# leaves the factor 2 to 0.99 (1 - cos <= 5e-3), so every bound is 1 - 2 (1 - cos): fcos 0.9679, atss 0.9667, ota 0.9290, freeanchor 0.9670.
# (The losses of the two oracles differ by at most 5.7e-4, 3.0e-4, 3.2e-3 and 7.0e-4: far inside 2e-2.)
MEASURED = {"fcos": 1.606e-2, "atss": 1.663e-2, "ota": 3.550e-2, "freeanchor": 1.648e-2}


def cosine_bound(family):
    d = MEASURED[family]
    return 0.99 if 2 * d <= 1e-2 else 1 - 2 * d


def fixture(family):
    """cfg, params, batch: the family's fixture of tests/test_model_gpu.py / test_ota_gpu.py / test_freeanchor_gpu.py on R18 with both
    norms live and every norm's gamma / beta / running statistics randomised."""
    from basedet_amd import configs as K
    from basedet_amd.models import params as P
    from basedet_amd.utils import DummyLoader
    cfg = getattr(K, FAMILIES[family][0])()
    cfg.MODEL.BATCHSIZE = 2
    cfg.merge(dict(MODEL=R18))
    if family == "freeanchor":
        params = P.init_retinanet_params(cfg, seed=0)
    else:
        params = P.init_fcos_params(cfg, seed=0, residual_gamma=0.25)
        rng = np.random.default_rng(7)
        for k in list(params):
            if k.startswith("head.") and k.endswith((".1.weight", ".4.weight", ".7.weight", ".10.weight")):
                params[k] = rng.uniform(0.7, 1.3, params[k].shape).astype(np.float32)       # GroupNorm gamma
            if k == "head.scales":
                params[k] = rng.uniform(0.8, 1.2, params[k].shape).astype(np.float32)
        params["head.bbox_pred.bias"] = np.full_like(params["head.bbox_pred.bias"], 0.5)    # keep relu(bbox_pred * scale) alive
    params = randomise_backbone_norms(randomise_norms(params))
    batch = next(DummyLoader(2, SIZE, seed=0))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    if family != "freeanchor":
        # The loader draws some boxes on whole pixels, so a regression target can be a value like 32.0 that the bf16 prediction (a grid
        # of 0.25 px there) hits exactly.  At such a tie min / max have no derivative: the kernel gives 0 to both sides,
        # autograd half to each.  The boxes move off the grid by 0.37 px, as tests/test_iou_loss_types_gpu.py moves its targets;
        # _check_assignment asserts that no tie is left.
        batch["gt_boxes"] = np.array(batch["gt_boxes"], np.float32)
        for n, valid in enumerate(np.asarray(batch["im_info"])[:, 4].astype(int)):
            batch["gt_boxes"][n, :valid, :4] += 0.37
    return cfg, params, batch


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))


def _flat(grads, names):
    return torch.cat([grads[n].detach().double().reshape(-1) for n in names])


def measure_oracle_distance(family):
    """The CPU measurement behind MEASURED: fp32 oracle and sim_bf16 oracle (no stored activation injected), one step each."""
    from basedet_amd.models import params as P
    cfg, params, batch = fixture(family)
    names = P.trainable_names(params, 0, "BN")
    Orc = backbone_norm_oracle_cls(norm_oracle_cls())
    out = []
    for sim in (False, True):
        orc = Orc(dict(params), P.oracle_arch(cfg), trainable=names, sim_bf16=sim)
        losses, _ = getattr(orc, FAMILIES[family][2])(batch)
        out.append((losses, orc.grads(losses["total_loss"])))
    (l0, g0), (l1, g1) = out
    rel = {k: abs(float(l1[k]) - float(l0[k])) / abs(float(l0[k])) for k in FAMILIES[family][3]}
    return 1 - _cos(_flat(g1, names), _flat(g0, names)), rel


def _check_assignment(family, pl, aux):
    lab = pl.labels.cpu().numpy()
    if family == "freeanchor":               # no assignment: the bag loss reads every anchor
        return
    fg = torch.from_numpy(lab.reshape(-1) > 0)
    ties = pl.offsets.float().cpu().reshape(-1, 4)[fg] == pl.gt_offsets.cpu().reshape(-1, 4)[fg]
    assert int(fg.sum()) > 0 and not bool(ties.any()), "a predicted side equals its target: the GIoU gradient is not defined there"
    assert np.array_equal(lab, aux["labels"])
    got, want = pl.gt_offsets.cpu().numpy().reshape(-1, 4), np.asarray(aux["gt_offsets"]).reshape(-1, 4)
    rows = fg.numpy() if family == "ota" else slice(None)      # (OTA's oracle fills the targets of foreground points only)
    assert np.array_equal(got[rows], want[rows])
    assert aux["num_fg"] > 10 and pl.stats.cpu().numpy()[0] == aux["num_fg"]


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_step_matches_oracle(family):
    from basedet_amd import models as M
    from basedet_amd.models import params as P
    cfg, params, batch = fixture(family)
    _, cls, losses_fn, loss_keys = FAMILIES[family]
    model = getattr(M, cls)(cfg, params=params)
    names = P.trainable_names(params, 0, "BN")
    assert sorted(names) == sorted(model.state_dict_trainable_names())
    bu = "backbone.bottom_up"
    assert bu + ".bn1.weight" in names and bu + ".layer1.0.bn1.bias" in names and "backbone.fpn_lateral3.norm.weight" in names
    if family != "freeanchor":
        assert "head.scales" in names and "head.cls_subnet.1.weight" in names
    Orc = backbone_norm_oracle_cls(norm_oracle_cls())
    orc = Orc(dict(params), P.oracle_arch(cfg), trainable=names)
    ref, aux = getattr(orc, losses_fn)(batch)
    ref_grads = orc.grads(ref["total_loss"])
    out = model(batch)
    pl = model._cur
    _check_assignment(family, pl, aux)
    rel_loss = {k: abs(float(out[k]) - float(ref[k].detach())) / abs(float(ref[k].detach())) for k in loss_keys}
    print(family, "losses vs the fp32 oracle, rel", rel_loss)
    model.backward()
    torch.cuda.synchronize()
    got = model.reference_grads()
    cos = _cos(_flat(got, names), _flat(ref_grads, names))
    print(family, "whole-model gradient cosine", cos, "bound", cosine_bound(family))
    # per parameter: the sim_bf16 oracle on the stored activations, the stored dL/dz of every backbone norm and the stored dL/d lat_s
    acts = model.debug_activations()
    for s in model.fpn_stages:
        g = pl.blk[pl.res[s]].gout
        acts[f"g_lat{s}"] = pl.g_lat[s].float().cpu().view(pl.N, g.H[0], g.W[0], -1).permute(0, 3, 1, 2).contiguous()
    orc2 = Orc(dict(params), P.oracle_arch(cfg), trainable=names, sim_bf16=True, inject=acts)
    if family == "ota":
        forced = (pl.labels.cpu().numpy(), pl.gt_offsets.cpu().numpy(), pl.gt_ctr.cpu().numpy())
        l2, _ = orc2.ota_losses(batch, forced=forced)
        tight = {k: abs(float(out[k]) - float(l2[k].detach())) / abs(float(l2[k].detach())) for k in loss_keys}
        print("ota losses vs the oracle on the device's own assignment, rel", tight)
    else:
        l2, _ = getattr(orc2, losses_fn)(batch)
    g2 = orc2.grads(l2["total_loss"])
    print(family, "oracle's own dL/dz against the stored one, worst rel-L2", max(orc2.grad_check.items(), key=lambda t: t[1]))
    rels = {n: float((got[n].double().reshape(-1) - g2[n].detach().double().reshape(-1)).norm() / (g2[n].detach().double().norm() + 1e-30))
            for n in names}
    bad = {n: r for n, r in rels.items() if not r < 1e-2}
    print(family, "worst per-parameter rel-L2", max(rels.items(), key=lambda t: t[1]), "over 1e-2:", bad)
    # running statistics: momentum 0.1, unbiased variance, over the float64 statistics of the stored bf16 pre-norm tensors
    worst_m = worst_v = 0.0
    stats_bad = []
    sd = model.state_dict()
    for n in model.norms:
        y = pl.norm_y[n.name].double().cpu().numpy()
        cnt = y.shape[0]
        mu, var = y.mean(0), y.var(0)
        rm = 0.9 * params[n.name + ".running_mean"].astype(np.float64) + 0.1 * mu
        rv = 0.9 * params[n.name + ".running_var"].astype(np.float64) + 0.1 * var * cnt / (cnt - 1)
        em = np.abs(sd[n.name + ".running_mean"] - rm) / (np.abs(mu) + np.sqrt(var))
        ev = np.abs(sd[n.name + ".running_var"] - rv) / rv
        worst_m, worst_v = max(worst_m, float(em.max())), max(worst_v, float(ev.max()))
        if not (np.all(em <= 1e-5) and np.all(ev <= 1e-4)):
            stats_bad.append(n.name)
        assert not np.array_equal(sd[n.name + ".running_var"], params[n.name + ".running_var"]), n.name
    print(family, "running statistics: worst mean error / (|mu| + sigma)", worst_m, "worst relative variance error", worst_v)
    # ---- the assertions, after every figure is printed -------------------------------------------------------------------------------
    for k in loss_keys:
        assert rel_loss[k] < 2e-2, (k, rel_loss[k])
    if family == "ota":
        for k in loss_keys:                  # same activations, same targets: tight
            assert tight[k] < 2e-2, (k, tight[k])
    assert cos > cosine_bound(family), cos
    assert len(orc2.grad_check) == 1 + sum(len(b["convs"]) for b in model.blocks) + len(model.fpn_stages)
    assert all(v < 1e-2 for v in orc2.grad_check.values()), {k: v for k, v in orc2.grad_check.items() if not v < 1e-2}
    assert not bad, bad
    assert len(model.norms) > 20 and not stats_bad, stats_bad
    for n in (bu + ".bn1.weight", bu + ".layer2.1.bn2.bias", bu + ".layer2.0.downsample.1.weight", "backbone.fpn_output3.norm.weight",
              "backbone.fpn_lateral4.norm.bias"):
        assert float(got[n].abs().sum()) > 0 and _cos(got[n], g2[n].detach()) > 0.999, n
