"""MODEL.LOSSES.IOU_LOSS_TYPE on the device: bd_iou_ltrb_fwd_bwd (csrc/losses.hip) for "iou", "linear_iou", "giou" and "square_iou"
against float64, and FCOS / ATSS / OTA trained with each of them.

Reference: the loss values are oracle.box_ops.iou_loss_ltrb (float64 numpy, the reference's four types); the derivative is torch-CPU
autograd through a float64 restatement of the same formula (_loss64), which is first held to the oracle's values.  The prediction is
rounded to bf16 before either side sees it, so both evaluate the same numbers.

Tolerances are those tests/test_boxops_gpu.py::test_giou_and_bce_losses applies to the giou type of iou_ltrb_fwd_bwd: 1e-4 relative on the loss sum (fp32
summation order), rtol 3e-2 / atol 2e-6 on the bf16 gradient.  The normaliser of the kernel tests is a small constant, not the weight sum,
so that the gradients of a million-row launch stay far above that atol."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TYPES = ("iou", "linear_iou", "giou", "square_iou")
NEW_TYPES = ("iou", "linear_iou", "square_iou")
EPS = 1e-8
NORM = 8.0


def _ops():
    from basedet_amd import ops
    return ops


def _grid_cap():
    """The block cap of the loss launchers (bd_loss_grid_cap): past 256 x cap rows a thread walks more than one row."""
    cap = _ops().loss_grid_cap()
    assert 1 <= cap <= 65536
    return cap


def _row_counts():
    return (1, 255, 256, 257, 256 * _grid_cap() + 777)


# hand-built foreground rows (pred, target), appended behind the random ones
HAND = (
    ((-30.0, 4.0, 40.0, 6.0), (10.0, 10.0, 10.0, 10.0)),         # pred to the right of the target: wi_raw = 10 - 30 < 0, no overlap
    ((5.0, 3.0, -9.0, 4.0), (10.0, 10.0, 10.0, 10.0)),           # negative width: l + r < 0
    ((10.3, 7.7, 12.9, 5.1), (10.3, 7.7, 12.9, 5.1)),            # target == pred, not bf16-exact: no tie once pred is rounded
)
NONOVERLAP, NEGWIDTH, SAME = 0, 1, 2


def _loss64(p, t, loss_type):
    """iou_loss(box_mode="ltrb") (layers/losses/iou_loss.py:9-105) on float64 torch tensors, for autograd."""
    a1 = (p[:, 0] + p[:, 2]).clamp(min=0) * (p[:, 1] + p[:, 3]).clamp(min=0)
    a2 = (t[:, 0] + t[:, 2]).clamp(min=0) * (t[:, 1] + t[:, 3]).clamp(min=0)
    wi = (torch.minimum(p[:, 2], t[:, 2]) + torch.minimum(p[:, 0], t[:, 0])).clamp(min=0)
    hi = (torch.minimum(p[:, 3], t[:, 3]) + torch.minimum(p[:, 1], t[:, 1])).clamp(min=0)
    ai = wi * hi
    au = a1 + a2 - ai
    iou = ai / au.clamp(min=EPS)
    if loss_type == "giou":
        gw = torch.maximum(p[:, 2], t[:, 2]) + torch.maximum(p[:, 0], t[:, 0])
        gh = torch.maximum(p[:, 3], t[:, 3]) + torch.maximum(p[:, 1], t[:, 1])
        ac = gw * gh
        return 1 - (iou - (ac - au) / ac.clamp(min=EPS))
    if loss_type == "iou":
        return -torch.log(iou.clamp(min=EPS))
    if loss_type == "square_iou":
        return 1 - iou ** 2
    return 1 - iou


@functools.lru_cache(maxsize=None)
def _inputs(rows):
    """rows rows in all: random ltrb in (0, 64), about half foreground, then the HAND rows (foreground) where they fit."""
    rng = np.random.default_rng(1000 + rows)
    nh = len(HAND) if rows > len(HAND) else 0
    pred = rng.uniform(0.0, 64.0, (rows, 4)).astype(np.float32)
    tgt = rng.uniform(0.0, 64.0, (rows, 4)).astype(np.float32)
    w = rng.uniform(0.05, 1.0, rows).astype(np.float32)
    lab = (rng.uniform(size=rows) < 0.5).astype(np.int32) * rng.integers(1, 81, rows).astype(np.int32)
    lab[rng.uniform(size=rows) < 0.02] = -1                      # ignored rows are background to this loss as well
    if rows == 1:
        lab[:] = 3
    for i, (p, t) in enumerate(HAND[:nh]):
        r = rows - nh + i
        pred[r], tgt[r], lab[r] = p, t, 1 + i
    pred_bf = torch.from_numpy(pred).to(torch.bfloat16)
    p64 = pred_bf.float().numpy().astype(np.float64)
    tie = p64 == tgt.astype(np.float64)
    tgt[tie] += 0.37                                             # no exact ties: the derivative is defined
    assert not (p64 == tgt.astype(np.float64)).any()
    assert (lab > 0).any()
    dev = dict(pred=pred_bf.cuda(), tgt=torch.from_numpy(tgt).cuda(), w=torch.from_numpy(w).cuda(), lab=torch.from_numpy(lab).cuda())
    return dict(rows=rows, nh=nh, p64=p64, tgt=tgt, w=w, lab=lab, dev=dev)


@functools.lru_cache(maxsize=None)
def _reference(rows, loss_type):
    """Per-row float64 loss (the oracle's) and d loss / d pred (autograd), unweighted and unnormalised; never modified afterwards."""
    import oracle.box_ops as ob
    d = _inputs(rows)
    loss = ob.iou_loss_ltrb(d["p64"], d["tgt"].astype(np.float64), loss_type, EPS)
    p = torch.from_numpy(d["p64"]).requires_grad_(True)
    l64 = _loss64(p, torch.from_numpy(d["tgt"].astype(np.float64)), loss_type)
    assert np.allclose(l64.detach().numpy(), loss, rtol=1e-12, atol=1e-13)      # the restatement is the oracle's formula
    l64.sum().backward()
    grad = p.grad.numpy()
    loss.setflags(write=False); grad.setflags(write=False)
    return loss, grad


def _launch(d, loss_type, weighted, norm=NORM, loss_weight=1.0, lab=None, entry="iou"):
    ops = _ops()
    dev = d["dev"]
    rows = d["rows"]
    loss = torch.zeros((1,), dtype=torch.float32, device="cuda")
    dp = torch.full((rows, 4), float("nan"), dtype=torch.bfloat16, device="cuda")
    nrm = torch.tensor([norm], dtype=torch.float32, device="cuda")
    lab = dev["lab"] if lab is None else lab
    w = dev["w"] if weighted else None
    if entry == "giou":
        ops.iou_ltrb_fwd_bwd(dev["pred"], dev["tgt"], w, lab, rows, ops.IOU_LOSS_TYPES["giou"], nrm, loss_weight, loss, dp)
    else:
        ops.iou_ltrb_fwd_bwd(dev["pred"], dev["tgt"], w, lab, rows, ops.IOU_LOSS_TYPES[loss_type], nrm, loss_weight, loss, dp)
    torch.cuda.synchronize()
    return loss, dp


def _expected(d, loss_type, weighted, norm, loss_weight=1.0):
    loss, grad = _reference(d["rows"], loss_type)
    fg = d["lab"] > 0
    w = d["w"].astype(np.float64) if weighted else np.ones(d["rows"])
    scale = loss_weight / max(norm, 1.0)
    return float((loss * w)[fg].sum() * scale), grad * (w * fg)[:, None] * scale


@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "noweight"])
@pytest.mark.parametrize("loss_type", TYPES)
@pytest.mark.parametrize("which", range(5))
def test_kernel_matches_float64(which, loss_type, weighted):
    rows = _row_counts()[which]
    d = _inputs(rows)
    loss, dp = _launch(d, loss_type, weighted)
    ref_loss, ref_grad = _expected(d, loss_type, weighted, NORM)
    got_loss, got = float(loss.item()), dp.float().cpu().numpy()
    rel = abs(got_loss - ref_loss) / ref_loss
    err = np.abs(got - ref_grad) - 3e-2 * np.abs(ref_grad)
    print(f"rows={rows} {loss_type} weighted={weighted}: loss {got_loss:.9g} ref {ref_loss:.9g} rel {rel:.3g}; "
          f"gradient worst |err| - rtol |ref| = {err.max():.3g} (atol 2e-6)")
    assert rel < 1e-4
    assert np.isfinite(got).all()
    assert np.allclose(got, ref_grad, rtol=3e-2, atol=2e-6)
    assert not dp[d["dev"]["lab"] <= 0].view(torch.int16).any()             # background and ignored rows: +0
    if d["nh"]:
        base = rows - d["nh"]
        if loss_type == "iou":
            # no overlap, and the negative-width pred, whose intersection is empty too: zero gradient (their loss value alone:
            # test_row_without_intersection_alone)
            for r in (base + NONOVERLAP, base + NEGWIDTH):
                assert not dp[r].view(torch.int16).any()
        if loss_type != "giou":
            assert not (got[base + NEGWIDTH] != 0).any()
        assert (got[base + SAME] != 0).all()                                 # near the optimum, but no tie: every side has a slope


@pytest.mark.parametrize("which", [NONOVERLAP, NEGWIDTH], ids=["nonoverlap", "negwidth"])
@pytest.mark.parametrize("loss_type", TYPES)
def test_row_without_intersection_alone(loss_type, which):
    """One HAND row without intersection (the non-overlapping pair, or the pred of negative width) as the launch's only foreground
    row, weighted, so that the loss sum is that row's loss: the float64 value times the weight for every type, which for "iou" is
    -log(1e-8) times the weight, with a gradient of exactly zero; for "linear_iou" and "square_iou" 1 times the weight."""
    d = _inputs(257)
    r = 257 - d["nh"] + which
    lab = torch.zeros_like(d["dev"]["lab"])
    lab[r] = 1
    loss, dp = _launch(d, loss_type, True, norm=1.0, lab=lab)
    w = float(d["w"][r])
    ref = float(_reference(257, loss_type)[0][r]) * w
    if loss_type == "iou":
        assert abs(ref + math.log(1e-8) * w) < 1e-12
        assert not dp.view(torch.int16).any()
    elif loss_type != "giou":
        assert ref == w
        assert bool((dp == 0).all())                    # (-diou = -0.0 is a zero gradient as well)
    print(f"{loss_type} row {which}: loss {float(loss.item()):.9g} float64 {ref:.9g}")
    assert abs(float(loss.item()) - ref) / ref < 1e-4


@pytest.mark.parametrize("loss_type", TYPES)
def test_all_background_launch(loss_type):
    d = _inputs(257)
    lab = torch.zeros_like(d["dev"]["lab"])
    lab[::7] = -1
    loss, dp = _launch(d, loss_type, True, lab=lab)
    assert float(loss.item()) == 0.0 and not loss.view(torch.int32).any()
    assert not dp.view(torch.uint8).any()


@pytest.mark.parametrize("loss_type", TYPES)
def test_norm_below_one_is_clamped(loss_type):
    d = _inputs(257)
    loss, dp = _launch(d, loss_type, True, norm=0.25, loss_weight=2.0)
    one, dp_one = _launch(d, loss_type, True, norm=1.0, loss_weight=2.0)
    assert torch.equal(loss.view(torch.int32), one.view(torch.int32)) and torch.equal(dp.view(torch.int16), dp_one.view(torch.int16))
    ref_loss, ref_grad = _expected(d, loss_type, True, 0.25, 2.0)
    assert abs(float(loss.item()) - ref_loss) / ref_loss < 1e-4
    assert np.allclose(dp.float().cpu().numpy(), ref_grad, rtol=3e-2, atol=2e-6)


@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "noweight"])
@pytest.mark.parametrize("which", range(5))
def test_giou_entry_points_agree_bit_for_bit(which, weighted):
    d = _inputs(_row_counts()[which])
    a, da = _launch(d, "giou", weighted, entry="iou")
    b, db = _launch(d, "giou", weighted, entry="giou")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(da.view(torch.int16), db.view(torch.int16))


@pytest.mark.parametrize("code", [-1, 4, 99])
def test_unknown_loss_type_is_refused_before_any_launch(code):
    from basedet_amd import _lib
    ops = _ops()
    d = _inputs(257)
    dev = d["dev"]
    loss = torch.full((1,), 7.0, dtype=torch.float32, device="cuda")
    dp = torch.full((257, 4), 3.0, dtype=torch.bfloat16, device="cuda")
    nrm = torch.tensor([1.0], dtype=torch.float32, device="cuda")
    rc = ops.L().bd_iou_ltrb_fwd_bwd(_lib.ptr(dev["pred"]), _lib.ptr(dev["tgt"]), _lib.ptr(dev["w"]), _lib.ptr(dev["lab"]), 257, code,
                                     _lib.ptr(nrm), ctypes.c_float(1.0), _lib.ptr(loss), _lib.ptr(dp), _lib.stream_ptr())
    assert rc == -1                                                          # BD_EINVAL
    assert str(code) in ops.L().bd_last_error_string().decode()
    with pytest.raises(_lib.BasedetHipError):
        ops.iou_ltrb_fwd_bwd(dev["pred"], dev["tgt"], dev["w"], dev["lab"], 257, code, nrm, 1.0, loss, dp)
    torch.cuda.synchronize()
    assert float(loss.item()) == 7.0 and bool((dp == 3.0).all())             # nothing ran


# ---- models -------------------------------------------------------------------------------------------------------------------

MODELS = ("FCOS", "ATSS", "OTA")
KEYS = {"FCOS": ("cls_loss", "reg_loss", "ctr_loss"), "ATSS": ("cls_loss", "reg_loss", "ctr_loss"), "OTA": ("loss_cls", "loss_offsets", "loss_ious")}


def _model_setup(name, loss_type):
    """The small configuration of tests/test_model_gpu.py (FCOS, ATSS) and tests/test_ota_gpu.py (OTA): 2 x 128 x 160."""
    from basedet_amd import configs, models
    from basedet_amd.models import params as P
    from basedet_amd.utils import DummyLoader
    N, size = 2, (128, 160)
    cfg = getattr(configs, name + "Config")()
    cfg.MODEL.BATCHSIZE = N
    cfg.MODEL.LOSSES.IOU_LOSS_TYPE = loss_type
    params = P.init_fcos_params(cfg, seed=0, residual_gamma=0.25)
    params["head.bbox_pred.bias"] = np.full_like(params["head.bbox_pred.bias"], 0.5)      # keep relu(bbox_pred * scale) alive
    batch = next(DummyLoader(N, size, seed=0))
    batch["data"] = (batch["data"] * 255).astype(np.float32)
    return cfg, getattr(models, name)(cfg, params=params), batch


@functools.lru_cache(maxsize=None)
def _model_step(name, loss_type):
    """One training forward / backward; the losses and what the regression loss was computed from, read back to the host."""
    cfg, model, batch = _model_setup(name, loss_type)
    out = model(batch)
    pl = model._cur
    losses = {k: out[k].detach().clone().cpu() for k in KEYS[name]}
    model.backward()
    torch.cuda.synchronize()
    return dict(losses=losses, labels=pl.labels.cpu().numpy().reshape(-1),
                gt_offsets=pl.gt_offsets.cpu().numpy().reshape(-1, 4), gt_ctr=pl.gt_ctr.cpu().numpy().reshape(-1),
                stats=pl.stats.cpu().numpy().copy(), offsets=pl.offsets.float().cpu().numpy().reshape(-1, 4),
                d_off=pl.d_off.float().cpu().numpy().reshape(-1, 4), reg_weight=float(cfg.MODEL.LOSSES.REG_LOSS_WEIGHT))


@pytest.mark.parametrize("loss_type", NEW_TYPES)
@pytest.mark.parametrize("name", MODELS)
def test_model_regression_loss_matches_float64(name, loss_type):
    """reg_loss of one step against oracle.box_ops.iou_loss_ltrb in float64 on the plan's own targets and bf16 offsets: 2e-2 relative, the
    bound of the existing model tests for reg_loss.  The other losses of the step are those of the "giou" run, bit for bit."""
    import oracle.box_ops as ob
    s = _model_step(name, loss_type)
    fg = s["labels"] > 0
    assert fg.sum() >= 5
    loss = ob.iou_loss_ltrb(s["offsets"][fg].astype(np.float64), s["gt_offsets"][fg].astype(np.float64), loss_type, EPS)
    if name == "OTA":                                   # emd_losses (ota.py:211-216): 2 x sum / max(1, num_fg)
        ref = 2.0 * loss.sum() / max(1.0, float(s["stats"][0]))
    else:                                               # fcos.py:157-164: REG_LOSS_WEIGHT x sum(loss x ctr) / max(1, sum_ctr)
        ref = s["reg_weight"] * (loss * s["gt_ctr"][fg].astype(np.float64)).sum() / max(1.0, float(s["stats"][1]))
    cls_key, reg_key, other_key = KEYS[name]
    got = float(s["losses"][reg_key])
    print(f"{name} {loss_type}: {reg_key} {got:.9g} float64 {ref:.9g} rel {abs(got - ref) / abs(ref):.3g}")
    assert np.isfinite(got) and abs(got - ref) / abs(ref) < 2e-2, (got, ref)
    assert np.isfinite(s["d_off"]).all() and (s["d_off"][~fg] == 0).all() and (s["d_off"][fg] != 0).any()
    g = _model_step(name, "giou")
    for k in (cls_key, other_key):
        assert torch.equal(s["losses"][k].view(torch.int32), g["losses"][k].view(torch.int32)), k
    assert np.array_equal(s["labels"], g["labels"]) and np.array_equal(s["offsets"], g["offsets"])
    assert float(g["losses"][reg_key]) != got


@pytest.mark.parametrize("loss_type", NEW_TYPES)
def test_fcos_regression_loss_decreases(loss_type):
    """20 SGD steps on one fixed batch at the solver's own rate (SOLVER.BASIC_LR x batch, as DetSolver.build sets it): the last reg_loss
    is below the first."""
    from basedet_amd.solver import DetSolver
    cfg, model, batch = _model_setup("FCOS", loss_type)
    solver = DetSolver.build(cfg, model)
    assert solver.optimizer.param_groups[0]["lr"] == cfg.SOLVER.BASIC_LR * cfg.MODEL.BATCHSIZE
    vals = []
    for it in range(20):
        out = solver.minimize(model, batch)
        vals.append(float(out["reg_loss"]))
        assert np.isfinite(vals[-1]), vals
    print(f"FCOS {loss_type}: reg_loss {vals[0]:.6g} -> {vals[-1]:.6g} (lr {solver.optimizer.param_groups[0]['lr']:g}: " + " ".join(f"{v:.4f}" for v in vals) + ")")
    assert vals[-1] < vals[0], vals
