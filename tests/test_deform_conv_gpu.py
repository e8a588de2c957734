"""csrc/deform_conv.hip (bd_deform_conv_fwd / _bwd_data / _wgrad) and basedet.layers.DeformConvWithOff / ModulatedDeformConvWithOff against
the float64 oracle of tests/deform_conv_oracle.py on the same bf16 operands.

Every operand lives in a util.guarded allocation: inputs between NaN guards and compared bit for bit afterwards, outputs and workspaces
between sentinel guards.  Bounds (util.bound_ratio <= 1, tol = rel |ref| + abs_s S, S = the sum of the magnitudes of the result's terms):
  rel = 2^-8 for the bf16 outputs (their own rounding);
  y, d_w: abs_s = 2^-9 + 2^-16 -- one bf16 rounding of the sampled operand in the LDS tile, plus the fp32 accumulation term of the audits;
  d_x, d_om: abs_s = 2^-8 -- the bf16 column gradient (2^-9) plus one further operand rounding;
  fp32 outputs (d_w, d_bias): the abs_s term plus 2^-24 |ref|.
y, d_om, d_w and d_bias must repeat bit for bit; d_x (fp32 atomics) must hold its bound both times."""
import functools

import pytest
import torch
import torch.nn.functional as TF

import deform_conv_oracle as O
import util
from util import bf16_round, bound_ratio, guarded

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 7, 8, 8), (3, 13, 21, 72, 40), (2, 16, 16, 128, 64), (2, 8, 8, 256, 128)]
FAMILIES = ["normal", "zero", "halves", "outside", "edges"]
REL = 2.0 ** -8
ABS_FWD = 2.0 ** -9 + 2.0 ** -16
ABS_BWD = 2.0 ** -8


def _offsets(family, N, H, W, modulated, g):
    """om (N, H, W, ld) float32 holding bf16 values; the pad channels hold NaN: nobody may read them as data."""
    ld = 32 if modulated else 24
    om = torch.full((N, H, W, ld), float("nan"))
    base_h = (torch.arange(H).view(1, H, 1, 1) - 1 + (torch.arange(9) // 3).view(1, 1, 1, 9)).float().expand(N, H, W, 9)
    base_w = (torch.arange(W).view(1, 1, W, 1) - 1 + (torch.arange(9) % 3).view(1, 1, 1, 9)).float().expand(N, H, W, 9)
    logits = torch.randn(N, H, W, 9, generator=g)
    if family == "normal":
        dy, dx = 2.0 * torch.randn(N, H, W, 9, generator=g), 2.0 * torch.randn(N, H, W, 9, generator=g)
    elif family == "zero":
        dy, dx = torch.zeros(N, H, W, 9), torch.zeros(N, H, W, 9)
        logits = torch.full((N, H, W, 9), 30.0)
    elif family == "halves":
        dy = torch.randint(-6, 7, (N, H, W, 9), generator=g).float() * 0.5
        dx = torch.randint(-6, 7, (N, H, W, 9), generator=g).float() * 0.5
    elif family == "outside":
        sign = torch.randint(0, 2, (N, H, W, 9), generator=g).float() * 2 - 1
        dy, dx = sign * (H + 3), torch.randn(N, H, W, 9, generator=g)
    else:       # edges: samples at exactly -1, 0, H - 1, H (rows) and -1, 0, W - 1, W (columns), mixed with ordinary positions
        th = torch.tensor([-1.0, 0.0, H - 1.0, float(H)])[torch.randint(0, 4, (N, H, W, 9), generator=g)]
        tw = torch.tensor([-1.0, 0.0, W - 1.0, float(W)])[torch.randint(0, 4, (N, H, W, 9), generator=g)]
        dy, dx = th - base_h, tw - base_w
        keep_h, keep_w = torch.rand(N, H, W, 9, generator=g) < 0.3, torch.rand(N, H, W, 9, generator=g) < 0.3
        dy = torch.where(keep_h, bf16_round(torch.randn(N, H, W, 9, generator=g)), dy)
        dx = torch.where(keep_w, bf16_round(torch.randn(N, H, W, 9, generator=g)), dx)
    om[..., 0:18:2], om[..., 1:18:2] = bf16_round(dy), bf16_round(dx)
    if modulated:
        om[..., 18:27] = bf16_round(logits)
    return om


def _in(data, dtype, name):
    rows, cols = (data.shape[0], None) if data.dim() == 1 else data.shape
    t, h = guarded(rows, cols, dtype, "cuda", fill="nan", name=name)
    h.set(data.to(dtype))
    h.snapshot()
    return t, h


def _out(rows, cols, dtype, name):
    return guarded(rows, cols, dtype, "cuda", fill="sentinel", name=name)


@functools.lru_cache(maxsize=None)
def _case(shape, family, modulated):
    """Runs forward once and both backward entries twice; returns the GPU results (CPU copies) and the oracle."""
    from basedet_amd import ops
    N, H, W, Cin, Cout = shape
    M = N * H * W
    g = torch.Generator().manual_seed(1000 * SHAPES.index(shape) + 10 * FAMILIES.index(family) + int(modulated))
    x = bf16_round(torch.randn(M, Cin, generator=g))
    w = torch.randn(Cout, 3, 3, Cin, generator=g) * (1.0 / (9 * Cin)) ** 0.5
    bias = torch.randn(Cout, generator=g)
    dy = bf16_round(torch.randn(M, Cout, generator=g))
    add = bf16_round(torch.randn(M, Cin, generator=g))
    om = _offsets(family, N, H, W, modulated, g).view(M, -1)
    ld = om.shape[1]

    wf, hwf = _out(Cout * 9, Cin, torch.bfloat16, "w_fwd")
    wd, hwd = _out(Cin * 9, Cout, torch.bfloat16, "w_dgrad")
    ops.weight_pack(w.cuda(), None, wf, wd, Cout, 9, Cin)
    hwf.snapshot(), hwd.snapshot()
    ins = [_in(x, torch.bfloat16, "x"), _in(om, torch.bfloat16, "om"), _in(bias, torch.float32, "bias"), _in(dy, torch.bfloat16, "dy"),
           _in(add, torch.bfloat16, "add")]
    (tx, _), (tom, _), (tb, _), (tdy, _), (tadd, _) = ins
    handles = [h for _, h in ins] + [hwf, hwd]

    res = {"shape": shape, "ld": ld}
    y, hy = _out(M, Cout, torch.bfloat16, "y")
    ops.deform_conv_fwd(tx, tom, wf, tb, y, N, H, W, Cin, Cout, modulated)
    torch.cuda.synchronize()
    hy.check()
    y2, hy2 = _out(M, Cout, torch.bfloat16, "y (second run)")
    ops.deform_conv_fwd(tx, tom, wf, tb, y2, N, H, W, Cin, Cout, modulated)
    torch.cuda.synchronize()
    hy2.check()
    res["y"], res["y2"] = y.cpu(), y2.cpu()

    runs = []
    for r in range(2):
        ws1, hws1 = _out(ops.deform_conv_bwd_data_workspace_bytes(N, H, W, Cin, Cout), None, torch.uint8, "bwd_data workspace")
        ws2, hws2 = _out(ops.deform_conv_wgrad_workspace_bytes(N, H, W, Cin, Cout), None, torch.uint8, "wgrad workspace")
        dx, hdx = _out(M, Cin, torch.bfloat16, "d_x")
        dom, hdom = _out(M, ld, torch.bfloat16, "d_om")
        dw, hdw = _out(Cout * 9, Cin, torch.float32, "d_w")
        db, hdb = _out(Cout, None, torch.float32, "d_bias")
        ops.deform_conv_bwd_data(tx, tom, tdy, wd, dx, dom, ws1, N, H, W, Cin, Cout, modulated, add=tadd if r == 0 else None)
        ops.deform_conv_wgrad(tx, tom, tdy, dw, db, ws2, N, H, W, Cin, Cout, modulated)
        torch.cuda.synchronize()
        for h in (hws1, hws2, hdx, hdom, hdw, hdb):
            h.check()
        out = dict(d_x=dx.cpu(), d_om=dom.cpu(), d_w=dw.cpu().view(Cout, 3, 3, Cin), d_b=db.cpu())
        if r == 1:          # accumulate: a second launch into the same d_w / d_bias doubles them
            ops.deform_conv_wgrad(tx, tom, tdy, dw, db, ws2, N, H, W, Cin, Cout, modulated, accumulate=True)
            torch.cuda.synchronize()
            hdw.check(), hdb.check()
            out["d_w_twice"], out["d_b_twice"] = dw.cpu().view(Cout, 3, 3, Cin), db.cpu()
        runs.append(out)
    for h in handles:
        h.assert_unchanged()
    res["runs"] = runs
    res["add"] = add.double()
    res["bias"] = bias
    res["x64"], res["w64"] = x.double(), wf.float().cpu().double().view(Cout, 3, 3, Cin)
    res["ref"] = O.oracle(x.view(N, H, W, Cin), om.view(N, H, W, ld), wf.float().cpu().view(Cout, 3, 3, Cin), bias, dy.view(N, H, W, Cout),
                          modulated)
    return res


def _worst(got, ref, S, rel, abs_s, what):
    r = float(bound_ratio(got.reshape(ref.shape), ref, S, rel, abs_s).max())
    print(f"{what}: worst error / bound = {r:.3f}")
    return r


CASES = [(s, f, m) for s in SHAPES for f in FAMILIES for m in (False, True)]
IDS = ["x".join(map(str, s)) + f"-{f}-" + ("dcnv2" if m else "dcnv1") for s, f, m in CASES]


@pytest.mark.parametrize("shape,family,modulated", CASES, ids=IDS)
def test_forward(shape, family, modulated):
    c = _case(shape, family, modulated)
    ref = c["ref"]
    assert _worst(c["y"], ref["y"], ref["S_y"], REL, ABS_FWD, "y") <= 1.0
    assert torch.equal(c["y"].view(torch.int16), c["y2"].view(torch.int16)), "y differs between two runs"
    if family == "outside":
        want = c["bias"].to(torch.bfloat16).expand_as(c["y"])
        assert torch.equal(c["y"].view(torch.int16), want.contiguous().view(torch.int16)), "every sample is outside: y must be bias exactly"
    if family == "zero":        # the plain 3x3 convolution (mask = sigmoid(30) = 1 - 1e-13)
        N, H, W, Cin, Cout = shape
        plain = TF.conv2d(c["x64"].view(N, H, W, Cin).permute(0, 3, 1, 2), c["w64"].permute(0, 3, 1, 2), c["bias"].double(),
                          padding=1).permute(0, 2, 3, 1)
        assert _worst(c["y"], plain, ref["S_y"], REL, ABS_FWD, "y vs conv2d") <= 1.0


@pytest.mark.parametrize("shape,family,modulated", CASES, ids=IDS)
def test_data_gradients(shape, family, modulated):
    c = _case(shape, family, modulated)
    ref = c["ref"]
    N, H, W, Cin, Cout = shape
    for r, run in enumerate(c["runs"]):
        add = c["add"].view(N, H, W, Cin) if r == 0 else torch.zeros(N, H, W, Cin, dtype=torch.float64)
        assert _worst(run["d_x"], ref["d_x"] + add, ref["S_d_x"] + add.abs(), REL, ABS_BWD, f"d_x (run {r})") <= 1.0
        assert _worst(run["d_om"], ref["d_om"], ref["S_d_om"], REL, ABS_BWD, f"d_om (run {r})") <= 1.0
        pad = run["d_om"][:, (27 if modulated else 18):]
        assert int(pad.view(torch.int16).count_nonzero()) == 0, "the pad channels' gradient must be +0"
    a, b = c["runs"]
    assert torch.equal(a["d_om"].view(torch.int16), b["d_om"].view(torch.int16)), "d_om differs between two runs"
    if family == "outside":
        assert int(b["d_x"].view(torch.int16).count_nonzero()) == 0 and int(b["d_om"].view(torch.int16).count_nonzero()) == 0, \
            "every sample is outside: d_x and d_om must be exactly +0"


@pytest.mark.parametrize("shape,family,modulated", CASES, ids=IDS)
def test_weight_gradients(shape, family, modulated):
    c = _case(shape, family, modulated)
    ref = c["ref"]
    for r, run in enumerate(c["runs"]):
        assert _worst(run["d_w"], ref["d_w"], ref["S_d_w"], 2.0 ** -24, ABS_FWD, f"d_w (run {r})") <= 1.0
        # d_bias sums exact bf16 values in fp32: only the accumulation term
        assert _worst(run["d_b"], ref["d_b"], ref["S_d_b"], 2.0 ** -24, 2.0 ** -16, f"d_bias (run {r})") <= 1.0
    a, b = c["runs"]
    assert torch.equal(a["d_w"].view(torch.int32), b["d_w"].view(torch.int32)), "d_w differs between two runs"
    assert torch.equal(a["d_b"].view(torch.int32), b["d_b"].view(torch.int32)), "d_bias differs between two runs"
    # accumulate: v + v in fp32 is exact
    assert torch.equal(b["d_w_twice"], 2 * b["d_w"]) and torch.equal(b["d_b_twice"], 2 * b["d_b"])


# ---- the layers ----------------------------------------------------------------------------------------------------------------------------
LAYER_SHAPE = (2, 13, 21, 72, 40)


@functools.lru_cache(maxsize=None)
def _layer_case(modulated):
    import basedet.layers as BL
    from basedet_amd import ops
    N, H, W, Cin, Cout = LAYER_SHAPE
    cls = BL.ModulatedDeformConvWithOff if modulated else BL.DeformConvWithOff
    layer = cls(Cin, Cout, seed=3)
    g = torch.Generator().manual_seed(77 + int(modulated))
    sd = layer.state_dict()
    off, dcn = layer.OFFSET_NAME, layer.DCN_NAME
    sd[off + ".bias"] = 0.5 * torch.randn(sd[off + ".bias"].shape, generator=g)          # (the default init's biases are zero)
    sd[dcn + ".bias"] = torch.randn(sd[dcn + ".bias"].shape, generator=g)
    layer.load_state_dict(sd)
    x = bf16_round(2.0 * torch.randn(N, Cin, H, W, generator=g))
    dy = bf16_round(torch.randn(N, Cout, H, W, generator=g))
    y = layer(x.cuda()).cpu()
    om_gpu = layer.last_offset_mask.clone()
    dx = layer.backward(dy.cuda()).cpu()
    grads = {k: v.cpu() for k, v in layer.grads().items()}
    layer.backward(dy.cuda(), accumulate=True)
    grads2 = {k: v.cpu() for k, v in layer.grads().items()}
    return dict(layer=layer, sd=sd, x=x, dy=dy, y=y, om_gpu=om_gpu, dx=dx, grads=grads, grads2=grads2, ops=ops)


@pytest.mark.parametrize("modulated", [False, True], ids=["dcnv1", "dcnv2"])
def test_layer_offset_conv_and_state_dict(modulated):
    c = _layer_case(modulated)
    layer, ops, sd = c["layer"], c["ops"], c["sd"]
    N, H, W, Cin, Cout = LAYER_SHAPE
    K, ld = (27, 32) if modulated else (18, 24)
    assert sorted(sd) == sorted(layer.names()) and tuple(sd[layer.OFFSET_NAME + ".weight"].shape) == (K, Cin, 3, 3)
    assert tuple(sd[layer.DCN_NAME + ".weight"].shape) == (Cout, Cin, 3, 3)
    # the offset convolution, run directly: its K rows padded with zero rows to ld
    w = torch.zeros(ld, Cin, 3, 3)
    w[:K] = sd[layer.OFFSET_NAME + ".weight"]
    b = torch.zeros(ld)
    b[:K] = sd[layer.OFFSET_NAME + ".bias"]
    wf, _ = util.pack_weights(ops, w)
    geom = ops.single(N, H, W)
    om = torch.empty((N * H * W, ld), dtype=torch.bfloat16, device="cuda")
    ops.conv2d_fwd(ops.conv_desc(geom, geom, Cin, ld, 3, 3, 1, 1), util.nchw_to_pm(c["x"]), wf, b.cuda(), om)
    assert c["om_gpu"].dtype == torch.bfloat16 and tuple(c["om_gpu"].shape) == (N * H * W, ld)
    assert torch.equal(om.view(torch.int16), c["om_gpu"].view(torch.int16)), "last_offset_mask is not the padded offset conv's output"
    # a second instance (other seed) that loads the state reproduces the output bit for bit
    other = type(layer)(Cin, Cout, seed=11)
    assert not torch.equal(other(c["x"].cuda()).cpu(), c["y"])
    other.load_state_dict(layer.state_dict())
    assert torch.equal(other(c["x"].cuda()).cpu(), c["y"])


@pytest.mark.parametrize("modulated", [False, True], ids=["dcnv1", "dcnv2"])
def test_layer_against_composed_oracle(modulated):
    """om = conv64(x); om_used = om + (om_gpu - om).detach(): the sampling positions the GPU used, gradients still flowing through the
    offset convolution.  The deformable part keeps the operator bounds.  What passes through the bf16 d_om propagates linearly: with
    tol_om = 2^-8 |d_om| + 2^-8 S_d_om (d_om's bound), the offset conv's weight gradient may be off by sum |x| tol_om, its bias gradient
    by sum tol_om and its data gradient by sum |w_off| tol_om, each plus the 2^-16 fp32 accumulation term of that convolution on
    (|d_om| + tol_om) and the output's own rounding (2^-24 |ref| fp32; 2^-8 |ref| for the bf16 d_x, whose deformable part was rounded to
    bf16 once before: + 2^-8 |d_x part| + 2^-8 S_d_x)."""
    c = _layer_case(modulated)
    layer, sd = c["layer"], c["sd"]
    N, H, W, Cin, Cout = LAYER_SHAPE
    K, ld = (27, 32) if modulated else (18, 24)
    off, dcn = layer.OFFSET_NAME, layer.DCN_NAME
    x = c["x"].double().requires_grad_(True)
    w_off = bf16_round(sd[off + ".weight"]).double().requires_grad_(True)
    b_off = sd[off + ".bias"].double().requires_grad_(True)
    w_dcn = bf16_round(sd[dcn + ".weight"]).double().requires_grad_(True)
    b_dcn = sd[dcn + ".bias"].double().requires_grad_(True)
    om = TF.conv2d(x, w_off, b_off, padding=1).permute(0, 2, 3, 1)
    om = torch.cat([om, torch.zeros(N, H, W, ld - K, dtype=torch.float64)], -1)
    om_gpu = c["om_gpu"].cpu().double().view(N, H, W, ld)
    om_used = om + (om_gpu - om).detach()
    xn, wn = x.permute(0, 2, 3, 1), w_dcn.permute(0, 2, 3, 1)
    y = O.forward(xn, om_used, wn, b_dcn, modulated)
    dyn = c["dy"].double().permute(0, 2, 3, 1)
    gx, gwo, gbo, gwd, gbd = torch.autograd.grad(y, [x, w_off, b_off, w_dcn, b_dcn], dyn)
    r = O.oracle(xn, om_gpu, wn, b_dcn, dyn, modulated)

    def nchw(t):
        return t.permute(0, 3, 1, 2)
    assert _worst(nchw_pm(c["y"]), y.detach(), r["S_y"], REL, ABS_FWD, "layer y") <= 1.0
    got = c["grads"]
    assert _worst(got[dcn + ".weight"], gwd, nchw(r["S_d_w"]), 2.0 ** -24, ABS_FWD, "dcn weight gradient") <= 1.0
    assert _worst(got[dcn + ".bias"], gbd, r["S_d_b"], 2.0 ** -24, 2.0 ** -16, "dcn bias gradient") <= 1.0
    d_om = nchw(r["d_om"])[:, :K]
    tol_om = nchw(REL * r["d_om"].abs() + ABS_BWD * r["S_d_om"])[:, :K]
    big = d_om.abs() + tol_om
    xa, wa = x.detach().abs(), w_off.detach().abs()
    e_w = torch.nn.grad.conv2d_weight(xa, w_off.shape, tol_om, padding=1) + 2.0 ** -16 * torch.nn.grad.conv2d_weight(xa, w_off.shape, big, padding=1)
    assert _worst(got[off + ".weight"], gwo, e_w, 2.0 ** -24, 1.0, "offset conv weight gradient") <= 1.0
    e_b = tol_om.sum((0, 2, 3)) + 2.0 ** -16 * big.sum((0, 2, 3))
    assert _worst(got[off + ".bias"], gbo, e_b, 2.0 ** -24, 1.0, "offset conv bias gradient") <= 1.0
    e_x = TF.conv_transpose2d(tol_om, wa, padding=1) + 2.0 ** -16 * TF.conv_transpose2d(big, wa, padding=1) \
        + REL * nchw(r["d_x"]).abs() + ABS_BWD * nchw(r["S_d_x"])
    assert _worst(c["dx"], gx, e_x, REL, 1.0, "layer d_x") <= 1.0
    # accumulate: the second backward adds the same (reproducible) gradients
    for k, v in c["grads2"].items():
        assert bool(((v.double() - 2 * got[k].double()).abs() <= 2.0 ** -23 * (2 * got[k].double()).abs()).all()), k


def nchw_pm(t):
    """NCHW fp32 -> NHWC (the oracle's layout)."""
    return t.permute(0, 2, 3, 1)


# ---- one storage path: a layer on its own storage and one adopt()ed onto a caller's -------------------------------------------------------
def _pair(modulated, seed=3):
    """Two layers of one seed at LAYER_SHAPE: `own` on the storage it allocated, `ad` adopted onto flat fp32 tensors."""
    import basedet.layers as BL
    _, _, _, Cin, Cout = LAYER_SHAPE
    cls = BL.ModulatedDeformConvWithOff if modulated else BL.DeformConvWithOff
    own, ad = cls(Cin, Cout, seed=seed), cls(Cin, Cout, seed=seed)
    w_flat, g_flat, w, g = util.flat_storage(ad.arena_shapes())
    ad.adopt(w, g)
    return own, ad, w_flat, g_flat


def _other_state(layer, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in layer.state_dict().items()}


@pytest.mark.parametrize("modulated", [False, True], ids=["dcnv1", "dcnv2"])
def test_layer_standalone_equals_adopted(modulated):
    """The same forward and backward on both: y and every entry of grads() are the same bits -- the offset convolution's gradients are
    bd_conv2d_wgrad_bias of d_om, which repeats bit for bit (above).  Only d_x, which bd_deform_conv_bwd_data sums with fp32 atomics
    (DESIGN 4t), is held to the rel-L2 bound of two runs of one build, 2^-10
    (tests/test_centernet_model_gpu.py::test_neck_and_head_gradients_in_the_arena)."""
    c = _layer_case(modulated)
    own, ad, w_flat, g_flat = _pair(modulated)
    x, dy = c["x"].cuda(), c["dy"].cuda()
    ya, yb = own(x), ad(x)
    assert torch.equal(ya, yb)
    da, db = own.backward(dy), ad.backward(dy)
    ga, gb = own.grads(), ad.grads()
    assert list(ga) == list(gb) == own.names()
    for k in ga:
        assert ga[k].shape == gb[k].shape and torch.equal(ga[k], gb[k]), k
    assert util.rel_l2(da, db) <= 2.0 ** -10
    assert all(util.lies_inside(t, g_flat) for t in ad._store.g.values()) and all(util.lies_inside(t, w_flat) for t in ad.params().values())
    assert not any(bool(torch.isnan(t).any()) for t in ad._store.g.values()), "a backward writes every gradient element, pad rows included"


@pytest.mark.parametrize("adopted", [False, True], ids=["own", "adopted"])
@pytest.mark.parametrize("modulated", [False, True], ids=["dcnv1", "dcnv2"])
def test_layer_loads_and_repacks_in_place(modulated, adopted):
    """load_state_dict() copies into the masters (a params() view taken before shows the loaded values, at the same address) and the next
    forward is that of a fresh layer loaded with the same state; repack() writes the bf16 operands where they are, and after an in-place
    change through params() gives the forward of a fresh layer loaded with the changed state."""
    c = _layer_case(modulated)
    own, ad, _, _ = _pair(modulated)
    layer, x = (ad if adopted else own), c["x"].cuda()
    held = layer.params()
    ptrs = {k: v.data_ptr() for k, v in held.items()}
    state = _other_state(layer, 5)
    layer.load_state_dict(state)
    assert {k: v.data_ptr() for k, v in layer.params().items()} == ptrs
    assert all(torch.equal(held[k].cpu(), state[k]) for k in state)
    fresh = type(layer)(*LAYER_SHAPE[3:], seed=11)
    fresh.load_state_dict(state)
    assert torch.equal(layer(x), fresh(x))
    packed = [layer._off_wf, layer._off_wd, layer._dcn_wf, layer._dcn_wd]
    where = [t.data_ptr() for t in packed]
    for k, v in held.items():
        v.mul_(0.5 if k.endswith(".weight") else -1.0)
    layer.repack()
    assert [t.data_ptr() for t in (layer._off_wf, layer._off_wd, layer._dcn_wf, layer._dcn_wd)] == where
    fresh.load_state_dict(layer.state_dict())
    assert torch.equal(layer(x), fresh(x)) and not torch.equal(layer.state_dict()[layer.DCN_NAME + ".weight"], state[layer.DCN_NAME + ".weight"])
