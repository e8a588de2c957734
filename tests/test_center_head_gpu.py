"""csrc/center_head.hip (bd_center_head_out_fwd / _bwd) and basedet.layers.CenternetDeconv / CenterHead against the float64 oracle of
tests/center_head_oracle.py.

The fused kernel: every operand in a util.guarded allocation, every launch twice and compared bit for bit.  Bounds (util.bound_ratio <= 1,
tol = rel |ref| + abs_s S, S = the sum of the magnitudes of the result's terms; the forms of tests/test_deform_conv_gpu.py):
  bf16 results (logits, wr, d_feat): rel = 2^-8 (their own rounding), abs_s = 2^-16 (fp32 accumulation of exact bf16 products);
  fp32 results (dw, db): rel = 2^-24, abs_s = 2^-16.

The layers: stage by stage from the saved pixel-major intermediates, each stage's oracle fed the device's own input of that stage; then the
wiring end to end through the loss kernels, and a short training run (docstrings below)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import center_head_oracle as O
import util
from util import bf16_round, bound_ratio, guarded

pytestmark = pytest.mark.gpu

REL16, REL32, ACC = 2.0 ** -8, 2.0 ** -24, 2.0 ** -16
BF, F32 = torch.bfloat16, torch.float32
# M: no tile size (16, 32, 64) divides 1, 70 = 2 * 5 * 7 or 4099 (prime; more than one workgroup in both directions)
KERNEL_CASES = [(M, 64, K) for M in (1, 70, 4099) for K in (1, 20, 80, 365)] + [(M, 16, 3) for M in (1, 70, 4099)]


def _in(data, dtype, name):
    rows, cols = (data.shape[0], None) if data.dim() == 1 else data.shape
    t, h = guarded(rows, cols, dtype, "cuda", fill="nan", name=name)
    h.set(data.to(dtype))
    h.snapshot()
    return t, h


def _out(rows, cols, dtype, name):
    return guarded(rows, cols, dtype, "cuda", fill="sentinel", name=name)


def _worst(got, ref, S, rel, abs_s, what, exact=None):
    r = float(bound_ratio(got.reshape(ref.shape), ref, S, rel, abs_s, exact).max())
    print(f"{what}: worst error / bound = {r:.3f}")
    return r


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@functools.lru_cache(maxsize=None)
def _kernel_case(M, C, K):
    from basedet_amd import ops
    g = torch.Generator().manual_seed(M * 1000 + C * 7 + K)
    ld = (K + 7) // 8 * 8
    feat = bf16_round(torch.relu(torch.randn(M, 3 * C, generator=g)))
    ws = [torch.randn(n, C, generator=g) * C ** -0.5 for n in (K, 2, 2)]
    bs = [torch.randn(n, generator=g) for n in (K, 2, 2)]
    d_logits = bf16_round(torch.randn(M, ld, generator=g))
    d_wr = bf16_round(torch.randn(M, 8, generator=g))
    ins = [_in(feat, BF, "feat")] + [_in(w, F32, f"w{i}") for i, w in enumerate(ws)] + [_in(b, F32, f"b{i}") for i, b in enumerate(bs)] \
        + [_in(d_logits, BF, "d_logits"), _in(d_wr, BF, "d_wr")]
    tf, tw0, tw1, tw2, tb0, tb1, tb2, tdl, tdw = (t for t, _ in ins)
    # the same gradients with NaN bit patterns in the pad slots (>= K, 4-7)
    nan_logits, nan_wr = d_logits.clone(), d_wr.clone()
    nan_logits[:, K:] = float("nan")
    nan_wr[:, 4:] = float("nan")
    (tdl_nan, hn1), (tdw_nan, hn2) = _in(nan_logits, BF, "d_logits (NaN pads)"), _in(nan_wr, BF, "d_wr (NaN pads)")

    res = dict(K=K, C=C, M=M, ld=ld)
    fwd = []
    for r in range(2):
        logits, hl = _out(M, ld, BF, "logits")
        wr, hw = _out(M, 8, BF, "wr")
        ops.center_head_out_fwd(tf, tw0, tb0, tw1, tb1, tw2, tb2, M, C, K, logits, wr)
        torch.cuda.synchronize()
        hl.check(), hw.check()
        fwd.append((logits.cpu(), wr.cpu()))
    res["fwd"] = fwd
    logits, _ = _out(M, ld, BF, "logits (no bias)")
    wr, _ = _out(M, 8, BF, "wr (no bias)")
    ops.center_head_out_fwd(tf, tw0, None, tw1, None, tw2, None, M, C, K, logits, wr)
    res["fwd_nobias"] = (logits.cpu(), wr.cpu())

    nbytes = ops.center_head_out_bwd_workspace_bytes(M, C, K)
    assert nbytes > 0
    runs = []
    for r in range(3):          # 0, 1: the same launch twice; 2: NaN pads
        ws_, hws = _out(nbytes, None, torch.uint8, "workspace")
        df, hdf = _out(M, 3 * C, BF, "d_feat")
        outs = [_out(n, c, F32, nm) for nm, n, c in (("dw_cls", K, C), ("db_cls", K, None), ("dw_wh", 2, C), ("db_wh", 2, None),
                                                     ("dw_reg", 2, C), ("db_reg", 2, None))]
        gl, gw = (tdl_nan, tdw_nan) if r == 2 else (tdl, tdw)
        ops.center_head_out_bwd(tf, gl, gw, tw0, tw1, tw2, M, C, K, df, *[t for t, _ in outs], ws_)
        torch.cuda.synchronize()
        for h in [hws, hdf] + [h for _, h in outs]:
            h.check()
        run = dict(d_feat=df.cpu(), grads=[t.cpu().clone() for t, _ in outs])
        if r == 1:              # accumulate: a second launch into the same buffers doubles them (v + v is exact)
            ops.center_head_out_bwd(tf, gl, gw, tw0, tw1, tw2, M, C, K, df, *[t for t, _ in outs], ws_, accumulate=True)
            torch.cuda.synchronize()
            for h in [hws, hdf] + [h for _, h in outs]:
                h.check()
            run["twice"] = [t.cpu().clone() for t, _ in outs]
        runs.append(run)
    for _, h in ins + [(None, hn1), (None, hn2)]:
        h.assert_unchanged()
    res["runs"] = runs
    res["feat"] = feat
    res["ref"] = O.head_out(feat, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], d_logits[:, :K], d_wr[:, :4])
    res["ref_nobias"] = O.head_out(feat, ws[0], None, ws[1], None, ws[2], None)
    return res


IDS = [f"M{m}-C{c}-K{k}" for m, c, k in KERNEL_CASES]


@pytest.mark.parametrize("M,C,K", KERNEL_CASES, ids=IDS)
def test_fused_forward(M, C, K):
    c = _kernel_case(M, C, K)
    for (logits, wr), ref, tag in ((c["fwd"][0], c["ref"], ""), (c["fwd_nobias"], c["ref_nobias"], " (no bias)")):
        assert _worst(logits[:, :K], ref["logits"], ref["S_logits"], REL16, ACC, "logits" + tag) <= 1.0
        assert _worst(wr[:, :4], ref["wr"], ref["S_wr"], REL16, ACC, "wr" + tag) <= 1.0
        assert int(_bits(logits[:, K:]).count_nonzero()) == 0 and int(_bits(wr[:, 4:]).count_nonzero()) == 0, "pad slots must be +0"
    (l0, w0), (l1, w1) = c["fwd"]
    assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(_bits(w0), _bits(w1)), "forward differs between two runs"


@pytest.mark.parametrize("M,C,K", KERNEL_CASES, ids=IDS)
def test_fused_backward(M, C, K):
    c = _kernel_case(M, C, K)
    ref = c["ref"]
    a, b, n = c["runs"]
    assert _worst(a["d_feat"], ref["d_feat"], ref["S_d_feat"], REL16, ACC, "d_feat", exact=ref["closed"]) <= 1.0
    assert int(_bits(a["d_feat"])[c["feat"] == 0].count_nonzero()) == 0, "d_feat must be +0 where feat is 0"
    names = ("dw_cls", "db_cls", "dw_wh", "db_wh", "dw_reg", "db_reg")
    for name, got in zip(names, a["grads"]):
        assert _worst(got, ref[name], ref["S_" + name], REL32, ACC, name) <= 1.0
    assert torch.equal(_bits(a["d_feat"]), _bits(b["d_feat"])), "d_feat differs between two runs"
    assert torch.equal(_bits(a["d_feat"]), _bits(n["d_feat"])), "NaN bit patterns in the pad slots changed d_feat"
    for name, x, y, z, tw in zip(names, a["grads"], b["grads"], n["grads"], b["twice"]):
        assert torch.equal(_bits(x), _bits(y)), f"{name} differs between two runs"
        assert torch.equal(_bits(x), _bits(z)), f"NaN bit patterns in the pad slots changed {name}"
        assert torch.equal(tw, 2 * x), f"{name}: accumulate must add to the previous gradient"


def test_fused_refuses_unbuilt_shapes():
    from basedet_amd import ops
    from basedet_amd._lib import BasedetHipError
    M = 64
    mk = lambda *s, dt=BF: torch.zeros(s, dtype=dt, device="cuda")
    for C, K, ld in ((24, 8, 8), (144, 8, 8), (64, 8, 16), (64, 2000, 2000), (128, 365, 368)):
        with pytest.raises(BasedetHipError, match="center_head_out"):
            ops.center_head_out_fwd(mk(M, 3 * C), mk(K, C, dt=F32), None, mk(2, C, dt=F32), None, mk(2, C, dt=F32), None, M, C, K,
                                    mk(M, ld), mk(M, 8)) if (C, K) != (128, 365) else \
                ops.center_head_out_bwd(mk(M, 3 * C), mk(M, ld), mk(M, 8), mk(K, C, dt=F32), mk(2, C, dt=F32), mk(2, C, dt=F32), M, C, K,
                                        mk(M, 3 * C), mk(K, C, dt=F32), None, mk(2, C, dt=F32), None, mk(2, C, dt=F32), None,
                                        mk(1 << 20, dt=torch.uint8))
    assert ops.center_head_out_bwd_workspace_bytes(M, 24, 8) == 0


# ---- the layers ------------------------------------------------------------------------------------------------------------------------------
ABS_DCN = 2.0 ** -9 + 2.0 ** -16          # tests/test_deform_conv_gpu.py: one bf16 rounding of the sampled operand plus fp32 accumulation


def _nhwc(t, n, h, w):
    return t.float().cpu().view(n, h, w, -1)


@functools.lru_cache(maxsize=None)
def _model_case(K, modulated):
    """Neck + head on the shared problem: one training forward, the loss kernels, one backward.  Everything the tests read is kept."""
    import basedet.layers as BL
    from basedet_amd import ops
    x, gt, num, tgt = O.problem(K)
    p0 = O.init_params(K, modulated)
    neck = BL.CenternetDeconv(O.CHANNELS, O.KERNELS, modulated)
    head = BL.CenterHead(O.CHANNELS[-1], K)
    neck.load_state_dict({k: v for k, v in p0.items() if k.startswith("deconv")})
    head.load_state_dict({k: v for k, v in p0.items() if "_head." in k})
    N, H, W, T = O.N, 4 * O.H0, 4 * O.W0, O.T
    M = N * H * W
    dev = "cuda"
    t = ops.centernet_targets(torch.from_numpy(gt).to(dev), torch.from_numpy(num).to(dev), K, H, W, T, 0.25, 0.7)

    def step():
        f = neck.forward_pm(util.nchw_to_pm(x), N, O.H0, O.W0)
        logits, wr = head.forward_pm(f, N, H, W)
        loss = torch.zeros(1, dtype=F32, device=dev)
        d_logits = torch.empty_like(logits)
        ops.centernet_focal_fwd_bwd(logits, t["score_map"], M, K, logits.shape[1], t["num_pos"], 1.0, 1.0, loss, d_logits)
        d_wh, d_reg = torch.empty_like(wr), torch.empty_like(wr)      # each call writes all of its buffer: two buffers, then summed
        ops.centernet_l1_fwd_bwd(wr, 8, 0, t["index"], t["reg_mask"], t["wh"], N, H, W, T, 0.1, 1.0, loss, d_wh)
        ops.centernet_l1_fwd_bwd(wr, 8, 2, t["index"], t["reg_mask"], t["reg"], N, H, W, T, 1.0, 1.0, loss, d_reg)
        d_wr = ops.add_bf16(d_wh, d_reg, torch.empty_like(wr))
        g_f = head.backward_pm(d_logits, d_wr)
        neck.backward_pm(g_f)
        return f, logits, wr, float(loss.cpu()), d_logits, d_wr, g_f
    f, logits, wr, loss, d_logits, d_wr, g_f = step()
    torch.cuda.synchronize()
    grads = {k: v.cpu().clone() for k, v in {**neck.grads(), **head.grads()}.items()}
    stages = [{k: v.clone() for k, v in l.stages.items()} for _, l in neck.layers()]
    sgrads = [{k: v.clone() for k, v in l.stage_grads.items()} for _, l in neck.layers()]
    oms = [l.dcn.last_offset_mask.clone() for _, l in neck.layers()]
    bn = [{n: dict(mean=b.mean.cpu().clone(), inv_std=b.inv_std.cpu().clone(), g=dict((k, v.cpu().clone()) for k, v in b.g.items()))
           for n, b in (("dcn_bn", l.dcn_bn), ("up_bn", l.up_bn))} for _, l in neck.layers()]
    state1 = {**neck.state_dict(), **head.state_dict()}
    return dict(neck=neck, head=head, ops=ops, x=x, tgt=tgt, p0=p0, f=f.clone(), logits=logits.clone(), wr=wr.clone(), loss=loss,
                d_logits=d_logits.clone(), d_wr=d_wr.clone(), g_f=g_f.clone(), grads=grads, stages=stages, sgrads=sgrads, oms=oms, bn=bn,
                state1=state1, feat=head.feat_pm.clone(), d_feat=head.d_feat_pm.clone(), step=step, K=K, modulated=modulated)


MODEL_CASES = [(80, True), (3, False)]
MODEL_IDS = ["K80-dcnv2", "K3-dcnv1"]


@pytest.mark.parametrize("K,modulated", MODEL_CASES, ids=MODEL_IDS)
def test_neck_stage_by_stage(K, modulated):
    """Every stage of both DeconvLayers against float64 on the device's own input of that stage.
    dcn: the operator bounds of tests/test_deform_conv_gpu.py (y, d_w, d_bias; its d_x is covered there and by the wiring test).
    norms: tests/test_batchnorm_gpu.py's conventions -- statistics within 1e-5 (|mu| + sigma) / 1e-4 var, the apply and the backward apply
    within one bf16 step of the float64 formula on the kernel's own statistics, dgamma / dbeta within 1e-5 of the sum of |terms|.
    up_sample: a bf16 result of an fp32 accumulation (2^-8 |ref| + 2^-16 S); its weight gradient fp32 (2^-24 |ref| + 2^-16 S)."""
    import deform_conv_oracle as DO
    c = _model_case(K, modulated)
    N = O.N
    off, dcn = O.dcn_names(modulated)
    for i, (st, sg, om, bn) in enumerate(zip(c["stages"], c["sgrads"], c["oms"], c["bn"])):
        pre = f"deconv{i + 1}"
        H, W = O.H0 * 2 ** i, O.W0 * 2 ** i
        Cin, C = O.CHANNELS[i], O.CHANNELS[i + 1]
        p = c["p0"]
        # dcn
        w = bf16_round(p[f"{pre}.dcn.{dcn}.weight"]).permute(0, 2, 3, 1)
        r = DO.oracle(_nhwc(st["x"], N, H, W), _nhwc(om, N, H, W), w, p[f"{pre}.dcn.{dcn}.bias"], _nhwc(sg["dcn"], N, H, W), modulated)
        assert _worst(_nhwc(st["dcn"], N, H, W), r["y"], r["S_y"], REL16, ABS_DCN, pre + " dcn y") <= 1.0
        assert _worst(c["grads"][f"{pre}.dcn.{dcn}.weight"].permute(0, 2, 3, 1), r["d_w"], r["S_d_w"], REL32, ABS_DCN, pre + " dcn d_w") <= 1.0
        assert _worst(c["grads"][f"{pre}.dcn.{dcn}.bias"], r["d_b"], r["S_d_b"], REL32, ACC, pre + " dcn d_b") <= 1.0
        # the two norms (+ ReLU)
        for name, yk, Hn, Wn in (("dcn_bn", "dcn", H, W), ("up_bn", "up_sample", 2 * H, 2 * W)):
            y64 = st[yk].double().cpu().numpy()
            Mn = y64.shape[0]
            mu, var = y64.mean(0), y64.var(0)
            sig = np.sqrt(var)
            mean, inv = bn[name]["mean"].double().numpy(), bn[name]["inv_std"].double().numpy()
            assert np.all(np.abs(mean - mu) <= 1e-5 * (np.abs(mu) + sig)), name
            assert np.all(np.abs(1.0 / inv ** 2 - O.EPS - var) <= 1e-4 * var), name
            gam, bet = p[f"{pre}.{name}.weight"].double().numpy(), p[f"{pre}.{name}.bias"].double().numpy()
            rm_ref = 0.9 * p[f"{pre}.{name}.running_mean"].double().numpy() + 0.1 * mu
            rv_ref = 0.9 * p[f"{pre}.{name}.running_var"].double().numpy() + 0.1 * var * Mn / (Mn - 1)
            assert np.all(np.abs(c["state1"][f"{pre}.{name}.running_mean"].double().numpy() - rm_ref) <= 1e-5 * (np.abs(mu) + sig))
            assert np.all(np.abs(c["state1"][f"{pre}.{name}.running_var"].double().numpy() - rv_ref) <= 1e-4 * rv_ref)
            xh = (y64 - mean) * inv
            zr = torch.relu(torch.from_numpy(gam * xh + bet).to(BF).double())          # one rounding, then the ReLU
            z = st[name].cpu()
            assert int(util.bf16_ulps(z, zr).max()) <= 1, f"{pre}.{name} apply"
            g = sg[name].double().cpu().numpy() * (z.double().numpy() > 0)
            dg, db = bn[name]["g"]["weight"].double().numpy(), bn[name]["g"]["bias"].double().numpy()
            assert np.all(np.abs(dg - (g * xh).sum(0)) <= 1e-5 * np.abs(g * xh).sum(0) + 1e-30), f"{pre}.{name} dgamma"
            assert np.all(np.abs(db - g.sum(0)) <= 1e-5 * np.abs(g).sum(0) + 1e-30), f"{pre}.{name} dbeta"
            gr = gam * inv * (g - db / Mn - xh * dg / Mn)
            assert int(util.bf16_ulps(sg[yk].cpu(), torch.from_numpy(gr)).max()) <= 1, f"{pre}.{name} backward apply"
        # up_sample
        wu = bf16_round(p[f"{pre}.up_sample.weight"]).double()
        z0 = _nhwc(st["dcn_bn"], N, H, W).double().permute(0, 3, 1, 2)
        gy = _nhwc(sg["up_sample"], N, 2 * H, 2 * W).double().permute(0, 3, 1, 2)
        ref, S = TF.conv_transpose2d(z0, wu, stride=2, padding=1), TF.conv_transpose2d(z0.abs(), wu.abs(), stride=2, padding=1)
        assert _worst(_nhwc(st["up_sample"], N, 2 * H, 2 * W).permute(0, 3, 1, 2), ref, S, REL16, ACC, pre + " up_sample y") <= 1.0
        ref, S = TF.conv2d(gy, wu, stride=2, padding=1), TF.conv2d(gy.abs(), wu.abs(), stride=2, padding=1)
        assert _worst(_nhwc(sg["dcn_bn"], N, H, W).permute(0, 3, 1, 2), ref, S, REL16, ACC, pre + " up_sample d_x") <= 1.0
        # weight (in, out, 4, 4) of the transposed convolution = the OIHW weight of the fine -> coarse convolution
        ref = torch.nn.grad.conv2d_weight(gy, wu.shape, z0, stride=2, padding=1)
        S = torch.nn.grad.conv2d_weight(gy.abs(), wu.shape, z0.abs(), stride=2, padding=1)
        assert _worst(c["grads"][f"{pre}.up_sample.weight"], ref, S, REL32, ACC, pre + " up_sample d_w") <= 1.0


@pytest.mark.parametrize("K,modulated", MODEL_CASES, ids=MODEL_IDS)
def test_head_stage_by_stage(K, modulated):
    """feat_conv (one 3C-row launch) and the fused output kernel inside the layer, each on the device's own input; the parameter
    gradients under the reference's names."""
    c = _model_case(K, modulated)
    p, N, H, W, C = c["p0"], O.N, 4 * O.H0, 4 * O.W0, O.CHANNELS[-1]
    f = _nhwc(c["f"], N, H, W).double().permute(0, 3, 1, 2)
    wf = torch.cat([bf16_round(p[f"{b}_head.feat_conv.weight"]) for b in ("cls", "wh", "reg")], 0).double()
    bf = torch.cat([p[f"{b}_head.feat_conv.bias"] for b in ("cls", "wh", "reg")], 0).double()
    ref = torch.relu(TF.conv2d(f, wf, bf, padding=1))
    S = TF.conv2d(f.abs(), wf.abs(), bf.abs(), padding=1)
    feat = _nhwc(c["feat"], N, H, W).permute(0, 3, 1, 2)
    assert _worst(feat, ref, S, REL16, ACC, "feat") <= 1.0
    r = O.head_out(c["feat"].float().cpu(), *[t for b in ("cls", "wh", "reg") for t in (p[f"{b}_head.out_conv.weight"].view(-1, C),
                                                                                       p[f"{b}_head.out_conv.bias"])],
                   c["d_logits"].float().cpu()[:, :K], c["d_wr"].float().cpu()[:, :4])
    assert _worst(c["logits"].float().cpu()[:, :K], r["logits"], r["S_logits"], REL16, ACC, "logits") <= 1.0
    assert _worst(c["wr"].float().cpu()[:, :4], r["wr"], r["S_wr"], REL16, ACC, "wr") <= 1.0
    assert _worst(c["d_feat"].float().cpu(), r["d_feat"], r["S_d_feat"], REL16, ACC, "d_feat", exact=r["closed"]) <= 1.0
    for b in ("cls", "wh", "reg"):
        assert _worst(c["grads"][f"{b}_head.out_conv.weight"], r["dw_" + b], r["S_dw_" + b], REL32, ACC, b + " out_conv d_w") <= 1.0
        assert _worst(c["grads"][f"{b}_head.out_conv.bias"], r["db_" + b], r["S_db_" + b], REL32, ACC, b + " out_conv d_b") <= 1.0
    gd = _nhwc(c["d_feat"], N, H, W).double().permute(0, 3, 1, 2)
    ref, S = torch.nn.grad.conv2d_weight(f, wf.shape, gd, padding=1), torch.nn.grad.conv2d_weight(f.abs(), wf.shape, gd.abs(), padding=1)
    got = torch.cat([c["grads"][f"{b}_head.feat_conv.weight"] for b in ("cls", "wh", "reg")], 0)
    assert _worst(got, ref, S, REL32, ACC, "feat_conv d_w") <= 1.0
    got = torch.cat([c["grads"][f"{b}_head.feat_conv.bias"] for b in ("cls", "wh", "reg")], 0)
    assert _worst(got, gd.sum((0, 2, 3)), gd.abs().sum((0, 2, 3)), REL32, ACC, "feat_conv d_b") <= 1.0
    ref, S = TF.conv_transpose2d(gd, wf, padding=1), TF.conv_transpose2d(gd.abs(), wf.abs(), padding=1)
    assert _worst(_nhwc(c["g_f"], N, H, W).permute(0, 3, 1, 2), ref, S, REL16, ACC, "head d_x") <= 1.0


@pytest.mark.parametrize("K,modulated", MODEL_CASES, ids=MODEL_IDS)
def test_nchw_wrappers_eval_and_state_dict(K, modulated):
    """The NCHW methods are the pixel-major path; forward bits repeat; eval() applies the running statistics (each norm within one bf16
    step of the float64 formula on its own input); a saved and reloaded state gives the same forward bits; host tensors are refused."""
    import basedet.layers as BL
    from basedet_amd._lib import BasedetHipError
    c = _model_case(K, modulated)
    neck, head, x = c["neck"], c["head"], c["x"]
    state = {**neck.state_dict(), **head.state_dict()}
    y = neck(x.cuda())
    out = head(y)
    y2 = neck(x.cuda())
    assert torch.equal(y, y2) and tuple(y.shape) == (O.N, 64, 12, 20)
    assert tuple(out["cls"].shape) == (O.N, K, 12, 20) and tuple(out["wh"].shape) == tuple(out["reg"].shape) == (O.N, 2, 12, 20)
    assert torch.equal(out["cls"], torch.sigmoid(util.pm_to_nchw(head.logits_pm[:, :K], O.N, 12, 20).cuda()))
    dx = head.backward(torch.randn_like(out["cls"]), torch.randn_like(out["wh"]), torch.randn_like(out["reg"]))
    assert tuple(neck.backward(dx).shape) == tuple(x.shape)
    with pytest.raises(BasedetHipError):
        neck(x)
    with pytest.raises(BasedetHipError):
        head(y.cpu())
    neck.load_state_dict({k: v for k, v in state.items() if k.startswith("deconv")})        # (the forwards above moved the running statistics)
    neck.eval(), head.eval()
    ye = neck(x.cuda())
    for i, (_, l) in enumerate(neck.layers()):
        for name, yk in (("dcn_bn", "dcn"), ("up_bn", "up_sample")):
            q = {k: state[f"deconv{i + 1}.{name}.{k}"].double() for k in ("weight", "bias", "running_mean", "running_var")}
            zr = q["weight"] * (l.stages[yk].double().cpu() - q["running_mean"]) / torch.sqrt(q["running_var"] + O.EPS) + q["bias"]
            assert int(util.bf16_ulps(l.stages[name].cpu(), torch.relu(zr.to(BF).double())).max()) <= 1, name
    assert neck.state_dict()["deconv1.up_bn.running_mean"].equal(state["deconv1.up_bn.running_mean"]), "eval() must not move the running statistics"
    other_n, other_h = BL.CenternetDeconv(O.CHANNELS, O.KERNELS, modulated, seed=5).eval(), BL.CenterHead(64, K, seed=5).eval()
    assert not torch.equal(other_n(x.cuda()), ye)
    other_n.load_state_dict(neck.state_dict()), other_h.load_state_dict(head.state_dict())
    assert torch.equal(other_n(x.cuda()), ye)
    a, b = head(ye), other_h(ye)
    assert all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(KeyError):
        head.load_state_dict({k: v for k, v in head.state_dict().items() if k != "wh_head.out_conv.bias"})
    neck.train(), head.train()


@pytest.mark.parametrize("K,modulated", MODEL_CASES, ids=MODEL_IDS)
def test_end_to_end_wiring(K, modulated):
    """Neck + head + focal + two L1 calls against the float64 oracle: the device's rel-L2 distance may be at most twice the distance of
    the faithful=True oracle (bf16 at the device's storage points) from it, for the loss and for every parameter gradient.
    The bias of a deformable convolution feeds a training-mode batch norm, which removes any constant: its true gradient is exactly 0 and
    the float64 value is rounding noise (1e-17), so a rel-L2 against it measures nothing.  For those two names the check is absolute:
    d_bias sums the bf16 gradient g, each term rounded by at most 2^-9 |g|, so |d_bias| <= 2^-8 sum |g| + the fp32 accumulation term."""
    c = _model_case(K, modulated)
    l64, g64 = O.loss_and_grads(c["x"], c["p0"], c["tgt"], modulated, False)
    lf, gf = O.loss_and_grads(c["x"], c["p0"], c["tgt"], modulated, True)
    print(f"loss: device {c['loss']:.6f} faithful {lf:.6f} float64 {l64:.6f}")
    assert abs(c["loss"] - l64) <= 2 * abs(lf - l64) + 2.0 ** -22 * abs(l64)
    _, dcn = O.dcn_names(modulated)
    assert set(g64) == set(c["grads"])
    for k in sorted(g64):
        if k.endswith(f".dcn.{dcn}.bias"):
            i = int(k[6]) - 1
            bound = (2.0 ** -8 + ACC) * c["sgrads"][i]["dcn"].double().abs().sum(0).cpu()
            assert bool((c["grads"][k].double().abs() <= bound).all()), k
            continue
        d, f = util.rel_l2(c["grads"][k], g64[k]), util.rel_l2(gf[k], g64[k])
        print(f"{k}: device {d:.3e} faithful {f:.3e} ratio {d / f:.2f}")
        assert d <= 2 * f, k


def test_short_training_run():
    """20 plain SGD steps through params() / repack() on one fixed batch, at the learning rate at which the float64 oracle's loss falls
    (tests/test_center_head_cpu.py): every loss finite, the last five below the first five."""
    c = _model_case(3, False)
    neck, head = c["neck"], c["head"]
    neck.load_state_dict({k: v for k, v in c["p0"].items() if k.startswith("deconv")})
    head.load_state_dict({k: v for k, v in c["p0"].items() if "_head." in k})
    neck.train(), head.train()
    losses = []
    for _ in range(O.TRAIN_STEPS):
        losses.append(c["step"]()[3])
        for layer in (neck, head):
            g = layer.grads()
            for k, v in layer.params().items():
                v.sub_(O.TRAIN_LR * g[k])
            layer.repack()
    print("losses:", " ".join(f"{v:.3f}" for v in losses))
    assert all(np.isfinite(losses))
    assert np.mean(losses[-5:]) < np.mean(losses[:5])


# ---- one storage path: a layer on its own storage and one adopt()ed onto a caller's -------------------------------------------------------
# DeconvLayer(16, 64, 4) and CenterHead(16, K) for one K that is no multiple of 8 and one that is, N = 2 on an odd 5 x 7 map
KINDS = ["deconv", "head3", "head8"]
ONE_N, ONE_H, ONE_W, ONE_C = 2, 5, 7, 16


def _make(kind, seed=2):
    import basedet.layers as BL
    return BL.DeconvLayer(ONE_C, 64, 4, seed=seed) if kind == "deconv" else BL.CenterHead(ONE_C, int(kind[4:]), seed=seed)


def _adopt(layer):
    """Onto flat fp32 tensors (and, DeconvLayer, two hand-filled norm records) -> (w_flat, g_flat, records)."""
    w_flat, g_flat, w, g = util.flat_storage(layer.arena_shapes())
    recs = [util.norm_record(layer.out_planes) for _ in range(2)] if hasattr(layer, "dcn") else []
    layer.adopt(w, g, *recs)
    return w_flat, g_flat, recs


def _rand_pm(shape, seed, scale=1.0):
    return (scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))).to(BF).cuda()


def _run(layer, scale=1.0, accumulate=False):
    """One forward and backward on fixed pixel-major tensors -> ([outputs], d_x).  scale = 2 doubles the gradient exactly."""
    x = _rand_pm((ONE_N * ONE_H * ONE_W, ONE_C), 1)
    if hasattr(layer, "dcn"):
        y = layer.forward_pm(x, ONE_N, ONE_H, ONE_W)
        return [y], layer.backward_pm(_rand_pm(y.shape, 2, scale), accumulate)
    logits, wr = layer.forward_pm(x, ONE_N, ONE_H, ONE_W)
    return [logits, wr], layer.backward_pm(_rand_pm(logits.shape, 3, scale), _rand_pm(wr.shape, 4, scale), accumulate)


def _other_state(layer, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: (v + 0.05 * torch.randn(v.shape, generator=g)).abs() + 0.1 if k.endswith("running_var") else v + 0.05 * torch.randn(v.shape, generator=g)
            for k, v in layer.state_dict().items()}


def _packed(layer):
    if hasattr(layer, "dcn"):
        return [layer._up_wf, layer._up_wd, layer.dcn._off_wf, layer.dcn._off_wd, layer.dcn._dcn_wf, layer.dcn._dcn_wd]
    return [layer._feat_wf, layer._feat_wd]


@pytest.mark.parametrize("kind", KINDS)
def test_standalone_equals_adopted(kind):
    """Two layers of one seed, one adopted: the same forward and backward.  Bitwise: every output and every entry of grads() -- a single
    DeconvLayer has no parameter below its deformable convolution's d_x, and its offset convolution's gradients come from d_om, which
    repeats bit for bit (tests/test_deform_conv_gpu.py).  Only the DeconvLayer's d_x (fp32 atomics in bd_deform_conv_bwd_data) is held
    to 2^-10 rel-L2, the bound between two runs of one build
    (tests/test_centernet_model_gpu.py::test_neck_and_head_gradients_in_the_arena).  The adopted layer's gradients live in the caller's
    tensors, and a backward wrote all of them (they started at NaN)."""
    own, ad = _make(kind), _make(kind)
    w_flat, g_flat, recs = _adopt(ad)
    (oa, da), (ob, db) = _run(own), _run(ad)
    assert all(torch.equal(a, b) for a, b in zip(oa, ob))
    ga, gb = own.grads(), ad.grads()
    assert list(ga) == list(gb) == [k for k in own.names() if "running_" not in k]
    for k in ga:
        assert ga[k].shape == gb[k].shape and torch.equal(ga[k], gb[k]), k
    assert util.rel_l2(da, db) <= 2.0 ** -10 if kind == "deconv" else torch.equal(da, db)
    store = list(ad._store.g.values()) + (list(ad.dcn._store.g.values()) if kind == "deconv" else [])
    assert all(util.lies_inside(t, g_flat) and not bool(torch.isnan(t).any()) for t in store)
    for bn, rec in zip((ad.dcn_bn, ad.up_bn) if kind == "deconv" else (), recs):
        assert all(util.lies_inside(t, rec.buf) for t in (*bn.g.values(), *bn.p.values(), bn.mean, bn.inv_std, bn.sums))
        assert not bool(torch.isnan(rec.buf).any())
    assert all(util.lies_inside(v, w_flat) or any(util.lies_inside(v, r.buf) for r in recs) for v in ad.params().values())


def test_refused_adopt_moves_nothing():
    """A wrong shape anywhere -- the layer's own entry or its deformable convolution's -- raises before any tensor moved."""
    layer = _make("deconv")
    ptrs = {k: v.data_ptr() for k, v in layer.params().items()}
    for bad in ("up_sample.weight", "dcn.dcnv2.bias"):
        _, _, w, g = util.flat_storage(layer.arena_shapes())
        g[bad] = g[bad].reshape(-1)[:-1]
        with pytest.raises(ValueError, match="adopt"):
            layer.adopt(w, g, util.norm_record(64), util.norm_record(64))
        assert {k: v.data_ptr() for k, v in layer.params().items()} == ptrs and layer._store.g is None and layer.dcn._store.g is None


@pytest.mark.parametrize("adopted", [False, True], ids=["own", "adopted"])
@pytest.mark.parametrize("kind", KINDS)
def test_loads_and_repacks_in_place(kind, adopted):
    """load_state_dict() copies into the masters -- a params() view taken before shows the loaded values at the same address, so an
    optimizer that holds the views keeps training the layer -- and the next forward is that of a fresh layer loaded with the same state.
    repack() writes the bf16 operands where they are; after an in-place change through params() it gives the forward of a fresh layer
    loaded with the changed state."""
    layer = _make(kind)
    if adopted:
        _adopt(layer)
    held = layer.params()
    ptrs = {k: v.data_ptr() for k, v in held.items()}
    state = _other_state(layer, 5)
    layer.load_state_dict(state)
    assert {k: v.data_ptr() for k, v in layer.params().items()} == ptrs
    assert all(torch.equal(v.cpu(), state[k]) for k, v in held.items())
    assert all(torch.equal(v, state[k]) for k, v in layer.state_dict().items())
    fresh = _make(kind, seed=9)
    fresh.load_state_dict(state)
    assert all(torch.equal(a, b) for a, b in zip(_run(layer)[0], _run(fresh)[0]))
    where = [t.data_ptr() for t in _packed(layer)]
    for k, v in held.items():
        v.mul_(0.5 if k.endswith(".weight") else -1.0)
    layer.repack()
    assert [t.data_ptr() for t in _packed(layer)] == where
    changed = layer.state_dict()
    assert not torch.equal(changed[layer.names()[0]], state[layer.names()[0]])
    fresh.load_state_dict(changed)
    assert all(torch.equal(a, b) for a, b in zip(_run(layer)[0], _run(fresh)[0]))


@pytest.mark.parametrize("kind", KINDS)
def test_grads_do_not_alias_the_storage(kind):
    """What grads() returned after one backward does not change at the next (the gradient storage is allocated once and overwritten)."""
    layer = _make(kind)
    with pytest.raises(RuntimeError, match="before a backward"):
        layer.grads()
    _run(layer)
    kept = layer.grads()
    copy = {k: v.clone() for k, v in kept.items()}
    _run(layer, scale=2.0)
    again = layer.grads()
    assert all(torch.equal(kept[k], copy[k]) for k in kept)
    changed = [k for k in kept if not torch.equal(again[k], kept[k])]
    assert all(k in changed for k in kept if k.endswith("out_conv.weight") or k.endswith("bn.weight") or k == "up_sample.weight"), changed


@pytest.mark.parametrize("adopted", [False, True], ids=["own", "adopted"])
@pytest.mark.parametrize("act", ["relu", "silu"])
def test_batch_norm_act_accumulates(act, adopted):
    """A second identical backward with accumulate=True gives exactly twice the first dgamma / dbeta (v + v is exact in fp32) and the same
    data gradient: the apply launch read this backward's sums, not the accumulated ones.  eval() has no backward."""
    from basedet_amd.layers.batch_norm import BatchNormAct
    C, M = 16, ONE_N * ONE_H * ONE_W
    bn = BatchNormAct(C, act, 1e-5, 0.1, torch.device("cuda"))
    bn.p["weight"].copy_(1.0 + 0.1 * torch.randn(C, generator=torch.Generator().manual_seed(6)))
    if adopted:
        rec = util.norm_record(C)
        bn.adopt(rec)
        assert util.lies_inside(bn.g["weight"], rec.buf) and util.lies_inside(bn.p["running_var"], rec.buf)
    y, g = _rand_pm((M, C), 7), _rand_pm((M, C), 8)
    z = bn.forward_pm(y, ONE_N, ONE_H, ONE_W)
    assert z.shape == y.shape and bool(((z >= 0).all() if act == "relu" else (z >= -0.28).all()))       # (min of silu: -0.2785)
    gy1 = bn.backward_pm(g)
    first = {k: v.clone() for k, v in bn.g.items()}
    where = {k: v.data_ptr() for k, v in bn.g.items()}
    gy2 = bn.backward_pm(g, accumulate=True)
    assert torch.equal(gy1, gy2) and {k: v.data_ptr() for k, v in bn.g.items()} == where
    assert all(bool(torch.isfinite(first[k]).all()) and float(first[k].abs().sum()) > 0 and torch.equal(bn.g[k], 2 * first[k]) for k in first)
    bn.backward_pm(g)
    assert all(torch.equal(bn.g[k], first[k]) for k in first), "accumulate=False overwrites"
    bn.training = False
    bn.forward_pm(y, ONE_N, ONE_H, ONE_W)
    with pytest.raises(RuntimeError, match="eval"):
        bn.backward_pm(g)
