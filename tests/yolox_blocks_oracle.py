"""float64 restatement (torch, CPU) of Focus, SPPBottleneck, Bottleneck, CSPLayer, CSPDarknet and YOLOPAFPN (basedet_amd/layers/
yolox_blocks.py), differentiated with torch.autograd, in the form of tests/yolox_head_oracle.py: activations NCHW, parameters a dict
under the layers' names (state_dict()), and the same `faithful` switch.

faithful=True rounds to bf16 where the device stores bf16: inside every convolution block (yolox_head_oracle.conv_bn_silu: the weight
operand, the convolution output, the norm + SiLU output, and the gradients on their way back) and after Bottleneck's shortcut add, which
is a second rounding after the SiLU's.  The max-pools, the concatenations, the nearest upsample and Focus's space-to-depth select or move
values and round nothing.  max_pool2d's float64 CPU autograd sends a window's gradient to the window's first maximum in row-major order
(tests/test_yolox_blocks_cpu.py checks that), which is bd_spp_bwd's rule."""
import numpy as np
import torch
import torch.nn.functional as TF

from yolox_head_oracle import _r, conv_bn_silu, double_params  # noqa: F401  (double_params: re-exported for the tests)


def _c(x, p, name, k, stride, kw):
    return conv_bn_silu(x, p, name, k, stride, kw.get("training", True), kw.get("faithful", False), kw.get("stats"))


def _j(prefix, name):
    return f"{prefix}.{name}" if prefix else name


# ---- the glue, on its own ------------------------------------------------------------------------------------------------------------------------
def space_to_depth(x):
    """Focus's slicing (basic_block.py:25-31): (N, C, H, W) -> (N, 4C, H/2, W/2) = (top-left, bottom-left, top-right, bottom-right)."""
    return torch.cat((x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]), 1)


def spp_cat(x):
    """(x, maxpool5, maxpool9, maxpool13), stride 1, padding k // 2 (padding never wins: max_pool2d pads with -inf)."""
    return torch.cat([x] + [TF.max_pool2d(x, k, 1, k // 2) for k in (5, 9, 13)], 1)


def upsample2x(x):
    return x.repeat_interleave(2, 2).repeat_interleave(2, 3)


# ---- the modules -----------------------------------------------------------------------------------------------------------------------------------
def focus(x, p, prefix="", **kw):
    return _c(space_to_depth(x), p, _j(prefix, "conv"), 3, 1, kw)


def spp_bottleneck(x, p, prefix="", **kw):
    return _c(spp_cat(_c(x, p, _j(prefix, "conv1"), 1, 1, kw)), p, _j(prefix, "conv2"), 1, 1, kw)


def bottleneck(x, p, prefix="", use_add=True, **kw):
    y = _c(_c(x, p, _j(prefix, "conv1"), 1, 1, kw), p, _j(prefix, "conv2"), 3, 1, kw)
    return _r(y + x, kw.get("faithful", False)) if use_add else y


def csp_layer(x, p, prefix="", n=1, shortcut=True, **kw):
    x1, x2 = _c(x, p, _j(prefix, "conv1"), 1, 1, kw), _c(x, p, _j(prefix, "conv2"), 1, 1, kw)
    for i in range(n):
        x1 = bottleneck(x1, p, _j(prefix, f"m.{i}"), shortcut, **kw)          # (hidden -> hidden: the shortcut is used whenever it is asked for)
    return _c(torch.cat((x1, x2), 1), p, _j(prefix, "conv3"), 1, 1, kw)


def darknet(x, p, depth_factor, prefix="", **kw):
    """{stem, dark2 .. dark5}."""
    d = max(round(depth_factor * 3), 1)
    out = {"stem": focus(x, p, _j(prefix, "stem"), **kw)}
    x = out["stem"]
    for name, n in (("dark2", d), ("dark3", 3 * d), ("dark4", 3 * d)):
        x = csp_layer(_c(x, p, _j(prefix, f"{name}.0"), 3, 2, kw), p, _j(prefix, f"{name}.1"), n, True, **kw)
        out[name] = x
    x = spp_bottleneck(_c(x, p, _j(prefix, "dark5.0"), 3, 2, kw), p, _j(prefix, "dark5.1"), **kw)
    out["dark5"] = csp_layer(x, p, _j(prefix, "dark5.2"), d, False, **kw)
    return out


def pafpn(x, p, depth, **kw):
    """(pan_out2, pan_out1, pan_out0) of YOLOPAFPN on CSPDarknet(depth, .)."""
    f = darknet(x, p, depth, "backbone", **kw)
    x2, x1, x0 = f["dark3"], f["dark4"], f["dark5"]
    n = round(3 * depth)
    fpn_out0 = _c(x0, p, "lateral_conv0", 1, 1, kw)
    f_out0 = csp_layer(torch.cat((upsample2x(fpn_out0), x1), 1), p, "C3_p4", n, False, **kw)
    fpn_out1 = _c(f_out0, p, "reduce_conv1", 1, 1, kw)
    pan_out2 = csp_layer(torch.cat((upsample2x(fpn_out1), x2), 1), p, "C3_p3", n, False, **kw)
    pan_out1 = csp_layer(torch.cat((_c(pan_out2, p, "bu_conv2", 3, 2, kw), fpn_out1), 1), p, "C3_n3", n, False, **kw)
    pan_out0 = csp_layer(torch.cat((_c(pan_out1, p, "bu_conv1", 3, 2, kw), fpn_out0), 1), p, "C3_n4", n, False, **kw)
    return pan_out2, pan_out1, pan_out0


# ---- problems the tests share -------------------------------------------------------------------------------------------------------------------
def random_state(shapes, seed=0):
    """A state with every norm away from its initial values, so that each parameter matters (yolox_head_oracle.head_state's recipe)."""
    g = torch.Generator().manual_seed(200 + seed)
    p = {}
    for k, shape in shapes.items():
        if k.endswith("norm.weight"):
            v = 1.0 + 0.3 * torch.randn(shape, generator=g)
        elif k.endswith("norm.bias") or k.endswith("running_mean"):
            v = 0.3 * torch.randn(shape, generator=g)
        elif k.endswith("running_var"):
            v = 0.5 + torch.rand(shape, generator=g)
        else:
            v = torch.randn(shape, generator=g) * (1.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        p[k] = v.float()
    return p


def run(fn, x, p0, d_outs, faithful, **kw):
    """Forward and one backward of sum(out * d_out) through fn(x, p, faithful=...): (outputs, d_x or None, {name: parameter gradient},
    the running statistics after the forward).  fn returns a tensor, a tuple or a dict of tensors; d_outs has the same form."""
    p = double_params(p0, True)
    xr = x.double().clone().requires_grad_(True)
    stats = {}
    out = fn(xr, p, faithful=faithful, stats=stats, **kw)
    flat = lambda o: list(o.values()) if isinstance(o, dict) else list(o) if isinstance(o, (tuple, list)) else [o]
    outs, ds = flat(out), flat(d_outs)
    sum((o * d.double()).sum() for o, d in zip(outs, ds)).backward()
    return ([o.detach() for o in outs], xr.grad, {k: v.grad for k, v in p.items() if v.requires_grad}, stats)


def bf16_step(ref):
    """One bf16 step at each |ref| (float64 numpy): 2^(floor(log2 |ref|) - 7), the smallest normal's below that."""
    a = np.maximum(np.abs(np.asarray(ref, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def spp_bwd_terms(x, g_cat):
    """The float64 adjoint of spp_cat at x (N, C, H, W) for the gradient g_cat (N, 4C, H, W), with what the bound needs: (d_x, sum |terms|,
    term count) per element."""
    x = x.double()
    out = []
    for g in (g_cat.double(), g_cat.double().abs(), torch.ones_like(g_cat, dtype=torch.float64)):
        xr = x.clone().requires_grad_(True)
        (spp_cat(xr) * g).sum().backward()
        out.append(xr.grad)
    return out
