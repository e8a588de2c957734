"""The optimizer rules of csrc/optim.hip restated in numpy float32, one rounding per operation and in the kernel's order (shared by
tests/test_optim_cpu.py, which checks the restatement against float64 optimizers, and tests/test_optim_gpu.py, which checks the kernels
against the restatement bit for bit).  float32 array (op) float32 scalar is one correctly rounded fp32 operation in numpy, square root
and division included; nothing here is fused.  Inputs are left alone, results are new arrays."""
import numpy as np

F = np.float32


def adam_scalars(betas, step):
    """(beta1, 1 - beta1, beta2, 1 - beta2, 1 - beta1**step, 1 - beta2**step), formed in Python float64 and then cast to fp32."""
    b1, b2 = float(betas[0]), float(betas[1])
    return tuple(F(x) for x in (b1, 1 - b1, b2, 1 - b2, 1 - b1 ** step, 1 - b2 ** step))


def adam(w, m, v, g, lr, betas, eps, wd, step, grad_scale=1.0, decoupled=False):
    """megengine.optimizer.Adam (decoupled False) / AdamW (True), update number `step` from 1 -> (w, m, v)."""
    assert all(a.dtype == F for a in (w, m, v, g))
    b1, omb1, b2, omb2, bc1, bc2 = adam_scalars(betas, step)
    lr, eps, wd, gs = F(lr), F(eps), F(wd), F(grad_scale)
    gg = g * gs
    if not decoupled:
        gg = gg + wd * w
    m = b1 * m + omb1 * gg
    v = b2 * v + omb2 * (gg * gg)
    d = (m / bc1) / (np.sqrt(v / bc2) + eps)
    if decoupled:
        d = d + wd * w
    w = w - lr * d
    return w, m, v


def sgd_nesterov(w, v, g, lr, momentum, wd, grad_scale=1.0):
    """megengine.optimizer.SGD(nesterov=True) -> (w, v)."""
    assert all(a.dtype == F for a in (w, v, g))
    lr, mom, wd, gs = F(lr), F(momentum), F(wd), F(grad_scale)
    gg = g * gs + wd * w
    v = mom * v + gg
    w = w - lr * (gg + mom * v)
    return w, v


def ema(e, w, m):
    """layers/common/ema.py:80 `v * m + (1 - m) * model_state`: (e * f32(m)) + (f32(1 - m) * w)."""
    return (e * F(m)) + (F(1 - m) * w)
