"""Training-mode batch norm plus activation over one dense pixel-major tensor, on csrc/batchnorm.hip: the norm of DeconvLayer (ReLU) and of
ConvBNSiLU (SiLU).  eps and momentum are in torch's convention; the running statistics move in train(), and in eval() the same apply
launch is fed running_mean and 1 / sqrt(running_var + eps).

relu: bd_bn_stats_fwd -> bd_bn_apply_act_fwd; backward bd_relu_bwd_bf16 -> bd_bn_bwd_reduce -> bd_bn_bwd_apply.
silu: bd_bn_stats_fwd -> bd_bn_silu_fwd; backward bd_bn_silu_bwd_reduce -> bd_bn_silu_bwd_apply, which recompute the gate from the
pre-norm tensor: the forward output is not kept."""
import torch

from .. import ops
from ._pm import F32, workspace

__all__ = ["BatchNormAct"]


class BatchNormAct:
    KEYS = ("weight", "bias", "running_mean", "running_var")

    def __init__(self, C, act, eps, momentum, device):
        if act not in ("relu", "silu"):
            raise ValueError(f"BatchNormAct: act={act!r} is not built (relu or silu)")
        self.C, self.act, self.eps, self.momentum, self.device, self.training = C, act, float(eps), float(momentum), device, True
        f = dict(dtype=F32, device=device)
        self.p = {"weight": torch.ones(C, **f), "bias": torch.zeros(C, **f), "running_mean": torch.zeros(C, **f),
                  "running_var": torch.ones(C, **f)}
        self.mean, self.inv_std, self.sums = torch.empty(C, **f), torch.empty(C, **f), torch.empty((3, C), **f)
        self.g = None              # {"weight", "bias"}: allocated at the first backward, or adopt()ed
        self._saved = None
        self._eval_inv_std = None

    def adopt(self, state):
        """Live on a model's norm record (models/live_norm.py BatchNormState): gamma / beta and their gradients are its arena views, the
        running statistics and the batch statistics its buffers -- where the optimizer, the EMA's buffer average and the parameter
        broadcast find them.  The current values move in."""
        old = self.p
        self.p = {"weight": state.gamma, "bias": state.beta, "running_mean": state.running_mean, "running_var": state.running_var}
        for k, v in old.items():
            self.p[k].copy_(v)
        self.mean, self.inv_std, self.sums = state.mean, state.inv_std, state.sums
        self.g = {"weight": state.g_gamma, "bias": state.g_beta}

    def refresh_eval(self):
        """1 / sqrt(running_var + eps) for the eval() forward, computed once (at eval() / after a load) instead of per call."""
        self._eval_inv_std = 1.0 / torch.sqrt(self.p["running_var"] + self.eps)

    def load(self, p, prefix):
        """The four vectors `prefix + key` of a loaded state, copied in place."""
        for k in self.KEYS:
            self.p[k].copy_(p[prefix + k])
        if self._eval_inv_std is not None:
            self.refresh_eval()

    def state(self, prefix):
        return {prefix + k: self.p[k].detach().cpu().clone() for k in self.KEYS}

    def forward_pm(self, y, N, H, W):
        """y bf16 [N H W][C] (kept for the backward) -> act(norm(y)), a new tensor."""
        geom, p = ops.single(N, H, W), self.p
        if self.training:
            ops.bn_stats_fwd(y, geom, self.C, self.eps, self.momentum, self.mean, self.inv_std, self.sums, p["running_mean"],
                             p["running_var"], workspace(ops.bn_workspace_bytes(N * H * W, self.C), self.device))
            mean, inv_std = self.mean, self.inv_std
        else:
            mean = p["running_mean"]
            inv_std = self._eval_inv_std if self._eval_inv_std is not None else 1.0 / torch.sqrt(p["running_var"] + self.eps)
        z = torch.empty_like(y)
        if self.act == "relu":
            ops.bn_apply_act_fwd(y, geom, mean, inv_std, p["weight"], p["bias"], z, geom, self.C, relu=True)
        else:
            ops.bn_silu_fwd(y, geom, mean, inv_std, p["weight"], p["bias"], z, geom, self.C)
        self._saved = (y, z if self.act == "relu" else None, geom, self.training)
        return z

    def backward_pm(self, g, accumulate=False):
        """g bf16 [N H W][C] -> the gradient of y.  dgamma / dbeta go to self.g: written by the reduce launch, or (accumulate) reduced
        into a scratch -- the apply launch reads THIS backward's sums -- and added onto self.g."""
        y, z, geom, training = self._saved
        if not training:
            raise RuntimeError("backward() through a norm in eval() mode is not built")
        C, p = self.C, self.p
        if self.g is None:
            accumulate = False
            self.g = dict(zip(("weight", "bias"), torch.empty((2, C), dtype=F32, device=self.device)))
        dgamma, dbeta = torch.empty((2, C), dtype=F32, device=self.device) if accumulate else (self.g["weight"], self.g["bias"])
        ws = workspace(ops.bn_workspace_bytes(y.shape[0], C), self.device)
        if self.act == "relu":
            gm = ops.relu_bwd_bf16(g, z, torch.empty_like(g))
            ops.bn_bwd_reduce(gm, geom, y, geom, self.mean, self.inv_std, C, dgamma, dbeta, ws)
            gy = ops.bn_bwd_apply(gm, geom, y, geom, self.mean, self.inv_std, p["weight"], dgamma, dbeta, self.sums[0], torch.empty_like(g),
                                  geom, C)
        else:
            ops.bn_silu_bwd_reduce(g, geom, y, geom, self.mean, self.inv_std, p["weight"], p["bias"], C, dgamma, dbeta, ws)
            gy = ops.bn_silu_bwd_apply(g, geom, y, geom, self.mean, self.inv_std, p["weight"], p["bias"], dgamma, dbeta, self.sums[0],
                                       torch.empty_like(g), geom, C)
        if accumulate:
            self.g["weight"].add_(dgamma)
            self.g["bias"].add_(dbeta)
        return gy
