"""Oracle of the batch-normalised FPN (MODEL.FPN.NORM = "BN" / "SyncBN"; fpn_backbone.py:49-76) in torch-CPU autograd: a helper, not a test.

norm_oracle_cls() subclasses oracle/model.py's Oracle and overrides fpn(): every lateral / output convolution is biasless and followed by
BatchNorm2d (eps 1e-5; training: batch mean and biased variance over N H W; running = 0.9 running + 0.1 batch with the unbiased
variance; evaluation: the running statistics).  top_block.p6 / p7 and FPNP6 have no norm.

With `inject` holding "g_lat{s}" (the stored bf16 gradient dL/d lat_s of the HIP run, NCHW) the oracle's own gradient at that point is
first compared with it (rel-L2 into self.grad_check["g_lat{s}"]) and then replaced by it, so that everything below -- the lateral norm's
dgamma / dbeta among it -- sums the very bf16 terms the kernels summed, as tests/test_batchnorm_gpu.py compares them.  (d loss / d beta of
a lateral norm is a border residual of a tensor that sums to zero in the interior: the output norm removes any constant.  Against two
differently rounded gradient tensors its rel-L2 measures their rounding, 1.3e-2, not the kernels.)"""
import numpy as np
import torch
import torch.nn.functional as TF

EPS, MOMENTUM = 1e-5, 0.1


def randomise_norms(params, seed=7):
    """gamma / beta away from 1 / 0 (both signs), running statistics away from 0 / 1: a dropped term shows."""
    rng = np.random.default_rng(seed)
    for k in list(params):
        if ".norm." not in k:
            continue
        n = params[k].shape[0]
        if k.endswith(".norm.weight"):
            params[k] = (rng.uniform(0.6, 1.4, n) * rng.choice([-1.0, 1.0], n, p=[0.25, 0.75])).astype(np.float32)
        elif k.endswith(".norm.bias"):
            params[k] = rng.normal(0, 0.2, n).astype(np.float32)
        elif k.endswith("running_mean"):
            params[k] = rng.normal(0, 0.1, n).astype(np.float32)
        else:
            params[k] = rng.uniform(0.5, 1.5, n).astype(np.float32)
    return params


def norm_oracle_cls():
    from oracle.model import Oracle

    class NormOracle(Oracle):
        training = True          # False: the running statistics (eval())

        def _lat(self, key, x):
            """_act for lat_s, with the stored gradient injected behind it when the HIP run's is given."""
            y = self._act(key, x, False)
            g_key = "g_" + key
            if self.inject is not None and g_key in self.inject and y.requires_grad:
                stored = self.inject[g_key]
                check = self.__dict__.setdefault("grad_check", {})

                def hook(g):
                    check[g_key] = float((stored.double() - g.double()).norm() / (g.double().norm() + 1e-30))
                    return stored.to(g.dtype)
                y.register_hook(hook)
            return y

        def _norm(self, y, name):
            p = self.p
            g, b = p[name + ".norm.weight"], p[name + ".norm.bias"]
            if not self.training:
                scale = g / torch.sqrt(p[name + ".norm.running_var"] + EPS)
                return y * scale.view(1, -1, 1, 1) + (b - p[name + ".norm.running_mean"] * scale).view(1, -1, 1, 1)
            mu, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
            with torch.no_grad():
                m = y.numel() // y.shape[1]
                p[name + ".norm.running_mean"] = (1 - MOMENTUM) * p[name + ".norm.running_mean"] + MOMENTUM * mu
                p[name + ".norm.running_var"] = (1 - MOMENTUM) * p[name + ".norm.running_var"] + MOMENTUM * var * m / max(m - 1, 1)
            xh = (y - mu.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + EPS)
            return xh * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)

        def _conv_norm(self, x, name, pad=0):
            # sim_bf16: the HIP path stores the convolution's output as bf16 (the statistics and the backward read that tensor); in
            # evaluation it never exists -- the affine is folded into the convolution's launch
            y = self._conv(x, name, 1, pad)
            return self._norm(self._q(y) if self.training else y, name)

        def fpn(self, feats):
            names = self.arch.get("fpn_in", ["res3", "res4", "res5"])
            stages = [int(n[-1]) for n in names]
            x = [feats[n] for n in names[::-1]]
            st = stages[::-1]
            q, act = self._q, self._act
            deconv = self.arch.get("upsample") == "deconv"
            prev = self._lat(f"lat{st[0]}", self._conv_norm(x[0], f"backbone.fpn_lateral{st[0]}"))
            results = [act(f"P{st[0]}", self._conv_norm(prev, f"backbone.fpn_output{st[0]}", 1), False)]
            for f, sc, s in zip(x[1:], st[:-1], st[1:]):
                if deconv:
                    td = TF.conv_transpose2d(prev, q(self.p[f"backbone.fpn_upsample{sc}.weight"]), stride=2, padding=1)
                else:
                    td = TF.interpolate(prev, scale_factor=2, mode="bilinear", align_corners=False)
                prev = self._lat(f"lat{s}", q(self._conv_norm(f, f"backbone.fpn_lateral{s}")) + td)
                results.insert(0, act(f"P{s}", self._conv_norm(prev, f"backbone.fpn_output{s}", 1), False))
            top = stages[-1]
            if self.arch.get("top_block") == "pool":          # FPNP6 (fpn_backbone.py:172-183)
                return results + [TF.max_pool2d(results[-1], kernel_size=1, stride=2, padding=0)]
            p6 = act(f"P{top + 1}", self._conv(feats["res5"], "backbone.top_block.p6", 2, 1), False)
            p7 = act(f"P{top + 2}", self._conv(TF.relu(p6), "backbone.top_block.p7", 2, 1), False)
            return results + [p6, p7]
    return NormOracle
