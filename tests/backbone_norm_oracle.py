"""Oracle of the batch-normalised backbone (MODEL.BACKBONE.NORM = "BN" / "SyncBN"; layers/backbone/build.py:27-30, models/cls/resnet.py) in
torch-CPU autograd: a helper, not a test.

backbone_norm_oracle_cls(base) subclasses oracle/model.py's Oracle (or, for a config that also sets MODEL.FPN.NORM, the class of
tests/fpn_norm_oracle.py::norm_oracle_cls()) and overrides `_bn` / `_conv_bn` and the stem: every bnK / downsample.1 and the stem's bn1 is
a BatchNorm2d in training mode (eps 1e-5; batch mean and biased variance over N H W; running = 0.9 running + 0.1 batch with the unbiased
variance; `training = False`: the running statistics, i.e. the FrozenBN arithmetic of the base class).  fp32 throughout; with sim_bf16 the
convolution's output is rounded to bf16 before the statistics (the HIP path stores it so) and `inject` / `record` work as in the base class,
with more keys: "stem_out", the stem's stored ReLU output (the max-pool then sees the same gates and maxima on both sides), and "g_<key>"
for every stored post-norm activation <key> (stem_out, <block>.a0 / .a1 / .out): the stored bf16 gradient dL/d(pre-activation) of that
tensor, i.e. dL/dz of its norm.  As tests/fpn_norm_oracle.py does with "g_lat{s}", the oracle's own gradient there -- computed from the
stored gradient one layer above -- is first compared with it (rel-L2 into self.grad_check[g_key]) and then replaced by it, so that every
norm's dgamma / dbeta and every weight gradient sum the very bf16 terms the kernels summed.  (dL/d beta of a norm is a sum over all
pixels of a channel that cancels to a small residue: the next norm removes most of a per-channel constant.  Against two differently rounded
gradient tensors its rel-L2 measures their rounding -- 2.0e-2 on bn1.bias and layer1's bn2.bias of the R18 fixture -- not the kernels.)"""
import numpy as np
import torch
import torch.nn.functional as TF

EPS, MOMENTUM = 1e-5, 0.1


def is_backbone_norm_key(k):
    return "backbone.bottom_up" in k and (".bn" in k or "downsample.1" in k)


def randomise_backbone_norms(params, seed=11):
    """gamma of both signs (the magnitudes of the fixture stay: the last norm of a residual branch is damped), beta and the running
    statistics away from 0 / 0 / 1: a dropped term shows.

    The running variances are drawn from U(0.125, 0.375), well below the batch variances of the convolution outputs (O(1)): a forward pass
    that normalised with the running statistics -- the key ignored -- amplifies every layer by about 2 and shows in the losses far beyond
    the 2e-2 the GPU tests hold them to (tests/test_backbone_norm_cpu.py::test_the_fixture_feels_the_key: the R18 fixture's losses move
    by 0.54 relative, its FrozenBN activations stay below 4e2).  With U(0.5, 1.5) the move was 4.6e-3: the head starts at N(0, 0.01) and
    its prior sets the losses unless the features change scale.  Training-mode results do not depend on these values."""
    rng = np.random.default_rng(seed)
    for k in list(params):
        if not is_backbone_norm_key(k):
            continue
        n = params[k].shape[0]
        if k.endswith(".weight"):
            mag = np.where(np.abs(params[k]) == 1.0, rng.uniform(0.7, 1.3, n), np.abs(params[k]))
            params[k] = (mag * rng.choice([-1.0, 1.0], n, p=[0.25, 0.75])).astype(np.float32)
        elif k.endswith(".bias"):
            params[k] = rng.normal(0, 0.1, n).astype(np.float32)
        elif k.endswith("running_mean"):
            params[k] = rng.normal(0, 0.1, n).astype(np.float32)
        else:
            params[k] = (rng.uniform(0.5, 1.5, n) * 0.25).astype(np.float32)
    return params


def batch_norm(y, gamma, beta, running_mean=None, running_var=None):
    """Training-mode BatchNorm2d of an NCHW tensor; returns z and, when given, the updated running statistics."""
    mu, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    xh = (y - mu.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + EPS)
    z = xh * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    if running_mean is None:
        return z
    with torch.no_grad():
        m = y.numel() // y.shape[1]
        rm = (1 - MOMENTUM) * running_mean + MOMENTUM * mu
        rv = (1 - MOMENTUM) * running_var + MOMENTUM * var * m / max(m - 1, 1)
    return z, rm, rv


def backbone_norm_oracle_cls(base=None):
    from oracle.model import RESNET_SPECS, Oracle
    base = Oracle if base is None else base

    class BackboneNormOracle(base):
        training = True          # False: the running statistics (eval()), the base class's FrozenBN arithmetic

        def _bn(self, x, prefix):
            if not self.training:
                return super()._bn(x, prefix)
            p = self.p
            z, rm, rv = batch_norm(x, p[prefix + ".weight"], p[prefix + ".bias"], p[prefix + ".running_mean"], p[prefix + ".running_var"])
            p[prefix + ".running_mean"], p[prefix + ".running_var"] = rm, rv
            return z

        def _act(self, key, x, relu):
            g_key = "g_" + key
            if self.training and self.inject is not None and g_key in self.inject and x.requires_grad:
                stored = self.inject[g_key]
                check = self.__dict__.setdefault("grad_check", {})

                def hook(g):
                    check[g_key] = float((stored.double() - g.double()).norm() / (g.double().norm() + 1e-30))
                    return stored.to(g.dtype)
                x.register_hook(hook)
            return super()._act(key, x, relu)

        def _conv_bn(self, x, name, bn, stride=1, pad=0):
            if not self.training:
                return super()._conv_bn(x, name, bn, stride, pad)
            # sim_bf16: the HIP path stores the bare convolution's output as bf16; the statistics and the backward pass read that tensor
            return self._bn(self._q(self._conv(x, name, stride, pad)), bn)

        def backbone(self, x):
            """ResNet.extract_features (resnet.py:236-252): conv7x7 -> BN -> ReLU -> maxpool, then the blocks of the base class."""
            if not self.training:
                return super().backbone(x)
            bu = "backbone.bottom_up"
            kind, layers = RESNET_SPECS[self.arch["backbone"]]
            x = self._act("stem_out", self._conv_bn(self._q(x), bu + ".conv1", bu + ".bn1", 2, 3), True)
            x = TF.max_pool2d(x, 3, 2, 1)
            outs = {"stem": x}
            block = self._bottleneck if kind == "bottleneck" else self._basic
            for li, nblk in enumerate(layers):
                for b in range(nblk):
                    stride = 2 if (b == 0 and li > 0) else 1
                    has_ds = (bu + f".layer{li + 1}.{b}.downsample.0.weight") in self.p
                    x = block(x, bu + f".layer{li + 1}.{b}", stride, has_ds)
                outs[f"res{li + 2}"] = x
            return outs
    return BackboneNormOracle
