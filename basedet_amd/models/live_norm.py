"""The live batch norms of a model (MODEL.BACKBONE.NORM / MODEL.FPN.NORM = "BN" / "SyncBN"): one record per normalised convolution and
one owner of their buffers."""
import numpy as np
import torch


class BatchNormState:
    """The norm record of one normalised convolution (MODEL.FPN.NORM = "BN" / "SyncBN", layers.get_norm at fpn_backbone.py:49-76, named
    `<conv>.norm`; MODEL.BACKBONE.NORM, layers/backbone/build.py:27-30, named `...bnK` / `...downsample.1` like the FrozenBN it replaces):
    gamma / beta are trainable fp32 vectors in the parameter arena, right behind the convolution's weight (`<name>.weight` / `.bias`);
    the running statistics are buffers (`.running_mean` / `.running_var`); mean / inv_std / sums are the batch statistics of the last
    training forward (sums = [M, sum y, sum y^2]; the backward pass reads the count M).  The buffers are views of LiveNorms' flat tensors,
    set by LiveNorms.allocate."""

    EPS, MOMENTUM = 1e-5, 0.1      # MegEngine's BatchNorm2d defaults (momentum 0.9 in its convention = 0.1 in torch's); documented choice

    def __init__(self, name, C):
        self.name, self.C = name, C
        self.running_mean = self.running_var = self.mean = self.inv_std = self.sums = None
        self.gamma = self.beta = self.g_gamma = self.g_beta = None
        self.fold_scale = self.fold_shift = None      # eval(): the affine the convolution's epilogue applies

    def reserve(self, arena):
        self._gi = arena.reserve(self.name + ".weight", (self.C,))
        self._bi = arena.reserve(self.name + ".bias", (self.C,))

    def bind_views(self, arena):
        """gamma / beta and their gradients: the views of the allocated arena's entries reserve() made."""
        self.gamma, self.g_gamma = arena.view("w", self._gi), arena.view("g", self._gi)
        self.beta, self.g_beta = arena.view("w", self._bi), arena.view("g", self._bi)

    def bind(self, arena, params):
        self.bind_views(arena)
        for t, k in ((self.gamma, "weight"), (self.beta, "bias"), (self.running_mean, "running_mean"), (self.running_var, "running_var")):
            t.copy_(torch.from_numpy(np.asarray(params[f"{self.name}.{k}"], np.float32).reshape(-1)))

    def export(self, out):
        for t, k in ((self.gamma, "weight"), (self.beta, "bias"), (self.running_mean, "running_mean"), (self.running_var, "running_var")):
            out[f"{self.name}.{k}"] = t.cpu().numpy().copy()

    def export_grad(self, out):
        out[self.name + ".weight"] = self.g_gamma.detach().cpu().clone()
        out[self.name + ".bias"] = self.g_beta.detach().cpu().clone()

    def fold(self):
        """fold_scale / fold_shift from the running statistics, on the host like FrozenBN's (ConvLayer.bind): evaluation only."""
        g, b = self.gamma.cpu().numpy(), self.beta.cpu().numpy()
        scale = g / np.sqrt(self.running_var.cpu().numpy() + np.float32(self.EPS))
        self.fold_scale.copy_(torch.from_numpy(scale.astype(np.float32)))
        self.fold_shift.copy_(torch.from_numpy((b - self.running_mean.cpu().numpy() * scale).astype(np.float32)))


class LiveNorms:
    """Every live BatchNormState of a model, in forward order (backbone, then FPN), and the three flat fp32 tensors their buffers are
    views of: `running` (per norm [mean | var], 2 C: one broadcast covers every norm), `stats` (per norm [mean | inv_std] of the batch)
    and `sums` (3 C).  Two-phase like ParamArena: add() while the layers are built, allocate() once after the last."""

    def __init__(self, device):
        self.device = device
        self._norms = []
        self.running = self.stats = self.sums = None

    def add(self, name, C):
        n = BatchNormState(name, C)
        self._norms.append(n)
        return n

    def allocate(self):
        f32 = dict(dtype=torch.float32, device=self.device)
        tot = sum(n.C for n in self._norms)
        self.running, self.stats, self.sums = torch.zeros(2 * tot, **f32), torch.zeros(2 * tot, **f32), torch.zeros(3 * tot, **f32)
        o = 0
        for n in self._norms:
            c = n.C
            n.running_mean, n.running_var = self.running[2 * o: 2 * (o + c)].view(2, c)
            n.mean, n.inv_std = self.stats[2 * o: 2 * (o + c)].view(2, c)
            n.sums = self.sums[3 * o: 3 * (o + c)].view(3, c)
            n.fold_scale, n.fold_shift = torch.empty(c, **f32), torch.empty(c, **f32)
            o += c

    def __iter__(self):
        return iter(self._norms)

    def __len__(self):
        return len(self._norms)
