"""What the pixel-major layers (deformable.py, center_head.py, yolox_head.py, yolox_blocks.py, batch_norm.py) share: the NCHW fp32 <->
pixel-major bf16 [N H W][C] wrappers, the strict state loader, workspaces, ParamStore -- the fp32 masters and parameter gradients of one
layer -- and Container, the composition of such layers under the reference's names.

The layer protocol, which a Container provides from its children's: `names()`, `params()`, `grads()`, `state_dict()`,
`load_state_dict()`, `repack()`, `arena_shapes()`, `adopt(w, g, ...)`, `refresh_eval()`, `train()`.  A layer that is not itself a
Container (a leaf) also declares NORMS, the names of its norms relative to itself: its adopt() takes one norm record for each, in that
order, after w and g."""
import numpy as np
import torch

from .._lib import BasedetHipError

BF16, F32 = torch.bfloat16, torch.float32


def round_up8(n):
    return (n + 7) // 8 * 8


def round_up32(n):
    return (int(n) + 31) // 32 * 32


def cut(d, name):
    """The entries of d under `name.`, without that prefix."""
    return {k[len(name) + 1:]: v for k, v in d.items() if k.startswith(name + ".")}


def need_device(t, what):
    """A layer's refusal of a host tensor."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise BasedetHipError(f"{what}: needs a tensor on a HIP device (got a host tensor); there is no CPU fallback")


def need_device_all(tensors, module):
    """A model module's refusal, in its own words: every argument given (None: an optional one that was not) is a device tensor."""
    for t in tensors:
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise BasedetHipError(f"{module} needs tensors on a HIP device; there is no CPU fallback")


def to_pm(x):
    N, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(N * H * W, C).to(BF16).contiguous()


def to_nchw(t, N, H, W):
    return t.float().reshape(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


def load_strict(state, want, device, extra_ok=False):
    """Strict names and shapes -> fp32 device tensors; nothing is returned (or changed) unless every entry passes."""
    extra = sorted(set(state) - set(want))
    if extra and not extra_ok:
        raise KeyError(f"unexpected parameter(s) {extra}")
    out = {}
    for k, shape in want.items():
        if k not in state:
            raise KeyError(f"missing parameter {k!r}")
        v = torch.as_tensor(np.asarray(state[k]) if not torch.is_tensor(state[k]) else state[k]).detach().float()
        if tuple(v.shape) != tuple(shape):
            raise ValueError(f"parameter {k!r}: shape {tuple(v.shape)}, expected {tuple(shape)}")
        out[k] = v.to(device).contiguous()
    return out


def workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def check_views(shapes, w, g):
    """ValueError unless w and g hold a view of each of `shapes`; nothing is touched."""
    for name, shape in shapes.items():
        if tuple(w[name].shape) != tuple(shape) or tuple(g[name].shape) != tuple(shape):
            raise ValueError(f"adopt: {name!r} needs fp32 views of shape {tuple(shape)}")


class ParamStore:
    """The fp32 masters `w` and parameter gradients `g` of one layer: {name: tensor} in the kernels' own layouts (`shapes`, the layer's
    arena_shapes()).  A layer starts on storage it allocates here; move() puts it on storage a caller provides (a model's parameter
    arena).  Either way the layer has one path: it packs from `w` and its backward writes into `g`."""

    def __init__(self, shapes, device):
        self.shapes, self.device = shapes, device
        self.w = {k: torch.zeros(s, dtype=F32, device=device) for k, s in shapes.items()}
        self.g = None

    def grad(self, accumulate):
        """(g, accumulate) for a backward.  The storage is allocated once, at the first backward, which has nothing to add onto."""
        if self.g is None:
            self.g = {k: torch.empty(s, dtype=F32, device=self.device) for k, s in self.shapes.items()}
            return self.g, False
        return self.g, accumulate

    def check(self, w, g):
        """ValueError unless w and g hold views of `shapes`; nothing is touched."""
        check_views(self.shapes, w, g)

    def move(self, w, g):
        """The current values move into w; w and g (fp32 device views of `shapes`) are the masters and gradients from here on."""
        self.check(w, g)
        for name in self.shapes:
            w[name].copy_(self.w[name])
        self.w, self.g = {k: w[k] for k in self.shapes}, {k: g[k] for k in self.shapes}


class Container:
    """A composition of layers and other Containers: `_children()` lists them under the reference's names and order, and the layer
    protocol follows from theirs."""
    training = True

    def _children(self):
        raise NotImplementedError

    def _leaves(self):
        """[(name, layer)] of the layers that are not Containers, in the reference's order."""
        out = []
        for n, c in self._children():
            out += [(f"{n}.{k}", v) for k, v in c._leaves()] if isinstance(c, Container) else [(n, c)]
        return out

    def _merge(self, fn):
        return {f"{n}.{k}": v for n, c in self._children() for k, v in fn(c).items()}

    def _shapes(self):
        return self._merge(lambda c: c._shapes())

    def names(self):
        return list(self._shapes())

    def params(self):
        return self._merge(lambda c: c.params())

    def grads(self):
        return self._merge(lambda c: c.grads())

    def state_dict(self):
        return self._merge(lambda c: c.state_dict())

    def load_state_dict(self, state):
        """Strict: every name and shape is checked before any child loads."""
        p = load_strict(state, self._shapes(), self.device)
        for n, c in self._children():
            c.load_state_dict(cut(p, n))

    def repack(self):
        for _, c in self._children():
            c.repack()

    def arena_shapes(self):
        """name -> shape of the fp32 masters in the kernels' layouts, "<leaf>.<the leaf's name>".  The norms' vectors are not listed:
        adopt() takes norm records."""
        return self._merge(lambda c: c.arena_shapes())

    def adopt(self, w, g, norms):
        """Live on the caller's storage (a model's parameter arena): w / g = {name: fp32 view} of arena_shapes(), norms =
        {"<leaf>.<norm>": the model's norm record} for every name in a leaf's NORMS.  Every shape is checked before anything moves: a
        refused adopt leaves every leaf where it was."""
        plan = [(c, cut(w, n), cut(g, n), [norms[f"{n}.{r}"] for r in c.NORMS]) for n, c in self._leaves()]
        for c, cw, cg, _ in plan:
            check_views(c.arena_shapes(), cw, cg)
        for c, cw, cg, recs in plan:
            c.adopt(cw, cg, *recs)

    def refresh_eval(self):
        for _, c in self._children():
            c.refresh_eval()

    def train(self, mode=True):
        self.training = bool(mode)
        for _, c in self._children():
            c.train(mode)
        return self

    def eval(self):
        return self.train(False)


class Block(Container):
    """A Container with one pixel-major input and one output of the same size: the NCHW wrappers."""

    def __call__(self, x):
        need_device(x, type(self).__name__)
        N, C, H, W = x.shape
        if C != self.cin:
            raise ValueError(f"input has {C} channels, the layer {self.cin}")
        self._in_size = (N, H, W)
        return to_nchw(self.forward_pm(to_pm(x), N, H, W), N, H, W)

    forward = __call__

    def backward(self, dy, accumulate=False):
        need_device(dy, type(self).__name__ + ".backward")
        if getattr(self, "_in_size", None) is None:
            raise RuntimeError("backward() before a forward")
        N, H, W = self._in_size
        if tuple(dy.shape) != (N, self.cout, H, W):
            raise ValueError(f"gradient shape {tuple(dy.shape)} does not match the forward output")
        return to_nchw(self.backward_pm(to_pm(dy), accumulate), N, H, W)
