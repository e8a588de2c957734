"""What the pixel-major layers (deformable.py, center_head.py, yolox_head.py, batch_norm.py) share: the NCHW fp32 <-> pixel-major bf16
[N H W][C] wrappers, the strict state loader, workspaces, and ParamStore -- the fp32 masters and parameter gradients of one layer."""
import numpy as np
import torch

from .._lib import BasedetHipError

BF16, F32 = torch.bfloat16, torch.float32


def round_up8(n):
    return (n + 7) // 8 * 8


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
        for name, shape in self.shapes.items():
            if tuple(w[name].shape) != shape or tuple(g[name].shape) != shape:
                raise ValueError(f"adopt: {name!r} needs fp32 views of shape {shape}")

    def move(self, w, g):
        """The current values move into w; w and g (fp32 device views of `shapes`) are the masters and gradients from here on."""
        self.check(w, g)
        for name in self.shapes:
            w[name].copy_(self.w[name])
        self.w, self.g = {k: w[k] for k in self.shapes}, {k: g[k] for k in self.shapes}
