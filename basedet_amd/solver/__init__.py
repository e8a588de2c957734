"""DetSolver (basedet/solver/default_solver.py:79-124) + the basecore `Solver.minimize` step it returns.

lr = BASIC_LR * BATCHSIZE * world_size for MEAN reduction (:99-106); SOLVER.OPTIMIZER_NAME (SGD, Adam or AdamW, :47-55) over the
trainable parameter arena in ONE fused launch; gradients are all-reduced (mean) over RCCL in arena buckets that
follow the backward order (head -> FPN -> layer4 -> ... -> layer2) on the communicator's stream, overlapped with backward.
The collectives are the bd_comm_* entry points of the C ABI (basedet_amd/comm.py); no c10d process group is involved.
"""
import math

import numpy as np
import torch

from .. import comm as _comm
from .. import ops
from ..streams import fork, join
from ..utils.registry import registers


class _ParamGroupView(dict):
    pass


def _moments_out(model, buf):
    """An arena-shaped buffer as {reference parameter name: numpy array in the reference's shape}: `buf` trades places with the arena's
    weights and the model's own export gathers it (layouts, fused predictors, PaddedClsConv's pad rows dropped) -- the way
    ModelEMA.state_dict reads its average."""
    w = model.arena.w
    ops.swap_f32(buf, w)
    try:
        states = model.state_dict()
    finally:
        ops.swap_f32(buf, w)
    return {k: states[k] for k in model.state_dict_trainable_names()}


def _moments_in(model, buf, values):
    """The inverse of `_moments_out`, through the model's own binding code (pad rows come back as zeros); the live weights are untouched."""
    own = model.state_dict()
    trainable = set(model.state_dict_trainable_names())
    missing = sorted(trainable - set(values))
    if missing:
        raise ValueError(f"optimizer state lacks {len(missing)} trainable parameter(s), e.g. {missing[0]!r}")
    merged = {k: (values[k] if k in trainable else v) for k, v in own.items()}
    w = model.arena.w
    try:
        ops.swap_f32(buf, w)
        try:
            model._bind_params(merged)
        finally:
            ops.swap_f32(buf, w)
    finally:
        model.repack_weights()


class SGD:
    """megengine.optimizer.SGD semantics: g' = g + wd*w; v = momentum*v + g'; w -= lr*v, or with `nesterov` w -= lr*(g' + momentum*v)
    (fused HIP kernels)."""

    def __init__(self, model, lr, weight_decay, momentum=0.9, nesterov=False):
        if nesterov and momentum <= 0:                   # megengine/optimizer/sgd.py raises the same
            raise ValueError("SGD: nesterov=True requires a momentum > 0")
        self.model = model
        self.nesterov = bool(nesterov)
        self.step_count = 0
        self.param_groups = [_ParamGroupView(lr=lr, weight_decay=weight_decay, momentum=momentum)]

    def step(self, grad_scale=1.0, ema=None):
        """`ema`: the trainer's ModelEMA (engine/trainer.py:98-100 steps it right after minimize).  Past its burn-in the average is
        updated from the new weights inside this launch (bd_sgd_momentum_ema_step; `ema.step()` then only counts); up to and including
        the burn-in iteration, and without `ema`, the launch is the plain one.  With `nesterov` the two launches are
        bd_sgd_nesterov_step / bd_sgd_nesterov_ema_step."""
        a = self.model.arena
        g = self.param_groups[0]
        m = ema.fused_momentum() if ema is not None else None
        plain, fused = (ops.sgd_nesterov_step, ops.sgd_nesterov_ema_step) if self.nesterov else \
            (ops.sgd_momentum_step, ops.sgd_momentum_ema_step)
        if m is None:
            plain(a.w, a.v, a.g, g["lr"], g["momentum"], g["weight_decay"], grad_scale)
        else:
            fused(a.w, a.v, a.g, ema.e, g["lr"], g["momentum"], g["weight_decay"], grad_scale, m)
        self.step_count += 1
        self.model.repack_trainable()
        return self

    def clear_grad(self):
        return self   # every gradient slot is overwritten by the next backward (no accumulation across steps)

    def state_dict(self):
        """For TRAINER.RESUME: {"step", "momentum_buffer": {parameter name: array in the reference's shape}}."""
        return {"step": self.step_count, "momentum_buffer": _moments_out(self.model, self.model.arena.v)}

    def load_state_dict(self, states):
        self.step_count = int(states["step"])
        _moments_in(self.model, self.model.arena.v, states["momentum_buffer"])


class Adam:
    """megengine.optimizer.Adam semantics in one fused HIP launch (bd_adam_step): g' = g + wd*w; m = b1*m + (1 - b1)*g';
    v = b2*v + (1 - b2)*g'^2; w -= lr * (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps), t = the step number from 1.

    The first moment lives in `arena.v` (the buffer SGD keeps its velocity in); the second moment is this object's own buffer.  The
    step count stays on the host: the bias corrections travel to the kernel as arguments."""

    decoupled = False

    def __init__(self, model, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8):
        if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
            raise ValueError(f"{type(self).__name__}: betas must be two values in [0, 1), got {betas!r}")
        betas = (float(betas[0]), float(betas[1]))
        if eps < 0:
            raise ValueError(f"{type(self).__name__}: eps must not be negative, got {eps!r}")
        self.model = model
        self.step_count = 0
        self.param_groups = [_ParamGroupView(lr=lr, weight_decay=weight_decay, betas=betas, eps=eps)]
        a = model.arena
        self.exp_avg_sq = torch.zeros(a.total, dtype=torch.float32, device=a.w.device)

    def step(self, grad_scale=1.0, ema=None):
        """`ema`: as SGD.step -- past the burn-in the average is updated inside this launch (bd_adam_ema_step)."""
        a = self.model.arena
        g = self.param_groups[0]
        m = ema.fused_momentum() if ema is not None else None
        t = self.step_count + 1
        if m is None:
            ops.adam_step(a.w, a.v, self.exp_avg_sq, a.g, g["lr"], g["betas"], g["eps"], g["weight_decay"], t, grad_scale,
                          self.decoupled)
        else:
            ops.adam_ema_step(a.w, a.v, self.exp_avg_sq, a.g, ema.e, g["lr"], g["betas"], g["eps"], g["weight_decay"], t, grad_scale,
                              self.decoupled, m)
        self.step_count = t
        self.model.repack_trainable()
        return self

    def clear_grad(self):
        return self   # as SGD.clear_grad

    def state_dict(self):
        """For TRAINER.RESUME: {"step", "exp_avg", "exp_avg_sq"}, the moments as {parameter name: array in the reference's shape}."""
        return {"step": self.step_count, "exp_avg": _moments_out(self.model, self.model.arena.v),
                "exp_avg_sq": _moments_out(self.model, self.exp_avg_sq)}

    def load_state_dict(self, states):
        self.step_count = int(states["step"])
        _moments_in(self.model, self.model.arena.v, states["exp_avg"])
        _moments_in(self.model, self.exp_avg_sq, states["exp_avg_sq"])


class AdamW(Adam):
    """megengine.optimizer.AdamW: Adam with the decay decoupled from the gradient -- w -= lr * (m^ / (sqrt(v^) + eps) + wd*w)."""

    decoupled = True


# SOLVER.OPTIMIZER_NAME -> (class, the EXTRA_OPT_ARGS it takes): megengine.optimizer's names
OPTIMIZERS = {"SGD": (SGD, ("momentum", "nesterov")), "Adam": (Adam, ("betas", "eps")), "AdamW": (AdamW, ("betas", "eps"))}


def build_optimizer(name, model, lr, weight_decay, extra):
    """`getattr(megengine.optimizer, name)(params, lr=, weight_decay=, **extra)` (solver/default_solver.py:47-55) over the three
    optimizers this build has; anything else raises instead of training with another rule."""
    if name not in OPTIMIZERS:
        raise ValueError(f"SOLVER.OPTIMIZER_NAME = {name!r} is not supported: one of {sorted(OPTIMIZERS)} is implemented")
    cls, takes = OPTIMIZERS[name]
    unknown = sorted(set(extra) - set(takes))
    if unknown:
        raise ValueError(f"SOLVER.EXTRA_OPT_ARGS {unknown} not supported by OPTIMIZER_NAME = {name!r}: it takes {list(takes)}")
    if cls is SGD:
        extra = dict(extra)
        extra.setdefault("momentum", 0.0)               # megengine.optimizer.SGD's default
    return cls(model, lr=lr, weight_decay=weight_decay, **extra)


class GradBuckets:
    """Asynchronous bucketed all-reduce of the gradient arena (replaces dist.make_allreduce_cb,
    solver/default_solver.py:121).  Buckets = contiguous arena ranges closed in backward order."""

    def __init__(self, model, mode="MEAN", comm=None, wire_dtype="fp32"):
        self.model = model
        self.mode = mode
        # SOLVER.ALLREDUCE_DTYPE = "bf16" (opt-in): the buckets cross xGMI as bf16 (75 MB instead of 151 MB per step for RetinaNet-R50);
        # the update then differs from the fp32 exchange by bf16 resolution (rel-L2 ~1e-3: tests/test_dist_cpu.py, test_dist_gpu.py)
        assert wire_dtype in ("fp32", "bf16"), wire_dtype
        self.wire_dtype = wire_dtype
        self._wire_tmp = None
        self.comm = comm if comm is not None else _comm.get_comm()
        # a communicator of one rank (BD_FORCE_ALLREDUCE=1 in bench / tests) still sends every bucket through RCCL: the identity
        # reduction exercises the stream plumbing on a single GPU
        self.enabled = self.comm is not None
        self.world = self.comm.world if self.enabled else 1
        self.ranges = self._ranges()

    def _ranges(self):
        """name of the backward phase -> (start, end) element range of the arena.  A model that defines grad_buckets() (YOLOX: one
        bucket) supplies its own."""
        if hasattr(self.model, "grad_buckets"):
            return dict(self.model.grad_buckets())
        ent = self.model.arena.entries
        groups = {}
        for name, _, off, n in ent:
            if name.startswith(("head.", "rpn.", "rcnn.", "upsample.")):       # (upsample.: CenterNet's neck, finished with its head)
                k = "head"
            elif "fpn_" in name or "top_block" in name:
                k = "fpn"
            else:
                parts = name.split(".")    # backbone.bottom_up.layerX... (CenterNet holds the bare ResNet: backbone.layerX...)
                k = parts[2] if parts[1] == "bottom_up" else parts[1]
                if k == "bn1":             # the stem's live norm (MODEL.BACKBONE.NORM): finished with conv1's weight gradient
                    k = "conv1"
            lo, hi = groups.get(k, (off, off))
            groups[k] = (min(lo, off), max(hi, (off + n + 63) // 64 * 64))
        return groups

    def on_ready(self, phase, producers=()):
        """All gradients of `phase` have been ENQUEUED on the current stream and on the `producers` streams (the weight-gradient
        side stream).  bd_comm_allreduce_async records an event on each of them, makes the communication stream wait for those
        events and enqueues the collective there -- the compute streams never wait for each other or for the collective, and the
        host does not block."""
        if not self.enabled or phase not in self.ranges:
            return
        lo, hi = self.ranges[phase]
        buf = self.model.arena.g[lo:hi]
        prod = []
        if buf.is_cuda:
            prod = [torch.cuda.current_stream()] + [s for s in producers if s is not None]
        if self.wire_dtype == "bf16":
            if self._wire_tmp is None:
                self._wire_tmp = torch.empty(self.model.arena.g.numel(), dtype=torch.bfloat16, device=buf.device)
            self.comm.allreduce_async_bf16(buf, self._wire_tmp[lo:hi], prod, "sum")      # each bucket has its own slice of the scratch
        else:
            self.comm.allreduce_async(buf, prod, "sum")

    def wait(self):
        """The current stream (the SGD launch comes next) waits for every bucket; returns the gradient scale of the reduce mode."""
        if self.enabled:
            self.comm.wait()
        return 1.0 / self.world if (self.enabled and self.mode == "MEAN") else 1.0


class GradClip:
    """What basecore's `clip_grad(params, type, **args)` returns (engine/trainer.py:57-61; configs/extra_cfg.py:99-105): a callable the
    solver invokes between the gradient all-reduce and the optimizer step.  TYPE "value" (ARGS lower, upper) =
    megengine.optimizer.clip_grad_value, TYPE "norm" (ARGS max_norm, ord = 2) = clip_grad_norm over ALL trainable gradients -- here one
    or three launches over the flat gradient arena (bd_clip_grad_value / bd_clip_grad_norm), no host synchronisation.  The
    reduce-mode factor (1 / world) the SGD launch would apply is folded in (`pre_scale`): the reference clips the averaged gradients."""

    def __init__(self, model, clip_type="value", **args):
        assert clip_type in ("value", "norm"), clip_type            # basecore asserts the same two types
        self.model, self.type, self.args = model, clip_type, dict(args)
        if clip_type == "value":
            self.lower, self.upper = float(args["lower"]), float(args["upper"])
        else:
            self.max_norm, self.ord = float(args["max_norm"]), float(args.get("ord", 2.0))
        self.last_norm = None          # device scalar: the gradient norm of the last step (TYPE "norm")
        self._ws = None

    def __call__(self, pre_scale=1.0):
        g = self.model.arena.g
        if self.type == "value":
            ops.clip_grad_value(g, self.lower, self.upper, pre_scale)
        else:
            if self._ws is None:
                self._ws = torch.empty((ops.clip_grad_norm_workspace_bytes(),), dtype=torch.uint8, device=g.device)
                self.last_norm = torch.zeros((1,), dtype=torch.float32, device=g.device)
            ops.clip_grad_norm(g, self.max_norm, self.ord, pre_scale, self.last_norm, self._ws)
        return 1.0


def clip_grad(model, clip_type="value", **args):
    """basecore.engine.clip_grad with the model in place of its parameter list (the gradients live in model.arena.g)."""
    return GradClip(model, clip_type, **args)


class GradScaler:
    """Stand-in for megengine.amp.GradScaler as DetSolver builds it (solver/default_solver.py:66-76: init_scale 65536 with
    DYNAMIC_SCALE, else 128; growth_interval 2000 / 0).  The reference needs it because its AMP is fp16; this build's mixed precision is
    bf16 activations with fp32 accumulation and fp32 master weights, which has fp32's exponent range, so the scale factor is
    carried for the protocol (`solver.grad_scaler is not None`, engine/trainer.py:53-54) and never applied."""

    def __init__(self, init_scale=128.0, growth_interval=0):
        self.scale_factor = float(init_scale)
        self.growth_interval = int(growth_interval)


class Solver:
    """basecore.engine.Solver protocol used by DetTrainer (engine/trainer.py:55-61,98)."""

    def __init__(self, optimizer, buckets, grad_scaler=None, grad_clip_fn=None):
        self.optimizer = optimizer
        self.buckets = buckets
        self.grad_scaler = grad_scaler
        self.grad_clip_fn = grad_clip_fn

    def minimize(self, model, inputs, ema=None):
        """One training step (basecore Solver.minimize; called at engine/trainer.py:98); `ema`: see SGD.step.  `high_priority_main = True` runs the step's main
        chain (forward, losses, data gradients, SGD) on a HIGH-priority stream owned by the solver, ahead of the weight-gradient side
        stream at workgroup dispatch (the caller's stream waits for it at the end).  Round 2 measured +0.8 % for it; since layer1 runs as
        one persistent launch per block (round 3) the caller's default-priority stream is the faster one -- 9 of 9 alternations on two
        boxes, +0.5 % on average -- and is the default."""
        hp = self._main_stream(model)
        with fork(hp):
            losses = self._step(model, inputs, ema)
        join(hp)
        return losses

    def _main_stream(self, model):
        if not getattr(self, "high_priority_main", False) or not torch.cuda.is_available() or getattr(model, "device", None) is None \
                or model.device.type != "cuda":
            return None
        if getattr(self, "_hp", None) is None:
            self._hp = torch.cuda.Stream(device=model.device, priority=-1)
        return self._hp

    def _step(self, model, inputs, ema=None):
        losses = model(inputs)
        model.backward(on_bucket_ready=self.buckets.on_ready)
        prof = getattr(self, "comm_profile", None)        # bench.py (N > 1): [(backward done on this stream, collectives done on the comm stream)]
        if prof is not None and self.buckets.enabled and torch.cuda.is_available():
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
        scale = self.buckets.wait()
        if prof is not None and self.buckets.enabled and torch.cuda.is_available():
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(self.buckets.comm.stream)
            prof.append((e0, e1))
        if self.grad_clip_fn is not None:                 # engine/trainer.py:57-61: between the all-reduce and the optimizer step
            if isinstance(self.grad_clip_fn, GradClip):
                scale = self.grad_clip_fn(pre_scale=scale)
            else:                                         # a foreign callable sees the averaged gradients
                if scale != 1.0:
                    model.arena.g.mul_(scale)
                self.grad_clip_fn()
                scale = 1.0
        if ema is None:
            self.optimizer.step(grad_scale=scale)
        else:
            self.optimizer.step(grad_scale=scale, ema=ema)
        self.optimizer.clear_grad()
        return losses


class WarmupMultiStepLR:
    """LRSchedulerHook.build_lr_scheduler (engine/hooks.py:222-248): MultiStepLR with iteration-wise milestones
    (epochs * iters_per_epoch) wrapped in basecore's WarmUpScheduler(scheduler, warmup_length=WARM_ITERS).

    basecore is not vendored, so the SHAPE of its warm-up ramp is an assumption of this build (parity unpinned):
    by default a linear ramp lr * (it + 1) / WARM_ITERS that reaches the base rate at the last warm-up iteration.  Two config keys
    select the other common forms should basecore's differ: SOLVER.WARMUP_START_FACTOR = f ramps lr * (f + (1 - f) * it / WARM_ITERS)
    (detectron-style, starts at f * lr); SOLVER.WARMUP_MODE = "constant" holds lr * f for the whole warm-up."""

    def __init__(self, optimizer, cfg, world_size=1):
        s = cfg.SOLVER
        self.optimizer = optimizer
        self.base_lr = optimizer.param_groups[0]["lr"]
        iters_per_epoch = int(s.NUM_IMAGE_PER_EPOCH / world_size / cfg.MODEL.BATCHSIZE)     # engine/trainer.py:48
        self.milestones = [int(e) * iters_per_epoch for e in s.LR_DECAY_STAGES]
        self.gamma = s.LR_DECAY_RATE
        self.warm_iters = s.get("WARM_ITERS", 0)
        self.warm_mode = s.get("WARMUP_MODE", "linear")
        self.warm_start = s.get("WARMUP_START_FACTOR", None)
        assert self.warm_mode in ("linear", "constant")

    def lr_at(self, it):
        lr = self.base_lr * self.gamma ** sum(1 for m in self.milestones if it >= m)
        if it < self.warm_iters:
            if self.warm_mode == "constant":
                lr *= self.warm_start if self.warm_start is not None else 1.0 / self.warm_iters
            elif self.warm_start is not None:
                lr *= self.warm_start + (1.0 - self.warm_start) * it / self.warm_iters
            else:
                lr *= (it + 1) / self.warm_iters
        return lr

    def step(self, it):
        self.optimizer.param_groups[0]["lr"] = self.lr_at(it)


@registers.solvers.register()
class DetSolver:
    @classmethod
    def build(cls, cfg, model):
        solver_cfg = cfg.SOLVER
        mode = solver_cfg.get("REDUCE_MODE", "MEAN")
        assert mode in ["MEAN", "SUM"]
        world = _comm.world_size()
        lr = solver_cfg.BASIC_LR * cfg.MODEL.BATCHSIZE
        wd = solver_cfg.WEIGHT_DECAY
        if mode == "MEAN":
            lr = lr * world
        else:
            wd = wd * world
        extra = dict(solver_cfg.get("EXTRA_OPT_ARGS", {}))
        opt = build_optimizer(solver_cfg.get("OPTIMIZER_NAME", "SGD"), model, lr, wd, extra)
        amp = cfg.get("TRAINER", {}).get("AMP", {}) if hasattr(cfg, "get") else {}
        scaler = None
        if amp.get("ENABLE", False):                      # default_solver.py:66-76
            dyn = bool(amp.get("DYNAMIC_SCALE", False))
            scaler = GradScaler(65536.0 if dyn else 128.0, 2000 if dyn else 0)
        return Solver(opt, GradBuckets(model, mode, wire_dtype=str(solver_cfg.get("ALLREDUCE_DTYPE", "fp32"))), grad_scaler=scaler)


class YOLOXSGD(SGD):
    """The optimizer of solver/yolox_solver.py: Nesterov SGD whose weight decay reaches the convolution weights only.  The model's arena
    holds them in front -- elements [0, model.decay_end) -- and every 1-D parameter (BN gamma / beta, the predictor biases) behind, so
    the step is the existing launch run on the two slices, with the moment and EMA buffers sliced likewise: no new kernel.  Two
    param_groups in arena order ("range": their element range); a scheduler sets `lr` on both."""

    def __init__(self, model, lr, weight_decay, momentum=0.9):
        super().__init__(model, lr, weight_decay, momentum=momentum, nesterov=True)
        cut, total = int(model.decay_end), int(model.arena.total)
        assert 0 <= cut <= total and cut % 64 == 0, (cut, total)
        self.param_groups = [_ParamGroupView(lr=lr, weight_decay=weight_decay, momentum=momentum, range=(0, cut)),
                             _ParamGroupView(lr=lr, weight_decay=0.0, momentum=momentum, range=(cut, total))]

    def step(self, grad_scale=1.0, ema=None):
        a = self.model.arena
        m = ema.fused_momentum() if ema is not None else None
        for g in self.param_groups:
            lo, hi = g["range"]
            if hi == lo:
                continue
            if m is None:
                ops.sgd_nesterov_step(a.w[lo:hi], a.v[lo:hi], a.g[lo:hi], g["lr"], g["momentum"], g["weight_decay"], grad_scale)
            else:
                ops.sgd_nesterov_ema_step(a.w[lo:hi], a.v[lo:hi], a.g[lo:hi], ema.e[lo:hi], g["lr"], g["momentum"], g["weight_decay"],
                                          grad_scale, m)
        self.step_count += 1
        self.model.repack_trainable()
        return self


class YoloxLR:
    """YoloxLRSchedulerHook (engine/yolo_hooks.py:15-59): quadratic warm-up over SOLVER.WARM_EPOCH epochs from lr * MIN_LR_RATIO, a
    cosine down to lr * MIN_LR_RATIO, and that rate held for the last AUG.TRAIN_SETTING.NO_AUG_EPOCH epochs.  `epoch` and `it` count from
    1, as basecore's Progress does; every param_group follows the one rate."""

    def __init__(self, optimizer, cfg, world_size=1):
        s = cfg.SOLVER
        self.optimizer = optimizer
        self.lr = optimizer.param_groups[0]["lr"]
        self.min_lr = self.lr * s.MIN_LR_RATIO
        self.warm_epoch, self.no_aug_epoch = int(s.WARM_EPOCH), int(cfg.AUG.TRAIN_SETTING.NO_AUG_EPOCH)
        self.max_epoch = int(s.MAX_EPOCH)
        self.max_iter = int(s.NUM_IMAGE_PER_EPOCH / world_size / cfg.MODEL.BATCHSIZE)          # engine/trainer.py:48

    def lr_at(self, epoch, it):
        if epoch <= self.warm_epoch:
            cur = (epoch - 1) * self.max_iter + it
            return (self.lr - self.min_lr) * pow(cur / float(self.warm_epoch * self.max_iter), 2) + self.min_lr
        if epoch > self.max_epoch - self.no_aug_epoch:
            return self.min_lr
        cur = (epoch - self.warm_epoch) * self.max_iter + it
        span = (self.max_epoch - self.warm_epoch - self.no_aug_epoch) * self.max_iter
        return self.min_lr + 0.5 * (self.lr - self.min_lr) * (1.0 + math.cos(math.pi * (cur - self.warm_epoch * self.max_iter) / span))

    def step(self, epoch, it):
        lr = self.lr_at(epoch, it)
        for g in self.optimizer.param_groups:
            g["lr"] = lr


class SyncSizeHook:
    """engine/yolo_hooks.py:62-89: every `change_iter` iterations rank 0 draws the training size from `sizes`, the draw is broadcast,
    and the model's target_size is set; the model's pre_process resizes the next batches to it.  The draw comes from a generator seeded
    here (the reference uses numpy's global one), so a run can be repeated."""

    def __init__(self, model, sizes, change_iter=10, seed=0):
        self.model, self.sizes, self.change_iter = model, [int(v) for v in sizes], int(change_iter)
        self.rng = np.random.default_rng(seed)

    @classmethod
    def build(cls, cfg, model, seed=0):
        """engine/build.py:63-69; None when AUG.TRAIN_SETTING.MULTISCALE_RANGE is empty."""
        t = cfg.AUG.TRAIN_SETTING
        rng = tuple(t.get("MULTISCALE_RANGE", ()) or ())
        if not rng:
            return None
        lo, hi = rng
        return cls(model, [32 * x for x in range(lo, hi + 1)], t.SYNC_ITER, seed)

    def before_iter(self, epoch, it, max_iter):
        cur = (epoch - 1) * max_iter + it
        if not self.model.training or cur % self.change_iter:
            return
        size = int(self.rng.choice(self.sizes)) if _comm.rank() == 0 else 0
        c = _comm.get_comm()
        if c is not None and c.world > 1:
            t = torch.tensor([size], dtype=torch.int32, device=self.model.device)
            c.bcast(t, root=0)
            size = int(t.item())
        self.model.target_size = (size, size)


@registers.solvers.register()
class YOLOXSolver:
    """solver/yolox_solver.py: lr = BASIC_LR * BATCHSIZE * world, Nesterov SGD with SOLVER.MOMENTUM, WEIGHT_DECAY on the convolution
    weights only (YOLOXSGD)."""

    @classmethod
    def build(cls, cfg, model):
        s = cfg.SOLVER
        if not hasattr(model, "decay_end"):
            raise ValueError("YOLOXSolver needs a model whose arena separates the decayed weights (decay_end): YOLOX")
        lr = s.BASIC_LR * cfg.MODEL.BATCHSIZE * _comm.world_size()
        opt = YOLOXSGD(model, lr=float(lr), weight_decay=s.WEIGHT_DECAY, momentum=s.MOMENTUM)
        return Solver(opt, GradBuckets(model, s.get("REDUCE_MODE", "MEAN"), wire_dtype=str(s.get("ALLREDUCE_DTYPE", "fp32"))))


def broadcast_parameters(model, src=0):
    """configs/detection_cfg.py:80-82 (dist.bcast_list_ of params and buffers) as one flat broadcast."""
    c = _comm.get_comm()
    if c is not None and c.world > 1:
        c.bcast(model.arena.w, root=src)
        if getattr(model, "norms", None):      # buffers: the running statistics of every live norm (backbone and FPN)
            c.bcast(model.norms.running, root=src)
        model.repack_trainable()
