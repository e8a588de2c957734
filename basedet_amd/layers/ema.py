"""Model EMA (basedet/layers/common/ema.py:10-93): a moving average of the weights, kept next to the parameter arena.

The reference deep-copies the model and updates every parameter and buffer tensor by tensor.  Here the average is ONE fp32 buffer
with the layout of `model.arena.w`, updated by one launch (bd_ema_update) or inside the SGD launch (bd_sgd_momentum_ema_step), and
evaluated by trading places with the arena's weights (`applied()`, bd_swap_f32) -- no second model exists.  A model with live batch
norms (MODEL.BACKBONE.NORM / MODEL.FPN.NORM = "BN" / "SyncBN") has buffers that move too: their average is a second fp32 buffer with
the layout of `model.norms.running`, updated by a bd_ema_update launch of its own and swapped along with the first."""
import contextlib

from .. import ops


def calculate_momentum(alpha, total_iter, update_period):
    """ema.py:10-29 (pycls style): the momentum that makes `alpha` mean the same whatever the schedule length and update period;
    90000 is the iteration count of a 1x COCO schedule."""
    return max(0, 1 - alpha * (90000 * update_period / total_iter))


class ModelEMA:
    """ema.py:32-93 over the trainable arena: `e = e * m + (1 - m) * w`, both products and the sum rounded to fp32 (no FMA).

    State: `e`, fp32, the shape and device of `model.arena.w`, a copy of it at construction; and, when the model has live norms, `r`,
    the same for `model.norms.running` (every live norm's running_mean / running_var: ema.py:52-55 averages the buffers too), else
    None.  DEVIATION: frozen parameters and FrozenBN buffers never change, so they are not duplicated -- `state_dict()["model"]` holds
    the model's own values for them, where the reference computes `m * x + (1 - m) * x`, which can differ from x in the last bit."""

    def __init__(self, model, momentum, start_iter=0, burnin_iter=2000):
        self.model = model
        self.momentum = momentum
        self.iters = start_iter
        self.burnin_iter = burnin_iter
        self.e = model.arena.w.clone()
        norms = getattr(model, "norms", None)
        self.r = norms.running.clone() if norms else None
        self._fused = False            # the optimizer has already applied this iteration's update (fused_momentum)

    def step(self):
        """ema.py:57-69: nothing below `burnin_iter`; at it, `update(0)` (the average becomes the weights) then `update(momentum)`;
        above it, `update(momentum)` -- unless SGD.step folded that update into its launch, then the counter advances and only the
        norm buffers, which no optimizer launch sees, are averaged here."""
        self.iters += 1
        if self._fused:
            self._fused = False
            self._update_buffers(self.momentum)
            return
        if self.iters < self.burnin_iter:
            return
        elif self.iters == self.burnin_iter:
            self.update(0)
        self.update(self.momentum)

    def fused_momentum(self):
        """For SGD.step(ema=...): the momentum to fold into the optimizer launch that is about to run, or None when the `step()`
        that follows it is a burn-in iteration (nothing, or the two-update start) and runs its own launches."""
        if self.iters + 1 > self.burnin_iter:
            self._fused = True
            return self.momentum
        return None

    def update(self, m):
        """ema.py:71-81 for every trainable element in one launch (bd_ema_update), and one more for the live norms' buffers."""
        ops.ema_update(self.e, self.model.arena.w, m)
        self._update_buffers(m)

    def _update_buffers(self, m):
        if self.r is not None:
            ops.ema_update(self.r, self.model.norms.running, m)

    def _swap(self):
        ops.swap_f32(self.e, self.model.arena.w)
        if self.r is not None:
            ops.swap_f32(self.r, self.model.norms.running)

    @contextlib.contextmanager
    def _swapped(self):
        self._swap()
        try:
            yield
        finally:
            self._swap()

    @contextlib.contextmanager
    def applied(self):
        """Inside the block the model IS the averaged model (engine/hooks.py:274-284 evaluates `ema.ema`): the average and the arena's
        weights trade places, so do the averaged and the live running statistics, and the packed bf16 copies follow -- with them, in
        eval(), the folded affine of every live norm (repack_trainable; a later eval() folds what is in place then); on exit all are
        put back, so training continues with the same bits.  bf16 weights only: with fp8 weights the repack would also re-stage the
        delayed scales."""
        dt = getattr(self.model, "weight_dtype", "bf16")
        if dt != "bf16":
            raise ValueError(f"ModelEMA.applied() with MODEL.WEIGHT_DTYPE = {dt!r} is not supported: only 'bf16' is implemented")
        self._swap()
        self.model.repack_trainable()
        try:
            yield self.model
        finally:
            self._swap()
            self.model.repack_trainable()

    def state_dict(self):
        """ema.py:89-93: {"iter", "model"} with the keys and layouts of `model.state_dict()`."""
        with self._swapped():
            states = self.model.state_dict()
        return {"iter": self.iters, "model": states}

    def load_state_dict(self, states):
        """ema.py:83-87.  Trainable entries go into `e`, and the running statistics of live norms into `r`, through the model's own
        binding code (layouts, padding, fused predictors); frozen entries of `states` are ignored (see the class docstring)."""
        state_iters = states.get("iter", None)
        if state_iters is not None:
            self.iters = state_iters
        self._load_model(states["model"])

    def _load_model(self, values):
        own = self.model.state_dict()
        averaged = set(self.model.state_dict_trainable_names())
        if self.r is not None:
            averaged.update(n.name + s for n in self.model.norms for s in (".running_mean", ".running_var"))
        merged = {k: (values[k] if k in averaged else v) for k, v in own.items()}
        try:
            with self._swapped():
                self.model._bind_params(merged)
        finally:
            self.model.repack_weights()
            if self.r is not None and not self.model.training:      # _bind_params folded the averaged norms: back to the model's own
                self.model._fold_norms()
