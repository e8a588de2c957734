"""Delayed scaling and stochastic rounding of the e5m2 gradients of the fp8 layers: probe readings -> per-group history -> power-of-two
scale -> staged per layer until the next weight repack."""
import numpy as np
import torch

from .. import ops


def initial_grad_scale(m):
    """MODEL.FP8_GRAD_SCALE: the initial (pre-probe) scale of the e5m2 gradients.  Every loss is normalised by a count that grows with the
    batch (num_fg, sample counts), so the gradients shrink like 1 / batch: a fixed 4 096 put the head's gradients of a 32-image batch next
    to e5m2's subnormals for the first FP8_AMAX_DELAY steps (tests/test_bench_batch_gpu.py: cls_subnet weight gradient 51 % off the
    batch-2 one).  4 096 was tuned on two images; the default follows the batch in powers of two until the first probe takes over."""
    return m.get("FP8_GRAD_SCALE", 4096.0 * 2.0 ** max(0, int(round(np.log2(max(1, int(m.get("BATCHSIZE", 2))) / 2.0)))))


class Fp8GradScaler:
    """Delayed scaling of the e5m2 gradients (the reference's hook for this is the AMP GradScaler, solver/default_solver.py:66-76): one
    scale for all fp8 data gradients (twins pass from layer to layer, so the layers must agree on it), re-derived every
    FP8_AMAX_INTERVAL steps from max |g| over the gradients those launches consume -- measured by bd_absmax_bf16 on the probe step,
    copied to the host asynchronously and applied FP8_AMAX_DELAY steps later, after that step's data gradients and before its
    weight repack, so that quantisation and the folded 1 / scale of the packed weights always agree.  A static scale underflows
    once training has shrunk the gradients: 4 096 diverged after ~1 500 steps of the repeated-batch run, 65 536 did not."""

    def __init__(self, m, device, convs):
        self.device = torch.device(device)
        self.convs = convs
        self.grad_layers = [c for c in convs.values() if c.fp8_dgrad or c.fp8_1x1_dgrad or c.fp8_wgrad]
        if self.grad_layers:
            for c in convs.values():             # one scale everywhere at the start (a twin's producer reads it off the consumer's layer object)
                c.grad_scale = float(initial_grad_scale(m))
        self.delayed = bool(m.get("FP8_DELAYED_SCALING", True)) and bool(self.grad_layers) and self.device.type == "cuda"
        # Stochastic rounding of those gradients (bd_conv_desc.sr_seed): round-to-nearest e5m2 repeats the same error on the
        # same value every step, which a repeated batch turns into a drift (the long repeated-batch runs)
        self.stochastic_rounding = bool(m.get("FP8_STOCHASTIC_ROUNDING", True)) and bool(self.grad_layers) and self.device.type == "cuda"
        self.amax_interval = int(m.get("FP8_AMAX_INTERVAL", 10))
        self.amax_delay = int(m.get("FP8_AMAX_DELAY", 4))
        self.amax_history = max(1, int(m.get("FP8_AMAX_HISTORY", 4)))         # probes whose maximum sets the scale
        # max |g| * scale lands in (2^(t-1), 2^t]; e5m2 tops out at 1.75 * 2^15 and everything above is CLAMPED.  One global scale: t = 15 (R50:
        # 12 and the static 4 096 diverged in the 2 020-step run, 13 - 15 did not; R101 at batch 32: 14 diverged before step 1 020): only
        # the head sits at the top of the range, every other layer has binades of headroom.  Per-group scales put EVERY group at the top,
        # and a group whose gradients grow between two probes then saturates: R101 batch 32 at t = 15 had layer3 at 92 672 = 1.6 x the
        # maximum at step 100 and left the finite range before step 400, while t = 12 (0.3035 after 1 500 steps) and an eight-probe
        # history at t = 15 (0.3306) both ran through (profiles/r03_fp8_scale_groups.txt).  Round 3 shipped t = 13 with a four-probe
        # history, a combination that had NOT run through (seed 0 diverged on it, same file, section 2): the default is t = 12 with the
        # four-probe history, the combination that did; the round-4 seed matrix is profiles/r04_fp8_stability.txt.
        self.amax_target = float(m.get("FP8_AMAX_TARGET_LOG2", 15.0 if str(m.get("FP8_SCALE_GROUPS", "group")) == "global" else 12.0))
        # Granularity of the delayed scale (round 3).  One scale for all layers had to span the 2^9.7 spread between max |g| at the head and
        # at the backbone's conv1 layers (scripts/exp/fp8_amax_spread.py): with the head's maximum at 2^15 the backbone's gradients sat
        # ten binades lower and their small values flushed to zero -- R101 at the batch-32 learning rate left the finite range.  "group"
        # (default) keeps one scale per backward phase (head / fpn / layer4 / layer3 / layer2: the all-reduce buckets), "layer" one
        # per layer, "global" the round-2 behaviour.  Every twin is written with its CONSUMER's scale (q_scale at each hand-off) and a
        # layer's transposed fp8 weights fold in 1 / its own scale, so any partition is consistent.
        self.scale_groups = str(m.get("FP8_SCALE_GROUPS", "group"))
        assert self.scale_groups in ("global", "group", "layer"), self.scale_groups
        self.t, self._pending, self.history = 0, None, {}
        self.staged = None                       # {conv: scale} waiting for the next weight repack (optimizer step)
        self.scale_log = []
        self.group_scales = {}
        self.last_fill = {}
        if self.delayed:
            n = len(self.grad_layers)
            self.amax_dev = torch.zeros(n, dtype=torch.float32, device=self.device)
            self.amax_host = torch.zeros(n, dtype=torch.float32).pin_memory()
            self.probe_ctl = [False]
            for i, c in enumerate(self.grad_layers):
                c.amax_slot, c.probe_ctl = self.amax_dev[i:i + 1], self.probe_ctl

    def begin_step(self):
        """Start of a backward pass; True when this step probes max |g|."""
        if self.stochastic_rounding:              # this step's e5m2 quantisers: a new hash seed per step (reset at the end of backward)
            ops.fp8_set_stochastic_rounding(((self.t + 1) * 2654435761 + 0x9E3779B9) | 1)
        t = self.t
        self.t += 1
        if self.delayed and self._pending is None and t % self.amax_interval == 0:
            self.amax_dev.zero_()
            self.probe_ctl[0] = True
            return True
        return False

    def scale_key(self, c):
        if self.scale_groups == "global":
            return "all"
        if self.scale_groups == "layer":
            return "fpn_output" if "fpn_output" in c.name else c.name      # the output convolutions all read ONE twin of dL/dP
        n = c.name
        if n.startswith(("head.", "rpn.", "rcnn.")):
            return "head"
        if "fpn_" in n or "top_block" in n:
            return "fpn"
        return n.split(".")[2] if n.startswith("backbone.bottom_up.") else "head"

    def apply_staged(self):
        """New gradient scales take effect HERE, together with the weight repack that folds 1 / scale into the transposed fp8 weights
        (repack_trainable, i.e. the optimizer step): a second backward() without a step keeps quantisers and weights consistent."""
        st, self.staged = self.staged, None
        if st:
            for c, sc in st.items():
                c.grad_scale = sc

    def end_step(self, probing):
        if self.stochastic_rounding:
            ops.fp8_set_stochastic_rounding(0)
        if not self.delayed:
            return
        t = self.t - 1
        if probing:
            self.probe_ctl[0] = False
            from .. import comm as _comm
            cm = _comm.get_comm()
            if cm is not None and cm.world > 1:       # every rank quantises with the same scales: max |g| over the ranks
                cm.allreduce_async(self.amax_dev, [torch.cuda.current_stream()], "max")
                cm.wait()
            self.amax_host.copy_(self.amax_dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending = (ev, t)
        elif self._pending is not None and t >= self._pending[1] + self.amax_delay:
            ev, t0 = self._pending
            ev.synchronize()                      # long done: the host runs a few steps ahead of the device, not FP8_AMAX_DELAY + the queue
            self._pending = None
            self.stage_from_amax(self.amax_host.numpy(), t0, t)

    def stage_from_amax(self, amax, t0, t):
        """Host arithmetic of a finished probe (no device API): amax[i] = max |g| read by grad_layers[i] at step t0 -> maximum per scale
        group -> history -> power-of-two scale, staged for every layer of the group at step t."""
        am = np.asarray(amax).astype(np.float64)
        keys = {}
        for i, c in enumerate(self.grad_layers):
            k = self.scale_key(c)
            if np.isfinite(am[i]):
                keys[k] = max(keys.get(k, 0.0), float(am[i]))
        scales = {}
        # diagnostic: where the probe's largest value sat in e5m2's range under the scale it was quantised with (> 57 344: clamped)
        cur = {self.scale_key(c): c.grad_scale for c in self.grad_layers}
        self.last_fill = {k: a * cur[k] for k, a in keys.items()}
        for k, amax in keys.items():
            if amax > 0.0:
                hist = self.history.setdefault(k, [])          # probe history: a scale never chases a single small reading
                hist.append(amax)
                del hist[:-self.amax_history]
                eff = max(hist)
                scales[k] = float(2.0 ** min(max(np.floor(self.amax_target - np.log2(eff)), -16.0), 40.0))
        if scales:
            staged = {}
            for c in self.convs.values():         # every layer of a group (a twin's producer reads the scale off its CONSUMER's layer object)
                k = self.scale_key(c)
                if k in scales:
                    staged[c] = scales[k]
            self.staged = staged
            self.group_scales.update(scales)
            top = max(keys.values())
            self.scale_log.append((t0, t, top, min(scales.values())))
