"""When the weight-gradient kernels of a backward pass run: their forks onto the model's weight-gradient stream (streams.py), and the
deferred-reduce queue with its partial-sum arena."""
import torch

from .. import ops
from ..streams import fork, join


class WgradScheduler:
    def __init__(self, device, queue_mode, streams):
        self.device = torch.device(device)
        # weight-gradient kernels run on a side stream (streams.wgrad()), concurrently with the dgrad chain they do not feed: tails and
        # barrier bubbles of one kernel are filled by the other (streams.enabled = False serialises, e.g. for per-kernel timing)
        self.streams = streams
        # WGRAD_QUEUE: "layer" (default again since round 5) = one fixed-order reduce per layer right behind its partial-sum kernel: the slabs
        # are still in the Infinity Cache when they are read back; "bucket" (round 4's default) = the reduces of a gradient bucket (head /
        # fpn / layer4 / layer3 / layer2) in ONE launch (bd_wgrad_queue_*: 5 reduce launches per step instead of 60); an integer =
        # additionally flush whenever that many bytes of partial sums are pending.  Same bits in every mode (tests/test_wgrad_queue_gpu.py).
        # Measured, alternating on one box (profiles/r05_workloads.txt, r05_queue_ab.txt; round 4 had read the same sign and called it
        # neutral): layer 635.8 / 637.0 / 636.3 img/s, bucket 632.0 / 630.9 / 635.1 -- and 647.4 / 643.7 against 643.2 / 639.5 on two other boxes.
        self.queue_mode = queue_mode
        self.queue = None
        self.need = {}                      # (layer name, full geometry) -> workspace bytes
        # ONE partial-sum arena per model, as large as the largest flush interval (gradient bucket) seen so far: a flush's reduce and
        # every later partial-sum kernel run on the same stream, so the slices are re-used from offset 0 after each flush
        self.arena = None
        self.off = self.pending = self.peak = 0

    def run(self, conv, x, g, gin, gout, ws, cws=None, x8=None, g8=None):
        """conv.wgrad on the side stream: it only needs x and g as they are NOW (everything enqueued so far on the main
        stream), and nothing on the main stream reads its outputs before `join`.  Callers must not overwrite g/x
        later in the same backward pass (the heads keep one gradient buffer per layer for that reason)."""
        q = None
        if self.queue_mode != "layer" and self.device.type == "cuda" and not (conv.fp8_wgrad and x8 is not None and g8 is not None):
            # deferred reduce: this layer's partial sums get their own slice of the model's arena, untouched until the next flush (a
            # gradient bucket's end, or the byte threshold).  A layer that does not fit (the first backward pass of a model, a larger
            # input size, another set of queued layers) runs un-queued on the plan's shared workspace -- same bits -- and the arena is
            # re-grown to the recorded peak at join
            key = (conv.name, gin.N, tuple(gin.H), tuple(gin.W), tuple(gout.H), tuple(gout.W))
            need = self.need.get(key)
            if need is None:
                need = self.need[key] = (conv.wgrad_ws_bytes(gin, gout) + 255) // 256 * 256
            off = self.off
            self.off = off + need
            arena = self.arena
            if arena is not None and off + need <= arena.numel() * 4:
                ws = arena[off // 4: (off + need) // 4]
                self.pending += need
                if self.queue is None:
                    self.queue = ops.WgradQueue()
                q = self.queue
        with fork(self.streams.wgrad()):
            conv.wgrad(x, g, gin, gout, ws, cws, x8=x8, g8=g8, queue=q)
        if q is not None and isinstance(self.queue_mode, int) and self.pending >= self.queue_mode:
            self.flush()

    def begin(self):
        """Start of a backward pass (also the head modules' own, layers/modules.py): the arena is free from offset 0 -- UNLESS partial sums
        are already waiting for the head bucket's flush: Faster R-CNN runs its RPN head's backward inside get_losses, under the proposal
        chain, and those slices must survive until then.  (Rounds 4's reset here let the box head's kernels overwrite them: the RPN
        weight gradients of every queued step were wrong -- found by tests/test_wgrad_queue_gpu.py, the first test of the queued path.)"""
        if self.queue is None or not self.queue.pending():
            self.off = self.pending = 0

    def flush(self):
        """One launch reduces every weight gradient queued since the last flush (on the stream the partial sums were computed on); the
        arena is free again from offset 0 for the kernels enqueued behind that reduce."""
        self.peak = max(self.peak, self.off)
        self.off = self.pending = 0
        q = self.queue
        if q is None or not q.pending():
            return
        with fork(self.streams.wgrad(), wait=False):         # (behind the partial sums already there: no main -> side dependency per flush)
            q.flush()

    def join(self):
        self.flush()
        join(self.streams.wgrad())
        have = 0 if self.arena is None else self.arena.numel() * 4
        if self.queue_mode != "layer" and self.peak > have:
            # (behind the join: the old arena's last readers have been ordered in front of the current stream, which owns both allocations)
            self.arena = None
            self.arena = torch.empty((self.peak // 4 + 64,), dtype=torch.float32, device=self.device)
