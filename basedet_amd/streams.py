"""Fork work onto a side stream and join it again: the one place where a training step makes one stream wait for another."""
from contextlib import contextmanager

import torch


@contextmanager
def fork(stream, wait=True):
    """Run the body on `stream`, behind everything enqueued so far on the current stream (wait=False: behind nothing -- for work that
    only follows what is already on `stream`).  None: the body runs inline on the current stream.  Every fork needs a `join` (or a
    `SideStreams.join_all`) before the current stream reads what the body wrote."""
    if stream is None:
        yield
        return
    if wait:
        stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        yield


def join(stream):
    """The current stream waits for everything enqueued so far on `stream` (None: nothing to wait for)."""
    if stream is not None:
        torch.cuda.current_stream().wait_stream(stream)


class SideStreams:
    """The two side streams of a model; without a GPU there are none.  What each one carries, and where the main stream joins it:

    wgrad -- the weight-gradient stream
      * every weight gradient of a backward pass, one fork per launch, and the deferred reduces (WgradScheduler.run / flush); joined
        once, at the end of the backward pass (WgradScheduler.join)
      * the P6/P7 forward of a LastLevelP6P7 top block, beside the lateral / output convolutions; joined behind the lateral loop
        (FPNDetector.network_forward)
      * Faster R-CNN's early RPN targets, under the backbone's forward pass; joined in front of the RPN losses (get_losses)
    aux -- the auxiliary stream
      * the P6/P7 data gradients; joined in front of the top lateral's data gradient (FPNDetector.backward)
      * RetinaNet's, ATSS's (and, on request, FCOS's) target assignment, under the forward pass; joined in front of the losses
      * RetinaNet's box tower beside the class tower; joined at the end of head_forward
      * Faster R-CNN's proposal chain and RoI sampling, under the RPN losses and the RPN head's backward; joined in front of the box head

    A further stream for any of these was measured and is not worth having: with the box tower on a stream of its own a process
    under torch.distributed had five (main, wgrad, aux, communicator, that one) and the step lost 2.8 ms (577 against 643 img/s with
    one rank and a forced all-reduce: profiles/r06_head_towers_ab.txt; cause not established -- GPU_MAX_HW_QUEUES=8 did not remove it).

    `enabled` (the model's async_wgrad; bench.py and the tests assign it between steps) is read at every call: off, both accessors
    return None and every fork runs inline, e.g. for clean per-kernel timing."""

    def __init__(self, device):
        self.enabled = True
        on_gpu = torch.cuda.is_available() and torch.device(device).type == "cuda"
        self.wgrad_stream = torch.cuda.Stream() if on_gpu else None
        self.aux_stream = torch.cuda.Stream() if on_gpu else None

    def wgrad(self):
        return self.wgrad_stream if self.enabled else None

    def aux(self):
        return self.aux_stream if self.enabled else None

    def join_all(self):
        """The current stream waits for both streams, whatever `enabled` says now: they may hold work from before it was cleared.
        (PlanArena's join: everything that touches plan memory or model scratch off the main stream runs on one of the two.)"""
        join(self.wgrad_stream)
        join(self.aux_stream)
