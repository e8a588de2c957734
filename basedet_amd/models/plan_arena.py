"""The plan arena: byte layout of a shape plan's per-step buffers (_Carver) and the one grow-only device buffer per model that every
plan's buffers are views into (PlanArena).  Pure layout and view re-basing -- no kernel, no stream: the owner passes the `join` that
orders its side streams in front of the current one."""
import torch


def _round_up(v, m):
    return (v + m - 1) // m * m


class _Plan:
    """Shape-dependent state for one (N, Hp, Wp).  Per-shape constants (geometry, level tables, anchors / points, routing decisions) are
    the plan's own; every per-step buffer (activations, gradients, twins, targets, counters, workspaces) is a view into the model's plan
    arena, laid out by a _Carver at fixed offsets from 0 -- the views of different shapes alias the same memory."""


class _Carver:
    """Byte layout of one plan's per-step buffers in the plan arena.  While FPNDetector._plan runs they are meta placeholders (nothing is
    allocated); PlanArena.place swaps them for arena views once the arena is large enough."""

    ALIGN = 256
    BIG_ALIGN = 2 << 20

    def __init__(self):
        self.nbytes = 0
        self.slots = {}          # id(placeholder) -> (byte offset, placeholder)
        self.zero = []           # (byte offset, bytes): buffers whose all-zero start state is re-established whenever the plan is bound

    def empty(self, shape, dtype, zero=False):
        t = torch.empty(shape, dtype=dtype, device="meta")
        n = t.numel() * t.element_size()
        # buffers of 1 MiB and more start on a 2 MiB boundary, as the caching allocator's large blocks mostly did (packed at 256 B the
        # fixed-shape step measured ~0.9 % slower)
        off = _round_up(self.nbytes, self.BIG_ALIGN if n >= (1 << 20) else self.ALIGN)
        self.nbytes = off + _round_up(n, self.ALIGN)
        self.slots[id(t)] = (off, t)
        if zero and n:
            self.zero.append((off, n))
        return t

    def zeros(self, shape, dtype):
        return self.empty(shape, dtype, zero=True)

    def like(self, t):
        return self.empty(tuple(t.shape), t.dtype)


def _map_tensors(v, fn):
    """Replace every tensor t held by v (a plan: attributes, nested plans, lists, tuples, dicts) by fn(t).  (A plain recursive function:
    a self-referencing closure would be a reference cycle that keeps fn -- and the arena it names -- alive until the next gc pass.)"""
    if torch.is_tensor(v):
        return fn(v)
    if isinstance(v, _Plan):
        d = v.__dict__
        for k in list(d):
            d[k] = _map_tensors(d[k], fn)
    elif isinstance(v, list):
        v[:] = [_map_tensors(x, fn) for x in v]
    elif isinstance(v, tuple):
        return tuple(_map_tensors(x, fn) for x in v)
    elif isinstance(v, dict):
        for k in list(v):
            v[k] = _map_tensors(v[k], fn)
    return v


class PlanArena:
    """ONE plan arena per model (uint8): every plan's per-step buffers are carved from offset 0, so device memory for them is what the
    largest shape seen needs, whatever the number of shapes (multi-scale training).  Only one step runs at a time; `bound` is the plan
    whose state the arena holds now (bind re-establishes a plan's start state when another one used the memory in between)."""

    def __init__(self, device, join):
        self.device = torch.device(device)
        self._join = join                 # the current stream waits for every side stream that touches plan memory or scratch
        self.buf = None
        self.bound = None
        self.grows = 0
        self.epoch = 0                    # counts the events after which a plan's buffers may hold other bytes than its own last step's
        self.plans = []                   # every placed plan: re-based when the arena grows
        self._scratch = {}                # model-level grow-only workspaces whose size follows the batch (Gmax), not the shape

    @property
    def nbytes(self):
        """Bytes of the arena (what the largest plan seen so far needs, rounded up to 2 MiB)."""
        return 0 if self.buf is None else self.buf.numel()

    def place(self, pl):
        """Swap the carved placeholders of a new plan for views into the arena (grown first if the plan needs more bytes)."""
        c = pl._carve
        self.grow(c.nbytes)
        buf = self.buf

        def place(t):
            if not t.is_meta:
                return t
            off, ph = c.slots[id(t)]
            assert ph is t, "a meta tensor that the carver did not lay out"
            return buf[off: off + t.numel() * t.element_size()].view(t.dtype).view(t.shape)

        _map_tensors(pl, place)
        c.slots = None
        self.plans.append(pl)

    def grow(self, nbytes):
        """Replace the arena by a larger one.  The old storage is freed only once no stream can still touch it (device synchronisation:
        growth happens a few times per run at most); its contents move along, so the last step's buffers stay readable, and every placed
        plan's views are re-based onto the new storage at the same offsets."""
        have = self.nbytes
        if nbytes <= have:
            return
        nbytes = _round_up(nbytes, 2 << 20)
        old = self.buf
        if old is not None and self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        new = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        if old is not None:
            new[:have].copy_(old)
            base = old.data_ptr()

            def rebase(t):
                if t.device != new.device or t.untyped_storage().data_ptr() != base:
                    return t
                off = t.data_ptr() - base
                return new[off: off + t.numel() * t.element_size()].view(t.dtype).view(t.shape)

            for p in self.plans:
                _map_tensors(p, rebase)
        self.buf = new
        self.grows += 1
        self.epoch += 1

    def bind(self, pl):
        """Start of a step at plan pl.  When another plan used the arena since pl's last step, every buffer of pl's can hold that plan's
        data: the main stream first waits for every stream that touched plan memory (the weight-gradient stream, the auxiliary stream;
        the communicator only reads the parameter arena and the FCOS statistics, behind a wait of its own), then the buffers whose start
        state is all-zero (counters, loss sums, d_rpn_raw's padding channel) are cleared -- as torch.zeros did once per plan."""
        if self.bound is pl:
            return
        if self.bound is not None:
            self._join()
        buf = self.buf
        for off, n in pl._carve.zero:
            buf[off: off + n].zero_()
        self.bound = pl
        self.epoch += 1

    def scratch(self, name, nbytes):
        """Model-level grow-only uint8 workspace (its size follows the batch -- Gmax -- rather than the shape).  Before a smaller one is
        freed the current stream waits for the side streams, so that no later allocation on it can overlap a reader still running."""
        nbytes = max(int(nbytes), 1)
        t = self._scratch.get(name)
        if t is None or t.numel() < nbytes:
            if t is not None:
                self._join()
            t = self._scratch[name] = torch.empty((_round_up(nbytes, 256),), dtype=torch.uint8, device=self.device)
        return t[:nbytes]
