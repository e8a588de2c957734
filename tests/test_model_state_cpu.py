"""The three state machines FPNDetector delegates to, on CPU tensors and without the native library: the plan arena's byte layout and
view re-basing (models/plan_arena.py), the host arithmetic of the delayed e5m2 gradient scales (models/fp8_scaling.py) and the
weight-gradient scheduler's bookkeeping (models/wgrad_sched.py) -- and what its stream helpers (streams.py) do when there is no stream.
Every expected value is written out by hand from the rules."""
import threading

import numpy as np
import pytest
import torch

from basedet_amd.models.fp8_scaling import Fp8GradScaler, initial_grad_scale
from basedet_amd.models.plan_arena import PlanArena, _Carver, _Plan
from basedet_amd.models.wgrad_sched import WgradScheduler
from basedet_amd.streams import SideStreams, fork, join

MiB = 1 << 20


def _nbytes(t):
    return t.numel() * t.element_size()


def _plan_a():
    """256 B slots: a 0, lst[0] 256, d['k'] 512, child.t 768 (600 B -> three slots, end 1 536); the 1 MiB buffer on the next 2 MiB
    boundary, the tail right behind it at 3 MiB; 3 MiB + 256 B in all."""
    pl, child = _Plan(), _Plan()
    C = pl._carve = _Carver()
    pl.a = C.empty((100,), torch.uint8)
    pl.lst = [C.empty((3, 5), torch.float32)]
    pl.d = {"k": C.zeros((7,), torch.int32)}
    child.t = C.empty((300,), torch.bfloat16)
    pl.child = child
    pl.big = C.empty((MiB,), torch.uint8)
    pl.tail = C.like(pl.a)
    pl.const = torch.arange(4)                  # a per-shape constant: not the arena's
    pl.n = 3
    return pl


def _tensors(pl):
    return {"a": pl.a, "lst": pl.lst[0], "k": pl.d["k"], "t": pl.child.t, "big": pl.big, "tail": pl.tail}


def _single(nbytes):
    pl = _Plan()
    pl._carve = _Carver()
    pl.x = pl._carve.empty((nbytes,), torch.uint8)
    return pl


def test_carver_layout_and_arena_growth_rebinding_and_scratch():
    joins = []
    arena = PlanArena("cpu", lambda: joins.append(1))
    assert arena.nbytes == 0 and arena.grows == 0
    A = _plan_a()
    assert A._carve.nbytes == 3 * MiB + 256 and A._carve.zero == [(512, 28)]
    assert all(t.is_meta for t in _tensors(A).values())
    const = A.const
    arena.place(A)
    assert arena.grows == 1 and arena.nbytes == 4 * MiB                          # 3 MiB + 256 B rounded up to 2 MiB
    want = {"a": 0, "lst": 256, "k": 512, "t": 768, "big": 2 * MiB, "tail": 3 * MiB}
    shapes = {"a": (100,), "lst": (3, 5), "k": (7,), "t": (300,), "big": (MiB,), "tail": (100,)}

    def offsets(pl):
        base = arena.buf.data_ptr()
        ts = _tensors(pl)
        assert not any(t.is_meta for t in ts.values())
        assert all(t.untyped_storage().data_ptr() == base for t in ts.values())
        assert {k: tuple(t.shape) for k, t in ts.items()} == shapes
        return {k: t.data_ptr() - base for k, t in ts.items()}

    assert offsets(A) == want
    assert all(o % 256 == 0 for o in want.values()) and want["big"] % (2 * MiB) == 0
    spans = sorted((o, o + _nbytes(_tensors(A)[k])) for k, o in want.items())
    assert all(e0 <= s1 for (_, e0), (s1, _) in zip(spans, spans[1:]))           # no two slots overlap
    assert A.const is const and A.n == 3                                         # what is not a carved placeholder stays as it is

    # contents move along when a larger plan arrives; the first plan keeps its offsets in the new storage
    for i, t in enumerate(_tensors(A).values()):
        t.view(-1).view(torch.uint8).copy_((torch.arange(_nbytes(t)) * (i + 3) % 251).to(torch.uint8))
    saved = {k: t.clone() for k, t in _tensors(A).items()}
    old_ptr = arena.buf.data_ptr()
    B = _single(5 * MiB)
    arena.place(B)
    assert arena.grows == 2 and arena.nbytes == 6 * MiB and arena.buf.data_ptr() != old_ptr
    assert offsets(A) == want and A.const is const
    assert all(torch.equal(t, saved[k]) for k, t in _tensors(A).items())
    assert B.x.data_ptr() == arena.buf.data_ptr() and not B.x.is_meta           # every plan is carved from offset 0
    Csmall = _single(1000)
    arena.place(Csmall)
    assert arena.grows == 2 and arena.nbytes == 6 * MiB                          # a plan that fits grows nothing
    assert arena.plans == [A, B, Csmall] and not joins

    # zero-start buffers are re-cleared only when another plan was bound in between
    arena.bind(A)
    assert not joins and int(A.d["k"].abs().sum()) == 0
    assert torch.equal(A.a, saved["a"]) and torch.equal(A.child.t, saved["t"])   # only the zero range is touched
    A.d["k"].fill_(7)
    arena.bind(A)
    assert not joins and A.d["k"].tolist() == [7] * 7                            # bound twice in a row: left alone
    arena.bind(B)
    assert len(joins) == 1 and A.d["k"].tolist() == [7] * 7                      # (B has no zero range)
    arena.bind(A)
    assert len(joins) == 2 and A.d["k"].tolist() == [0] * 7 and arena.bound is A

    # scratch: a view of the requested size; the storage is kept when less is asked for, replaced behind one join when more is
    s = arena.scratch("x", 100)
    assert s.dtype == torch.uint8 and s.numel() == 100 and s.untyped_storage().nbytes() == 256 and len(joins) == 2
    p = s.data_ptr()
    s2 = arena.scratch("x", 50)
    assert s2.numel() == 50 and s2.data_ptr() == p and len(joins) == 2
    s3 = arena.scratch("x", 300)
    assert s3.numel() == 300 and s3.untyped_storage().nbytes() == 512 and len(joins) == 3
    assert arena.scratch("y", 0).numel() == 1 and len(joins) == 3                # a new name joins nothing
    assert arena.scratch("x", 300).data_ptr() == s3.data_ptr()


class _Layer:
    def __init__(self, name, grad=True):
        self.name = name
        self.fp8_dgrad, self.fp8_1x1_dgrad, self.fp8_wgrad = grad, False, False
        self.grad_scale = 1.0


_NAMES = ["head.cls_subnet.0", "backbone.fpn_output3", "backbone.top_block.p6", "backbone.bottom_up.layer3.0.conv2", "rpn.rpn_conv"]
_PLAIN = ["backbone.bottom_up.layer3.0.conv1", "backbone.fpn_lateral3"]          # no fp8 gradient of their own, but members of a group


def _scaler(**cfg):
    convs = {n: _Layer(n) for n in _NAMES}
    convs.update({n: _Layer(n, grad=False) for n in _PLAIN})
    s = Fp8GradScaler(dict(cfg), "cpu", convs)
    assert [c.name for c in s.grad_layers] == _NAMES
    return s, convs


def test_fp8_scale_keys_for_the_three_granularities():
    want = {
        "global": ["all"] * 7,
        "group": ["head", "fpn", "fpn", "layer3", "head", "layer3", "fpn"],
        "layer": ["head.cls_subnet.0", "fpn_output", "backbone.top_block.p6", "backbone.bottom_up.layer3.0.conv2", "rpn.rpn_conv",
                  "backbone.bottom_up.layer3.0.conv1", "backbone.fpn_lateral3"],
    }
    for mode, keys in want.items():
        s, convs = _scaler(FP8_SCALE_GROUPS=mode)
        assert [s.scale_key(convs[n]) for n in _NAMES + _PLAIN] == keys, mode
        assert s.amax_target == (15.0 if mode == "global" else 12.0)
        assert not s.delayed and not s.stochastic_rounding                       # no device: nothing to probe
    s, _ = _scaler()                                                             # the default: "group"
    assert s.scale_key(_Layer("rcnn.fc1")) == "head" and s.scale_key(_Layer("backbone.bottom_up.layer2.3.conv3")) == "layer2"


def test_fp8_initial_scale_follows_the_batch():
    assert initial_grad_scale({}) == 4096.0 and initial_grad_scale({"BATCHSIZE": 2}) == 4096.0
    assert initial_grad_scale({"BATCHSIZE": 16}) == 32768.0 and initial_grad_scale({"BATCHSIZE": 32}) == 65536.0
    assert initial_grad_scale({"BATCHSIZE": 32, "FP8_GRAD_SCALE": 512.0}) == 512.0
    s, convs = _scaler(BATCHSIZE=32)
    assert all(c.grad_scale == 65536.0 for c in convs.values())                  # every layer, the plain ones included
    assert (s.amax_interval, s.amax_delay, s.amax_history, s.scale_groups) == (10, 4, 4, "group")


def test_fp8_scales_from_amax_history_and_staging():
    s, convs = _scaler(FP8_GRAD_SCALE=4096.0, FP8_AMAX_HISTORY=2)
    head = ["head.cls_subnet.0", "rpn.rpn_conv"]
    fpn = ["backbone.fpn_output3", "backbone.top_block.p6", "backbone.fpn_lateral3"]
    l3 = ["backbone.bottom_up.layer3.0.conv2", "backbone.bottom_up.layer3.0.conv1"]
    # probe 1.  head: max(3, 1) = 3 -> floor(12 - 1.58) = 10; fpn: max(0.5, 0.75) -> floor(12 + 0.41) = 12; layer3: 2^-10 -> 22
    s.stage_from_amax(np.array([3.0, 0.5, 0.75, 2.0 ** -10, 1.0], np.float32), 0, 4)
    assert s.group_scales == {"head": 1024.0, "fpn": 4096.0, "layer3": 2.0 ** 22}
    assert s.last_fill == {"head": 3.0 * 4096, "fpn": 0.75 * 4096, "layer3": 4.0}
    assert s.scale_log == [(0, 4, 3.0, 1024.0)]
    assert {c.name: v for c, v in s.staged.items()} == {**{n: 1024.0 for n in head}, **{n: 4096.0 for n in fpn}, **{n: 2.0 ** 22 for n in l3}}
    assert all(c.grad_scale == 4096.0 for c in convs.values())                   # staged, not applied
    s.apply_staged()
    assert s.staged is None
    assert {n: c.grad_scale for n, c in convs.items()} == {**{n: 1024.0 for n in head}, **{n: 4096.0 for n in fpn}, **{n: 2.0 ** 22 for n in l3}}
    s.apply_staged()                                                             # nothing staged: nothing changes
    assert convs["rpn.rpn_conv"].grad_scale == 1024.0
    # probe 2.  head reads less (0.5): the 3.0 is still in the two-probe window, the scale stays; fpn read inf / nan and layer3 zero:
    # skipped, no scale staged for them and their history untouched
    s.stage_from_amax(np.array([0.5, np.inf, np.nan, 0.0, 0.25], np.float32), 10, 14)
    assert {c.name: v for c, v in s.staged.items()} == {n: 1024.0 for n in head}
    assert s.group_scales == {"head": 1024.0, "fpn": 4096.0, "layer3": 2.0 ** 22}
    assert s.last_fill == {"head": 0.5 * 1024, "layer3": 0.0}
    assert s.history == {"head": [3.0, 0.5], "fpn": [0.75], "layer3": [2.0 ** -10]}
    assert s.scale_log[-1] == (10, 14, 0.5, 1024.0)
    s.apply_staged()
    # probe 3.  the 3.0 has left the window: max(0.5, 0.5) -> floor(12 + 1) = 13
    s.stage_from_amax(np.array([0.5, 0.0, 0.0, 0.0, 0.0], np.float32), 20, 24)
    assert s.history["head"] == [0.5, 0.5] and s.group_scales["head"] == 8192.0
    assert convs["head.cls_subnet.0"].grad_scale == 1024.0
    s.apply_staged()
    assert convs["head.cls_subnet.0"].grad_scale == 8192.0 and convs["rpn.rpn_conv"].grad_scale == 8192.0
    assert convs["backbone.fpn_output3"].grad_scale == 4096.0
    # a probe without a usable reading stages nothing and logs nothing
    n = len(s.scale_log)
    s.stage_from_amax(np.array([0.0, np.nan, 0.0, np.inf, 0.0], np.float32), 30, 34)
    assert s.staged is None and len(s.scale_log) == n


def test_fp8_scale_clamps_and_global_group():
    s, convs = _scaler(FP8_GRAD_SCALE=4096.0, FP8_SCALE_GROUPS="layer", FP8_AMAX_HISTORY=1)
    # 12 + 40 = 52 -> clamped to 40; 12 - 30 = -18 -> clamped to -16; exactly 2^12 -> 2^0; just above 2^12 -> 2^-1
    s.stage_from_amax(np.array([2.0 ** -40, 2.0 ** 30, 4096.0, 4097.0, 0.0], np.float64), 0, 1)
    assert s.group_scales == {"head.cls_subnet.0": 2.0 ** 40, "fpn_output": 2.0 ** -16, "backbone.top_block.p6": 1.0,
                              "backbone.bottom_up.layer3.0.conv2": 0.5}
    assert {c.name for c in s.staged} == set(_NAMES[:4])                         # "layer": the plain layers belong to no probed key
    g, gconvs = _scaler(FP8_GRAD_SCALE=4096.0, FP8_SCALE_GROUPS="global")
    g.stage_from_amax(np.array([3.0, 0.5, 0.75, 2.0 ** -10, 1.0], np.float32), 0, 4)       # floor(15 - 1.58) = 13
    assert g.group_scales == {"all": 8192.0} and {c.name: v for c, v in g.staged.items()} == {n: 8192.0 for n in _NAMES + _PLAIN}
    assert g.last_fill == {"all": 3.0 * 4096}


class _Conv:
    name, fp8_wgrad = "head.cls_subnet.0", False

    def __init__(self):
        self.calls = []

    def wgrad_ws_bytes(self, gin, gout):
        raise AssertionError("'layer' mode never sizes a slice of the partial-sum arena")

    def wgrad(self, *a, **kw):
        self.calls.append((a, kw))


def test_wgrad_scheduler_layer_mode_hands_out_the_shared_workspace():
    """Only the "layer" mode is checked here: the queued modes need ops.WgradQueue, i.e. the native library and a GPU
    (tests/test_wgrad_queue_gpu.py)."""
    st = SideStreams("cpu")
    s = WgradScheduler("cpu", "layer", st)
    assert st.enabled and st.wgrad() is None and st.aux() is None                # no GPU: no side streams, whatever the flag says
    conv = _Conv()
    x, g, gin, gout, ws, cws, x8 = (object() for _ in range(7))
    s.begin()
    s.run(conv, x, g, gin, gout, ws, cws)
    s.run(conv, x, g, gin, gout, ws, x8=x8)
    s.flush()
    s.run(conv, g, x, gout, gin, ws, cws)
    s.join()
    st.join_all()
    assert conv.calls == [((x, g, gin, gout, ws, cws), dict(x8=None, g8=None, queue=None)),
                          ((x, g, gin, gout, ws, None), dict(x8=x8, g8=None, queue=None)),
                          ((g, x, gout, gin, ws, cws), dict(x8=None, g8=None, queue=None))]
    assert s.queue is None and s.arena is None and s.need == {} and (s.off, s.pending, s.peak) == (0, 0, 0)
    st.enabled = False
    assert st.wgrad() is None and st.aux() is None


def test_fork_and_join_without_a_stream_run_inline():
    ran = []
    with fork(None):
        ran.append(threading.get_ident())
    with fork(None, wait=False):
        ran.append(threading.get_ident())
    assert ran == [threading.get_ident()] * 2                  # each body once, on the calling thread
    with pytest.raises(KeyError, match="from the body"):
        with fork(None):
            raise KeyError("from the body")
    assert join(None) is None
    st = SideStreams("cpu")
    for flag in (True, False):
        st.enabled = flag
        assert st.wgrad() is None and st.aux() is None and st.wgrad_stream is None and st.aux_stream is None
        st.join_all()
