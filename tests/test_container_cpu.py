"""layers/_pm.py Container and models/adopted.py AdoptedParts on stub leaves: plain objects that implement the layer protocol on CPU
tensors.  What the GPU tests of the real layers assert of one family each -- names in the reference's order, strict loads that change
nothing when they raise, an adopt() that moves nothing when it refuses -- is asserted here of the container itself."""
import numpy as np
import pytest
import torch

from basedet_amd.layers._pm import Container, ParamStore, load_strict
from basedet_amd.models.adopted import AdoptedParts

CPU = torch.device("cpu")


class Leaf:
    """A layer with one master `weight` (n,), a state entry per norm it declares, and a record of what adopt() handed it."""

    def __init__(self, n, norms=(), fill=1.0):
        self.NORMS, self.device, self.training = tuple(norms), CPU, True
        self._store = ParamStore({"weight": (n,)}, CPU)
        self._store.w["weight"].fill_(fill)
        self.stats = {r: torch.zeros(n) for r in norms}
        self.got, self.repacks, self.refreshed = None, 0, 0

    def _shapes(self):
        return {"weight": self._store.shapes["weight"], **{f"{r}.running_mean": tuple(v.shape) for r, v in self.stats.items()}}

    def names(self):
        return list(self._shapes())

    def params(self):
        return dict(self._store.w)

    def grads(self):
        return {k: v.clone() for k, v in self._store.g.items()}

    def state_dict(self):
        return {"weight": self._store.w["weight"].clone(), **{f"{r}.running_mean": v.clone() for r, v in self.stats.items()}}

    def load_state_dict(self, state):
        p = load_strict(state, self._shapes(), CPU)
        self._store.w["weight"].copy_(p["weight"])
        for r, v in self.stats.items():
            v.copy_(p[f"{r}.running_mean"])
        self.repack()

    def repack(self):
        self.repacks += 1

    def arena_shapes(self):
        return dict(self._store.shapes)

    def adopt(self, w, g, *records):
        self._store.move(w, g)
        self.got = records

    def refresh_eval(self):
        self.refreshed += 1

    def train(self, mode=True):
        self.training = bool(mode)
        return self


class Pair(Container):
    def __init__(self, a, b):
        self.a, self.b, self.device = a, b, CPU

    def _children(self):
        return [("first", self.a), ("second", self.b)]


class Tree(Container):
    """second-before-first on purpose: the order is _children()'s, not the alphabet's or the constructor's."""

    def __init__(self):
        self.device = CPU
        self.plain, self.one, self.two = Leaf(2), Leaf(3, ("norm",)), Leaf(4, ("dcn_bn", "up_bn"))
        self.pair = Pair(self.one, self.two)

    def _children(self):
        return [("z", self.pair), ("a.0", self.plain)]


def _leaves(t):
    return [t.one, t.two, t.plain]


def _storage(shapes):
    mk = lambda: {k: torch.full(s, float("nan")) for k, s in shapes.items()}
    return mk(), mk()


def _records(t):
    return {"z.first.norm": object(), "z.second.dcn_bn": object(), "z.second.up_bn": object()}


def test_nested_names_come_out_in_children_order():
    t = Tree()
    want = ["z.first.weight", "z.first.norm.running_mean", "z.second.weight", "z.second.dcn_bn.running_mean",
            "z.second.up_bn.running_mean", "a.0.weight"]
    assert t.names() == want == list(t.state_dict())
    assert [n for n, _ in t._leaves()] == ["z.first", "z.second", "a.0"] and [c for _, c in t._leaves()] == _leaves(t)
    assert list(t.params()) == list(t.arena_shapes()) == ["z.first.weight", "z.second.weight", "a.0.weight"]
    assert t.arena_shapes() == {"z.first.weight": (3,), "z.second.weight": (4,), "a.0.weight": (2,)}
    assert t.params()["z.second.weight"].data_ptr() == t.two._store.w["weight"].data_ptr()
    t.eval()
    assert not t.training and not t.pair.training and not any(c.training for c in _leaves(t))
    t.refresh_eval()
    t.repack()
    assert [c.refreshed for c in _leaves(t)] == [1, 1, 1] and [c.repacks for c in _leaves(t)] == [1, 1, 1]


def test_load_state_dict_is_strict_and_atomic():
    t = Tree()
    good = {k: v + 1 for k, v in t.state_dict().items()}
    before = {k: v.clone() for k, v in t.state_dict().items()}
    missing = {k: v for k, v in good.items() if k != "a.0.weight"}                 # the LAST leaf's: the earlier ones must not have loaded
    for bad, err in ((dict(good, extra=torch.zeros(1)), KeyError), (missing, KeyError),
                     (dict(good, **{"a.0.weight": torch.zeros(3)}), ValueError)):
        with pytest.raises(err):
            t.load_state_dict(bad)
        after = t.state_dict()
        assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
        assert [c.repacks for c in _leaves(t)] == [0, 0, 0]
    ptrs = {k: v.data_ptr() for k, v in t.params().items()}
    t.load_state_dict({k: v.numpy() for k, v in good.items()})
    after = t.state_dict()
    assert all(torch.equal(after[k], good[k]) for k in good) and {k: v.data_ptr() for k, v in t.params().items()} == ptrs
    assert [c.repacks for c in _leaves(t)] == [1, 1, 1]


def test_refused_adopt_moves_no_leaf():
    t = Tree()
    ptrs = {k: v.data_ptr() for k, v in t.params().items()}
    w, g = _storage(t.arena_shapes())
    g["a.0.weight"] = g["a.0.weight"][:-1]                                          # one wrong shape, in the last leaf
    with pytest.raises(ValueError, match="adopt"):
        t.adopt(w, g, _records(t))
    assert {k: v.data_ptr() for k, v in t.params().items()} == ptrs
    assert all(c._store.g is None and c.got is None for c in _leaves(t))
    assert all(bool(torch.isnan(v).all()) for v in w.values())
    w, g = _storage(t.arena_shapes())
    with pytest.raises(KeyError):                                                   # a norm record missing: nothing moves either
        t.adopt(w, g, {k: v for k, v in _records(t).items() if k != "z.second.up_bn"})
    assert {k: v.data_ptr() for k, v in t.params().items()} == ptrs and all(c._store.g is None for c in _leaves(t))


def test_adopt_hands_each_leaf_the_norm_records_it_declares():
    t = Tree()
    w, g = _storage(t.arena_shapes())
    recs = _records(t)
    t.adopt(w, g, recs)
    assert t.plain.got == () and t.one.got == (recs["z.first.norm"],) and t.two.got == (recs["z.second.dcn_bn"], recs["z.second.up_bn"])
    for k, v in t.params().items():
        assert v.data_ptr() == w[k].data_ptr() and bool((v == 1).all())            # the values moved in
    assert t.two._store.g["weight"].data_ptr() == g["z.second.weight"].data_ptr()


class Arena:
    """models/engine.py ParamArena's reserve / view on CPU tensors."""

    def __init__(self):
        self.entries, self.t = [], {}

    def reserve(self, name, shape):
        self.entries.append((name, tuple(shape)))
        return len(self.entries) - 1

    def view(self, which, i):
        name, shape = self.entries[i]
        return self.t.setdefault((which, name), torch.zeros(shape))


class Record:
    bound = None

    def bind_views(self, arena):
        self.bound = arena


def test_adopted_parts_bind_skips_absent_prefixes_and_loads_the_others():
    neck, head = Pair(Leaf(3, ("norm",)), Leaf(4)), Leaf(2)
    parts = AdoptedParts([("upsample", neck), ("head", head)], CPU)
    assert parts.names() == ["upsample.first.weight", "upsample.first.norm.running_mean", "upsample.second.weight", "head.weight"]
    assert parts.grad_names() == ["upsample.first.weight", "upsample.second.weight", "head.weight"]
    state = parts.state_dict()
    assert all(isinstance(v, np.ndarray) for v in state.values()) and list(state) == parts.names()
    # a backbone-only checkpoint: nothing of either part, nothing loads; then the head alone
    parts.bind({"backbone.conv1.weight": np.zeros(3)})
    assert head.repacks == 0 and neck.a.repacks == 0
    parts.bind({"backbone.conv1.weight": np.zeros(3), "head.weight": np.full(2, 7.0, np.float32)})
    assert head.repacks == 1 and neck.a.repacks == 0 and neck.b.repacks == 0
    assert bool((head._store.w["weight"] == 7).all()) and bool((neck.a._store.w["weight"] == 1).all())
    with pytest.raises(KeyError):                                                   # a part the dict has entries of is loaded strictly
        parts.bind({"upsample.first.weight": np.zeros(3, np.float32)})
    assert bool((neck.a._store.w["weight"] == 1).all())
    # the arena's order is the caller's
    arena, rec = Arena(), Record()
    parts.reserve(arena, ["head.weight"])
    parts.reserve(arena, ["upsample.second.weight", "upsample.first.weight"])
    assert [e[0] for e in arena.entries] == ["head.weight", "upsample.second.weight", "upsample.first.weight"]
    parts.adopt_onto(arena, {"upsample.first.norm": rec})
    assert rec.bound is arena and neck.a.got == (rec,) and head.got == ()
    assert head._store.w["weight"].data_ptr() == arena.t[("w", "head.weight")].data_ptr()
    assert neck.b._store.g["weight"].data_ptr() == arena.t[("g", "upsample.second.weight")].data_ptr()
    assert bool((arena.t[("w", "head.weight")] == 7).all())
