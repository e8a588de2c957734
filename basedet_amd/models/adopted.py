"""The layers of a model that live on its parameter arena through their adopt() (layers/_pm.py): CenterNet's neck and head, YOLOX's
PAFPN and head."""
from ..layers._pm import Container, cut


class AdoptedParts(Container):
    """[(name, layer)]: the layers under their state_dict names (`name.` is the prefix of the layer's entries).  A Container of them,
    so names(), params(), repack(), refresh_eval() and train() are the layers' own; what a model adds is below.  It is the model's end of
    the protocol, not a layer: state_dict() and grads() return what a model exports (numpy arrays, host tensors), and the way onto the
    arena is reserve() ... adopt_onto(), not the inherited adopt(w, g, norms), which adopt_onto() calls with the arena's views.  The
    order of the arena's entries is the caller's: reserve() takes the names in the order it is given them."""

    def __init__(self, parts, device):
        self.parts, self.device = list(parts), device
        self.slots = {}

    def _children(self):
        return self.parts

    def bind(self, params):
        """(Re)load from a reference-layout dict: each part that the dict has entries of goes in through its layer's strict
        load_state_dict, which copies in place (the arena views stay where they are) and repacks."""
        for n, layer in self.parts:
            own = cut(params, n)
            if own:
                layer.load_state_dict(own)

    def state_dict(self):
        return {k: v.numpy() for k, v in super().state_dict().items()}

    def grads(self):
        return {k: v.detach().cpu() for k, v in super().grads().items()}

    def grad_names(self):
        return [k for k in self.names() if "running_" not in k]

    def reserve(self, arena, names):
        """An arena entry for each of `names` (of arena_shapes()), in that order."""
        shapes = self.arena_shapes()
        for k in names:
            self.slots[k] = arena.reserve(k, shapes[k])

    def adopt_onto(self, arena, norms):
        """After arena.allocate(): norms = {"<leaf>.<norm>": BatchNormState, reserved in the arena}; the records take their arena views
        and every layer moves onto the entries reserve() made."""
        missing = [k for k in self.arena_shapes() if k not in self.slots]
        if missing:
            raise KeyError(f"adopt_onto: no arena entry was reserved for {missing}")
        for r in norms.values():
            r.bind_views(arena)
        super().adopt(*({k: arena.view(which, i) for k, i in self.slots.items()} for which in ("w", "g")), norms)
