"""Liveness maps (bd_conv_desc.gskip_gmap / gskip_dxmap / gskip_dx_clean, MODEL.SPARSE_BOX_CHAIN): a chain of hinted data gradients that
hands its liveness down in maps -- no scan of the 256-channel gradients, no compaction launch, no full zero fill at a fixed shape -- must
give the SAME BITS as the same calls with the hint off (gskip = 0: the dense route is the oracle, there is no tolerance).

Kernel level on a small pyramid, 2 images x levels (24, 40), (12, 20), (6, 10), (3, 5), (2, 3), 256 -> 256: every level ends in a ragged
4 x 16 AND a ragged 8 x 8 patch, the two coarsest levels are smaller than one patch, and level / image boundaries are adjacent in memory.
Step level: RetinaNet-R50 at 2 x 800 x 1344 over two consecutive steps (the second one runs with the promise)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LEVELS = [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)]
N, C = 2, 256
NAN16 = 0x7FC1
NEG0 = -0x8000          # bf16 -0.0 as int16


def _last_kernel():
    from basedet_amd import _lib
    return _lib.load().bd_conv_last_kernel().decode()


class _Ctx:
    """Operands shared by every test of this module (made once, never modified)."""

    def __init__(self):
        from basedet_amd import ops
        self.ops = ops
        self.geo = ops.Geom(N, [h for h, _ in LEVELS], [w for _, w in LEVELS])
        self.P = N * self.geo.pix_per_img
        self.d = ops.conv_desc(self.geo, self.geo, C, C, 3, 3, 1, 1)
        gen = torch.Generator(device="cuda").manual_seed(11)
        rn = lambda *s: torch.randn(s, device="cuda", generator=gen)      # noqa: E731
        self.w = [(rn(C, 9, C) * 0.05).to(torch.bfloat16) for _ in range(4)]
        self.act = [rn(self.P, C).to(torch.bfloat16) for _ in range(4)]             # ReLU gates (> 0 keeps) = the layers' inputs
        self.vals = rn(self.P, C).to(torch.bfloat16)
        self.vals = torch.where(self.vals == 0, torch.ones_like(self.vals), self.vals)
        self.scratch = torch.empty((ops.conv2d_dgrad_gskip_bytes(self.d) + 3) // 4, dtype=torch.int32, device="cuda")
        self.map_ints = (ops.conv2d_gskip_map_bytes(self.d) + 3) // 4
        assert self.map_ints > 8 and ops.conv2d_gskip_map_bytes(self.d, True) == ops.conv2d_gskip_map_bytes(self.d)
        self.ws_n = ops.conv2d_wgrad_bias_workspace_bytes(ops.gskip_desc(self.d)) // 4 + 64

    def new_map(self):
        return torch.full((self.map_ints,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")      # (garbage: a map needs no initialisation)

    def seed(self, pixels):
        """g with self.vals at the given (image, level, y, x) pixels (all channels), +0 elsewhere."""
        m = torch.zeros((N, self.geo.pix_per_img), dtype=torch.bool)
        for n, l, y, x in pixels:
            H, W = LEVELS[l]
            m[n, self.geo.off[l] + (y % H) * W + (x % W)] = True
        m = m.reshape(self.P, 1).cuda()
        return torch.where(m, self.vals, torch.zeros((), dtype=torch.bfloat16, device="cuda")).contiguous()

    def nan(self):
        return torch.full((self.P, C), NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)

    def wgrad(self, desc, x, g):
        ws = torch.empty((self.ws_n,), dtype=torch.float32, device="cuda")
        dw = torch.full((C, 3, 3, C), 7.0, device="cuda")
        db = torch.full((C,), 7.0, device="cuda")
        self.ops.conv2d_wgrad_bias(desc, x, g, dw, db, ws)
        return dw, db

    def chain(self, g0, hinted):
        """Four gated data gradients g0 -> dx1 -> .. -> dx4 plus the weight / bias gradients of the four layers.  hinted: the first call scans
        g0 and leaves dx1's map; every later call (and the weight gradients of dx1 .. dx3) reads the map its producer left."""
        ops, d = self.ops, self.d
        maps = [self.new_map() for _ in range(4)]
        g, out, names = g0, [], set()
        for i in range(4):
            if not hinted:
                hd = wd = d
            elif i == 0:
                hd = ops.gskip_desc(d, self.scratch, dxmap=maps[0])
                wd = ops.gskip_desc(d)
            else:
                hd = ops.gskip_desc(d, gmap=maps[i - 1], dxmap=maps[i])           # (no scratch: nothing is scanned)
                wd = ops.gskip_desc(d, gmap=maps[i - 1])
            out.append(self.wgrad(wd, self.act[i], g))
            names.add(_last_kernel())
            dx = self.nan()
            ops.conv2d_dgrad(hd, g, self.w[i], dx, mask=self.act[i], flags=ops.EPI_MASK)
            names.add(_last_kernel())
            out.append(dx)
            g = dx
        torch.cuda.synchronize()
        return out, names, maps


_CTX = []


@pytest.fixture(scope="module")
def ctx():
    if not _CTX:
        _CTX.append(_Ctx())
    return _CTX[0]


def _same(a, b, what):
    if isinstance(a, tuple):
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, (what, k))
        return
    bits = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    assert torch.equal(a.view(bits), b.view(bits)), (what, int((a.view(bits) != b.view(bits)).sum()))


def _placement():
    """Single pixels on patch corners, edges and centres of both tile geometries (4 x 16 and 8 x 8), the last row and column of a level, and
    the first pixel of image 1."""
    px = []
    for l, (H, W) in enumerate(LEVELS[:2]):
        px += [(0, l, 0, 0), (0, l, 3, 15), (0, l, 4, 16), (0, l, 7, 7), (0, l, 8, 8), (0, l, 2, 8), (0, l, 5, 20), (0, l, 3, 7),
               (0, l, H - 1, W - 1), (0, l, H - 1, 3), (0, l, 5, W - 1)]
    px += [(0, 4, 1, 2), (1, 0, 0, 0), (1, 2, 5, 9), (1, 3, 1, 1)]
    return px


SEEDS = {
    "placement": _placement,
    "dead": lambda: [],
    "live": lambda: [(n, l, y, x) for n in range(N) for l, (H, W) in enumerate(LEVELS) for y in range(H) for x in range(W)],
    "one": lambda: [(1, 1, 11, 19)],
}


@pytest.mark.parametrize("kind", ["placement", "dead", "live", "one", "negzero"])
def test_chain_of_four(ctx, kind):
    if kind == "negzero":                                   # the only nonzero BITS are one -0.0: it counts as live, as in the scan
        g0 = ctx.seed([])
        g0.view(torch.int16)[ctx.geo.pix_per_img + ctx.geo.off[1] + 7, 5] = NEG0
    else:
        g0 = ctx.seed(SEEDS[kind]())
    ref, _, _ = ctx.chain(g0, hinted=False)
    got, names, _ = ctx.chain(g0, hinted=True)
    assert names == {"conv3x3_pp_kernel", "conv_wgrad3x3_ring_kernel"}, names          # both hinted routes were taken
    for k, (a, b) in enumerate(zip(ref, got)):
        _same(a, b, (kind, k))


def test_promise_over_successive_calls(ctx):
    """Three calls on the same dx with different seeds -- disjoint, overlapping, empty -- from a NaN-filled dx and the promise off for the
    first call only: after each, ALL of dx equals the dense result (a patch left dirty, or cleared instead of computed, shows).  Then the
    promise is withdrawn (dx refilled with NaN in between, which the promise would not survive) and a last call runs."""
    ops, d = ctx.ops, ctx.d
    seeds = [[(0, 0, 2, 3), (1, 1, 11, 19), (0, 2, 5, 9)],
             [(0, 0, 20, 35), (1, 0, 0, 0), (1, 3, 2, 4)],                                   # disjoint from the first
             [(0, 0, 20, 35), (0, 0, 2, 3), (0, 1, 6, 10), (1, 4, 0, 0)],                   # overlaps both
             [],                                                                              # empty
             [(1, 1, 11, 19)]]
    gs = [ctx.seed(s) for s in seeds]
    gmap, dxmap = ctx.new_map(), ctx.new_map()
    dx = ctx.nan()
    for k, g in enumerate(gs):
        ref = ctx.nan()
        ops.conv2d_dgrad(d, g, ctx.w[0], ref, mask=ctx.act[0], flags=ops.EPI_MASK)
        clean = k not in (0, 4)
        if k == 4:
            dx.view(torch.int16).fill_(NAN16)
        if k % 2 == 0:        # the call scans g itself ...
            hd = ops.gskip_desc(d, ctx.scratch, dxmap=dxmap, dx_clean=clean)
        else:                 # ... or reads g's map
            ops.gskip_map_scan(d, g, gmap)
            hd = ops.gskip_desc(d, gmap=gmap, dxmap=dxmap, dx_clean=clean)
        ops.conv2d_dgrad(hd, g, ctx.w[0], dx, mask=ctx.act[0], flags=ops.EPI_MASK)
        torch.cuda.synchronize()
        _same(ref, dx, ("call", k))


@pytest.mark.parametrize("kind", ["placement", "live", "dead"])
def test_map_completeness(ctx, kind):
    """A producer's output map against the full scan of its dx: the producer tests the VALUES of every patch it computed and every other
    patch holds +0, so the flags of both geometries, the consumer's live flags, its live list and the count are all EQUAL (no superset)."""
    ops, d = ctx.ops, ctx.d
    g0 = ctx.seed(SEEDS[kind]())
    out, _, maps = ctx.chain(g0, hinted=True)
    p4 = (ops.conv2d_dgrad_gskip_bytes(d) // 4 - 4) // 3
    p8 = ctx.map_ints - 8 - 4 * p4
    assert p8 > 0
    for i in range(4):
        dx = out[2 * i + 1]
        ref = ops.gskip_map_scan(d, dx, ctx.new_map(), of_dx=True).cpu().numpy()
        got = maps[i].cpu().numpy()
        rc, gc = int(ref[0]) & 1, int(got[0]) & 1
        m4, m8, lv = slice(8, 8 + p4), slice(8 + p4, 8 + p4 + p8), slice(8 + p4 + p8, 8 + 2 * p4 + p8)
        assert np.array_equal(ref[m4], got[m4]), (kind, i, "4 x 16 words", np.flatnonzero(ref[m4] != got[m4])[:8])
        # (an 8 x 8 flag means "nonzero iff the patch holds a nonzero bit": the scan leaves its GS_* word there, the producer 0 / 1)
        assert np.array_equal(ref[m8] != 0, got[m8] != 0), (kind, i, "8 x 8 flags", np.flatnonzero((ref[m8] != 0) != (got[m8] != 0))[:8])
        assert np.array_equal(ref[lv], got[lv]), (kind, i, "live", np.flatnonzero(ref[lv] != got[lv])[:8])
        nr, ng = int(ref[2 + rc]), int(got[2 + gc])
        assert nr == ng, (kind, i, nr, ng)
        lr = ref[8 + 2 * p4 + p8 + rc * p4:][:nr]
        lg = got[8 + 2 * p4 + p8 + gc * p4:][:ng]
        assert np.array_equal(lr, lg) and np.all(np.diff(lg) > 0), (kind, i)
        assert int(got[1]) == 0                                 # the finished-workgroup counter is back at zero


def test_refusals(ctx):
    ops, d = ctx.ops, ctx.d
    from basedet_amd import _lib
    from basedet_amd._lib import BasedetHipError
    g = ctx.seed([(0, 0, 1, 1)])
    dx = ctx.nan()
    full, small = ctx.new_map(), ctx.new_map()[: ctx.map_ints - 1]
    ops.gskip_map_scan(d, g, full)
    for hd in (ops.gskip_desc(d, gmap=small), ops.gskip_desc(d, gmap=full, dxmap=small),
               ops.gskip_desc(d, ctx.scratch, dxmap=small), ops.gskip_desc(d, ctx.scratch, dx_clean=True)):        # (a promise without a map)
        with pytest.raises(BasedetHipError):
            ops.conv2d_dgrad(hd, g, ctx.w[0], dx, mask=ctx.act[0], flags=ops.EPI_MASK)
    with pytest.raises(BasedetHipError):                   # a map of dx under an in-place accumulate: dx outside the list is not +0
        ops.conv2d_dgrad(ops.gskip_desc(d, gmap=full, dxmap=ctx.new_map()), g, ctx.w[0], dx, add=dx, flags=ops.EPI_ADD_BEFORE)
    with pytest.raises(BasedetHipError):
        ctx.wgrad(ops.gskip_desc(d, gmap=small), ctx.act[0], g)
    with pytest.raises(BasedetHipError):
        ops.gskip_map_scan(d, g, small)
    torch.cuda.synchronize()
    assert torch.equal(dx.view(torch.int16), ctx.nan().view(torch.int16))          # nothing was launched
    # a library of another ABI version is refused at load time
    assert _lib.load().bd_version() == _lib.ABI_VERSION
    with pytest.raises(BasedetHipError):
        _lib.check_version(_lib.ABI_VERSION - 1)


def test_retinanet_two_steps_same_bits():
    """RetinaNet-R50 at 2 x 800 x 1344, two consecutive steps on different batches (the second one carries the promise): the gradient arena
    and dL/dP after each step equal those of the model with SPARSE_BOX_BWD = 0, bit for bit."""
    from basedet_amd.models import RetinaNet
    from basedet_amd.utils import DummyLoader
    from tests.test_model_gpu import _setup
    cfg, params, batch0 = _setup("resnet50", 2, (800, 1344))
    batch1 = next(DummyLoader(2, (800, 1344), seed=7))
    batch1["data"] = (batch1["data"] * 255).astype(np.float32)

    def run(on):
        cfg.MODEL.SPARSE_BOX_BWD = on
        model = RetinaNet(cfg, params=params)
        res = []
        for b in (batch0, batch1, batch0):
            model({k: (v if isinstance(v, dict) else torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in b.items()})
            model.backward()
            torch.cuda.synchronize()
            res.append((model.arena.g.clone(), model._cur.g_P.clone(), [t.clone() for t in model._cur.g_tower[1]]))
        chained = model._cur.g_map is not None and model._cur.chain_epoch == model.plan_arena.epoch
        del model
        torch.cuda.empty_cache()
        return res, chained

    ref, c0 = run(0)
    got, c1 = run(1)
    assert c1 and not c0                                    # the chain (and, from the second step on, the promise) was really on
    for k, (a, b) in enumerate(zip(ref, got)):
        _same(a[0], b[0], ("arena", k))
        _same(a[1], b[1], ("g_P", k))
        for i, (x, y) in enumerate(zip(a[2], b[2])):
            _same(x, y, ("g_tower", k, i))
