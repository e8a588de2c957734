"""Device half of CenterNet's training input: bd_affine_jitter_normalize against the numpy oracle (tests/center_affine_oracle.py), and
CenterNet trained one step from a CenterNetRawCollator batch against the same model fed the oracle's float batch.

Every comparison is BIT equality, with no tolerance: the warp is integer arithmetic, the colour stages are fp32 expressions of one IEEE
operation per numpy operation (multiply-add contraction off), the contrast mean comes from exact integer sums, and the expected x_halo
is bd_pad_normalize's own output from the oracle's bytes.  Every operand of every launch here lives between poisoned guards
(tests/test_guard_gpu.py Run): inputs keep their bits, outputs are written whole, nothing outside them changes.  The workspace starts
as 0xFF bytes in every run (the guard helper's fill for one-byte tensors): the entry zeroes its own counters.

Shapes: three sources of 37 x 53, 64 x 64 and 130 x 97 into 64 x 96 (wider than high, so a swapped height / width shows; 6 blocks of
256 lanes per image in launch 2, the last one ragged), and 33 images of 8 x 8 into 32 x 32 for the 32-descriptor batches."""
import functools

import numpy as np
import pytest
import torch

from tests import center_affine_oracle as O

pytestmark = pytest.mark.gpu

MEAN, STD = (103.53, 116.28, 123.675), (57.375, 57.12, 58.395)
SIZES = [(37, 53), (64, 64), (130, 97)]
OUT_H, OUT_W = 64, 96
V = 0.4
EVERY = O.BRIGHTNESS | O.CONTRAST | O.SATURATION | O.LIGHTING


@functools.lru_cache(maxsize=None)
def _images():
    rng = np.random.default_rng(11)
    out = []
    for h, w in SIZES:
        # smooth ramps plus noise: interpolation between unequal neighbours everywhere, every byte value present
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(3 * xx + 5 * yy) % 256, (7 * xx + yy) % 256, (xx * yy) % 256], -1)
        out.append(((base + rng.integers(0, 64, (h, w, 3))) % 256).astype(np.uint8))
    return out


def _center_map(h, w, cx, cy, side):
    """The inverse map of a CenterAffine draw (output_size = (OUT_W, OUT_H))."""
    return O.invert(O.forward_matrix(np.array([cx, cy], np.float32), side, (OUT_W, OUT_H)))


def _maps():
    """Per image: a source square smaller than the output (magnified: scale > 1), one much larger (scale < 1), one that hangs over
    the right and bottom borders of its image (zero-fill taps)."""
    return [_center_map(37, 53, 26, 18, 30.0), _center_map(64, 64, 31, 33, 150.0), _center_map(130, 97, 90, 120, 80.0)]


def _rotated():
    """Maps no CenterAffine draws: rotation, shear and unequal scales, so all six entries matter."""
    return [np.array([[0.61, -0.37, 9.3], [0.29, 0.83, -4.6]]), np.array([[-1.31, 0.22, 70.25], [0.4, 1.17, -8.0]]),
            np.array([[1.9, 0.55, -20.5], [-0.75, 2.4, 30.125]])]


LO, HI = 1 - V, 1 + V
DARK, BRIGHT = (-300.0, 12.25, 300.0), (300.0, -300.0, -7.5)          # saturate a channel at 0 and at 255
CASES = {
    # name: (maps, flips, stages, brightness, contrast, saturation, deltas) per image
    "warp": (_maps, (0, 0, 0), (0, 0, 0), None, None, None, None),
    "warp_rotated": (_rotated, (0, 1, 0), (0, 0, 0), None, None, None, None),
    "flip": (_maps, (1, 1, 1), (0, 0, 0), None, None, None, None),
    "brightness": (_maps, (0, 0, 0), (1, 1, 1), (LO, HI, 1.17), None, None, None),
    "contrast": (_maps, (0, 0, 0), (2, 2, 2), None, (LO, HI, 0.83), None, None),
    "saturation": (_maps, (0, 0, 0), (4, 4, 4), None, None, (LO, HI, 1.29), None),
    "lighting": (_maps, (0, 0, 0), (8, 8, 8), None, None, None, (DARK, BRIGHT, (-0.0179, 0.0162, 3.6))),
    "all": (_maps, (1, 0, 1), (EVERY, EVERY, EVERY), (HI, LO, 0.91), (LO, HI, 1.08), (HI, LO, 0.77), (BRIGHT, (1.5, -2.25, 0.5), DARK)),
    "mixed": (_rotated, (0, 1, 1), (EVERY, 0, O.BRIGHTNESS | O.SATURATION), (LO, 1.0, HI), (HI, 1.0, 1.0), (LO, 1.0, HI),
              (DARK, (0, 0, 0), (0, 0, 0))),
    "no_contrast": (_maps, (1, 0, 0), (13, 13, 5), (HI, LO, HI), None, (LO, HI, LO), (BRIGHT, DARK, (0, 0, 0))),      # the fused launch
}


def _descs(name, images=None):
    from basedet_amd import _lib
    maps, flips, stages, ab, ac, asat, deltas = CASES[name]
    images = images or _images()
    one = (1.0,) * len(images)
    out, off = [], 0
    for i, img in enumerate(images):
        d = _lib.AffineDesc(offset=off, src_h=img.shape[0], src_w=img.shape[1], flip=flips[i], stages=stages[i],
                            alpha_brightness=(ab or one)[i], alpha_contrast=(ac or one)[i], alpha_saturation=(asat or one)[i])
        d.inv[:] = maps()[i].reshape(6).tolist()
        d.delta[:] = list((deltas or ((0.0, 0.0, 0.0),) * len(images))[i])
        out.append(d)
        off += img.size
    return out


def _pack(images):
    return torch.from_numpy(np.concatenate([im.reshape(-1) for im in images]))


def _expected_halo(u8_images, out_h, out_w):
    """bd_pad_normalize's own output from the oracle's bytes."""
    from basedet_amd import ops
    out = torch.empty((len(u8_images), out_h + 6, out_w + 8, 4), dtype=torch.bfloat16, device="cuda")
    ops.pad_normalize(torch.from_numpy(O.to_batch(u8_images)).cuda(), out_h, out_w, MEAN, STD, out)
    return out


def _launch(descs, images, out_h, out_w, fill="nan", want_u8=True, ws_bytes=None):
    """One guarded call: (x_halo bits, u8 bytes) on the host."""
    from basedet_amd import ops
    from tests.test_guard_gpu import Run
    N = len(descs)
    r = Run(fill)
    packed = r.inp("packed", _pack(images))
    halo = r.out("x_halo", N * (out_h + 6) * (out_w + 8), 4, torch.bfloat16)
    # (255 is a byte the kernel may write: the u8 output starts as zeros instead of the sentinel, its guards hold the sentinel)
    u8 = r.inout("u8_out", torch.zeros((N * out_h * out_w, 3), dtype=torch.uint8)) if want_u8 else None
    ws = r.ws("ws", ops.affine_jitter_workspace_bytes(N, out_h, out_w) if ws_bytes is None else ws_bytes)
    assert bool((ws == 0xFF).all())
    ops.affine_jitter_normalize(packed, descs, out_h, out_w, MEAN, STD, halo.view(N, out_h + 6, out_w + 8, 4), ws, u8)
    got = r.finish()
    return got["x_halo"].cpu(), (got["u8_out"].cpu().numpy().reshape(N, out_h, out_w, 3) if want_u8 else None)


def _first_bad(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} element(s) differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


@pytest.mark.parametrize("name", list(CASES))
def test_bytes_and_x_halo_equal_the_oracle(name):
    descs = _descs(name)
    want = [O.pipeline_of_desc(img, d, OUT_H, OUT_W) for img, d in zip(_images(), descs)]
    if name == "warp":
        assert all((w == 0).all(-1).any() for w in want[2:]) and want[2][-1, -1].sum() == 0, "the third map must reach past its image"
    if name == "lighting":
        assert (want[0][..., 0] == 0).all() and (want[0][..., 2] == 255).all() and (want[1][..., 0] == 255).all()
    halo, u8 = _launch(descs, _images(), OUT_H, OUT_W)
    for i in range(len(descs)):
        assert np.array_equal(u8[i], want[i]), f"{name}: image {i}: " + _first_bad(u8[i], want[i])
    exp = _expected_halo(want, OUT_H, OUT_W).view(torch.int16).reshape(-1, 4).cpu()
    assert torch.equal(halo, exp), f"{name}: x_halo: " + _first_bad(halo.numpy(), exp.numpy())


def test_without_u8_out_and_across_input_fills():
    """u8_out = NULL writes the same x_halo; the guards of the packed input may hold anything (the dword taps stay inside it)."""
    base = None
    for fill, want_u8 in (("zero", False), ("max", True), ("nan", False)):
        halo, _ = _launch(_descs("all"), _images(), OUT_H, OUT_W, fill=fill, want_u8=want_u8)
        base = halo if base is None else base
        assert torch.equal(halo, base), fill


def test_descriptor_batches_of_32():
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, (8, 8, 3), dtype=np.uint8) for _ in range(33)]
    from basedet_amd import _lib
    for stages in (EVERY, O.BRIGHTNESS | O.LIGHTING):            # two launches per batch of 32, and the fused one
        descs = []
        for i, img in enumerate(images):
            d = _lib.AffineDesc(offset=i * 192, src_h=8, src_w=8, flip=i % 2, stages=stages, alpha_brightness=0.6 + 0.025 * i,
                                alpha_contrast=1.4 - 0.02 * i, alpha_saturation=0.7 + 0.02 * i)
            d.inv[:] = [0.25 + 0.01 * i, 0.02, -0.3 * (i % 5), -0.03, 0.27, 0.1 * (i % 3)]
            d.delta[:] = [i - 16.0, 0.5 * i, -1.0 * i]
            descs.append(d)
        want = [O.pipeline_of_desc(img, d, 32, 32) for img, d in zip(images, descs)]
        assert len({w.tobytes() for w in want}) == 33
        halo, u8 = _launch(descs, images, 32, 32)
        for i in range(33):
            assert np.array_equal(u8[i], want[i]), f"image {i}: " + _first_bad(u8[i], want[i])
        assert torch.equal(halo, _expected_halo(want, 32, 32).view(torch.int16).reshape(-1, 4).cpu())


def test_two_runs_give_the_same_bytes_from_a_dirty_workspace():
    """The same tensors twice; the workspace holds 0xFF before each run (counters included): the entry zeroes them itself."""
    from basedet_amd import ops
    descs, images = _descs("all"), _images()
    N = len(descs)
    packed = _pack(images).cuda()
    halo = torch.empty((N, OUT_H + 6, OUT_W + 8, 4), dtype=torch.bfloat16, device="cuda")
    u8 = torch.empty((N, OUT_H, OUT_W, 3), dtype=torch.uint8, device="cuda")
    ws = torch.empty(ops.affine_jitter_workspace_bytes(N, OUT_H, OUT_W), dtype=torch.uint8, device="cuda")
    runs = []
    for _ in range(2):
        ws.fill_(0xFF)
        halo.view(torch.int16).fill_(0x7fc1)
        u8.fill_(7)
        ops.affine_jitter_normalize(packed, descs, OUT_H, OUT_W, MEAN, STD, halo, ws, u8)
        runs.append((halo.view(torch.int16).cpu().clone(), u8.cpu().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    want = np.stack([O.pipeline_of_desc(img, d, OUT_H, OUT_W) for img, d in zip(images, descs)])
    assert np.array_equal(runs[1][1].numpy(), want)


def test_invalid_arguments_return_einval_and_write_nothing():
    from basedet_amd import _lib, ops
    img = _images()[0]
    packed = _pack([img]).cuda()
    out = torch.empty((1, 38, 40, 4), dtype=torch.bfloat16, device="cuda")
    out.view(torch.int16).fill_(0x7fc1)
    ws = torch.full((ops.affine_jitter_workspace_bytes(1, 32, 32),), 0xFF, dtype=torch.uint8, device="cuda")
    ident = [1.0, 0, 0, 0, 1.0, 0]

    def desc(inv=ident, **kw):
        d = _lib.AffineDesc(**{**dict(offset=0, src_h=37, src_w=53, stages=EVERY, alpha_brightness=1.0, alpha_contrast=1.0,
                                      alpha_saturation=1.0), **kw})
        d.inv[:] = inv
        return d
    run = lambda d, h=32, w=32, o=out, s=ws: ops.affine_jitter_normalize(packed, [d], h, w, MEAN, STD, o, s)
    wide = torch.empty((1, 38, 56, 4), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.BasedetHipError, match="multiples of 32"):
        run(desc(), 32, 48, wide)                                             # out_w not a multiple of 32
    with pytest.raises(_lib.BasedetHipError, match="end past"):
        run(desc(offset=packed.numel() + 1))                                  # an offset past packed_bytes
    with pytest.raises(_lib.BasedetHipError, match="end past"):
        run(desc(offset=3))                                                   # ... and an image that ends past them
    with pytest.raises(_lib.BasedetHipError, match="singular"):
        run(desc(inv=[0.0] * 6))                                              # what inverting a singular map gives
    with pytest.raises(_lib.BasedetHipError, match="singular"):
        run(desc(inv=[1.0, 2.0, 0, 2.0, 4.0, 0]))
    with pytest.raises(_lib.BasedetHipError, match="not finite"):
        run(desc(inv=[float("nan"), 0, 0, 0, 1.0, 0]))
    with pytest.raises(_lib.BasedetHipError, match="not finite"):
        run(desc(alpha_contrast=float("inf")))
    with pytest.raises(_lib.BasedetHipError, match="workspace"):
        run(desc(), s=ws[:-4])                                                # contrast enabled, workspace too small
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == 0x7fc1).all()) and bool((ws == 0xFF).all())
    run(desc())                                                               # and the valid descriptor runs
    torch.cuda.synchronize()
    assert not bool((out.view(torch.int16) == 0x7fc1).any())


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _e2e_cfg():
    from basedet_amd.configs import CenterNetConfig
    cfg = CenterNetConfig()
    cfg.merge(dict(MODEL=dict(BATCHSIZE=4, WEIGHTS=None, BACKBONE=dict(NAME="resnet18", NORM="BN", FREEZE_AT=0),
                              HEAD=dict(DECONV_CHANNEL=[512, 256, 128, 64], IN_CHANNELS=64, TENSOR_DIM=8), OUTPUT_SIZE=(16, 16)),
                   DATA=dict(NUM_CLASSES=3)))
    return cfg


def test_centernet_trains_from_the_collator_as_from_the_oracle_batch():
    from basedet.data import CenterNetRawCollator
    from basedet_amd.models import CenterNet
    cfg = _e2e_cfg()
    spec = [(n, dict(kw, output_size=(64, 64)) if n == "CenterAffine" else kw) for n, kw in cfg.AUG.TRAIN_VALUE]
    rng = np.random.default_rng(21)
    samples = []
    for (h, w) in SIZES + [(48, 80)]:
        x = np.sort(rng.uniform(0, w, (3, 2)), axis=1)
        y = np.sort(rng.uniform(0, h, (3, 2)), axis=1)
        boxes = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32)
        samples.append((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), boxes, rng.integers(1, 4, (3,)).astype(np.float32), (h, w)))
    batch = CenterNetRawCollator(spec, np.random.default_rng(2))(samples)
    descs = batch["data"].descs
    assert batch["im_info"][:, 4].sum() > 0 and all(d.stages == EVERY for d in descs), "the batch must carry boxes and every stage"
    floats = O.to_batch([O.pipeline_of_desc(s[0], d, 64, 64) for s, d in zip(samples, descs)])
    torch.manual_seed(0)
    model = CenterNet(cfg)
    got = {k: v.clone() for k, v in model(batch).items()}
    model.backward()
    x_raw = model._cur.x_halo.clone()
    want = {k: v.clone() for k, v in model(dict(data=floats, gt_boxes=batch["gt_boxes"], im_info=batch["im_info"])).items()}
    model.backward()
    torch.cuda.synchronize()
    assert torch.equal(x_raw.view(torch.int16), model._cur.x_halo.view(torch.int16)), "the two input paths fill x_halo differently"
    for k in ("total_loss", "loss_cls", "loss_box_wh", "loss_center_reg"):
        assert bool(torch.isfinite(got[k])), (k, got[k])
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (k, float(got[k]), float(want[k]))
