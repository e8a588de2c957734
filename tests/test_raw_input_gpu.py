"""Device half of the raw-image input: bd_resize_pad_normalize and FPNDetector.pre_process on a RawImageBatch against the path they
stand in for -- numpy Compose (data/transforms.py), DetectionPadCollator, fp32 batch to the device, bd_pad_normalize -- on the same
seeded samples.

Every comparison is BIT equality of the bf16 x_halo tensor (as int16, halo and pad region included), with no tolerance: with multiply-add
contraction off every step of the kernel's resize is the same IEEE operation numpy performs (float64 source coordinate, fp32 blends,
rint), the normalisation is bd_pad_normalize's own expression, and the pad region is (0 - mean) / std on both sides.  A mismatch is a
bug (usually a contracted a * (1 - f) + b * f flipping rint at a tie), not noise.

The five image sizes and the spec of the main case are fixed by the feature's acceptance: up- and downscaling (200 x 300 -> 64 x 96 is a
factor above 3), odd resized widths (69: the two-pixel lane's tail), images smaller than the batch maximum (per-image pad region), both
flip states.  None of those five reaches the max_size clamp at max_size = 100 (the largest long edge comes out at 99), so a further
case with 40 x 90 and 90 x 40 images (-> 44 x 100 and 100 x 44) covers it.  The identity resize (min_size = the short edge) also reads
the very last pixel of the packed buffer, where the kernel's dword load gives way to byte loads."""
import numpy as np
import pytest
import torch

from basedet_amd.data import DetectionPadCollator, RawBatchCollator, build_transform

pytestmark = pytest.mark.gpu

MEAN, STD = (103.53, 116.28, 123.675), (57.375, 57.12, 58.395)
SPEC = (("ShortestEdgeResize", dict(min_size=(48, 64), max_size=100, sample_style="choice")),
        ("RandomHorizontalFlip", dict(prob=0.5)), ("ToMode", dict(mode="CHW")))
SIZES = [(37, 53), (150, 97), (64, 80), (33, 31), (200, 300)]


def _round_up(v, m):
    return (v + m - 1) // m * m


def _samples(seed, sizes):
    rng = np.random.default_rng(seed)
    out = []
    for h, w in sizes:
        n = int(rng.integers(1, 4))
        x = np.sort(rng.uniform(0, w, (n, 2)), axis=1)
        y = np.sort(rng.uniform(0, h, (n, 2)), axis=1)
        boxes = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32)
        out.append((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), boxes, rng.integers(0, 80, (n,)).astype(np.float32), (h, w)))
    return out


def _existing_batch(spec, seed, samples):
    compose = build_transform(spec, "train", rng=np.random.default_rng(seed))
    done = []
    for img, boxes, cat, info in samples:
        im, bx, ct = compose((img, boxes, cat))
        done.append((im, bx, ct, info))
    return DetectionPadCollator()(done)


def _raw_batch(spec, seed, samples):
    return RawBatchCollator(build_transform(spec, "train", rng=np.random.default_rng(seed)))(samples)


def _x_halo_existing(data):
    from basedet_amd import ops
    N, _, H, W = data.shape
    Hp, Wp = _round_up(H, 32), _round_up(W, 32)
    out = torch.empty((N, Hp + 6, Wp + 8, 4), dtype=torch.bfloat16, device="cuda")
    ops.pad_normalize(torch.from_numpy(data).cuda(), Hp, Wp, MEAN, STD, out)
    return out


def _x_halo_raw(raw):
    from basedet_amd import ops
    Hp, Wp = _round_up(raw.Hmax, 32), _round_up(raw.Wmax, 32)
    out = torch.empty((raw.N, Hp + 6, Wp + 8, 4), dtype=torch.bfloat16, device="cuda")
    out.view(torch.int16).fill_(0x7fc1)              # a NaN pattern neither path produces: every element must be written
    ops.resize_pad_normalize(raw.packed.cuda(), raw.descs, Hp, Wp, MEAN, STD, out)
    return out


def _assert_same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(torch.int16), want.view(torch.int16)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        first = [(tuple(int(v) for v in ix), float(got[tuple(ix)]), float(want[tuple(ix)])) for ix in bad[:8]]
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} bf16 elements differ; first (n, yb, xb, c), got, want: {first}")


def _check_case(spec, seed, samples, what, want_flips=None):
    want = _existing_batch(spec, seed, samples)
    got = _raw_batch(spec, seed, samples)
    if want_flips is not None:
        assert {d.flip for d in got["data"].descs} == want_flips, "the seed must flip some images and leave some"
    assert np.array_equal(got["im_info"], want["im_info"]) and np.array_equal(got["gt_boxes"], want["gt_boxes"])
    _assert_same_bits(_x_halo_raw(got["data"]), _x_halo_existing(want["data"]), what)
    return got["data"]


@pytest.mark.parametrize("seed", [6, 1])
def test_kernel_bits_five_images(seed):
    """seed 6: resized 48x69 (flipped), 99x64 (flipped), 64x80, 51x48, 48x72 (flipped); seed 1: 48x69 not flipped, the rest flipped."""
    raw = _check_case(SPEC, seed, _samples(40, SIZES), f"five images, seed {seed}", want_flips={0, 1})
    assert any(d.dst_w % 2 for d in raw.descs), "an odd resized width must be among the cases"
    assert any(d.dst_h < raw.Hmax for d in raw.descs) and any(d.dst_w < raw.Wmax for d in raw.descs)
    assert any(d.src_h > 2 * d.dst_h for d in raw.descs) and any(d.src_h < d.dst_h for d in raw.descs)


def test_kernel_bits_identity_resize():
    spec = (("ShortestEdgeResize", dict(min_size=(64,), max_size=100, sample_style="choice")),) + SPEC[1:]
    raw = _check_case(spec, 2, _samples(41, [(64, 80), (80, 64), (64, 64), (64, 77)]), "identity resize", want_flips={0, 1})
    assert all((d.src_h, d.src_w) == (d.dst_h, d.dst_w) for d in raw.descs)


def test_kernel_bits_max_size_clamp():
    raw = _check_case(SPEC, 3, _samples(42, [(40, 90), (90, 40), (30, 91)]), "max_size clamp")
    assert all(max(d.dst_h, d.dst_w) == 100 for d in raw.descs)


def test_kernel_bits_two_launch_groups():
    """33 images cross the 32-descriptor group of one launch; every resized image lies inside Hp = Wp = 32."""
    spec = (("ShortestEdgeResize", dict(min_size=(24, 32), max_size=32, sample_style="choice")),) + SPEC[1:]
    sizes = [(9 + i % 12, 11 + (7 * i) % 10) for i in range(33)]
    assert min(sizes) == (9, 11) and max(h for h, _ in sizes) == 20 and max(w for _, w in sizes) == 20
    raw = _check_case(spec, 4, _samples(43, sizes), "33 images", want_flips={0, 1})
    assert raw.N == 33 and (_round_up(raw.Hmax, 32), _round_up(raw.Wmax, 32)) == (32, 32)


def test_validation_launches_nothing():
    from basedet_amd import _lib, ops
    img = np.random.default_rng(0).integers(0, 256, (10, 12, 3), dtype=np.uint8)
    packed = torch.from_numpy(img.reshape(-1).copy()).cuda()
    out = torch.empty((1, 32 + 6, 32 + 8, 4), dtype=torch.bfloat16, device="cuda")
    out.view(torch.int16).fill_(0x7fc1)
    ok = dict(offset=0, src_h=10, src_w=12, dst_h=20, dst_w=24, flip=0)
    bad = [dict(ok, dst_w=33), dict(ok, dst_h=33), dict(ok, offset=img.size), dict(ok, offset=1), dict(ok, offset=-1), dict(ok, src_h=11),
           dict(ok, src_w=0), dict(ok, dst_h=0)]
    for kw in bad:
        with pytest.raises(RuntimeError):
            ops.resize_pad_normalize(packed, [_lib.ImageDesc(**kw)], 32, 32, MEAN, STD, out)
    with pytest.raises(RuntimeError):                # Wp not a multiple of 32 (an output of the same element count)
        ops.resize_pad_normalize(packed, [_lib.ImageDesc(**ok)], 32, 24, MEAN, STD, out.view(-1)[: 38 * 32 * 4].view(1, 38, 32, 4))
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == 0x7fc1).all()), "a rejected call wrote to the output"
    ops.resize_pad_normalize(packed, [_lib.ImageDesc(**ok)], 32, 32, MEAN, STD, out)        # and the valid descriptor runs
    torch.cuda.synchronize()
    assert not bool((out.view(torch.int16) == 0x7fc1).any())


# ---- model level: RetinaNet R18, two images that resize to 128 x 160 and 113 x 160 ---------------------------------------------------
MODEL_SIZES = [(96, 120), (100, 141)]
TRAIN_SPEC = (("ShortestEdgeResize", dict(min_size=(128,), max_size=160, sample_style="choice")),
              ("RandomHorizontalFlip", dict(prob=0.5)), ("ToMode", dict(mode="CHW")))
TEST_SPEC = (("ShortestEdgeResize", dict(min_size=128, max_size=160, sample_style="choice")), ("ToMode", dict(mode="NCHW")))


def test_model_losses_bit_equal():
    from basedet_amd.models import RetinaNet
    from tests.test_model_gpu import _setup
    cfg, params, _ = _setup("resnet18", 2, (128, 160), seed=0)
    samples = _samples(44, MODEL_SIZES)
    want_batch = _existing_batch(TRAIN_SPEC, 9, samples)
    got_batch = _raw_batch(TRAIN_SPEC, 9, samples)
    assert want_batch["data"].shape == (2, 3, 128, 160) and {d.flip for d in got_batch["data"].descs} == {0, 1}
    model = RetinaNet(cfg, params=params)
    want = {k: float(v) for k, v in model.get_losses(want_batch).items()}
    x_want = model._cur.x_halo.clone()
    got = {k: float(v) for k, v in model.get_losses(got_batch).items()}
    _assert_same_bits(model._cur.x_halo, x_want, "x_halo of the model's plan")
    assert set(got) == set(want) == {"total_loss", "cls_loss", "reg_loss"}
    for k in want:
        assert np.isfinite(want[k]) and got[k] == want[k], (k, got[k], want[k])
    # a second raw batch through the same collator and model: the packed buffer is reused after the first copy has drained
    coll = RawBatchCollator(build_transform(TRAIN_SPEC, "train", rng=np.random.default_rng(9)))
    for _ in range(2):
        again = {k: float(v) for k, v in model.get_losses(coll(samples)).items()}
    ref2 = _existing_batch(TRAIN_SPEC, 9, samples + samples)      # (the second pass of the stream: samples 3 and 4 of one Compose)
    ref2 = {k: v[2:] for k, v in ref2.items()}
    want2 = {k: float(v) for k, v in model.get_losses(ref2).items()}
    assert again == want2


def test_model_inference_batch_same_detections():
    from basedet_amd.models import RetinaNet
    from tests.test_batched_inference_gpu import _shift_for_fraction
    from tests.test_model_gpu import _setup
    cfg, params, _ = _setup("resnet18", 2, (128, 160), seed=5)
    params["head.cls_score.weight"] = params["head.cls_score.weight"] * 8
    params["head.bbox_pred.weight"] = params["head.bbox_pred.weight"] * 8
    images = [s[0] for s in _samples(45, MODEL_SIZES)]
    ttc = build_transform(TEST_SPEC, "test")
    data = np.zeros((2, 3, 128, 160), np.float32)
    info = np.zeros((2, 5), np.float32)
    for i, img in enumerate(images):
        out, inf = ttc(img)
        data[i, :, :out.shape[2], :out.shape[3]] = out[0]
        info[i, :4] = inf[0]
    want_batch = {"data": data, "im_info": info}
    got_batch = RawBatchCollator(build_transform(TEST_SPEC, "test"))(images)
    assert np.array_equal(got_batch["im_info"], info)
    # enough candidates above TEST.CLS_THRESHOLD for the comparison to mean something (tests/test_batched_inference_gpu.py's recipe)
    model = RetinaNet(cfg, params=params).eval()
    model.inference_batch(want_batch)
    logits = model._plan(2, 128, 160).logits.float().reshape(-1)
    thr = cfg.TEST.CLS_THRESHOLD
    shift = _shift_for_fraction(lambda s: float((torch.sigmoid(logits + s) > thr).float().mean()), 2e-2)
    params["head.cls_score.bias"] = params["head.cls_score.bias"] + np.float32(shift)
    model = RetinaNet(cfg, params=params).eval()
    want = [{k: torch.as_tensor(o[k]).clone() for k in ("boxes", "box_scores", "box_labels")} for o in model.inference_batch(want_batch)]
    got = model.inference_batch(got_batch)
    assert len(got) == len(want) == 2 and sum(w["box_scores"].numel() for w in want) > 0
    for g, w in zip(got, want):
        for k in ("boxes", "box_scores", "box_labels"):
            assert torch.equal(torch.as_tensor(g[k]), w[k]), k
