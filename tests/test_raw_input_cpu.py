"""Host half of the raw-image input (basedet_amd/data/raw.py): RawBatchCollator against the path it stands in for, the numpy Compose of
data/transforms.py followed by DetectionPadCollator, on the same seeded samples.  No device: boxes, im_info, the per-image resize / flip
parameters and the RNG stream are compared exactly; the pixels are the kernel's business (tests/test_raw_input_gpu.py)."""
import numpy as np
import pytest

from basedet_amd.data import (DetectionPadCollator, RawBatchCollator, RawImageBatch, RandomHorizontalFlip, ShortestEdgeResize, ToMode,
                              build_transform)
from basedet_amd.data.transforms import Compose, _Transform

SPEC = (("ShortestEdgeResize", dict(min_size=(48, 64), max_size=100, sample_style="choice")),
        ("RandomHorizontalFlip", dict(prob=0.5)), ("ToMode", dict(mode="CHW")))
SIZES = [(37, 53), (150, 97), (64, 80), (33, 31), (200, 300)]


def _samples(seed, sizes=SIZES):
    """(image HWC uint8, boxes (n, 4) inside the image, categories, (H, W)) per size; the third image has no box."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (h, w) in enumerate(sizes):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        n = 0 if i == 2 else int(rng.integers(1, 5))
        x = np.sort(rng.uniform(0, w, (n, 2)), axis=1)
        y = np.sort(rng.uniform(0, h, (n, 2)), axis=1)
        boxes = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32).reshape(-1, 4)
        out.append((img, boxes, rng.integers(0, 80, (n,)).astype(np.float32), (h, w)))
    return out


def _numpy_path(compose, samples):
    """What the dataset does today: Compose per sample, then the pad collator.  Also returns every sample's (dst_h, dst_w, flip)."""
    done, params = [], []
    for img, boxes, cat, info in samples:
        im, bx, ct = compose((img, boxes, cat))
        flips = [t._flip for t in compose.transforms if isinstance(t, RandomHorizontalFlip)]
        params.append((im.shape[1], im.shape[2], int(sum(flips) % 2)))
        done.append((im, bx, ct, info))
    return DetectionPadCollator()(done), params


def test_rng_stream_boxes_and_im_info_match_the_numpy_pipeline():
    raw = RawBatchCollator(build_transform(SPEC, "train", rng=np.random.default_rng(7)))
    compose = build_transform(SPEC, "train", rng=np.random.default_rng(7))
    seen_flips = set()
    for batch_seed in (11, 12):                      # the second batch continues the same RNG stream
        samples = _samples(batch_seed)
        got = raw.apply(samples)
        want, params = _numpy_path(compose, samples)
        assert isinstance(got["data"], RawImageBatch) and got["data"].N == len(samples)
        assert got["gt_boxes"].dtype == np.float32 and got["gt_boxes"].shape == want["gt_boxes"].shape
        assert np.array_equal(got["gt_boxes"].view(np.int32), want["gt_boxes"].view(np.int32))
        assert got["im_info"].dtype == np.float32 and np.array_equal(got["im_info"].view(np.int32), want["im_info"].view(np.int32))
        assert [(d.dst_h, d.dst_w, d.flip) for d in got["data"].descs] == params
        assert [(d.src_h, d.src_w) for d in got["data"].descs] == SIZES
        assert (got["data"].Hmax, got["data"].Wmax) == want["data"].shape[2:]
        seen_flips |= {p[2] for p in params}
    assert seen_flips == {0, 1}, "the seed must flip some images and leave some"


def test_packed_bytes_offsets_and_buffer_reuse():
    raw = RawBatchCollator(build_transform(SPEC, "train", rng=np.random.default_rng(3)))
    samples = _samples(21)
    batch = raw.apply(samples)["data"]
    flat = batch.packed.numpy()
    assert batch.packed.dtype.is_floating_point is False and flat.dtype == np.uint8
    end = 0
    for (img, _, _, _), d in zip(samples, batch.descs):
        assert d.offset >= end, "images overlap in the packed buffer"
        end = d.offset + img.size
        assert np.array_equal(flat[d.offset:end].reshape(img.shape), img)
    assert end <= flat.size
    first = batch.packed.data_ptr()
    for sizes in (SIZES, SIZES[:3]):                 # an equal and a smaller batch land in the same storage
        again = raw.apply(_samples(22, sizes))["data"]
        assert again.packed.data_ptr() == first and again.N == len(sizes)
    bigger = raw.apply(_samples(23, SIZES + [(120, 130)]))["data"]
    assert bigger.packed.numel() > batch.packed.numel()
    img = _samples(23, SIZES + [(120, 130)])[-1][0]
    d = bigger.descs[-1]
    assert np.array_equal(bigger.packed.numpy()[d.offset:d.offset + img.size].reshape(img.shape), img)


def test_a_strided_image_is_packed_contiguously():
    raw = RawBatchCollator(build_transform(SPEC, "train", rng=np.random.default_rng(0)))
    img, boxes, cat, info = _samples(5, [(40, 50)])[0]
    wide = np.zeros((40, 70, 3), np.uint8)
    wide[:, :50] = img
    batch = raw.apply([(wide[:, :50], boxes, cat, info)])["data"]
    assert np.array_equal(batch.packed.numpy()[:img.size].reshape(img.shape), img)


class _Blur(_Transform):
    pass


class _MyResize(ShortestEdgeResize):
    pass


def test_rejections():
    good = build_transform(SPEC, "train", rng=np.random.default_rng(0))
    raw = RawBatchCollator(good)
    img, boxes, cat, info = _samples(1, [(20, 30)])[0]
    with pytest.raises(ValueError):
        raw.apply([(img.astype(np.float32), boxes, cat, info)])
    with pytest.raises(ValueError):
        raw.apply([(img[:, :, :1], boxes, cat, info)])
    with pytest.raises(ValueError):
        raw.apply([(img[:, :, 0], boxes, cat, info)])
    with pytest.raises(ValueError):
        RawBatchCollator(Compose([ShortestEdgeResize(48, 100), _Blur(), ToMode("CHW")]))
    with pytest.raises(ValueError):                  # a subclass may do anything to the pixels
        RawBatchCollator(Compose([_MyResize(48, 100), ToMode("CHW")]))
    with pytest.raises(ValueError):                  # flip before resize is not what the kernel computes
        RawBatchCollator(Compose([RandomHorizontalFlip(0.5), ShortestEdgeResize(48, 100), ToMode("CHW")]))
    with pytest.raises(ValueError):                  # the device pads with 0
        RawBatchCollator(good, pad_value=114.0)
    with pytest.raises(ValueError):
        RawBatchCollator(lambda s: s)


def test_test_mode_im_info():
    spec = (("ShortestEdgeResize", dict(min_size=48, max_size=100, sample_style="choice")), ("ToMode", dict(mode="NCHW")))
    raw = RawBatchCollator(build_transform(spec, "test"))
    ttc = build_transform(spec, "test")
    images = [s[0] for s in _samples(31)]
    got = raw.apply(images)
    assert got["gt_boxes"].shape == (len(images), 0, 5)
    for i, img in enumerate(images):
        out, info = ttc(img)
        assert np.array_equal(got["im_info"][i], np.concatenate([info[0], [0]]).astype(np.float32))
        d = got["data"].descs[i]
        assert (d.dst_h, d.dst_w, d.flip) == (out.shape[2], out.shape[3], 0)
    assert (got["data"].Hmax, got["data"].Wmax) == (max(d.dst_h for d in got["data"].descs), max(d.dst_w for d in got["data"].descs))
