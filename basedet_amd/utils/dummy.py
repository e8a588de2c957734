"""Synthetic batch generator restating basedet/utils/dummy.py:8-63 (the reference's benchmark input,
tools/benchmark.py:173).  The annotation pattern is data (also pinned in tests/golden/dummy_loader.npz).

MultiScaleDummyLoader (DATA.DUMMY_MULTISCALE): the same pattern on synthetic images of COCO-like original sizes, through the
training recipe's own host pipeline -- AUG.TRAIN_VALUE (ShortestEdgeResize 640..800 / max 1333 + flip), aspect-ratio grouping and the
pad collator -- so that a run sees the recipe's stream of batch shapes."""
import numpy as np

__all__ = ["DummyLoader", "MultiScaleDummyLoader", "DUMMY_ORIG_SIZES"]

# (H, W) of the synthetic originals: common COCO train2017 image sizes, landscape and portrait
DUMMY_ORIG_SIZES = ((480, 640), (427, 640), (640, 480), (640, 427), (424, 640), (375, 500), (500, 375), (612, 612), (640, 512),
                    (333, 500), (640, 360), (360, 640))

_ANNO = np.array([
    [[0., 0., 800., 800., 61.], [148.33984, 488.73206, 667.7124, 602.64056, 52.],
     [170.45752, 422.78433, 572.1176, 552.15686, 52.], [228.24835, 486.88892, 600.71893, 589.39874, 52.],
     [71.803894, 54.444447, 110.20911, 78.19608, 43.], [237.46405, 0., 418.64053, 32.03922, 41.],
     [315.08798, 101.472, 464.52798, 797.696, 80.], [280.448, 118.096, 370.336, 786.864, 70.],
     [228.31999, 104.71999, 307.40802, 791.456, 40.], [145.61601, 94.736, 246.288, 786.86395, 20.]],
    [[315.08798, 101.472, 464.52798, 797.696, 30.], [280.448, 118.096, 370.336, 786.864, 20.],
     [228.31999, 104.71999, 307.40802, 791.456, 10.], [145.61601, 94.736, 246.288, 786.86395, 60.],
     [68.32, 101.12, 244.496, 787.872, 70.], [0., 0., 0., 0., 0.], [0., 0., 0., 0., 0.], [0., 0., 0., 0., 0.],
     [0., 0., 0., 0., 0.], [0., 0., 0., 0., 0.]],
], dtype="float32")


class DummyLoader:
    def __init__(self, batch_size=2, output_size=(800, 1344), seed=None):
        self.batch_size = batch_size
        self.output_size = output_size
        self.anno = _ANNO.copy()
        self.anno *= min(output_size[0] / 800, output_size[1] / 800)          # dummy.py:40-41
        self.im_info = np.array([[*output_size, 612., 612., 10.], [*output_size, 500., 375., 5.]], dtype="float32")
        # the reference draws unseeded float64 noise (dummy.py:60); a seed makes parity runs reproducible
        self._rng = np.random.default_rng(seed)

    def __iter__(self):
        return self

    def _tile(self, x):
        repeat = self.batch_size // len(self.anno)                           # dummy.py:51-57
        remain = self.batch_size % len(self.anno)
        return np.concatenate([np.repeat(x, repeat, axis=0), x[:remain, ...]], axis=0)

    def __next__(self):
        return {
            "data": self._rng.random(size=(self.batch_size, 3, *self.output_size)),
            "gt_boxes": self._tile(self.anno),
            "im_info": self._tile(self.im_info),
        }


class _SizeTable:
    """The dataset protocol AspectRatioGroupSampler reads (len, get_img_info) over a fixed list of original sizes."""

    def __init__(self, sizes):
        self.sizes = [tuple(int(v) for v in hw) for hw in sizes]

    def __len__(self):
        return len(self.sizes)

    def get_img_info(self, i):
        h, w = self.sizes[i]
        return {"height": h, "width": w}


class MultiScaleDummyLoader:
    """Endless batches of `batch_size` synthetic images: original sizes from `orig_sizes`, uint8 noise, DummyLoader's boxes scaled to
    each original as DummyLoader scales them to its output size; every sample goes through `build_transform(transform_spec)`,
    batches are formed by AspectRatioGroupSampler (one aspect group per batch) and padded by DetectionPadCollator.

    Seeded: the sampler draws the index lists from `seed`; batch b's pixels and transform draws come from its own generator
    (seed, b), so `make_batch(b, indices)` can run in worker processes and still give exactly the batches `next()` gives."""

    def __init__(self, batch_size=2, transform_spec=None, orig_sizes=DUMMY_ORIG_SIZES, seed=None, aspect_grouping=(1,)):
        from ..data import AspectRatioGroupSampler
        self.batch_size = int(batch_size)
        self.seed = 0 if seed is None else int(seed)
        self.transform_spec = transform_spec
        self.sizes = [tuple(int(v) for v in hw) for hw in orig_sizes]
        self._sampler = AspectRatioGroupSampler(_SizeTable(self.sizes), self.batch_size, aspect_grouping, seed=self.seed)
        self._batches = iter(())
        self._b = 0

    def __iter__(self):
        return self

    def next_indices(self):
        """(batch number, original-size indices) of the next batch: the sequential, cheap part of next()."""
        idx = next(self._batches, None)
        while idx is None:
            self._batches = iter(self._sampler)          # one sampler pass; the groups' partial queues carry over
            idx = next(self._batches, None)
        b, self._b = self._b, self._b + 1
        return b, list(idx)

    def make_batch(self, b, indices):
        from ..data import DetectionPadCollator, build_transform
        rng = np.random.default_rng([self.seed, int(b)])
        tf = build_transform(self.transform_spec, "train", rng=rng)
        samples = []
        for k, i in enumerate(indices):
            h, w = self.sizes[i]
            anno = _ANNO[k % len(_ANNO)]
            anno = anno[anno[:, 4] > 0].copy()
            anno[:, :4] *= np.float32(min(h / 800, w / 800))                 # inside the original: coordinates <= 800 before scaling
            # the pixels are noise: the transforms run on a zero-channel stand-in of the original (every geometric draw -- size choice,
            # flip -- and the box mapping are the pipeline's own) and the noise is drawn at the transformed size, which spares the ~0.1 s
            # bilinear resize of noise per image
            image, boxes, cat = tf.apply((np.empty((h, w, 0), np.uint8), anno[:, :4].copy(), anno[:, 4].copy()))
            nh, nw = image.shape[1:]
            image = rng.integers(0, 256, size=(3, nh, nw), dtype=np.uint8)
            # a box on the border comes out of resize + flip a rounding error outside the image (x' = W - x2 = -6e-5): clip it
            boxes = np.clip(boxes, 0, np.array([nw, nh, nw, nh], np.float32))
            samples.append((image, boxes, cat, (h, w)))
        return DetectionPadCollator().apply(samples)

    def __next__(self):
        return self.make_batch(*self.next_indices())
