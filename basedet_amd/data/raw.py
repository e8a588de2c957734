"""Raw-image batches: the decoded uint8 HWC images travel to the device as they are, and ONE kernel (bd_resize_pad_normalize) resizes,
flips, pads and normalises them there -- instead of the numpy resize of transforms.py, the fp32 (N, 3, Hmax, Wmax) batch of
DetectionPadCollator and twelve times the bytes over the link.

``RawBatchCollator`` stands where ``Compose`` + ``DetectionPadCollator`` stand today.  It draws every sample's augmentation parameters
through the transforms' own ``_get_params`` (the RNG stream is the one ``Compose.apply`` consumes, sample for sample), transforms the
boxes on the host with the transforms' own ``_apply_boxes`` (a few hundred floats per batch), and describes what is left to do to the
pixels in one descriptor per image.  ``FPNDetector.pre_process`` accepts the resulting ``RawImageBatch`` as ``inputs["data"]``; what it
writes into the plan is bit for bit what the existing path writes from the same samples."""
import numpy as np
import torch

from .. import _lib
from .._lib import AffineDesc, ImageDesc
from .centernet_transforms import (BrightnessTransform, CenterAffine, ContrastTransform, Lighting, SaturationTransform,
                                   invert_affine)
from .transforms import Compose, RandomHorizontalFlip, ShortestEdgeResize, TestTimeCompose, ToMode

__all__ = ["RawImageBatch", "AffineImageBatch", "RawBatchCollator", "CenterNetRawCollator"]


class RawImageBatch:
    """packed: uint8 host tensor (pinned where a device exists) holding image i as C-contiguous [src_h][src_w][3] at descs[i].offset;
    descs: one _lib.ImageDesc per image; Hmax / Wmax: the largest resized height / width of the batch."""

    def __init__(self, packed, descs, Hmax, Wmax, owner=None):
        self.packed, self.descs, self.N, self.Hmax, self.Wmax = packed, list(descs), len(descs), int(Hmax), int(Wmax)
        self._owner = owner

    def copied(self, event):
        """The consumer enqueued its copy of ``packed``; ``event`` fires once it has drained (the collator then reuses the buffer)."""
        if self._owner is not None:
            self._owner._pending = event


class AffineImageBatch(RawImageBatch):
    """A RawImageBatch whose descs are _lib.AffineDesc records (bd_affine_jitter_normalize): every image comes out Hmax x Wmax."""


class _Shape:
    """What the transforms' _get_params read of an image: its shape (the pixels stay where they are)."""
    __slots__ = ("shape",)

    def __init__(self, h, w):
        self.shape = (int(h), int(w), 3)


class _PackedOwner:
    """The grow-only pinned buffer of a raw collator and the handshake that guards it (RawImageBatch.copied)."""
    _buf = None                  # grow-only packed buffer
    _pending = None              # event of the previous batch's copy

    def _packed(self, nbytes):
        if self._pending is not None:        # the previous batch's copy still reads the buffer
            self._pending.synchronize()
            self._pending = None
        if self._buf is None or self._buf.numel() < nbytes:
            self._buf = torch.empty((nbytes,), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        return self._buf[:nbytes]


class RawBatchCollator(_PackedOwner):
    """transform: the Compose / TestTimeCompose of build_transform.  One batch is in flight per collator: ``apply`` waits for the previous
    batch's copy (RawImageBatch.copied) before it overwrites the packed buffer."""

    def __init__(self, transform, pad_value: float = 0.0):
        if not isinstance(transform, Compose):
            raise ValueError(f"RawBatchCollator needs a Compose / TestTimeCompose, got {type(transform).__name__}")
        if pad_value != 0.0:
            raise ValueError("RawBatchCollator pads images on the device with 0 before normalising: pad_value must be 0")
        seen_resize = seen_flip = False
        for t in transform.transforms:
            # exact types: a subclass may redefine what happens to the pixels, and the device would silently not do it
            if type(t) not in (ShortestEdgeResize, RandomHorizontalFlip, ToMode):
                raise ValueError(f"RawBatchCollator cannot run {type(t).__name__} on the device (ShortestEdgeResize, RandomHorizontalFlip, "
                                 "ToMode only)")
            if type(t) is ShortestEdgeResize:
                if seen_resize or seen_flip:      # the kernel resizes once, then flips: another order rounds differently
                    raise ValueError("RawBatchCollator needs at most one ShortestEdgeResize, before any RandomHorizontalFlip")
                seen_resize = True
            seen_flip = seen_flip or type(t) is RandomHorizontalFlip
        self.transform, self.pad_value = transform, pad_value
        self.test_mode = isinstance(transform, TestTimeCompose)

    def _params(self, image, boxes):
        """One sample through the transform list without touching a pixel: (dst_h, dst_w, flip, boxes)."""
        h, w = image.shape[:2]
        flip = False
        for t in self.transform.transforms:
            if type(t) is ShortestEdgeResize:
                if not self.test_mode or t._shape_info is None or t._shape_info[:2] != (h, w):      # (TestTimeCompose: _apply_image's rule)
                    t._get_params(_Shape(h, w))
                h, w = t._shape_info[2:]
            elif type(t) is RandomHorizontalFlip:
                if not self.test_mode:           # (an image-only apply never draws: it flips by the transform's standing state)
                    t._get_params(_Shape(h, w))
                flip ^= t._flip
            if boxes is not None:
                boxes = t._apply_boxes(boxes)
        return h, w, flip, boxes

    def apply(self, samples):
        """samples: (image HWC uint8, boxes (n, 4), boxes_category (n,), info with info[0:2] = original (H, W)) per image; bare images
        under a TestTimeCompose."""
        rows, nbytes = [], 0
        for s in samples:
            image, boxes, category, info = (s, None, (), None) if self.test_mode else s
            image = np.asarray(image)
            if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or image.size == 0:
                raise ValueError(f"RawBatchCollator needs uint8 (H, W, 3) images, got {image.dtype} {image.shape}")
            dh, dw, flip, boxes = self._params(image, boxes)
            boxes = np.zeros((0, 4), np.float32) if boxes is None else np.asarray(boxes, np.float32).reshape(-1, 4)
            category = np.asarray(category, np.float32).reshape(-1)
            assert len(boxes) == len(category)
            orig = image.shape[:2] if info is None else (info[0], info[1])
            rows.append((image, nbytes, dh, dw, flip, boxes, category, orig))
            nbytes += image.size
        n = len(rows)
        packed = self._packed(nbytes)
        flat = packed.numpy()
        gmax = max((len(r[5]) for r in rows), default=0)
        gt_boxes = np.full((n, gmax, 5), self.pad_value, np.float32)
        im_info = np.empty((n, 5), np.float32)
        descs = []
        for i, (image, off, dh, dw, flip, boxes, category, orig) in enumerate(rows):
            sh, sw = image.shape[:2]
            np.copyto(flat[off:off + image.size].reshape(sh, sw, 3), image)
            descs.append(ImageDesc(offset=off, src_h=sh, src_w=sw, dst_h=dh, dst_w=dw, flip=int(flip)))
            g = len(boxes)
            gt_boxes[i, :g, :4] = boxes
            gt_boxes[i, :g, 4] = category
            im_info[i] = (dh, dw, orig[0], orig[1], g)
        hmax = max((d.dst_h for d in descs), default=0)
        wmax = max((d.dst_w for d in descs), default=0)
        return {"data": RawImageBatch(packed, descs, hmax, wmax, owner=self), "gt_boxes": gt_boxes, "im_info": im_info}

    __call__ = apply


class CenterNetRawCollator(_PackedOwner):
    """The pipeline of CenterNetConfig.AUG.TRAIN_VALUE over raw images: spec_or_transforms is that (name, kwargs) list (every transform
    then draws from `rng`) or a list of transform objects.  The order is the one the device runs: CenterAffine, RandomHorizontalFlip
    (optional), then any of Brightness -> Contrast -> Saturation -> Lighting in that order, then ToMode("CHW").  Parameters are drawn
    per sample through the transforms' own _get_params, boxes move on the host, boxes left without width or height are dropped
    (models/det/centernet.py:93 filter_by_size), and the pixels wait for bd_affine_jitter_normalize (FPNDetector.pre_process)."""
    _BY_NAME = {"CenterAffine": CenterAffine, "MGE_RandomHorizontalFlip": RandomHorizontalFlip, "RandomHorizontalFlip": RandomHorizontalFlip,
                "MGE_BrightnessTransform": BrightnessTransform, "MGE_ContrastTransform": ContrastTransform,
                "MGE_SaturationTransform": SaturationTransform, "MGE_Lighting": Lighting, "MGE_ToMode": ToMode, "ToMode": ToMode}
    _ORDER = (CenterAffine, RandomHorizontalFlip, BrightnessTransform, ContrastTransform, SaturationTransform, Lighting, ToMode)

    def __init__(self, spec_or_transforms, rng=None):
        ts = []
        for item in spec_or_transforms:
            if isinstance(item, (tuple, list)):
                name, kw = item
                if name not in self._BY_NAME:
                    raise ValueError(f"CenterNetRawCollator: the transform {name!r} is unknown; built: {sorted(self._BY_NAME)}")
                cls = self._BY_NAME[name]
                item = cls(**kw) if cls is ToMode else cls(**kw, rng=rng)
            ts.append(item)
        last = -1
        for t in ts:
            # exact types: a subclass may redefine what happens to the pixels, and the device would silently not do it
            if type(t) not in self._ORDER:
                raise ValueError(f"CenterNetRawCollator cannot run {type(t).__name__} on the device "
                                 f"({', '.join(c.__name__ for c in self._ORDER)} only)")
            rank = self._ORDER.index(type(t))
            if rank <= last or (last < 0 and rank != 0):
                raise ValueError(f"CenterNetRawCollator: {type(t).__name__} is out of order or repeated: the device runs "
                                 f"{' -> '.join(c.__name__ for c in self._ORDER)}, each at most once, CenterAffine first")
            last = rank
        if not ts or type(ts[-1]) is not ToMode or ts[-1].mode != "CHW":
            raise ValueError('CenterNetRawCollator: the pipeline ends with ToMode("CHW")')
        self.affine = ts[0]
        if not self.affine.random_aug:
            raise NotImplementedError("Non-random augmentation not implemented")
        w, h = self.affine.output_size
        if w <= 0 or h <= 0 or w % 32 or h % 32:
            raise ValueError(f"CenterNetRawCollator: CenterAffine's output_size {(w, h)} must be positive multiples of 32")
        self.transforms = ts

    def _params(self, image, boxes):
        """One sample through the transform list without touching a pixel: (AffineDesc without its offset, boxes)."""
        w, h = self.affine.output_size
        d = AffineDesc(src_h=image.shape[0], src_w=image.shape[1], alpha_brightness=1.0, alpha_contrast=1.0, alpha_saturation=1.0)
        for t in self.transforms:
            t._get_params(_Shape(*image.shape[:2]) if type(t) is CenterAffine else _Shape(h, w))
            if type(t) is CenterAffine:
                d.inv[:] = invert_affine(t.affine).reshape(6).tolist()
            elif type(t) is RandomHorizontalFlip:
                d.flip = int(t._flip)
            elif type(t) is BrightnessTransform and t.value != 0:
                d.stages, d.alpha_brightness = d.stages | _lib.AFFINE_BRIGHTNESS, t._alpha
            elif type(t) is ContrastTransform and t.value != 0:
                d.stages, d.alpha_contrast = d.stages | _lib.AFFINE_CONTRAST, t._alpha
            elif type(t) is SaturationTransform and t.value != 0:
                d.stages, d.alpha_saturation = d.stages | _lib.AFFINE_SATURATION, t._alpha
            elif type(t) is Lighting and t.scale != 0:
                d.stages = d.stages | _lib.AFFINE_LIGHTING
                d.delta[:] = t._delta.tolist()
            boxes = t._apply_boxes(boxes)
        return d, boxes

    def apply(self, samples):
        """samples: (image HWC uint8, boxes (n, 4), boxes_category (n,), info with info[0:2] = original (H, W)) per image."""
        w, h = self.affine.output_size
        rows, nbytes = [], 0
        for image, boxes, category, info in samples:
            image = np.asarray(image)
            if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or image.size == 0:
                raise ValueError(f"CenterNetRawCollator needs uint8 (H, W, 3) images, got {image.dtype} {image.shape}")
            boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
            category = np.asarray(category, np.float32).reshape(-1)
            assert len(boxes) == len(category)
            d, boxes = self._params(image, boxes)
            keep = (boxes[:, 2] - boxes[:, 0] > 0) & (boxes[:, 3] - boxes[:, 1] > 0)
            d.offset = nbytes
            orig = image.shape[:2] if info is None else (info[0], info[1])
            rows.append((image, d, boxes[keep], category[keep], orig))
            nbytes += image.size
        n = len(rows)
        flat = (packed := self._packed(nbytes)).numpy()
        gmax = max((len(r[2]) for r in rows), default=0)
        gt_boxes = np.zeros((n, gmax, 5), np.float32)
        im_info = np.empty((n, 5), np.float32)
        for i, (image, d, boxes, category, orig) in enumerate(rows):
            np.copyto(flat[d.offset:d.offset + image.size].reshape(image.shape), image)
            g = len(boxes)
            gt_boxes[i, :g, :4] = boxes
            gt_boxes[i, :g, 4] = category
            im_info[i] = (h, w, orig[0], orig[1], g)
        return {"data": AffineImageBatch(packed, [r[1] for r in rows], h, w, owner=self), "gt_boxes": gt_boxes, "im_info": im_info}

    __call__ = apply
