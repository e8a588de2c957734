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

from .._lib import ImageDesc
from .transforms import Compose, RandomHorizontalFlip, ShortestEdgeResize, TestTimeCompose, ToMode

__all__ = ["RawImageBatch", "RawBatchCollator"]


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


class _Shape:
    """What the transforms' _get_params read of an image: its shape (the pixels stay where they are)."""
    __slots__ = ("shape",)

    def __init__(self, h, w):
        self.shape = (int(h), int(w), 3)


class RawBatchCollator:
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
        self._buf = None             # grow-only packed buffer
        self._pending = None         # event of the previous batch's copy

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

    def _packed(self, nbytes):
        if self._pending is not None:        # the previous batch's copy still reads the buffer
            self._pending.synchronize()
            self._pending = None
        if self._buf is None or self._buf.numel() < nbytes:
            self._buf = torch.empty((nbytes,), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        return self._buf[:nbytes]
