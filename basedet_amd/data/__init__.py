"""Host side of the batch contract next to the hot path (basedet/data/collators/pad_collator.py, data/samplers/group_sampler.py).

Pure numpy, no MegEngine: the reference subclasses ``megengine.data.Collator`` / ``RandomSampler`` only for their interfaces.
What the training step consumes is the dict produced by ``DetectionPadCollator.apply`` -- ``data`` (N,3,H,W) float32,
``gt_boxes`` (N,G,5) float32, ``im_info`` (N,5) float32 -- which ``FPNDetector.pre_process`` then pads to a multiple of 32 and
normalises on the device (bd_pad_normalize).  ``RawBatchCollator`` is the second way in: the raw uint8 images go to the device and
bd_resize_pad_normalize does the transform's pixel work there (data/raw.py).  ``CenterNetRawCollator`` is CenterNet's: the pipeline
of ``CenterNetConfig.AUG.TRAIN_VALUE`` (data/centernet_transforms.py draws its parameters), its pixels in bd_affine_jitter_normalize."""
from .centernet_transforms import (BrightnessTransform, CenterAffine, ContrastTransform, Lighting,  # noqa: F401
                                   SaturationTransform)
from .collators import DetectionPadCollator, calculate_padding_shape  # noqa: F401
from .raw import AffineImageBatch, CenterNetRawCollator, RawBatchCollator, RawImageBatch  # noqa: F401
from .samplers import AspectRatioGroupSampler, GroupedRandomSampler  # noqa: F401
from .transforms import (Compose, RandomHorizontalFlip, ShortestEdgeResize, TestTimeCompose, ToMode,  # noqa: F401
                         build_transform)
