from .retinanet import RetinaNet  # noqa: F401
from .free_anchor import FreeAnchor  # noqa: F401
from .fcos import ATSS, FCOS, OTA  # noqa: F401
from .faster_rcnn import FasterRCNN  # noqa: F401
from . import centernet  # noqa: F401
from .centernet import CenterNet, CenterNetDecoder, CenterNetGT  # noqa: F401
from . import yolox  # noqa: F401
from .yolox import YOLOX, yolox_assignments, yolox_inference, yolox_losses  # noqa: F401
