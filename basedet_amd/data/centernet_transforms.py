"""CenterNet's training augmentations (`data/transforms/centernet_transform.py:14-96` CenterAffine; megengine's BrightnessTransform,
ContrastTransform, SaturationTransform and Lighting, which `CenterNetConfig.AUG.TRAIN_VALUE` names): the HOST half.

These classes draw what the reference draws, in the reference's order, and move the boxes.  They do not touch a pixel: the warp and
the colour passes run on the device, in bd_affine_jitter_normalize, from the parameters drawn here (data/raw.py
CenterNetRawCollator builds one descriptor per image from them).  Calling one of them on an image raises."""
import numpy as np

from .transforms import _Transform

__all__ = ["CenterAffine", "BrightnessTransform", "ContrastTransform", "SaturationTransform", "Lighting", "invert_affine"]


def _no_pixels(self, image):
    raise NotImplementedError(f"{type(self).__name__} has no host pixel path: its pixels run on the device "
                              "(basedet.data.CenterNetRawCollator)")


def invert_affine(m):
    """cv2.warpAffine's inversion of a float64 (2, 3) map, operation by operation (a singular map gives zeros)."""
    m = np.asarray(m, np.float64)
    d = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m[1, 1] * d, m[0, 0] * d
    out = np.empty((2, 3), np.float64)
    out[0, 0], out[0, 1], out[1, 0], out[1, 1] = a11, m[0, 1] * -d, m[1, 0] * -d, a22
    out[0, 2] = -out[0, 0] * m[0, 2] - out[0, 1] * m[1, 2]
    out[1, 2] = -out[1, 0] * m[0, 2] - out[1, 1] * m[1, 2]
    return out


class CenterAffine(_Transform):
    """A random square of the image (side = the longer edge x one of np.arange(0.6, 1.4, 0.1), centre drawn inside the borders) mapped onto
    output_size = (width, height).  After _get_params: `affine`, the float64 (2, 3) forward map (cv2.getAffineTransform of the three
    point pairs), `center` and `scale`."""

    def __init__(self, border=128, output_size=(512, 512), random_aug=True, rng=None):
        self.border, self.output_size, self.random_aug = border, tuple(int(v) for v in output_size), random_aug
        self.rng = rng if rng is not None else np.random.default_rng()
        self.affine = self.center = self.scale = None

    @staticmethod
    def _get_border(border, size):
        i = 1
        size //= 2
        while size <= border // i:
            i *= 2
        return border // i

    def generate_center_and_scale(self, img_shape):
        height, width = img_shape
        center = np.array([width / 2, height / 2], dtype=np.float32)
        scale = float(max(img_shape))
        if not self.random_aug:
            raise NotImplementedError("Non-random augmentation not implemented")
        scale = scale * self.rng.choice(np.arange(0.6, 1.4, 0.1))
        h_border = self._get_border(self.border, height)
        w_border = self._get_border(self.border, width)
        center[0] = self.rng.integers(w_border, width - w_border)
        center[1] = self.rng.integers(h_border, height - h_border)
        return center, scale

    @staticmethod
    def forward_matrix(center, scale, output_size):
        """cv2.getAffineTransform(src, dst) of the three float32 point pairs, solved in float64."""
        from ..models.centernet import CenterNetDecoder           # (models imports data: not at module level)
        src, dst = CenterNetDecoder.generate_src_and_dst(center, scale, output_size)
        a = np.column_stack((np.float32(src).astype(np.float64), np.ones(3)))
        return np.linalg.solve(a, np.float32(dst).astype(np.float64)).T

    def _get_params(self, image):
        self.center, self.scale = self.generate_center_and_scale(image.shape[:2])
        self.affine = self.forward_matrix(self.center, self.scale, self.output_size)

    _apply_image = _no_pixels

    def _apply_coords(self, coords):
        w, h = self.output_size
        coords = np.column_stack((coords, np.ones(coords.shape[0]))) @ self.affine.T
        coords[..., 0] = np.clip(coords[..., 0], 0, w - 1)
        coords[..., 1] = np.clip(coords[..., 1], 0, h - 1)
        return coords

    def _apply_boxes(self, boxes):
        """Four corners -> map -> clip -> min / max (megengine VisionTransform._apply_boxes); float64 inside, float32 out."""
        b = np.asarray(boxes).reshape(-1, 4)
        corners = self._apply_coords(b[:, [0, 1, 2, 1, 0, 3, 2, 3]].reshape(-1, 2)).reshape(-1, 4, 2)
        return np.concatenate((corners.min(axis=1), corners.max(axis=1)), axis=1).astype(np.float32)


class _Jitter(_Transform):
    """alpha = uniform(max(0, 1 - value), 1 + value); value 0 draws nothing and is the identity."""

    def __init__(self, value, rng=None):
        if value < 0:
            raise ValueError(f"{type(self).__name__}: value must not be negative, got {value}")
        self.value = value
        self.rng = rng if rng is not None else np.random.default_rng()
        self._alpha = 1.0

    def _get_params(self, image):
        if self.value != 0:
            self._alpha = float(self.rng.uniform(max(0, 1 - self.value), 1 + self.value))

    _apply_image = _no_pixels


class BrightnessTransform(_Jitter):
    pass


class ContrastTransform(_Jitter):
    pass


class SaturationTransform(_Jitter):
    pass


class Lighting(_Transform):
    """AlexNet-style PCA noise: delta = eigvec @ (normal(0, scale, 3) * eigval), one value per channel of a BGR image, float64 rounded to
    three float32; scale 0 draws nothing and is the identity."""
    EIGVAL = np.array([0.2175, 0.0188, 0.0045])
    EIGVEC = np.array([[-0.5836, -0.6948, 0.4203], [-0.5808, -0.0045, -0.8140], [-0.5675, 0.7192, 0.4009]])

    def __init__(self, scale, rng=None):
        if scale < 0:
            raise ValueError(f"Lighting: scale must not be negative, got {scale}")
        self.scale = scale
        self.rng = rng if rng is not None else np.random.default_rng()
        self._delta = np.zeros(3, np.float32)

    @classmethod
    def delta_of(cls, alpha_std):
        return (cls.EIGVEC @ (np.asarray(alpha_std, np.float64) * cls.EIGVAL)).astype(np.float32)

    def _get_params(self, image):
        if self.scale != 0:
            self._delta = self.delta_of(self.rng.normal(0, self.scale, 3))

    _apply_image = _no_pixels
