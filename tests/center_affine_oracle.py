"""The arithmetic of CenterNet's training input, stated once in numpy: CenterAffine's warp, horizontal flip, brightness, contrast,
saturation, lighting, normalisation (CenterNetConfig.AUG.TRAIN_VALUE).  bd_affine_jitter_normalize must reproduce `pipeline` bit for bit.

This is a restatement of published behaviour, not a recording: cv2 and MegEngine are not installed where this project is built, so
parity with a real cv2.warpAffine / megengine.data.transform is UNPINNED.  Two choices below are definitions of this project:

  * the bilinear weight table.  cv2 builds a 32 x 32 table of float weights (1 - fy / 32, fy / 32) x (1 - fx / 32, fx / 32), scales by
    32768, rounds to int16 and, where the four do not sum to 32768, adds the residue to the largest.  With 1/32 fractions every product
    is the exact integer 32 a b (a + a' = 32), so the four always sum to 32768 and there is no residue to place; the one weight that
    does not fit int16 (32768, at fx = fy = 0) is what "32767 plus the residue 1" gives in a wider integer.  The rule here: weights are
    those exact integers, held in int32 (`weights` asserts the sum).  An identity map therefore reproduces the image.
  * integer promotion in the colour stages.  Every stage here reads bytes and writes bytes: fp32 arithmetic of one IEEE operation per
    step in the order written, clip to [0, 255], truncate.  The contrast mean comes from exact integer channel sums, combined in float64
    and rounded once to fp32 (a sum in any order gives the same integers).

Images are (H, W, 3) uint8 in the channel order of the model's mean / std (BGR); maps are float64 (2, 3)."""
import numpy as np

AB_BITS, INTER_BITS = 10, 5
GREY = (np.float32(0.114), np.float32(0.587), np.float32(0.299))
EIGVAL = np.array([0.2175, 0.0188, 0.0045])
EIGVEC = np.array([[-0.5836, -0.6948, 0.4203], [-0.5808, -0.0045, -0.8140], [-0.5675, 0.7192, 0.4009]])
BRIGHTNESS, CONTRAST, SATURATION, LIGHTING = 1, 2, 4, 8


# ---- parameters -------------------------------------------------------------------------------------------------------------------------
def get_border(border, size):
    i = 1
    size //= 2
    while size <= border // i:
        i *= 2
    return border // i


def src_and_dst(center, side, output_size):
    """The three point pairs of CenterAffine (float32 (3, 2) each): the square's centre, the point half a side above it, that point moved
    half a side to the left; output_size = (width, height)."""
    def pts(c, width):
        p = np.zeros((3, 2), np.float32)
        p[0] = c
        p[1] = p[0] + np.array([0, width * -0.5])
        p[2] = p[1] + np.array([width * -0.5, 0])
        return p
    dw, dh = output_size
    return pts(center, side), pts((dw * 0.5, dh * 0.5), dw)


def forward_matrix(center, side, output_size):
    """cv2.getAffineTransform(src, dst): the float64 solve of the three pairs."""
    src, dst = src_and_dst(center, side, output_size)
    a = np.column_stack((src.astype(np.float64), np.ones(3)))
    return np.linalg.solve(a, dst.astype(np.float64)).T


def invert(m):
    """cv2.warpAffine's inversion, operation by operation."""
    m = np.asarray(m, np.float64)
    d = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m[1, 1] * d, m[0, 0] * d
    a12, a21 = m[0, 1] * -d, m[1, 0] * -d
    return np.array([[a11, a12, -a11 * m[0, 2] - a12 * m[1, 2]], [a21, a22, -a21 * m[0, 2] - a22 * m[1, 2]]], np.float64)


def lighting_delta(alpha_std):
    return (EIGVEC @ (np.asarray(alpha_std, np.float64) * EIGVAL)).astype(np.float32)


# ---- boxes ------------------------------------------------------------------------------------------------------------------------------
def warp_boxes(boxes, m, output_size):
    """Four corners -> map -> clip x to [0, w - 1], y to [0, h - 1] -> min / max; float64."""
    w, h = output_size
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    out = np.empty_like(b)
    for i, (x1, y1, x2, y2) in enumerate(b):
        c = np.array([[x1, y1, 1.0], [x2, y1, 1.0], [x1, y2, 1.0], [x2, y2, 1.0]]) @ np.asarray(m, np.float64).T
        c[:, 0] = np.clip(c[:, 0], 0, w - 1)
        c[:, 1] = np.clip(c[:, 1], 0, h - 1)
        out[i] = (*c.min(0), *c.max(0))
    return out


def flip_boxes(boxes, width):
    b = np.asarray(boxes).copy()
    b[:, 0], b[:, 2] = width - boxes[:, 2], width - boxes[:, 0]
    return b


def keep_boxes(boxes):
    """filter_by_size(sizes=0): width and height both above zero."""
    return (boxes[:, 2] - boxes[:, 0] > 0) & (boxes[:, 3] - boxes[:, 1] > 0)


# ---- pixels -----------------------------------------------------------------------------------------------------------------------------
def weights(ax, ay):
    """The four bilinear weights (w00, w01, w10, w11) of the 1/32 fractions ax, ay (int64 arrays): exact integers, sum 32768."""
    n = 1 << INTER_BITS
    w = ((n - ax) * (n - ay) * 32, ax * (n - ay) * 32, (n - ax) * ay * 32, ax * ay * 32)
    assert np.all(w[0] + w[1] + w[2] + w[3] == 1 << 15)
    return w


def warp_affine(img, inv, out_h, out_w):
    """cv2.warpAffine(img, M, (out_w, out_h), INTER_LINEAR), constant border 0, from inv = invert(M)."""
    inv = np.asarray(inv, np.float64)
    h, w = img.shape[:2]
    xs, ys = np.arange(out_w, dtype=np.float64), np.arange(out_h, dtype=np.float64)
    delta = 1 << (AB_BITS - INTER_BITS - 1)
    adelta = np.rint(inv[0, 0] * xs * 1024.0).astype(np.int64)
    bdelta = np.rint(inv[1, 0] * xs * 1024.0).astype(np.int64)
    x0 = np.rint((inv[0, 1] * ys + inv[0, 2]) * 1024.0).astype(np.int64) + delta
    y0 = np.rint((inv[1, 1] * ys + inv[1, 2]) * 1024.0).astype(np.int64) + delta
    assert max(np.abs(adelta).max(), np.abs(bdelta).max()) <= 1 << 28 and max(np.abs(x0).max(), np.abs(y0).max()) <= (1 << 29) + delta
    X = (x0[:, None] + adelta[None, :]) >> (AB_BITS - INTER_BITS)
    Y = (y0[:, None] + bdelta[None, :]) >> (AB_BITS - INTER_BITS)
    sx, sy, ax, ay = X >> INTER_BITS, Y >> INTER_BITS, X & 31, Y & 31
    src = img.astype(np.int64)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(ok[..., None], src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0)
    w00, w01, w10, w11 = (v[..., None] for v in weights(ax, ay))
    acc = w00 * tap(sy, sx) + w01 * tap(sy, sx + 1) + w10 * tap(sy + 1, sx) + w11 * tap(sy + 1, sx + 1)
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def _byte(v):
    return np.clip(v, np.float32(0), np.float32(255)).astype(np.uint8)          # clip, then truncate


def flip(img):
    return img[:, ::-1].copy()


def brightness(img, alpha):
    return _byte(img.astype(np.float32) * np.float32(alpha))


def grey_mean(img):
    """The fp32 mean grey level of contrast: exact channel sums, float64 combination, one rounding."""
    s = img.reshape(-1, 3).astype(np.int64).sum(0)
    g = np.float64(GREY[0]) * np.float64(s[0]) + np.float64(GREY[1]) * np.float64(s[1]) + np.float64(GREY[2]) * np.float64(s[2])
    return np.float32(g / (np.float64(img.shape[0]) * np.float64(img.shape[1])))


def contrast(img, alpha):
    a = np.float32(alpha)
    t = grey_mean(img) * (np.float32(1) - a)
    return _byte(img.astype(np.float32) * a + t)


def saturation(img, alpha):
    a = np.float32(alpha)
    f = img.astype(np.float32)
    grey = GREY[0] * f[..., 0] + GREY[1] * f[..., 1] + GREY[2] * f[..., 2]
    t = grey * (np.float32(1) - a)
    return _byte(f * a + t[..., None])


def lighting(img, delta):
    return _byte(img.astype(np.float32) + np.asarray(delta, np.float32).reshape(1, 1, 3))


def to_gray(img):
    """float64 grey image with the textbook coefficients (what grey_mean is compared with)."""
    f = img.astype(np.float64)
    return 0.114 * f[..., 0] + 0.587 * f[..., 1] + 0.299 * f[..., 2]


def pipeline(img, inv, out_h, out_w, flipped=False, stages=0, alpha_brightness=1.0, alpha_contrast=1.0, alpha_saturation=1.0,
             delta=(0.0, 0.0, 0.0)):
    """The bytes bd_affine_jitter_normalize writes to u8_out for one image."""
    out = warp_affine(img, inv, out_h, out_w)
    if flipped:
        out = flip(out)
    if stages & BRIGHTNESS:
        out = brightness(out, alpha_brightness)
    if stages & CONTRAST:
        out = contrast(out, alpha_contrast)
    if stages & SATURATION:
        out = saturation(out, alpha_saturation)
    if stages & LIGHTING:
        out = lighting(out, delta)
    return out


def pipeline_of_desc(img, d, out_h, out_w):
    """pipeline() from a bd_affine_desc-like record (basedet_amd._lib.AffineDesc)."""
    return pipeline(img, np.array(list(d.inv), np.float64).reshape(2, 3), out_h, out_w, bool(d.flip), int(d.stages), d.alpha_brightness,
                    d.alpha_contrast, d.alpha_saturation, tuple(d.delta))


def to_batch(images):
    """[(H, W, 3) uint8] of one size -> the float32 (N, 3, H, W) batch of the float input path."""
    return np.ascontiguousarray(np.stack(images).transpose(0, 3, 1, 2), dtype=np.float32)
