"""Host half of CenterNet's training input: the parameters CenterNetRawCollator draws, its matrices, boxes and refusals, the numpy
oracle's own properties (tests/center_affine_oracle.py), and the C ABI of bd_affine_jitter_normalize.  Imports of the package happen
inside the tests."""
import os
import re

import numpy as np
import pytest

from tests import center_affine_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bd_affine_jitter_workspace_bytes", "bd_affine_jitter_normalize")
SPEC = (("CenterAffine", dict(border=128, output_size=(512, 512))), ("MGE_RandomHorizontalFlip", dict(prob=0.5)),
        ("MGE_BrightnessTransform", dict(value=0.4)), ("MGE_ContrastTransform", dict(value=0.4)),
        ("MGE_SaturationTransform", dict(value=0.4)), ("MGE_Lighting", dict(scale=0.1)), ("MGE_ToMode", dict(mode="CHW")))


def _image(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _restated_draws(rng, h, w, border=128, out=(512, 512), prob=0.5, v=0.4, scale=0.1):
    """The reference's sequence on one generator, straight line: scale, cx, cy, flip, brightness, contrast, saturation, lighting(3)."""
    side = float(max(h, w)) * rng.choice(np.arange(0.6, 1.4, 0.1))
    wb, hb = O.get_border(border, w), O.get_border(border, h)
    center = np.array([w / 2, h / 2], np.float32)
    center[0] = rng.integers(wb, w - wb)
    center[1] = rng.integers(hb, h - hb)
    flip = bool(rng.random() < prob)
    ab = rng.uniform(max(0, 1 - v), 1 + v)
    ac = rng.uniform(max(0, 1 - v), 1 + v)
    asat = rng.uniform(max(0, 1 - v), 1 + v)
    delta = O.lighting_delta(rng.normal(0, scale, 3))
    return dict(center=center, side=side, flip=flip, ab=np.float32(ab), ac=np.float32(ac), asat=np.float32(asat), delta=delta,
                m=O.forward_matrix(center, side, out))


@pytest.mark.parametrize("seed", [0, 1, 7])
def test_collator_draws_equal_the_restated_sequence(seed):
    from basedet.data import CenterNetRawCollator
    from basedet_amd import _lib
    assert len(np.arange(0.6, 1.4, 0.1)) in (8, 9)          # (whatever numpy gives is what both sides draw from)
    sizes = [(20, 30), (480, 640), (37, 53)]
    img_rng = np.random.default_rng(100)
    samples = [(_image(img_rng, h, w), np.zeros((0, 4), np.float32), [], (h, w)) for h, w in sizes]
    batch = CenterNetRawCollator(SPEC, np.random.default_rng(seed))(samples)
    rng = np.random.default_rng(seed)
    data = batch["data"]
    assert (data.N, data.Hmax, data.Wmax) == (3, 512, 512)
    off = 0
    for d, (h, w) in zip(data.descs, sizes):
        want = _restated_draws(rng, h, w)
        assert (d.offset, d.src_h, d.src_w, d.flip) == (off, h, w, int(want["flip"]))
        assert d.stages == _lib.AFFINE_BRIGHTNESS | _lib.AFFINE_CONTRAST | _lib.AFFINE_SATURATION | _lib.AFFINE_LIGHTING
        assert np.array_equal(np.array(list(d.inv)).reshape(2, 3), O.invert(want["m"]))
        assert (np.float32(d.alpha_brightness), np.float32(d.alpha_contrast), np.float32(d.alpha_saturation)) == \
            (want["ab"], want["ac"], want["asat"])
        assert np.array_equal(np.array(list(d.delta), np.float32), want["delta"])
        off += h * w * 3
    # every image's bytes are in the packed buffer at its offset
    for d, s in zip(data.descs, samples):
        assert np.array_equal(data.packed.numpy()[d.offset:d.offset + s[0].size].reshape(s[0].shape), s[0])
    assert np.array_equal(batch["im_info"], np.array([[512, 512, h, w, 0] for h, w in sizes], np.float32))


def test_get_border_halves_more_than_once_on_a_small_image():
    from basedet.data import CenterAffine
    assert CenterAffine._get_border(128, 20) == O.get_border(128, 20) == 8 and O.get_border(128, 30) == 8
    assert O.get_border(128, 480) == 128 and O.get_border(128, 256) == 64 and CenterAffine._get_border(128, 640) == 128


def test_a_zero_value_draws_nothing_and_disables_the_stage():
    from basedet.data import CenterNetRawCollator
    spec = (SPEC[0], ("MGE_BrightnessTransform", dict(value=0)), ("MGE_ContrastTransform", dict(value=0.4)), ("MGE_Lighting", dict(scale=0)),
            SPEC[-1])
    batch = CenterNetRawCollator(spec, np.random.default_rng(3))([(_image(np.random.default_rng(0), 40, 50), np.zeros((0, 4)), [], None)])
    rng = np.random.default_rng(3)
    rng.choice(np.arange(0.6, 1.4, 0.1)), rng.integers(8, 42), rng.integers(8, 32)
    d = batch["data"].descs[0]
    assert d.stages == 2 and d.flip == 0 and np.float32(d.alpha_contrast) == np.float32(rng.uniform(0.6, 1.4))
    assert d.alpha_brightness == 1.0 and list(d.delta) == [0.0, 0.0, 0.0]


def test_forward_matrix_is_the_solve_and_the_decoder_matrix_its_inverse():
    from basedet.data import CenterAffine
    from basedet_amd.data.centernet_transforms import invert_affine
    from basedet_amd.models.centernet import CenterNetDecoder
    rng = np.random.default_rng(5)
    for out in ((512, 512), (64, 96)):
        for _ in range(5):
            center = np.array([rng.integers(10, 600), rng.integers(10, 400)], np.float32)
            side = float(rng.uniform(20, 900))
            m = CenterAffine.forward_matrix(center, side, out)
            src, dst = O.src_and_dst(center, side, out)
            assert m.dtype == np.float64 and np.array_equal(m, O.forward_matrix(center, side, out))
            assert np.allclose(np.column_stack((src.astype(np.float64), np.ones(3))) @ m.T, dst, rtol=0, atol=1e-9)
            back = CenterNetDecoder.affine_matrix(center, side, out)
            full = lambda a: np.vstack((a, [0, 0, 1]))
            assert np.abs(full(m) @ full(back) - np.eye(3)).max() < 1e-9
            assert np.array_equal(invert_affine(m), O.invert(m)) and np.abs(invert_affine(m) - back).max() < 1e-9


def test_boxes_warp_clip_flip_and_drop():
    from basedet.data import CenterNetRawCollator
    img_rng = np.random.default_rng(9)
    boxes = np.array([[100, 120, 300, 360], [0, 0, 639, 479], [5, 5, 6, 6], [250.5, 200.25, 260, 210]], np.float32)
    far = np.array([[-5000, -5000, -4000, -4500]], np.float32)            # lands wholly outside: clipped to zero size
    samples = [(_image(img_rng, 480, 640), np.concatenate((boxes, far)), [1, 2, 3, 4, 5], (480, 640)),
               (_image(img_rng, 37, 53), far, [7], (37, 53))]
    for seed in range(6):                                                     # both flip states occur
        batch = CenterNetRawCollator(SPEC, np.random.default_rng(seed))(samples)
        rng = np.random.default_rng(seed)
        gmax = 0
        for i, (img, b, cat, _) in enumerate(samples):
            p = _restated_draws(rng, *img.shape[:2])
            want = O.warp_boxes(b, p["m"], (512, 512)).astype(np.float32)
            if p["flip"]:
                want = O.flip_boxes(want, 512)
            keep = O.keep_boxes(want)
            assert not keep[-1]
            g = int(keep.sum())
            gmax = max(gmax, g)
            assert batch["im_info"][i, 4] == g
            assert np.array_equal(batch["gt_boxes"][i, :g, :4], want[keep])
            assert np.array_equal(batch["gt_boxes"][i, :g, 4], np.asarray(cat, np.float32)[keep])
            assert np.all(batch["gt_boxes"][i, g:] == 0)
        assert batch["gt_boxes"].shape == (2, gmax, 5) and batch["im_info"][1, 4] == 0
    empty = CenterNetRawCollator(SPEC, np.random.default_rng(0))([samples[1], samples[1]])
    assert empty["gt_boxes"].shape == (2, 0, 5) and np.all(empty["im_info"][:, 4] == 0)


def test_collator_refusals():
    from basedet.data import BrightnessTransform, CenterAffine, CenterNetRawCollator, SaturationTransform, ToMode
    aff, flip, bri, con, sat, lig, mode = SPEC
    with pytest.raises(ValueError, match="ContrastTransform"):                 # saturation before contrast
        CenterNetRawCollator((aff, flip, bri, sat, con, lig, mode))
    with pytest.raises(ValueError, match="RandomHorizontalFlip"):              # flip before CenterAffine
        CenterNetRawCollator((flip, aff, bri, mode))
    with pytest.raises(ValueError, match="CenterAffine"):                      # a second CenterAffine
        CenterNetRawCollator((aff, flip, aff, mode))

    class Brighter(BrightnessTransform):
        pass
    with pytest.raises(ValueError, match="Brighter"):                          # a subclass
        CenterNetRawCollator([CenterAffine(), Brighter(0.4), ToMode("CHW")])
    with pytest.raises(ValueError, match="MGE_ShortestEdgeResize"):
        CenterNetRawCollator((aff, ("MGE_ShortestEdgeResize", dict(min_size=800, max_size=1333)), mode))
    with pytest.raises(ValueError, match="ToMode"):
        CenterNetRawCollator((aff, flip))
    with pytest.raises(ValueError, match="output_size"):
        CenterNetRawCollator((("CenterAffine", dict(output_size=(500, 512))), mode))
    with pytest.raises(NotImplementedError):
        CenterNetRawCollator((("CenterAffine", dict(random_aug=False)), mode))
    with pytest.raises(NotImplementedError):
        CenterAffine(random_aug=False)._get_params(np.zeros((40, 50, 3), np.uint8))
    # no host pixel path: the transforms refuse an image instead of handing it back unchanged
    for t in (CenterAffine(), BrightnessTransform(0.4), SaturationTransform(0.4)):
        with pytest.raises(NotImplementedError):
            t.apply(np.zeros((40, 50, 3), np.uint8))
    ok = CenterNetRawCollator([CenterAffine(), SaturationTransform(0.4), ToMode("CHW")])       # a subset in order is accepted
    assert len(ok.transforms) == 3


def test_build_transform_still_refuses_the_pipeline():
    from basedet.data import build_transform
    with pytest.raises(ValueError, match="CenterAffine"):
        build_transform(SPEC, mode="train")


# ---- the oracle's own properties --------------------------------------------------------------------------------------------------------
IDENTITY = np.array([[1.0, 0, 0], [0, 1.0, 0]])


def test_oracle_identity_map_reproduces_the_image():
    img = _image(np.random.default_rng(0), 33, 47)
    assert np.array_equal(O.warp_affine(img, O.invert(IDENTITY), 33, 47), img)
    big = O.warp_affine(img, O.invert(IDENTITY), 64, 64)                      # a larger canvas: the image, then zeros
    assert np.array_equal(big[:33, :47], img) and not big[33:].any() and not big[:, 47:].any()


def test_oracle_integer_translation_shifts_and_zero_fills():
    img = _image(np.random.default_rng(1), 40, 50)
    m = np.array([[1.0, 0, 7], [0, 1.0, -3]])                                 # output (x, y) = source (x - 7, y + 3)
    out = O.warp_affine(img, O.invert(m), 40, 50)
    assert np.array_equal(out[:37, 7:], img[3:, :43])
    assert not out[37:].any() and not out[:, :7].any()


def test_oracle_half_pixel_shift_averages_neighbours():
    img = _image(np.random.default_rng(2), 8, 9)
    out = O.warp_affine(img, np.array([[1.0, 0, 0.5], [0, 1.0, 0]]), 8, 8)
    want = (img[:, :-1].astype(np.int64) * 16384 + img[:, 1:].astype(np.int64) * 16384 + 16384) >> 15
    assert np.array_equal(out, want.astype(np.uint8))


def test_oracle_weights_are_exact_and_sum_to_32768():
    ax, ay = np.meshgrid(np.arange(32), np.arange(32))
    w = O.weights(ax, ay)
    fx, fy = ax.astype(np.float32) / 32, ay.astype(np.float32) / 32
    table = [((1 - fx) * (1 - fy)), (fx * (1 - fy)), ((1 - fx) * fy), (fx * fy)]           # cv2's float table
    for got, t in zip(w, table):
        assert np.array_equal(got, (t * np.float32(32768)).astype(np.int64))              # no rounding happens: no residue to place


def test_oracle_neutral_parameters_leave_the_bytes_unchanged():
    img = _image(np.random.default_rng(3), 31, 45)
    assert np.array_equal(O.brightness(img, 1.0), img)
    assert np.array_equal(O.contrast(img, 1.0), img)
    assert np.array_equal(O.saturation(img, 1.0), img)
    assert np.array_equal(O.lighting(img, (0.0, 0.0, 0.0)), img)
    every = O.BRIGHTNESS | O.CONTRAST | O.SATURATION | O.LIGHTING
    assert np.array_equal(O.pipeline(img, O.invert(IDENTITY), 31, 45, stages=every), img)
    assert np.array_equal(O.pipeline(img, O.invert(IDENTITY), 31, 45, flipped=True), img[:, ::-1])


def test_oracle_colour_stages_saturate():
    img = _image(np.random.default_rng(4), 16, 16)
    assert np.array_equal(O.lighting(img, (-300.0, 300.0, 0.0))[..., 0], np.zeros((16, 16), np.uint8))
    assert np.array_equal(O.lighting(img, (-300.0, 300.0, 0.0))[..., 1], np.full((16, 16), 255, np.uint8))
    assert np.array_equal(O.brightness(img, 1.4), np.minimum(np.trunc(img.astype(np.float32) * np.float32(1.4)), 255).astype(np.uint8))
    assert np.array_equal(O.contrast(img, 0.0), np.full_like(img, int(O.grey_mean(img))))


@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (512, 512)])
def test_oracle_contrast_mean_from_integer_sums(shape):
    """fp32 rounding of the three coefficients moves each by at most 2^-24 relative (6e-8 x 255 grey levels in total), the final
    rounding to fp32 by at most 2^-24 x 255 = 1.6e-5: 1e-4 grey levels bounds both."""
    for seed in range(4):
        img = _image(np.random.default_rng(seed), *shape)
        assert abs(float(O.grey_mean(img)) - O.to_gray(img).mean()) < 1e-4
    assert O.grey_mean(np.full((*shape, 3), 255, np.uint8)) == np.float32(255.0)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_bound_and_exported():
    import ctypes as C
    from basedet_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "basedet_hip.h")).read()
    build = open(os.path.join(ROOT, "basedet_amd", "build.py")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert '"image_affine.hip": ["-ffp-contract=off"]' in build
    assert _lib.ABI_VERSION == 118 and lib.bd_version() == 118               # one above the detector's 117
    assert C.sizeof(_lib.AffineDesc) == 96 and C.sizeof(_lib.AffineDesc) % 16 == 0
    assert _lib.AffineDesc.inv.offset == 16 and _lib.AffineDesc.flip.offset == 64 and _lib.AffineDesc.delta.offset == 84
    assert re.search(r"double inv\[6\];", header) and "BD_AFFINE_LIGHTING 8" in header
    assert hasattr(ops, "affine_jitter_normalize")
    # counters (3 x 8 bytes per image, rounded up to 256) + one dword per intermediate pixel
    assert lib.bd_affine_jitter_workspace_bytes(3, 64, 96) == 256 + 3 * 64 * 96 * 4
    assert lib.bd_affine_jitter_workspace_bytes(33, 32, 32) == 1024 + 33 * 32 * 32 * 4
    assert lib.bd_affine_jitter_workspace_bytes(0, 64, 96) == 0
