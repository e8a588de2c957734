"""CenterNet tail without a GPU: the numpy / float64 oracle (tests/centernet_oracle.py) against hand-computed cases, gradcheck of the two
loss oracles, the decode oracle's tie order, the Python wrappers' argument errors, and the new symbols in the header and the binding."""
import os
import re

import numpy as np
import pytest
import torch

import centernet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["bd_centernet_targets_workspace_bytes", "bd_centernet_targets", "bd_centernet_focal_fwd_bwd", "bd_centernet_l1_fwd_bwd",
           "bd_centernet_decode_workspace_bytes", "bd_centernet_decode"]


def _one(boxes_cells, K=2, H=8, W=10, T=6):
    b = np.asarray(boxes_cells, np.float32).reshape(1, -1, 5).copy()
    b[..., :4] *= 4
    return O.targets(b, np.asarray([b.shape[1]], np.int32), K, H, W, T, 0.25, 0.7)


def test_radius_zero_box():
    r = _one([[1.25, 1.25, 2.75, 2.75, 1]])
    assert 0 < r["radius"][0] < 1                       # 1.5 x 1.5 cells: r3 = 0.41
    m = r["score_map"][0, 0]
    assert m[2, 2] == 1 and (m != 0).sum() == 1 and r["num_pos"] == 1
    assert r["index"][0, 0] == 2 * 10 + 2 and r["reg_mask"][0, 0] == 1
    np.testing.assert_array_equal(r["reg"][0, 0], [0, 0])
    np.testing.assert_array_equal(r["wh"][0, 0], [1.5, 1.5])


@pytest.mark.parametrize("box,cell,rows,cols", [
    ([-2.5, 1.0, 3.5, 7.0], (4, 0), (3, 4, 5), (0, 1)),           # left
    ([6.5, 1.0, 12.5, 7.0], (4, 9), (3, 4, 5), (8, 9)),           # right
    ([2.0, -2.5, 8.0, 3.5], (0, 5), (0, 1), (4, 5, 6)),           # top
    ([2.0, 4.5, 8.0, 10.5], (7, 5), (6, 7), (4, 5, 6)),           # bottom
])
def test_window_clipped_at_an_edge(box, cell, rows, cols):
    r = _one([box + [1]])
    assert int(r["radius"][0]) == 1                     # 6 x 6 cells: radius 1.64, sigma = 0.5
    m = r["score_map"][0, 0]
    ys, xs = np.nonzero(m)
    assert sorted(set(ys)) == list(rows) and sorted(set(xs)) == list(cols)
    assert m[cell] == 1
    e2, e4 = np.float32(np.exp(-2.0)), np.float32(np.exp(-4.0))       # one step: exp(-1 / (2 * 0.25)); the diagonal: exp(-2 / 0.5)
    got = sorted(m[ys, xs].tolist())
    assert got == sorted([1.0] + [float(e2)] * 3 + [float(e4)] * 2)


def test_overlapping_discs_take_the_max():
    a, b = [1.0, 0.5, 5.0, 4.5, 1], [3.0, 0.5, 7.0, 4.5, 1]       # 4 x 4 cells, centres (3, 2) and (5, 2): radius 1
    r, ra, rb = _one([a, b]), _one([a]), _one([b])
    assert int(r["radius"][0]) == 1
    both = (ra["score_map"] > 0) & (rb["score_map"] > 0)
    assert both.sum() == 3                                            # the column x = 4
    np.testing.assert_array_equal(r["score_map"], np.maximum(ra["score_map"], rb["score_map"]))
    assert r["num_pos"] == 2


def test_two_boxes_in_one_cell_count_once():
    r = _one([[3.0, 2.0, 5.0, 4.0, 2], [3.25, 2.25, 5.25, 4.25, 2]])
    assert r["index"][0, 0] == r["index"][0, 1] == 3 * 10 + 4
    assert r["reg_mask"][0, :2].tolist() == [1, 1] and r["num_pos"] == 1
    np.testing.assert_array_equal(r["reg"][0, 1], [0.25, 0.25])


def test_zero_width_dropped_and_label_zero_kept():
    r = _one([[3, 1, 3, 4, 1], [1, 1, 4, 4, 0], [5, 5, 7, 7, 1]])
    assert r["reg_mask"][0].tolist() == [1, 1, 0, 0, 0, 0]            # the zero-width box took no slot
    np.testing.assert_array_equal(r["wh"][0, 0], [3, 3])              # label 0: slot kept ...
    assert r["index"][0, 0] == 2 * 10 + 2
    assert r["score_map"][0, :, :4, :4].sum() == 0                    # ... nothing drawn
    assert r["num_pos"] == 1 and r["score_map"][0, 0, 6, 6] == 1


def test_more_than_T_and_outside_centre():
    r = _one([[0, 0, 2, 2, 1]] * 3 + [[20, 1, 24, 3, 1]], T=2)
    assert r["reg_mask"][0].tolist() == [1, 1]
    r = _one([[20, 1, 24, 3, 1], [0, 0, 2, 2, 1]])
    assert r["reg_mask"][0, :2].tolist() == [0, 1] and r["index"][0, 0] == 0 and r["num_pos"] == 1


@pytest.mark.parametrize("shape", O.TARGET_SHAPES)
def test_shared_problems_do_not_rest_on_a_rounding(shape):
    """The GPU test compares radii exactly: none of its boxes has a radius within one float32 step of an integer."""
    gt, num = O.target_problem(*shape)
    r = O.targets(gt, num, *shape[1:], O.BOX_SCALE, O.MIN_OVERLAP)
    assert len(r["radius"]) >= 3 and O.radius_margin_ulps(r["radius"]).min() > 1


@pytest.mark.parametrize("with_pos", [True, False])
def test_focal_oracle_gradcheck(with_pos):
    g = torch.Generator().manual_seed(3)
    p = torch.rand(2, 3, 4, 5, generator=g, dtype=torch.float64) * 0.9 + 0.05
    gt = torch.rand(2, 3, 4, 5, generator=g, dtype=torch.float64) * 0.9
    if with_pos:
        gt[0, 1, 2, 3] = gt[1, 0, 0, 0] = 1.0
    assert torch.autograd.gradcheck(lambda q: O.focal_loss(q, gt), (p.requires_grad_(True),))
    if not with_pos:                                                  # loss = -neg_loss, not divided
        ref = -(torch.log(1 - p) * p ** 2 * (1 - gt) ** 4).sum()
        assert torch.allclose(O.focal_loss(p, gt), ref)


def test_l1_oracle_gradcheck():
    g = torch.Generator().manual_seed(4)
    out = torch.randn(2, 2, 3, 4, generator=g, dtype=torch.float64)
    index = torch.tensor([[0, 5, 5, 11], [3, 3, 3, 0]])
    mask = torch.tensor([[1.0, 1, 1, 0], [1, 0, 1, 0]], dtype=torch.float64)
    tgt = torch.randn(2, 4, 2, generator=g, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda o: O.l1_loss(o, mask, index, tgt), (out.requires_grad_(True),))
    want = sum(abs(out[n, c].flatten()[index[n, t]] - tgt[n, t, c]) for n in range(2) for t in range(4) for c in range(2)
               if mask[n, t] > 0) / (2 * 5 + 1e-4)
    assert torch.allclose(O.l1_loss(out, mask, index, tgt), want)
    assert float(O.l1_loss(out.detach(), mask * 0, index, tgt)) == 0.0


def test_decode_oracle_tie_order():
    s = np.full((1, 2, 3, 4), 0.5, np.float32)                        # a constant map: every element is its window's maximum
    wh = np.ones((1, 12, 2))
    cls, pix, sc, boxes = O.decode(s, wh, None, 10)
    assert cls[0].tolist() == [0] * 10 and pix[0].tolist() == list(range(10)) and (sc == 0.5).all()
    np.testing.assert_array_equal(boxes[0, 5], [1.0, 1.0, 2.0, 2.0])  # pixel 5 = (x 1, y 1), +0.5, -+ 0.5
    s[0, 1, 2, 3] = 0.75                                              # a peak: its three neighbours drop to 0 and lose to every 0.5
    cls, pix, sc, _ = O.decode(s, wh, None, 12 + 9)
    assert (cls[0, 0], pix[0, 0], sc[0, 0]) == (1, 11, 0.75)
    assert cls[0, 1:13].tolist() == [0] * 12 and cls[0, 13:].tolist() == [1] * 8
    assert pix[0, 13:].tolist() == [0, 1, 2, 3, 4, 5, 8, 9]


def test_wrapper_value_errors():
    from basedet.models import centernet as cn
    import basedet_amd.models.centernet as cn2
    assert cn is cn2
    f = torch.full((1, 2, 4, 4), 0.5)
    wh = torch.ones(1, 2, 4, 4)
    with pytest.raises(ValueError):
        cn.CenterNetDecoder.decode(f, wh, cat_spec_wh=True)
    with pytest.raises(ValueError):
        cn.CenterNetDecoder.decode(f, wh, K=17)
    with pytest.raises(ValueError):
        cn.CenterNetDecoder.decode(f, torch.ones(1, 3, 4, 4))
    with pytest.raises(ValueError):
        cn.reg_l1_loss(torch.ones(1, 3, 4, 4), torch.ones(1, 2), torch.zeros(1, 2, dtype=torch.int32), torch.ones(1, 2, 2))
    with pytest.raises(ValueError):
        cn.modified_focal_loss(f, torch.zeros(1, 2, 4, 5))
    from basedet_amd._lib import BasedetHipError
    with pytest.raises(BasedetHipError):                              # host tensors: no CPU path
        cn.modified_focal_loss(f, torch.zeros(1, 2, 4, 4))
    with pytest.raises(BasedetHipError):
        cn.CenterNetDecoder.decode(f, wh, K=5)


def test_host_helpers_match_the_oracle():
    from basedet_amd.models.centernet import CenterNetDecoder, CenterNetGT
    wh = np.asarray([[6, 6], [1.5, 1.5], [4, 4], [33.25, 7.5]], np.float32)
    np.testing.assert_array_equal(CenterNetGT.get_gaussian_radius(wh, 0.7), O.radius_f32(wh[:, 0], wh[:, 1], 0.7))
    fmap = np.zeros((2, 8, 10), np.float32)
    CenterNetGT.generate_score_map(fmap, np.asarray([0, -1, 1]), wh[:3], np.asarray([[0, 4], [2, 2], [5, 2]]), 0.7)
    ref = _one([[-2.5, 1.0, 3.5, 7.0, 1], [1.25, 1.25, 2.75, 2.75, 0], [3.0, 0.5, 7.0, 4.5, 2]])
    np.testing.assert_array_equal(fmap, ref["score_map"][0])
    # the affine map of the decoder: output cells of a 160 x 120 map back to a 640 x 480 image
    out = CenterNetDecoder.transform_boxes(np.asarray([[10, 20, 30, 40.0]]), (320, 240), np.asarray([640, 480]), (160, 120))
    np.testing.assert_allclose(out, [[40, 80, 120, 160]], rtol=0, atol=1e-9)


def test_symbols_declared_and_bound():
    from basedet_amd import _lib
    header = open(os.path.join(ROOT, "include", "basedet_hip.h")).read()
    build = open(os.path.join(ROOT, "basedet_amd", "build.py")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert '"centernet.hip"' in build and _lib.ABI_VERSION >= 115
