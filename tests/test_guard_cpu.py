"""The guard-band helper of tests/util.py (guarded, Guarded.check, gapped_geom) on host tensors: the mutation check for
tests/test_guard_gpu.py.  A clean tensor passes; a single planted element in the front guard, the back guard, a gap between two levels
or the gap behind an image is reported with its place -- and is NOT reported when check() is told to skip exactly that place, so each of
the four places is shown to be looked at; NaN guards compare as bits (an untouched NaN guard passes, another NaN payload fails)."""
import pytest
import torch

from tests import util as U

BF = torch.bfloat16
LEVELS = [(9, 17), (5, 3), (1, 2)]


def _gapped(fill, C=40, dtype=BF, gap=7):
    geom, kind = U.gapped_geom(2, LEVELS, gap=gap)
    t, h = U.guarded(geom.pixels, C, dtype, "cpu", fill=fill, name="x")
    h.set(torch.randn(geom.pixels, C).to(dtype)).set_gaps(kind)
    return geom, kind, t, h


def _one_bit(t, r, c):
    """Flip the lowest mantissa bit of one element."""
    U.bits_of(t)[r, c] ^= 1


@pytest.mark.parametrize("fill", U.FILLS + ("sentinel",))
@pytest.mark.parametrize("dtype,C", [(BF, 40), (BF, 72), (BF, 256), (BF, 7), (torch.float32, 9), (torch.float32, None), (torch.uint8, 200)])
def test_clean_tensor_passes_and_interior_is_aligned(fill, dtype, C):
    t, h = U.guarded(37, C, dtype, "cpu", fill=fill)
    assert t.shape == ((37,) if C is None else (37, C)) and t.is_contiguous()
    assert t.data_ptr() % 256 == 0
    es = t.element_size()
    assert h.g >= 512 and h.g * (C or 1) * es >= 4096 and (h.g * (C or 1) * es) % 256 == 0
    h.check()
    t.copy_(torch.ones_like(t))          # writing every element the tensor owns touches no guard
    h.check()
    if fill == "sentinel":
        assert U.count_sentinel(t) == 0


def test_gapped_geometry_layout():
    geom, kind = U.gapped_geom(2, LEVELS, gap=7)
    assert geom.off == [0, 153 + 7, 153 + 7 + 15 + 7] and geom.pix_per_img == 153 + 15 + 2 + 21 and geom.pixels == kind.numel()
    k = kind.view(2, -1)
    for n in range(2):
        assert (k[n, :153] == 0).all() and (k[n, 153:160] == 1).all() and (k[n, 160:175] == 0).all() and (k[n, 175:182] == 1).all()
        assert (k[n, 182:184] == 0).all() and (k[n, 184:] == 2).all() and k[n, 184:].numel() == 7
    assert geom.level(1).off == [160] and geom.level(1).pix_per_img == geom.pix_per_img


@pytest.mark.parametrize("fill", U.FILLS + ("sentinel",))
def test_each_place_is_checked(fill):
    """One planted element per place: reported with the place, its row and the count; invisible only if that very place is skipped."""
    geom, kind, t, h = _gapped(fill)
    h.check()
    ppi = geom.pix_per_img
    level_gap_row = geom.off[1] - 3                      # between level 0 and level 1 of image 0
    image_gap_row = ppi + geom.off[2] + 2 + 4            # behind the last level of image 1
    assert kind[level_gap_row] == 1 and kind[image_gap_row] == 2
    plants = {
        "front guard": (h._rows2d, h.g - 1, h.g - 1),                    # the row right above the interior
        "back guard": (h._rows2d, h.g + h.rows + 5, 5),
        "level gap": (t, level_gap_row, level_gap_row),
        "image gap": (t, image_gap_row, image_gap_row),
    }
    for place, (view, r, reported) in plants.items():
        _one_bit(view, r, 11)
        with pytest.raises(U.GuardError) as e:
            h.check()
        msg = str(e.value)
        assert place in msg and f"row {reported} " in msg and "column 11" in msg and "1 element(s)" in msg, msg
        h.check(ignore=(place,))                                   # skipping this place (and only this one) hides the write
        for other in U.Guarded.PLACES:
            if other != place:
                with pytest.raises(U.GuardError):
                    h.check(ignore=(other,))
        _one_bit(view, r, 11)                                       # restore
        h.check()


def test_writes_inside_owned_rows_are_not_reported():
    geom, kind, t, h = _gapped("nan")
    t[kind == 0] = 1.0
    h.check()
    t[geom.off[1] - 1, 0] = 1.0                         # last row of the gap in front of level 1
    with pytest.raises(U.GuardError, match="level gap"):
        h.check()


@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_nan_guards_compare_as_bits(dtype):
    t, h = U.guarded(5, 8, dtype, "cpu", fill="nan")
    assert torch.isnan(h._rows2d[:h.g]).all()
    h.check()                                            # NaN != NaN as floats; the same bits pass
    other_nan = 0x7FC1 if dtype == BF else 0x7FC00001
    U.bits_of(h._rows2d)[h.g + 5 + 2, 3] = other_nan      # still a NaN, another payload
    assert torch.isnan(h._rows2d[h.g + 5 + 2, 3])
    with pytest.raises(U.GuardError) as e:
        h.check()
    assert "back guard" in str(e.value) and "row 2 " in str(e.value)
    # the output sentinel is a NaN too: a kernel that writes a quiet NaN over it is seen
    t2, h2 = U.guarded(5, 8, dtype, "cpu")
    assert U.count_sentinel(t2) == 40
    h2._rows2d[0, 0] = float("nan")
    with pytest.raises(U.GuardError, match="front guard"):
        h2.check()


def test_max_fill_alternates_sign_and_is_finite():
    for dtype, C in ((BF, 40), (BF, 7), (torch.float32, None)):
        t, h = U.guarded(6, C, dtype, "cpu", fill="max")
        g = h._rows2d[:h.g].flatten()
        assert torch.isfinite(g).all() and (g.abs() == torch.finfo(dtype).max).all()
        assert (g[0::2] > 0).all() and (g[1::2] < 0).all()
        h.check()


def test_snapshot_sees_a_changed_input():
    geom, kind, t, h = _gapped("max", C=72)
    h.snapshot()
    h.assert_unchanged()
    r = geom.off[1] + 2
    _one_bit(t, r, 5)
    with pytest.raises(U.GuardError) as e:
        h.assert_unchanged()
    assert f"row {r} " in str(e.value) and "column 5" in str(e.value)


@pytest.mark.parametrize("dtype,C", [(BF, 40), (BF, 72), (BF, 256), (torch.float32, 40), (torch.float32, None), (torch.float32, 9)])
def test_interior_alignment(dtype, C):
    for rows in (1, 37, 513):
        t, h = U.guarded(rows, C, dtype, "cpu", fill="zero")
        assert t.data_ptr() % 256 == 0, (dtype, C, rows)
        assert (h.g * (C or 1) * t.element_size()) % 256 == 0


def test_one_byte_max_fill_is_finite_in_its_own_format():
    """0x7e is the largest finite e4m3 number but a NaN in e5m2: a one-byte tensor of e5m2 numbers (fmt="e5m2") gets 0x7b / 0xfb."""
    for fmt, view, top in ((None, torch.float8_e4m3fn, 448.0), ("e5m2", torch.float8_e5m2, 57344.0)):
        t, h = U.guarded(33, 80, torch.uint8, "cpu", fill="max", fmt=fmt)
        g = h._rows2d[:h.g].flatten().view(view).float()
        assert torch.isfinite(g).all() and (g[0::2] == top).all() and (g[1::2] == -top).all()
        h.check()
        h._rows2d[h.g + 33, 1] ^= 1
        with pytest.raises(U.GuardError, match="back guard"):
            h.check()
        for fill in ("nan", "sentinel"):
            t, h = U.guarded(33, 80, torch.uint8, "cpu", fill=fill, fmt=fmt)
            assert torch.isnan(h._rows2d[:h.g].flatten().view(view).float()).all()
            h.check()
