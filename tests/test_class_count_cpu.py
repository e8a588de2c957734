"""The padded class predictor's scatter / gather (basedet_amd/models/engine.py: pad_class_rows, unpad_class_rows, PaddedClsConv) as pure
numpy round trips: reference rows (A*K, ...) -> A groups of cls_ld = round_up(K, 8) rows -> reference rows."""
import numpy as np
import pytest

from basedet_amd.models.engine import cls_ld, pad_class_rows, unpad_class_rows


def test_cls_ld():
    assert [cls_ld(k) for k in (1, 7, 8, 9, 13, 80, 365, 368)] == [8, 8, 8, 16, 16, 80, 368, 368]


@pytest.mark.parametrize("A", [1, 9])
@pytest.mark.parametrize("K", [1, 13, 80, 365])
def test_scatter_gather_round_trip(A, K):
    rng = np.random.default_rng(A * 1000 + K)
    ld = cls_ld(K)
    w = rng.standard_normal((A * K, 4, 3, 3)).astype(np.float32)
    b = rng.standard_normal((A * K,)).astype(np.float32)
    w[w == 0] = 1.0
    b[b == 0] = 1.0
    for ref in (w, b):
        p = pad_class_rows(ref, A, K)
        assert p.shape == (A * ld,) + ref.shape[1:] and p.dtype == ref.dtype
        g = p.reshape((A, ld) + ref.shape[1:])
        assert np.array_equal(g[:, :K], ref.reshape((A, K) + ref.shape[1:]))      # anchor a's class k sits at row a * cls_ld + k
        assert not g[:, K:].any()                                                  # pad rows are zero
        assert np.count_nonzero(p) == ref.size
        back = unpad_class_rows(p, A, K)
        assert back.shape == ref.shape and np.array_equal(back, ref)
        if K % 8 == 0:
            assert np.array_equal(p, ref)                                          # the identity: nothing moves at K = 80


def test_gather_accepts_torch_tensors():
    import torch
    A, K = 9, 13
    ref = torch.arange(A * K * 2, dtype=torch.float32).reshape(A * K, 2) + 1
    p = torch.from_numpy(pad_class_rows(ref.numpy(), A, K))
    assert torch.equal(unpad_class_rows(p, A, K), ref)


def test_shape_mismatch_is_an_error():
    with pytest.raises(AssertionError):
        pad_class_rows(np.zeros((10, 3)), 1, 13)
    with pytest.raises(AssertionError):
        unpad_class_rows(np.zeros((13, 3)), 1, 13)
