"""DATA.DUMMY_MULTISCALE (CPU only): the synthetic multi-scale data source of DetectionConfig.build_dataloader -- AUG.TRAIN_VALUE
(ShortestEdgeResize 640..800 / max 1333, flip), aspect-ratio grouping and the pad collator over COCO-like original sizes."""
import numpy as np


def _cfg(*opts):
    from basedet_amd.configs import RetinaNetConfig
    cfg = RetinaNetConfig()
    cfg.DATA.BUILDER_NAME = "DummyLoader"
    cfg.MODEL.BATCHSIZE = 16
    if opts:
        cfg.merge(list(opts))
    return cfg


def test_multiscale_loader_is_reproducible_and_keeps_the_collator_contract():
    cfg = _cfg("DATA.DUMMY_MULTISCALE", "True")
    assert cfg.DATA.DUMMY_MULTISCALE is True
    a, b = cfg.build_dataloader(), cfg.build_dataloader()
    shapes = set()
    for i in range(200):
        x, y = next(a), next(b)
        for k in ("data", "gt_boxes", "im_info"):
            assert np.array_equal(x[k], y[k]), (i, k)
        data, gt, info = x["data"], x["gt_boxes"], x["im_info"]
        N, C, H, W = data.shape
        assert (N, C) == (16, 3) and data.dtype == np.float32
        assert gt.ndim == 3 and gt.shape[0] == N and gt.shape[2] == 5 and gt.dtype == np.float32
        assert info.shape == (N, 5) and info.dtype == np.float32
        for n in range(N):
            h, w, oh, ow, g = info[n]
            assert 0 < h <= H and 0 < w <= W and (oh, ow) != (0, 0)
            assert 640 <= min(h, w) <= 800 and max(h, w) <= 1333, info[n]
            g = int(g)
            assert g > 0 and np.all(gt[n, :g, 4] > 0)
            bx = gt[n, :g, :4]
            assert np.all(bx[:, 0] >= 0) and np.all(bx[:, 1] >= 0) and np.all(bx[:, 2] <= w) and np.all(bx[:, 3] <= h), (i, n)
            assert np.all(bx[:, 2] >= bx[:, 0]) and np.all(bx[:, 3] >= bx[:, 1])
            assert np.all(data[n, :, int(h):, :] == 0) and np.all(data[n, :, :, int(w):] == 0)      # padded bottom / right
        Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
        assert Hp <= 1344 and Wp <= 1344
        shapes.add((Hp, Wp))
    assert len(shapes) >= 2, shapes


def test_multiscale_loader_is_seeded_per_rank():
    from basedet_amd.configs import RetinaNetConfig
    from basedet_amd.utils.dummy import MultiScaleDummyLoader
    aug = RetinaNetConfig().AUG.TRAIN_VALUE
    x, y = next(MultiScaleDummyLoader(4, aug, seed=0)), next(MultiScaleDummyLoader(4, aug, seed=1))
    assert x["data"].shape != y["data"].shape or not np.array_equal(x["data"], y["data"])


def test_without_multiscale_the_loader_is_the_dummy_loader():
    from basedet_amd.utils import DummyLoader
    for cfg in (_cfg(), _cfg("DATA.DUMMY_MULTISCALE", "False")):
        assert cfg.DATA.DUMMY_MULTISCALE is False
        got = cfg.build_dataloader()
        assert type(got) is DummyLoader
        want = DummyLoader(16, (800, 1344), seed=0)
        for _ in range(2):
            x, y = next(got), next(want)
            for k in ("data", "gt_boxes", "im_info"):
                assert np.array_equal(x[k], y[k]), k
