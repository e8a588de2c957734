"""YOLOX behind the head without a GPU: the float64 oracle (tests/yolox_oracle.py) on hand-worked cases, the properties the shared
problems must have, FastPointGenerator, YOLOXConfig against the reference's values (tests/golden/yolox_cfg.json), the new symbols in the
header and the binding, and the refusals of the Python surface."""
import json
import os
import re

import numpy as np
import pytest
import torch

import yolox_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["bd_yolox_assign_workspace_bytes", "bd_yolox_assign", "bd_yolox_loss_workspace_bytes", "bd_yolox_loss_fwd_bwd",
           "bd_yolox_candidates"]


def _hand(points_xy, gts, cls, raw, obj=4.0, stride=8.0, K=2):
    """A one-image problem on hand-placed points of one level."""
    pts = np.asarray(points_xy, np.float32)
    P = pts.shape[0]
    c = np.zeros((1, P, 8))
    c[0, :, :K] = cls
    bo = np.zeros((1, P, 8))
    bo[0, :, :4] = raw
    bo[0, :, 4] = obj
    gt = np.asarray(gts, np.float32).reshape(1, -1, 5)
    return dict(K=K, pts=pts, stride=np.full(P, stride), gt=gt, num=np.asarray([gt.shape[1]], np.int32), cls=c, box_obj=bo,
                lvl_start=[0, P])


def test_one_gt_five_points():
    """gt (8, 8)-(40, 40), class 1; points at 0, 16, 24, 32 (inside or near the centre 24) and 80 (neither).  Point (24, 24) predicts the gt
    exactly (IoU 1), (16, 16) predicts a 16 x 16 box inside it (IoU 0.25), the others a 8 x 8 box: the top IoUs sum to 1.25 + 3/16 ->
    k = 1, and the cheapest candidate is the exact one."""
    raw = np.zeros((5, 4))
    raw[2] = [0, 0, np.log(4.0), np.log(4.0)]         # w = h = 32 around (24, 24)
    raw[1] = [0, 0, np.log(2.0), np.log(2.0)]         # 16 x 16 around (16, 16)
    prob = _hand([[0, 0], [16, 16], [24, 24], [32, 32], [80, 80]], [[8, 8, 40, 40, 1]], [[-1.0, -3.0]] * 5, raw)
    m, u, aux = O.assign(prob)
    a = aux[0]
    # (0, 0) lies outside the gt but within 20 px of its centre in x and y: (24 - 20, 24 + 20) holds 16, 24, 32 and not 0 -> not a candidate
    assert a["cand"].tolist() == [1, 2, 3]
    np.testing.assert_allclose(a["iou"][0], [0.25, 1.0, 64 / 1024], rtol=1e-12)
    assert a["dyn"].tolist() == [1] and m[0].tolist() == [-1, -1, 0, -1, -1] and u[0, 2] == 1.0
    s = np.sqrt(1 / (1 + np.exp(1.0)) / (1 + np.exp(-4.0)))
    s2 = np.sqrt(1 / (1 + np.exp(3.0)) / (1 + np.exp(-4.0)))
    want = -np.log(s) - np.log(1 - s2) + 3 * -np.log(1 + 1e-8)
    assert abs(a["cost"][0, 1] - want) < 1e-12
    # a point inside neither the box nor the centre box of the gt pays the penalty
    prob2 = _hand([[0, 0], [24, 24]], [[8, 8, 40, 40, 1], [-4, -4, 4, 4, 2]], [[-1.0, -3.0]] * 2, raw[[0, 2]])
    a2 = O.assign(prob2)[2][0]
    assert a2["cand"].tolist() == [0, 1] and a2["cost"][0, 0] > 1e5 and a2["cost"][0, 1] < 100


def test_two_gt_conflict_goes_to_the_cheaper_gt():
    """Two overlapping gts of different classes and one candidate point both select (k = 1 each): the point's class logits favour
    class 2, so gt 1 wins although gt 0 has the lower index."""
    raw = np.asarray([[0, 0, np.log(4.0), np.log(4.0)]])
    prob = _hand([[24, 24]], [[8, 8, 40, 40, 1], [8, 8, 40, 40, 2]], [[-3.0, 2.0]], raw)
    m, u, aux = O.assign(prob)
    assert aux[0]["sel"].sum() == 2 and aux[0]["cost"][1, 0] < aux[0]["cost"][0, 0]
    assert m[0].tolist() == [1] and u[0, 0] == 1.0


def test_duplicate_gt_goes_to_the_lower_index():
    raw = np.asarray([[0, 0, np.log(4.0), np.log(4.0)]] * 2)
    prob = _hand([[24, 24], [16, 24]], [[8, 8, 40, 40, 1], [8, 8, 40, 40, 1]], [[-1.0, -3.0]] * 2, raw)
    m, _, aux = O.assign(prob)
    assert np.array_equal(aux[0]["cost"][0], aux[0]["cost"][1])
    assert (m[0][m[0] >= 0] == 0).all() and (m[0] >= 0).any()


def test_no_gt_and_no_candidate():
    prob = _hand([[0, 0], [8, 8]], [[500, 500, 540, 540, 1]], [[0.0, 0.0]] * 2, np.zeros((2, 4)))
    m, u, _ = O.assign(prob)
    assert (m == -1).all() and (u == 0).all()
    prob["num"][:] = 0
    assert (O.assign(prob)[0] == -1).all()


@pytest.mark.parametrize("shape", O.SHAPES)
def test_shared_problems_hold_what_the_gpu_test_needs(shape):
    """Every batch with N > 1 has an image without gts; the two large problems each show a gt with k = 1, a gt with k >= 5, a point
    taken by several gts and a gt whose candidates all come from the centre test; the float64 oracle run on float32-rounded
    intermediates with the re-associated class cost stays inside the cap, every difference excused."""
    prob = O.problem(shape)
    ref = O.reference(shape)
    m, u, aux = ref
    N = shape[0]
    assert N == 1 or (prob["num"] == 0).any()
    assert (m >= 0).sum() >= 5 and np.isfinite(u).all()
    dyn = np.concatenate([a["dyn"] for a in aux if "dyn" in a])
    assert (dyn >= 5).any()
    if shape[4] >= 40:
        assert (dyn == 1).any()
        assert any((a["sel"].sum(0) > 1).any() for a in aux if "sel" in a)
    if shape[4] >= 7:
        assert any((~a["in_box"].any(1)).any() for a in aux if "in_box" in a)
    gt = prob["gt"][0, :int(prob["num"][0]), :4]
    assert (np.minimum(gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]) >= 4).all() and np.abs(gt).max() < 1024
    m32, u32, _ = O.assign(prob, np.float32, True)
    nfg, cap, diff = O.compare(prob, ref, m32)
    assert len(diff) <= cap and all(e is not None for _, _, e in diff), diff
    same = (m32 == m) & (m >= 0)
    assert np.abs(u32 - u)[same].max() < 2.0 ** -12


def test_edge_problem_holds_its_cases():
    prob = O.edge_problem()
    m, u, aux = O.reference("edge")
    gt = prob["gt"][0]
    assert gt[0, 0] == gt[0, 2] and gt[1, 0] > prob["W"] and np.array_equal(gt[2], gt[3]) and gt[4, :4].tolist() == [0, 0, prob["W"], prob["H"]]
    a = aux[0]
    assert not a["in_box"][0].any() and not (a["in_box"][1] | a["in_ctr"][1]).any()
    assert (m[0] == 2).any() and not (m[0] == 3).any()             # the copy never wins a tie against the lower index
    assert aux[1]["cand"].size == 0 and (m[1] == -1).all() and prob["num"][1] == 1
    assert np.isfinite(u).all()
    nfg, cap, diff = O.compare(prob, (m, u, aux), O.assign(prob, np.float32, True)[0])
    assert len(diff) <= cap and all(e is not None for _, _, e in diff), diff
    assert (O.reference("empty")[0] == -1).all()


def test_loss_oracle_parts():
    """The loss oracle on one foreground point, by hand: prediction = gt gives iou 1 (loss 0); obj and cls are plain BCE sums."""
    raw = np.asarray([[0, 0, np.log(4.0), np.log(4.0)], [0.5, 0.25, 0.0, 0.0]])
    prob = _hand([[24, 24], [80, 80]], [[8, 8, 40, 40, 2]], [[-1.0, 0.5]] * 2, raw, obj=0.0)
    prob["N"] = 1
    m = np.asarray([[0, -1]])
    u = np.asarray([[0.75, 0.0]])
    l, dc, db = O.losses(prob, m, u, 1.0, True)
    sp = lambda x: np.log1p(np.exp(x))
    assert abs(l[0]) < 1e-12 and abs(l[1] - 2 * np.log(2)) < 1e-12
    assert abs(l[2] - (sp(-1.0) + sp(0.5) - 0.75 * 0.5)) < 1e-12
    assert abs(l[3] - 0.0) < 1e-7                                     # raw equals the l1 target up to the 1e-8 inside the log
    assert (dc[0, 1] == 0).all() and (db[0, 1, :4] == 0).all() and abs(db[0, 1, 4] - 0.5) < 1e-12
    l2 = O.losses(prob, m, u, 4.0, False)[0]
    assert l2[3] == 0 and abs(l2[1] - l[1] / 4) < 1e-12


def test_fast_point_generator_order_and_values():
    from basedet_amd.layers import FastPointGenerator
    gen = FastPointGenerator(strides=(8, 16))
    a, b = gen.grid([(2, 3), (1, 2)])
    np.testing.assert_array_equal(a, [[0, 0], [8, 0], [16, 0], [0, 8], [8, 8], [16, 8]])
    np.testing.assert_array_equal(b, [[0, 0], [16, 0]])
    assert a.dtype == np.float32 and gen.level_starts([(2, 3), (1, 2)]) == [0, 6, 8]
    pts, start, stride = O.points([(2, 3), (1, 2)], (8, 16))
    np.testing.assert_array_equal(pts, np.concatenate([a, b]))
    assert start == [0, 6, 8] and stride.tolist() == [8] * 6 + [16] * 2
    assert FastPointGenerator().strides == (8, 16, 32)


def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def test_config_equals_reference_key_for_key():
    from basedet.configs import YOLOXConfig
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "yolox_cfg.json")))
    absent = want.pop("ABSENT")
    cfg = YOLOXConfig()

    def walk(w, have, path):
        for k, v in w.items():
            assert k in have, f"{path}{k} is missing"
            if isinstance(v, dict):
                walk(v, have[k], f"{path}{k}.")
            else:
                assert _plain(have[k]) == v, f"{path}{k}: {have[k]!r} != {v!r}"
    walk(want, cfg, "")
    assert set(cfg.MODEL) == set(want["MODEL"]) and set(cfg.AUG.TRAIN_SETTING) == set(want["AUG"]["TRAIN_SETTING"])
    assert set(cfg.SOLVER) >= set(want["SOLVER"])
    for key in absent:
        node = cfg
        parts = key.split(".")
        for p in parts[:-1]:
            node = node[p]
        assert parts[-1] not in node, key
    assert cfg.TEST.IOU_THRESHOLD == 0.5 and cfg.TEST.MAX_BOXES_PER_IMAGE == 100           # DetectionConfig's, which the model reads
    assert YOLOXConfig(MODEL=dict(BATCHSIZE=16)).MODEL.BATCHSIZE == 16


def test_symbols_declared_and_bound():
    from basedet_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "basedet_hip.h")).read()
    build = open(os.path.join(ROOT, "basedet_amd", "build.py")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"^(?:int|size_t) %s\(([^;]*)\);" % name, header, re.M).group(1)
        nargs = 0 if decl.strip() == "void" else decl.count(",") + 1
        assert nargs == len(_lib.SIGNATURES[name][1]), (name, nargs)
    assert '"yolox.hip": ["-ffp-contract=off"]' in build
    for name in ("yolox_assign", "yolox_assign_into", "yolox_loss_fwd_bwd", "yolox_loss_fwd_bwd_into", "yolox_candidates",
                 "yolox_candidates_into"):
        assert hasattr(ops, name), name
    assert lib.bd_yolox_assign_workspace_bytes(2, 8400) >= 2 * 8400 * 48 and lib.bd_yolox_loss_workspace_bytes() % 16 == 0


def test_python_surface_refusals():
    from basedet.models import yolox as Y
    import basedet_amd.models.yolox as Y2
    from basedet_amd._lib import BasedetHipError
    assert Y is Y2
    lg = [torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 2, 2)]
    of = [torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 2, 2)]
    ob = [torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 2, 2)]
    gt, num = torch.zeros(1, 2, 5), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(BasedetHipError):                              # host tensors: no CPU path
        Y.yolox_losses(lg, of, ob, gt, num, (8, 16))
    with pytest.raises(BasedetHipError):
        Y.yolox_inference(lg, of, ob, torch.ones(1, 4), None, strides=(8, 16))
    with pytest.raises(BasedetHipError):
        Y.yolox_assignments(torch.zeros(20, 8, dtype=torch.bfloat16), torch.zeros(20, 8, dtype=torch.bfloat16), torch.zeros(20, 2), (8, 16),
                            gt, num, K=3, lvl_start=[0, 16, 20])
    with pytest.raises(ValueError):
        Y.yolox_losses(lg, of[:1], ob, gt, num, (8, 16))
    with pytest.raises(ValueError):
        Y.yolox_losses(lg, [torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 3, 2)], ob, gt, num, (8, 16))
    with pytest.raises(ValueError):
        Y.yolox_losses(lg, of, [torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 2, 2)], gt, num, (8, 16))
    with pytest.raises(ValueError):
        Y.yolox_assignments(torch.zeros(20, 8), torch.zeros(20, 8), torch.zeros(20, 2), (8, 16), gt, num)      # one tensor, no lvl_start


# ---- the problems of tests/test_yolox_edges_gpu.py ----------------------------------------------------------------------------------------
def test_big_loss_problem_passes_the_grid_cap():
    """More 8-slot vectors than one trip of the capped loss launch takes; about 2 % foreground, every matched entry a valid gt of its
    image, every iou_t a float32 in (0, 1)."""
    prob, m, u = O.big_loss_problem()
    N, P, ld = prob["cls"].shape
    assert (N, prob["H"], prob["W"], prob["K"], prob["gt"].shape[1]) == O.BIG_SHAPE and P == 8400 and ld == 368
    assert N * P * ld // 8 == 1159200 > 4096 * 256                       # YX_GRID_CAP workgroups of 256 threads
    fg = m >= 0
    assert 0.015 < fg.mean() < 0.025 and fg.any(1).all()
    assert (m < prob["num"][:, None]).all() and np.isfinite(prob["gt"][0, :int(prob["num"][0])]).all()
    assert ((u[fg] > 0) & (u[fg] < 1)).all() and (u[~fg] == 0).all() and np.array_equal(u, u.astype(np.float32).astype(np.float64))
    assert np.array_equal(prob["cls"], O.bf16(prob["cls"])) and np.array_equal(prob["box_obj"], O.bf16(prob["box_obj"]))


def test_kink_problem_holds_its_cases():
    """Each named point is what its name says, exactly, in float32 and float64 and in both frames; the oracle takes matched = Gmax as
    background and gives the half weights at the ties."""
    prob = O.kink_problem()
    m, u, cases = prob["matched"], prob["iou_t"], prob["cases"]
    K, G = prob["K"], prob["gt"].shape[1]
    assert set(cases) == set(O.KINK_CASES) and len(set(cases.values())) == G and m[0, prob["bg_gmax"]] == G
    assert ((m >= 0) & (m < G)).sum() == G and (m == -1).sum() == m.size - G - 1
    pred = O.boxes_xyxy(prob)[0]
    ties = {}
    for name, p in cases.items():
        g = prob["gt"][0, m[0, p]].astype(np.float64)
        b = pred[p]
        raw = prob["box_obj"][0, p]
        assert raw[2] == 0 and raw[3] == 0 and (raw[:2] * 8 == np.round(raw[:2] * 8)).all() and (g[:4] * 4 == np.round(g[:4] * 4)).all()
        rel32 = (prob["gt"][0, m[0, p], :4] - np.tile(prob["pts"][p], 2)).astype(np.float32)           # the kernel's frame, in float32
        assert np.array_equal(rel32.astype(np.float64), g[:4] - np.tile(prob["pts"][p].astype(np.float64), 2))
        assert np.array_equal(b, b.astype(np.float32).astype(np.float64)) and (b[2:] - b[:2] == 8).all()
        ties[name] = [bool(b[j] == g[j]) for j in range(4)]
        iw, ih = min(b[2], g[2]) - max(b[0], g[0]), min(b[3], g[3]) - max(b[1], g[1])
        if name == "disjoint":
            assert iw < 0 and ih < 0
        elif name == "zero_area":
            assert g[0] == g[2] and g[1] == g[3] and b[0] < g[0] < b[2] and b[1] < g[1] < b[3] and iw == 0 and ih == 0
        else:
            assert iw > 0 and ih > 0
        assert int(g[4]) == {"label_0": 0, "label_K+1": K + 1}.get(name, int(g[4])) and (1 <= g[4] <= K) == (not name.startswith("label_"))
    assert ties["equal"] == [True] * 4 and ties["two_edges"] == [True, False, False, True]
    for j, name in enumerate(("edge_x1", "edge_y1", "edge_x2", "edge_y2")):
        assert ties[name] == [i == j for i in range(4)], name
    for name in ("disjoint", "inside", "label_0", "label_K+1", "zero_area"):
        assert ties[name] == [False] * 4, name
    g, b = prob["gt"][0, m[0, cases["inside"]]], pred[cases["inside"]]
    assert g[0] < b[0] and g[1] < b[1] and b[2] < g[2] and b[3] < g[3]
    # the oracle: matched = Gmax is background; prediction = gt has a zero box gradient only because each tie sends half each way
    loss, dc, db = O.losses(prob, m, u, 4.0, True)
    m2 = m.copy()
    m2[0, prob["bg_gmax"]] = -1
    loss2, dc2, db2 = O.losses(prob, m2, u, 4.0, True)
    assert np.array_equal(loss, loss2) and np.array_equal(dc, dc2) and np.array_equal(db, db2)
    assert (dc[0, prob["bg_gmax"]] == 0).all() and (db[0, prob["bg_gmax"], :4] == 0).all() and db[0, prob["bg_gmax"], 4] > 0
    # (with the L1 term, prediction = gt: raw dx, dy equal their targets, |x|' = 0 there; raw w, h miss theirs by the 1e-8 inside the log)
    assert np.allclose(db[0, cases["equal"], :2], 0, atol=1e-12) and np.allclose(db[0, cases["equal"], 2:4], -0.25, atol=1e-12)
    no_l1 = O.losses(prob, m, u, 4.0, False)[2]
    assert np.abs(no_l1[0, cases["equal"], :4]).max() < 1e-12 and np.abs(no_l1[0, cases["disjoint"], :4]).max() == 0
    assert np.abs(no_l1[0, cases["edge_x1"], :4]).max() > 1e-3
    for name in ("label_0", "label_K+1"):                             # every class column is a background term: the gradient is sigmoid(x) / nf
        x = prob["cls"][0, cases[name], :K]
        np.testing.assert_allclose(dc[0, cases[name]], 1 / (1 + np.exp(-x)) / 4.0, rtol=1e-12)
    assert loss[3] > 2 * 18.0 / 4.0                                   # two targets of log(1e-8) = -18.4 in the L1 sum


def test_tie_problem_is_decided_by_ties_alone():
    """The float32 restatement with the kernel's class-cost form agrees exactly with float64; within a gt two costs are equal or more than
    100 cost_tol apart; gt 1 of image 0 has its k-th and (k+1)-th cheapest candidates tied across the two 1024-point chunks; gts tie at
    the top-10 IoU cut; image 1's gt has fewer than 10 candidates."""
    prob = O.tie_problem()
    assert prob["pts"].shape[0] == 1344 and prob["lvl_start"][1] == 1024
    m, u, aux = O.assign(prob)
    m32, u32, _ = O.assign(prob, np.float32, True)
    assert np.array_equal(m, m32) and np.abs(u - u32).max() < 2.0 ** -20
    spans, iou_cut = [], []
    for n, a in enumerate(aux):
        for g in range(a["G"]):
            cost, k = a["cost"][g], int(a["dyn"][g])
            vals = np.unique(cost)
            assert all(vals[i + 1] - vals[i] > 100 * O.cost_tol(vals[i + 1]) for i in range(len(vals) - 1)), (n, g)
            s = float(a["sums"][g])                                   # (a sum of zeros is exact; any other stays clear of the integers)
            assert s == 0 or abs(s - round(s)) > 1e-3                 # compare()'s excuse c starts at 1e-4
            order = np.argsort(cost, kind="stable")
            if k < cost.size and cost[order[k - 1]] == cost[order[k]]:
                tied = a["cand"][cost == cost[order[k - 1]]]
                spans.append((n, g, bool((tied < 1024).any() and (tied >= 1024).any())))
            top = -np.sort(-a["iou"][g])
            if top.size > 10 and top[9] == top[10]:
                iou_cut.append((n, g, float(top[9])))
    assert (0, 1, True) in spans and (0, 0, False) in spans, spans
    assert {(n, g) for n, g, _ in iou_cut} == {(0, 0), (0, 1), (0, 2)} and (0, 0, 1 / 16) in iou_cut, iou_cut
    assert aux[1]["cand"].size == 8 and aux[0]["dyn"].tolist() == [1, 1, 1]
    # lowest point index, then lowest gt index
    assert np.argwhere(m >= 0).tolist() == [[0, 66], [0, 132], [0, 1316], [1, 1280]] and m[m >= 0].tolist() == [2, 1, 0, 0]
    assert u[0, 132] == 0.5 and u[0, 1316] == 1 / 16 and u[0, 66] == 0 and m[0, 1058] == -1
