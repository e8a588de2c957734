"""The OTA edge-case problems of tests/test_ota_edges_gpu.py are not tie-dominated: the oracle with its literal class cost (the sum over
the K one-hot columns) and the oracle with the kernel's association (S_bg - f(x_c, 0)) + f(x_c, 1) in float32 assign the same labels,
except at no more points than the GPU test's cap, each with one of the GPU test's excuses.  The caps of the GPU test mean something
only because the reference alone stays within them."""
import functools

import numpy as np
import pytest

from oracle import box_ops
from tests import util as U


@functools.lru_cache(maxsize=None)
def _case(name):
    prob = U.ota_edge_problem(*U.OTA_EDGE_CASES[name])
    args = (prob["pts"], prob["strides"], prob["logits"], prob["pred"], prob["gt"], prob["num"]) + U.OTA_ARGS
    return prob, args, box_ops.ota_ground_truth(*args)


@pytest.mark.parametrize("name", sorted(U.OTA_EDGE_CASES))
def test_ota_topk_labels_survive_the_reassociated_class_cost(name):
    prob, args, ref = _case(name)
    alt = box_ops.ota_ground_truth(*args, class_cost="reassociated")
    worst = max(float(np.abs(a[0] - b[0])[a[0] < 1e5].max(initial=0) / 1e-4) for a, b in zip(ref[3], alt[3]) if a[0].size)
    nfg, cap, diff = U.ota_topk_compare(prob, ref, alt[0], alt[1])
    print(f"{name}: foreground {nfg}, cap {cap}, differing points {diff}, largest cost difference below the penalty {worst * 1e-4:.2e}")
    assert nfg >= 5 and len(diff) <= cap, (len(diff), nfg)
    assert all(e is not None for _, _, e in diff), diff
    same = (alt[0] == ref[0]) & (ref[0] > 0)
    np.testing.assert_array_equal(alt[1][same], ref[1][same])
    np.testing.assert_array_equal(alt[2][same], ref[2][same])


def test_ota_oracle_class_cost_forms_agree():
    """The two associations are the same sum: the cost matrices agree to fp32 rounding of a K-term sum (K 2^-24 relative, K = 80 terms of
    one sign, on top of the float64 -> float32 rounding of the literal form), far inside the 1e-4 the excuses allow; the default is
    the literal form, and an unknown name is an error."""
    prob = U.ota_edge_problem(*U.OTA_EDGE_CASES["g1_1"])
    args = (prob["pts"], prob["strides"], prob["logits"], prob["pred"], prob["gt"], prob["num"]) + U.OTA_ARGS
    ref, lit, alt = box_ops.ota_ground_truth(*args), box_ops.ota_ground_truth(*args, class_cost="literal"), \
        box_ops.ota_ground_truth(*args, class_cost="reassociated")
    for a, b, c in zip(ref[3], lit[3], alt[3]):
        assert np.array_equal(a[0], b[0])
        inside = a[0] < 1e5
        assert inside.any()
        assert np.all(np.abs(c[0][inside].astype(np.float64) - a[0][inside]) <= 81 * 2.0 ** -24 * np.abs(a[0][inside]))
        assert np.all(np.abs(c[0][~inside].astype(np.float64) - a[0][~inside]) <= 0.0625)
    with pytest.raises(ValueError):
        box_ops.ota_ground_truth(*args, class_cost="other")


def _assign_with_wrong_rule(prob, ref, rule):
    """The top-k assignment from the oracle's own matrices with one index rule broken: "rank" restarts the rank among the points whose
    cost equals the dyn_k-th smallest in every 1024-point pass (so each pass takes its own first ones), "argmin" sends an exact tie
    of a conflict to the highest gt index.  Returns (labels, targets)."""
    lab, tgt = np.zeros_like(ref[0]), np.zeros_like(ref[1])
    for n, G in enumerate(prob["num"]):
        if G == 0:
            continue
        cost, ious = ref[3][n]
        dyn, _, mm, srt = U.ota_topk_selection(cost, ious, U.OTA_ARGS[4])
        P = cost.shape[1]
        if rule == "rank":
            for g in range(G):
                T = srt[g, dyn[g] - 1]
                mm[g] = cost[g] < T
                need = dyn[g] - mm[g].sum()
                for c0 in range(0, P, 1024):
                    mm[g, c0 + np.nonzero(cost[g, c0:c0 + 1024] == T)[0][:need]] = True
        multi = np.nonzero(mm.sum(0) > 1)[0]
        am = G - 1 - cost[::-1][:, multi].argmin(0) if rule == "argmin" else cost[:, multi].argmin(0)
        mm[:, multi] = False
        mm[am, multi] = True
        fg = np.nonzero(mm.any(0))[0]
        mg = mm.argmax(0)[fg]
        lab[n, fg] = prob["gt"][n, mg, 4].astype(np.int32)
        tgt[n, fg] = box_ops.point_encode(prob["allp"][fg], prob["gt"][n, mg, :4])
    return lab, tgt


@pytest.mark.parametrize("name", ["g100_0_37_1", "k13_ld16"])
def test_ota_edge_cases_tell_the_index_rules(name):
    """The planted exact ties make the two index rules of the kernel decisive: an assignment that breaks either one differs from the
    oracle at more points than the cap allows (every such point is a tie, so the excuses alone would let it pass), and the comparison
    itself reports no difference for the unbroken rules."""
    prob, _, ref = _case(name)
    lab, tgt = _assign_with_wrong_rule(prob, ref, None)
    assert np.array_equal(lab, ref[0]) and np.array_equal(tgt, ref[1])
    for rule in ("rank", "argmin"):
        lab, tgt = _assign_with_wrong_rule(prob, ref, rule)
        _, cap, diff = U.ota_topk_compare(prob, ref, lab, tgt)
        print(f"{name}: rule {rule} broken: {len(diff)} differing points, excuses {sorted(e or '-' for _, _, e in diff)}, cap {cap}")
        assert len(diff) > cap
        assert all(e in ("a", "b") for _, _, e in diff)
