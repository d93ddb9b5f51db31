"""tests/rerank_ref.py on the CPU, before any kernel is held to it.

The bound is not too tight: the reference's own fp32 outputs -- the six matrices of tests/golden/re_ranking.npz (produced by the
reference's utils/re_ranking.py) and oracle.re_ranking on every case of tests/test_gpu_rerank.py -- sit inside it (ratio <= 1) with
identical ``== 1.0`` masks; lambda = 1 is bit for bit D. The discrete layer is restated correctly: with the value layer in fp32 the
result is np.array_equal to oracle.re_ranking. The bound can tell: each of five subtle defects (half rounded half-up at k1 = 9, one
member dropped from one expanded set, k2 - 1 rows in the mean, the 2/3 test with >=, ties broken towards the higher index) breaks
the bound or the mask. The cases reach what they are named for: empty neighbour sets among the duplicates, half = 3 / 5 / 7 at
k1 = 5 / 9 / 13 (half-up would give 4 / 6 / 8), half = 16 and 1 at the limits of k1.

The largest set any case produces has nu = 62 (k1 = 30): the summation branches for nu > 128 of rr_kreciprocal_kernel stay unexercised."""
import os

import numpy as np
import pytest
import torch

import rerank_ref as R
from bounds import log_record
from oracle import vmgn_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "re_ranking.npz")
GOLD_SETTINGS = (("default", 20, 6, 0.3), ("k8_3", 8, 3, 0.2), ("k6_1", 6, 1, 0.5))
LAMBDAS = (0.3, 0.0, 1.0)


@pytest.mark.parametrize("metric", R.METRICS)
def test_reference_outputs_of_the_golden_fixture_sit_inside_the_bound(metric):
    z = np.load(GOLD)
    qf, gf = torch.from_numpy(z["qf"]), torch.from_numpy(z["gf"])
    fn = O.euclidean_squared if metric == "euclidean" else O.cosine
    q_g, q_q, g_g = (fn(a, b).numpy() for a, b in ((qf, gf), (qf, qf), (gf, gf)))
    for tag, k1, k2, lam in GOLD_SETTINGS:
        ref = R.Reference(q_g, q_q, g_g, k1, k2)
        got = z[metric + "_" + tag]
        ratio = R.worst_ratio(got, ref, lam)
        print("golden %s %s: worst err / bound %.3f" % (metric, tag, ratio))
        assert got.dtype == np.float32 and ratio <= 1.0, (metric, tag, ratio)
        # lambda != 0 here, so ``== 1.0`` is decided by fp32 roundings: the mask is compared with the fp32 restatement's
        assert np.array_equal(got == 1.0, R.restated_fp32(q_g, q_q, g_g, k1, k2, lam) == 1.0), (metric, tag)
        assert R.ranking_outside_near_ties(got, ref, lam)[0] == 0


@pytest.mark.parametrize("case", R.GRID, ids=["%s-%s-k%d_%d" % c for c in R.GRID])
def test_oracle_sits_inside_the_bound_and_the_restated_layers_match_it(case):
    name, metric, k1, k2 = case
    q_g, q_q, g_g = R.world(name, metric)
    ref = R.reference(name, metric, k1, k2)
    m = ref.m
    d = ref.disc
    for lam in LAMBDAS:
        orc = O.re_ranking(q_g, q_q, g_g, k1, k2, lam)
        if lam == 0.3:   # the layers below the blend do not depend on lambda
            assert np.array_equal(R.restated_fp32(q_g, q_q, g_g, k1, k2, lam), orc), (case, lam)
        ratio = R.worst_ratio(orc, ref, lam)
        print("oracle %s lambda %.1f: worst err / bound %.3f" % (case, lam, ratio))
        assert ratio <= 1.0, (case, lam, ratio)
        assert R.ranking_outside_near_ties(orc, ref, lam)[0] == 0
        if lam == 0.0:
            assert np.array_equal(orc == 1.0, ref.no_overlap), case
        if lam == 0.3:   # set membership at lambda != 0: without shared support jac is 1 and final the fp32 value of c_jac + D c_org
            alone = np.float32(1 - lam) + ref.D[:m, m:] * np.float32(lam)
            assert np.array_equal(orc == alone, ref.no_overlap), case
        if lam == 1.0:
            assert np.array_equal(orc, ref.D[:m, m:]), case
    assert d.half == {1: 1, 5: 3, 6: 4, 8: 5, 9: 5, 13: 7, 20: 11, 30: 16}[k1]
    if name == "duplicates":     # the last four of the 13 identical samples are not in their own neighbour list
        assert int((d.nu == 0).sum()) == 4 and not d.S1[d.nu == 0].any()
    assert d.nu.max() <= 128     # no case reaches the long-sum branches
    log_record({"name": "re_ranking cpu %s %s k1=%d k2=%d" % case, "nu_max": int(d.nu.max()), "nu_zero": int((d.nu == 0).sum()),
                "nnz_max": int(d.nnz.max())})


# defect -> the cases that must expose it (at least one of them, on the bound or on the mask)
TELLS = {
    "half_up": [("odd_k1", 9, 3)],
    "drop_member": [("odd_k1", 9, 3), ("ragged", 20, 6)],
    "k2_minus_1": [("odd_k1", 9, 3), ("k1_limits", 30, 31)],
    "ge_two_thirds": [("odd_k1", 9, 3), ("duplicates", 8, 3), ("n33", 6, 2)],
    "tie_order": [("duplicates", 8, 1)],
}


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_the_bound_can_tell(mut):
    broke = []
    for name, k1, k2 in TELLS[mut]:
        for metric in R.METRICS:
            q_g, q_q, g_g = R.world(name, metric)
            ref = R.reference(name, metric, k1, k2)
            wrong03 = R.restated_fp32(q_g, q_q, g_g, k1, k2, 0.3, mut)
            wrong0 = R.restated_fp32(q_g, q_q, g_g, k1, k2, 0.0, mut)
            ratio = max(R.worst_ratio(wrong03, ref, 0.3), R.worst_ratio(wrong0, ref, 0.0))
            mask = np.array_equal(wrong0 == 1.0, ref.no_overlap)
            print("%s on %s %s: worst err / bound %.3g, mask equal %s" % (mut, name, metric, ratio, mask))
            broke.append(ratio > 1.0 or not mask)
            # the defect never reaches D: lambda = 1 stays bit-equal, so that check alone would not see it
            assert np.array_equal(R.restated_fp32(q_g, q_q, g_g, k1, k2, 1.0, mut), ref.D[:ref.m, ref.m:])
    assert any(broke), (mut, broke)
    if mut in ("half_up", "tie_order", "k2_minus_1"):   # the three also tried on a deliberately wrong build of the kernel
        assert all(broke), (mut, broke)


def test_half_up_is_invisible_at_even_k1():
    """Why the even settings of test_re_ranking_device could not guard the rounding rule."""
    q_g, q_q, g_g = R.world("n33", "euclidean")
    assert np.array_equal(R.restated_fp32(q_g, q_q, g_g, 6, 2, 0.3, "half_up"), R.restated_fp32(q_g, q_q, g_g, 6, 2, 0.3))
