"""The edges of the rank protocol kernels (csrc/rank.hip: agrl_rank_mars behind agrl_rank_topk, agrl_rank_market1501) against the
oracle's restatement of the reference's torchreid/metrics/rank.py, under poisoned allocations and run twice.

MARS (evaluate_mars + Compute_AP): per-query AP bit-equal (fp64 in the reference's operation order), per-query CMC and the ranked lists
equal, mAP equal, on n = 4099 (radix top-k) with 30 % junk (pid -1), a query whose good matches all rank beyond max_rank, a query
with exactly one good match, a query with pid -1 (every good match is junk too) and exact distance ties across positions 49 / 50;
max_rank = 1 and max_rank = n at n = 64; a query without any good match whose whole list is junk (AP 0, nothing raised -- on the device
and in the numpy twin alike, as in the reference, which only divides by ngood at a non-junk entry).

market1501 (eval_market1501): m = 1; a query with 4097 correct matches -- one more than the kernel holds -- gives valid = -1 and a NaN
AP, and evaluate_rank (market1501 and cuhk03 branches) raises the RuntimeError that names the query; every query invalid hits the
reference's assertion.

On every case the device, the numpy twins in torchreid/metrics/rank.py and the oracle agree: neither side departs from the reference.
Tried on a deliberately wrong build of the library (a scratch copy): a CMC not shifted by the junk seen, NaN for a query without a good
match, same-camera samples counted as matches and an unreported overflow of the match list fail all seven tests but max_rank = 1,
which ties towards the higher index in the register top-k fails (its two nearest gallery samples tie exactly)."""
import numpy as np
import pytest
import torch

from bounds import poisoned_outputs
from oracle import vmgn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def i32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def mars_device(d, q_pids, g_pids, q_cam, g_cam, max_rank):
    """(ap, cmc, idx) numpy, from two poisoned runs that must agree bit for bit."""
    from torchreid import metrics
    args = (torch.from_numpy(d).to(DEV), i32(q_pids), i32(g_pids), i32(q_cam), i32(g_cam), max_rank)
    with poisoned_outputs():
        a = metrics.rank.hip_evaluate_mars_device(*args)
    with poisoned_outputs():
        b = metrics.rank.hip_evaluate_mars_device(*args)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two runs differ"
    return tuple(x.cpu().numpy() for x in a)


def check_mars(d, q_pids, g_pids, q_cam, g_cam, max_rank):
    from torchreid import metrics
    cmc_o, map_o, ap_o, cmcq_o, orders_o = O.evaluate_mars(d, q_pids, g_pids, q_cam, g_cam, max_rank, return_all=True)
    ap, cmc, idx = mars_device(d, q_pids, g_pids, q_cam, g_cam, max_rank)
    assert np.array_equal(idx, orders_o), "ranked lists differ"
    assert ap.dtype == np.float64 and np.array_equal(ap, ap_o), "per-query AP is not bit-equal: %r" % (np.nonzero(ap != ap_o)[0],)
    assert np.array_equal(cmc.astype(np.float64), cmcq_o), "per-query CMC differs"
    cmc2, map2 = metrics.evaluate_rank(d, q_pids, g_pids, q_cam, g_cam, max_rank=max_rank, use_metric_mars=True)
    assert map2 == map_o and np.array_equal(cmc2, cmc_o)
    cmc3, map3 = metrics.rank._evaluate_mars_host(d, q_pids, g_pids, q_cam, g_cam, max_rank)   # the numpy twin
    assert map3 == map_o and np.array_equal(cmc3, cmc_o)
    return ap_o, cmcq_o, orders_o


def test_mars_edges_at_n_4099():
    rng = np.random.RandomState(4099)
    m, n, max_rank = 8, 4099, 50
    d = rng.rand(m, n).astype(np.float32)
    q_pids, g_pids = rng.randint(0, 20, m), rng.randint(0, 20, n)
    q_cam, g_cam = rng.randint(0, 6, m), rng.randint(0, 6, n)
    g_pids[rng.rand(n) < 0.3] = -1                                # 30 % junk
    # query 0: every good match ranks beyond max_rank
    q_pids[0], q_cam[0] = 3, 0
    d[0, (g_pids == 3) & (g_cam != 0)] += 2.0
    # query 1: exactly one good match (rank ~ 10) and one same-camera sample of its identity (junk), nearer still
    q_pids[1], q_cam[1] = 100, 2
    g_pids[[1500, 2500]], g_cam[[1500, 2500]] = 100, (4, 2)
    d[1, 1500], d[1, 2500] = np.sort(d[1])[10], np.float32(-1.0)
    # query 2: pid -1 -- all its good matches are junk as well
    q_pids[2], q_cam[2] = -1, 1
    # query 3: exact ties across positions 49 / 50 (0-based 47 .. 52 hold one value), good and other identities mixed among them
    q_pids[3], q_cam[3] = 5, 0
    pick = rng.permutation(n)[:53]
    d[3, pick[:47]] = -np.linspace(1.0, 0.5, 47).astype(np.float32)
    d[3, pick[47:]] = np.float32(-0.25)
    g_pids[np.sort(pick[47:])[[1, 4]]], g_cam[np.sort(pick[47:])[[1, 4]]] = 5, 3      # a good match either side of position 50
    g_pids[np.sort(pick[47:])[[0, 3]]] = 7
    d[:, 7] = d[:, 3]                                              # and a tie in every row
    ap_o, cmc_o, orders_o = check_mars(d, q_pids, g_pids, q_cam, g_cam, max_rank)
    good0 = np.nonzero((g_pids == 3) & (g_cam != 0))[0]
    assert len(good0) > 0 and not np.isin(orders_o[0], good0).any() and ap_o[0] == 0.0 and cmc_o[0].max() == 0.0
    assert ((g_pids == 100) & (g_cam != 2)).sum() == 1 and 1500 in orders_o[1] and ap_o[1] > 0
    tied = np.sort(pick[47:])
    assert np.array_equal(np.sort(orders_o[3][47:50]), tied[:3]) and d[3, orders_o[3][49]] == d[3, tied[3]]   # the tie straddles the cut


@pytest.mark.parametrize("max_rank", [1, 64])
def test_mars_max_rank_1_and_n(max_rank):
    rng = np.random.RandomState(64 + max_rank)
    m, n = 6, 64
    d = rng.rand(m, n).astype(np.float32)
    d[:, 30] = d[:, 20]
    d[:, 2] = d[:, 9] = np.float32(-1.0)                           # the two nearest tie exactly: the stable order fills position 0
    q_pids, g_pids = rng.randint(0, 5, m), rng.randint(0, 5, n)
    q_cam, g_cam = rng.randint(0, 3, m), rng.randint(0, 3, n)
    g_pids[rng.rand(n) < 0.2] = -1
    check_mars(d, q_pids, g_pids, q_cam, g_cam, max_rank)


def test_mars_all_junk_list_without_a_good_match_is_ap_zero():
    rng = np.random.RandomState(10)
    m, n, max_rank = 3, 64, 10
    d = (1.0 + rng.rand(m, n)).astype(np.float32)
    q_pids, g_pids = np.array([7, 1, 2]), rng.randint(0, 3, n)
    q_cam, g_cam = np.array([1, 0, 2]), rng.randint(0, 3, n)
    g_pids[[0, 1]], g_cam[[0, 1]] = (1, 2), (1, 0)                 # queries 1 and 2 keep a good match
    near = rng.permutation(np.arange(2, n))[:max_rank]            # query 0's whole list: pid -1, or its identity in its own camera
    d[0, near] = rng.rand(max_rank).astype(np.float32)
    g_pids[near[::2]] = -1
    g_pids[near[1::2]], g_cam[near[1::2]] = 7, 1
    assert not ((g_pids == 7) & (g_cam != 1)).any()
    ap_o, cmc_o, _ = check_mars(d, q_pids, g_pids, q_cam, g_cam, max_rank)    # nothing raised anywhere
    assert ap_o[0] == 0.0 and cmc_o[0].max() == 0.0


def market_device(d, q_pids, g_pids, q_cam, g_cam, max_rank):
    from torchreid import hip_ops as ops
    args = (torch.from_numpy(d).to(DEV), i32(q_pids), i32(q_cam), i32(g_pids), i32(g_cam), max_rank)
    with poisoned_outputs():
        a = ops.rank_market1501(*args)
    with poisoned_outputs():
        b = ops.rank_market1501(*args)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), "two runs differ"   # bits: AP may be NaN
    return tuple(x.cpu().numpy() for x in a)


def test_market1501_single_query():
    from torchreid import metrics
    rng = np.random.RandomState(1)
    n = 300
    d = rng.rand(1, n).astype(np.float32)
    d[0, 5] = d[0, 3]
    q_pids, g_pids, q_cam, g_cam = np.array([2]), rng.randint(0, 6, n), np.array([1]), rng.randint(0, 4, n)
    cmc_o, map_o, ap_o, first_o = O.eval_market1501(d, q_pids, g_pids, q_cam, g_cam, 50, return_all=True)
    ap, cmc, valid = market_device(d, q_pids, g_pids, q_cam, g_cam, 50)
    assert valid[0] == 1 and abs(ap[0] - ap_o[0]) < 1e-14 and int(cmc[0].argmax()) == first_o[0]
    cmc2, map2 = metrics.evaluate_rank(d, q_pids, g_pids, q_cam, g_cam, max_rank=50, use_metric_market1501=True)
    assert np.array_equal(cmc2, cmc_o) and abs(map2 - map_o) < 1e-14


def test_market1501_more_matches_than_the_kernel_holds():
    from torchreid import metrics
    rng = np.random.RandomState(5000)
    m, n = 3, 5000
    d = rng.rand(m, n).astype(np.float32)
    q_pids, q_cam = np.array([0, 1, 2]), np.array([0, 0, 1])
    g_pids, g_cam = rng.randint(2, 6, n), rng.randint(0, 3, n)
    g_pids[:20] = 0
    where = rng.permutation(np.arange(20, n))[:4097]              # 4097 correct matches of query 1 (MK_MAXREL + 1)
    g_pids[where], g_cam[where] = 1, 1 + rng.randint(0, 2, 4097)
    assert ((g_pids == 1) & (g_cam != 0)).sum() == 4097
    _, _, ap_o, first_o = O.eval_market1501(d, q_pids, g_pids, q_cam, g_cam, 50, return_all=True)
    ap, cmc, valid = market_device(d, q_pids, g_pids, q_cam, g_cam, 50)
    assert list(valid) == [1, -1, 1] and np.isnan(ap[1]) and cmc[1].max() == 0.0
    for q in (0, 2):
        assert abs(ap[q] - ap_o[q]) < 1e-14 and (int(cmc[q].argmax()) if cmc[q].max() > 0 else -1) == (first_o[q] if first_o[q] < 50 else -1)
    with pytest.raises(RuntimeError, match="query 1 has more correct matches"):
        metrics.evaluate_rank(d, q_pids, g_pids, q_cam, g_cam, max_rank=50, use_metric_market1501=True)
    with pytest.raises(RuntimeError, match="query 1 has more correct matches"):
        metrics.evaluate_rank(d, q_pids, g_pids, q_cam, g_cam, max_rank=50, use_metric_cuhk03=True)


def test_market1501_every_query_invalid_hits_the_reference_assertion():
    from torchreid import metrics
    rng = np.random.RandomState(2)
    m, n = 4, 100
    d = rng.rand(m, n).astype(np.float32)
    q_pids, g_pids = np.array([50, 51, 1, 1]), rng.randint(0, 4, n)
    q_cam, g_cam = np.array([0, 1, 2, 2]), rng.randint(0, 2, n)      # identity 1 only in cameras 0 / 1 ... all of them camera 2's own
    g_cam[g_pids == 1] = 2
    with pytest.raises(AssertionError, match="all query identities do not appear in gallery"):
        O.eval_market1501(d, q_pids, g_pids, q_cam, g_cam, 50)
    ap, cmc, valid = market_device(d, q_pids, g_pids, q_cam, g_cam, 50)
    assert not valid.any() and np.isnan(ap).all() and cmc.max() == 0.0
    with pytest.raises(AssertionError, match="all query identities do not appear in gallery"):
        metrics.evaluate_rank(d, q_pids, g_pids, q_cam, g_cam, max_rank=50, use_metric_market1501=True)
