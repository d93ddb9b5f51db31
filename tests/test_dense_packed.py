"""The packed route of the dense test protocols without a GPU: evaluation.extract_features_packed fills model batches of exactly
``clip_batch`` clips from tracklets of different clip counts. On a batch-invariant stub (tests/dense_stub.py) it must equal
extract_features run tracklet by tracklet with torch.equal -- the test of the bookkeeping: straddling, a tracklet longer than the
buffer, the partial last buffer. And evaluation.clip_indices against the reference's own VideoDataset
(tests/golden/clip_indices.npz, written by tests/golden/make_clip_indices_golden.py)."""
import os

import numpy as np
import pytest
import torch

import dense_stub as DS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_indices.npz")


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
@pytest.mark.parametrize("pool", ["avg", "max"])
def test_packed_route_equals_the_per_tracklet_route(pool, dtype, layout):
    from torchreid import evaluation
    items = DS.tracklets(DS.CLIPS, seed=3, dtype=dtype, layout=layout)
    model = DS.StubModel()
    ref, ref_pids, ref_cams = evaluation.extract_features(model, items, pool=pool)
    assert ref.shape == (len(DS.CLIPS), DS.PIX + DS.ADJ)
    for c in (1, 4, 8, 64):
        model.calls = []
        got, pids, cams = evaluation.extract_features_packed(model, DS.grouped(items), clip_batch=c, pool=pool)
        assert torch.equal(got, ref), (c, (got != ref).nonzero()[:4])
        assert np.array_equal(pids, ref_pids) and np.array_equal(cams, ref_cams) and pids.tolist() == [100 + i for i in range(len(DS.CLIPS))]
        assert model.calls == DS.expected_calls(DS.CLIPS, c)       # full buffers, then the rows in use: no dummy clips


@pytest.mark.parametrize("pool", ["avg", "max"])
def test_packed_route_takes_batched_and_five_d_items(pool):
    """b = 2 where neighbours share n, and single-clip tracklets as the 5-D items of the 'evenly' sampler."""
    from torchreid import evaluation
    items = DS.tracklets(DS.CLIPS_PAIRED, seed=5)
    model = DS.StubModel()
    ref, ref_pids, ref_cams = evaluation.extract_features(model, items, pool=pool)
    for five_d in (False, True):
        loader = DS.grouped(items, five_d=five_d)
        assert sorted({it[0].shape[0] for it in loader}) == [1, 2] and (not five_d or any(it[0].dim() == 5 for it in loader))
        same_route, _, _ = evaluation.extract_features(model, loader, pool=pool)
        assert torch.equal(same_route, ref)
        for c in (1, 4, 8, 64):
            got, pids, cams = evaluation.extract_features_packed(model, iter(loader), clip_batch=c, pool=pool, prefetch=False)
            assert torch.equal(got, ref) and np.array_equal(pids, ref_pids) and np.array_equal(cams, ref_cams), (five_d, c)


def test_packed_route_refuses_what_it_cannot_pack():
    from torchreid import evaluation
    items = DS.tracklets(DS.CLIPS[:3], seed=3)
    model = DS.StubModel()
    with pytest.raises(ValueError, match="clip_batch"):
        evaluation.extract_features_packed(model, items, clip_batch=0)
    with pytest.raises(ValueError, match="share clip shape"):
        evaluation.extract_features_packed(model, items[:1] + DS.tracklets(DS.CLIPS[:1], seed=3, dtype=torch.float32), clip_batch=4)
    with pytest.raises(ValueError, match="needs frame_size"):
        evaluation.extract_features_packed(model, [items[0] + (np.zeros((1, 1, DS.S, 2)),)], clip_batch=4)
    with pytest.raises(ValueError, match="no batches"):
        evaluation.extract_features_packed(model, [], clip_batch=4)


@pytest.mark.parametrize("pool", ["avg", "max"])
def test_one_inf_clip_raises(pool):
    """The range check is on the RAW rows: one clip of a 17-clip tracklet embeds to inf."""
    from torchreid import evaluation
    model = DS.StubModel(poison=True)
    clean = DS.tracklets(DS.CLIPS, seed=3)
    evaluation.extract_features_packed(model, clean, clip_batch=8, pool=pool)
    bad = DS.tracklets(DS.CLIPS, seed=3, poison_clip=sum(DS.CLIPS[:8]) + 11)
    with pytest.raises(FloatingPointError, match="non-finite embeddings"):
        evaluation.extract_features_packed(model, bad, clip_batch=8, pool=pool)


def test_evaluate_routes_through_the_packed_extraction(monkeypatch):
    """evaluate(..., clip_batch=8) == evaluate(...). The ranking stage is HIP-only, so here it is replaced by a stand-in that returns
    a function of the features it was handed (tests/test_gpu_dense_packed.py runs the real one): what is checked is that both
    extractions take the packed route, with pool, and that the rest of evaluate sees the same tensors and labels."""
    from torchreid import evaluation
    seen = []

    def stand_in(qf, q_pids, q_camids, gf, g_pids, g_camids, *args, **kw):
        seen.append((qf.clone(), gf.clone(), q_pids.copy(), g_pids.copy(), q_camids.copy(), g_camids.copy(), args, kw))
        return np.array([float(qf.sum()), 0.0]), float(gf.sum())

    monkeypatch.setattr(evaluation, "match_and_rank", stand_in)
    q, g = DS.tracklets(DS.CLIPS[:5], seed=7), DS.tracklets(DS.CLIPS, seed=8)
    model = DS.StubModel()
    for pool in ("avg", "max"):
        model.calls = []
        plain = evaluation.evaluate(model, q, g, "cosine", pool=pool, max_rank=5)
        per_tracklet_calls, model.calls = model.calls, []
        packed = evaluation.evaluate(model, DS.grouped(q), DS.grouped(g), "cosine", pool=pool, max_rank=5, clip_batch=8)
        assert packed == plain
        assert per_tracklet_calls == list(DS.CLIPS[:5]) + list(DS.CLIPS)
        assert model.calls == DS.expected_calls(DS.CLIPS[:5], 8) + DS.expected_calls(DS.CLIPS, 8)
        a, b = seen[-2], seen[-1]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(np.array_equal(x, y) for x, y in zip(a[2:6], b[2:6]))
        assert a[6] == b[6] and a[7] == b[7] and b[7].get("local_only") is True


@pytest.mark.parametrize("max_len", [7, 1000])
@pytest.mark.parametrize("seq_len", [4, 8, 15])
@pytest.mark.parametrize("sample", ["evenly", "all", "dense", "skipdense"])
def test_clip_indices_are_the_reference_datasets(sample, seq_len, max_len):
    from torchreid import evaluation
    z = np.load(GOLDEN)
    tag = "%s_S%d_M%d" % (sample, seq_len, max_len)
    lens = z[tag + "_len"]
    assert len(lens) == 3 * seq_len + 1
    lists = np.split(z[tag + "_idx"], np.cumsum(lens)[:-1])
    for num, ref in zip(range(1, 3 * seq_len + 2), lists):
        got = evaluation.clip_indices(num, seq_len, sample, max_len=max_len)
        assert got.dtype == np.int64 and np.array_equal(got, ref), (tag, num, got, ref)


def test_clip_indices_quirks_and_refusals():
    from torchreid import evaluation
    assert len(evaluation.clip_indices(8, 4, "dense")) == 12                      # a multiple of seq_len: one extra clip of the last frame
    assert evaluation.clip_indices(8, 4, "dense")[8:].tolist() == [7, 7, 7, 7]
    assert evaluation.clip_indices(60, 8, "dense").size == 8 * 8 and evaluation.clip_indices(60, 15, "dense").size == 5 * 15
    assert evaluation.clip_indices(2000, 4, "all").size == 1000                   # max_len first
    for sample in ("random", "consecutive", "restricted", "nope"):
        with pytest.raises(KeyError):
            evaluation.clip_indices(9, 4, sample)
    with pytest.raises(ValueError):
        evaluation.clip_indices(0, 4, "dense")
