"""The packed route of the dense test protocols on the GPU (evaluation.extract_features_packed: staging buffers, copy stream,
agrl_clip_pool_ragged): bitwise against the per-tracklet route on the batch-invariant stub of tests/dense_stub.py, and the real
``vmgn`` in exact fp32 against what the REFERENCE DRIVER's own test() returned -- on the uniform dense fixture of
tests/golden/test_harness.npz and on the ragged one of tests/golden/test_harness_ragged.npz (tests/harness_ragged.py) -- at the bars
tests/test_gpu_eval.py::test_device_pipeline_equals_the_reference_test_function holds the per-tracklet route to."""
import os

import numpy as np
import pytest
import torch

import dense_stub as DS
import harness_ragged as HR
import harness_split as HS
from recipe import recipe_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the stub: bookkeeping, staging buffers, streams and the kernel, bit for bit ------------------------------------------------------
@pytest.mark.parametrize("prefetch", [True, False], ids=["prefetch", "one_stream"])
@pytest.mark.parametrize("source", ["host", "pinned", "device"])
@pytest.mark.parametrize("form", [(torch.uint8, "nhwc"), (torch.float32, "nchw")], ids=["u8_nhwc", "f32_nchw"])
def test_packed_route_equals_the_per_tracklet_route_on_the_gpu(form, source, prefetch):
    from torchreid import evaluation
    dtype, layout = form
    items = DS.tracklets(DS.CLIPS, seed=3, dtype=dtype, layout=layout)
    model = DS.StubModel().to(DEV)
    if source == "device":
        items = DS.to_device(items, DEV)
    elif source == "pinned":
        items = [(x.pin_memory(), p, c, a.pin_memory()) for x, p, c, a in items]
    for pool in ("avg", "max"):
        ref, ref_pids, ref_cams = evaluation.extract_features(model, items, pool=pool, prefetch=prefetch)
        assert ref.is_cuda and ref.shape == (len(DS.CLIPS), DS.PIX + DS.ADJ)
        for c in (1, 4, 8, 64):
            model.calls = []
            got, pids, cams = evaluation.extract_features_packed(model, DS.grouped(items), clip_batch=c, pool=pool, prefetch=prefetch)
            assert got.is_cuda and torch.equal(got, ref), (pool, c, (got != ref).nonzero()[:4])
            assert np.array_equal(pids, ref_pids) and np.array_equal(cams, ref_cams)
            assert model.calls == DS.expected_calls(DS.CLIPS, c)
    paired = DS.tracklets(DS.CLIPS_PAIRED, seed=5, dtype=dtype, layout=layout)
    ref, _, _ = evaluation.extract_features(model, paired, prefetch=prefetch)
    for five_d in (False, True):
        got, _, _ = evaluation.extract_features_packed(model, DS.grouped(paired, five_d=five_d), clip_batch=8, prefetch=prefetch)
        assert torch.equal(got, ref), five_d


@pytest.mark.parametrize("prefetch", [True, False], ids=["prefetch", "one_stream"])
def test_one_inf_clip_raises_on_the_gpu(prefetch):
    """The flag is the kernel's: one clip of the 17-clip tracklet embeds to inf, in a buffer whose tracklet is pooled two buffers later."""
    from torchreid import evaluation
    model = DS.StubModel(poison=True).to(DEV)
    evaluation.extract_features_packed(model, DS.tracklets(DS.CLIPS, seed=3), clip_batch=8, prefetch=prefetch)
    bad = DS.tracklets(DS.CLIPS, seed=3, poison_clip=sum(DS.CLIPS[:8]) + 1)
    with pytest.raises(FloatingPointError, match="non-finite embeddings"):
        evaluation.extract_features_packed(model, bad, clip_batch=8, prefetch=prefetch)


# ---- the real model against the reference driver's test() ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vmgn():
    from torchreid import models
    z = np.load(os.path.join(GOLDEN, "test_harness.npz"))
    m = models.init_model("vmgn", num_classes=HS.N_ID, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2,
                          num_scale=1, pyramid_part=True, use_pose=True, learn_graph=True)
    sd = recipe_state_dict(m.state_dict(), seed=0)
    for name, mean, var in (("global_bottleneck", "g_mean", "g_var"), ("att_bottleneck", "a_mean", "a_var")):
        sd[name + ".running_mean"] = torch.from_numpy(z[mean])
        sd[name + ".running_var"] = torch.from_numpy(z[var])
        sd[name + ".weight"] = torch.ones_like(sd[name + ".weight"])
        sd[name + ".bias"] = torch.zeros_like(sd[name + ".bias"])
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m.hip_precision = "fp32"
    return m


@pytest.fixture(scope="module")
def packed_features(vmgn):
    """the packed extraction of both fixtures, once (it does not depend on the metric)"""
    from torchreid import evaluation
    q_pids, q_cams, g_pids, g_cams = HS.make_split()
    out = {}
    for name, (ql, gl) in (("uniform", (HS.dense_loader(q_pids, q_cams, HS.Q_SEED), HS.dense_loader(g_pids, g_cams, HS.G_SEED))),
                           ("ragged", HR.loaders())):
        qf, qp, qc = evaluation.extract_features_packed(vmgn, ql, clip_batch=8, pool="avg")
        gf, gp, gc = evaluation.extract_features_packed(vmgn, gl, clip_batch=8, pool="avg")
        assert np.array_equal(qp, q_pids) and np.array_equal(qc, q_cams) and np.array_equal(gp, g_pids) and np.array_equal(gc, g_cams)
        out[name] = (qf, gf)
    return out


def hold_to_the_reference(z, tag, qf, gf, r1, mAP, metric):
    """the assertions of test_device_pipeline_equals_the_reference_test_function, and index-exactness PER QUERY -> queries exempted"""
    from torchreid import metrics
    q_pids, q_cams, g_pids, g_cams = HS.make_split()
    d = metrics.compute_distance_matrix(qf, gf, metric).cpu().numpy()
    ref = z[tag + "_distmat"]
    abs_err = np.abs(d - ref).max()
    err = abs_err / np.abs(ref).max()
    cmc, mAP2 = metrics.evaluate_rank(d, q_pids, g_pids, q_cams, g_cams, use_metric_mars=True)
    print("reference test() vs the packed route, %s: distmat rel err %.2e, Rank-1 %.4f mAP %.6f (reference %.4f %.6f)" % (
        tag, err, r1, mAP, z[tag + "_rank1"], z[tag + "_mAP"]))
    assert err < 1e-5
    assert abs(r1 - float(z[tag + "_rank1"])) < 1e-12 and abs(mAP - float(z[tag + "_mAP"])) < 1e-6
    assert abs(mAP2 - mAP) < 1e-9 and abs(cmc[0] - r1) < 1e-12      # the API path and the fused device path agree
    gaps = np.diff(np.sort(ref, axis=1)[:, :51], axis=1).min(axis=1)
    exempt = 0
    for r in range(ref.shape[0]):
        if gaps[r] > 4 * abs_err:      # no near-tie in this query's top-50 list: index-exact
            assert np.array_equal(np.argsort(d[r], kind="stable")[:50], np.argsort(ref[r], kind="stable")[:50]), (tag, r)
        else:
            exempt += 1
    if exempt == 0:
        assert np.array_equal(cmc, z[tag + "_cmc"]) and mAP2 == float(z[tag + "_mAP"])
    return exempt


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_packed_evaluate_equals_the_reference_test_function_on_the_uniform_fixture(vmgn, packed_features, metric):
    from torchreid import evaluation
    z = np.load(os.path.join(GOLDEN, "test_harness.npz"))
    q_pids, q_cams, g_pids, g_cams = HS.make_split()
    r1, mAP = evaluation.evaluate(vmgn, HS.dense_loader(q_pids, q_cams, HS.Q_SEED), HS.dense_loader(g_pids, g_cams, HS.G_SEED), metric,
                                  pool="avg", clip_batch=8)
    hold_to_the_reference(z, "%s_dense" % metric, *packed_features["uniform"], r1, mAP, metric)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_packed_evaluate_equals_the_reference_test_function_on_the_ragged_fixture(vmgn, packed_features, metric):
    """Tracklets of 1, 2, 3, 5 and 9 clips in model batches of 8: the reference pooled each tracklet on its own (--test-batch 1)."""
    from torchreid import evaluation
    z = np.load(os.path.join(GOLDEN, "test_harness_ragged.npz"))
    assert int(z["g_seed"]) == HR.G_SEED and int(z["q_seed"]) == HR.Q_SEED
    assert z["g_clips"].tolist() == HR.clip_counts(len(z["g_pids"]), HR.LONG_AT) and z["q_clips"].tolist() == HR.clip_counts(len(z["q_pids"]))
    assert int(z["%s_dense_exempt" % metric]) <= 2
    ql, gl = HR.loaders()
    r1, mAP = evaluation.evaluate(vmgn, ql, gl, metric, pool="avg", clip_batch=8)
    exempt = hold_to_the_reference(z, "%s_dense" % metric, *packed_features["ragged"], r1, mAP, metric)
    print("queries exempt from index-exactness: %d (the fixture's count at the 1e-5 bar: %d)" % (exempt, int(z["%s_dense_exempt" % metric])))
    assert exempt <= int(z["%s_dense_exempt" % metric])      # the observed error is below the bar, so the rule exempts no more than there


def test_packed_route_resamples_decoded_frames_into_the_staging_buffer(vmgn):
    """frame_size: ragged tracklets of 128 x 64 uint8 containers with valid extents. What the model is handed (a forward pre-hook keeps
    a copy) is torch.equal to _to_frame_size of every item, clip after clip, in batches of 8; the features give the per-item route's
    distance matrix within 1e-5."""
    from torchreid import evaluation, metrics
    counts, S = (1, 2, 3, 5, 2, 9, 1), 4
    g = torch.Generator().manual_seed(23)
    items = []
    for i, n in enumerate(counts):
        x = torch.randint(0, 256, (1, n, S, 128, 64, 3), generator=g, dtype=torch.uint8)
        sizes = torch.stack([torch.randint(100, 129, (1, n, S), generator=g), torch.randint(50, 65, (1, n, S), generator=g)], -1).numpy()
        items.append((x, torch.tensor([i]), torch.tensor([i % 2]), torch.ones((1, n, 28, 28)), sizes))
    want = torch.cat([evaluation._to_frame_size(it[0][0].to(DEV), it[4][0], (256, 128)) for it in items], 0)
    staged = []
    hook = vmgn.register_forward_pre_hook(lambda mod, args: staged.append(args[0].clone()))
    try:
        got, pids, _ = evaluation.extract_features_packed(vmgn, items, clip_batch=8, frame_size=(256, 128))
    finally:
        hook.remove()
    assert [s.shape[0] for s in staged] == DS.expected_calls(counts, 8) and staged[0].dtype == torch.uint8
    assert torch.equal(torch.cat(staged, 0), want)
    ref, ref_pids, _ = evaluation.extract_features(vmgn, items, frame_size=(256, 128))
    assert np.array_equal(pids, ref_pids)
    for metric in ("cosine", "euclidean"):
        d, d_ref = (metrics.compute_distance_matrix(f, f, metric).cpu().numpy() for f in (got, ref))
        err = np.abs(d - d_ref).max() / np.abs(d_ref).max()
        print("frame_size, %s: distmat rel err vs the per-item route %.2e" % (metric, err))
        assert err < 1e-5
