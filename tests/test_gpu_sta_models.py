"""Eval forwards of ``res50tp``, ``simple_sta`` and ``sta`` on the GPU (torchreid/models/_sta_hip.py) against the fixtures captured
from the reference implementation (tests/golden/*_b2s4.npz), at (B, S) = (2, 4) on the fixture's clips.

  'fp32', 'fp16x3'   the selected frames equal the reference's for every (tracklet, part); the output is within 1e-3 max-normalised
                     (the project's parity bar).
  16-bit, 'bf16x3'   the bar allows each score a relative error of 1e-3, and the fixtures' smallest gap between the best and the
                     second-best frame is of that order. A device index that differs from the reference's is accepted only where the
                     reference's own t_a at the two frames differs by at most 2e-3 relative (two scores of 1e-3 each); the expected
                     output is then tests/sta_ref.py's float64 tail evaluated with the device's indices on the fixture's inputs (this
                     build's CPU layer-4 map, which test_sta_models.py ties to the reference). Any other difference fails. The number of
                     accepted swaps is printed and put on record (AGRL_BOUNDS_LOG). Index exactness in these modes is carried by
                     test_gpu_sta_kernels.py, whose scores are 5 % apart. Output bar: 1e-3 as above; 2e-2 for the 16-bit type of the
                     bfloat16 build (8 significand bits: the bar __graft_entry__.smoke() holds that build to).
uint8 frames in both layouts give the bit-identical output to the fp32 route on the same pixels; ``res50tp`` is bit-identical to
``gsta`` built without graph layers on four non-pyramid parts; the distance matrix of the (B, 1024) ``sta`` embeddings agrees with
float64 in both metrics.

Measured on an MI355X (fp16 build), output error max-normalised: fp32 1.9e-7 / 3.9e-7 / 4.3e-7 (res50tp / simple_sta / sta), fp16x3
2.8e-7 / 4.6e-7 / 3.6e-7, bf16x3 3.3e-5 / 3.0e-5 / 2.9e-5, fp16 3.0e-4 / 2.9e-4 / 2.9e-4; accepted index swaps: 0 in every mode."""
import copy

import numpy as np
import pytest
import torch

import sta_ref as SR
from bounds import check_rounded, log_record, n_acc_for, poisoned_outputs
from test_sta_models import DRIVER_KW, KINDS, built

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_DEVICE_MODELS, _MAPS = {}, {}


def precisions():
    from torchreid import hip_ops as ops
    return ["fp32", ops.LP_NAME, "bf16x3", "fp16x3"]


def device_model(kind):
    if kind not in _DEVICE_MODELS:
        _DEVICE_MODELS[kind] = copy.deepcopy(built(kind)[0]).eval().to(DEV)
    return _DEVICE_MODELS[kind]


def fixture_clips(kind):
    z = built(kind)[1]
    B, S, seed = [int(v) for v in z["meta"][:3]]
    return SR.sta_clips(B, S, seed), B, S


def cpu_map(kind):
    """this build's fp32 layer-4 map of the fixture's clips, on the CPU, once"""
    if kind not in _MAPS:
        m = built(kind)[0].eval()
        x, B, S = fixture_clips(kind)
        with torch.no_grad():
            _MAPS[kind] = m.featuremaps(x.view((B * S,) + tuple(x.shape[2:])))
    return _MAPS[kind]


def forward(kind, m, x, stages=None):
    from torchreid.models import _sta_hip
    fn = _sta_hip.hip_forward_res50tp if kind == "res50tp" else _sta_hip.hip_forward_sta
    with poisoned_outputs():
        out = fn(m, x, stages)
    torch.cuda.synchronize()
    return out


def rel(a, b):
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("precision", ["fp32", "lp16", "bf16x3", "fp16x3"])
@pytest.mark.parametrize("kind", KINDS)
def test_eval_forward_matches_reference(kind, precision):
    from torchreid import hip_ops as ops
    precision = ops.LP_NAME if precision == "lp16" else precision
    m, (_, z, sd) = device_model(kind), built(kind)
    x, B, S = fixture_clips(kind)
    m.hip_precision = precision
    stages = {}
    out = forward(kind, m, x.to(DEV), stages)
    assert m(x.to(DEV), None).equal(out) and m(x.to(DEV)).equal(out)     # the public call takes the same route; the adjacency is ignored
    assert tuple(out.shape) == tuple(z["out"].shape) and torch.isfinite(out).all()
    bar = 2e-2 if (precision == "bf16") else 1e-3
    expected, swaps = z["out"], 0
    if kind != "res50tp":
        idx = stages["idx"].cpu().long()
        ref_idx = torch.from_numpy(z["idx"]).long()
        ta = torch.from_numpy(z["t_a"]).double()
        exact_modes = ("fp32", "fp16x3")
        for b, p in (idx != ref_idx).nonzero().tolist():
            assert precision not in exact_modes, "%s %s: selected frame %d, the reference %d at tracklet %d part %d" % (
                kind, precision, int(idx[b, p]), int(ref_idx[b, p]), b, p)
            hi, lo = float(ta[b, ref_idx[b, p], p]), float(ta[b, idx[b, p], p])
            assert (hi - lo) / hi <= 2e-3, "%s %s: frame %d selected at tracklet %d part %d, but the reference's scores differ by %.3e" % (
                kind, precision, int(idx[b, p]), b, p, (hi - lo) / hi)
            swaps += 1
        if swaps:
            expected = SR.tail_ref(kind, cpu_map(kind), B, S, sd, idx=idx)["out"]
        print("%s %s: t_a err %.3e, pre-head f_g err %.3e, accepted index swaps %d" % (
            kind, precision, rel(stages["t_a"].cpu(), z["t_a"]), rel(stages["f_g"].cpu(), z["f_g"]) if not swaps else float("nan"), swaps))
        log_record({"name": "sta index swaps %s %s" % (kind, precision), "swaps": swaps, "min_gap": float(z["gaps"].min())})
    err = rel(out.cpu(), expected)
    print("%s %s: output max-normalised err %.3e (bar %.0e)" % (kind, precision, err, bar))
    assert err < bar, err


@pytest.mark.parametrize("kind", KINDS)
def test_uint8_frames_are_bitwise_the_fp32_route(kind):
    from torchreid import hip_ops as ops
    m = device_model(kind)
    x, B, S = fixture_clips(kind)
    u8 = SR.clips_u8(x)
    x32 = ops.frames_normalize_reference(u8).to(DEV)
    for precision in precisions():
        m.hip_precision = precision
        ref = forward(kind, m, x32)
        assert torch.isfinite(ref).all()
        for name, d in (("nchw", u8), ("nhwc", u8.permute(0, 1, 3, 4, 2).contiguous())):
            got = forward(kind, m, d.to(DEV))
            assert torch.equal(got, ref), "%s %s %s: %d of %d elements differ" % (kind, precision, name, int((got != ref).sum()), ref.numel())
    m.hip_precision = "fp32"


@pytest.mark.parametrize("precision", ["fp32", "lp16", "bf16x3", "fp16x3"])
def test_res50tp_is_gsta_without_graph_layers(precision):
    """Pins the reuse: the same weights through ``gsta`` built with num_gb=0, pyramid_part=False, num_split=4 give the same bits."""
    from torchreid import hip_ops as ops
    from torchreid import models
    precision = ops.LP_NAME if precision == "lp16" else precision
    m = device_model("res50tp")
    if "gsta" not in _DEVICE_MODELS:
        g = models.init_model("gsta", **dict(DRIVER_KW, num_gb=0, pyramid_part=False, num_split=4, pretrained=False))
        g.load_state_dict(built("res50tp")[2])
        _DEVICE_MODELS["gsta"] = g.eval().to(DEV)
    g = _DEVICE_MODELS["gsta"]
    x, B, S = fixture_clips("res50tp")
    m.hip_precision = g.hip_precision = precision
    a = m(x.to(DEV), None)
    b = g(x.to(DEV), torch.zeros((B, S * 4, S * 4), device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(a, b), "%s: %d of %d elements differ" % (precision, int((a != b).sum()), a.numel())
    m.hip_precision = "fp32"


def test_route_never_writes_the_map_where_the_pooling_fuses(monkeypatch):
    """simple_sta / res50tp in the 16-bit mode at 256 x 128: the part means come out of layer 4's last conv; sta stores its map and reads
    it once (agrl_sta_frame_stats). Seen through the entry points each forward calls."""
    from torchreid import _hip
    from torchreid import hip_ops as ops
    calls = []
    real = _hip.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for kind, want, absent in (("simple_sta", ["agrl_conv1x1_packed_res_pool", "agrl_sta_fuse", "agrl_linear_bn_relu"], ["agrl_part_pool", "agrl_sta_frame_stats"]),
                               ("res50tp", ["agrl_conv1x1_packed_res_pool", "agrl_row_sqnorm", "agrl_attn_pool_bnneck"], ["agrl_part_pool"]),
                               ("sta", ["agrl_sta_frame_stats", "agrl_sta_fuse", "agrl_linear_bn_relu"], ["agrl_part_pool", "agrl_conv1x1_packed_res_pool"])):
        m = device_model(kind)
        m.hip_precision = ops.LP_NAME
        del calls[:]
        forward(kind, m, fixture_clips(kind)[0].to(DEV))
        for name in want:
            assert name in calls, (kind, name, sorted(set(calls)))
        for name in absent:
            assert name not in calls, (kind, name)
        m.hip_precision = "fp32"
        del calls[:]
        forward(kind, m, fixture_clips(kind)[0].to(DEV))
        assert ("agrl_part_pool" in calls) == (kind != "sta"), (kind, sorted(set(calls)))


def test_pack_is_cached_and_follows_the_weights():
    m = device_model("sta")
    m.hip_precision = "fp32"
    x, B, S = fixture_clips("sta")
    a = forward("sta", m, x.to(DEV))
    pack = m._hip_packs[(0, "fp32")]
    forward("sta", m, x.to(DEV))
    assert m._hip_packs[(0, "fp32")] is pack
    saved = m.fc1[1].bias.detach().clone()
    with torch.no_grad():
        m.fc1[1].bias.add_(1.0)
    b = forward("sta", m, x.to(DEV))
    assert m._hip_packs[(0, "fp32")] is not pack and float((b - a).abs().max()) > 0.5
    with torch.no_grad():
        m.fc1[1].bias.copy_(saved)
    m.invalidate_hip_cache()
    assert not m._hip_packs
    assert torch.equal(forward("sta", m, x.to(DEV)), a)


def test_distance_matrix_of_sta_embeddings():
    """(B, 1024) embeddings through compute_distance_matrix, both metrics, against float64 on the same fp32 rows. Chains: the exact-fp32
    MFMA's 1024 / 4 steps (bounds.n_acc_for) plus, for the cosine, the two row normalisations (a lane's 1024 / 256 x 4 fmafs, six shuffle
    steps, three partial sums, sqrt, the quotient: <= 32 each)."""
    from torchreid import metrics
    m = device_model("sta")
    m.hip_precision = "fp32"
    x, B, S = fixture_clips("sta")
    q = forward("sta", m, x.to(DEV))
    g = torch.cat([q, forward("sta", m, SR.sta_clips(B, S, 12345).to(DEV))], 0)
    assert q.shape[1] == 1024
    qd, gd = q.cpu().double(), g.cpu().double()
    d = metrics.compute_distance_matrix(q, g, "euclidean")
    exact = qd.pow(2).sum(1, keepdim=True) + gd.pow(2).sum(1, keepdim=True).t() - 2 * qd @ gd.t()
    mag = qd.pow(2).sum(1, keepdim=True) + gd.pow(2).sum(1, keepdim=True).t() + 2 * qd.abs() @ gd.abs().t()
    w1 = check_rounded(d, exact, mag, n_acc_for(1024, 4) + 16, torch.float32, name="sta distmat euclidean")[0]
    d = metrics.compute_distance_matrix(q, g, "cosine")
    qn, gn = qd / qd.norm(dim=1, keepdim=True).clamp(min=1e-12), gd / gd.norm(dim=1, keepdim=True).clamp(min=1e-12)
    w2 = check_rounded(d, 1 - qn @ gn.t(), 1 + qn.abs() @ gn.abs().t(), n_acc_for(1024, 4) + 64, torch.float32, name="sta distmat cosine")[0]
    print("sta distmat worst err / bound: euclidean %.3f cosine %.3f" % (w1, w2))
    assert float(d[0, 1]) > 1e-4 > abs(float(d[0, 0]))   # two different tracklets are apart by more than the bound on a row's distance to itself
