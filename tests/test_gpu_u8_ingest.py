"""uint8 frames on the GPU. The bar everywhere is BITWISE equality (torch.equal), not a tolerance: the kernels only look the
normalised value of a byte up in the caller's table (hip_ops.frame_table, pinned on ToTensor + Normalize by tests/test_u8_ingest.py),
so a uint8 launch must stage exactly the fp32 values the fp32 launch reads from the table-normalised tensor -- in both layouts,
(N,3,H,W) and (N,H,W,3), through every stem entry point, every tile order / LDS form, whole models, one native train step and
extract_features end to end. Outputs are NaN-poisoned before the launch: an element a kernel does not write shows up."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bounds import poisoned_outputs
from lp16 import LP16, LP_DTYPE
from recipe import recipe_state_dict, synthetic_adj, synthetic_clips
from torchreid import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER = ((0.41, 0.5, 0.37), (0.31, 0.2, 0.27))   # a non-default mean / std
LAYOUTS = ("nchw", "nhwc")


def random_frames(shape, seed):
    """uint8 (N,3,H,W) on the CPU."""
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def as_layout(u8, layout):
    """channel-first uint8 (...,3,H,W) -> the same frames in ``layout``, contiguous."""
    return u8.contiguous() if layout == "nchw" else u8.movedim(-3, -1).contiguous()


# ---- agrl_frames_normalize_u8 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [None, OTHER])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", [(256, 128), (224, 112), (37, 23)])
def test_frames_normalize_is_the_table_bit_for_bit(size, layout, norm):
    from torchreid import hip_ops as ops
    H, W = size
    u8 = random_frames((5, 3, H, W), H + W)
    args = norm if norm is not None else ()
    ref = ops.frame_table(*args)[torch.arange(3).view(1, 3, 1, 1), u8.long()]
    assert torch.equal(ref, ops.frames_normalize_reference(u8, *args))
    d = as_layout(u8, layout).to(DEV)
    with poisoned_outputs():
        out = ops.frames_normalize(d, *args)
    torch.cuda.synchronize()
    assert out.shape == (5, 3, H, W) and out.dtype == torch.float32 and torch.equal(out.cpu(), ref)
    # a source that is not 4-byte aligned (a view one byte into a buffer) takes the element-wise form: the same values
    buf = torch.zeros(d.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = d.reshape(-1)
    odd = buf[1:].view(d.shape)
    assert odd.data_ptr() % 4 != 0 and odd.is_contiguous()
    with poisoned_outputs():
        out2 = ops.frames_normalize(odd, *args)
    torch.cuda.synchronize()
    assert torch.equal(out2.cpu(), ref)


# ---- the three stems ----------------------------------------------------------------------------------------------------------------
def stem_launcher(entry, seed):
    """-> f(frames): one of the three stem entry points on fixed random weights; frames fp32 NCHW or uint8 in either layout."""
    from torchreid import hip_ops as ops
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn((64, 3, 7, 7), generator=g) * 0.1).permute(0, 2, 3, 1).contiguous().to(DEV)
    b = (torch.randn((64,), generator=g) * 0.1).to(DEV)
    if entry == "lp16":
        wpk = ops.pack_stem_weights_lp16(w)
        return lambda x, *norm: ops.stem_lp16(x, wpk, b, *norm)
    if entry == "split16":
        wh, wl, unscale = ops.pack_stem_weights_split16(w)
        return lambda x, *norm: ops.stem_split16(x, wh, wl, unscale, b, *norm)
    out_dtype = {"fp32": torch.float32, "fp32_out16": LP_DTYPE}[entry]
    return lambda x, *norm: ops.stem(x, w, b, out_dtype, *norm)


def frame_cases():
    return [
        ("n256", lambda: random_frames((256, 3, 256, 128), 1)),   # the benchmarked dispatch
        ("n3", lambda: random_frames((3, 3, 256, 128), 2)),       # per-XCD tile order off
        ("n10", lambda: random_frames((10, 3, 64, 48), 3)),       # uneven XCD shares
        ("n33", lambda: random_frames((33, 3, 256, 128), 4)),
        ("ragged", lambda: random_frames((9, 3, 37, 29), 5)),     # ragged tiles, all four borders
        ("all0", lambda: torch.zeros((8, 3, 64, 48), dtype=torch.uint8)),
        ("all255", lambda: torch.full((8, 3, 64, 48), 255, dtype=torch.uint8)),
    ]


def check_stem_entry(entry, case, monkeypatch, norm=()):
    from torchreid import hip_ops as ops
    u8 = dict(frame_cases())[case]()
    run = stem_launcher(entry, 11)
    x32 = ops.frames_normalize_reference(u8, *norm).to(DEV)
    forms = [{}, {"AGRL_STEM_XCD_MAP": "0"}, {"AGRL_STEM_SPLIT_LDS": "0"}]
    for env in forms:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _hip.reload_options()
        with poisoned_outputs():
            ref = run(x32)
        torch.cuda.synchronize()
        assert torch.isfinite(ref).all() and float(ref.float().abs().max()) > 0
        for layout in LAYOUTS:
            d = as_layout(u8, layout).to(DEV)
            with poisoned_outputs():
                got = run(d, *norm)
            torch.cuda.synchronize()
            assert got.dtype == ref.dtype and got.shape == ref.shape
            assert torch.equal(got, ref), "%s %s %s %s: %d of %d elements differ" % (
                entry, case, layout, env, int((got != ref).sum()), ref.numel())
        for k in env:
            monkeypatch.delenv(k)
        _hip.reload_options()


CASES = [c for c, _ in frame_cases()]


@pytest.mark.parametrize("case", CASES)
def test_stem_lp16_u8_equals_its_fp32_launch(case, monkeypatch):
    check_stem_entry("lp16", case, monkeypatch)


@pytest.mark.parametrize("case", CASES)
def test_stem_split16_u8_equals_its_fp32_launch(case, monkeypatch):
    check_stem_entry("split16", case, monkeypatch)


@pytest.mark.parametrize("case", CASES)
def test_stem_fp32_u8_equals_its_fp32_launch(case, monkeypatch):
    check_stem_entry("fp32", case, monkeypatch)


@pytest.mark.parametrize("entry", ["lp16", "split16", "fp32", "fp32_out16"])
def test_stem_u8_with_other_constants_and_16_bit_output(entry, monkeypatch):
    """A non-default mean / std reaches every kernel (the device table is cached per triple), and the fp32 stem's 16-bit output form."""
    check_stem_entry(entry, "ragged", monkeypatch, OTHER)
    check_stem_entry(entry, "n10", monkeypatch)


def test_stem_u8_rejects_what_it_cannot_read():
    from torchreid import hip_ops as ops
    run = stem_launcher("lp16", 11)
    with pytest.raises(ValueError):
        run(torch.zeros((4, 4, 64, 48), dtype=torch.uint8, device=DEV))
    table = torch.zeros((3, 257), device=DEV)
    x = torch.zeros((2, 3, 64, 48), dtype=torch.uint8, device=DEV)
    out = torch.zeros((2, 16, 12, 64), dtype=torch.float32, device=DEV)
    with pytest.raises(_hip.HipKernelError, match="bad layout"):
        _hip.call("agrl_frames_normalize_u8", x.data_ptr(), table.data_ptr(), 2, out.data_ptr(), 2, 64, 48, _hip.stream_ptr(x.device))
    with pytest.raises(_hip.HipKernelError, match="null"):
        _hip.call("agrl_frames_normalize_u8", x.data_ptr(), None, 0, out.data_ptr(), 2, 64, 48, _hip.stream_ptr(x.device))
    assert ops.frames_layout((2, 3, 64, 48)) == "nchw" and ops.frames_layout((2, 64, 48, 3)) == "nhwc"


# ---- whole models -------------------------------------------------------------------------------------------------------------------
KW = dict(num_classes=5, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1, pyramid_part=True,
          use_pose=True, learn_graph=True)
MODELS = {"vmgn": {}, "gsta": dict(pretrained=False), "ganet": dict(knn=4, pretrained=False)}


def build(name, **kw):
    from torchreid import models
    m = models.init_model(name, **dict(KW, **dict(MODELS[name], **kw)))
    m.load_state_dict(recipe_state_dict(m.state_dict(), seed=0))
    return m.eval()


def uint8_clips(B, S, H=256, W=128, seed=0, identities=None):
    """The recipe's identity-patterned clips as a decoder would hand them over: uint8 (B,S,3,H,W)."""
    x = synthetic_clips(B, S, H=H, W=W, seed=seed, identities=identities)
    return (x * 48.0 + 128.0).round().clamp(0, 255).to(torch.uint8)


def check_model(m, B, S, precisions):
    from torchreid import hip_ops as ops
    u8 = uint8_clips(B, S, seed=B + S)
    adj = synthetic_adj(B, S, seed=B + S).to(DEV)
    x32 = ops.frames_normalize_reference(u8).to(DEV)
    for precision in precisions:
        m.hip_precision = precision
        with poisoned_outputs():
            ref = m(x32, adj)
        torch.cuda.synchronize()
        assert torch.isfinite(ref).all()
        for layout in LAYOUTS:
            d = as_layout(u8, layout).to(DEV)
            with poisoned_outputs():
                got = m(d, adj)
            torch.cuda.synchronize()
            assert torch.equal(got, ref), "%s %s B=%d S=%d: %d of %d elements differ" % (
                precision, layout, B, S, int((got != ref).sum()), ref.numel())
    # the model's own constants are the ones applied
    m.pixel_mean, m.pixel_std = OTHER
    got = m(u8.to(DEV), adj)
    assert torch.equal(got, m(ops.frames_normalize_reference(u8, *OTHER).to(DEV), adj)) and not torch.equal(got, ref)


@pytest.mark.parametrize("B,S", [(32, 8), (2, 4)])
def test_vmgn_eval_from_uint8_is_bitwise_the_fp32_forward(B, S):
    check_model(build("vmgn").to(DEV), B, S, ["fp32", LP16, "bf16x3", "fp16x3"])


@pytest.mark.parametrize("name", ["gsta", "ganet"])
def test_sibling_models_eval_from_uint8(name):
    check_model(build(name).to(DEV), 2, 4, ["fp32", LP16])


def test_model_dtype_and_shape_errors_on_the_gpu():
    m = build("vmgn").to(DEV)
    adj = synthetic_adj(2, 4, seed=1).to(DEV)
    for dtype in (torch.int16, torch.float64):
        with pytest.raises(TypeError, match="frames must be float32"):
            m(torch.zeros((2, 4, 3, 64, 32), dtype=dtype, device=DEV), adj)
    with pytest.raises(ValueError):
        m(torch.zeros((2, 4, 4, 64, 32), dtype=torch.uint8, device=DEV), adj)


def test_native_train_step_from_uint8_frames():
    """Training normalises first (agrl_frames_normalize_u8), then runs exactly the fp32 step: the same loss and the same gradients."""
    from torchreid import hip_ops as ops, losses
    P, K, S = 2, 2, 4
    pids = torch.arange(P).repeat_interleave(K)
    u8 = uint8_clips(P * K, S, H=128, W=64, seed=9, identities=pids.tolist())
    adj = synthetic_adj(P * K, S, seed=9).to(DEV)
    y = pids.to(DEV)
    m = build("vmgn", consistent_loss=False).to(DEV)
    assert m.hip_train and m.hip_train_tail
    ce = losses.CrossEntropyLabelSmooth(num_classes=5, use_gpu=True)
    htri = losses.TripletLoss(margin=0.3, soft=True)

    def step(x):
        m.train()
        torch.manual_seed(1234)
        outs, feats = m(x, adj)
        loss = losses.DeepSupervision(ce, outs, y) + losses.DeepSupervision(htri, feats, y)
        m.zero_grad()
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}

    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    loss32, grads32 = step(ops.frames_normalize_reference(u8).to(DEV))
    again, grads_again = step(ops.frames_normalize_reference(u8).to(DEV))   # running statistics moved; the step itself does not read them
    assert len(grads32) > 100 and torch.isfinite(loss32)
    repeatable = torch.equal(loss32, again) and all(torch.equal(grads32[k], grads_again[k]) for k in grads32)
    assert repeatable, "the fp32 step is not bitwise repeatable: the uint8 comparison below would not mean anything"
    for layout in LAYOUTS:
        m.load_state_dict(sd)
        loss8, grads8 = step(as_layout(u8, layout).to(DEV))
        assert torch.equal(loss8, loss32), (layout, float(loss8), float(loss32))
        assert grads8.keys() == grads32.keys()
        bad = [k for k in grads32 if not torch.equal(grads8[k], grads32[k])]
        assert not bad, (layout, bad[:5])


# ---- extract_features end to end ----------------------------------------------------------------------------------------------------
N_ID, S_E = 6, 4


def eval_batches(pids, cams, seed, dtype, dense=0, layout="nchw", bs=6):
    """Host batches as a loader yields them: uint8 (as decoded) or the table-normalised fp32 of the same frames; ``dense`` clips per tracklet."""
    from torchreid import hip_ops as ops
    n = max(dense, 1)
    for i in range(0, len(pids), bs):
        sl = slice(i, i + bs)
        b = len(pids[sl])
        idents = [int(p) for p in pids[sl] for _ in range(n)]
        u8 = uint8_clips(b * n, S_E, seed=seed + i, identities=idents)
        adj = synthetic_adj(b * n, S_E, seed=seed + i)
        x = as_layout(u8, layout) if dtype == torch.uint8 else ops.frames_normalize_reference(u8)
        if dense:
            x, adj = x.view((b, n) + tuple(x.shape[1:])), adj.view((b, n) + tuple(adj.shape[1:]))
        yield x.pin_memory(), pids[sl], cams[sl], adj


@pytest.mark.parametrize("dense,layout", [(0, "nchw"), (0, "nhwc"), (2, "nhwc"), (2, "nchw")])
@pytest.mark.parametrize("precision", ["fp32", LP16])
def test_extract_features_from_uint8_host_batches(dense, layout, precision):
    from torchreid import evaluation
    m = build("vmgn", num_classes=N_ID).to(DEV)
    m.hip_precision = precision
    q_pids, q_cams = np.arange(N_ID), np.zeros(N_ID, dtype=np.int64)
    g_pids, g_cams = np.repeat(np.arange(N_ID), 3), np.tile(np.arange(1, 4), N_ID)
    res = {}
    for dtype in (torch.float32, torch.uint8):
        qf, qp, qc = evaluation.extract_features(m, eval_batches(q_pids, q_cams, 100, dtype, dense, layout))
        gf, gp, gc = evaluation.extract_features(m, eval_batches(g_pids, g_cams, 500, dtype, dense, layout))
        assert qf.shape == (N_ID, 4096) and gf.shape == (3 * N_ID, 4096) and np.array_equal(gp, g_pids) and np.array_equal(qc, q_cams)
        cmc, mAP = evaluation.match_and_rank(qf, qp, qc, gf, gp, gc, "cosine", 10, precision)
        res[dtype] = (qf, gf, cmc, mAP)
    a, b = res[torch.float32], res[torch.uint8]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert np.array_equal(a[2], b[2]) and a[3] == b[3]
    print("extract_features uint8 %s dense=%d %s: Rank-1 %.3f mAP %.4f, identical to the fp32 run" % (layout, dense, precision, b[2][0], b[3]))


# ---- the other build ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(os.environ.get("AGRL_HIP_LP16", "fp16") == "bf16", reason="this process already runs the bf16 build")
def test_bf16_build_passes_the_16_bit_stem_tests_in_a_fresh_process():
    """libagrl_hip_bf16.so instantiates the same uint8 staging in front of bf16 MFMAs: this file's 16-bit stem tests in a FRESH CHILD
    interpreter (the 16-bit type is fixed when torchreid is imported) -- started with subprocess, never a re-exec of a process that has
    touched the GPU."""
    lib = os.path.join(ROOT, "agrl.pytorch_amd", "lib", "libagrl_hip_bf16.so")
    assert os.path.exists(lib), "libagrl_hip_bf16.so is not built (make -C agrl.pytorch_amd/csrc)"
    env = dict(os.environ, AGRL_HIP_LP16="bf16")
    env.pop("AGRL_HIP_LIB", None)
    env.pop("AGRL_HIP_PRECISION", None)
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_u8_ingest.py",
                          "-k", "test_stem_lp16_u8_equals_its_fp32_launch or test_stem_u8_with_other_constants_and_16_bit_output"],
                         env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    tail = out.stdout.decode()[-3000:]
    print(tail)
    assert out.returncode == 0 and " passed" in tail and "skipped" not in tail, tail
    probe = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, 'tests'); import lp16; from torchreid import _hip; "
                            "_hip.lib(); print(_hip.LP_NAME, _hip.LIB_PATH)"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=600)
    assert probe.returncode == 0 and "bf16 " in probe.stdout.decode() and "libagrl_hip_bf16.so" in probe.stdout.decode(), probe.stdout.decode() + probe.stderr.decode()[-2000:]
