"""agrl_clip_resample_u8 on the GPU: resize / crop / flip of uint8 clips, BITWISE Pillow's bytes. Every comparison is torch.equal /
array_equal -- against the Pillow fixture (tests/golden/clip_resample.npz), against hip_ops.clip_resample_reference (which
tests/test_clip_resample.py pins on Pillow), and end to end: a model, extract_features(frame_size=...) and the native train step give
exactly what they give on clips resampled on the CPU beforehand. Outputs are poisoned before every launch."""
import os

import numpy as np
import pytest
import torch

from bounds import poisoned_outputs
from lp16 import LP16
from recipe import recipe_state_dict, synthetic_adj, synthetic_clips
from torchreid import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_resample.npz")
CASES = ("identity_32x16", "window_30x15_at_1_1", "upscale_16x8", "odd_19x11", "down_37x23", "down_70x50", "one_pixel",
         "horizontal_only_32x20", "vertical_only_40x16", "flip_37x23", "misalign_pad_top", "misalign_pad_bottom", "checker_37x23")


def load_case(name):
    with np.load(GOLDEN) as z:
        return (torch.from_numpy(z[name + ".frames"]), z[name + ".geometry"], tuple(int(v) for v in z[name + ".out_hw"]),
                torch.from_numpy(z[name + ".expected"]))


def noise(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def whole(N, h, w, flip=0):
    return np.array([[h, w, 0, 0, h, w, flip, 0]] * N, dtype=np.int32)


def run(frames_dev, geometry, out_hw, **kw):
    from torchreid import hip_ops as ops
    with poisoned_outputs():
        out = ops.clip_resample(frames_dev, geometry, out_hw, **kw)
    torch.cuda.synchronize()
    return out


def check(frames, geometry, out_hw, what):
    """frames uint8 on the CPU: the kernel's output == the reference's, byte for byte. Returns (reference, kernel output)."""
    from torchreid import hip_ops as ops
    ref = ops.clip_resample_reference(frames, geometry, out_hw)
    got = run(frames.to(DEV), geometry, out_hw)
    assert got.dtype == torch.uint8 and got.shape == ref.shape and got.is_cuda
    bad = got.cpu() != ref
    assert not bad.any(), "%s: %d of %d bytes differ, first at %s" % (what, int(bad.sum()), ref.numel(), bad.nonzero()[0].tolist())
    return ref, got


# ---- the taps: the device's fp64 against the host's --------------------------------------------------------------------------------
def test_device_taps_equal_the_host_taps():
    from torchreid import hip_ops as ops
    pairs = [(size, out) for out in (16, 32, 128, 256) for size in list(range(1, 301)) + [8 * out]]
    with poisoned_outputs():
        dev = [ops.resample_taps_device(size, out, DEV) for size, out in pairs]
    torch.cuda.synchronize()
    for (size, out), (k_d, b_d) in zip(pairs, dev):
        k, bounds = ops.resample_taps(size, out, ops.RESAMPLE_TAPS)
        assert np.array_equal(b_d.cpu().numpy(), bounds), (size, out)
        assert np.array_equal(k_d.cpu().numpy(), k), (size, out, int((k_d.cpu().numpy() != k).sum()))
        if size <= ops.RESAMPLE_MAX_SCALE * out:   # inside the kernel's capacity the 17 taps are the whole row
            full, fb = ops.resample_taps(size, out)
            assert np.array_equal(fb, bounds) and np.array_equal(k[:, :full.shape[1]], full[:, :17]) and not k[:, full.shape[1]:].any()
    k, bounds = ops.resample_taps(8 * 16, 16, ops.RESAMPLE_TAPS)
    assert bounds[:, 1].max() >= 16   # the edge of the capacity is reached


# ---- Pillow's bytes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_pillow_fixture(name):
    frames, g, out_hw, expected = load_case(name)
    got = run(frames.to(DEV), g, out_hw).cpu()
    assert got.shape == expected.shape
    assert torch.equal(got, expected), "%s: %d of %d bytes differ from Pillow's" % (name, int((got != expected).sum()), expected.numel())


# ---- further shapes, against the reference -------------------------------------------------------------------------------------------
def test_random_crop_windows_to_the_model_size():
    rng = np.random.default_rng(3)
    g = whole(5, 256, 128)
    g[:, 2], g[:, 3], g[:, 4], g[:, 5] = rng.integers(0, 17, 5), rng.integers(0, 9, 5), 240, 120
    g[3:, 6] = 1
    g[0, 2:4], g[1, 2:4] = (0, 0), (16, 8)
    check(noise((5, 256, 128, 3), 11), g, (256, 128), "240x120 windows -> 256x128")


def test_eightfold_downscale():
    check(noise((3, 256, 128, 3), 12), whole(3, 256, 128), (32, 16), "256x128 -> 32x16")
    g = whole(2, 256, 128)
    g[1] = (256, 128, -4, -3, 256, 128, 1, 0)   # 17-tap rows, reaching outside the frame, mirrored
    check(noise((2, 256, 128, 3), 13), g, (32, 16), "8 x with edge replication")


def test_upscale_to_the_model_size_and_a_wide_output():
    check(noise((3, 128, 64, 3), 14), whole(3, 128, 64), (256, 128), "128x64 -> 256x128")
    check(noise((2, 40, 300, 3), 15), whole(2, 40, 300, 1), (37, 510), "40x300 -> 37x510, flipped")   # 8 column tiles, ragged last tile
    check(noise((2, 33, 9, 3), 16), whole(2, 33, 9), (5, 3), "33x9 -> 5x3")                           # 45-byte output frames


def test_slivers_whose_pass_order_does_not_show():
    """More than 100 times as tall as wide, where Pillow runs the vertical pass first: accepted when the horizontal pass copies (one
    column) or is skipped (as wide as the output); the reference, which follows Pillow's order, and the kernel agree."""
    check(noise((2, 201, 1, 3), 31), whole(2, 201, 1), (32, 16), "201x1 -> 32x16")
    check(noise((1, 2001, 16, 3), 32), whole(1, 2001, 16, 1), (251, 16), "2001x16 -> 251x16, flipped")


def test_ragged_batch_never_reads_the_padding():
    from torchreid import hip_ops as ops
    extents = ((70, 50), (37, 23), (19, 11), (1, 1))
    g = np.concatenate([whole(1, h, w) for h, w in extents])
    frames = noise((4, 70, 50, 3), 17)
    outs = []
    for fill in (0x00, 0xC3):
        box = frames.clone()
        for n, (h, w) in enumerate(extents):
            box[n, h:] = fill
            box[n, :, w:] = fill
        ref, got = check(box, g, (32, 16), "ragged batch, padding %#x" % fill)
        outs.append(got.cpu())
    assert torch.equal(outs[0], outs[1])
    for n, (h, w) in enumerate(extents):   # and each frame is what it is alone
        alone = ops.clip_resample_reference(frames[n:n + 1, :h, :w].contiguous(), whole(1, h, w), (32, 16))
        assert torch.equal(outs[0][n], alone[0])


@pytest.mark.parametrize("Ws", [23, 50])
def test_unaligned_sources(Ws):
    """69-byte rows (Ws = 23), and a source one byte into its buffer: the dword loads follow the actual address."""
    from torchreid import hip_ops as ops
    frames = noise((3, 37, Ws, 3), 18 + Ws)
    g = whole(3, 37, Ws)
    g[2] = (37, Ws, 2, 1, 30, Ws - 3, 1, 0)
    ref, _ = check(frames, g, (32, 16), "Ws=%d" % Ws)
    buf = torch.zeros(frames.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = frames.to(DEV).reshape(-1)
    odd = buf[1:].view(frames.shape)
    assert odd.data_ptr() % 2 == 1 and odd.is_contiguous()
    assert torch.equal(run(odd, g, (32, 16)).cpu(), ref)


@pytest.mark.parametrize("out_hw", [(32, 16), (5, 3)])
def test_output_guard_bytes_stay_intact(out_hw):
    from torchreid import hip_ops as ops
    frames = noise((3, 37, 23, 3), 21)
    g = whole(3, 37, 23)
    ref = ops.clip_resample_reference(frames, g, out_hw)
    n = ref.numel()
    buf = torch.full((64 + n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    out = buf[64:64 + n].view(ref.shape)
    assert run(frames.to(DEV), g, out_hw, out=out) is out
    host = buf.cpu()
    assert torch.equal(host[64:64 + n].view(ref.shape), ref)
    assert (host[:64] == 0xA5).all() and (host[64 + n:] == 0xA5).all()


def test_two_runs_are_bitwise_equal():
    frames = noise((8, 128, 64, 3), 22).to(DEV)
    g = whole(8, 128, 64)
    g[::2, 6] = 1
    a = run(frames, g, (256, 128)).clone()
    b = run(frames, g, (256, 128))
    assert torch.equal(a, b)


# ---- the C ABI's own checks ----------------------------------------------------------------------------------------------------------
def test_cabi_rejects_what_it_cannot_do():
    from torchreid import hip_ops as ops
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    g = torch.from_numpy(whole(1, 8, 8)).to(DEV)
    out = torch.zeros((1, 512, 512, 3), dtype=torch.uint8, device=DEV)
    s = _hip.stream_ptr(x.device)
    for args in ((None, g.data_ptr(), out.data_ptr()), (x.data_ptr(), None, out.data_ptr()), (x.data_ptr(), g.data_ptr(), None)):
        with pytest.raises(_hip.HipKernelError, match="null pointer"):
            _hip.call("agrl_clip_resample_u8", *args, 1, 8, 8, 32, 16, s)
    with pytest.raises(_hip.HipKernelError, match="output size 0x16"):
        _hip.call("agrl_clip_resample_u8", x.data_ptr(), g.data_ptr(), out.data_ptr(), 1, 8, 8, 0, 16, s)
    with pytest.raises(_hip.HipKernelError, match="output size 32x513"):
        _hip.call("agrl_clip_resample_u8", x.data_ptr(), g.data_ptr(), out.data_ptr(), 1, 8, 8, 32, 513, s)
    with pytest.raises(_hip.HipKernelError, match="bad shape"):
        _hip.call("agrl_clip_resample_u8", x.data_ptr(), g.data_ptr(), out.data_ptr(), 0, 8, 8, 32, 16, s)
    with pytest.raises(_hip.HipKernelError, match="null pointer"):
        _hip.call("agrl_resample_taps_u8", 8, 4, None, out.data_ptr(), s)
    with pytest.raises(_hip.HipKernelError, match="bad sizes"):
        _hip.call("agrl_resample_taps_u8", 0, 4, out.data_ptr(), out.data_ptr(), s)
    # the wrapper's host checks, on device frames
    with pytest.raises(ValueError, match="1..512"):
        ops.clip_resample(x, whole(1, 8, 8), (32, 513))
    with pytest.raises(ValueError, match="frame 0 has a window of 8 x 129, more than 8 times"):
        ops.clip_resample(x, np.array([[8, 8, 0, 0, 8, 129, 0, 0]], dtype=np.int32), (32, 16))
    with pytest.raises(ValueError, match="frame 0 has a valid extent of 9 x 8"):
        ops.clip_resample(x, whole(1, 9, 8), (32, 16))
    with pytest.raises(ValueError, match="contiguous"):
        ops.clip_resample(torch.zeros((1, 8, 16, 3), dtype=torch.uint8, device=DEV)[:, :, ::2], whole(1, 8, 8), (32, 16))
    with pytest.raises(ValueError, match="host array"):
        ops.clip_resample(x, g, (32, 16))
    out = ops.clip_resample(x, whole(1, 8, 8), (512, 512))   # the largest output
    torch.cuda.synchronize()
    assert out.shape == (1, 512, 512, 3) and not out.any()


# ---- whole models ------------------------------------------------------------------------------------------------------------------
KW = dict(num_classes=5, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1, pyramid_part=True,
          use_pose=True, learn_graph=True)


def build(**kw):
    from torchreid import models
    m = models.init_model("vmgn", **dict(KW, **kw))
    m.load_state_dict(recipe_state_dict(m.state_dict(), seed=0))
    return m.eval()


def uint8_clips(B, S, H, W, seed=0, identities=None):
    """The recipe's identity-patterned clips as a decoder hands them over: uint8 channel-last (B,S,H,W,3)."""
    x = synthetic_clips(B, S, H=H, W=W, seed=seed, identities=identities)
    return (x * 48.0 + 128.0).round().clamp(0, 255).to(torch.uint8).movedim(-3, -1).contiguous()


def resampled_on_the_cpu(clips, geometry, out_hw):
    from torchreid import hip_ops as ops
    B, S = clips.shape[:2]
    out = ops.clip_resample_reference(clips.reshape((B * S,) + tuple(clips.shape[2:])), np.asarray(geometry).reshape(B * S, 8), out_hw)
    return out.view(B, S, out_hw[0], out_hw[1], 3)


def test_vmgn_on_device_resampled_clips():
    from torchreid.device_transforms import DeviceClipTransform, eval_geometry
    m = build().to(DEV)
    x = uint8_clips(2, 4, 128, 64, seed=6)
    adj = synthetic_adj(2, 4, seed=6).to(DEV)
    t = DeviceClipTransform(256, 128)
    ref_clips = resampled_on_the_cpu(x, eval_geometry(np.full((2, 4, 2), (128, 64))), (256, 128))
    for precision in ("fp32", LP16):
        m.hip_precision = precision
        with poisoned_outputs():
            got_clips = t(x.to(DEV))
            got = m(got_clips, adj)
        ref = m(ref_clips.to(DEV), adj)
        torch.cuda.synchronize()
        assert got_clips.shape == (2, 4, 256, 128, 3) and torch.equal(got_clips.cpu(), ref_clips)
        assert torch.isfinite(ref).all() and torch.equal(got, ref), precision


# ---- extract_features(frame_size=...) ------------------------------------------------------------------------------------------------
N_ID, S_E = 6, 4


def eval_batches(pids, cams, seed, variant, resized, bs=6):
    """Host batches of 128x64 uint8 channel-last clips. 'dense': two clips per tracklet, (b,2,S,128,64,3); 'ragged': 5-tuples whose last
    element gives each frame's valid extent inside the 128x64 container. ``resized``: the same batches resampled to 256x128 on the CPU
    beforehand, as 4-tuples."""
    n = 2 if variant == "dense" else 1
    for i in range(0, len(pids), bs):
        sl = slice(i, i + bs)
        b = len(pids[sl])
        idents = [int(p) for p in pids[sl] for _ in range(n)]
        u8 = uint8_clips(b * n, S_E, 128, 64, seed=seed + i, identities=idents)
        adj = synthetic_adj(b * n, S_E, seed=seed + i)
        sizes = np.full((b * n, S_E, 2), (128, 64), dtype=np.int64)
        if variant == "ragged":
            rng = np.random.default_rng(seed + i)
            sizes[..., 0], sizes[..., 1] = rng.integers(90, 129, (b, S_E)), rng.integers(40, 65, (b, S_E))
            sizes[0, 0] = (128, 64)
            for c in range(b):
                for f in range(S_E):
                    u8[c, f, sizes[c, f, 0]:] = 0x77   # container padding: must not matter
                    u8[c, f, :, sizes[c, f, 1]:] = 0x77
        if resized:
            from torchreid.device_transforms import eval_geometry
            u8 = resampled_on_the_cpu(u8, eval_geometry(sizes), (256, 128))
        x = u8.view((b, n) + tuple(u8.shape[1:])) if n > 1 else u8
        adj = adj.view((b, n) + tuple(adj.shape[1:])) if n > 1 else adj
        item = (x.pin_memory(), pids[sl], cams[sl], adj)
        yield item + (sizes.reshape((b, n, S_E, 2)) if n > 1 else sizes,) if variant == "ragged" and not resized else item


@pytest.mark.parametrize("variant", ["dense", "ragged"])
def test_extract_features_resamples_raw_frames(variant):
    from torchreid import evaluation
    m = build(num_classes=N_ID).to(DEV)
    q_pids, q_cams = np.arange(N_ID), np.zeros(N_ID, dtype=np.int64)
    g_pids, g_cams = np.repeat(np.arange(N_ID), 3), np.tile(np.arange(1, 4), N_ID)
    res = {}
    for resized in (True, False):
        qf, qp, qc = evaluation.extract_features(m, eval_batches(q_pids, q_cams, 100, variant, resized), frame_size=(256, 128))
        gf, gp, gc = evaluation.extract_features(m, eval_batches(g_pids, g_cams, 500, variant, resized), frame_size=(256, 128))
        assert qf.shape == (N_ID, 4096) and gf.shape == (3 * N_ID, 4096) and np.array_equal(gp, g_pids) and np.array_equal(qc, q_cams)
        cmc, mAP = evaluation.match_and_rank(qf, qp, qc, gf, gp, gc, "cosine", 10, "fp32")
        res[resized] = (qf, gf, cmc, mAP)
    a, b = res[True], res[False]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert np.array_equal(a[2], b[2]) and a[3] == b[3]
    # frames already at the model's size pass through frame_size untouched, and the default takes them as before
    qf2, _, _ = evaluation.extract_features(m, eval_batches(q_pids, q_cams, 100, variant, True))
    assert torch.equal(qf2, a[0])


def test_extract_features_refuses_what_it_cannot_resample():
    from torchreid import evaluation
    m = build(num_classes=N_ID).to(DEV)
    adj = synthetic_adj(2, S_E, seed=1)
    pids, cams = np.arange(2), np.zeros(2, dtype=np.int64)
    for imgs in (torch.zeros((2, S_E, 3, 128, 64), dtype=torch.uint8), torch.zeros((2, S_E, 3, 128, 64), dtype=torch.float32),
                 torch.zeros((2, S_E, 128, 64, 3), dtype=torch.float32)):
        with pytest.raises(ValueError, match="cannot be resampled"):
            evaluation.extract_features(m, [(imgs, pids, cams, adj)], frame_size=(256, 128))
    with pytest.raises(ValueError, match="needs frame_size"):
        evaluation.extract_features(m, [(torch.zeros((2, S_E, 128, 64, 3), dtype=torch.uint8), pids, cams, adj, np.zeros((2, S_E, 2), dtype=np.int64))])


# ---- the native train step ----------------------------------------------------------------------------------------------------------
def test_native_train_step_on_device_augmented_clips():
    """transform_train's random crop + flip as geometry, resampled on the device to the 128x64 the train-step tests use: the same
    loss and the same gradients as from the clips resampled on the CPU."""
    from torchreid import losses
    from torchreid.device_transforms import DeviceClipTransform
    P, K, S = 2, 2, 4
    pids = torch.arange(P).repeat_interleave(K)
    raw = uint8_clips(P * K, S, 256, 128, seed=9, identities=pids.tolist())
    adj = synthetic_adj(P * K, S, seed=9).to(DEV)
    y = pids.to(DEV)
    t = DeviceClipTransform(128, 64, train=True, rng=5, rand_crop=True, flip=True)
    with poisoned_outputs():
        x_dev = t(raw.to(DEV))
    geo = t.last_geometry
    assert geo.shape == (P * K, S, 8) and (geo[..., 4] == 240).all() and (geo[..., 5] == 120).all() and len(np.unique(geo[..., 6])) == 2
    assert len({tuple(r) for r in geo[:, 0, 2:4].tolist()}) > 1, "the clips drew different crop offsets"
    x_cpu = resampled_on_the_cpu(raw, geo, (128, 64))
    torch.cuda.synchronize()
    assert torch.equal(x_dev.cpu(), x_cpu)
    m = build(consistent_loss=False).to(DEV)
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
    loss_ref, grads_ref = step(x_cpu.to(DEV))
    m.load_state_dict(sd)
    loss_dev, grads_dev = step(x_dev)
    assert len(grads_ref) > 100 and torch.isfinite(loss_ref)
    assert torch.equal(loss_dev, loss_ref), (float(loss_dev), float(loss_ref))
    assert grads_dev.keys() == grads_ref.keys()
    bad = [k for k in grads_ref if not torch.equal(grads_dev[k], grads_ref[k])]
    assert not bad, bad[:5]
