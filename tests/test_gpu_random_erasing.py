"""agrl_frames_normalize_erase_u8 on the GPU: uint8 frames normalised and randomly erased in one pass. Every comparison is torch.equal
against hip_ops.frames_normalize_erase_reference (which tests/test_random_erasing.py pins on the reference's GroupRandomErasing /
RandomErasing outputs): the operation is a table look-up or a constant. Outputs are NaN-poisoned before every launch."""
import numpy as np
import pytest
import torch

from bounds import poisoned_outputs
from torchreid import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("nchw", "nhwc")
# 256x128: the model's size, eight workgroups per frame; 4x6 and 6x6: H W % 4 == 0 with W % 4 != 0, a thread's four pixels straddle
# rows; 8x4: one row per thread; 37x23: H W % 4 != 0, the element-wise form; 1x9: every drawn rectangle has height 0
SHAPES = ((256, 128), (4, 6), (6, 6), (8, 4), (37, 23), (1, 9))
OTHER = ((0.41, 0.5, 0.37), (0.31, 0.2, 0.27))   # a non-default mean / std
VALUE = (0.25, -1.5, 3.0)
IMAX, IMIN = 2 ** 31 - 1, -2 ** 31


def random_frames(shape, seed):
    """uint8 (N,3,H,W) on the CPU."""
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def as_layout(u8, layout):
    return u8.contiguous() if layout == "nchw" else u8.movedim(-3, -1).contiguous()


def run(frames_dev, rects, counts, *args):
    from torchreid import hip_ops as ops
    with poisoned_outputs():
        out = ops.frames_normalize_erase(frames_dev, rects, counts, *args)
    torch.cuda.synchronize()
    return out


def check(u8, layout, rects, counts, what, *args):
    """u8 (N,3,H,W) on the CPU: the kernel's output == the reference's, bit for bit. Returns the reference."""
    from torchreid import hip_ops as ops
    ref = ops.frames_normalize_erase_reference(u8, rects, counts, *args)
    got = run(as_layout(u8, layout).to(DEV), rects, counts, *args)
    assert got.dtype == torch.float32 and got.shape == ref.shape and got.is_cuda
    bad = ~((got.cpu() == ref) & ~torch.isnan(got.cpu()))
    assert not bad.any(), "%s: %d of %d elements differ, first at %s" % (what, int(bad.sum()), ref.numel(), bad.nonzero()[0].tolist())
    return ref


def hand_made(H, W, R):
    """Five frames, counts [0, 1, R, 3, 0] (3 cut to R), rows (y, x, h, w); GARBAGE behind every frame's count."""
    inner = (H // 4, W // 4, H // 2, W // 2)
    pool = [(0, 0, 1, W),                       # the top border = a full-width row
            (0, 0, H, 1),                       # the left border, full height
            (H - 1, 0, 1, W), (0, W - 1, H, 1),   # bottom and right borders
            (H - 1, W - 1, 1, 1),               # the last pixel alone
            (H // 2, 0, 0, W), (0, W // 2, H, 0), (H, W, 0, 0),   # zero-sized: erase nothing
            inner, (inner[0], inner[1], inner[2] // 2, inner[3] // 2), inner,   # nested, and a duplicate
            (0, 0, 1, 1)]
    garbage = [(0, 0, H, W), (IMIN, IMAX, IMAX, IMIN), (-5, 3, 1 << 30, -7), (IMAX, IMAX, IMAX, IMAX)]
    rects = np.array([[garbage[(n + i) % 4] for i in range(R)] for n in range(5)], dtype=np.int64)
    counts = np.array([0, 1, R, min(3, R), 0])
    rects[1, 0] = {1: (0, 0, H, W), 7: (H - 1, W - 1, 1, 1)}.get(R, (0, W - 1, H, 1))   # a full frame / the last pixel / the right border
    rects[2] = [pool[i % len(pool)] for i in range(R)]
    rects[3, :counts[3]] = [(H // 2, 0, 1, W), (0, 0, 0, 0), (0, 0, H, W)][:counts[3]]   # from R = 3 on the whole frame goes
    return rects, counts


@pytest.mark.parametrize("R", [1, 7, 128])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_kernel_on_hand_made_lists(hw, layout, R):
    from torchreid import hip_ops as ops
    H, W = hw
    u8 = random_frames((5, 3, H, W), H + W)
    rects, counts = hand_made(H, W, R)
    ref = check(u8, layout, rects, counts, "%dx%d %s R=%d" % (H, W, layout, R))
    norm = ops.frames_normalize_reference(u8)
    assert torch.equal(ref[0], norm[0]) and torch.equal(ref[4], norm[4]), "the garbage behind a count of 0 does not show"
    fill = torch.tensor(ops.PIXEL_MEAN).view(3, 1, 1)
    if R >= 3:
        assert torch.equal(ref[3], fill.expand(3, H, W))
    if R >= 7:
        assert torch.equal(ref[2, :, H - 1, W - 1], fill.view(3)) and torch.equal(ref[2, :, 0, :], fill.view(3, 1).expand(3, W))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_kernel_on_the_references_draws(hw, layout):
    """erase_geometry at probability 1: up to 100 rectangles a frame in the 'all' mode, one in the 'first' mode."""
    from torchreid import device_transforms as T
    H, W = hw
    u8 = random_frames((3, 3, H, W), 7 + H * W)
    for attempts in ("all", "first"):
        rects, counts = T.erase_geometry(3, H, W, np.random.default_rng(H), probability=1, attempts=attempts)
        assert counts.min() >= 1
        check(u8, layout, rects, counts, "%dx%d %s %s" % (H, W, layout, attempts))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", [(8, 4), (37, 23), (4, 6)], ids=lambda hw: "%dx%d" % hw)
def test_other_constants(hw, layout):
    from torchreid import hip_ops as ops
    H, W = hw
    u8 = random_frames((5, 3, H, W), 21)
    rects, counts = hand_made(H, W, 7)
    ref = check(u8, layout, rects, counts, "other constants", VALUE, *OTHER)
    assert not torch.equal(ref, ops.frames_normalize_erase_reference(u8, rects, counts))
    assert torch.equal(ref[1, :, H - 1, W - 1], torch.tensor(VALUE))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_unaligned_source_takes_the_elementwise_form(layout):
    from torchreid import device_transforms as T, hip_ops as ops
    u8 = random_frames((3, 3, 16, 8), 31)
    rects, counts = T.erase_geometry(3, 16, 8, 4, probability=1)
    ref = check(u8, layout, rects, counts, "aligned")
    d = as_layout(u8, layout).to(DEV)
    buf = torch.zeros(d.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = d.reshape(-1)
    odd = buf[1:].view(d.shape)
    assert odd.data_ptr() % 4 != 0 and odd.is_contiguous()
    assert torch.equal(run(odd, rects, counts).cpu(), ref)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", [(256, 128), (37, 23), (4, 6)], ids=lambda hw: "%dx%d" % hw)
def test_no_rectangles_is_frames_normalize_bit_for_bit(hw, layout):
    from torchreid import hip_ops as ops
    H, W = hw
    d = as_layout(random_frames((5, 3, H, W), 41), layout).to(DEV)
    with poisoned_outputs():
        plain = ops.frames_normalize(d)
    torch.cuda.synchronize()
    assert not torch.isnan(plain).any()
    empty = run(d, np.zeros((5, 0, 4), dtype=np.int32), np.zeros(5, dtype=np.int32))   # max_rects = 0: null lists
    assert torch.equal(empty, plain)
    garbage = hand_made(H, W, 7)[0]
    garbage[:] = garbage[0]
    assert torch.equal(run(d, garbage, np.zeros(5, dtype=np.int32)), plain)             # a list, every count 0


@pytest.mark.parametrize("offset", [64, 63])   # a 16-byte aligned output: the vectorised form; 63 floats in: the element-wise one
def test_two_launches_are_bitwise_equal_and_the_guard_stays(offset):
    from torchreid import hip_ops as ops
    H, W, N, R = 16, 8, 5, 7
    u8 = random_frames((N, 3, H, W), 51)
    rects, counts = hand_made(H, W, R)
    ref = ops.frames_normalize_erase_reference(u8, rects, counts)
    r, c = ops.erase_lists(rects, counts, N, H, W)
    x = u8.to(DEV)
    r_d, c_d = torch.from_numpy(r).to(DEV), torch.from_numpy(c).to(DEV)
    table = ops._device_frame_table(x.device, ops.PIXEL_MEAN, ops.PIXEL_STD)
    n = ref.numel()
    outs = []
    for _ in range(2):
        buf = torch.full((offset + n + 64,), -12345.0, dtype=torch.float32, device=DEV)
        out = buf[offset:offset + n]
        _hip.call("agrl_frames_normalize_erase_u8", x.data_ptr(), table.data_ptr(), _hip.FRAMES_NCHW, r_d.data_ptr(), c_d.data_ptr(), R,
                  *ops.PIXEL_MEAN, out.data_ptr(), N, H, W, _hip.stream_ptr(x.device))
        torch.cuda.synchronize()
        host = buf.cpu()
        assert (host[:offset] == -12345.0).all() and (host[offset + n:] == -12345.0).all()
        outs.append(host[offset:offset + n].view(ref.shape))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], ref)


def test_device_clip_transform_with_rand_erase():
    """transform_train with all four augmentation flags on a padded ragged batch: resample, then normalise + erase."""
    from torchreid import hip_ops as ops
    from torchreid.device_transforms import DeviceClipTransform
    B, S = 2, 3
    rng = np.random.default_rng(8)
    sizes = np.stack([rng.integers(34, 41, (B, S)), rng.integers(17, 25, (B, S))], -1)
    sizes[0, 0] = (40, 24)
    clips = random_frames((B, S, 40, 24, 3), 61)
    for b in range(B):
        for s in range(S):
            clips[b, s, sizes[b, s, 0]:] = 0x77   # container padding: must not matter
            clips[b, s, :, sizes[b, s, 1]:] = 0x77
    t = DeviceClipTransform(32, 16, train=True, misalign=True, rand_crop=True, crop_size=(30, 15), flip=True, rand_erase=True, rng=3)
    with poisoned_outputs():
        got = t(clips.to(DEV), sizes)
    torch.cuda.synchronize()
    rects, counts = t.last_erase
    assert got.dtype == torch.float32 and got.shape == (B, S, 3, 32, 16) and got.is_cuda
    assert rects.shape[:2] == counts.shape == (B, S) and t.last_geometry.shape == (B, S, 8)
    assert (counts == 0).any() and (counts > 1).any(), "the seed draws frames that are passed over and frames that are erased"
    resampled = ops.clip_resample_reference(clips.view(B * S, 40, 24, 3), t.last_geometry.reshape(B * S, 8), (32, 16))
    ref = ops.frames_normalize_erase_reference(resampled.view(B, S, 32, 16, 3), *t.last_erase)
    assert torch.equal(got.cpu(), ref)
    assert not torch.equal(ref, ops.frames_normalize_reference(resampled.view(B, S, 32, 16, 3)))
    # without the flag the transform still hands the uint8 clip over
    plain = DeviceClipTransform(32, 16, train=True, misalign=True, rand_crop=True, crop_size=(30, 15), flip=True, rng=3)
    out = plain(clips.to(DEV), sizes)
    assert out.dtype == torch.uint8 and out.shape == (B, S, 32, 16, 3) and plain.last_erase is None
    assert np.array_equal(plain.last_geometry, t.last_geometry), "the erase draws come after the clip geometry's"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_clips_to_float_with_erase_equals_the_cpu(layout):
    from torchreid import device_transforms as T, hip_ops as ops
    x = as_layout(random_frames((2, 3, 3, 16, 8), 71), layout)
    rects, counts = T.erase_geometry((2, 3), 16, 8, 6, probability=0.7)
    for erase in ((rects, counts), (rects, counts, VALUE)):
        cpu = ops.clips_to_float(x, *OTHER, erase=erase)
        with poisoned_outputs():
            got = ops.clips_to_float(x.to(DEV), *OTHER, erase=erase)
        torch.cuda.synchronize()
        assert got.is_cuda and got.shape == (2, 3, 3, 16, 8) and torch.equal(got.cpu(), cpu)
    assert torch.equal(ops.clips_to_float(x.to(DEV)).cpu(), ops.clips_to_float(x))


def test_cabi_rejects_what_it_cannot_do():
    from torchreid import hip_ops as ops
    x = torch.zeros((2, 3, 8, 4), dtype=torch.uint8, device=DEV)
    table = ops._device_frame_table(x.device, ops.PIXEL_MEAN, ops.PIXEL_STD)
    rects = torch.zeros((2, 3, 4), dtype=torch.int32, device=DEV)
    counts = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.full((2, 3, 8, 4), -12345.0, device=DEV)
    s = _hip.stream_ptr(x.device)

    def call(x_p, table_p, layout, rects_p, counts_p, max_rects, out_p):
        _hip.call("agrl_frames_normalize_erase_u8", x_p, table_p, layout, rects_p, counts_p, max_rects, 0.0, 0.0, 0.0, out_p, 2, 8, 4, s)

    good = (x.data_ptr(), table.data_ptr(), 0, rects.data_ptr(), counts.data_ptr(), 3, out.data_ptr())
    for i, match in ((0, "null pointer"), (1, "null table"), (3, "null pointer"), (4, "null pointer"), (6, "null pointer")):
        with pytest.raises(_hip.HipKernelError, match=match):
            call(*(None if j == i else v for j, v in enumerate(good)))
    with pytest.raises(_hip.HipKernelError, match="max_rects=129, 0..128"):
        call(*(129 if j == 5 else v for j, v in enumerate(good)))
    with pytest.raises(_hip.HipKernelError, match="max_rects=-1"):
        call(*(-1 if j == 5 else v for j, v in enumerate(good)))
    with pytest.raises(_hip.HipKernelError, match="bad layout 2"):
        call(*(2 if j == 2 else v for j, v in enumerate(good)))
    torch.cuda.synchronize()
    assert (out == -12345.0).all(), "a refused call launches nothing"
    call(*good)
    call(x.data_ptr(), table.data_ptr(), 0, None, None, 0, out.data_ptr())   # max_rects = 0 takes null lists
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ops.frames_normalize_reference(x.cpu()))
