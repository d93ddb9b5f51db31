"""Random erasing, the host side (no GPU): device_transforms.erase_geometry -- the reference's draws restated as geometry -- followed by
hip_ops.frames_normalize_erase_reference against the REFERENCE's own outputs (tests/golden/random_erasing.npz, written by
tests/golden/make_random_erasing_golden.py from GroupRandomErasing and RandomErasing); the numpy-Generator path; the host validation of
hip_ops.frames_normalize_erase; the flags. Every comparison is torch.equal / array_equal: a table look-up or a constant needs no
tolerance."""
import os
import random

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_erasing.npz")
SMALL = ((16, 8), (5, 7), (4, 6), (2, 2), (1, 9))
LARGE = (256, 128)


def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def frames_of(z, hw):
    """uint8 (n, 3, H, W): stored for the small cases, rebuilt from the seed for 256x128 (as the fixture's script builds them)."""
    name = "%dx%d" % hw
    if hw != LARGE:
        return torch.from_numpy(z[name + ".frames"])
    return torch.randint(0, 256, (4, 3) + hw, dtype=torch.uint8, generator=torch.Generator().manual_seed(int(z[name + ".seed"])))


def expected_of(z, hw, key, norm, mean):
    """The reference's output: stored for the small cases, for 256x128 rebuilt from the stored mask."""
    name = "%dx%d" % hw
    if hw != LARGE:
        return torch.from_numpy(z["%s.%s" % (name, key)])
    mask = torch.from_numpy(np.unpackbits(z["%s.%s_mask" % (name, key)])[:4 * hw[0] * hw[1]].reshape((4, 1) + hw).astype(bool))
    return torch.where(mask, torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1).expand_as(norm), norm)


def test_fixture_holds_every_case():
    z = load()
    assert [tuple(s) for s in z["sizes"].tolist()] == list(SMALL + (LARGE,)) and os.path.getsize(GOLDEN) < 300 * 1024
    for hw in SMALL:
        name = "%dx%d" % hw
        assert z[name + ".frames"].dtype == np.uint8 and z[name + ".frames"].shape == (16, 3) + hw
        assert z[name + ".group"].dtype == np.float32 and z[name + ".group"].shape == z[name + ".single"].shape == (16, 3) + hw
    assert z["256x128.group_mask"].shape == z["256x128.single_mask"].shape == (4 * 256 * 128 // 8,)
    assert z["group_mean"].tolist() == [0.485, 0.456, 0.406] and z["single_mean"].tolist() == [0.4914, 0.4822, 0.4465]


@pytest.mark.parametrize("hw", SMALL + (LARGE,), ids=lambda hw: "%dx%d" % hw)
def test_all_attempts_equal_the_references_group_random_erasing(hw):
    """The driver's GroupRandomErasing(): per frame, EVERY attempt of the 100 that fits erases."""
    from torchreid import device_transforms as T, hip_ops as ops
    z = load()
    u8 = frames_of(z, hw)
    seed = int(z["%dx%d.seed" % hw])
    rects, counts = T.erase_geometry(len(u8), hw[0], hw[1], random.Random(seed), attempts='all')
    assert rects.dtype == counts.dtype == np.int32 and rects.shape == (len(u8), max(int(counts.max()), 1), 4) and counts.shape == (len(u8),)
    got = ops.frames_normalize_erase_reference(u8, rects, counts)
    norm = ops.frames_normalize_reference(u8)
    assert torch.equal(got, expected_of(z, hw, "group", norm, ops.PIXEL_MEAN))
    assert counts.min() == 0 and counts.max() > 1, "frames that are passed over and frames with many rectangles"
    if hw == LARGE:
        assert counts.max() > 90 and float((got != norm).any(1)[counts > 0].float().mean()) > 0.9   # the loop never returns
    if hw[0] == 1:
        assert counts.max() > 0 and not rects[..., 2].any() and torch.equal(got, norm)   # zero-height rectangles: drawn, erase nothing
    # the same frames in the other layout
    assert torch.equal(ops.frames_normalize_erase_reference(u8.movedim(1, -1).contiguous(), rects, counts), got)


@pytest.mark.parametrize("hw", SMALL + (LARGE,), ids=lambda hw: "%dx%d" % hw)
def test_first_attempt_equals_the_references_random_erasing(hw):
    from torchreid import device_transforms as T, hip_ops as ops
    z = load()
    u8 = frames_of(z, hw)
    seed = int(z["%dx%d.seed" % hw]) + 1
    mean = tuple(z["single_mean"].tolist())
    rects, counts = T.erase_geometry((len(u8),), hw[0], hw[1], random.Random(seed), probability=float(z["single_probability"]),
                                     attempts='first')
    assert rects.shape == (len(u8), 1, 4) and set(counts.tolist()) <= {0, 1}
    got = ops.frames_normalize_erase_reference(u8, rects, counts, mean)
    assert torch.equal(got, expected_of(z, hw, "single", ops.frames_normalize_reference(u8), mean))
    if hw in ((16, 8), LARGE):
        assert set(counts.tolist()) == {0, 1}


def test_numpy_generator_path():
    from torchreid import device_transforms as T
    a = T.erase_geometry((3, 4), 256, 128, np.random.default_rng(5))
    b = T.erase_geometry((3, 4), 256, 128, 5)
    c = T.erase_geometry((3, 4), 256, 128, 6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[1], c[1])
    rects, counts = a
    assert rects.shape == (3, 4, int(counts.max()), 4) and counts.shape == (3, 4) and rects.dtype == counts.dtype == np.int32
    for hw in ((256, 128), (16, 8), (5, 7), (1, 9), (1, 1)):
        rects, counts = T.erase_geometry(40, hw[0], hw[1], np.random.default_rng(hw[0]), probability=0.7)
        assert counts.min() >= 0 and counts.max() <= 100
        live = np.arange(rects.shape[1])[None, :] < counts[:, None]
        y, x, h, w = (rects[..., i] for i in range(4))
        assert (rects >= 0).all() and (h[live] < hw[0]).all() and (w[live] < hw[1]).all()
        assert (y + h <= hw[0])[live].all() and (x + w <= hw[1])[live].all() and not rects[~live].any()
    rects, counts = T.erase_geometry((2, 3), 256, 128, 1, probability=0)
    assert rects.shape == (2, 3, 1, 4) and not counts.any() and not rects.any()
    rects, counts = T.erase_geometry(12, 256, 128, 2, probability=1)
    assert (counts >= 1).all()
    rects, counts = T.erase_geometry(12, 256, 128, 2, probability=1, attempts='first')
    assert (counts == 1).all() and rects.shape == (12, 1, 4)
    with pytest.raises(ValueError, match="attempts"):
        T.erase_geometry(2, 8, 8, 0, attempts='some')


def test_wrapper_validates_the_lists_before_anything_is_uploaded():
    from torchreid import hip_ops as ops
    u8 = torch.zeros((2, 3, 8, 6), dtype=torch.uint8)
    good = np.array([[[0, 0, 8, 6], [7, 5, 1, 1]], [[2, 1, 0, 0], [99, 99, 99, 99]]])   # the last row lies behind counts[1] = 1
    r, c = ops.erase_lists(good, np.array([2, 1]), 2, 8, 6)
    assert r.dtype == c.dtype == np.int32 and np.array_equal(r, good) and c.tolist() == [2, 1]
    assert ops.ERASE_MAX_RECTS == 128
    with pytest.raises(ValueError, match="on the GPU"):   # every list check passed: only then the frames' device is looked at
        ops.frames_normalize_erase(u8, good, np.array([2, 1]))
    with pytest.raises(ValueError, match="frame 1 has a count of 3, 0..2"):
        ops.frames_normalize_erase(u8, good, np.array([2, 3]))
    with pytest.raises(ValueError, match="count of -1"):
        ops.frames_normalize_erase(u8, good, np.array([2, -1]))
    with pytest.raises(ValueError, match="129 rectangles per frame, at most 128"):
        ops.frames_normalize_erase(u8, np.zeros((2, 129, 4), dtype=np.int32), np.zeros(2, dtype=np.int32))
    with pytest.raises(ValueError, match=r"frame 1 has rectangle 1 = \(y 99, x 99, h 99, w 99\) outside its 8 x 6 frame"):
        ops.frames_normalize_erase(u8, good, np.array([2, 2]))
    for bad in ([0, 0, 9, 1], [0, 0, 1, 7], [1, 0, 8, 1], [0, 6, 0, 1], [-1, 0, 1, 1], [0, 0, -1, 1]):
        with pytest.raises(ValueError, match="frame 0 has rectangle 0"):
            ops.frames_normalize_erase(u8, np.array([[bad], [[0, 0, 0, 0]]]), np.array([1, 1]))
    for rects, counts in ((np.zeros((2, 2, 3), dtype=np.int32), np.zeros(2, dtype=np.int32)),      # rows of three
                          (np.zeros((3, 2, 4), dtype=np.int32), np.zeros(3, dtype=np.int32)),      # another N
                          (np.zeros((2, 2, 4), dtype=np.int32), np.zeros((2, 1), dtype=np.int32)),
                          (np.zeros((2, 2, 4), dtype=np.float32), np.zeros(2, dtype=np.int32))):
        with pytest.raises(ValueError, match="integer"):
            ops.frames_normalize_erase(u8, rects, counts)
    with pytest.raises(ValueError, match="uint8"):
        ops.frames_normalize_erase(u8.float(), good, np.array([2, 1]))
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="host arrays"):
            ops.frames_normalize_erase(u8, torch.from_numpy(good).cuda(), np.array([2, 1]))
    else:   # no device here: a stand-in that says it lives on one
        class OnDevice(torch.Tensor):
            is_cuda = True
        with pytest.raises(ValueError, match="host arrays"):
            ops.frames_normalize_erase(u8, torch.from_numpy(good).as_subclass(OnDevice), np.array([2, 1]))
    # the reference form runs the same checks
    with pytest.raises(ValueError, match="count of 3"):
        ops.frames_normalize_erase_reference(u8, good, np.array([2, 3]))


def test_reference_form_is_slice_assignment():
    from torchreid import hip_ops as ops
    u8 = torch.randint(0, 256, (2, 3, 8, 6), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    rects = np.array([[[0, 0, 8, 6], [0, 0, 0, 0]], [[2, 1, 3, 4], [7, 5, 1, 1]]])
    value = (0.25, -1.5, 3.0)
    got = ops.frames_normalize_erase_reference(u8, rects, np.array([0, 2]), value, (0.41, 0.5, 0.37), (0.31, 0.2, 0.27))
    want = ops.frames_normalize_reference(u8, (0.41, 0.5, 0.37), (0.31, 0.2, 0.27))
    assert torch.equal(got[0], want[0])   # count 0: the full-frame rectangle behind it is not read
    for c in range(3):
        want[1, c, 2:5, 1:5] = value[c]
        want[1, c, 7:8, 5:6] = value[c]
    assert torch.equal(got, want)


def test_flags():
    from torchreid import device_transforms as T, hip_ops as ops
    with pytest.raises(TypeError):
        T.DeviceClipTransform(32, 16, rand_erase=True)                          # a train flag without train=True
    with pytest.raises(TypeError):
        T.DeviceClipTransform(32, 16, train=True, erase={"probability": 1.0})   # goes with rand_erase=True
    with pytest.raises(TypeError):
        T.DeviceClipTransform(32, 16, train=True, rand_erase=True, erase={"chance": 1.0})
    t = T.DeviceClipTransform(32, 16, train=True, rand_erase=True, flip=True, erase={"probability": 1.0, "attempts": "first", "value": (1, 2, 3)},
                              pixel_mean=(0.41, 0.5, 0.37), pixel_std=(0.31, 0.2, 0.27))
    assert t.rand_erase and t.flags == {"flip": True} and t.erase == {"probability": 1.0, "attempts": "first"} and t.erase_value == (1, 2, 3)
    assert t.pixel_mean == (0.41, 0.5, 0.37) and t.last_erase is None
    plain = T.DeviceClipTransform(32, 16, train=True, flip=True)
    assert not plain.rand_erase and plain.flags == {"flip": True}
    assert "GroupRandomErasing" in T.__doc__ and "rand_erase" in T.__doc__
    # clips_to_float: nothing changes without erase; with it the CPU takes the reference form
    x = torch.randint(0, 256, (2, 3, 8, 6, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    assert torch.equal(ops.clips_to_float(x, erase=None), ops.frames_normalize_reference(x)) and torch.equal(ops.clips_to_float(x), ops.clips_to_float(x, erase=None))
    rects, counts = T.erase_geometry((2, 3), 8, 6, 9, probability=1)
    got = ops.clips_to_float(x, erase=(rects, counts))
    assert got.shape == (2, 3, 3, 8, 6) and torch.equal(got, ops.frames_normalize_erase_reference(x, rects, counts)) and counts.min() > 0
    assert not torch.equal(got, ops.clips_to_float(x)) and not torch.equal(got, ops.clips_to_float(x, erase=(rects, counts, (9, 9, 9))))
    with pytest.raises(ValueError, match="erase is"):
        ops.clips_to_float(x, erase=(rects[0], counts[0]))
