"""Resize / crop / flip of uint8 clips, the host side (no GPU): hip_ops.clip_resample_reference -- the integer restatement the GPU kernel
is compared with -- against PILLOW's own bytes, from tests/golden/clip_resample.npz (tools/make_clip_resample_golden.py: Pillow only) and,
where PIL imports, live on random sizes; the taps; the geometry sampling of torchreid/device_transforms.py; the host validation of
hip_ops.clip_resample. Every comparison is array_equal / torch.equal: there is no tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_resample.npz")
CASES = ("identity_32x16", "window_30x15_at_1_1", "upscale_16x8", "odd_19x11", "down_37x23", "down_70x50", "one_pixel",
         "horizontal_only_32x20", "vertical_only_40x16", "flip_37x23", "misalign_pad_top", "misalign_pad_bottom", "checker_37x23")


def load_case(name):
    with np.load(GOLDEN) as z:
        return (torch.from_numpy(z[name + ".frames"]), z[name + ".geometry"], tuple(int(v) for v in z[name + ".out_hw"]),
                torch.from_numpy(z[name + ".expected"]))


def test_fixture_holds_every_case():
    with np.load(GOLDEN) as z:
        assert tuple(z["names"].tolist()) == CASES and str(z["pillow_version"])
        for name in CASES:
            frames, g, out_hw = z[name + ".frames"], z[name + ".geometry"], z[name + ".out_hw"]
            assert frames.dtype == np.uint8 and frames.shape[0] == 1 and frames.shape[1] <= 70 and frames.shape[2] <= 50
            assert g.shape == (1, 8) and g.dtype == np.int32 and z[name + ".expected"].shape == (1, out_hw[0], out_hw[1], 3)
        g = {n: z[n + ".geometry"][0].tolist() for n in CASES}
    # the cases are the ones the kernel's contract names
    assert g["window_30x15_at_1_1"] == [32, 16, 1, 1, 30, 15, 0, 0] and g["flip_37x23"] == [37, 23, 0, 0, 37, 23, 1, 0]
    assert g["misalign_pad_top"] == [32, 16, -1, 0, 33, 16, 0, 0] and g["misalign_pad_bottom"] == [32, 16, 0, 0, 33, 16, 0, 0]
    assert g["one_pixel"][:2] == [1, 1] and g["horizontal_only_32x20"][:2] == [32, 20] and g["vertical_only_40x16"][:2] == [40, 16]


@pytest.mark.parametrize("name", CASES)
def test_reference_equals_pillow_fixture(name):
    from torchreid import hip_ops as ops
    frames, g, out_hw, expected = load_case(name)
    got = ops.clip_resample_reference(frames, g, out_hw)
    assert got.dtype == torch.uint8 and got.shape == expected.shape
    assert torch.equal(got, expected), "%s: %d of %d bytes differ from Pillow's" % (name, int((got != expected).sum()), expected.numel())
    if name == "checker_37x23":
        assert set(frames.unique().tolist()) == {0, 255}
    if name == "flip_37x23":   # the flip is applied after the resize
        assert torch.equal(got.flip(2), load_case("down_37x23")[3])
    if name == "identity_32x16":
        assert torch.equal(got, frames)


def test_window_is_an_image_of_its_own():
    """crop().resize() -- the filter support ends at the window's edge -- differs from resampling the frame with a box."""
    from torchreid import hip_ops as ops
    frames, g, out_hw, expected = load_case("window_30x15_at_1_1")
    cropped = frames[:, 1:31, 1:16].contiguous()
    again = ops.clip_resample_reference(cropped, np.array([[30, 15, 0, 0, 30, 15, 0, 0]], dtype=np.int32), out_hw)
    assert torch.equal(again, expected)


def pillow_side(frame, geometry, out_hw):
    from PIL import Image
    sh, sw, y0, x0, wh, ww, flip = (int(v) for v in geometry[:7])
    valid = frame[:sh, :sw]
    top, left = max(0, -y0), max(0, -x0)
    bottom, right = max(0, y0 + wh - sh), max(0, x0 + ww - sw)
    if top or left or bottom or right:
        valid = np.pad(valid, ((top, bottom), (left, right), (0, 0)), mode="edge")
    img = Image.fromarray(np.ascontiguousarray(valid)).crop((x0 + left, y0 + top, x0 + left + ww, y0 + top + wh))
    img = img.resize((int(out_hw[1]), int(out_hw[0])), Image.BILINEAR)
    return np.asarray(img.transpose(Image.FLIP_LEFT_RIGHT) if flip else img)


def test_reference_equals_live_pillow_on_random_sizes():
    pytest.importorskip("PIL")
    from torchreid import hip_ops as ops
    rng = np.random.default_rng(2024)
    sizes = [(1, 1), (300, 300), (1, 300), (300, 1), (256, 128), (240, 120), (128, 64), (207, 2), (300, 2), (200, 2)] + [
        (int(rng.integers(1, 301)), int(rng.integers(1, 301))) for _ in range(40)]
    for n, (h, w) in enumerate(sizes):
        frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        geos = [(h, w, 0, 0, h, w, n % 2, 0)]
        if h > 4 and w > 4:   # a window inside the frame, and one that leaves it on every side
            y0, x0 = int(rng.integers(0, h // 2)), int(rng.integers(0, w // 2))
            geos.append((h, w, y0, x0, int(rng.integers(1, h - y0 + 1)), int(rng.integers(1, w - x0 + 1)), (n + 1) % 2, 0))
            geos.append((h, w, -3, -2, h + 5, w + 7, 0, 0))
        for g in geos:
            for out_hw in ((32, 16), (256, 128)):
                got = ops.clip_resample_reference(torch.from_numpy(frame)[None], np.array([g], dtype=np.int32), out_hw)[0].numpy()
                want = pillow_side(frame, g, out_hw)
                assert np.array_equal(got, want), "%s -> %s: %d bytes differ from Pillow's" % (g, out_hw, int((got != want).sum()))


def test_padded_container_and_batches():
    """Valid extents inside a larger container: the bytes outside them never matter, and frames of a batch are independent."""
    from torchreid import hip_ops as ops
    names = ("down_70x50", "down_37x23", "odd_19x11", "one_pixel")
    for fill in (0, 0xEE):
        box = torch.full((4, 70, 50, 3), fill, dtype=torch.uint8)
        geo = np.zeros((4, 8), dtype=np.int32)
        for n, name in enumerate(names):
            frames, g, _, _ = load_case(name)
            box[n, :frames.shape[1], :frames.shape[2]] = frames[0]
            geo[n] = g[0]
        got = ops.clip_resample_reference(box, geo, (32, 16))
        for n, name in enumerate(names):
            assert torch.equal(got[n], load_case(name)[3][0]), (name, fill)


def test_resample_taps():
    from torchreid import hip_ops as ops
    for out in (16, 32, 128, 256):
        for size in list(range(1, 301)) + [8 * out]:
            k, bounds = ops.resample_taps(size, out)
            lo, count = bounds[:, 0], bounds[:, 1]
            assert k.dtype == np.int32 and bounds.dtype == np.int32 and k.shape[0] == out and bounds.shape == (out, 2)
            assert (k >= 0).all() and (lo >= 0).all() and (count >= 1).all() and (lo + count <= size).all()
            assert (k[np.arange(k.shape[1])[None, :] >= count[:, None]] == 0).all()
            assert (np.abs(k.sum(1).astype(np.int64) - (1 << 22)) <= k.shape[1]).all()   # each tap is rounded on its own
            assert (np.diff(lo) >= 0).all() and (np.diff(lo + count) >= 0).all()
            if size == out:
                assert (count == 1).all() and np.array_equal(lo, np.arange(out)) and (k[:, 0] == 1 << 22).all() and (k[:, 1:] == 0).all()
            if size <= ops.RESAMPLE_MAX_SCALE * out:   # what the kernel holds is the whole row
                k17, b17 = ops.resample_taps(size, out, ops.RESAMPLE_TAPS)
                assert k17.shape == (out, 17) and np.array_equal(b17, bounds)
                assert np.array_equal(k17[:, :k.shape[1]], k[:, :17]) and (k17[:, k.shape[1]:] == 0).all()
    k, bounds = ops.resample_taps(2, 4)   # by hand: centres 0.25, 0.75, 1.25, 1.75
    assert bounds.tolist() == [[0, 1], [0, 2], [0, 2], [1, 1]]
    assert k[:, :2].tolist() == [[1 << 22, 0], [3 << 20, 1 << 20], [1 << 20, 3 << 20], [1 << 22, 0]]
    with pytest.raises(ValueError):
        ops.resample_taps(0, 4)


SIZES = np.array([[[256, 128]] * 4, [[250, 125]] * 4, [[300, 140]] * 4])


def misalign_kind(g, h):
    y0, win_h = int(g[2]), int(g[4])
    if win_h == h:
        return None
    return ("up" if y0 != 0 else "bottom", "crop" if win_h < h else "pad")


def test_train_geometry_samples_once_per_clip():
    from torchreid import device_transforms as T
    kinds, flips = set(), set()
    for seed in range(200):
        g = T.train_geometry(SIZES, np.random.default_rng(seed), misalign=True, flip=True)
        assert g.shape == (3, 4, 8) and g.dtype == np.int32
        assert np.array_equal(g, T.train_geometry(SIZES, np.random.default_rng(seed), misalign=True, flip=True))   # reproducible
        for b in range(3):
            h, w = SIZES[b, 0]
            assert (g[b] == g[b, 0]).all(), "every frame of a clip shares the draw"
            assert g[b, 0, :2].tolist() == [h, w] and g[b, 0, 3] == 0 and g[b, 0, 5] == w and g[b, 0, 7] == 0
            kind = misalign_kind(g[b, 0], h)
            th = int(h * 0.05)
            want = {None: (0, h), ("up", "crop"): (th, h - th), ("bottom", "crop"): (0, h - th), ("up", "pad"): (-th, h + th),
                    ("bottom", "pad"): (0, h + th)}[kind]
            assert (int(g[b, 0, 2]), int(g[b, 0, 4])) == want
            kinds.add(kind)
            flips.add(int(g[b, 0, 6]))
    assert kinds == {None, ("up", "crop"), ("bottom", "crop"), ("up", "pad"), ("bottom", "pad")} and flips == {0, 1}
    assert T.train_geometry(SIZES[0], 7, misalign=True, rand_crop=True, flip=True).shape == (4, 8)   # one clip; a seed for rng


def test_train_geometry_crop_stays_inside_the_padded_frame():
    from torchreid import device_transforms as T
    ragged = np.array([[[256, 128], [254, 126], [260, 130], [270, 121]]])   # frames of one clip may differ: the draw is still shared
    offsets = set()
    for seed in range(200):
        g = T.train_geometry(ragged, np.random.default_rng(seed), misalign=True, rand_crop=True, flip=True)[0]
        plain = T.train_geometry(ragged, np.random.default_rng(seed), misalign=True, flip=True)[0]   # the same misalign draw, no crop
        assert (g[:, 4] == 240).all() and (g[:, 5] == 120).all() and len(set(g[:, 6].tolist())) == 1
        assert len(set((g[:, 2] - plain[:, 2]).tolist())) == 1 and len(set(g[:, 3].tolist())) == 1, "one crop offset per clip"
        # inside the misaligned (cropped or edge-padded) frame: [plain.y0, plain.y0 + plain.win_h) x [0, w)
        assert (g[:, 2] >= plain[:, 2]).all() and (g[:, 2] + 240 <= plain[:, 2] + plain[:, 4]).all()
        assert (g[:, 3] >= 0).all() and (g[:, 3] + 120 <= ragged[0, :, 1]).all()
        offsets.add((int(g[0, 2] - plain[0, 2]), int(g[0, 3])))
    assert len(offsets) > 20
    exact = T.train_geometry(np.array([[240, 120]] * 2), 0, rand_crop=True)
    assert exact.tolist() == [[240, 120, 0, 0, 240, 120, 0, 0]] * 2
    with pytest.raises(ValueError, match="too small"):
        T.train_geometry(np.array([[256, 128], [239, 128]]), 0, rand_crop=True)
    with pytest.raises(ValueError, match="too small"):
        T.train_geometry(np.array([[[128, 64]] * 4]), 0, rand_crop=True)
    off = T.train_geometry(SIZES, 3)   # nothing switched on: transform_test
    assert np.array_equal(off, T.eval_geometry(SIZES))


def test_eval_geometry_and_transform_arguments():
    from torchreid import device_transforms as T
    g = T.eval_geometry(np.array([[[128, 64], [70, 50]]]))
    assert g.dtype == np.int32 and g.tolist() == [[[128, 64, 0, 0, 128, 64, 0, 0], [70, 50, 0, 0, 70, 50, 0, 0]]]
    with pytest.raises(ValueError):
        T.eval_geometry(np.array([[0, 5]]))
    with pytest.raises(ValueError):
        T.eval_geometry(np.array([[1.0, 5.0]]))
    with pytest.raises(TypeError):
        T.DeviceClipTransform(256, 128, rand_crop=True)          # train flags without train=True
    with pytest.raises(TypeError):
        T.DeviceClipTransform(256, 128, train=True, erase=True)   # random erasing is not a geometry
    with pytest.raises(ValueError, match="uint8"):
        T.DeviceClipTransform(256, 128)(torch.zeros((1, 2, 8, 8, 3)))
    assert "erasing" in T.__doc__ and "OUT OF SCOPE" in T.__doc__


def test_geometry_validation_names_the_frame():
    """What hip_ops.clip_resample checks on the host before anything is uploaded (resample_geometry with the kernel's scale limit)."""
    from torchreid import hip_ops as ops
    shape, out_hw = (3, 70, 50, 3), (32, 16)
    good = np.array([[70, 50, 0, 0, 70, 50, 0, 0]] * 3, dtype=np.int32)
    assert np.array_equal(ops.resample_geometry(good, shape, out_hw, ops.RESAMPLE_MAX_SCALE), good)

    def bad(frame, col, value, match, **kw):
        g = good.copy()
        g[frame, col] = value
        with pytest.raises(ValueError, match=match):
            ops.resample_geometry(g, shape, out_hw, **kw)

    bad(1, 4, 0, "frame 1 has a window of 0 x 50")
    bad(2, 5, -3, "frame 2 has a window")
    bad(0, 0, 71, "frame 0 has a valid extent of 71 x 50")
    bad(2, 1, 51, "frame 2 has a valid extent of 70 x 51")
    bad(1, 0, 0, "frame 1 has a valid extent")
    bad(1, 4, 8 * 32 + 1, "frame 1 has a window of 257 x 50, more than 8 times", max_scale=8)
    bad(2, 5, 8 * 16 + 1, "frame 2 has a window of 70 x 129, more than 8 times", max_scale=8)
    g = good.copy()
    g[1, 2:6] = (-80, 0, 201, 2)        # Image.resize runs the vertical pass first on such a sliver; the kernel never does
    with pytest.raises(ValueError, match="frame 1 has a window of 201 x 2, over 100 times as tall as wide"):
        ops.resample_geometry(g, shape, out_hw, ops.RESAMPLE_MAX_SCALE)
    assert ops.resample_vertical_first(201, 2, 32) and not ops.resample_vertical_first(200, 2, 32) and not ops.resample_vertical_first(201, 2, 201)
    g[1, 2:6] = (-80, 0, 200, 2)
    ops.resample_geometry(g, shape, out_hw, ops.RESAMPLE_MAX_SCALE)
    # slivers whose horizontal pass cannot change a byte are accepted: the order of the passes does not show
    g[1, 2:6] = (-80, 0, 201, 1)      # one column: the pass copies it
    ops.resample_geometry(g, shape, out_hw, ops.RESAMPLE_MAX_SCALE)
    g[1, 2:6] = (0, 0, 2001, 16)      # as wide as the output: Pillow skips the pass
    ops.resample_geometry(g, (3, 2001, 50, 3), (251, 16), ops.RESAMPLE_MAX_SCALE)
    for h, w, out in ((201, 1, (32, 16)), (2001, 16, (251, 16))):
        a = np.random.default_rng(h).integers(0, 256, (h, w, 3)).astype(np.int64)
        horizontal_first = ops._resample_axis(ops._resample_axis(a.transpose(1, 0, 2), out[1]).transpose(1, 0, 2), out[0])
        vertical_first = ops._resample_axis(ops._resample_axis(a, out[0]).transpose(1, 0, 2), out[1]).transpose(1, 0, 2)
        assert ops.resample_vertical_first(h, w, out[0]) and np.array_equal(horizontal_first, vertical_first)
    g = good.copy()
    g[:, 4], g[:, 5] = 8 * 32, 8 * 16   # exactly 8 x: allowed
    ops.resample_geometry(g, shape, out_hw, ops.RESAMPLE_MAX_SCALE)
    for wrong in (good[:2], good.astype(np.float32), good.reshape(-1)):
        with pytest.raises(ValueError, match="geometry is an integer"):
            ops.resample_geometry(wrong, shape, out_hw)
    frames = torch.zeros(shape, dtype=torch.uint8)
    for args in ((frames.float(), good, out_hw), (frames[..., :2], good, out_hw), (frames[0], good, out_hw)):
        with pytest.raises(ValueError, match="uint8"):
            ops.clip_resample_reference(*args)
        with pytest.raises(ValueError, match="uint8"):
            ops.clip_resample(*args)
    with pytest.raises(ValueError, match="on the GPU"):   # the GPU entry takes device frames: there is no quiet CPU route
        ops.clip_resample(frames, good, out_hw)
