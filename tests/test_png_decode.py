"""PNG decode, the CPU half: parse_png (chunks, CRCs, the subset), the restatement hip_ops.png_decode_reference (inflate with inflate's own
rejections, the five row filters) against zlib and Pillow's pixels (tests/golden/png_decode.npz), the coverage the fixture must have,
the status of every broken stream, and the decoders on a CPU device. The restatement runs once over the fixture (png_cases.reference)."""
import logging
import zlib

import numpy as np
import pytest
import torch

import jpeg_cases as J
import png_cases as P
from torchreid import device_decode as dd, hip_ops as ops


# ---- parse_png ---------------------------------------------------------------------------------------------------------------------------
def test_parse_png_reads_every_fixture_file_without_inflating():
    for name, (png, px) in P.fixture().items():
        fr = dd.parse_png(png)
        assert (fr.height, fr.width) == px.shape[:2] == tuple(int(v) for v in name.split("_")[0].split("x")), name
        assert fr.channels == (1 if "_grey_" in name else 3), name
        assert sum(fr.idat_sizes) == len(fr.stream) and isinstance(fr.stream, bytes)
        assert len(zlib.decompress(fr.stream)) == ops.png_frame_inflated(fr.height, fr.width, fr.channels), name
    assert len(dd.parse_png(P.fixture()["64x128_rgb_smooth_mixed_dynamic_split"][0]).idat_sizes) > 100
    for name, (png, _) in P.broken().items():      # their chunks are sound
        assert dd.parse_png(png).stream


UNSUPPORTED = {"palette": "colour type 3", "grey_alpha": "colour type 4", "rgb_alpha": "colour type 6", "depth_16": "bit depth 16",
               "depth_1": "bit depth 1", "depth_2": "bit depth 2", "depth_4": "bit depth 4", "trns": "tRNS", "adam7": "Adam7", "actl": "acTL",
               "crc_mismatch": "CRC mismatch", "over_the_size_bound": "over the size bound", "not_a_png": "not a PNG"}


def test_parse_png_refuses_everything_outside_the_subset_by_name():
    assert sorted(P.unsupported()) == sorted(UNSUPPORTED)
    for name, (data, _) in P.unsupported().items():
        with pytest.raises(dd.UnsupportedPng, match=UNSUPPORTED[name]):
            dd.parse_png(data)
    good = P.fixture()["7x9_rgb_smooth_pillow"][0]
    for cut in (4, 20, 40, len(good) - 15):
        with pytest.raises(dd.UnsupportedPng, match="not a PNG|ends early|without an IDAT"):
            dd.parse_png(good[:cut])
    assert issubclass(dd.UnsupportedPng, ValueError) and ops.PNG_MAX_INFLATED >= 98560 == ops.png_frame_inflated(256, 128, 3)


def test_png_batch_plan_lays_the_streams_out_for_the_kernel():
    order, plan, _, _, _ = P.reference()
    assert plan.desc.dtype == np.int32 and plan.desc.shape == (len(order), ops.PNG_DESC) and plan.streams.size % ops.PNG_STREAM_ALIGN == 0
    for f, name in enumerate(order):
        fr = dd.parse_png(P.fixture()[name][0])
        off, n = int(plan.desc[f, ops.PD_OFF]), int(plan.desc[f, ops.PD_LEN])
        assert off % ops.PNG_STREAM_ALIGN == 0 and plan.streams[off:off + n].tobytes() == fr.stream
        end = int(plan.desc[f + 1, ops.PD_OFF]) if f + 1 < len(order) else plan.streams.size
        assert end - (off + n) >= ops.PNG_STREAM_PAD and not plan.streams[off + n:end].any()
        assert plan.desc[f, 2:].tolist() == [fr.height, fr.width, fr.channels, 0, 0, 0] and plan.sizes[f].tolist() == [fr.height, fr.width]
    assert plan.container == (256, 128)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def test_restatement_inflates_what_zlib_inflates():
    order, plan, _, status, info = P.reference()
    assert not status.any(), status.tolist()
    for f, name in enumerate(order):
        assert info[f]["inflated"] == zlib.decompress(dd.parse_png(P.fixture()[name][0]).stream), name


def test_restatement_equals_pillows_pixels():
    order, plan, clip, status, _ = P.reference()
    want, sizes = P.container([P.fixture()[n][1] for n in order])
    assert clip.dtype == torch.uint8 and status.dtype == torch.int32 and np.array_equal(plan.sizes, sizes)
    assert np.array_equal(clip.numpy(), want)
    pytest.importorskip("PIL")
    for f, name in enumerate(order):
        px = dd.pillow_decode(P.fixture()[name][0])
        assert np.array_equal(px, P.fixture()[name][1]) and np.array_equal(clip[f].numpy()[:px.shape[0], :px.shape[1]], px), name


def test_fixture_exercises_every_path_the_decoder_has():
    """a CONDITION on the fixture, taken by the restatement now and equal to what the generator stored"""
    order, _, _, _, info = P.reference()
    live = {n: {k: (sorted(v) if isinstance(v, set) else int(v)) for k, v in c.items() if k != "inflated"} for n, c in zip(order, info)}
    assert live == P.counters()
    c = list(live.values())
    assert {0, 1, 2} <= set().union(*[set(v["btypes"]) for v in c])
    assert any(v["empty_stored"] for v in c) and any(v["blocks"] > 1 for v in c)
    assert set().union(*[set(v["filters"]) for v in c]) == {0, 1, 2, 3, 4}
    assert max(v["max_len"] for v in c) == 258 and any(v["dist_lt_len"] for v in c) and any(v["dist_1"] for v in c)
    assert max(v["max_dist"] for v in c) >= 32000 and live[P.LARGE]["max_dist"] == 85 * 385
    assert any(v["split_codes"] for v in c) and any(v["wbits"] < 15 for v in c)
    for shape in P.SHAPES:                    # the issue's shapes, in grey and RGB
        for mode in P.MODES:
            assert P.names(shape, mode), (shape, mode)
    # every filter on a FIRST row and on a later one
    assert {c["inflated"][0] for c in info} == {0, 1, 2, 3, 4}
    assert {c["inflated"][len(c["inflated"]) // 7 * 6] for n, c in zip(order, info) if n.startswith("7x9_")} == {0, 1, 2, 3, 4}


def test_code_table_rejections_are_inflates_own():
    t = ops._png_code_table
    assert t([1], ops._PNG_DISTS)[0] == ops.PNG_OK and t([0, 0], ops._PNG_DISTS)[0] == ops.PNG_OK       # one code; none at all
    assert t([1], ops._PNG_LENS)[0] == ops.PNG_ERR_INCOMPLETE and t([1], ops._PNG_CODES)[0] == ops.PNG_ERR_INCOMPLETE
    assert t([2, 0, 0], ops._PNG_DISTS)[0] == ops.PNG_ERR_INCOMPLETE and t([0] * 19, ops._PNG_CODES)[0] == ops.PNG_ERR_INCOMPLETE
    assert t([1, 1, 1], ops._PNG_DISTS)[0] == ops.PNG_ERR_OVERSUB and t([1, 2, 2, 15], ops._PNG_LENS)[0] == ops.PNG_ERR_OVERSUB
    st, table, bits = t([2, 1, 3, 3], ops._PNG_LENS)
    assert st == ops.PNG_OK and bits == 3 and sorted(set(table.tolist())) == [(1 << 16) | 1, (2 << 16) | 0, (3 << 16) | 2, (3 << 16) | 3]


STATED = {"cut": ops.PNG_ERR_INPUT, "distance_before_start": ops.PNG_ERR_DIST, "block_type_3": ops.PNG_ERR_BTYPE,
          "len_nlen_mismatch": ops.PNG_ERR_STORED, "oversubscribed_table": ops.PNG_ERR_OVERSUB, "wrong_adler": ops.PNG_ERR_ADLER,
          "filter_byte_5": ops.PNG_ERR_FILTER, "inflated_too_short": ops.PNG_ERR_SHORT, "inflated_too_long": ops.PNG_ERR_LONG}


@pytest.mark.parametrize("name", sorted(P.broken()))
def test_broken_stream_gets_its_status_and_its_neighbours_stay_exact(name):
    plan, clip, status, want = P.broken_batch(name)
    got = int(status[1])
    assert got != 0 and got != ops.PNG_ERR_DESC and got == P.broken()[name][1] and got == STATED.get(name, got)
    assert status.tolist() == [0, got, 0, 0] and np.array_equal(clip.numpy(), want)      # the broken frame's slot is all zero
    stream = dd.parse_png(P.broken()[name][0]).stream
    if got not in (ops.PNG_ERR_SHORT, ops.PNG_ERR_LONG, ops.PNG_ERR_FILTER):              # those three zlib itself inflates
        with pytest.raises(zlib.error):
            zlib.decompress(stream)
    else:
        assert len(zlib.decompress(stream)) % 28 == 0


def test_status_zero_only_for_streams_zlib_accepts():
    """every good small stream damaged in fixed-seed ways: wherever the restatement says 0, zlib inflates the stream to the same bytes"""
    rng = np.random.default_rng(11)
    zeros = 0
    for name in P.names((7, 9)) + P.names((1, 7)):
        fr = dd.parse_png(P.fixture()[name][0])
        for k in range(12):
            b = bytearray(fr.stream)
            at = int(rng.integers(0, len(b)))
            if k % 3 == 0:
                b = b[:at]
            elif k % 3 == 1:
                b[at] ^= 1 << int(rng.integers(0, 8))
            else:
                b[at:at + 3] = rng.integers(0, 256, len(b[at:at + 3]), dtype=np.uint8).tobytes()
            info = []
            _, status = ops.png_decode_reference(dd.png_batch_plan([fr._replace(stream=bytes(b))]), info=info)
            if int(status[0]) == 0:
                zeros += 1
                assert zlib.decompress(bytes(b)) == info[0]["inflated"], (name, k)
            elif int(status[0]) not in (ops.PNG_ERR_SHORT, ops.PNG_ERR_LONG, ops.PNG_ERR_FILTER):
                with pytest.raises(zlib.error):
                    zlib.decompress(bytes(b))
    assert zeros < 40


def test_a_descriptor_row_outside_its_buffers_gets_status_5():
    names = ["7x9_rgb_smooth_f1", "1x7_grey_smooth_f2", "7x1_rgb_smooth_pillow"]
    plan = dd.png_batch_plan([dd.parse_png(P.fixture()[n][0]) for n in names])
    for col, value in ((ops.PD_OFF, plan.streams.size), (ops.PD_OFF, 4), (ops.PD_LEN, -1), (ops.PD_H, 8), (ops.PD_W, 0), (ops.PD_CH, 2)):
        desc = plan.desc.copy()
        desc[1, col] = value
        clip, status = ops.png_decode_reference(plan._replace(desc=desc))
        assert status.tolist() == [0, ops.PNG_ERR_DESC, 0] and not clip[1].any()
        assert np.array_equal(clip[0, :7, :9].numpy(), P.fixture()[names[0]][1])


# ---- the decoders on a CPU device ----------------------------------------------------------------------------------------------------------
def test_device_png_decoder_on_cpu_shapes_sizes_and_counters():
    pytest.importorskip("PIL")
    fx = P.fixture()
    names = ["7x9_rgb_smooth_f4", "1x7_grey_smooth_f3", "64x128_grey_smooth_paeth_w9", "7x1_rgb_smooth_mixed_fixed", "1x1_grey_smooth_pillow",
             "7x9_grey_smooth_flushes", "7x18_grey_dynamic_one_distance", "7x9_rgb_dynamic_deep", "7x9_grey_dynamic_no_distance",
             "64x128_rgb_solid_none", "7x9_rgb_smooth_level0_split", "1x7_rgb_smooth_f1"]
    dec = dd.DevicePngDecoder("cpu")
    want, want_sizes = P.container([fx[n][1] for n in names])
    for shape in ((3, 4), (2, 3, 2), None):
        imgs, sizes = dec.decode([fx[n][0] for n in names], shape=shape)
        lead = shape or (12,)
        assert imgs.dtype == torch.uint8 and tuple(imgs.shape) == lead + (64, 128, 3) and sizes.shape == lead + (2,) and sizes.dtype == np.int64
        assert np.array_equal(imgs.reshape(12, 64, 128, 3).numpy(), want) and np.array_equal(sizes.reshape(12, 2), want_sizes)
    assert dec.frames == 36 and dec.fallback_frames == 0
    with pytest.raises(ValueError, match="do not fill shape"):
        dec.decode([fx[names[0]][0]] * 3, shape=(2, 2))


def test_device_png_decoder_fallback_counts_logs_and_takes_pillows_pixels(caplog):
    pytest.importorskip("PIL")
    fx, un, br = P.fixture(), P.unsupported(), P.broken()
    outside = ["palette", "rgb_alpha", "grey_alpha", "depth_16", "depth_1", "trns", "adam7"]
    files = [fx["7x9_rgb_smooth_f2"][0]] + [un[n][0] for n in outside] + [br["inflated_too_long"][0], fx["1x7_grey_smooth_f0"][0]]
    dec = dd.DevicePngDecoder("cpu")
    with caplog.at_level(logging.WARNING, logger="torchreid.device_decode"):
        imgs, sizes = dec.decode(files)
    assert dec.frames == 10 and dec.fallback_frames == 8 and "8 of 10 frames took the Pillow fallback" in caplog.text
    for f, data in enumerate(files):
        px = dd.pillow_decode(data)
        assert sizes[f].tolist() == list(px.shape[:2]) and np.array_equal(imgs[f, :px.shape[0], :px.shape[1]].numpy(), px), f
        assert not imgs[f, px.shape[0]:].any() and not imgs[f, :, px.shape[1]:].any()
    for f, n in enumerate(outside):
        assert np.array_equal(imgs[1 + f, :un[n][1].shape[0], :un[n][1].shape[1]].numpy(), un[n][1]), n
    # what Pillow cannot decode either: the error names the frame
    for name in ("cut", "wrong_adler", "filter_byte_5"):
        with pytest.raises(dd.UnsupportedPng, match="frame 1: device status %d .* Pillow cannot decode it either" % br[name][1]):
            dec.decode([files[0], br[name][0]])
    with pytest.raises(dd.UnsupportedPng, match="frame 2: .*CRC mismatch.* Pillow cannot decode it either"):
        dec.decode([files[0], files[0], un["crc_mismatch"][0]])
    with pytest.raises(dd.UnsupportedPng, match="frame 0: not a PNG"):
        dec.decode([un["not_a_png"][0]])


def test_device_image_decoder_on_cpu_merges_jpeg_and_png_in_the_callers_order():
    pytest.importorskip("PIL")
    jx, px = J.fixture(), P.fixture()
    files = [jx["17x9_422_q30_noise"][0], px["7x9_rgb_smooth_f4"][0], px["64x128_grey_smooth_paeth_w9"][0], jx["33x47_gray_q85_noise_opt"][0],
             P.unsupported()["palette"][0], jx["16x16_420_q100_noise"][0], px["1x7_grey_smooth_f3"][0], jx["8x8_444_q30_noise"][0]]
    dec = dd.DeviceImageDecoder("cpu")
    imgs, sizes = dec.decode(files, shape=(2, 4))
    assert tuple(imgs.shape) == (2, 4, 64, 128, 3) and sizes.shape == (2, 4, 2)
    flat = imgs.reshape(8, 64, 128, 3)
    for f, data in enumerate(files):
        want = dd.pillow_decode(data)
        assert sizes.reshape(8, 2)[f].tolist() == list(want.shape[:2]), f
        assert np.array_equal(flat[f, :want.shape[0], :want.shape[1]].numpy(), want), f
        assert not flat[f, want.shape[0]:].any() and not flat[f, :, want.shape[1]:].any()
    assert dec.frames == 8 == dec.jpeg.frames + dec.png.frames and dec.jpeg.frames == 4
    assert dec.fallback_frames == 1 == dec.png.fallback_frames and dec.jpeg.fallback_frames == 0
    only_png, sizes = dec.decode([px["7x9_rgb_smooth_f0"][0]])          # one kind alone: that decoder's own container
    assert tuple(only_png.shape) == (1, 7, 9, 3) and dec.frames == 9
