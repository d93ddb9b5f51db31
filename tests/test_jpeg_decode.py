"""Baseline JPEG decode without a GPU: the header parser's accept / reject table, the decode-ready Huffman tables against brute force,
hip_ops.jpeg_decode_reference -- the arithmetic agrl_jpeg_decode_u8 is held to -- against Pillow's pixels (the fixture of
tools/make_jpeg_golden.py, and live Pillow where it imports) by exact equality, the status codes of broken scans, the fallback, and the
5-tuple contract of evaluation.decode_batches."""
import io
import logging

import numpy as np
import pytest
import torch

import dense_stub as DS
import jpeg_cases as J


def mods():
    from torchreid import device_decode as dd, hip_ops as ops
    return dd, ops


def decode_one(data):
    dd, ops = mods()
    plan = dd.jpeg_batch_plan([dd.parse_jpeg(data)])
    clip, status = ops.jpeg_decode_reference(plan)
    return clip[0].numpy(), int(status[0])


# ---- the parser ------------------------------------------------------------------------------------------------------------------
def segments(data):
    """[(marker, offset of its FF, offset behind its payload)] of the header, up to and including SOS"""
    out, at = [(0xD8, 0, 2)], 2
    while True:
        assert data[at] == 0xFF
        m, n = data[at + 1], (data[at + 2] << 8) | data[at + 3]
        out.append((m, at, at + 2 + n))
        at += 2 + n
        if m == 0xDA:
            return out


def patched(data, marker, edit, nth=0):
    """the file with ``edit(payload bytearray)`` applied to the payload of its nth ``marker`` segment (the length is rewritten)"""
    m, lo, hi = [s for s in segments(data) if s[0] == marker][nth]
    payload = bytearray(data[lo + 4:hi])
    payload = edit(payload) or payload
    return data[:lo + 2] + bytes([(len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + bytes(payload) + data[hi:]


def set_byte(i, v):
    def edit(p):
        p[i] = v
    return edit


def set_marker(data, marker, new):
    lo = [s for s in segments(data) if s[0] == marker][0][1]
    return data[:lo + 1] + bytes([new]) + data[lo + 2:]


def base(sampling="420"):
    return J.fixture()["17x9_%s_q30_noise" % sampling][0]


def test_parser_accepts_the_subset():
    dd, ops = mods()
    code = {"444": ops.JPEG_444, "422": ops.JPEG_422, "420": ops.JPEG_420, "gray": ops.JPEG_GRAY}
    for name, (data, px) in J.fixture().items():
        fr = dd.parse_jpeg(data)
        assert (fr.height, fr.width) == px.shape[:2] and fr.sampling == code[name.split("_")[1]], name
        assert len(fr.components) == (1 if "_gray_" in name else 3) and (fr.restart_interval > 0) == ("_rst" in name), name
        assert bytes(fr.scan) in data and data.endswith(b"\xff\xd9") and data.index(bytes(fr.scan)) + len(fr.scan) == len(data) - 2, name
    # what the subset tolerates: SOF1 (extended sequential, Huffman, 8 bit), APPn / COM segments (EXIF among them), a missing EOI
    d = base()
    px = J.fixture()["17x9_420_q30_noise"][1]
    exif = b"\xff\xe1\x00\x10Exif\x00\x00MM\x00\x2a\x00\x00\x00\x08" + b"\xff\xfe\x00\x05abc"
    for variant in (set_marker(d, 0xC0, 0xC1), d[:2] + exif + d[2:], d[:-2]):
        got, status = decode_one(variant)
        assert status == 0 and np.array_equal(got, px)
    # an Adobe segment that says YCbCr (transform 1)
    adobe1 = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01"
    assert dd.parse_jpeg(d[:2] + adobe1 + d[2:]).sampling == ops.JPEG_420
    # the largest dimension passes the parser
    assert dd.JPEG_MAX_DIM == 4096
    assert dd.parse_jpeg(patched(d, 0xC0, lambda p: p.__setitem__(slice(1, 3), b"\x10\x00"))).height == 4096


def sof_components(ids=None, sampling0=None, four=False):
    def edit(p):
        if ids:
            for c, i in enumerate(ids):
                p[6 + 3 * c] = i
        if sampling0 is not None:
            p[7] = sampling0
        if four:
            p[5] = 4
            return p + bytearray([4, 0x11, 0])
    return edit


def sos_ids(ids):
    def edit(p):
        for c, i in enumerate(ids):
            p[1 + 2 * c] = i
    return edit


def one_component_scan(p):
    return bytearray([1, p[1], p[2]]) + p[-3:]


REJECTS = [
    ("progressive", lambda d: set_marker(d, 0xC0, 0xC2), r"progressive \(SOF2\)"),
    ("lossless", lambda d: set_marker(d, 0xC0, 0xC3), r"lossless \(SOF3\)"),
    ("arithmetic", lambda d: set_marker(d, 0xC0, 0xC9), r"arithmetic coding \(SOF9\)"),
    ("arithmetic progressive", lambda d: set_marker(d, 0xC0, 0xCA), r"arithmetic coding, progressive"),
    ("12 bit", lambda d: patched(d, 0xC0, set_byte(0, 12)), "12-bit precision"),
    ("16-bit quant", lambda d: patched(d, 0xDB, set_byte(0, 0x10)), "16-bit quant tables"),
    ("4 components", lambda d: patched(d, 0xC0, sof_components(four=True)), "4 components"),
    ("adobe rgb", lambda d: d[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + d[2:], "Adobe transform 0"),
    ("ids rgb", lambda d: patched(patched(d, 0xC0, sof_components(ids=b"RGB")), 0xDA, sos_ids(b"RGB")), "component ids 'R', 'G', 'B'"),
    ("partial scan", lambda d: patched(d, 0xDA, one_component_scan), "multiple scans: the first scan covers 1 of the 3"),
    ("second scan", lambda d: d[:-2] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00\x00" + b"\xff\xd9", "multiple scans: a second SOS marker"),
    ("spectral selection", lambda d: patched(d, 0xDA, set_byte(-2, 5)), "sequential scans only"),
    ("4:4:0", lambda d: patched(d, 0xC0, sof_components(sampling0=0x12)), "sampling 1x2, 1x1, 1x1"),
    ("4:1:1", lambda d: patched(d, 0xC0, sof_components(sampling0=0x41)), "sampling 4x1, 1x1, 1x1"),
    ("height 0", lambda d: patched(d, 0xC0, lambda p: p.__setitem__(slice(1, 3), b"\x00\x00")), "a dimension of 0 x 9"),
    ("width above the limit", lambda d: patched(d, 0xC0, lambda p: p.__setitem__(slice(3, 5), b"\x10\x01")), "a dimension of 17 x 4097"),
    ("missing quant table", lambda d: patched(d, 0xC0, set_byte(8, 3)), "names a table no segment defined"),
    ("missing huffman table", lambda d: patched(d, 0xDA, set_byte(2, 0x33)), "names a table no segment defined"),
    # the standard DC table has five codes of length 3: three of them claimed as codes of length 1
    ("no prefix code", lambda d: patched(d, 0xC4, lambda p: (p.__setitem__(1, 3), p.__setitem__(3, p[3] - 3)) and None), None),
    ("not a jpeg", lambda d: b"\x89PNG" + d, "not a JPEG"),
    ("EOI before the scan", lambda d: d[:2] + b"\xff\xd9", "EOI before any scan"),
]


@pytest.mark.parametrize("case", REJECTS, ids=[r[0] for r in REJECTS])
def test_parser_rejects_by_its_own_message(case):
    dd, ops = mods()
    _, make, message = case
    data = make(base())
    if message is None:     # the table is interned -- and found to be no prefix code -- when the batch is planned
        fr = dd.parse_jpeg(data)
        with pytest.raises(dd.UnsupportedJpeg, match="no prefix code"):
            dd.jpeg_batch_plan([fr])
        return
    with pytest.raises(dd.UnsupportedJpeg, match=message):
        dd.parse_jpeg(data)


@pytest.mark.parametrize("sampling", ["420", "gray"])
def test_header_cut_at_every_marker_boundary_and_inside_every_segment(sampling):
    dd, _ = mods()
    data = base(sampling)
    segs = segments(data)
    assert [s[0] for s in segs][-1] == 0xDA and len(segs) >= 5
    cuts = set()
    for m, lo, hi in segs:
        cuts |= {lo, lo + 1, lo + 2, lo + 3, (lo + hi) // 2, hi - 1}
    for cut in sorted(c for c in cuts if c < segs[-1][2]):
        with pytest.raises(dd.UnsupportedJpeg, match="header ends early|not a JPEG"):
            dd.parse_jpeg(data[:cut])
    dd.parse_jpeg(data[:segs[-1][2]])    # the whole header with an empty scan parses: the scan's end is the decoder's business


# ---- the Huffman tables ------------------------------------------------------------------------------------------------------------
def test_huffman_tables_against_brute_force():
    dd, ops = mods()
    rng = np.random.default_rng(5)
    tables = []
    for fr in (dd.parse_jpeg(J.fixture()[n][0]) for n in ("33x47_420_q100_noise", "33x47_444_q85_noise_opt", "8x8_gray_q85_noise_opt")):
        tables += list(fr.huff_dc.values()) + list(fr.huff_ac.values())
    bits = np.zeros(16, dtype=np.uint8)       # a full tree of sixteen lengths: one code each, two of length 16 minus the all-ones code
    bits[:] = 1
    tables.append((bits, np.arange(16, dtype=np.uint8)))
    bits = np.zeros(16, dtype=np.uint8)
    bits[8], bits[9], bits[15] = 200, 40, 16  # codes around the look-ahead's 9 bits, and 16-bit ones
    tables.append((bits, rng.permutation(256).astype(np.uint8)))
    for bits, values in tables:
        row = dd.huffman_table(bits, values)
        codes, code, at = {}, 0, 0             # T.81 annex C: codes of one length are consecutive, the next length starts at (last + 1) << 1
        for l in range(1, 17):
            for _ in range(int(bits[l - 1])):
                codes[(l, code)] = int(values[at])
                code, at = code + 1, at + 1
            code <<= 1
        assert len(codes) == len(values)
        taken = np.zeros(1 << 16, dtype=bool)
        for (l, code), sym in codes.items():
            lo, n = code << (16 - l), 1 << (16 - l)
            taken[lo:lo + n] = True
            for window in {lo, lo + n - 1, lo + int(rng.integers(n))}:
                assert ops.jpeg_huffman_symbol(row, window) == (l, sym), (l, code, window)
        free = np.flatnonzero(~taken)
        for window in free[:: max(1, len(free) // 50)].tolist():
            assert ops.jpeg_huffman_symbol(row, window) == (0, 0), window
    with pytest.raises(dd.UnsupportedJpeg, match="no prefix code"):
        dd.huffman_table([3] + [0] * 15, [1, 2, 3])
    with pytest.raises(dd.UnsupportedJpeg, match="bad Huffman table"):
        dd.huffman_table([1] + [0] * 15, [1, 2])


# ---- the arithmetic against Pillow --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(J.fixture()))
def test_reference_equals_the_pillow_fixture(name):
    data, px = J.fixture()[name]
    got, status = decode_one(data)      # parse_jpeg raising here would be a failure: no accepted case is skipped or falls back
    assert status == 0
    assert got.shape == px.shape and np.array_equal(got, px), "%s: %d of %d bytes differ from Pillow's" % (name, int((got != px).sum()), px.size)


def test_the_fixture_covers_what_it_says():
    names = list(J.fixture())
    for shape in J.SHAPES:
        for sampling in J.SAMPLINGS:
            assert J.names(shape, sampling), (shape, sampling)
    for tag in ("_q30_", "_q100_", "_opt", "_rst3", "_rstrow", "_saturated"):
        assert [n for n in names if tag in n], tag
    dd, _ = mods()
    q100 = dd.parse_jpeg(J.fixture()["33x47_420_q100_noise"][0])
    assert all((t == 1).all() for t in q100.quant.values())         # quality 100: all-ones tables, the largest coefficients
    sat = J.fixture()["33x47_444_q75_saturated"][1]
    assert (sat == 0).any() and (sat == 255).any()                   # the colour clamp is reached


def test_one_batch_interns_the_tables_and_keeps_the_frame_order():
    dd, ops = mods()
    names = [n for n in J.fixture() if not n.startswith("256x128")]
    plan = dd.jpeg_batch_plan([dd.parse_jpeg(J.fixture()[n][0]) for n in names])
    standard = [i for i, n in enumerate(names) if "_opt" not in n]
    assert len(np.unique(plan.desc[standard][:, ops.JD_DC0:ops.JD_AC0 + 3])) <= 4      # one encoder's standard tables: 2 DC + 2 AC
    assert plan.ws_blocks == sum(ops.jpeg_frame_blocks(h, w, s) for h, w, s in plan.desc[:, [ops.JD_H, ops.JD_W, ops.JD_SAMP]].tolist())
    assert (plan.desc[:, ops.JD_OFF] % ops.JPEG_SCAN_ALIGN == 0).all() and plan.scans.size % ops.JPEG_SCAN_ALIGN == 0
    ends = plan.desc[:, ops.JD_OFF] + plan.desc[:, ops.JD_LEN]
    assert (np.append(plan.desc[1:, ops.JD_OFF], plan.scans.size) - ends >= ops.JPEG_SCAN_PAD).all()
    clip, status = ops.jpeg_decode_reference(plan)
    want, sizes = J.container([J.fixture()[n][1] for n in names])
    assert not status.any() and np.array_equal(plan.sizes, sizes) and np.array_equal(clip.numpy(), want)


def test_reference_equals_live_pillow_on_fresh_frames():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(9)
    for k, (h, w) in enumerate(((23, 31), (40, 24), (9, 70))):
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        px[h // 2:] = (px[h // 2:] // 64) * 85                        # half noise, half flat patches
        for sub, kw in ((0, {}), (1, dict(optimize=True)), (2, dict(restart_marker_rows=1)), (None, {})):
            buf = io.BytesIO()
            img = Image.fromarray(px[..., 0]) if sub is None else Image.fromarray(px)
            img.save(buf, "JPEG", quality=(50, 90, 97)[k], **(kw if sub is None else dict(kw, subsampling=sub)))
            want = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
            got, status = decode_one(buf.getvalue())
            assert status == 0 and np.array_equal(got, want), (h, w, sub)


# ---- broken scans ----------------------------------------------------------------------------------------------------------------
BROKEN = ("33x47_420_q75_noise_rst3", "33x47_444_q100_noise", "256x128_420_q75_smooth")


@pytest.mark.parametrize("name", BROKEN)
def test_broken_scans_end_in_a_status(name):
    dd, ops = mods()
    fr = dd.parse_jpeg(J.fixture()[name][0])
    good = dd.parse_jpeg(J.fixture()["17x9_422_q30_noise"][0])
    plan = dd.jpeg_batch_plan([good, J.broken(fr, "cut"), good, J.broken(fr, "noise")])
    clip, status = ops.jpeg_decode_reference(plan)
    status = status.tolist()
    assert status[0] == status[2] == 0 and np.array_equal(clip[0, :17, :9].numpy(), J.fixture()["17x9_422_q30_noise"][1])
    assert torch.equal(clip[0], clip[2])
    # half a scan: the reader passes its end (1) -- or, with restart intervals, misses the next marker (4)
    assert status[1] in ((ops.JPEG_ERR_END, ops.JPEG_ERR_MARKER) if fr.restart_interval else (ops.JPEG_ERR_END,)), status
    assert status[3] in (ops.JPEG_ERR_END, ops.JPEG_ERR_CODE, ops.JPEG_ERR_INDEX, ops.JPEG_ERR_MARKER), status
    again = ops.jpeg_decode_reference(plan)
    assert torch.equal(again[0], clip) and again[1].tolist() == status


def test_decoder_falls_back_to_pillow_and_counts(caplog):
    pytest.importorskip("PIL.Image")
    dd, _ = mods()
    fx = J.fixture()
    good = ["17x9_420_q30_noise", "16x16_gray_q100_noise", "33x47_422_q85_noise_opt"]
    data = [fx[n][0] for n in good]
    progressive_px = fx["8x8_444_q30_noise"][1]
    import PIL.Image as Image
    buf = io.BytesIO()
    Image.fromarray(progressive_px).save(buf, "JPEG", quality=90, progressive=True)
    want_prog = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    # a scan the device gives up on (status 4: the first restart marker carries the wrong number) and libjpeg resynchronises over
    rst = fx["33x47_420_q75_noise_rst3"][0]
    at = rst.index(bytes(dd.parse_jpeg(rst).scan))
    cut = rst[:at] + rst[at:].replace(b"\xff\xd0", b"\xff\xd3", 1)
    assert cut != rst and decode_one(cut)[1] == 4
    dec = dd.DeviceJpegDecoder("cpu")
    with caplog.at_level(logging.WARNING, logger="torchreid.device_decode"):
        imgs, sizes = dec.decode([data[0], buf.getvalue(), data[1], cut, data[2], data[0]], shape=(3, 2))
    assert imgs.shape == (3, 2, 33, 47, 3) and sizes.shape == (3, 2, 2) and imgs.dtype == torch.uint8
    assert dec.frames == 6 and dec.fallback_frames == 2 and "2 of 6 frames took the Pillow fallback" in caplog.text
    flat, s = imgs.view(6, 33, 47, 3).numpy(), sizes.reshape(6, 2)
    for k, want in enumerate((fx[good[0]][1], want_prog, fx[good[1]][1], None, fx[good[2]][1], fx[good[0]][1])):
        if want is not None:
            assert tuple(s[k]) == want.shape[:2] and np.array_equal(flat[k, :s[k, 0], :s[k, 1]], want), k
    assert tuple(s[3]) == (33, 47)       # the damaged file: whatever Pillow makes of it, in its slot
    assert np.array_equal(flat[3], dd.pillow_decode(cut))
    with pytest.raises(ValueError, match="do not fill shape"):
        dec.decode(data, shape=(2, 2))
    truncated = J.broken_file(fx["33x47_444_q100_noise"][0], dd.parse_jpeg(fx["33x47_444_q100_noise"][0]), "cut")
    with pytest.raises(dd.UnsupportedJpeg, match="frame 1: device status 1, and Pillow cannot decode it either"):
        dec.decode([data[0], truncated])


def test_decoder_without_pillow_raises_with_the_frame_index(monkeypatch):
    dd, _ = mods()

    def no_pillow(data):
        raise ImportError("No module named 'PIL'")

    monkeypatch.setattr(dd, "pillow_decode", no_pillow)
    fx = J.fixture()
    d = fx["17x9_420_q30_noise"][0]
    with pytest.raises(dd.UnsupportedJpeg, match=r"frame 1: progressive \(SOF2\).*Pillow, the fallback, cannot be imported"):
        dd.DeviceJpegDecoder("cpu").decode([d, set_marker(d, 0xC0, 0xC2)])
    cut = J.broken_file(d, dd.parse_jpeg(d), "cut")
    with pytest.raises(dd.UnsupportedJpeg, match=r"frame 2: device status 1 .*cannot be imported"):
        dd.DeviceJpegDecoder("cpu").decode([d, d, cut])


# ---- the 5-tuple contract --------------------------------------------------------------------------------------------------------
def test_decode_batches_feeds_extract_features(monkeypatch):
    """JPEG bytes -> decode_batches -> extract_features(frame_size=...) equals the fixture's Pillow pixels handed over as decoded frames
    with their valid extents. On the CPU the resample is the reference's (the device wrapper refuses host frames)."""
    from torchreid import evaluation, hip_ops as ops
    monkeypatch.setattr(ops, "clip_resample", lambda frames, geometry, out_hw, out=None: ops.clip_resample_reference(frames, geometry, out_hw))
    fx = J.fixture()
    order = ["17x9_420_q30_noise", "16x16_444_q100_noise", "33x47_gray_q30_noise", "8x8_422_q30_noise", "33x47_420_q75_noise_rst3",
             "16x16_420_q85_noise_opt", "17x9_gray_q100_noise", "33x47_422_q75_saturated"]
    S = 2
    model = DS.StubModel()
    adj = torch.rand((len(order) // S, DS.V, DS.V), generator=torch.Generator().manual_seed(1))
    pids, cams = np.arange(len(order) // S), np.zeros(len(order) // S, dtype=np.int64)

    def encoded():
        for i in range(0, len(order) // S, 2):
            yield ([[fx[n][0] for n in order[S * t:S * t + S]] for t in (i, i + 1)], pids[i:i + 2], cams[i:i + 2], adj[i:i + 2])

    def decoded():
        for i in range(0, len(order) // S, 2):
            box, sizes = J.container([fx[n][1] for n in order[S * i:S * i + 2 * S]])
            yield (torch.from_numpy(box).view((2, S) + box.shape[1:]), pids[i:i + 2], cams[i:i + 2], adj[i:i + 2], sizes.reshape(2, S, 2))

    items = list(evaluation.decode_batches(encoded(), torch.device("cpu")))
    assert all(len(it) == 5 and it[0].dtype == torch.uint8 and it[0].dim() == 5 and it[0].shape[-1] == 3 for it in items)
    assert np.array_equal(items[0][4], np.array([[(17, 9), (16, 16)], [(33, 47), (8, 8)]]))
    got = evaluation.extract_features(model, iter(items), frame_size=(16, 8), prefetch=False)
    want = evaluation.extract_features(model, decoded(), frame_size=(16, 8), prefetch=False)
    assert got[0].shape == (4, DS.PIX + DS.ADJ) and torch.equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the dense shape [b][n][S] and tensors passing through
    nested = [([[[fx[n][0] for n in order[:2]], [fx[n][0] for n in order[2:4]]]], pids[:1], cams[:1], adj[:2].view(1, 2, DS.V, DS.V))]
    (item,) = list(evaluation.decode_batches(nested, torch.device("cpu")))
    assert item[0].shape == (1, 2, S, 33, 47, 3) and item[4].shape == (1, 2, S, 2)
    assert torch.equal(item[0].view(4, 33, 47, 3), items[0][0].view(4, 33, 47, 3))
    through = (torch.zeros((1, S, 8, 4, 3), dtype=torch.uint8), pids[:1], cams[:1], adj[:1])
    assert list(evaluation.decode_batches([through], torch.device("cpu")))[0] is through
    with pytest.raises(ValueError, match="nested list"):
        list(evaluation.decode_batches([([fx[order[0]][0]], pids[:1], cams[:1], adj[:1])], torch.device("cpu")))
