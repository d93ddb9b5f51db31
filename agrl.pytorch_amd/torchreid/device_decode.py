"""Baseline JPEG decode on the device: the host parses HEADERS, the GPU decodes the pixels.

The reference reads every frame with ``Image.open(path).convert('RGB')`` (dataset_loader.py:23-36); MARS and DukeMTMC-VideoReID are JPEG.
Here the host walks the markers of each file (``parse_jpeg``), interns the quantisation and Huffman tables of a batch and lays the
entropy-coded scans end to end (``jpeg_batch_plan``); ``hip_ops.jpeg_decode`` (agrl_jpeg_decode_u8) does the entropy decoding, the
IDCT, the chroma upsampling and the colour conversion, byte for byte what Pillow (libjpeg-turbo) returns. The host never touches an
entropy-coded bit -- the rule of device_transforms ("geometry, not pixels") applied to decode. The result is what everything downstream
already takes: uint8 channel-last frames in a padded container plus each frame's valid (height, width).

    accepted                                                   rejected (UnsupportedJpeg, before anything touches the GPU)
    --------------------------------------------------------   ----------------------------------------------------------------
    SOF0 / SOF1, 8-bit samples, 8-bit quantisation tables       progressive (SOF2), arithmetic, lossless, hierarchical coding
    Huffman coding, ONE interleaved scan over all components    12-bit samples, 16-bit quantisation tables, several scans
    1 component (grayscale), or 3 components YCbCr with luma    4 components, Adobe transform 0 (RGB-coded), component ids R, G, B
    sampling (1,1), (2,1) or (2,2) and chroma (1,1)             any other sampling (4:4:0, 4:1:1, ...)
    DRI / RSTn restart intervals                                a dimension of 0 or above JPEG_MAX_DIM (4096)
    APPn / COM skipped; EXIF orientation ignored, as            a header that ends early, a table the scan names but no segment
    convert('RGB') ignores it                                   defined, a Huffman table that is no prefix code

Rejected files and frames the device reports a non-zero status for (a broken scan) take the FALLBACK: Pillow on the host, when it can
be imported; otherwise the error is raised with the frame's index. ``DeviceJpegDecoder`` logs how many frames took it.

PNG (iLIDS-VID, PRID2011) has its own half of this module, below: ``parse_png``, ``png_batch_plan``, ``DevicePngDecoder``; and
``DeviceImageDecoder`` takes a batch of both. OUT OF SCOPE: file reading, dataset classes.
"""
from __future__ import annotations

import io
import logging
import struct
import zlib
from collections import namedtuple

import numpy as np
import torch

from torchreid import hip_ops as ops

log = logging.getLogger(__name__)

JPEG_MAX_DIM = ops.JPEG_MAX_DIM


class UnsupportedJpeg(ValueError):
    """The byte string is not a JPEG of the subset the device decodes."""


JpegFrame = namedtuple("JpegFrame", "height width components sampling quant huff_dc huff_ac restart_interval scan")
JpegFrame.__doc__ = """One parsed file. components: ((id, h, v, quant index, dc index, ac index), ...); sampling: hip_ops.JPEG_GRAY / _444 /
_422 / _420; quant: {index: uint16 (64,) natural order}; huff_dc / huff_ac: {index: (bits uint8 (16,), values uint8 (n,))};
scan: the entropy-coded segment, a memoryview into the file's bytes."""

JpegPlan = namedtuple("JpegPlan", "scans desc quant huff sizes container ws_blocks")
JpegPlan.__doc__ = """The device operands of one batch, host side. scans: uint8 (bytes,), every scan at a multiple of JPEG_SCAN_ALIGN
with at least JPEG_SCAN_PAD zero bytes behind it; desc: int32 (F, 16) rows (scan offset, scan length, H, W, sampling code, restart
interval, quant index x 3, DC table index x 3, AC table index x 3, first workspace block); quant: uint16 (NQ, 64) natural order;
huff: int32 (NH, 360) decode-ready tables (``huffman_table``); sizes: int64 (F, 2) = (H, W); container: (Hmax, Wmax); ws_blocks:
8x8 blocks of all frames together."""

_SOF_NAMES = {0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "hierarchical (SOF5)", 0xC6: "hierarchical progressive (SOF6)",
              0xC7: "hierarchical lossless (SOF7)", 0xC9: "arithmetic coding (SOF9)", 0xCA: "arithmetic coding, progressive (SOF10)",
              0xCB: "arithmetic coding, lossless (SOF11)", 0xCD: "arithmetic coding, hierarchical (SOF13)",
              0xCE: "arithmetic coding, hierarchical progressive (SOF14)", 0xCF: "arithmetic coding, hierarchical lossless (SOF15)"}
_SAMPLING = {((1, 1), (1, 1), (1, 1)): ops.JPEG_444, ((2, 1), (1, 1), (1, 1)): ops.JPEG_422, ((2, 2), (1, 1), (1, 1)): ops.JPEG_420}


def huffman_table(bits, values):
    """A DHT table -- ``bits``: how many codes have length 1..16, ``values``: the symbols in code order -- in libjpeg's decode-ready shape
    -> int32 (JPEG_HUFF_WORDS,): a 9-bit look-ahead table (512 uint16: code length << 8 | symbol for every 9-bit window that starts with a
    code of at most 9 bits, else 0), maxcode[17] (the largest code of each length, -1 where there is none), valoffset[17] (index of the
    length's first symbol minus its first code) and the 256 symbols. UnsupportedJpeg when the counts do not describe a prefix code."""
    bits = np.asarray(bits, dtype=np.int64).reshape(-1)
    values = np.asarray(values, dtype=np.int64).reshape(-1)
    if bits.size != 16 or bits.min() < 0 or int(bits.sum()) != values.size or values.size > 256 or (values.size and (values.min() < 0 or values.max() > 255)):
        raise UnsupportedJpeg("bad Huffman table: %d symbols for counts %s" % (values.size, bits.tolist()))
    row = np.zeros(ops.JPEG_HUFF_WORDS, dtype=np.int32)
    look = row[ops.JH_LOOK:ops.JH_LOOK + 256].view(np.uint16)
    row[ops.JH_MAXCODE:ops.JH_MAXCODE + 17] = -1
    row[ops.JH_VAL:ops.JH_VAL + 64].view(np.uint8)[:values.size] = values
    code = at = 0
    for l in range(1, 17):
        n = int(bits[l - 1])
        if code + n > (1 << l):
            raise UnsupportedJpeg("bad Huffman table: %d codes of length %d from code %d on are no prefix code" % (n, l, code))
        if n:
            row[ops.JH_VALOFF + l] = at - code
            row[ops.JH_MAXCODE + l] = code + n - 1
            if l <= ops.JPEG_LOOK:
                for i in range(n):
                    lo = (code + i) << (ops.JPEG_LOOK - l)
                    look[lo:lo + (1 << (ops.JPEG_LOOK - l))] = (l << 8) | int(values[at + i])
            code, at = code + n, at + n
        code <<= 1
    return row


def _segment(data, at, what):
    """the payload bounds of the marker segment whose length field starts at ``at``"""
    if at + 2 > len(data):
        raise UnsupportedJpeg("header ends early: inside the length of %s at byte %d" % (what, at))
    n = (data[at] << 8) | data[at + 1]
    if n < 2 or at + n > len(data):
        raise UnsupportedJpeg("header ends early: %s at byte %d says %d bytes, %d are left" % (what, at, n, len(data) - at))
    return at + 2, at + n


def parse_jpeg(data):
    """Walk the markers of one file -> JpegFrame; UnsupportedJpeg, each case by its own message, for everything outside the subset in the
    module's table. Only headers are read: the entropy-coded segment is returned as a view, from behind the SOS header to the first
    marker that is neither a stuffed ``FF 00`` nor a restart marker (or to the end of the data)."""
    data = bytes(data) if not isinstance(data, (bytes, bytearray)) else data
    if len(data) < 2 or data[0] != 0xFF or data[1] != 0xD8:
        raise UnsupportedJpeg("not a JPEG: no SOI marker at the start")
    quant, huff_dc, huff_ac = {}, {}, {}
    frame = None
    ri = 0
    adobe_transform = None
    at = 2
    while True:
        if at + 2 > len(data):
            raise UnsupportedJpeg("header ends early: no SOS marker before byte %d" % len(data))
        if data[at] != 0xFF:
            raise UnsupportedJpeg("not a JPEG: byte %#x at %d where a marker should stand" % (data[at], at))
        m = data[at + 1]
        if m == 0xFF:          # fill byte
            at += 1
            continue
        at += 2
        if m == 0xD9:
            raise UnsupportedJpeg("header ends early: EOI before any scan")
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in _SOF_NAMES:
            raise UnsupportedJpeg("%s is not decoded on the device" % _SOF_NAMES[m])
        lo, hi = _segment(data, at, "marker %#x" % m)
        seg = data[lo:hi]
        if m in (0xC0, 0xC1):
            if frame is not None:
                raise UnsupportedJpeg("a second frame header")
            if len(seg) < 6 or len(seg) < 6 + 3 * seg[5]:
                raise UnsupportedJpeg("header ends early: the frame header is %d bytes" % len(seg))
            if seg[0] != 8:
                raise UnsupportedJpeg("%d-bit precision: 8-bit samples only" % seg[0])
            H, W, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if H < 1 or W < 1 or H > JPEG_MAX_DIM or W > JPEG_MAX_DIM:
                raise UnsupportedJpeg("a dimension of %d x %d: 1..%d each" % (H, W, JPEG_MAX_DIM))
            if nc not in (1, 3):
                raise UnsupportedJpeg("%d components: grayscale or YCbCr only" % nc)
            frame = (H, W, [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)])
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                pq, tq = seg[p] >> 4, seg[p] & 15
                if pq != 0:
                    raise UnsupportedJpeg("16-bit quant tables: 8-bit ones only")
                if tq > 3 or p + 65 > len(seg):
                    raise UnsupportedJpeg("header ends early: a quantisation table of %d bytes" % (len(seg) - p))
                t = np.zeros(64, dtype=np.uint16)
                t[ops.JPEG_ZIGZAG] = np.frombuffer(seg, dtype=np.uint8, count=64, offset=p + 1)
                quant[tq] = t
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                tc, th = seg[p] >> 4, seg[p] & 15
                if tc > 1 or th > 3 or p + 17 > len(seg):
                    raise UnsupportedJpeg("header ends early: a Huffman table header of %d bytes (class %d, index %d)" % (len(seg) - p, tc, th))
                bits = np.frombuffer(seg, dtype=np.uint8, count=16, offset=p + 1)
                n = int(bits.sum())
                if p + 17 + n > len(seg):
                    raise UnsupportedJpeg("header ends early: a Huffman table of %d symbols in %d bytes" % (n, len(seg) - p - 17))
                (huff_ac if tc else huff_dc)[th] = (bits.copy(), np.frombuffer(seg, dtype=np.uint8, count=n, offset=p + 17).copy())
                p += 17 + n
        elif m == 0xDD:
            if len(seg) < 2:
                raise UnsupportedJpeg("header ends early: a restart interval of %d bytes" % len(seg))
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xEE and len(seg) >= 12 and bytes(seg[:5]) == b"Adobe":
            adobe_transform = seg[11]
        elif m == 0xDA:
            break
        at = hi
    if frame is None:
        raise UnsupportedJpeg("a scan before any frame header")
    H, W, comps = frame
    nc = len(comps)
    if not len(seg) or len(seg) < 4 + 2 * seg[0]:
        raise UnsupportedJpeg("header ends early: the scan header is %d bytes" % len(seg))
    if seg[0] != nc or [seg[1 + 2 * c] for c in range(nc)] != [c[0] for c in comps]:
        raise UnsupportedJpeg("multiple scans: the first scan covers %d of the %d components" % (seg[0], nc))
    if (seg[1 + 2 * nc], seg[2 + 2 * nc], seg[3 + 2 * nc]) != (0, 63, 0):
        raise UnsupportedJpeg("a scan of coefficients %d..%d, approximation %#x: sequential scans only" % (seg[1 + 2 * nc], seg[2 + 2 * nc], seg[3 + 2 * nc]))
    if nc == 3:
        if adobe_transform == 0:
            raise UnsupportedJpeg("Adobe transform 0: the components are RGB, not YCbCr")
        if [c[0] for c in comps] == [ord("R"), ord("G"), ord("B")]:
            raise UnsupportedJpeg("component ids 'R', 'G', 'B': the components are RGB, not YCbCr")
        sampling = _SAMPLING.get(tuple((c[1], c[2]) for c in comps))
        if sampling is None:
            raise UnsupportedJpeg("sampling %s: 4:4:4, 4:2:2 (2x1) and 4:2:0 (2x2) only" % ", ".join("%dx%d" % (c[1], c[2]) for c in comps))
    else:
        sampling = ops.JPEG_GRAY        # a one-component scan has one block per MCU whatever its sampling factors say
    components = []
    for c, (cid, h, v, tq) in enumerate(comps):
        td, ta = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
        if tq not in quant or td not in huff_dc or ta not in huff_ac:
            raise UnsupportedJpeg("component %d names a table no segment defined (quant %d, DC %d, AC %d)" % (cid, tq, td, ta))
        if huff_dc[td][1].size and int(huff_dc[td][1].max()) > 11:
            raise UnsupportedJpeg("DC table %d has a category of %d: 0..11 for 8-bit samples" % (td, int(huff_dc[td][1].max())))
        components.append((cid, h, v, tq, td, ta))
    # the entropy-coded segment: up to the first marker that is neither FF 00 nor RSTn
    start, end = hi, len(data)
    p = data.find(b"\xff", start)
    while p != -1 and p + 1 < len(data):
        if data[p + 1] == 0 or 0xD0 <= data[p + 1] <= 0xD7:
            p = data.find(b"\xff", p + 2)
            continue
        if data[p + 1] == 0xFF:
            p = data.find(b"\xff", p + 1)
            continue
        end = p
        break
    # what follows the scan: another SOS is a second scan
    p = end
    while p + 4 <= len(data) and data[p] == 0xFF:
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0xD9:
            break
        if m == 0xDA:
            raise UnsupportedJpeg("multiple scans: a second SOS marker at byte %d" % p)
        n = (data[p + 2] << 8) | data[p + 3]
        if n < 2:
            break
        p += 2 + n
    return JpegFrame(H, W, tuple(components), sampling, quant, huff_dc, huff_ac, ri, memoryview(data)[start:end])


def jpeg_batch_plan(frames):
    """JpegFrames -> JpegPlan, the operands of ONE decode launch: the scans laid end to end (aligned and zero-padded: the device reads
    whole words), one descriptor row per frame, and the tables interned -- files of one encoder share them, so a batch normally holds
    2 quantisation + 4 Huffman tables whatever its size."""
    frames = list(frames)
    qkeys, hkeys, qrows, hrows = {}, {}, [], []

    def intern_q(t):
        key = t.tobytes()
        if key not in qkeys:
            qkeys[key] = len(qrows)
            qrows.append(t)
        return qkeys[key]

    def intern_h(bits_values):
        key = (bits_values[0].tobytes(), bits_values[1].tobytes())
        if key not in hkeys:
            hkeys[key] = len(hrows)
            hrows.append(huffman_table(*bits_values))
        return hkeys[key]

    desc = np.zeros((len(frames), ops.JPEG_DESC), dtype=np.int32)
    chunks, at, ws = [], 0, 0
    for f, fr in enumerate(frames):
        n = len(fr.scan)
        room = -(-(n + ops.JPEG_SCAN_PAD) // ops.JPEG_SCAN_ALIGN) * ops.JPEG_SCAN_ALIGN
        chunk = np.zeros(room, dtype=np.uint8)
        chunk[:n] = np.frombuffer(fr.scan, dtype=np.uint8)
        chunks.append(chunk)
        d = desc[f]
        d[ops.JD_OFF], d[ops.JD_LEN], d[ops.JD_H], d[ops.JD_W] = at, n, fr.height, fr.width
        d[ops.JD_SAMP], d[ops.JD_RI], d[ops.JD_WS] = fr.sampling, fr.restart_interval, ws
        for c, (_, _, _, tq, td, ta) in enumerate(fr.components):
            d[ops.JD_Q0 + c], d[ops.JD_DC0 + c], d[ops.JD_AC0 + c] = intern_q(fr.quant[tq]), intern_h(fr.huff_dc[td]), intern_h(fr.huff_ac[ta])
        at += room
        ws += ops.jpeg_frame_blocks(fr.height, fr.width, fr.sampling)
        if at >= 2 ** 31 or ws >= 2 ** 24:
            raise ValueError("jpeg_batch_plan: the batch is too large for one launch at frame %d (%d scan bytes, %d blocks)" % (f, at, ws))
    sizes = np.array([(fr.height, fr.width) for fr in frames], dtype=np.int64).reshape(len(frames), 2)
    return JpegPlan(np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.uint8), desc,
                    np.stack(qrows) if qrows else np.zeros((0, 64), dtype=np.uint16),
                    np.stack(hrows) if hrows else np.zeros((0, ops.JPEG_HUFF_WORDS), dtype=np.int32), sizes,
                    (int(sizes[:, 0].max()) if len(frames) else 0, int(sizes[:, 1].max()) if len(frames) else 0), ws)


def pillow_decode(data):
    """the reference's own decode, ``Image.open(...).convert('RGB')`` -> uint8 (H, W, 3); ImportError without Pillow"""
    from PIL import Image
    with Image.open(io.BytesIO(bytes(data))) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


def _nested(items, path=()):
    """flatten a nested list of byte strings -> (list of bytes, shape); every level must be rectangular"""
    if isinstance(items, (bytes, bytearray, memoryview)):
        return [items], ()
    flat, shapes = [], []
    for it in items:
        sub, shape = _nested(it)
        flat.extend(sub)
        shapes.append(shape)
    if len(set(shapes)) > 1:
        raise ValueError("the nested list of encoded frames is not rectangular: %s" % sorted(set(shapes)))
    return flat, (len(shapes),) + (shapes[0] if shapes else ())


class DeviceJpegDecoder:
    """``DeviceJpegDecoder(device).decode(list_of_bytes, shape=None)``: encoded frames -> ``(imgs uint8 (*shape, Hmax, Wmax, 3) on the
    device, sizes int64 (*shape, 2))`` -- exactly the ``imgs`` and the fifth batch element that ``extract_features(frame_size=...)``,
    ``extract_features_packed`` and ``DeviceClipTransform`` take. ``shape``: the leading axes, e.g. (b, S) or (b, n, S); default
    (len(list),). Headers are parsed and the batch planned on the host, the compressed bytes uploaded from pinned memory on the
    caller's stream, and the device status is read ONCE per call (the call's one synchronisation). Frames outside the subset and
    frames with a non-zero status are decoded by Pillow on the host and copied into their slots -- or, without Pillow, the error is
    raised with the frame's index. ``fallback_frames`` / ``frames`` count over the decoder's life; every call that took the fallback
    logs how many frames did. On a CPU device the arithmetic's restatement (``hip_ops.jpeg_decode_reference``) decodes: the same bytes."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.frames = self.fallback_frames = 0

    def decode(self, encoded, shape=None):
        encoded = list(encoded)
        F = len(encoded)
        shape = (F,) if shape is None else tuple(int(v) for v in shape)
        if int(np.prod(shape, dtype=np.int64)) != F:
            raise ValueError("DeviceJpegDecoder.decode: %d frames do not fill shape %s" % (F, shape))
        parsed, fallback = [], {}
        for i, data in enumerate(encoded):
            try:
                parsed.append((i, parse_jpeg(data)))
            except UnsupportedJpeg as e:
                fallback[i] = self._fallback(i, data, e)
        plan = jpeg_batch_plan([fr for _, fr in parsed])
        sizes = np.zeros((F, 2), dtype=np.int64)
        for i, fr in parsed:
            sizes[i] = (fr.height, fr.width)
        for i, px in fallback.items():
            sizes[i] = px.shape[:2]
        Hc, Wc = (int(sizes[:, 0].max()), int(sizes[:, 1].max())) if F else (0, 0)
        plan = plan._replace(container=(Hc, Wc))
        cuda = self.device.type == "cuda"
        if parsed:
            if cuda:
                with torch.cuda.device(self.device):
                    clip, status = ops.jpeg_decode(plan, device=self.device)
                status = status.cpu().numpy()          # the one synchronisation of the call
            else:
                clip, status = ops.jpeg_decode_reference(plan)
                status = status.numpy()
        else:
            clip, status = torch.zeros((0, Hc, Wc, 3), dtype=torch.uint8, device=self.device), np.zeros(0, dtype=np.int32)
        for k in np.flatnonzero(status).tolist():
            i = parsed[k][0]
            fallback[i] = self._fallback(i, encoded[i], "device status %d" % int(status[k]))
            if fallback[i].shape[:2] != tuple(sizes[i]):
                raise UnsupportedJpeg("frame %d: Pillow decodes %s where the header says %s" % (i, fallback[i].shape[:2], tuple(sizes[i])))
        if len(parsed) == F:
            out = clip
        else:
            out = torch.zeros((F, Hc, Wc, 3), dtype=torch.uint8, device=self.device)
            if parsed:
                out[torch.as_tensor([i for i, _ in parsed], device=self.device)] = clip
        if fallback:
            host = torch.zeros((len(fallback), Hc, Wc, 3), dtype=torch.uint8)
            for k, (i, px) in enumerate(sorted(fallback.items())):
                host[k, :px.shape[0], :px.shape[1]] = torch.from_numpy(np.array(px, dtype=np.uint8))
            out[torch.as_tensor(sorted(fallback), device=self.device)] = host.to(self.device)
            log.warning("DeviceJpegDecoder: %d of %d frames took the Pillow fallback", len(fallback), F)
        self.frames += F
        self.fallback_frames += len(fallback)
        return out.view(shape + (Hc, Wc, 3)), sizes.reshape(shape + (2,))

    @staticmethod
    def _fallback(i, data, why):
        try:
            return pillow_decode(data)
        except ImportError:
            if isinstance(why, UnsupportedJpeg):
                raise UnsupportedJpeg("frame %d: %s (and Pillow, the fallback, cannot be imported)" % (i, why)) from why
            raise UnsupportedJpeg("frame %d: %s (and Pillow, the fallback, cannot be imported)" % (i, why))
        except OSError as e:     # what the reference's own read would raise for this file
            raise UnsupportedJpeg("frame %d: %s, and Pillow cannot decode it either: %s" % (i, why, e)) from e


# ---- PNG (iLIDS-VID, PRID2011): the sibling of the JPEG decoder ------------------------------------------------------------------------
# The host walks the CHUNKS of each file and never inflates; the device (hip_ops.png_decode, agrl_png_decode_u8) inflates the zlib
# stream and undoes the row filters, byte for byte what Pillow returns (PNG is lossless: there is no arithmetic to argue about).
#
#     accepted                                                   rejected (UnsupportedPng, before anything touches the GPU)
#     --------------------------------------------------------   ----------------------------------------------------------------
#     bit depth 8, colour type 0 (grey, replicated to RGB as      colour types 3 (palette), 4 and 6 (alpha); bit depths 1, 2, 4, 16
#     convert('RGB') does) and colour type 2 (RGB)                Adam7 interlacing; a tRNS chunk (transparency); an acTL chunk (APNG)
#     non-interlaced, any number of IDAT chunks                   a chunk whose CRC does not match, a chunk that ends early
#     any mix of stored / fixed / dynamic deflate blocks, any     an inflated size H * (1 + W * channels) above PNG_MAX_INFLATED, a
#     declared window                                             dimension of 0 or above PNG_MAX_DIM; anything that is not a PNG
#
# Rejected files and frames the device reports a non-zero status for (hip_ops.PNG_STATUS_NAMES: every one of inflate's own rejections,
# a wrong Adler-32, a filter byte above 4) take the same FALLBACK as JPEG: Pillow on the host, counted and logged.
PNG_MAX_DIM = ops.PNG_MAX_DIM
PNG_MAX_INFLATED = ops.PNG_MAX_INFLATED
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


class UnsupportedPng(ValueError):
    """The byte string is not a PNG of the subset the device decodes."""


PngFrame = namedtuple("PngFrame", "height width channels stream idat_sizes")
PngFrame.__doc__ = """One parsed file. channels: 1 (grey) or 3 (RGB); stream: the IDAT payloads joined, ONE zlib stream (bytes), not
inflated; idat_sizes: the payload length of each IDAT chunk, in order."""

PngPlan = namedtuple("PngPlan", "streams desc sizes container boundaries")
PngPlan.__doc__ = """The device operands of one batch, host side. streams: uint8 (bytes,), every zlib stream at a multiple of
PNG_STREAM_ALIGN with at least PNG_STREAM_PAD zero bytes behind it; desc: int32 (F, 8) rows (stream offset, stream length, H, W,
channels, three spare zeros); sizes: int64 (F, 2) = (H, W); container: (Hmax, Wmax); boundaries: per frame the byte offsets inside its
stream where one IDAT chunk ended and the next began (host only: the restatement's coverage counters read them)."""

_PNG_COLOUR = {3: "colour type 3 (palette)", 4: "colour type 4 (grey + alpha)", 6: "colour type 6 (RGB + alpha)"}


def parse_png(data):
    """Walk the chunks of one file -> PngFrame; UnsupportedPng, each case by its own message, for everything outside the subset in the
    table above. Signature, IHDR fields and EVERY chunk's CRC (zlib.crc32) are checked; the IDAT payloads are joined and returned as
    they are: nothing is inflated here."""
    data = bytes(data) if not isinstance(data, (bytes, bytearray)) else data
    if len(data) < 8 or bytes(data[:8]) != PNG_SIGNATURE:
        raise UnsupportedPng("not a PNG: no signature at the start")
    at, header, idat, seen_end = 8, None, [], False
    while at < len(data) and not seen_end:
        if at + 12 > len(data):
            raise UnsupportedPng("a chunk ends early: %d bytes at byte %d where a chunk needs 12" % (len(data) - at, at))
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        if at + 12 + n > len(data):
            raise UnsupportedPng("a chunk ends early: %r at byte %d says %d bytes, %d are left" % (kind, at, n, len(data) - at - 12))
        body = data[at + 8:at + 8 + n]
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        if zlib.crc32(data[at + 4:at + 8 + n]) & 0xFFFFFFFF != crc:
            raise UnsupportedPng("chunk CRC mismatch: %r at byte %d" % (kind, at))
        if header is None and kind != b"IHDR":
            raise UnsupportedPng("not a PNG: the first chunk is %r, not IHDR" % kind)
        if kind == b"IHDR":
            if header is not None or n != 13:
                raise UnsupportedPng("a second IHDR, or one of %d bytes" % n)
            W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            if colour in _PNG_COLOUR or colour not in (0, 2):
                raise UnsupportedPng("%s is not decoded on the device" % _PNG_COLOUR.get(colour, "colour type %d" % colour))
            if depth != 8:
                raise UnsupportedPng("bit depth %d: 8-bit samples only" % depth)
            if lace != 0:
                raise UnsupportedPng("Adam7 interlacing (interlace method %d) is not decoded on the device" % lace)
            if comp != 0 or filt != 0:
                raise UnsupportedPng("compression method %d, filter method %d: 0 and 0 only" % (comp, filt))
            if H < 1 or W < 1 or H > PNG_MAX_DIM or W > PNG_MAX_DIM:
                raise UnsupportedPng("a dimension of %d x %d: 1..%d each" % (H, W, PNG_MAX_DIM))
            channels = 3 if colour == 2 else 1
            if ops.png_frame_inflated(H, W, channels) > PNG_MAX_INFLATED:
                raise UnsupportedPng("a frame of %d x %d x %d inflates to %d bytes: over the size bound PNG_MAX_INFLATED = %d" % (
                    H, W, channels, ops.png_frame_inflated(H, W, channels), PNG_MAX_INFLATED))
            header = (H, W, channels)
        elif kind == b"tRNS":
            raise UnsupportedPng("a tRNS chunk (transparency) is not decoded on the device")
        elif kind == b"acTL":
            raise UnsupportedPng("an acTL chunk (animated PNG) is not decoded on the device")
        elif kind == b"IDAT":
            idat.append(bytes(body))
        elif kind == b"IEND":
            seen_end = True
        at += 12 + n
    if header is None:
        raise UnsupportedPng("not a PNG: no IHDR chunk")
    if not idat:
        raise UnsupportedPng("a PNG without an IDAT chunk")
    return PngFrame(header[0], header[1], header[2], b"".join(idat), tuple(len(b) for b in idat))


def png_batch_plan(frames):
    """PngFrames -> PngPlan, the operands of ONE decode launch: the zlib streams laid end to end (aligned and zero-padded: the device
    reads whole words, one ahead) and one descriptor row per frame."""
    frames = list(frames)
    desc = np.zeros((len(frames), ops.PNG_DESC), dtype=np.int32)
    chunks, at, boundaries = [], 0, []
    for f, fr in enumerate(frames):
        n = len(fr.stream)
        room = -(-(n + ops.PNG_STREAM_PAD) // ops.PNG_STREAM_ALIGN) * ops.PNG_STREAM_ALIGN
        chunk = np.zeros(room, dtype=np.uint8)
        chunk[:n] = np.frombuffer(fr.stream, dtype=np.uint8)
        chunks.append(chunk)
        d = desc[f]
        d[ops.PD_OFF], d[ops.PD_LEN], d[ops.PD_H], d[ops.PD_W], d[ops.PD_CH] = at, n, fr.height, fr.width, fr.channels
        boundaries.append(tuple(np.cumsum(fr.idat_sizes)[:-1].tolist()))
        at += room
        if at >= 2 ** 31:
            raise ValueError("png_batch_plan: the batch is too large for one launch at frame %d (%d stream bytes)" % (f, at))
    sizes = np.array([(fr.height, fr.width) for fr in frames], dtype=np.int64).reshape(len(frames), 2)
    return PngPlan(np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.uint8), desc, sizes,
                   (int(sizes[:, 0].max()) if len(frames) else 0, int(sizes[:, 1].max()) if len(frames) else 0), tuple(boundaries))


class DevicePngDecoder:
    """``DevicePngDecoder(device).decode(list_of_bytes, shape=None)``: the arguments, the return value and the counters of
    ``DeviceJpegDecoder.decode``, for PNG files: ``(imgs uint8 (*shape, Hmax, Wmax, 3) on the device, sizes int64 (*shape, 2))``. Chunks
    are walked and the batch planned on the host, the compressed bytes uploaded from pinned memory, and the device status is read ONCE
    per call. Files outside the subset and frames with a non-zero status are decoded by Pillow on the host and copied into their slots;
    where Pillow cannot decode a frame either (or cannot be imported), UnsupportedPng is raised with the frame's index. On a CPU
    device the restatement (``hip_ops.png_decode_reference``) decodes: the same bytes."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.frames = self.fallback_frames = 0

    def decode(self, encoded, shape=None):
        encoded = list(encoded)
        F = len(encoded)
        shape = (F,) if shape is None else tuple(int(v) for v in shape)
        if int(np.prod(shape, dtype=np.int64)) != F:
            raise ValueError("DevicePngDecoder.decode: %d frames do not fill shape %s" % (F, shape))
        parsed, fallback = [], {}
        for i, data in enumerate(encoded):
            try:
                parsed.append((i, parse_png(data)))
            except UnsupportedPng as e:
                fallback[i] = self._fallback(i, data, e)
        plan = png_batch_plan([fr for _, fr in parsed])
        sizes = np.zeros((F, 2), dtype=np.int64)
        for i, fr in parsed:
            sizes[i] = (fr.height, fr.width)
        for i, px in fallback.items():
            sizes[i] = px.shape[:2]
        Hc, Wc = (int(sizes[:, 0].max()), int(sizes[:, 1].max())) if F else (0, 0)
        plan = plan._replace(container=(Hc, Wc))
        if parsed:
            if self.device.type == "cuda":
                with torch.cuda.device(self.device):
                    clip, status = ops.png_decode(plan, device=self.device)
                status = status.cpu().numpy()          # the one synchronisation of the call
            else:
                clip, status = ops.png_decode_reference(plan)
                status = status.numpy()
        else:
            clip, status = torch.zeros((0, Hc, Wc, 3), dtype=torch.uint8, device=self.device), np.zeros(0, dtype=np.int32)
        for k in np.flatnonzero(status).tolist():
            i = parsed[k][0]
            fallback[i] = self._fallback(i, encoded[i], "device status %d (%s)" % (int(status[k]), ops.PNG_STATUS_NAMES[int(status[k])]))
            if fallback[i].shape[:2] != tuple(sizes[i]):
                raise UnsupportedPng("frame %d: Pillow decodes %s where the header says %s" % (i, fallback[i].shape[:2], tuple(sizes[i])))
        if len(parsed) == F:
            out = clip
        else:
            out = torch.zeros((F, Hc, Wc, 3), dtype=torch.uint8, device=self.device)
            if parsed:
                out[torch.as_tensor([i for i, _ in parsed], device=self.device)] = clip
        if fallback:
            host = torch.zeros((len(fallback), Hc, Wc, 3), dtype=torch.uint8)
            for k, (i, px) in enumerate(sorted(fallback.items())):
                host[k, :px.shape[0], :px.shape[1]] = torch.from_numpy(np.array(px, dtype=np.uint8))
            out[torch.as_tensor(sorted(fallback), device=self.device)] = host.to(self.device)
            log.warning("DevicePngDecoder: %d of %d frames took the Pillow fallback", len(fallback), F)
        self.frames += F
        self.fallback_frames += len(fallback)
        return out.view(shape + (Hc, Wc, 3)), sizes.reshape(shape + (2,))

    @staticmethod
    def _fallback(i, data, why):
        try:
            return pillow_decode(data)
        except ImportError:
            if isinstance(why, UnsupportedPng):
                raise UnsupportedPng("frame %d: %s (and Pillow, the fallback, cannot be imported)" % (i, why)) from why
            raise UnsupportedPng("frame %d: %s (and Pillow, the fallback, cannot be imported)" % (i, why))
        except (OSError, SyntaxError, ValueError) as e:     # what the reference's own read would raise for this file
            raise UnsupportedPng("frame %d: %s, and Pillow cannot decode it either: %s" % (i, why, e)) from e


class DeviceImageDecoder:
    """``DeviceImageDecoder(device).decode(list_of_bytes, shape=None)``: a batch of JPEG and PNG files in any mix. Each frame's first
    bytes decide: JPEG frames go to a ``DeviceJpegDecoder``, PNG frames (and whatever is neither: the PNG decoder's fallback names it)
    to a ``DevicePngDecoder``; both results are merged into ONE container, with sizes, in the caller's order. ``frames`` and
    ``fallback_frames`` are the sums of the two decoders' counters. It is what a caller passes as ``decode_batches(..., decoder=...)``."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.jpeg = DeviceJpegDecoder(device)
        self.png = DevicePngDecoder(device)

    @property
    def frames(self):
        return self.jpeg.frames + self.png.frames

    @property
    def fallback_frames(self):
        return self.jpeg.fallback_frames + self.png.fallback_frames

    def decode(self, encoded, shape=None):
        encoded = list(encoded)
        F = len(encoded)
        shape = (F,) if shape is None else tuple(int(v) for v in shape)
        if int(np.prod(shape, dtype=np.int64)) != F:
            raise ValueError("DeviceImageDecoder.decode: %d frames do not fill shape %s" % (F, shape))
        is_jpeg = [bytes(data[:2]) == b"\xff\xd8" for data in encoded]
        parts = []
        for dec, want in ((self.jpeg, True), (self.png, False)):
            idx = [i for i in range(F) if is_jpeg[i] == want]
            if idx:
                imgs, sizes = dec.decode([encoded[i] for i in idx])
                parts.append((idx, imgs, sizes))
        Hc = max([p[1].shape[1] for p in parts], default=0)
        Wc = max([p[1].shape[2] for p in parts], default=0)
        sizes = np.zeros((F, 2), dtype=np.int64)
        if len(parts) == 1 and parts[0][0] == list(range(F)):
            out, sizes = parts[0][1], parts[0][2]
        else:
            out = torch.zeros((F, Hc, Wc, 3), dtype=torch.uint8, device=self.device)
            for idx, imgs, sz in parts:
                out[torch.as_tensor(idx, device=self.device), :imgs.shape[1], :imgs.shape[2]] = imgs
                sizes[idx] = sz
        return out.view(shape + (Hc, Wc, 3)), sizes.reshape(shape + (2,))
