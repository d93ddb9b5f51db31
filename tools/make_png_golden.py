#!/usr/bin/env python
"""Writes tests/golden/png_decode.npz: PNG byte strings and the pixels PILLOW decodes from them (``Image.open(...).convert('RGB')``, the
reference's read, dataset_loader.py:23-36). It pins hip_ops.png_decode_reference and agrl_png_decode_u8 on Pillow's own bytes
(tests/test_png_decode.py, tests/test_gpu_png_decode.py), also where this Pillow is not installed.

    python tools/make_png_golden.py [output.npz]

Pillow's encoder picks filters and block types itself, so most files are written BY HAND here: the rows filtered in numpy with a chosen
filter per row, compressed with ``zlib.compressobj`` (Z_FIXED, level 0, Z_SYNC_FLUSH / Z_FULL_FLUSH in mid-stream, wbits=9) or, where
zlib cannot be made to emit what is wanted (a match 32 725 bytes back, 15-bit codes behind both table roots, a distance set of one
code or of none, the broken streams), by the few lines of fixed- and dynamic-Huffman encoder below; then wrapped in chunks, IDAT split
where wanted. The expected pixels are always Pillow's decode of the finished file.

Keys: ``names`` (the decodable cases, HxW_mode_how), ``pillow_version``, per case ``NAME.png`` uint8 (bytes,), ``NAME.pixels`` uint8
(H,W,3); ``counters`` (JSON: per case what the restatement, hip_ops.png_decode_reference, saw the stream exercise -- block types, match
lengths and distances, filters, codes split by an IDAT boundary, the declared window); ``broken_names`` with ``NAME.png`` and
``NAME.status`` (the restatement's status: the chunks of these files are sound, their zlib streams are not); ``unsupported_names`` with
``NAME.png`` and, where Pillow decodes the file, ``NAME.pixels``: the files parse_png refuses."""
import io
import json
import os
import struct
import sys
import zlib

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "agrl.pytorch_amd")]

SIGNATURE = b"\x89PNG\r\n\x1a\n"
SHAPES = ((1, 1), (1, 7), (7, 1), (7, 9), (64, 128))
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def content(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "solid":
        return np.full((h, w, 3), 77, dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.uniform(0, 6.28, 6)
    ch = [127.5 + 100 * np.sin(x / (7.0 + 3 * c) + ph[c]) * np.cos(y / (11.0 + 2 * c) + ph[c + 3]) for c in range(3)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def samples(pixels, mode):
    """(H,W,3) -> the frame's samples (H, W * channels)"""
    return pixels[..., 1].copy() if mode == "grey" else pixels.reshape(pixels.shape[0], -1).copy()


def filter_rows(rows, bpp, filters):
    """samples uint8 (H, rowbytes) -> the bytes a PNG stream inflates to: per row the filter byte ``filters[y]`` and the filtered row"""
    H, rb = rows.shape
    out = np.zeros((H, 1 + rb), dtype=np.uint8)
    prev = np.zeros(rb, dtype=np.int64)
    for y in range(H):
        cur = rows[y].astype(np.int64)
        left = np.concatenate([np.zeros(bpp, dtype=np.int64), cur[:-bpp]]) if rb > bpp else np.zeros(rb, dtype=np.int64)
        upleft = np.concatenate([np.zeros(bpp, dtype=np.int64), prev[:-bpp]]) if rb > bpp else np.zeros(rb, dtype=np.int64)
        ft = int(filters[y])
        if ft == 0:
            pred = 0
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (left + prev) >> 1
        elif ft == 4:
            p = left + prev - upleft
            pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, upleft))
        else:                      # not a filter: the byte goes in, the row as it is
            pred = 0
        out[y, 0] = ft
        out[y, 1:] = (cur - pred) & 255
        prev = cur
    return out.tobytes()


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def wrap(H, W, stream, colour, depth=8, interlace=0, split=None, extra=b""):
    """a zlib stream -> a PNG file; ``split``: bytes per IDAT chunk (default: one chunk); ``extra``: chunks between IHDR and IDAT"""
    parts = [stream] if not split else [stream[i:i + split] for i in range(0, len(stream), split)]
    return (SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, colour, 0, 0, interlace)) + extra +
            b"".join(chunk(b"IDAT", p) for p in parts) + chunk(b"IEND", b""))


def deflate(raw, level=9, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flushes=()):
    """zlib.compressobj over ``raw``; ``flushes``: (fraction of the input, flush mode) in order"""
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    out, at = b"", 0
    for frac, mode in flushes:
        to = int(len(raw) * frac)
        out += co.compress(raw[at:to]) + co.flush(mode)
        at = to
    return out + co.compress(raw[at:]) + co.flush()


class BitWriter:
    """deflate's bit order: fields LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.acc = self.n = 0
        self.out = bytearray()

    def put(self, value, bits):
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, bits):
        self.put(int(format(code, "0%db" % bits)[::-1], 2), bits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def fixed_symbol(self, sym):
        if sym < 144:
            self.code(0x30 + sym, 8)
        elif sym < 256:
            self.code(0x190 + sym - 144, 9)
        elif sym < 280:
            self.code(sym - 256, 7)
        else:
            self.code(0xC0 + sym - 280, 8)

    def fixed_block(self, tokens, final):
        """one fixed-Huffman block: a token is a literal byte or (length, distance)"""
        self.put(int(final), 1)
        self.put(1, 2)
        for t in tokens:
            if isinstance(t, tuple):
                n, dist = t
                i = max(k for k in range(29) if LBASE[k] <= n)
                self.fixed_symbol(257 + i)
                self.put(n - LBASE[i], LEXT[i])
                j = max(k for k in range(30) if DBASE[k] <= dist)
                self.code(j, 5)
                self.put(dist - DBASE[j], DEXT[j])
            else:
                self.fixed_symbol(int(t))
        self.fixed_symbol(256)


def zlib_wrap(body, raw, adler=None):
    return b"\x78\x01" + bytes(body) + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF if adler is None else adler)


def period_stream(raw, period):
    """``raw`` repeats with ``period``: its first period as literals, the rest as matches of up to 258 bytes exactly one period back"""
    w = BitWriter()
    tokens = list(raw[:period])
    at = period
    while at < len(raw):
        n = min(258, len(raw) - at)
        assert n >= 3 and raw[at:at + n] == raw[at - period:at - period + n]
        tokens.append((n, period))
        at += n
    w.fixed_block(tokens, True)
    w.align()
    return zlib_wrap(w.out, raw)


def canonical(lens):
    """code lengths -> {symbol: (code, length)}, RFC 1951 3.2.2"""
    out, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


def dynamic_stream(raw, tokens, litlens, distlens):
    """one final dynamic-Huffman block with the GIVEN code lengths (zlib would never choose them): ``litlens`` {symbol: length}, ``distlens``
    a list. The lengths go out one code-length symbol each, no repeats, under a flat 4-bit code-length code."""
    nlen = max(max(litlens) + 1, 257)
    lens = [litlens.get(s, 0) for s in range(nlen)] + list(distlens)
    lit, dst = canonical(lens[:nlen]), canonical(distlens)
    w = BitWriter()
    w.put(1, 1)
    w.put(2, 2)
    w.put(nlen - 257, 5)
    w.put(len(distlens) - 1, 5)
    w.put(19 - 4, 4)
    for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        w.put(4 if s < 16 else 0, 3)
    for l in lens:
        w.code(l, 4)
    for t in tokens + [256]:
        if isinstance(t, tuple):
            n, dist = t
            i = max(k for k in range(29) if LBASE[k] <= n)
            w.code(*lit[257 + i])
            w.put(n - LBASE[i], LEXT[i])
            j = max(k for k in range(30) if DBASE[k] <= dist)
            w.code(*dst[j])
            w.put(dist - DBASE[j], DEXT[j])
        else:
            w.code(*lit[int(t)])
    w.align()
    return zlib_wrap(w.out, raw)


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return bytes(out)


def dynamic_cases():
    """code sets zlib's deflate never emits and its inflate accepts: 15-bit codes behind both roots (a chain of lengths 1, 2, ..., 15, 15),
    a distance set of ONE code, a distance set of none"""
    out = []
    chain = list(range(1, 16)) + [15]
    rng = np.random.default_rng(77)
    syms = list(range(10)) + [256, 257, 258, 265, 284, 285]
    litlens = dict(zip(syms, rng.permutation(chain).tolist()))
    distlens = rng.permutation(chain).tolist()          # distance symbols 0..15: 1..255 bytes back
    tokens = []
    for y in range(7):                                   # 7 rows of 1 + 27 bytes, every row's filter byte a literal
        tokens.append(int(y % 5))
        left = 27
        while left:
            done = len(expand(tokens))
            n = int(rng.choice([3, 4, 11, 12]))
            if done > 30 and left >= n and rng.random() < 0.6:
                tokens.append((n, int(rng.integers(1, min(done, 255) + 1))))
                left -= n
            else:
                tokens.append(int(rng.integers(0, 10)))
                left -= 1
    raw = expand(tokens)
    assert len(raw) == 7 * 28 and all(raw[28 * y] < 5 for y in range(7))
    out.append(("7x9_rgb_dynamic_deep", wrap(7, 9, dynamic_stream(raw, tokens, litlens, distlens), 2)))
    tokens = [0, 1] + [(61, 1)] + [1, 7, 3] + [(60, 1)] + [2] + [(6, 1)]       # 7 rows of 1 + 18 bytes: runs, every filter byte inside one
    raw = expand(tokens)
    assert len(raw) == 7 * 19 and all(raw[19 * y] < 5 for y in range(7))
    lit = {0: 3, 1: 3, 2: 3, 3: 3, 4: 3, 7: 3, 256: 3, 257 + 3: 4, 257 + 19: 5, 257 + 20: 5}   # lengths 6, 59..66 (3 extra), 67..82
    out.append(("7x18_grey_dynamic_one_distance", wrap(7, 18, dynamic_stream(raw, tokens, lit, [1]), 0)))
    tokens = [int(v) for v in rng.integers(0, 4, 7 * 10)]
    lit = {0: 2, 1: 2, 2: 2, 3: 3, 256: 3}
    out.append(("7x9_grey_dynamic_no_distance", wrap(7, 9, dynamic_stream(bytes(tokens), tokens, lit, [0]), 0)))
    return out


def pillow_png(pixels, mode, **kw):
    buf = io.BytesIO()
    Image.fromarray(pixels[..., 1] if mode == "grey" else pixels).save(buf, "PNG", **kw)
    return buf.getvalue()


def decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def cases():
    """(name, png bytes) of the decodable files"""
    out, seed = [], 0
    for h, w in SHAPES:
        for mode in ("grey", "rgb"):
            colour, bpp = (0, 1) if mode == "grey" else (2, 3)
            tag = "%dx%d_%s" % (h, w, mode)
            seed += 1
            px = content("smooth", h, w, seed)
            rows = samples(px, mode)
            out.append((tag + "_smooth_pillow", pillow_png(px, mode)))
            mixed = [(y + h + w) % 5 for y in range(h)]
            out.append((tag + "_smooth_mixed_fixed", wrap(h, w, deflate(filter_rows(rows, bpp, mixed), strategy=zlib.Z_FIXED), colour)))
            if (h, w) in ((1, 7), (7, 9)):
                for ft in range(5):     # every filter on a first row and on the rows below it
                    out.append(("%s_smooth_f%d" % (tag, ft), wrap(h, w, deflate(filter_rows(rows, bpp, [ft] * h)), colour)))
            if (h, w) == (7, 9):
                raw = filter_rows(rows, bpp, mixed)
                out.append((tag + "_smooth_flushes", wrap(h, w, deflate(raw, flushes=((0.3, zlib.Z_SYNC_FLUSH), (0.6, zlib.Z_FULL_FLUSH))), colour)))
                out.append((tag + "_smooth_level0_split", wrap(h, w, deflate(raw, level=0, flushes=((0.5, zlib.Z_SYNC_FLUSH),)), colour, split=5)))
            if (h, w) == (64, 128):
                raw = filter_rows(rows, bpp, mixed)
                out.append((tag + "_smooth_mixed_dynamic_split", wrap(h, w, deflate(raw), colour, split=61)))
                out.append((tag + "_smooth_paeth_w9", wrap(h, w, deflate(filter_rows(rows, bpp, [4] * h), wbits=9), colour)))
                out.append((tag + "_smooth_flushes", wrap(h, w, deflate(raw, level=6, flushes=((0.25, zlib.Z_SYNC_FLUSH), (0.5, zlib.Z_FULL_FLUSH),
                                                                                           (0.5, zlib.Z_SYNC_FLUSH))), colour, split=1000)))
                noise = content("noise", h, w, seed + 100)
                if mode == "grey":       # uniform noise compresses to stored blocks only
                    out.append((tag + "_noise_pillow", pillow_png(noise, mode)))
                else:
                    out.append((tag + "_noise_level0", wrap(h, w, deflate(filter_rows(samples(noise, mode), bpp, mixed), level=0), colour)))
                out.append((tag + "_solid_none", wrap(h, w, deflate(filter_rows(samples(content("solid", h, w, 0), mode), bpp, [0] * h)), colour)))
    # 256 x 128 RGB whose rows repeat with a period of 85 rows: matches reach back 85 * 385 = 32 725 bytes, further than zlib's own
    # deflate looks (32 506), so the stream is written by the encoder above
    h, w = 256, 128
    base = content("noise", 85, w, 999)
    px = np.concatenate([base, base, base, base])[:h]
    raw = filter_rows(samples(px, "rgb"), 3, [0] * h)
    out.append(("256x128_rgb_period85_fixed", wrap(h, w, period_stream(raw, 85 * 385), 2, split=8192)))
    return out + dynamic_cases()


def rewrap(png, mutate):
    """the file with its zlib stream replaced by mutate(stream): the chunks (and their CRCs) stay sound"""
    from torchreid import device_decode as dd
    fr = dd.parse_png(png)
    return wrap(fr.height, fr.width, mutate(fr.stream), 0 if fr.channels == 1 else 2)


def broken(good):
    """(name, png bytes): files whose chunks are sound and whose zlib streams are not"""
    base = good["64x128_rgb_smooth_mixed_dynamic_split"]
    small = good["7x9_rgb_smooth_mixed_fixed"]
    out = [("cut", rewrap(base, lambda s: s[:len(s) // 2]))]

    def noise(s):
        b = bytearray(s)
        n = len(b)
        b[n // 3:2 * n // 3] = np.random.default_rng(20).integers(0, 256, 2 * n // 3 - n // 3, dtype=np.uint8).tobytes()
        return bytes(b)
    out.append(("noise", rewrap(base, noise)))
    raw = bytes(range(7 * 28))                   # 7 rows of 1 + 9 * 3 bytes, whatever they hold
    w = BitWriter()
    w.fixed_block([1, 2, 3, (5, 10)] + list(raw[8:]), True)
    w.align()
    out.append(("distance_before_start", wrap(7, 9, zlib_wrap(w.out, raw), 2)))
    w = BitWriter()
    w.put(1, 1)
    w.put(3, 2)
    w.align()
    out.append(("block_type_3", wrap(7, 9, zlib_wrap(w.out + bytes(16), raw), 2)))
    w = BitWriter()
    w.put(1, 1)
    w.put(0, 2)
    w.align()
    w.put(len(raw), 16)
    w.put((len(raw) ^ 0xFFFF) ^ 0x0100, 16)
    out.append(("len_nlen_mismatch", wrap(7, 9, zlib_wrap(w.out + raw, raw), 2)))
    w = BitWriter()
    w.put(1, 1)
    w.put(2, 2)
    w.put(0, 5)
    w.put(0, 5)
    w.put(15, 4)
    for _ in range(19):                          # nineteen code-length codes of one bit each
        w.put(1, 3)
    w.align()
    out.append(("oversubscribed_table", wrap(7, 9, zlib_wrap(w.out + bytes(16), raw), 2)))
    out.append(("wrong_adler", rewrap(small, lambda s: s[:-1] + bytes([s[-1] ^ 0x40]))))
    px = content("smooth", 7, 9, 5)
    rows = samples(px, "rgb")
    out.append(("filter_byte_5", wrap(7, 9, deflate(filter_rows(rows, 3, [0, 1, 2, 5, 4, 3, 0])), 2)))
    good_raw = filter_rows(rows, 3, [1] * 7)
    out.append(("inflated_too_short", wrap(7, 9, deflate(good_raw[:-28]), 2)))
    out.append(("inflated_too_long", wrap(7, 9, deflate(good_raw + good_raw[:28]), 2)))
    return out


def unsupported(good):
    """(name, bytes): what parse_png refuses"""
    px = content("smooth", 7, 9, 11)
    out = []

    def pil(name, im, **kw):
        buf = io.BytesIO()
        im.save(buf, "PNG", **kw)
        out.append((name, buf.getvalue()))
    rgb = Image.fromarray(px)
    pil("palette", rgb.convert("P", palette=Image.ADAPTIVE, colors=16))
    pil("grey_alpha", rgb.convert("LA"))
    pil("rgb_alpha", rgb.convert("RGBA"))
    pil("depth_16", Image.fromarray((px[..., 0].astype(np.uint16) * 257)))
    pil("depth_1", rgb.convert("1"))
    pil("trns", rgb, transparency=(1, 2, 3))
    one = zlib.compress(b"\x00\x80")
    out.append(("depth_2", wrap(1, 1, one, 0, depth=2)))
    out.append(("depth_4", wrap(1, 1, one, 0, depth=4)))
    out.append(("adam7", wrap(1, 1, zlib.compress(b"\x00\x10\x20\x30"), 2, interlace=1)))
    small = good["7x9_rgb_smooth_mixed_fixed"]
    ihdr_end = 8 + 25
    out.append(("actl", small[:ihdr_end] + chunk(b"acTL", struct.pack(">II", 1, 0)) + small[ihdr_end:]))
    at = small.index(b"IDAT") + 6
    out.append(("crc_mismatch", small[:at] + bytes([small[at] ^ 1]) + small[at + 1:]))
    out.append(("over_the_size_bound", wrap(300, 200, zlib.compress(bytes(300 * 601), 9), 2)))
    out.append(("not_a_png", b"GIF89a" + bytes(32)))
    return out


def main(path):
    from torchreid import device_decode as dd, hip_ops as ops
    data = {"pillow_version": np.array(PIL.__version__), "zlib_version": np.array(zlib.ZLIB_RUNTIME_VERSION)}
    names, counters = [], {}
    good = dict(cases())
    for name, png in good.items():
        names.append(name)
        data[name + ".png"] = np.frombuffer(png, dtype=np.uint8)
        data[name + ".pixels"] = decode(png)
        info = []
        clip, status = ops.png_decode_reference(dd.png_batch_plan([dd.parse_png(png)]), info=info)
        assert int(status[0]) == 0 and np.array_equal(clip[0].numpy(), data[name + ".pixels"]), (name, int(status[0]))
        c = info[0]
        counters[name] = {k: (sorted(v) if isinstance(v, set) else int(v)) for k, v in c.items() if k != "inflated"}
    data["names"] = np.array(names)
    data["counters"] = np.array(json.dumps(counters, sort_keys=True))
    bnames = []
    for name, png in broken(good):
        bnames.append(name)
        data[name + ".png"] = np.frombuffer(png, dtype=np.uint8)
        _, status = ops.png_decode_reference(dd.png_batch_plan([dd.parse_png(png)]))
        data[name + ".status"] = np.array(int(status[0]), dtype=np.int32)
        print("  broken %-24s status %2d (%s)" % (name, int(status[0]), ops.PNG_STATUS_NAMES[int(status[0])]))
    data["broken_names"] = np.array(bnames)
    unames = []
    for name, png in unsupported(good):
        unames.append(name)
        data[name + ".png"] = np.frombuffer(png, dtype=np.uint8)
        try:
            data[name + ".pixels"] = decode(png)
        except Exception as e:  # noqa: BLE001  (Pillow cannot read it either: parse_png's case only)
            print("  unsupported %-20s Pillow: %s" % (name, e))
    data["unsupported_names"] = np.array(unames)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **data)
    print("%s: %d cases, %d broken, %d unsupported, Pillow %s, zlib %s, %d bytes" % (
        path, len(names), len(bnames), len(unames), PIL.__version__, zlib.ZLIB_RUNTIME_VERSION, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "png_decode.npz"))
