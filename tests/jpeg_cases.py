"""The JPEG fixture (tests/golden/jpeg_decode.npz, written by tools/make_jpeg_golden.py: Pillow's encodings and Pillow's decoded pixels)
and the broken scans shared by tests/test_jpeg_decode.py and tests/test_gpu_jpeg_decode.py. A plain module (like lp16.py): the tests
import it."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_decode.npz")
SAMPLINGS = ("444", "422", "420", "gray")
SHAPES = ((8, 8), (16, 16), (17, 9), (33, 47), (256, 128))


@functools.lru_cache(maxsize=1)
def fixture():
    """-> {name: (jpeg bytes, pixels uint8 (H,W,3) read-only)} in the file's order"""
    out = {}
    with np.load(GOLDEN) as z:
        for name in z["names"]:
            px = z[str(name) + ".pixels"]
            px.setflags(write=False)
            out[str(name)] = (z[str(name) + ".jpeg"].tobytes(), px)
    return out


def names(shape=None, sampling=None):
    return [n for n in fixture() if (shape is None or n.startswith("%dx%d_" % shape)) and (sampling is None or "_%s_" % sampling in n)]


def broken(frame, kind):
    """A parsed frame with a broken scan: 'cut' at half its length, or 'noise': a fixed-seed byte pattern over its middle third."""
    b = bytearray(bytes(frame.scan))
    n = len(b)
    if kind == "cut":
        b = b[:n // 2]
    elif kind == "noise":
        b[n // 3:2 * n // 3] = np.random.default_rng(20).integers(0, 256, 2 * n // 3 - n // 3, dtype=np.uint8).tobytes()
    else:
        raise KeyError(kind)
    return frame._replace(scan=memoryview(bytes(b)))


def broken_file(data, frame, kind):
    """the same damage applied to the file's bytes (``frame`` = parse_jpeg(data)): for the decoder, which parses for itself"""
    scan = bytes(frame.scan)
    at = data.index(scan)
    bad = bytes(broken(frame, kind).scan)
    return data[:at] + bad + (data[at + len(scan):] if kind == "noise" else b"")


def container(pixels):
    """pixel arrays of any sizes -> (uint8 (F,Hmax,Wmax,3) zero-padded, sizes int64 (F,2))"""
    sizes = np.array([p.shape[:2] for p in pixels], dtype=np.int64)
    out = np.zeros((len(pixels), int(sizes[:, 0].max()), int(sizes[:, 1].max()), 3), dtype=np.uint8)
    for f, p in enumerate(pixels):
        out[f, :p.shape[0], :p.shape[1]] = p
    return out, sizes
