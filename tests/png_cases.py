"""The PNG fixture (tests/golden/png_decode.npz, written by tools/make_png_golden.py: PNG files, most of them written by hand, and
Pillow's decoded pixels) shared by tests/test_png_decode.py and tests/test_gpu_png_decode.py. A plain module (like jpeg_cases.py): the
tests import it. The restatement runs ONCE per process over the whole fixture (``reference()``); the tests share its result."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_decode.npz")
SHAPES = ((1, 1), (1, 7), (7, 1), (7, 9), (64, 128))
MODES = ("grey", "rgb")
LARGE = "256x128_rgb_period85_fixed"


@functools.lru_cache(maxsize=1)
def _load():
    good, broken, unsupported = {}, {}, {}
    with np.load(GOLDEN) as z:
        for name in z["names"]:
            px = z[str(name) + ".pixels"]
            px.setflags(write=False)
            good[str(name)] = (z[str(name) + ".png"].tobytes(), px)
        for name in z["broken_names"]:
            broken[str(name)] = (z[str(name) + ".png"].tobytes(), int(z[str(name) + ".status"]))
        for name in z["unsupported_names"]:
            key = str(name) + ".pixels"
            unsupported[str(name)] = (z[str(name) + ".png"].tobytes(), z[key] if key in z.files else None)
        counters = json.loads(str(z["counters"]))
    return good, broken, unsupported, counters


def fixture():
    """-> {name: (png bytes, pixels uint8 (H,W,3) read-only)}: the decodable cases, in the file's order"""
    return _load()[0]


def broken():
    """-> {name: (png bytes, the restatement's status when the file was written)}: sound chunks around a zlib stream that is not"""
    return _load()[1]


def unsupported():
    """-> {name: (bytes, Pillow's pixels or None)}: what parse_png refuses"""
    return _load()[2]


def counters():
    """-> {name: what the restatement saw the case's stream exercise when the file was written}"""
    return _load()[3]


def names(shape=None, mode=None):
    return [n for n in fixture() if (shape is None or n.startswith("%dx%d_" % shape)) and (mode is None or "_%s_" % mode in n)]


def container(pixels):
    """pixel arrays of any sizes -> (uint8 (F,Hmax,Wmax,3) zero-padded, sizes int64 (F,2))"""
    sizes = np.array([p.shape[:2] for p in pixels], dtype=np.int64)
    out = np.zeros((len(pixels), int(sizes[:, 0].max()), int(sizes[:, 1].max()), 3), dtype=np.uint8)
    for f, p in enumerate(pixels):
        out[f, :p.shape[0], :p.shape[1]] = p
    return out, sizes


@functools.lru_cache(maxsize=1)
def reference():
    """the restatement over EVERY decodable case in one batch, once -> (names, plan, clip uint8 tensor, status tensor, info dicts)"""
    from torchreid import device_decode as dd, hip_ops as ops
    order = list(fixture())
    plan = dd.png_batch_plan([dd.parse_png(fixture()[n][0]) for n in order])
    info = []
    clip, status = ops.png_decode_reference(plan, info=info)
    return order, plan, clip, status, info


# the broken frame between good ones; the good frames' pixels are Pillow's
NEIGHBOURS = ("7x9_rgb_smooth_f4", "1x7_grey_smooth_f3", "64x128_grey_smooth_paeth_w9")


@functools.lru_cache(maxsize=None)
def broken_batch(name):
    """-> (plan of [good, BROKEN, good, good], the restatement's clip and status for it, Pillow's container of the good frames)"""
    from torchreid import device_decode as dd, hip_ops as ops
    files = [fixture()[NEIGHBOURS[0]][0], broken()[name][0], fixture()[NEIGHBOURS[1]][0], fixture()[NEIGHBOURS[2]][0]]
    frames = [dd.parse_png(f) for f in files]
    plan = dd.png_batch_plan(frames)
    clip, status = ops.png_decode_reference(plan)
    pixels = [fixture()[NEIGHBOURS[0]][1], np.zeros((frames[1].height, frames[1].width, 3), dtype=np.uint8), fixture()[NEIGHBOURS[1]][1],
              fixture()[NEIGHBOURS[2]][1]]
    want, _ = container(pixels)
    return plan, clip, status, want
