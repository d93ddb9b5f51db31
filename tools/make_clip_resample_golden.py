#!/usr/bin/env python
"""Writes tests/golden/clip_resample.npz: small uint8 frames, per-frame geometries and what PILLOW makes of them -- the window cropped
(or the frame edge-padded with np.pad and then cropped), resized with Image.BILINEAR, flipped with Image.transpose. Nothing of this
package takes part: the file pins hip_ops.clip_resample_reference and agrl_clip_resample_u8 on Pillow's own bytes
(tests/test_clip_resample.py, tests/test_gpu_clip_resample.py), also where Pillow is not installed.

    python tools/make_clip_resample_golden.py [output.npz]

Keys: ``names`` (the cases), ``pillow_version``, and per case NAME: ``NAME.frames`` uint8 (1,Hs,Ws,3), ``NAME.geometry`` int32 (1,8) =
src_h, src_w, y0, x0, win_h, win_w, flip, 0, ``NAME.out_hw`` int32 (2,), ``NAME.expected`` uint8 (1,OH,OW,3).
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pillow_side(frame, geometry, out_hw):
    """frame uint8 (Hs,Ws,3), geometry (8,) -> uint8 (OH,OW,3): crop / edge-pad, resize, transpose -- Pillow only."""
    sh, sw, y0, x0, wh, ww, flip = (int(v) for v in geometry[:7])
    valid = frame[:sh, :sw]
    top, left = max(0, -y0), max(0, -x0)
    bottom, right = max(0, y0 + wh - sh), max(0, x0 + ww - sw)
    if top or left or bottom or right:
        valid = np.pad(valid, ((top, bottom), (left, right), (0, 0)), mode="edge")
    img = Image.fromarray(np.ascontiguousarray(valid))
    box = (x0 + left, y0 + top, x0 + left + ww, y0 + top + wh)
    if box != (0, 0) + img.size:
        img = img.crop(box)
    img = img.resize((int(out_hw[1]), int(out_hw[0])), Image.BILINEAR)
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(img)


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def ramp(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(7 * y + 3 * x) % 256, (255 - 5 * x - y) % 256, (11 * x * y) % 256], -1).astype(np.uint8)


def checker(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((x + y) % 2) * 255).astype(np.uint8)[..., None], 3, -1)


def whole(h, w, flip=0):
    return (h, w, 0, 0, h, w, flip, 0)


def cases():
    """(name, frame, geometry, (OH, OW))"""
    out = (32, 16)
    return [
        ("identity_32x16", noise(32, 16, 1), whole(32, 16), out),
        ("window_30x15_at_1_1", noise(32, 16, 2), (32, 16, 1, 1, 30, 15, 0, 0), out),      # crop().resize(), not resize(box=)
        ("upscale_16x8", noise(16, 8, 3), whole(16, 8), out),
        ("odd_19x11", noise(19, 11, 4), whole(19, 11), out),
        ("down_37x23", noise(37, 23, 5), whole(37, 23), out),
        ("down_70x50", noise(70, 50, 6), whole(70, 50), out),
        ("one_pixel", noise(1, 1, 7), whole(1, 1), out),
        ("horizontal_only_32x20", noise(32, 20, 8), whole(32, 20), out),
        ("vertical_only_40x16", noise(40, 16, 9), whole(40, 16), out),
        ("flip_37x23", noise(37, 23, 5), whole(37, 23, 1), out),
        ("misalign_pad_top", ramp(32, 16), (32, 16, -1, 0, 33, 16, 0, 0), out),
        ("misalign_pad_bottom", ramp(32, 16), (32, 16, 0, 0, 33, 16, 0, 0), out),
        ("checker_37x23", checker(37, 23), whole(37, 23), out),
    ]


def main(path):
    data = {"names": np.array([c[0] for c in cases()]), "pillow_version": np.array(PIL.__version__)}
    for name, frame, geometry, out_hw in cases():
        g = np.array(geometry, dtype=np.int32)
        data[name + ".frames"] = frame[None]
        data[name + ".geometry"] = g[None]
        data[name + ".out_hw"] = np.array(out_hw, dtype=np.int32)
        data[name + ".expected"] = pillow_side(frame, g, out_hw)[None]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **data)
    print("%s: %d cases, Pillow %s, %d bytes" % (path, len(cases()), PIL.__version__, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "clip_resample.npz"))
