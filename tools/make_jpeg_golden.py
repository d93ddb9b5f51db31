#!/usr/bin/env python
"""Writes tests/golden/jpeg_decode.npz: JPEG byte strings as PILLOW encodes them and the pixels PILLOW decodes from them
(``Image.open(...).convert('RGB')``, the reference's read, dataset_loader.py:23-36). Nothing of this package takes part: the file pins
hip_ops.jpeg_decode_reference and agrl_jpeg_decode_u8 on Pillow's own bytes (tests/test_jpeg_decode.py,
tests/test_gpu_jpeg_decode.py), also where this Pillow is not installed.

    python tools/make_jpeg_golden.py [output.npz]

Keys: ``names`` (the cases), ``pillow_version``, ``libjpeg_turbo`` (whether Pillow's JPEG codec is libjpeg-turbo), and per case NAME:
``NAME.jpeg`` uint8 (bytes,), ``NAME.pixels`` uint8 (H,W,3). Names read HxW_sampling_qQ_content[_opt][_rstN|_rstrow]: many frames of at
most 48x48 in every sampling, quality 30 and 100, noise / smooth / saturated content, per-file Huffman tables (optimize=True), restart
intervals; a handful of 256x128 ones with smooth content, to stay below the largest fixture already committed.
"""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLINGS = {"444": 0, "422": 1, "420": 2, "gray": None}
SHAPES = ((8, 8), (16, 16), (17, 9), (33, 47))


def content(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "smooth":
        ph = rng.uniform(0, 6.28, 6)
        ch = [127.5 + 100 * np.sin(x / (7.0 + 3 * c) + ph[c]) * np.cos(y / (11.0 + 2 * c) + ph[c + 3]) for c in range(3)]
        return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)
    if kind == "saturated":   # pure primaries in 5 x 3 patches: the colour conversion leaves 0..255 in every channel
        pal = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255], [255, 255, 255], [0, 0, 0]], dtype=np.uint8)
        return pal[((y // 5).astype(np.int64) * 3 + (x // 3).astype(np.int64) + seed) % 8]
    raise KeyError(kind)


def encode(pixels, sampling, quality, **kw):
    buf = io.BytesIO()
    if SAMPLINGS[sampling] is None:
        Image.fromarray(pixels[..., 1]).save(buf, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(pixels).save(buf, "JPEG", quality=quality, subsampling=SAMPLINGS[sampling], **kw)
    return buf.getvalue()


def decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def cases():
    """(name, jpeg bytes)"""
    out, seed = [], 0
    for h, w in SHAPES:
        for s in SAMPLINGS:
            for q in (30, 100):
                seed += 1
                out.append(("%dx%d_%s_q%d_noise" % (h, w, s, q), encode(content("noise", h, w, seed), s, q)))
            seed += 1
            out.append(("%dx%d_%s_q85_noise_opt" % (h, w, s), encode(content("noise", h, w, seed), s, 85, optimize=True)))
            out.append(("%dx%d_%s_q75_saturated" % (h, w, s), encode(content("saturated", h, w, seed), s, 75)))
    for s in SAMPLINGS:
        seed += 1
        px = content("noise", 33, 47, seed)
        out.append(("33x47_%s_q75_noise_rst3" % s, encode(px, s, 75, restart_marker_blocks=3)))
        out.append(("33x47_%s_q95_noise_rstrow" % s, encode(px, s, 95, restart_marker_rows=1)))
        out.append(("48x48_%s_q75_smooth_opt_rstrow" % s, encode(content("smooth", 48, 48, seed), s, 75, optimize=True, restart_marker_rows=1)))
    for k, s in enumerate(("420", "422", "444", "gray")):   # four 256x128 frames, one per sampling
        seed += 1
        out.append(("256x128_%s_q%d_smooth" % (s, (75, 95, 85, 30)[k]), encode(content("smooth", 256, 128, seed), s, (75, 95, 85, 30)[k])))
    return out


def main(path):
    data = {"pillow_version": np.array(PIL.__version__), "libjpeg_turbo": np.array(bool(features.check_feature("libjpeg_turbo")))}
    names = []
    for name, jpeg in cases():
        names.append(name)
        data[name + ".jpeg"] = np.frombuffer(jpeg, dtype=np.uint8)
        data[name + ".pixels"] = decode(jpeg)
    data["names"] = np.array(names)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **data)
    print("%s: %d cases, Pillow %s (libjpeg-turbo: %s), %d bytes" % (path, len(names), PIL.__version__, data["libjpeg_turbo"], os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz"))
