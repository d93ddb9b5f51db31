"""The Pillow half of the reference's input pipeline on the device: the host samples GEOMETRY, the GPU makes the pixels.

The reference resizes, crops, pads and flips every frame with Pillow on the host (transform_test / transform_train,
train_vidreid_xent_htri.py:192-217; the Group operations of its transforms.py draw once per clip and apply the draw to every frame).
Here a clip stays the uint8 the decoder produced: ``eval_geometry`` / ``train_geometry`` turn the frames' sizes (and the random draws)
into one window + flip bit per frame, and ``hip_ops.clip_resample`` (agrl_clip_resample_u8) resamples all frames of the batch in one
launch, byte for byte what ``Image.crop(window).resize((width, height), BILINEAR)`` and the flip give. The result is an ordinary uint8
channel-last clip: the models normalise it inside their stem kernels (ToTensor + Normalize), the native train step through
agrl_frames_normalize_u8.

    reference operation                       geometry
    ---------------------------------------   --------------------------------------------------------------------------
    GroupResize((height, width))              the window is the whole frame
    GroupMisAlignAugment(p, ratio)            th = int(h * ratio) rows cut from / replicated at the top or bottom edge: the
                                              window starts th rows lower, ends th rows higher, or reaches th rows outside
                                              the frame (the kernel replicates the edge row, as F.pad(padding_mode='edge'))
    GroupRandomCrop(crop_size)                a crop_size window at one random offset inside the (misaligned) frame
    GroupRandomHorizontalFlip(p)              the flip bit

Random erasing (GroupRandomErasing, --rand-erase) is the one operation of transform_train that is not a geometry of the uint8 clip: the
reference applies it after Normalize and writes the raw channel mean into the normalised tensor -- a value no uint8 pixel maps to. It
rides in the pass that makes the fp32 tensor instead: ``erase_geometry`` draws the reference's rectangles per frame on the host (all
fitting ones of its 100 attempts: its loop never returns), and ``hip_ops.frames_normalize_erase`` (agrl_frames_normalize_erase_u8)
normalises the resampled clip and erases in one launch. ``DeviceClipTransform(..., train=True, rand_erase=True)`` therefore returns the
normalised fp32 clip the train step takes, not a uint8 one. The host still produces geometry only, never pixels.

OUT OF SCOPE: one rectangle shared by the frames of a clip (the reference draws per frame), the reference's unused
GroupRandom2DTranslation, ElasticTransform and RandomPoseAugmentation. (JPEG decode, the stage in front of this one, is
torchreid/device_decode.py.)
"""
from __future__ import annotations

import math
import random

import numpy as np
import torch

from torchreid import hip_ops as ops

MISALIGN_KINDS = (("up", "crop"), ("up", "pad"), ("bottom", "crop"), ("bottom", "pad"))


def _sizes(sizes):
    s = np.asarray(sizes)
    if s.dtype.kind not in "iu" or s.ndim < 1 or s.shape[-1] != 2:
        raise ValueError("sizes is an integer (..., 2) array of (height, width), got %s %s" % (s.dtype, s.shape))
    if s.size and s.min() < 1:
        raise ValueError("frame sizes are >= 1")
    return s.astype(np.int64)


def eval_geometry(sizes):
    """transform_test: every frame whole. ``sizes`` int (..., 2) = (height, width) of each frame -> int32 (..., 8) geometry rows
    (src_h, src_w, y0, x0, win_h, win_w, flip, 0) of ``hip_ops.clip_resample``."""
    s = _sizes(sizes)
    g = np.zeros(s.shape[:-1] + (8,), dtype=np.int32)
    g[..., 0] = g[..., 4] = s[..., 0]
    g[..., 1] = g[..., 5] = s[..., 1]
    return g


def _clip_geometry(s, rng, misalign, rand_crop, flip, crop_size, misalign_ratio, p):
    """One clip: s int64 (S, 2). The draws are made once and shared by its frames, like the reference's Group operations."""
    S = s.shape[0]
    h, w = s[:, 0], s[:, 1]
    y0, x0 = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    win_h, win_w = h.copy(), w.copy()
    if misalign and not rng.random() > p:
        position, operation = MISALIGN_KINDS[int(rng.integers(4))]
        th = (h * misalign_ratio).astype(np.int64)      # per frame, from its own height
        if operation == "crop":
            win_h = h - th
            if position == "up":
                y0 = th.copy()
        else:
            win_h = h + th
            if position == "up":
                y0 = -th
    if rand_crop:
        ch, cw = int(crop_size[0]), int(crop_size[1])
        if (win_h < ch).any() or (win_w < cw).any():
            f = int(np.argmax((win_h < ch) | (win_w < cw)))
            raise ValueError("frame %d of the clip is %d x %d (after the misalign step): too small for a %d x %d crop" % (
                f, int(win_h[f]), int(win_w[f]), ch, cw))
        # one offset for the clip, inside every frame of it (the reference draws it from the first frame; its frames share a size)
        i = int(rng.integers(0, int(win_h.min()) - ch + 1))
        j = int(rng.integers(0, int(win_w.min()) - cw + 1))
        y0, x0 = y0 + i, x0 + j
        win_h, win_w = np.full(S, ch, dtype=np.int64), np.full(S, cw, dtype=np.int64)
    flipped = bool(flip and rng.random() < p)
    g = np.zeros((S, 8), dtype=np.int32)
    for c, v in enumerate((h, w, y0, x0, win_h, win_w)):
        g[:, c] = v
    g[:, 6] = int(flipped)
    return g


def train_geometry(sizes, rng, misalign=False, rand_crop=False, flip=False, crop_size=(240, 120), misalign_ratio=0.05, p=0.5):
    """transform_train as geometry. ``sizes`` int (S, 2) or (B, S, 2) = (height, width) of each frame; ``rng`` a numpy Generator (or a
    seed). Sampled ONCE PER CLIP: all S frames share the misalign kind, the crop offset and the flip bit. The misalign step (with
    probability p one of up / bottom x crop / pad, th = int(height * misalign_ratio) rows) and the random crop are composed into one
    window per frame. -> int32 (S, 8) / (B, S, 8). ValueError when a frame is too small for the crop."""
    if not isinstance(rng, np.random.Generator):
        rng = np.random.default_rng(rng)
    s = _sizes(sizes)
    if s.ndim == 2:
        return _clip_geometry(s, rng, misalign, rand_crop, flip, crop_size, misalign_ratio, p)
    if s.ndim != 3:
        raise ValueError("sizes is (S, 2) or (B, S, 2), got %s" % (s.shape,))
    return np.stack([_clip_geometry(c, rng, misalign, rand_crop, flip, crop_size, misalign_ratio, p) for c in s]) if len(s) else \
        np.zeros((0, s.shape[1], 8), dtype=np.int32)


ERASE_ATTEMPTS = 100   # the reference's loop (transforms.py:298, 511)


def _erase_frame(height, width, uniform, randint, probability, sl, sh, r1, first):
    """One frame's rectangles [(y, x, h, w), ...], draw for draw GroupRandomErasing._instance_process (``first``: RandomErasing.__call__,
    which returns at the first attempt that fits). ``uniform(a, b)`` / ``randint(a, b)`` (both ends included) are the random module's."""
    rects = []
    if uniform(0, 1) > probability:
        return rects
    for _ in range(ERASE_ATTEMPTS):
        target_area = uniform(sl, sh) * (height * width)
        aspect = uniform(r1, 1 / r1)
        h = int(round(math.sqrt(target_area * aspect)))   # Python's round: half to even
        w = int(round(math.sqrt(target_area / aspect)))
        if w < width and h < height:
            y = randint(0, height - h)
            x = randint(0, width - w)
            rects.append((y, x, h, w))   # h or w may be 0 (a frame one pixel high): drawn, erases nothing
            if first:
                break
    return rects


def erase_geometry(shape, height, width, rng, probability=0.5, sl=0.02, sh=0.4, r1=0.3, attempts='all'):
    """Random erasing as geometry: the rectangles the reference erases in ``shape`` (an int or a tuple, e.g. (B, S)) frames of
    height x width, drawn PER FRAME in C order -> (rects int32 (*shape, R, 4) of rows (y, x, h, w), zero behind each frame's rows;
    counts int32 (*shape)), R = the largest count (at least 1). Per frame: u = uniform(0, 1), nothing when u > probability; else 100
    attempts of area = uniform(sl, sh) H W, aspect = uniform(r1, 1 / r1), h = int(round(sqrt(area aspect))), w = int(round(sqrt(area /
    aspect))) and, where h < H and w < W, y = randint(0, H - h), x = randint(0, W - w). ``attempts='all'`` keeps every attempt that fits,
    as GroupRandomErasing does (transforms.py:293-321: its loop never returns; up to 100 rectangles, a 256x128 frame ends ~96 % covered);
    ``'first'`` stops at the first, as RandomErasing (transforms.py:506-531). ``rng``: a ``random.Random`` -- draw for draw the
    reference's stream: seeded like the random module it yields the reference's rectangles -- or a numpy Generator / a seed (the same
    rule on rng.uniform / rng.integers, as ``train_geometry`` samples)."""
    if attempts not in ('all', 'first'):
        raise ValueError("erase_geometry: attempts is 'all' (GroupRandomErasing) or 'first' (RandomErasing), got %r" % (attempts,))
    shape = (int(shape),) if np.ndim(shape) == 0 else tuple(int(v) for v in shape)
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError("erase_geometry: frames of %d x %d" % (height, width))
    if isinstance(rng, random.Random):
        uniform, randint = rng.uniform, rng.randint
    else:
        if not isinstance(rng, np.random.Generator):
            rng = np.random.default_rng(rng)
        uniform, randint = (lambda a, b: float(rng.uniform(a, b))), (lambda a, b: int(rng.integers(a, b + 1)))
    frames = [_erase_frame(height, width, uniform, randint, probability, sl, sh, r1, attempts == 'first')
              for _ in range(int(np.prod(shape, dtype=np.int64)))]
    counts = np.array([len(f) for f in frames], dtype=np.int32).reshape(shape)
    rects = np.zeros((len(frames), max([len(f) for f in frames] + [1]), 4), dtype=np.int32)
    for n, f in enumerate(frames):
        if f:
            rects[n, :len(f)] = f
    return rects.reshape(shape + rects.shape[1:]), counts


GEOMETRY_FLAGS = ("misalign", "rand_crop", "flip", "crop_size", "misalign_ratio", "p")
ERASE_FLAGS = ("probability", "sl", "sh", "r1", "attempts", "value")


class DeviceClipTransform:
    """``DeviceClipTransform(height, width, train=False, **flags)(clips, sizes=None)``: uint8 (B,S,Hs,Ws,3) clips on the GPU -> uint8
    (B,S,height,width,3), ready for ``model(x, adj)`` or the train step. ``sizes``: int (B,S,2) valid extents (height, width) of the
    frames inside the padded container, default the container's size. ``train=False`` is transform_test (resize); ``train=True`` takes
    the flags of ``train_geometry`` (misalign, rand_crop, flip, crop_size, misalign_ratio, p) and ``rng`` (a numpy Generator or a seed).
    The geometry of the last call is kept in ``last_geometry`` (host int32 (B,S,8)).

    ``rand_erase=True`` (train only) adds the reference's random erasing, which works on the normalised tensor: the call then returns
    the NORMALISED fp32 (B,S,3,height,width) clip the train step takes -- the resample, then ``hip_ops.frames_normalize_erase``: two
    launches. ``erase``: a dict of ``erase_geometry``'s keyword arguments (probability, sl, sh, r1, attempts) plus ``value`` (what is
    written, default hip_ops.PIXEL_MEAN as the driver's GroupRandomErasing()); ``pixel_mean`` / ``pixel_std``: the normalisation. The
    rectangles are drawn from ``rng`` after the clip geometry and kept in ``last_erase`` (host (rects (B,S,R,4), counts (B,S)))."""

    def __init__(self, height, width, train=False, rng=None, **flags):
        self.height, self.width, self.train = int(height), int(width), bool(train)
        unknown = set(flags) - set(GEOMETRY_FLAGS) - {"rand_erase", "erase", "pixel_mean", "pixel_std"}
        if unknown or (flags and not train):
            raise TypeError("DeviceClipTransform: unexpected arguments %s" % sorted(unknown or flags))
        self.flags = {k: v for k, v in flags.items() if k in GEOMETRY_FLAGS}
        self.rand_erase = bool(flags.get("rand_erase", False))
        erase = flags.get("erase")
        if not self.rand_erase and set(flags) & {"erase", "pixel_mean", "pixel_std"}:
            raise TypeError("DeviceClipTransform: erase, pixel_mean and pixel_std go with rand_erase=True")
        if erase is not None and (not isinstance(erase, dict) or set(erase) - set(ERASE_FLAGS)):
            raise TypeError("DeviceClipTransform: erase is a dict with keys from %s, got %r" % (ERASE_FLAGS, erase))
        self.erase = {k: v for k, v in (erase or {}).items() if k != "value"}
        self.pixel_mean, self.pixel_std = flags.get("pixel_mean", ops.PIXEL_MEAN), flags.get("pixel_std", ops.PIXEL_STD)
        self.erase_value = (erase or {}).get("value", ops.PIXEL_MEAN)
        self.rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        self.last_geometry = None
        self.last_erase = None

    def geometry(self, sizes):
        return train_geometry(sizes, self.rng, **self.flags) if self.train else eval_geometry(sizes)

    def __call__(self, clips, sizes=None):
        if not isinstance(clips, torch.Tensor) or clips.dtype != torch.uint8 or clips.dim() != 5 or clips.shape[-1] != 3:
            raise ValueError("DeviceClipTransform takes uint8 (B,S,Hs,Ws,3) clips, got %s" % (
                "%s %s" % (clips.dtype, tuple(clips.shape)) if isinstance(clips, torch.Tensor) else type(clips),))
        B, S, Hs, Ws = clips.shape[:4]
        if sizes is None:
            sizes = np.broadcast_to(np.array([Hs, Ws], dtype=np.int64), (B, S, 2))
        sizes = np.asarray(sizes.cpu() if isinstance(sizes, torch.Tensor) else sizes)
        if sizes.shape != (B, S, 2):
            raise ValueError("sizes is (B,S,2) = %s, got %s" % ((B, S, 2), sizes.shape))
        self.last_geometry = self.geometry(sizes)
        out = ops.clip_resample(clips.contiguous().view(B * S, Hs, Ws, 3), self.last_geometry.reshape(B * S, 8), (self.height, self.width))
        if not self.rand_erase:
            return out.view(B, S, self.height, self.width, 3)
        rects, counts = self.last_erase = erase_geometry((B, S), self.height, self.width, self.rng, **self.erase)
        out = ops.frames_normalize_erase(out, rects.reshape((B * S,) + rects.shape[2:]), counts.reshape(B * S), self.erase_value,
                                         self.pixel_mean, self.pixel_std)
        return out.view(B, S, 3, self.height, self.width)
