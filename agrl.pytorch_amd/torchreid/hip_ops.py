"""Tensor-level wrappers of the C-ABI entry points (include/agrl_hip.h).

Each function checks shapes/dtypes, allocates the output through torch's caching allocator on the
input's device, and launches on the calling thread's current HIP stream. No arithmetic happens here.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np
import torch

from . import _hip
from ._hip import F32, LP16, LP_DTYPE, LP_NAME, METRIC_COSINE, METRIC_EUCLIDEAN, call, dtype_code, ptr


import contextlib
import threading
import weakref

_MODE = threading.local()


@contextlib.contextmanager
def f32_split(on=True):
    """Inside this block fp32 convs / Linears use the split-bf16 recipe (dtype code AGRL_F32X3: every product as three
    bf16 MFMAs on the high / low halves of the operands, ~1e-5 relative, 2-3 x the exact-fp32 rate). Per thread."""
    prev = getattr(_MODE, 'split', False)
    _MODE.split = bool(on)
    try:
        yield
    finally:
        _MODE.split = prev


_SWITCHES = {}


def switch(name, default='1'):
    """A Python-side tuning switch (AGRL_HIP_*), read from the environment ONCE and cached like the library's own options:
    ``_hip.reload_options()`` (what the A/B tools and the tests call after changing the environment) drops the cache. Round-5 review:
    the dispatch predicates used to call os.environ.get 17 times per Bottleneck of every forward."""
    v = _SWITCHES.get(name)
    if v is None:
        v = _SWITCHES[name] = os.environ.get(name, default)
    return v


_hip.RELOAD_HOOKS.append(_SWITCHES.clear)


def _gemm_code(dt):
    if dt == torch.float32 and getattr(_MODE, 'split', False):
        return _hip.F32X3
    return dtype_code(dt)


def _stream(t):
    return _hip.stream_ptr(t.device)


def _dev(t):
    return torch.cuda.device(t.device)


def written(tensors):
    """The rule for every raw writer: a kernel writes through a pointer, which torch's version counters do not see, so a wrapper that
    had a kernel write tensors it did NOT allocate itself -- parameters, optimiser state, running statistics, a caller's ``out=`` --
    calls this on them after the launch. The writes then count as torch's own in-place operations do: whatever is keyed on
    ``_version`` (the pack cache's fingerprint in models/_resnet_hip.py, QueryOperandCache below) misses, and autograd refuses a
    backward whose saved tensors were written underneath it. Host only, one call for any number of tensors."""
    torch.autograd.graph.increment_version(tensors)


PIXEL_MEAN = (0.485, 0.456, 0.406)   # the reference's transform_test: Normalize(mean, std) behind ToTensor
PIXEL_STD = (0.229, 0.224, 0.225)    # (train_vidreid_xent_htri.py:214-217)


def frame_table(mean=PIXEL_MEAN, std=PIXEL_STD):
    """The canonical normalisation of a uint8 pixel value: (3, 256) fp32 on the CPU, T[c][u] = (float32(u) / 255 - mean[c]) / std[c] with
    mean / std rounded to fp32 first and every operation a correctly rounded fp32 operation -- what ``F.to_tensor`` + ``F.normalize``
    compute. (Multiplying by 1/255 instead of dividing is NOT the same: it differs in 322 of the 768 default entries.)"""
    m = torch.tensor([float(v) for v in mean], dtype=torch.float32).view(3, 1)
    s = torch.tensor([float(v) for v in std], dtype=torch.float32).view(3, 1)
    if m.numel() != 3 or s.numel() != 3 or not bool((s != 0).all()):
        raise ValueError("mean and std are three values each, std non-zero: got %r, %r" % (mean, std))
    u = torch.arange(256, dtype=torch.float32).view(1, 256)
    return u.div(255.0).sub(m).div(s)


def frames_layout(shape):
    """'nchw' for (..., 3, H, W) uint8 frames, 'nhwc' for (..., H, W, 3), decided by where the axis of size 3 sits (channel-first wins when
    both fit); ValueError when neither does."""
    if len(shape) >= 3 and shape[-3] == 3:
        return 'nchw'
    if len(shape) >= 3 and shape[-1] == 3:
        return 'nhwc'
    raise ValueError("uint8 frames are (..., 3, H, W) or (..., H, W, 3), got %s" % (tuple(shape),))


def frames_normalize_reference(u8, mean=PIXEL_MEAN, std=PIXEL_STD):
    """uint8 frames (..., 3, H, W) or (..., H, W, 3) -> fp32 (..., 3, H, W) by indexing ``frame_table``: pure torch, any device. What
    the CPU paths of the models use, and what the GPU kernels are compared with bit for bit."""
    assert u8.dtype == torch.uint8
    if frames_layout(u8.shape) == 'nhwc':
        u8 = u8.movedim(-1, -3)
    T = frame_table(mean, std).to(u8.device)
    idx = u8.long()
    return torch.stack([T[c][idx.select(-3, c)] for c in range(3)], dim=-3).contiguous()


_FRAME_TABLES = {}


def _device_frame_table(device, mean, std):
    """The kernels' form of ``frame_table`` on ``device``: (3, 257) fp32, entry 256 of every row = 0 (the stems' zero padding is 0 in the
    normalised domain). Cached per (device, mean, std): built -- one H2D copy -- the first time a triple is seen and never again, so a
    forward issues no host synchronisation and stays capturable as a HIP graph once it has run eagerly."""
    key = (str(device), tuple(float(v) for v in mean), tuple(float(v) for v in std))
    t = _FRAME_TABLES.get(key)
    if t is None:
        host = torch.zeros((3, 257), dtype=torch.float32)
        host[:, :256] = frame_table(mean, std)
        t = _FRAME_TABLES[key] = host.to(device).contiguous()
    return t


def _u8_frames(x, mean, std):
    """(N,3,H,W) / (N,H,W,3) uint8 -> (contiguous x, device table, layout code, N, H, W)."""
    assert x.dtype == torch.uint8 and x.dim() == 4
    layout = frames_layout(x.shape)
    x = x.contiguous()
    N, H, W = (x.shape[0], x.shape[2], x.shape[3]) if layout == 'nchw' else (x.shape[0], x.shape[1], x.shape[2])
    return x, _device_frame_table(x.device, mean, std), (_hip.FRAMES_NCHW if layout == 'nchw' else _hip.FRAMES_NHWC), N, H, W


def frames_normalize(u8, mean=PIXEL_MEAN, std=PIXEL_STD):
    """uint8 frames (N,3,H,W) or (N,H,W,3) on the GPU -> fp32 NCHW (N,3,H,W), ``frame_table`` applied by agrl_frames_normalize_u8: for
    the paths that do not fuse the normalisation into the stem (the native train step) and callers that want the tensor."""
    x, table, layout, N, H, W = _u8_frames(u8, mean, std)
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=x.device)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 0.0, "bytes": 1.0 * x.numel() + 4.0 * out.numel()}
    with _dev(x):
        call("agrl_frames_normalize_u8", ptr(x), ptr(table), layout, ptr(out), N, H, W, _stream(x))
    return out


def erase_lists(rects, counts, N, H, W):
    """Validate per-frame erase rectangles against N frames of H x W -> (rects int32 ndarray (N, R, 4), counts int32 ndarray (N,)).
    ``rects`` HOST integer (N, R, 4), rows (y, x, h, w) = image rows y .. y+h-1, columns x .. x+w-1; ``counts`` HOST integer (N,): the
    first counts[n] rows of frame n count, whatever stands behind them is ignored. ValueError naming the first offending frame: device
    arrays, a wrong shape, R above ERASE_MAX_RECTS, a count outside 0..R, a negative entry or a rectangle that leaves the frame."""
    for a in (rects, counts):
        if isinstance(a, torch.Tensor) and a.is_cuda:
            raise ValueError("frames_normalize_erase: rects and counts are host arrays (they are validated before the upload)")
    r = np.asarray(rects)
    c = np.asarray(counts)
    if r.dtype.kind not in "iu" or c.dtype.kind not in "iu" or r.ndim != 3 or r.shape[0] != N or r.shape[2] != 4 or c.shape != (N,):
        raise ValueError("frames_normalize_erase: rects is an integer (N, R, 4) array and counts an integer (N,) array with N = %d, got %s %s "
                         "and %s %s" % (N, r.dtype, r.shape, c.dtype, c.shape))
    R = r.shape[1]
    if R > ERASE_MAX_RECTS:
        raise ValueError("frames_normalize_erase: %d rectangles per frame, at most %d" % (R, ERASE_MAX_RECTS))
    r, c = np.ascontiguousarray(r, dtype=np.int64), np.ascontiguousarray(c, dtype=np.int64)
    if ((c < 0) | (c > R)).any():
        n = int(np.argmax((c < 0) | (c > R)))
        raise ValueError("frames_normalize_erase: frame %d has a count of %d, 0..%d" % (n, int(c[n]), R))
    live = np.arange(R)[None, :] < c[:, None]
    bad = live & ((r < 0).any(2) | (np.abs(r) >= 2 ** 30).any(2) | (r[..., 0] + r[..., 2] > H) | (r[..., 1] + r[..., 3] > W))
    if bad.any():
        n, i = (int(v) for v in np.argwhere(bad)[0])
        raise ValueError("frames_normalize_erase: frame %d has rectangle %d = (y %d, x %d, h %d, w %d) outside its %d x %d frame" % (
            (n, i) + tuple(int(v) for v in r[n, i]) + (H, W)))
    return r.astype(np.int32), c.astype(np.int32)


def _erase_value(value):
    v = torch.tensor([float(f) for f in value], dtype=torch.float32)
    if v.numel() != 3:
        raise ValueError("the erase value is three numbers, one per channel: got %r" % (value,))
    return v


def frames_normalize_erase_reference(u8, rects, counts, value=PIXEL_MEAN, mean=PIXEL_MEAN, std=PIXEL_STD):
    """``frames_normalize_reference`` followed by the reference's random erasing (GroupRandomErasing / RandomErasing, transforms.py:274-324,
    487-531) as slice assignment: out[n, c, y:y+h, x:x+w] = float32(value[c]) for the first counts[n] rows (y, x, h, w) of rects[n]. uint8
    frames (..., 3, H, W) or (..., H, W, 3) with rects (..., R, 4) and counts (...) -> fp32 (..., 3, H, W). Pure torch, any device: what
    the CPU path uses and agrl_frames_normalize_erase_u8 is compared with bit for bit."""
    out = frames_normalize_reference(u8, mean, std)
    H, W = out.shape[-2:]
    flat = out.view(-1, 3, H, W)
    r = np.asarray(rects)
    r, c = erase_lists(r.reshape((-1,) + tuple(r.shape[-2:])), np.asarray(counts).reshape(-1), flat.shape[0], H, W)
    fill = _erase_value(value).to(out.device)
    for n in range(flat.shape[0]):
        for y, x, h, w in r[n, :c[n]].tolist():
            flat[n, :, y:y + h, x:x + w] = fill.view(3, 1, 1)
    return out


def frames_normalize_erase(u8, rects, counts, value=PIXEL_MEAN, mean=PIXEL_MEAN, std=PIXEL_STD):
    """The same on the GPU (agrl_frames_normalize_erase_u8): uint8 frames (N,3,H,W) or (N,H,W,3) on the device; ``rects`` / ``counts``
    HOST integer arrays (N, R, 4) / (N,), validated here (``erase_lists``) and uploaded non-blocking from pinned memory, in one copy
    -> fp32 NCHW (N,3,H,W). One launch, no synchronisation."""
    if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8 or u8.dim() != 4:
        raise ValueError("frames_normalize_erase: frames are uint8 (N,3,H,W) or (N,H,W,3), got %s" % (
            "%s %s" % (u8.dtype, tuple(u8.shape)) if isinstance(u8, torch.Tensor) else type(u8),))
    nchw = frames_layout(u8.shape) == 'nchw'
    r, c = erase_lists(rects, counts, u8.shape[0], u8.shape[2 if nchw else 1], u8.shape[3 if nchw else 2])
    fill = [float(f) for f in _erase_value(value)]
    if not u8.is_cuda:
        raise ValueError("frames_normalize_erase: frames must be on the GPU (frames_normalize_erase_reference is the CPU form)")
    x, table, layout, N, H, W = _u8_frames(u8, mean, std)
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=x.device)
    if N == 0:
        return out
    R = r.shape[1]
    rects_d = counts_d = None
    if R > 0:
        lists = torch.from_numpy(np.concatenate([r.reshape(-1), c])).pin_memory().to(x.device, non_blocking=True)
        rects_d, counts_d = lists[:N * R * 4], lists[N * R * 4:]
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 0.0, "bytes": 1.0 * x.numel() + 4.0 * out.numel()}
    with _dev(x):
        call("agrl_frames_normalize_erase_u8", ptr(x), ptr(table), layout, ptr(rects_d), ptr(counts_d), R, fill[0], fill[1], fill[2],
             ptr(out), N, H, W, _stream(x))
    return out


def clip_frames(x):
    """Validate uint8 clips as the models take them -- (B,S,3,H,W) or (B,S,H,W,3) -> (layout, B, S, H, W); ValueError otherwise."""
    if x.dim() != 5:
        raise ValueError("uint8 frames are (B,S,3,H,W) or (B,S,H,W,3), got %s" % (tuple(x.shape),))
    layout = frames_layout(x.shape)
    H, W = (x.shape[3], x.shape[4]) if layout == 'nchw' else (x.shape[2], x.shape[3])
    return layout, x.shape[0], x.shape[1], H, W


def clips_to_float(x, mean=PIXEL_MEAN, std=PIXEL_STD, erase=None):
    """uint8 clips (B,S,3,H,W) / (B,S,H,W,3) -> fp32 (B,S,3,H,W), normalised: agrl_frames_normalize_u8 on the GPU, the table on the CPU.
    The models call this in front of every path that does not fuse the normalisation into the stem (training, CPU).
    ``erase`` = (rects, counts[, value]), host integer (B,S,R,4) / (B,S): random erasing in the same pass (``frames_normalize_erase`` on
    the GPU, ``frames_normalize_erase_reference`` on the CPU); value defaults to PIXEL_MEAN, what GroupRandomErasing writes."""
    _, B, S, H, W = clip_frames(x)
    if erase is not None:
        rects, counts = np.asarray(erase[0]), np.asarray(erase[1])
        value = erase[2] if len(erase) > 2 else PIXEL_MEAN
        if rects.ndim != 4 or rects.shape[:2] != (B, S) or counts.shape != (B, S):
            raise ValueError("clips_to_float: erase is (rects (B,S,R,4), counts (B,S)) with (B,S) = %s, got %s and %s" % (
                (B, S), rects.shape, counts.shape))
        if not x.is_cuda:
            return frames_normalize_erase_reference(x, rects, counts, value, mean, std)
        return frames_normalize_erase(x.reshape((B * S,) + tuple(x.shape[2:])), rects.reshape((B * S,) + tuple(rects.shape[2:])),
                                      counts.reshape(B * S), value, mean, std).view(B, S, 3, H, W)
    if x.is_cuda:
        return frames_normalize(x.reshape((B * S,) + tuple(x.shape[2:])), mean, std).view(B, S, 3, H, W)
    return frames_normalize_reference(x, mean, std)


# ---- resize / crop / flip of uint8 clips (include/agrl_hip.h, "uint8 frames": agrl_clip_resample_u8) ------------------------
RESAMPLE_TAPS = 17        # taps per output element the kernel holds: a downscale of up to RESAMPLE_MAX_SCALE per axis
RESAMPLE_MAX_SCALE = 8
RESAMPLE_MAX_OUT = 512
_RESAMPLE_BITS = 22       # Pillow's PRECISION_BITS for 8-bit channels
ERASE_MAX_RECTS = 128     # rectangles per frame agrl_frames_normalize_erase_u8 holds (the reference draws at most 100)


@functools.lru_cache(maxsize=4096)
def _resample_taps(in_size, out_size, max_taps):
    if in_size < 1 or out_size < 1:
        raise ValueError("resample_taps: sizes are >= 1, got in=%d out=%d" % (in_size, out_size))
    if in_size == out_size:   # Pillow skips the pass: the identity as one tap of weight 1
        k = np.zeros((out_size, max_taps or 1), dtype=np.int32)
        k[:, 0] = 1 << _RESAMPLE_BITS
        bounds = np.stack([np.arange(out_size), np.ones(out_size, dtype=np.int64)], 1).astype(np.int32)
    else:
        scale = np.float64(in_size) / np.float64(out_size)
        fs = np.float64(max(scale, 1.0))
        support = fs          # the triangle filter's support of 1, stretched by the downscale
        center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
        lo = np.maximum((center - support + 0.5).astype(np.int64), 0)          # astype truncates towards zero, as C's (int) does
        hi = np.minimum((center + support + 0.5).astype(np.int64), in_size)
        count = hi - lo
        if max_taps is not None:
            count = np.minimum(count, max_taps)
        width = max_taps or int(count.max())
        j = lo[:, None] + np.arange(width, dtype=np.int64)[None, :]
        t = np.abs((j.astype(np.float64) - center[:, None] + 0.5) / fs)
        w = np.where((np.arange(width)[None, :] < count[:, None]) & (t < 1.0), 1.0 - t, 0.0)
        total = np.zeros(out_size, dtype=np.float64)
        for c in range(width):   # tap by tap, as the C loop accumulates (np.sum adds pairwise)
            total = total + w[:, c]
        k = (0.5 + (w / total[:, None]) * np.float64(1 << _RESAMPLE_BITS)).astype(np.int32)
        bounds = np.stack([lo, count], 1).astype(np.int32)
    k.setflags(write=False)
    bounds.setflags(write=False)
    return k, bounds


def resample_taps(in_size, out_size, max_taps=None):
    """The integer filter taps of Pillow's ``Image.resize(..., BILINEAR)`` along one axis of ``in_size`` -> ``out_size`` elements, all in
    fp64 as ImagingResample computes them: scale = in / out, fs = max(scale, 1), center = (i + 0.5) scale, taps j in
    [max(int(center - fs + 0.5), 0), min(int(center + fs + 0.5), in)) with w = 1 - |(j - center + 0.5) / fs| (0 from 1 on), divided by their
    sum and stored as int(0.5 + w 2^22). ``in_size == out_size`` is the identity: one tap of 2^22 at j = i.
    -> (k int32 (out, width) zero behind each row's taps, bounds int32 (out, 2) = (lo, count)); read-only, cached.
    ``max_taps``: what agrl_resample_taps_u8 and the resample kernel hold (RESAMPLE_TAPS): width = max_taps, a row with more taps keeps
    its first max_taps, normalised among themselves -- identical to the full row whenever in <= RESAMPLE_MAX_SCALE * out."""
    return _resample_taps(int(in_size), int(out_size), None if max_taps is None else int(max_taps))


def _resample_axis(a, out_size):
    """One pass of the resample along axis 0 of an integer array: (2^21 + sum(pixel * k)) >> 22, clamped to 0..255."""
    in_size = a.shape[0]
    if in_size == out_size:
        return a
    k, bounds = resample_taps(in_size, out_size)
    idx = np.minimum(bounds[:, :1].astype(np.int64) + np.arange(k.shape[1])[None, :], in_size - 1)   # (out, width); k is 0 behind count
    acc = (a[idx] * k.astype(np.int64).reshape(k.shape + (1,) * (a.ndim - 1))).sum(1)
    return np.clip((acc + (1 << (_RESAMPLE_BITS - 1))) >> _RESAMPLE_BITS, 0, 255)


def resample_vertical_first(win_h, win_w, out_h):
    """Image.resize runs the vertical pass FIRST on a sliver -- more than 100 times as tall as wide, and shrinking vertically; every
    other image horizontal first. (The rounding to uint8 between the passes makes the order visible from a width of 2 on.)"""
    return (win_h > 100 * win_w) & (out_h < win_h)


def resample_geometry(geometry, frames_shape, out_hw, max_scale=None):
    """Validate per-frame geometry rows (src_h, src_w, y0, x0, win_h, win_w, flip, 0) against a (N,Hs,Ws,3) container and an output size
    -> int32 ndarray (N, 8). ValueError naming the first offending frame: a window smaller than 1, a valid extent outside the container,
    and -- with ``max_scale``, the kernel's limits -- a window more than max_scale times the output along an axis, or a sliver that
    Pillow resamples vertical pass first (``resample_vertical_first``), which the kernel, horizontal first always, would get other bytes
    for. Slivers whose horizontal pass cannot change a byte -- one column wide, or as wide as the output -- are accepted: there the
    order of the passes is invisible."""
    N, Hs, Ws = int(frames_shape[0]), int(frames_shape[1]), int(frames_shape[2])
    OH, OW = int(out_hw[0]), int(out_hw[1])
    if OH < 1 or OW < 1:
        raise ValueError("clip_resample: output size %dx%d" % (OH, OW))
    g = np.asarray(geometry.cpu() if isinstance(geometry, torch.Tensor) else geometry)
    if g.shape != (N, 8) or g.dtype.kind not in "iu":
        raise ValueError("clip_resample: geometry is an integer (N, 8) array with N = %d, got %s %s" % (N, g.dtype, g.shape))
    g = np.ascontiguousarray(g, dtype=np.int64)
    checks = (
        ((np.abs(g) >= 2 ** 30).any(1), "an entry beyond 2^30 (window %d x %d)", (4, 5)),
        ((g[:, 4] < 1) | (g[:, 5] < 1), "a window of %d x %d", (4, 5)),
        ((g[:, 0] < 1) | (g[:, 0] > Hs) | (g[:, 1] < 1) | (g[:, 1] > Ws), "a valid extent of %%d x %%d outside its %d x %d container" % (Hs, Ws), (0, 1)),
    )
    if max_scale is not None:
        checks += (((g[:, 4] > max_scale * OH) | (g[:, 5] > max_scale * OW),
                    "a window of %%d x %%d, more than %d times the %d x %d output" % (max_scale, OH, OW), (4, 5)),
                   # the order of the passes shows only where the horizontal pass does something between them: not where it is the
                   # identity (win_w == OW: Pillow skips it), and not on a single column (win_w == 1: every tap row is normalised, so
                   # the pass copies the column's value, exactly, into every output column)
                   (resample_vertical_first(g[:, 4], g[:, 5], OH) & (g[:, 5] > 1) & (g[:, 5] != OW),
                    "a window of %d x %d, over 100 times as tall as wide: Pillow resamples it vertical pass first, the kernel cannot", (4, 5)))
    for bad, what, cols in checks:
        if bad.any():
            n = int(np.argmax(bad))
            raise ValueError("clip_resample: frame %d has " % n + what % tuple(int(g[n, c]) for c in cols))
    return g.astype(np.int32)


def clip_resample_reference(frames, geometry, out_hw):
    """uint8 frames (N,Hs,Ws,3) + geometry (N,8) -> uint8 (N,OH,OW,3) on the frames' device: per frame, the window
    [y0, y0+win_h) x [x0, x0+win_w) of the valid extent (src_h, src_w) -- coordinates outside it replicate the nearest edge -- resized as
    Pillow's ``crop().resize((OW, OH), BILINEAR)`` does, byte for byte (horizontal pass, rounded to uint8, vertical pass, with
    ``resample_taps``), then mirrored left-right where flip is set. Integer numpy arithmetic, any window size: the counterpart of
    ``frames_normalize_reference``, what agrl_clip_resample_u8 is compared with bit for bit."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("clip_resample: frames are uint8 (N,Hs,Ws,3), got %s %s" % (frames.dtype, tuple(frames.shape)))
    OH, OW = int(out_hw[0]), int(out_hw[1])
    geo = resample_geometry(geometry, frames.shape, (OH, OW)).astype(np.int64)
    src = frames.detach().cpu().numpy()
    out = np.empty((src.shape[0], OH, OW, 3), dtype=np.uint8)
    for n, (sh, sw, y0, x0, wh, ww, flip, _) in enumerate(geo.tolist()):
        rows = np.clip(y0 + np.arange(wh), 0, sh - 1)
        cols = np.clip(x0 + np.arange(ww), 0, sw - 1)
        win = src[n][rows][:, cols].astype(np.int64)                            # (win_h, win_w, 3)
        if resample_vertical_first(wh, ww, OH):
            win = _resample_axis(_resample_axis(win, OH).transpose(1, 0, 2), OW).transpose(1, 0, 2)
        else:
            win = _resample_axis(win.transpose(1, 0, 2), OW).transpose(1, 0, 2)     # horizontal first, as ImagingResample
            win = _resample_axis(win, OH)
        out[n] = win[:, ::-1] if flip else win
    return torch.from_numpy(out).to(frames.device)


def clip_resample(frames, geometry, out_hw, out=None):
    """The same on the GPU (agrl_clip_resample_u8): ``frames`` uint8 (N,Hs,Ws,3) on the device, channel-last and contiguous;
    ``geometry`` a HOST integer (N,8) array, validated here (``resample_geometry`` with the kernel's RESAMPLE_MAX_SCALE) and uploaded
    non-blocking; -> uint8 (N,OH,OW,3) (``out``: written in place when given). One launch, no synchronisation."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("clip_resample: frames are uint8 (N,Hs,Ws,3), got %s" % (
            "%s %s" % (frames.dtype, tuple(frames.shape)) if isinstance(frames, torch.Tensor) else type(frames)))
    if not frames.is_cuda or not frames.is_contiguous():
        raise ValueError("clip_resample: frames must be contiguous on the GPU")
    if isinstance(geometry, torch.Tensor) and geometry.is_cuda:
        raise ValueError("clip_resample: geometry is a host array (it is validated before the upload)")
    OH, OW = int(out_hw[0]), int(out_hw[1])
    if not (1 <= OH <= RESAMPLE_MAX_OUT and 1 <= OW <= RESAMPLE_MAX_OUT):
        raise ValueError("clip_resample: output size %dx%d, 1..%d each" % (OH, OW, RESAMPLE_MAX_OUT))
    N, Hs, Ws = frames.shape[:3]
    geo = torch.from_numpy(resample_geometry(geometry, frames.shape, (OH, OW), RESAMPLE_MAX_SCALE))
    handed = out is not None
    if out is None:
        out = torch.empty((N, OH, OW, 3), dtype=torch.uint8, device=frames.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (N, OH, OW, 3) or out.device != frames.device or not out.is_contiguous():
        raise ValueError("clip_resample: out must be contiguous uint8 %s on %s" % ((N, OH, OW, 3), frames.device))
    if N == 0:
        return out
    geo_d = geo.pin_memory().to(frames.device, non_blocking=True)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 0.0, "bytes": 1.0 * frames.numel() + 1.0 * out.numel()}
    with _dev(frames):
        call("agrl_clip_resample_u8", ptr(frames), ptr(geo_d), ptr(out), N, Hs, Ws, OH, OW, _stream(frames))
    if handed:
        written(out)
    return out


def resample_taps_device(in_size, out_size, device):
    """agrl_resample_taps_u8: the taps as the GPU computes them -> (k int32 (out, RESAMPLE_TAPS), bounds int32 (out, 2)) on ``device``."""
    k = torch.empty((int(out_size), RESAMPLE_TAPS), dtype=torch.int32, device=device)
    bounds = torch.empty((int(out_size), 2), dtype=torch.int32, device=device)
    with _dev(k):
        call("agrl_resample_taps_u8", int(in_size), int(out_size), ptr(k), ptr(bounds), _stream(k))
    return k, bounds


# ---- baseline JPEG decode (include/agrl_hip.h, "JPEG": agrl_jpeg_decode_u8; the host side is torchreid/device_decode.py) -----
JPEG_MAX_DIM = 4096       # the largest frame height / width the decoder takes
JPEG_DESC = 16            # ints per descriptor row, columns below
(JD_OFF, JD_LEN, JD_H, JD_W, JD_SAMP, JD_RI, JD_Q0, JD_DC0, JD_AC0, JD_WS) = (0, 1, 2, 3, 4, 5, 6, 9, 12, 15)
JPEG_GRAY, JPEG_444, JPEG_422, JPEG_420 = 0, 1, 2, 3          # sampling codes
JPEG_SCAN_ALIGN = 16      # every scan starts on a multiple of this in the byte buffer
JPEG_SCAN_PAD = 16        # and at least this many zero bytes follow its last byte: the device reads whole 8-byte words
JPEG_LOOK = 9             # bits of the Huffman look-ahead table
JPEG_HUFF_WORDS = 360     # int32 words of one decode-ready Huffman table:
JH_LOOK, JH_MAXCODE, JH_VALOFF, JH_VAL = 0, 256, 273, 290     # look[512] u16 (length << 8 | symbol, 0: longer than 9 bits) |
#                                                                maxcode[17] | valoffset[17] | huffval[256] u8 (64 words); 6 spare
JPEG_OK, JPEG_ERR_END, JPEG_ERR_CODE, JPEG_ERR_INDEX, JPEG_ERR_MARKER, JPEG_ERR_DESC = 0, 1, 2, 3, 4, 5
JPEG_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                        35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                        62, 63], dtype=np.int64)   # natural index of the k-th coefficient of the stream


def jpeg_frame_geometry(H, W, samp):
    """The block geometry of one frame -> (ncomp, (h0, v0), [(blocks per row, block rows, cropped height, cropped width)] per component).
    An interleaved scan covers whole MCUs of 8 h0 x 8 v0 pixels; a one-component scan has one block per MCU."""
    h0, v0 = {JPEG_GRAY: (1, 1), JPEG_444: (1, 1), JPEG_422: (2, 1), JPEG_420: (2, 2)}[int(samp)]
    mx, my = -(-W // (8 * h0)), -(-H // (8 * v0))
    comps = [(mx * h0, my * v0, H, W)]
    if samp != JPEG_GRAY:
        comps += [(mx, my, -(-H // v0), -(-W // h0))] * 2
    return len(comps), (h0, v0), comps


def jpeg_frame_blocks(H, W, samp):
    return sum(bw * bh for bw, bh, _, _ in jpeg_frame_geometry(H, W, samp)[2])


class _JpegBits:
    """The bit reader of the entropy decoder, as the kernel has it: a 64-bit window refilled bytewise, ``FF 00`` -> ``FF``; at any
    other marker and at the end of the scan it stops consuming and feeds zero bits, and counts them (``fed``): a symbol that used one of
    those has passed the end."""

    def __init__(self, data):
        self.d, self.n, self.p = data, len(data), 0
        self.acc = self.nb = self.fed = 0
        self.marker = False

    def fill(self):
        while self.nb <= 56:
            b = 0
            if not self.marker and self.p < self.n:
                b = self.d[self.p]
                if b == 0xFF:
                    nxt = self.d[self.p + 1] if self.p + 1 < self.n else 0xFF   # a lone FF at the very end counts as a marker
                    if nxt == 0:
                        self.p += 2
                    else:
                        self.marker, b = True, 0
                        self.fed += 8
                else:
                    self.p += 1
            else:
                self.fed += 8
            self.acc = ((self.acc << 8) | b) & 0xFFFFFFFFFFFFFFFF
            self.nb += 8

    def peek(self, n):
        return (self.acc >> (self.nb - n)) & ((1 << n) - 1)

    def skip(self, n):
        self.nb -= n

    def passed_end(self):
        return self.nb < self.fed

    def restart(self, index):
        """byte-align, consume FF D0+index -> True; False when whole bytes still stand in front of the marker or it is not there"""
        real = self.nb - self.fed
        if real >= 8 or self.p + 1 >= self.n or self.d[self.p] != 0xFF or self.d[self.p + 1] != 0xD0 + (index & 7):
            return False
        self.p += 2
        self.acc = self.nb = self.fed = 0
        self.marker = False
        return True


def jpeg_huffman_symbol(table, window):
    """One symbol out of a decode-ready table row (int32 (JPEG_HUFF_WORDS,)): ``window`` holds the next 16 bits of the stream, MSB
    first -> (code length, symbol), or (0, 0) when the bits are no code of the table. The 9-bit look-ahead first, then libjpeg's
    maxcode / valoffset walk for the longer codes."""
    look = table[JH_LOOK:JH_LOOK + 256].view(np.uint16)
    e = int(look[window >> (16 - JPEG_LOOK)])
    if e:
        return e >> 8, e & 255
    for l in range(JPEG_LOOK + 1, 17):
        code = window >> (16 - l)
        if code <= int(table[JH_MAXCODE + l]):
            return l, int(table[JH_VAL:JH_VAL + 64].view(np.uint8)[(code + int(table[JH_VALOFF + l])) & 255])
    return 0, 0


def _jpeg_extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _jpeg_entropy_reference(scan, H, W, samp, ri, quant, dc, ac):
    """One scan -> (coefficients int16 (blocks, 64) natural order, dequantised, component after component in raster block order; status).
    ``quant`` / ``dc`` / ``ac``: the component's tables."""
    ncomp, (h0, v0), comps = jpeg_frame_geometry(H, W, samp)
    base = np.cumsum([0] + [bw * bh for bw, bh, _, _ in comps])
    coef = np.zeros((int(base[-1]), 64), dtype=np.int16)
    mx, my = -(-W // (8 * h0)), -(-H // (8 * v0))
    br = _JpegBits(scan)
    pred = [0] * ncomp
    zz = JPEG_ZIGZAG.tolist()
    q = [t.astype(np.int64).tolist() for t in quant]
    for m in range(mx * my):
        if ri and m and m % ri == 0:
            if not br.restart(m // ri - 1):
                return coef, JPEG_ERR_MARKER
            pred = [0] * ncomp
        for c in range(ncomp):
            bw = comps[c][0]
            hc, vc = (h0, v0) if c == 0 else (1, 1)
            for blk in range(hc * vc):
                row = coef[int(base[c]) + ((m // mx) * vc + blk // hc) * bw + (m % mx) * hc + blk % hc]
                k = 0
                while k < 64:
                    br.fill()
                    l, sym = jpeg_huffman_symbol(dc[c] if k == 0 else ac[c], br.peek(16))
                    if l == 0:
                        return coef, JPEG_ERR_CODE
                    br.skip(l)
                    r, s = (0, sym & 15) if k == 0 else (sym >> 4, sym & 15)
                    if k and s == 0:
                        if br.passed_end():
                            return coef, JPEG_ERR_MARKER if br.marker else JPEG_ERR_END
                        if r != 15:
                            break          # EOB
                        k += 16            # ZRL
                        if k > 64:
                            return coef, JPEG_ERR_INDEX
                        continue
                    k += r
                    if k > 63:
                        return coef, JPEG_ERR_INDEX
                    v = _jpeg_extend(br.peek(s), s) if s else 0
                    br.skip(s)
                    if br.passed_end():
                        return coef, JPEG_ERR_MARKER if br.marker else JPEG_ERR_END
                    if k == 0:
                        v = pred[c] = pred[c] + v
                    w = (v * q[c][zz[k]]) & 0xFFFF          # stored as int16: the low 16 bits
                    row[zz[k]] = w - 0x10000 if w >= 0x8000 else w
                    k += 1
    return coef, JPEG_OK


def _jpeg_idct_pass(x, shift):
    """libjpeg's accurate integer IDCT (jidctint.c, CONST_BITS 13) along axis 0 of an int32 (8, ...) array, descaled by ``shift``."""
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * 4433
    tmp2, tmp3 = z1 - z3 * 15137, z1 + z2 * 6270
    tmp0, tmp1 = (x[0] + x[4]) << 13, (x[0] - x[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    half = np.int32(1 << (shift - 1))
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
                    ) + half >> shift


def _jpeg_idct_reference(coef):
    """int16 (n, 64) dequantised blocks -> uint8 (n, 8, 8): columns (>> 11), rows (>> 18), + 128, clamped. int32 throughout."""
    x = coef.astype(np.int32).reshape(-1, 8, 8)
    with np.errstate(over="ignore"):
        ws = _jpeg_idct_pass(x.transpose(1, 0, 2), 11)            # (row, n, col): along the columns
        out = _jpeg_idct_pass(ws.transpose(2, 1, 0), 18)          # (col, n, row): along the rows
    return np.clip(out.transpose(1, 2, 0) + 128, 0, 255).astype(np.uint8)


def _jpeg_plane(samples, bw, bh, ph, pw):
    """(bw bh, 8, 8) blocks in raster order -> the component plane, cropped to ph x pw"""
    return samples.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)[:ph, :pw]


def _jpeg_upsample_h(p, rnd_even, rnd_odd, shift, weight):
    """the triangle filter along the last axis, edges replicated: out[2i] = (w p[i] + p[i-1] + rnd_even) >> shift, out[2i+1] likewise"""
    last, nxt = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), dtype=np.int32)
    out[:, 0::2] = (weight * p + last + rnd_even) >> shift
    out[:, 1::2] = (weight * p + nxt + rnd_odd) >> shift
    return out


def _jpeg_upsample_reference(p, samp, H, W):
    """a cropped chroma plane -> H x W, libjpeg's fancy upsampling"""
    p = p.astype(np.int32)
    if samp == JPEG_422:
        return _jpeg_upsample_h(p, 1, 2, 2, 3)[:H, :W]
    if samp == JPEG_420:
        up, down = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
        rows = np.empty((2 * p.shape[0], p.shape[1]), dtype=np.int32)
        rows[0::2], rows[1::2] = 3 * p + up, 3 * p + down           # colsum of output rows 2r and 2r + 1
        return _jpeg_upsample_h(rows, 8, 7, 4, 3)[:H, :W]
    return p


def jpeg_decode_reference(plan):
    """The decoder's arithmetic on the CPU, the definition agrl_jpeg_decode_u8 is held to bit for bit: ``plan`` (device_decode.JpegPlan)
    -> (clip uint8 (F,Hc,Wc,3), status int32 (F)) as CPU tensors. Huffman decode per ITU T.81 out of the plan's decode-ready tables
    (``_jpeg_entropy_reference``), libjpeg's accurate integer IDCT, its fancy chroma upsampling on planes cropped to the image, its
    16-bit fixed-point YCbCr -> RGB. Pixels outside a frame's valid extent are 0. A frame whose status is not 0 stopped decoding there:
    its pixels are what the coefficients decoded so far give."""
    desc = np.asarray(plan.desc)
    F = desc.shape[0]
    Hc, Wc = int(plan.container[0]), int(plan.container[1])
    out = np.zeros((F, Hc, Wc, 3), dtype=np.uint8)
    status = np.zeros(F, dtype=np.int32)
    for f in range(F):
        d = desc[f].tolist()
        H, W, samp = d[JD_H], d[JD_W], d[JD_SAMP]
        ncomp, _, comps = jpeg_frame_geometry(H, W, samp)
        scan = bytes(plan.scans[d[JD_OFF]:d[JD_OFF] + d[JD_LEN]])
        coef, status[f] = _jpeg_entropy_reference(scan, H, W, samp, d[JD_RI], [plan.quant[d[JD_Q0 + c]] for c in range(ncomp)],
                                                  [plan.huff[d[JD_DC0 + c]] for c in range(ncomp)],
                                                  [plan.huff[d[JD_AC0 + c]] for c in range(ncomp)])
        samples = _jpeg_idct_reference(coef)
        planes, at = [], 0
        for bw, bh, ph, pw in comps:
            planes.append(_jpeg_plane(samples[at:at + bw * bh], bw, bh, ph, pw))
            at += bw * bh
        y = planes[0].astype(np.int32)
        if ncomp == 1:
            out[f, :H, :W] = y[:, :, None].astype(np.uint8)
            continue
        cb = _jpeg_upsample_reference(planes[1], samp, H, W) - 128
        cr = _jpeg_upsample_reference(planes[2], samp, H, W) - 128
        rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), y + ((116130 * cb + 32768) >> 16)], -1)
        out[f, :H, :W] = np.clip(rgb, 0, 255).astype(np.uint8)
    return torch.from_numpy(out), torch.from_numpy(status)


def jpeg_workspace_bytes(plan):
    """bytes of device workspace agrl_jpeg_decode_u8 needs for ``plan`` (agrl_jpeg_decode_workspace)"""
    return int(_hip.lib().agrl_jpeg_decode_workspace(int(plan.ws_blocks)))


def jpeg_decode(plan, out=None, device=None, workspace=None, operands=None):
    """The same on the GPU (agrl_jpeg_decode_u8): ``plan`` is the HOST batch plan of device_decode.jpeg_batch_plan; its byte buffer,
    descriptors and tables are uploaded non-blocking from pinned memory on the current stream (``operands``: what ``jpeg_upload`` returned,
    for a caller that uploaded ahead) -> (clip uint8 (F,Hc,Wc,3), status int32 (F)) on the device; ``out``: the clip is written in place
    when given. The entry point validates every descriptor row against the buffers before anything is launched. Three launches
    (entropy decode, IDCT, upsample + colour), no synchronisation: the caller reads ``status`` when it wants to."""
    F = int(plan.desc.shape[0])
    Hc, Wc = int(plan.container[0]), int(plan.container[1])
    if operands is None:
        if device is None:
            device = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
        operands = jpeg_upload(plan, device)
    scans_d, desc_d, quant_d, huff_d = operands
    device = scans_d.device
    handed = out is not None
    if out is None:
        out = torch.empty((F, Hc, Wc, 3), dtype=torch.uint8, device=device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (F, Hc, Wc, 3) or out.device != device or not out.is_contiguous():
        raise ValueError("jpeg_decode: out must be contiguous uint8 %s on %s" % ((F, Hc, Wc, 3), device))
    status = torch.empty((F,), dtype=torch.int32, device=device)
    if F == 0:
        return out, status
    need = jpeg_workspace_bytes(plan)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=device)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.device != device or not workspace.is_contiguous():
        raise ValueError("jpeg_decode: workspace must be contiguous uint8 of at least %d bytes on %s" % (need, device))
    desc_h = np.ascontiguousarray(plan.desc, dtype=np.int32)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 0.0, "bytes": 1.0 * scans_d.numel() + 2.0 * need + 1.0 * out.numel()}   # workspace written, read once
    with _dev(out):
        call("agrl_jpeg_decode_u8", ptr(scans_d), scans_d.numel(), desc_h.ctypes.data, ptr(desc_d), F, ptr(quant_d), quant_d.shape[0],
             ptr(huff_d), huff_d.shape[0], ptr(workspace), workspace.numel(), ptr(out), Hc, Wc, ptr(status), JPEG_STAGE_ALL, _stream(out))
    if handed:
        written(out)  # (the workspace is scratch: nothing reads it after the call)
    return out, status


JPEG_STAGE_ENTROPY, JPEG_STAGE_IDCT, JPEG_STAGE_COLOUR, JPEG_STAGE_ALL = 1, 2, 4, 7   # the stage mask of agrl_jpeg_decode_u8


def jpeg_upload(plan, device):
    """the plan's device operands -> (scans uint8, desc int32 (F,16), quant int16 (NQ,64), huff int32 (NH,360)) on ``device``: one pinned
    staging buffer, one non-blocking copy on the current stream"""
    parts = [np.ascontiguousarray(plan.scans, dtype=np.uint8), np.ascontiguousarray(plan.desc, dtype=np.int32).view(np.uint8).reshape(-1),
             np.ascontiguousarray(plan.quant, dtype=np.uint16).view(np.uint8).reshape(-1),
             np.ascontiguousarray(plan.huff, dtype=np.int32).view(np.uint8).reshape(-1)]
    assert parts[0].size % JPEG_SCAN_ALIGN == 0
    sizes = [p.size for p in parts]
    host = torch.empty((sum(sizes),), dtype=torch.uint8).pin_memory() if torch.cuda.is_available() else torch.empty((sum(sizes),), dtype=torch.uint8)
    at = 0
    for p in parts:
        host[at:at + p.size] = torch.from_numpy(p)
        at += p.size
    dev = host.to(device, non_blocking=True)
    a, b, c = sizes[0], sizes[0] + sizes[1], sizes[0] + sizes[1] + sizes[2]
    return (dev[:a], dev[a:b].view(torch.int32).view(-1, JPEG_DESC), dev[b:c].view(torch.int16).view(-1, 64),
            dev[c:].view(torch.int32).view(-1, JPEG_HUFF_WORDS))


# ---- PNG decode (include/agrl_hip.h, "PNG": agrl_png_decode_u8; the host side is torchreid/device_decode.py) ------------------------
PNG_MAX_DIM = 4096            # the largest frame height / width the decoder takes
PNG_MAX_INFLATED = 131072     # the largest H * (1 + W * channels): the inflated stream of a frame lives in one workgroup's LDS
PNG_DESC = 8                  # ints per descriptor row, columns below (three spare, zero)
PD_OFF, PD_LEN, PD_H, PD_W, PD_CH = 0, 1, 2, 3, 4
PNG_STREAM_ALIGN = 16         # every zlib stream starts on a multiple of this in the byte buffer
PNG_STREAM_PAD = 16           # and at least this many zero bytes follow its last byte: the device reads whole 8-byte words, one ahead
# the status codes: what png_decode_reference returns for each of inflate's own rejections (zlib's inflate.c / inftrees.c)
(PNG_OK, PNG_ERR_INPUT, PNG_ERR_HEADER, PNG_ERR_BTYPE, PNG_ERR_STORED, PNG_ERR_DESC, PNG_ERR_COUNTS, PNG_ERR_OVERSUB, PNG_ERR_INCOMPLETE,
 PNG_ERR_REPEAT, PNG_ERR_NOEOB, PNG_ERR_LITLEN, PNG_ERR_DISTSYM, PNG_ERR_DIST, PNG_ERR_SHORT, PNG_ERR_LONG, PNG_ERR_ADLER,
 PNG_ERR_FILTER) = range(18)
PNG_STATUS_NAMES = ("decoded", "input exhausted", "bad CMF / FLG", "block type 3", "stored LEN / NLEN mismatch", "descriptor row refused",
                    "more than 286 literal/length or 30 distance symbols", "over-subscribed code set", "incomplete code set",
                    "length repeat with nothing before it, or overrunning", "no end-of-block code", "invalid literal/length code",
                    "invalid distance code", "distance before the start of the output", "output shorter than the frame",
                    "output longer than the frame", "Adler-32 mismatch", "filter byte above 4")
PNG_STAGE_INFLATE, PNG_STAGE_FILTER, PNG_STAGE_STORE, PNG_STAGE_ALL = 1, 2, 4, 7   # the stage mask of agrl_png_decode_u8
_PNG_LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_PNG_LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_PNG_DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
              16385, 24577)
_PNG_DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
_PNG_CLORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_PNG_CODES, _PNG_LENS, _PNG_DISTS = 0, 1, 2
_PNG_FIXED_LENS = np.array([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, dtype=np.int64)


def png_frame_inflated(H, W, channels):
    """bytes the zlib stream of an 8-bit non-interlaced frame inflates to: a filter byte and W * channels samples per row"""
    return int(H) * (1 + int(W) * int(channels))


def _png_code_table(lens, kind):
    """Code lengths -> (status, table int32 (1 << maxbits,), maxbits): the canonical Huffman code of RFC 1951 3.2.2 as a flat look-up by
    the next ``maxbits`` bits of the stream (LSB first); an entry is ``length << 16 | symbol``, 0 where no code starts with those bits.
    inflate's own rejections (inftrees.c): an over-subscribed set; an incomplete one, except a distance set of ONE code of length 1;
    a set with no code at all is accepted for distances (every look-up is an invalid code) and incomplete otherwise."""
    lens = np.asarray(lens, dtype=np.int64)
    count = np.bincount(lens, minlength=16)
    maxbits = int(np.flatnonzero(count[1:]).max()) + 1 if count[1:].any() else 0
    if maxbits == 0:
        return (PNG_OK if kind == _PNG_DISTS else PNG_ERR_INCOMPLETE), np.zeros(2, dtype=np.int32), 1
    left = 1
    for l in range(1, 16):
        left = (left << 1) - int(count[l])
        if left < 0:
            return PNG_ERR_OVERSUB, None, 0
    if left > 0 and (kind != _PNG_DISTS or maxbits != 1):
        return PNG_ERR_INCOMPLETE, None, 0
    table = np.zeros(1 << maxbits, dtype=np.int32)
    code = 0
    nxt = [0] * 17
    for l in range(1, 16):
        code = (code + int(count[l - 1] if l > 1 else 0)) << 1
        nxt[l] = code
    for sym, l in enumerate(lens.tolist()):
        if l:
            c = nxt[l]
            nxt[l] += 1
            rev = int(format(c, "0%db" % l)[::-1], 2)
            table[rev::1 << l] = (l << 16) | sym
    return PNG_OK, table, maxbits


class _PngBits:
    """deflate's bit reader, LSB first; zeros beyond the end, and ``over`` once a field used one of them"""

    def __init__(self, data):
        self.n = len(data)
        self.d = bytes(data) + b"\0" * 8
        self.pos = 0

    def peek(self, n):
        p = self.pos >> 3
        return (int.from_bytes(self.d[p:p + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1) if p < self.n else 0

    def take(self, n):
        v = self.peek(n)
        self.pos += n
        return v

    @property
    def over(self):
        return self.pos > 8 * self.n


def _png_inflate_reference(stream, expected, counters=None, boundaries=()):
    """One zlib stream (RFC 1950 / 1951) -> (the inflated bytes so far, status): exactly ``expected`` bytes for status 0. ``counters``: a
    dict that receives what the stream exercised (block types, matches, ...); ``boundaries``: byte offsets inside the stream (where one
    IDAT chunk ends and the next begins), for the counter of Huffman codes that straddle one."""
    br = _PngBits(stream)
    out = bytearray()
    cnt = counters if counters is not None else {}
    for k in ("blocks", "empty_stored", "max_len", "max_dist", "dist_lt_len", "dist_1", "split_codes"):
        cnt.setdefault(k, 0)
    cnt.setdefault("btypes", set())
    edges = [8 * b for b in boundaries]

    def code(table, bits):
        at = br.pos
        e = int(table[br.peek(bits)])
        br.pos += (e >> 16) if e else 1
        if e and any(at < b < br.pos for b in edges):
            cnt["split_codes"] += 1
        return e

    cmf, flg = br.take(8), br.take(8)
    if br.over:
        return out, PNG_ERR_INPUT
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31 or (flg & 32):
        return out, PNG_ERR_HEADER
    cnt["wbits"] = (cmf >> 4) + 8
    last = 0
    while not last:
        last, btype = br.take(1), br.take(2)
        if br.over:
            return out, PNG_ERR_INPUT
        if btype == 3:
            return out, PNG_ERR_BTYPE
        cnt["blocks"] += 1
        cnt["btypes"].add(btype)
        if btype == 0:
            br.pos = (br.pos + 7) & ~7
            n, inv = br.take(16), br.take(16)
            if br.over:
                return out, PNG_ERR_INPUT
            if n != (inv ^ 0xFFFF):
                return out, PNG_ERR_STORED
            at = br.pos >> 3
            if at + n > br.n:
                return out, PNG_ERR_INPUT
            if len(out) + n > expected:
                return out, PNG_ERR_LONG
            out += br.d[at:at + n]
            br.pos += 8 * n
            cnt["empty_stored"] += n == 0
            continue
        if btype == 1:
            lens, nlen, ndist = np.concatenate([_PNG_FIXED_LENS, np.full(32, 5, dtype=np.int64)]), 288, 32
        else:
            nlen, ndist, ncode = br.take(5) + 257, br.take(5) + 1, br.take(4) + 4
            if br.over:
                return out, PNG_ERR_INPUT
            if nlen > 286 or ndist > 30:
                return out, PNG_ERR_COUNTS
            cl = np.zeros(19, dtype=np.int64)
            for i in range(ncode):
                cl[_PNG_CLORDER[i]] = br.take(3)
            if br.over:
                return out, PNG_ERR_INPUT
            st, ctab, cbits = _png_code_table(cl, _PNG_CODES)
            if st:
                return out, st
            lens = np.zeros(nlen + ndist, dtype=np.int64)
            i = 0
            while i < nlen + ndist:
                e = code(ctab, cbits)
                if br.over:
                    return out, PNG_ERR_INPUT
                sym = e & 0xFFFF
                if sym < 16:
                    lens[i] = sym
                    i += 1
                    continue
                prev = 0
                if sym == 16:
                    if i == 0:
                        return out, PNG_ERR_REPEAT
                    prev, rep = int(lens[i - 1]), 3 + br.take(2)
                elif sym == 17:
                    rep = 3 + br.take(3)
                else:
                    rep = 11 + br.take(7)
                if br.over:
                    return out, PNG_ERR_INPUT
                if i + rep > nlen + ndist:
                    return out, PNG_ERR_REPEAT
                lens[i:i + rep] = prev
                i += rep
            if lens[256] == 0:
                return out, PNG_ERR_NOEOB
        st, ltab, lbits = _png_code_table(lens[:nlen], _PNG_LENS)
        if st:
            return out, st
        st, dtab, dbits = _png_code_table(lens[nlen:nlen + ndist], _PNG_DISTS)
        if st:
            return out, st
        while True:
            e = code(ltab, lbits)
            if br.over:
                return out, PNG_ERR_INPUT
            sym = e & 0xFFFF
            if e == 0 or sym > 285:
                return out, PNG_ERR_LITLEN
            if sym < 256:
                if len(out) >= expected:
                    return out, PNG_ERR_LONG
                out.append(sym)
                continue
            if sym == 256:
                break
            n = _PNG_LBASE[sym - 257] + br.take(_PNG_LEXT[sym - 257])
            if br.over:
                return out, PNG_ERR_INPUT
            e = code(dtab, dbits)
            if br.over:
                return out, PNG_ERR_INPUT
            sym = e & 0xFFFF
            if e == 0 or sym > 29:
                return out, PNG_ERR_DISTSYM
            dist = _PNG_DBASE[sym] + br.take(_PNG_DEXT[sym])
            if br.over:
                return out, PNG_ERR_INPUT
            if dist > len(out):
                return out, PNG_ERR_DIST
            if len(out) + n > expected:
                return out, PNG_ERR_LONG
            start = len(out) - dist
            out += bytes(out[start + k % dist] for k in range(n)) if dist < n else out[start:start + n]
            cnt["max_len"], cnt["max_dist"] = max(cnt["max_len"], n), max(cnt["max_dist"], dist)
            cnt["dist_lt_len"] += dist < n
            cnt["dist_1"] += dist == 1
    if len(out) < expected:
        return out, PNG_ERR_SHORT
    br.pos = (br.pos + 7) & ~7
    hi, lo = br.take(16), br.take(16)
    if br.over:
        return out, PNG_ERR_INPUT
    want = (((hi & 255) << 8 | hi >> 8) << 16) | (lo & 255) << 8 | lo >> 8
    # Adler-32 as the device takes it: a = 1 + sum d_i, b = N + sum (N - i) d_i, any partition of the sums, modulo 65521
    d = np.frombuffer(bytes(out), dtype=np.uint8).astype(np.uint64)
    N = d.size
    a = (1 + int(d.sum())) % 65521
    b = (N + int((d * (N - np.arange(N, dtype=np.uint64))).sum() % 65521)) % 65521
    if ((b << 16) | a) != want:
        return out, PNG_ERR_ADLER
    return out, PNG_OK


def _png_unfilter_reference(raw, H, W, ch, counters=None):
    """The inflated bytes of a frame -> (samples uint8 (H, W * ch), status): the PNG filters None, Sub, Up, Average, Paeth (PNG
    specification, 9.2), bytes modulo 256, the row above the first being zeros"""
    rb = W * ch
    rows = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(H, 1 + rb)
    out = np.zeros((H, rb), dtype=np.uint8)
    prev = np.zeros(rb, dtype=np.int64)
    for y in range(H):
        ft = int(rows[y, 0])
        if ft > 4:
            return out, PNG_ERR_FILTER
        if counters is not None:
            counters.setdefault("filters", set()).add(ft)
        x = rows[y, 1:].astype(np.int64)
        if ft == 0:
            cur = x
        elif ft == 1:
            cur = np.cumsum(x.reshape(W, ch), axis=0).reshape(rb) & 255
        elif ft == 2:
            cur = (x + prev) & 255
        else:
            cur = np.zeros(rb, dtype=np.int64)
            xs, ps = x.tolist(), prev.tolist()
            cs = [0] * rb
            for i in range(rb):
                a = cs[i - ch] if i >= ch else 0
                b = ps[i]
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    c = ps[i - ch] if i >= ch else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cs[i] = (xs[i] + pred) & 255
            cur[:] = cs
        out[y] = cur
        prev = cur
    return out, PNG_OK


def png_decode_reference(plan, info=None):
    """The PNG decoder's arithmetic on the CPU and the definition of its status codes: ``plan`` (device_decode.PngPlan) -> (clip uint8
    (F,Hc,Wc,3), status int32 (F)) as CPU tensors, the device's layout: a frame in the top-left corner of its slot, grey replicated to
    RGB, zeros elsewhere. RFC 1950 / 1951 inflate with inflate's own rejections, then the five row filters, in plain Python / numpy;
    zlib itself takes no part. A frame whose status is not 0 leaves its whole slot zero. ``info``: a list that receives one dict per
    frame: ``inflated`` (the bytes, as far as they came) and what the stream exercised (``_png_inflate_reference``'s counters)."""
    desc = np.asarray(plan.desc)
    F = desc.shape[0]
    Hc, Wc = int(plan.container[0]), int(plan.container[1])
    out = np.zeros((F, Hc, Wc, 3), dtype=np.uint8)
    status = np.zeros(F, dtype=np.int32)
    for f in range(F):
        d = desc[f].tolist()
        H, W, ch = d[PD_H], d[PD_W], d[PD_CH]
        counters = {}
        if info is not None:
            info.append(counters)
        if (not (1 <= H <= min(PNG_MAX_DIM, Hc) and 1 <= W <= min(PNG_MAX_DIM, Wc) and ch in (1, 3)) or png_frame_inflated(H, W, ch) > PNG_MAX_INFLATED
                or d[PD_OFF] < 0 or d[PD_LEN] < 0 or d[PD_OFF] % 8 or d[PD_OFF] + (d[PD_LEN] + 7) // 8 * 8 + 8 > plan.streams.size):
            status[f] = PNG_ERR_DESC
            continue
        stream = bytes(plan.streams[d[PD_OFF]:d[PD_OFF] + d[PD_LEN]])
        edges = plan.boundaries[f] if getattr(plan, "boundaries", None) is not None and f < len(plan.boundaries) else ()
        raw, status[f] = _png_inflate_reference(stream, png_frame_inflated(H, W, ch), counters, edges)
        counters["inflated"] = bytes(raw)
        if status[f]:
            continue
        px, status[f] = _png_unfilter_reference(raw, H, W, ch, counters)
        if status[f]:
            continue
        out[f, :H, :W] = px.reshape(H, W, ch) if ch == 3 else px.reshape(H, W, 1)
    return torch.from_numpy(out), torch.from_numpy(status)


def png_upload(plan, device):
    """the plan's device operands -> (streams uint8, desc int32 (F,8)) on ``device``: one pinned staging buffer, one non-blocking copy
    on the current stream"""
    parts = [np.ascontiguousarray(plan.streams, dtype=np.uint8), np.ascontiguousarray(plan.desc, dtype=np.int32).view(np.uint8).reshape(-1)]
    assert parts[0].size % PNG_STREAM_ALIGN == 0
    n = parts[0].size + parts[1].size
    host = torch.empty((n,), dtype=torch.uint8).pin_memory() if torch.cuda.is_available() else torch.empty((n,), dtype=torch.uint8)
    host[:parts[0].size] = torch.from_numpy(parts[0])
    host[parts[0].size:] = torch.from_numpy(parts[1])
    dev = host.to(device, non_blocking=True)
    return dev[:parts[0].size], dev[parts[0].size:].view(torch.int32).view(-1, PNG_DESC)


def png_decode(plan, out=None, device=None, operands=None, stages=PNG_STAGE_ALL):
    """The same on the GPU (agrl_png_decode_u8): ``plan`` is the HOST batch plan of device_decode.png_batch_plan; its byte buffer and
    descriptors are uploaded non-blocking from pinned memory on the current stream (``operands``: what ``png_upload`` returned, for a
    caller that uploaded ahead) -> (clip uint8 (F,Hc,Wc,3), status int32 (F)) on the device; ``out``: the clip is written in place when
    given. The entry point validates every descriptor row against the buffers before anything is launched. One launch, one wavefront
    per frame, no workspace (the inflated stream lives in LDS), no synchronisation: the caller reads ``status`` when it wants to."""
    F = int(plan.desc.shape[0])
    Hc, Wc = int(plan.container[0]), int(plan.container[1])
    if operands is None:
        if device is None:
            device = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
        operands = png_upload(plan, device)
    streams_d, desc_d = operands
    device = streams_d.device
    handed = out is not None
    if out is None:
        out = torch.empty((F, Hc, Wc, 3), dtype=torch.uint8, device=device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (F, Hc, Wc, 3) or out.device != device or not out.is_contiguous():
        raise ValueError("png_decode: out must be contiguous uint8 %s on %s" % ((F, Hc, Wc, 3), device))
    status = torch.empty((F,), dtype=torch.int32, device=device)
    if F == 0:
        return out, status
    desc_h = np.ascontiguousarray(plan.desc, dtype=np.int32)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 0.0, "bytes": 1.0 * streams_d.numel() + 1.0 * out.numel()}
    with _dev(out):
        call("agrl_png_decode_u8", ptr(streams_d), streams_d.numel(), desc_h.ctypes.data, ptr(desc_d), F, ptr(out), Hc, Wc, ptr(status),
             int(stages), _stream(out))
    if handed:
        written(out)
    return out, status


def _stem_frames(x, mean, std):
    """The frames argument of the three stems: fp32 NCHW, or uint8 in either layout (normalised inside the kernel's input staging) ->
    (x, N, H, W, bytes per input element, (table, layout) or None)."""
    if x.dtype == torch.uint8:
        x, table, layout, N, H, W = _u8_frames(x, mean, std)
        return x, N, H, W, 1.0, (table, layout)
    assert x.dtype == torch.float32 and x.dim() == 4 and x.size(1) == 3
    x = x.contiguous()
    return x, x.shape[0], x.shape[2], x.shape[3], 4.0, None


def stem_out_shape(H, W):
    """(H, W) of a frame -> (CH, CW, PH, PW): the 7x7/2 pad-3 conv map and the 3x3/2 pad-1 max-pooled map of the three stems."""
    CH, CW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    return CH, CW, (CH + 2 - 3) // 2 + 1, (CW + 2 - 3) // 2 + 1


def stem(x_nchw, w_ohwi, bias, out_dtype, mean=PIXEL_MEAN, std=PIXEL_STD):
    """(N,3,H,W) fp32 NCHW -- or uint8 frames, (N,3,H,W) / (N,H,W,3), normalised with ``frame_table(mean, std)`` while the kernel stages
    them -> (N,PH,PW,64) NHWC. vmgn.py:281-284."""
    x_nchw, N, H, W, _, u8 = _stem_frames(x_nchw, mean, std)
    _, _, PH, PW = stem_out_shape(H, W)
    out = torch.empty((N, PH, PW, 64), dtype=out_dtype, device=x_nchw.device)
    with _dev(x_nchw):
        if u8 is not None:
            call("agrl_stem_conv_bn_relu_maxpool_u8", ptr(x_nchw), ptr(u8[0]), u8[1], ptr(w_ohwi), ptr(bias), ptr(out), N, H, W,
                 dtype_code(out_dtype), _stream(x_nchw))
        else:
            call("agrl_stem_conv_bn_relu_maxpool", ptr(x_nchw), ptr(w_ohwi), ptr(bias), ptr(out), N, H, W,
                 dtype_code(out_dtype), _stream(x_nchw))
    return out


PRECISIONS = ('fp32', LP_NAME, 'bf16x3', 'fp16x3')


def check_precision(precision, allowed=PRECISIONS, what="hip_precision"):
    """'fp32' exact-fp32 MFMA | LP_NAME ('fp16' or 'bf16': the loaded library's 16-bit storage type, fp32 accumulation) |
    'bf16x3' fp32 tensors, split-bf16 products | 'fp16x3' (round 6) fp32 tensors, conv products as three fp16 MFMAs on fp16 high /
    low halves with pre-scaled weights (22 significand bits per operand). Asking for the OTHER 16-bit type is an error, not a silent substitution."""
    if precision in allowed:
        return precision
    if precision in ('fp16', 'bf16'):
        raise ValueError("%s %r: the loaded library stores 16-bit data as %s (set AGRL_HIP_LP16=%s before importing torchreid to load "
                         "the other build)" % (what, precision, LP_NAME, precision))
    raise ValueError("%s must be one of %s, got %r" % (what, ", ".join(repr(a) for a in allowed), precision))


def is_lp16(precision):
    """True for the 16-bit mode (validates the name)."""
    return check_precision(precision, PRECISIONS, "precision") == LP_NAME


def pack_stem_weights_lp16(w_ohwi):
    """(64,7,7,3) fp32 OHWI (BN folded) -> (64,240) bf16: per filter row 8 taps x 4 channels, zero padded; 480-byte rows
    (30 sixteen-byte slots: the stride that makes the kernel's weight-fragment reads bank-conflict free)."""
    assert tuple(w_ohwi.shape) == (64, 7, 7, 3)
    w = torch.zeros((64, 7, 8, 4), dtype=torch.float32, device=w_ohwi.device)
    w[:, :, :7, :3] = w_ohwi.float()
    packed = torch.zeros((64, 240), dtype=LP_DTYPE, device=w_ohwi.device)
    packed[:, :224] = w.view(64, 224).to(LP_DTYPE)
    return packed.contiguous()


def stem_lp16(x_nchw, w_packed, bias, mean=PIXEL_MEAN, std=PIXEL_STD):
    """16-bit-MFMA stem: (N,3,H,W) fp32 NCHW -- or uint8 frames in either layout, as in ``stem`` -> (N,PH,PW,64) NHWC in the library's
    16-bit type (LP_DTYPE). vmgn.py:281-284."""
    assert w_packed.dtype == LP_DTYPE and tuple(w_packed.shape) == (64, 240)
    x_nchw, N, H, W, ebytes, u8 = _stem_frames(x_nchw, mean, std)
    CH, CW, PH, PW = stem_out_shape(H, W)
    out = torch.empty((N, PH, PW, 64), dtype=LP_DTYPE, device=x_nchw.device)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * N * CH * CW * 64 * 147, "bytes": ebytes * x_nchw.numel() + 2.0 * out.numel() + 2.0 * w_packed.numel(),
                            "conv": (7, 2, 3, 64, PH, PW)}
    with _dev(x_nchw):
        if u8 is not None:
            call("agrl_stem_conv_bn_relu_maxpool_lp16_u8", ptr(x_nchw), ptr(u8[0]), u8[1], ptr(w_packed), ptr(bias), ptr(out), N, H, W,
                 _stream(x_nchw))
        else:
            call("agrl_stem_conv_bn_relu_maxpool_lp16", ptr(x_nchw), ptr(w_packed), ptr(bias), ptr(out), N, H, W,
                 _stream(x_nchw))
    return out


def conv_bn_act(x, w_ohwi, bias, stride, pad, relu, residual=None, x_presplit=False, out_presplit=False):
    """NHWC conv (BN folded) [+ residual] [+ ReLU]. vmgn.py:45-65. ``x_presplit`` / ``out_presplit`` ('fp16x3' weights only): the
    input was / the output is to be stored with its fp16 halves already formed (agrl_conv2d_bn_act_split16: a tensor only a GEMM reads;
    the same shape and bytes, not readable as fp32)."""
    N, H, W, Cin = x.shape
    Cout, R, S, Cin2 = w_ohwi.shape
    assert Cin == Cin2 and x.dtype == w_ohwi.dtype
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    out = torch.empty((N, OH, OW, Cout), dtype=x.dtype, device=x.device)
    if residual is not None:
        assert residual.shape == out.shape and residual.dtype == out.dtype
    if _hip.PROFILE is not None:
        e = x.element_size()
        _hip.PROFILE_TAG = {"flops": 2.0 * N * OH * OW * Cout * R * S * Cin,
                            "bytes": e * (x.numel() + w_ohwi.numel() + out.numel() * (2 if residual is not None else 1)),
                            "conv": (R, stride, Cin, Cout, OH, OW)}
    unscale = getattr(w_ohwi, 'agrl_unscale', None)
    with _dev(x):
        if unscale is not None:
            # 'fp16x3': weights pre-scaled by a power of two and pre-split at pack time (split16_inloop_weights); every product as three fp16 MFMAs
            assert x.dtype == torch.float32 and getattr(w_ohwi, 'agrl_presplit', False), "fp16x3 weights come from split16_inloop_weights"
            call("agrl_conv2d_bn_act_split16", ptr(x), ptr(w_ohwi), ptr(bias), ptr(residual), ptr(out), N, H, W, Cin, Cout, R, S,
                 stride, pad, 1 if relu else 0, float(unscale), 1 if x_presplit else 0, 1 if out_presplit else 0, _stream(x))
        else:
            assert not (x_presplit or out_presplit), "pre-split activations exist in the 'fp16x3' arithmetic only"
            call("agrl_conv2d_bn_act", ptr(x), ptr(w_ohwi), ptr(bias), ptr(residual), ptr(out), N, H, W, Cin, Cout, R, S,
                 stride, pad, 1 if relu else 0, _gemm_code(x.dtype), _stream(x))
    return out


def conv1x1_dual_split16(x, x2, w_cat, bias, stride, relu=True, x2_presplit=False, out_planes=0):
    """relu([x sampled at the stride | x2] @ w_cat^T + bias) in the split-fp16 arithmetic on fp32 tensors: a first Bottleneck's conv3 + its
    1x1 stride-s downsample conv in one GEMM (vmgn.py:56-64). x (N,H,W,K1) block input, x2 (N,OH,OW,K2) conv2's output, w_cat (Cout,
    K1+K2) from split16_inloop_weights of the concatenation (ONE power of two for both halves) -> (N,OH,OW,Cout) fp32. ``x2_presplit``: x2
    was written by conv_bn_act(..., out_presplit=True). ``out_planes`` 2 / 3: the result leaves as split-fp16 planes (N,OH,OW,out_planes
    Cout) fp16 -- to_split16_planes of the fp32 map, without the map."""
    N, H, W, K1 = x.shape
    K2 = x2.shape[3]
    Cout = w_cat.shape[0]
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert x.dtype == torch.float32 and x2.dtype == torch.float32 and x.is_contiguous() and x2.is_contiguous()
    assert tuple(x2.shape[:3]) == (N, OH, OW) and tuple(w_cat.shape) == (Cout, K1 + K2) and getattr(w_cat, 'agrl_presplit', False)
    assert out_planes in (0, 2, 3)
    out = (torch.empty((N, OH, OW, out_planes * Cout), dtype=torch.float16, device=x.device) if out_planes
           else torch.empty((N, OH, OW, Cout), dtype=torch.float32, device=x.device))
    if _hip.PROFILE is not None:
        M = N * OH * OW
        _hip.PROFILE_TAG = {"flops": 2.0 * M * Cout * (K1 + K2), "bytes": 4.0 * (M * (K1 + K2) + w_cat.numel()) + out.numel() * out.element_size(),
                            "conv": (1, stride, K1 + K2, Cout, OH, OW)}
    with _dev(x):
        call("agrl_conv1x1_dual_split16", ptr(x), ptr(x2), ptr(w_cat), ptr(bias), ptr(out), N, H, W, stride, K1, K2, Cout,
             1 if relu else 0, float(w_cat.agrl_unscale), 1 if x2_presplit else 0, int(out_planes), _stream(x))
    return out


def split16_prescale(w):
    """fp32 weights -> the same tensor times 2^k, k chosen so that max |w| 2^k lies in [2^13, 2^14) (exact; fp16's largest finite
    value is 65504 = ~2^16), with ``.agrl_unscale`` = 2^-k riding on the tensor object: what agrl_conv2d_bn_act_split16 expects.
    With the largest weight at ~2^13.5 a weight 2^-13 of it still has a NORMAL fp16 low half, and anything smaller is off by at
    most 2^-25 absolute = 2^-38 of the largest."""
    import math
    amax = float(w.detach().abs().max())
    if not (amax > 0.0 and math.isfinite(amax)):
        k = 0
    else:
        k = 13 - math.frexp(amax)[1] + 1       # frexp: amax = m 2^e, m in [0.5, 1) -> amax 2^k in [2^13, 2^14)
    ws = (w.detach().float() * (2.0 ** k)).contiguous()
    ws.agrl_unscale = 2.0 ** (-k)
    return ws


def split16_inloop_weights(w):
    """fp32 weights (.., K), K % 32 == 0 -> the weight operand of the kernels that split in the k-loop (conv_bn_act on 'fp16x3' weights,
    conv1x1_dual_split16, graph_linear_mix): split16_prescale, then the fp16 high / low halves of every 32-value k-tile side by side
    (the layout of agrl_split16_weights_inloop: the same shape and bytes, NOT readable as fp32 any more). ``.agrl_unscale`` = 2^-k and
    ``.agrl_presplit`` ride on the tensor; ``.agrl_scaled`` keeps the scaled fp32 tensor for packers that derive other forms from it
    (split16_true_weights)."""
    ws = split16_prescale(w)
    K = ws.shape[-1]
    assert K % 32 == 0, "the in-loop split needs whole 32-element k-tiles (K = %d)" % K
    # pack-time host logic in torch ops (any device; a C caller has agrl_split16_weights_inloop, byte-identical:
    # tests/test_gpu_kernels.py::test_split16_inloop_weight_layout): (rows, tile, c, half, e) = lane group c's eight values of a k-tile
    t = ws.view(-1, K // 32, 2, 4, 4).permute(0, 1, 3, 2, 4)
    hi = t.to(torch.float16)
    lo = (t - hi.float()).to(torch.float16)
    out = torch.stack([hi, lo], dim=2).contiguous().view(torch.float32).view(ws.shape)
    out.agrl_unscale = ws.agrl_unscale
    out.agrl_presplit = True
    out.agrl_scaled = ws
    return out


def split16_true_weights(t):
    """The fp32 weights a split16_prescale / split16_inloop_weights tensor was made from (the power-of-two scale undone: exact)."""
    src = t.agrl_scaled if getattr(t, 'agrl_presplit', False) else t
    return src * t.agrl_unscale


# ---- split-fp16 PLANES (round 6): the conforming mode at speed -- include/agrl_hip.h, "Split-fp16 PLANES" ----------------------
def pack_stem_weights_split16(w_ohwi):
    """(64,7,7,3) fp32 OHWI (BN folded) -> (wh_packed, wl_packed, w_unscale): the fp16 high / low halves of w 2^k, each in the 16-bit
    stem's (64, 240) layout (per filter row 8 taps x 4 channels, zero padded, 480-byte rows)."""
    assert tuple(w_ohwi.shape) == (64, 7, 7, 3)
    ws = split16_prescale(w_ohwi)
    w4 = torch.zeros((64, 7, 8, 4), dtype=torch.float32, device=w_ohwi.device)
    w4[:, :, :7, :3] = ws
    wh = w4.to(torch.float16)
    wl = (w4 - wh.float()).to(torch.float16)
    out = []
    for t in (wh, wl):
        packed = torch.zeros((64, 240), dtype=torch.float16, device=w_ohwi.device)
        packed[:, :224] = t.view(64, 224)
        out.append(packed.contiguous())
    return out[0], out[1], ws.agrl_unscale


def stem_split16(x_nchw, wh_packed, wl_packed, unscale, bias, mean=PIXEL_MEAN, std=PIXEL_STD):
    """Split-fp16 stem: (N,3,H,W) fp32 NCHW -- or uint8 frames in either layout, as in ``stem`` -> (N,PH,PW,64) fp32 NHWC
    (agrl_stem_split16). vmgn.py:281-284."""
    x_nchw, N, H, W, ebytes, u8 = _stem_frames(x_nchw, mean, std)
    CH, CW, PH, PW = stem_out_shape(H, W)
    out = torch.empty((N, PH, PW, 64), dtype=torch.float32, device=x_nchw.device)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * N * CH * CW * 64 * 147, "bytes": ebytes * x_nchw.numel() + 4.0 * out.numel() + 4.0 * wh_packed.numel(),
                            "conv": (7, 2, 3, 64, PH, PW)}
    with _dev(x_nchw):
        if u8 is not None:
            call("agrl_stem_split16_u8", ptr(x_nchw), ptr(u8[0]), u8[1], ptr(wh_packed), ptr(wl_packed), ptr(bias), ptr(out), N, H, W,
                 float(unscale), _stream(x_nchw))
        else:
            call("agrl_stem_split16", ptr(x_nchw), ptr(wh_packed), ptr(wl_packed), ptr(bias), ptr(out), N, H, W, float(unscale), _stream(x_nchw))
    return out


def split16_planes_available():
    """The plane kernels exist in the fp16 build of the library only."""
    return LP_NAME == 'fp16'


def split16_plane_weights(w, segments=None, pair_first=False):
    """fp32 weights (Cout, K) / OHWI (Cout, R, S, Cin) -> (fp16 tensor with 3 x the innermost axis = [wh | wh 2^-11 | wl] of w 2^k,
    2^-k): the operand the plane kernels multiply with activation planes [xh | xl 2^11 | xh] -- xh wh + xl wh + xh wl in one
    accumulator. k as in split16_prescale (max |w| 2^k in [2^13, 2^14)); ONE k for the whole tensor, also for the two-source form
    (``segments`` = [K1, K2]: the innermost axis is [W1 | W2] and each source gets its own plane triple, [W1 triple | W2 triple]).
    ``pair_first``: the first source is a plane PAIR [xh | xl 2^11] (include/agrl_hip.h, "Plane PAIRS"): its columns run per
    128-channel slab c as [wh_c | wl_c | wh_c 2^-11], against the kernel's slab reads [xh_c | xh_c | xl_c]."""
    ws = split16_prescale(w)
    parts = []
    for i, seg in enumerate(torch.split(ws, segments or [ws.shape[-1]], dim=-1)):
        wh = seg.to(torch.float16)
        wl = (seg - wh.float()).to(torch.float16)
        wh_s = (wh.float() * (2.0 ** -11)).to(torch.float16)
        if pair_first and i == 0:
            assert seg.shape[-1] % 128 == 0
            lead = tuple(seg.shape[:-1])
            slabs = [t.reshape(lead + (-1, 128)) for t in (wh, wl, wh_s)]
            parts.append(torch.stack(slabs, dim=-2).reshape(lead + (3 * seg.shape[-1],)))
        else:
            parts += [wh, wh_s, wl]
    return torch.cat(parts, dim=-1).contiguous(), ws.agrl_unscale


def to_split16_planes(x, nplanes=3):
    """fp32 (..., C) -> fp16 (..., 3 C) = [hi | lo 2^11 | hi], or with ``nplanes`` = 2 the pair (..., 2 C) = [hi | lo 2^11]
    (agrl_split16_planes)."""
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] % 4 == 0 and nplanes in (2, 3)
    Cc = x.shape[-1]
    out = torch.empty(tuple(x.shape[:-1]) + (nplanes * Cc,), dtype=torch.float16, device=x.device)
    with _dev(x):
        call("agrl_split16_planes", ptr(x), ptr(out), x.numel() // Cc, Cc, nplanes, _stream(x))
    return out


def to_split16_weight_planes(x, scale):
    """fp32 (rows, C) -> fp16 (rows, 3 C) = [h | h 2^-11 | l] of x * scale (a power of two), on the device (agrl_split16_weight_planes):
    the gallery side of distmat_split16."""
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2 and x.shape[1] % 4 == 0
    out = torch.empty((x.shape[0], 3 * x.shape[1]), dtype=torch.float16, device=x.device)
    with _dev(x):
        call("agrl_split16_weight_planes", ptr(x), ptr(out), x.shape[0], x.shape[1], float(scale), _stream(x))
    return out


def distmat_split16(q3, g3, metric, g_unscale, qn=None, gn=None, out=None):
    """q3 (m, 3D) query planes, g3 (n, 3D) gallery weight planes -> fp32 (m, n) distance matrix in the split-fp16 arithmetic
    (agrl_distmat_split16). distance.py:59-89."""
    m, D3 = q3.shape
    n = g3.shape[0]
    assert g3.shape[1] == D3 and q3.dtype == torch.float16 and g3.dtype == torch.float16
    handed = out is not None
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=q3.device)
    code = METRIC_EUCLIDEAN if metric == "euclidean" else METRIC_COSINE
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * m * n * D3 / 3, "mfma_flops": 2.0 * m * n * D3, "bytes": 2.0 * (m + n) * D3 + 4.0 * m * n}
    ws = None
    if (-(-m // 64)) * (-(-n // 128)) < 256:
        ws = torch.empty((8 * m * n,), dtype=torch.float32, device=q3.device)
    with _dev(q3):
        call("agrl_distmat_split16", ptr(q3), ptr(g3), ptr(qn), ptr(gn), out.data_ptr(), m, n, D3, out.stride(0), code, float(g_unscale),
             ptr(ws), 0 if ws is None else ws.numel() * 4, _stream(q3))
    if handed:
        written(out)
    return out


def from_split16_planes(x3, nplanes=3):
    """planes (..., 3 C) (or a pair, (..., 2 C)) -> fp32 (..., C) = hi + lo 2^-11 (exact): tests and the stage-by-stage parity hooks
    (torch arithmetic: not on the product path)."""
    Cc = x3.shape[-1] // nplanes
    return x3[..., :Cc].float() + x3[..., Cc:2 * Cc].float() * (2.0 ** -11)


def conv1x1_split16(x3, packed, unscale, bias, Cout, residual3=None, relu=True, x2=None, layout=0):
    """1x1 conv on planes: act(w_unscale [x3 | x2] @ W3^T + bias + residual) -> planes (N,H,W,3 Cout). vmgn.py:48-50, :56-64.
    ``layout`` bit 0: x3 is a plane pair (N,H,W,2 K) with weights from split16_plane_weights(pair_first=True); bit 1: the residual
    and the result are pairs (N,H,W,2 Cout). x2 is always a triple."""
    N, H, W, Kx = x3.shape
    K3 = Kx // 2 * 3 if layout & 1 else Kx     # the k-loop's columns
    K23 = 0 if x2 is None else x2.shape[3]
    M = N * H * W
    no = 2 if layout & 2 else 3
    assert x3.dtype == torch.float16 and x3.is_contiguous() and packed.numel() == 2 * (K3 + K23) * Cout
    assert residual3 is None or (residual3.dtype == torch.float16 and residual3.is_contiguous() and tuple(residual3.shape) == (N, H, W, no * Cout))
    out = torch.empty((N, H, W, no * Cout), dtype=torch.float16, device=x3.device)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * M * Cout * (K3 + K23) / 3, "mfma_flops": 2.0 * M * Cout * (K3 + K23),
                            "bytes": 2.0 * (x3.numel() + (0 if x2 is None else x2.numel()) + out.numel() + (0 if residual3 is None else residual3.numel() * 2 // no)) + packed.numel()}
    with _dev(x3):
        if x2 is None:
            call("agrl_conv1x1_split16", ptr(x3), ptr(packed), ptr(bias), ptr(residual3), ptr(out), M, K3, Cout, 1 if relu else 0,
                 float(unscale), int(layout), _stream(x3))
        else:
            assert residual3 is None and x2.dtype == torch.float16 and x2.is_contiguous() and tuple(x2.shape[:3]) == (N, H, W)
            call("agrl_conv1x1_split16_dual", ptr(x3), ptr(x2), ptr(packed), ptr(bias), ptr(out), M, K3, K23, Cout, 1 if relu else 0,
                 float(unscale), int(layout), _stream(x3))
    return out


def conv1x1_split16_pool(x3, packed, unscale, bias, Cout, residual3, splits, mean, relu=True, layout=0):
    """Last conv of a layer-4 branch on planes with the frame pooling in the epilogue (the unrounded fp32 values are pooled; no map).
    -> pooled fp32 (F, P, Cout). vmgn.py:56-64 + :298-308."""
    N, H, W, K3 = x3.shape
    assert x3.dtype == torch.float16 and x3.is_contiguous() and (H, W) == (16, 8) and packed.numel() == 2 * K3 * Cout
    assert not (layout & 1), "the pooled conv's input is conv2's output: a triple"
    assert residual3 is None or (residual3.dtype == torch.float16 and residual3.is_contiguous()
                                 and tuple(residual3.shape) == (N, H, W, (2 if layout & 2 else 3) * Cout))
    P = int(sum(splits))
    pooled = torch.empty((N, P, Cout), dtype=torch.float32, device=x3.device)
    arr = (C.c_int * len(splits))(*[int(s_) for s_ in splits])
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * N * H * W * Cout * K3 / 3, "mfma_flops": 2.0 * N * H * W * Cout * K3,
                            "bytes": 2.0 * (x3.numel() + (residual3.numel() if residual3 is not None else 0)) + packed.numel() + 4.0 * pooled.numel()}
    with _dev(x3):
        call("agrl_conv1x1_split16_pool", ptr(x3), ptr(packed), ptr(bias), ptr(residual3), ptr(pooled), N, H, W, K3, Cout,
             1 if relu else 0, arr, len(splits), 1 if mean else 0, float(unscale), int(layout), _stream(x3))
    return pooled


def conv3x3_split16(x3, packed, unscale, bias, Cout, relu=True):
    """relu(conv3x3(x) + bias), stride 1 / pad 1, on planes -> planes (N,H,W,3 Cout). vmgn.py:52-54."""
    N, H, W, Cin3 = x3.shape
    assert x3.dtype == torch.float16 and x3.is_contiguous() and packed.numel() == 2 * 9 * Cin3 * Cout
    out = torch.empty((N, H, W, 3 * Cout), dtype=torch.float16, device=x3.device)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * N * H * W * Cout * 9 * Cin3 / 3, "mfma_flops": 2.0 * N * H * W * Cout * 9 * Cin3,
                            "bytes": 2.0 * (x3.numel() + out.numel()) + packed.numel()}
    with _dev(x3):
        call("agrl_conv3x3_packed_split16", ptr(x3), ptr(packed), ptr(bias), ptr(out), N, H, W, Cin3, Cout, 1 if relu else 0,
             float(unscale), _stream(x3))
    return out


def conv1x1_dual_supported(x1, x2, w_cat):
    """The two-source pointwise GEMM exists for bf16, K1 == 2 K2, K1 % 64 == 0, Cout % 256 == 0 (layer-4 first blocks)."""
    K1, K2 = x1.shape[-1], x2.shape[-1]
    return (x1.dtype == LP_DTYPE and x2.dtype == LP_DTYPE and K1 == 2 * K2 and K1 % 64 == 0
            and w_cat.shape[0] % 256 == 0 and x1.shape[:-1] == x2.shape[:-1])


def conv1x1_dual(x1, x2, w_cat, bias, relu=True):
    """relu([x1 | x2] @ w_cat^T + bias): a first Bottleneck's conv3 + its 1x1 stride-1 downsample conv in one GEMM
    (vmgn.py:56-64). x1 (N,H,W,K1) block input, x2 (N,H,W,K2) conv2 output, w_cat (Cout, K1+K2) -> (N,H,W,Cout) bf16."""
    N, H, W, K1 = x1.shape
    K2 = x2.shape[-1]
    Cout = w_cat.shape[0]
    assert tuple(w_cat.shape) == (Cout, K1 + K2) and w_cat.dtype == x1.dtype
    out = torch.empty((N, H, W, Cout), dtype=x1.dtype, device=x1.device)
    M = N * H * W
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * M * Cout * (K1 + K2), "bytes": 2.0 * (x1.numel() + x2.numel() + w_cat.numel() + out.numel()),
                            "conv": (1, 1, K1 + K2, Cout, H, W)}
    with _dev(x1):
        call("agrl_conv1x1_dual_bn_act", ptr(x1), ptr(x2), ptr(w_cat), ptr(bias), ptr(out), M, K1, K2, Cout, 1 if relu else 0,
             _stream(x1))
    return out


def conv1x1_bn_act_pool(x, w_ohwi, bias, residual, splits, mean, want_lp, relu=True):
    """Last 1x1 conv of a layer4 branch with the frame pooling fused in (bf16, 128-pixel frames): the 2048-channel map
    is never written. -> pooled fp32 (F, P, Cout) [, bf16 copy]. vmgn.py:45-65 + :298-308."""
    N, H, W, Cin = x.shape
    Cout = w_ohwi.shape[0]
    assert x.dtype == LP_DTYPE and tuple(w_ohwi.shape[1:3]) == (1, 1) and H * W == 128
    P = int(sum(splits))
    pooled = torch.empty((N, P, Cout), dtype=torch.float32, device=x.device)
    pooled_lp = torch.empty((N, P, Cout), dtype=LP_DTYPE, device=x.device) if want_lp else None
    arr = (C.c_int * len(splits))(*[int(s) for s in splits])
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * N * H * W * Cout * Cin,
                            "bytes": 2.0 * (x.numel() + w_ohwi.numel() + (residual.numel() if residual is not None else 0)) + 4.0 * pooled.numel()}
    with _dev(x):
        call("agrl_conv1x1_bn_act_pool", ptr(x), ptr(w_ohwi), ptr(bias), ptr(residual), None, ptr(pooled), ptr(pooled_lp),
             N, H, W, Cin, Cout, 1 if relu else 0, arr, len(splits), 1 if mean else 0, _stream(x))
    return pooled, pooled_lp


# (Cmid, Cout, Cnext) of the layer-3 / layer-4 seams csrc/bottleneck_seam.hip is built for (the third: layer 3 -> a layer-4 branch)
SEAM_SHAPES = ((256, 1024, 256), (512, 2048, 512), (256, 1024, 512))


def bottleneck_seam_supported(w3, w1_next, pixels=None):
    """conv3 + residual -> next conv1 back to back (agrl_bottleneck_seam): 16-bit weights of a layer-3 / layer-4 seam, and --
    when ``pixels`` is given -- a pixel count made of whole 128-pixel tiles (16 x 8 frames)."""
    return (w3.dtype == LP_DTYPE and w1_next.dtype == LP_DTYPE and w3.dim() == 4 and tuple(w3.shape[1:3]) == (1, 1)
            and (w3.shape[3], w3.shape[0], w1_next.shape[0]) in SEAM_SHAPES and tuple(w1_next.shape[1:]) == (1, 1, w3.shape[0])
            and (pixels is None or pixels % 128 == 0))


def bottleneck_seam_pack(w3, w1_next):
    """The two (static) weight matrices of a seam re-ordered once into the per-wave MFMA fragment streams the kernel loads
    straight into registers -> one uint8 tensor of agrl_bottleneck_seam_packed_bytes bytes."""
    assert bottleneck_seam_supported(w3, w1_next)
    Cout, Cmid, Cnext = w3.shape[0], w3.shape[3], w1_next.shape[0]
    w3, w1_next = w3.contiguous(), w1_next.contiguous()
    nbytes = int(_hip.lib().agrl_bottleneck_seam_packed_bytes(Cmid, Cout, Cnext))
    assert nbytes == 2 * (w3.numel() + w1_next.numel())
    packed = torch.empty((nbytes,), dtype=torch.uint8, device=w3.device)
    with _dev(w3):
        call("agrl_bottleneck_seam_pack", ptr(w3), ptr(w1_next), ptr(packed), Cmid, Cout, Cnext, _stream(w3))
    return packed


def bottleneck_seam(y2, packed, b3, residual, b1_next, dims):
    """out = relu(conv3(y2) + residual), z = relu(conv1_next(out)) in one pass over 128-pixel tiles; ``packed`` from
    bottleneck_seam_pack, ``dims`` = (Cmid, Cout, Cnext). vmgn.py:56-64 (block i) + :48-50 (block i+1).
    -> out (N,H,W,Cout), z (N,H,W,Cnext) 16-bit NHWC."""
    Cmid, Cout, Cnext = dims
    N, H, W, C = y2.shape
    M = N * H * W
    assert y2.dtype == LP_DTYPE and C == Cmid and residual.shape == (N, H, W, Cout) and residual.dtype == y2.dtype and M % 128 == 0
    assert y2.is_contiguous() and residual.is_contiguous()
    out = torch.empty((N, H, W, Cout), dtype=y2.dtype, device=y2.device)
    z = torch.empty((N, H, W, Cnext), dtype=y2.dtype, device=y2.device)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * M * (Cmid * Cout + Cout * Cnext),
                            "bytes": 2.0 * (y2.numel() + residual.numel() + out.numel() + z.numel()) + packed.numel(),
                            "conv": (1, 1, Cmid, Cout, H, W)}
    with _dev(y2):
        call("agrl_bottleneck_seam", ptr(y2), ptr(packed), ptr(b3), ptr(residual), ptr(out), ptr(b1_next), ptr(z), M, Cmid, Cout,
             Cnext, _stream(y2))
    return out, z


CHAIN_MAX = 4   # Bottlenecks per agrl_bottleneck_chain launch


def bottleneck_chain_table(blocks):
    """The device table of agrl_bottleneck_chain for the consecutive Bottlenecks ``blocks`` (pack_stage dicts with 'c2p' and 'seam';
    blocks[i]['seam'] already holds the conv1 of the block behind it): one row of 8 pointers per block -- conv2's packed stream, b2,
    the seam's packed stream, b3, the next conv1's bias ('seam_b1n'). Built once per pack: the tensors it points into are the pack's."""
    rows = [[b['c2p'].data_ptr(), b['c2'][1].data_ptr(), b['seam'].data_ptr(), b['c3'][1].data_ptr(), b['seam_b1n'].data_ptr(), 0, 0, 0]
            for b in blocks]
    return torch.tensor(rows, dtype=torch.int64).to(blocks[0]['c2p'].device)


def bottleneck_chain_block_ok(blk):
    """A pack_stage block the chained kernel can run: packed 3x3 and seam of the 256 / 1024 / 256 shape, identity shortcut."""
    return ('c2p' in blk and 'seam' in blk and 'seam_b1n' in blk and blk['ds'] is None and blk['stride'] == 1
            and blk.get('seam_dims') == (256, 1024, 256) and tuple(blk['c2'][0].shape) == (256, 3, 3, 256)
            and blk['c2'][0].dtype == LP_DTYPE)


def bottleneck_chain_supported(z, a, blocks, forced=False):
    """agrl_bottleneck_chain applies: the 16-bit type, contiguous (F,16,8,256) / (F,16,8,1024) maps, 1 .. CHAIN_MAX blocks that are
    all bottleneck_chain_block_ok -- and the library's switch says so for this many frames (``forced``: the switch is not asked)."""
    if not (1 <= len(blocks) <= CHAIN_MAX and all(bottleneck_chain_block_ok(b) for b in blocks)):
        return False
    if not (z.dtype == LP_DTYPE and a.dtype == LP_DTYPE and z.dim() == 4 and tuple(z.shape[1:]) == (16, 8, 256)
            and tuple(a.shape) == (z.shape[0], 16, 8, 1024) and z.is_contiguous() and a.is_contiguous()):
        return False
    return forced or bool(_hip.lib().agrl_bottleneck_chain_enabled(int(z.shape[0])))


def bottleneck_chain(z, a, table, n, work=None, out=None):
    """``n`` chained Bottlenecks of layer 3 in one launch (csrc/bottleneck_chain.hip): z (F,16,8,256) conv1 output of the first, a
    (F,16,8,1024) the residual entering it, ``table`` from bottleneck_chain_table (rows 0 .. n-1 are used). ``work``: n - 1 buffers
    like ``a`` for the inner residual-stream maps, reusable from call to call (None: allocated here); ``out``: the buffer of a_n. No two
    of a, work[i], out may overlap (the library checks).
    -> (a_n, z_{n+1}): the last block's output and the conv1 output of the block behind the chain."""
    F = z.shape[0]
    assert 1 <= n <= CHAIN_MAX and table.dtype == torch.int64 and tuple(table.shape[1:]) == (8,) and table.shape[0] >= n
    assert z.dtype == LP_DTYPE and a.dtype == LP_DTYPE and tuple(z.shape) == (F, 16, 8, 256) and tuple(a.shape) == (F, 16, 8, 1024)
    assert z.is_contiguous() and a.is_contiguous()
    handed = ([] if out is None else [out]) + ([] if work is None else list(work[:n - 1]))     # the caller's buffers: bumped below
    if work is None:
        work = [torch.empty_like(a) for _ in range(n - 1)]
    assert len(work) >= n - 1 and all(w.dtype == a.dtype and w.numel() == a.numel() and w.is_contiguous() for w in work[:n - 1])
    out = torch.empty_like(a) if out is None else out
    assert out.dtype == a.dtype and out.numel() == a.numel() and out.is_contiguous()
    zn = torch.empty_like(z)
    bufs = (C.c_void_p * n)(*([ptr(w) for w in work[:n - 1]] + [ptr(out)]))
    if _hip.PROFILE is not None:
        M = F * 128
        _hip.PROFILE_TAG = {"flops": 2.0 * M * n * (9 * 256 * 256 + 2 * 256 * 1024),
                            "bytes": 2.0 * (z.numel() + zn.numel() + (2 * n) * a.numel()) + n * 2.0 * (9 * 256 * 256 + 2 * 256 * 1024)}
    with _dev(z):
        call("agrl_bottleneck_chain", ptr(z), ptr(a), ptr(table), bufs, ptr(zn), F, n, _stream(z))
    if handed:
        written(handed)
    return out, zn


def conv3x3_packed_enabled():
    """Always True: the models run every packed 3x3 weight through conv3x3_packed. Kept for bench.py's labels."""
    return True


def conv3x3_packed_supported(w_ohwi, H=None, W=None):
    """3x3 / stride 1 conv through the four-wave kernel with a pre-packed weight stream (csrc/conv3x3_fat.hip): 16-bit weights,
    Cin % 64 == 0 (>= 128), Cout % 256 == 0 -- or Cout == 128 (layer 2: packed as the lower half of a 256-channel tile) -- and, when
    given, maps made of whole 16 x 8 blocks."""
    return (w_ohwi.dtype == LP_DTYPE and w_ohwi.dim() == 4 and tuple(w_ohwi.shape[1:3]) == (3, 3) and w_ohwi.shape[3] % 64 == 0
            and w_ohwi.shape[3] >= 128 and (w_ohwi.shape[0] % 256 == 0 or w_ohwi.shape[0] == 128) and (H is None or (H % 16 == 0 and W % 8 == 0)))


def conv3x3_pack(w_ohwi):
    """OHWI 3x3 weights re-ordered once into per-wave MFMA fragment streams (agrl_conv3x3_pack) -> uint8 tensor."""
    assert conv3x3_packed_supported(w_ohwi)
    Cout, Cin = w_ohwi.shape[0], w_ohwi.shape[3]
    if Cout == 128:   # the lower half of one 256-channel tile; the upper half (zeros) is never read by the launch
        w_ohwi = torch.cat([w_ohwi, torch.zeros_like(w_ohwi)], dim=0)
        Cout = 256
    w_ohwi = w_ohwi.contiguous()
    nbytes = int(_hip.lib().agrl_conv3x3_packed_bytes(Cin, Cout))
    assert nbytes == 2 * w_ohwi.numel()
    packed = torch.empty((nbytes,), dtype=torch.uint8, device=w_ohwi.device)
    with _dev(w_ohwi):
        call("agrl_conv3x3_pack", ptr(w_ohwi), ptr(packed), Cin, Cout, _stream(w_ohwi))
    return packed


def conv3x3_packed(x, packed, bias, Cout, relu=True):
    """relu(conv3x3(x) + bias), stride 1 / pad 1, weights from conv3x3_pack. vmgn.py:52-54. -> (N,H,W,Cout) 16-bit NHWC."""
    N, H, W, Cin = x.shape
    assert x.dtype == LP_DTYPE and x.is_contiguous() and packed.numel() == 2 * 9 * Cin * max(Cout, 256)
    out = torch.empty((N, H, W, Cout), dtype=x.dtype, device=x.device)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * N * H * W * 9 * Cin * Cout, "bytes": 2.0 * (x.numel() + out.numel()) + 2.0 * 9 * Cin * Cout,
                            "conv": (3, 1, Cin, Cout, H, W)}
    with _dev(x):
        call("agrl_conv3x3_packed_bn_act", ptr(x), ptr(packed), ptr(bias), ptr(out), N, H, W, Cin, Cout, 1 if relu else 0, _stream(x))
    return out


def conv1x1_packed_supported(w):
    """1x1 / stride 1 conv through the four-wave kernel with a pre-packed weight stream (csrc/conv1x1_fat.hip): 16-bit weights
    (Cout, 1, 1, K) or (Cout, K) with K % 128 == 0 and Cout % 256 == 0."""
    w2 = w.reshape(w.shape[0], -1) if w.dim() == 4 and tuple(w.shape[1:3]) == (1, 1) else w
    return w2.dtype == LP_DTYPE and w2.dim() == 2 and w2.shape[1] % 128 == 0 and w2.shape[0] % 256 == 0


def conv1x1_pack(w):
    """(Cout, K) 16-bit weights (K = K1 + K2 for the two-source form: [W1 | W2]) re-ordered once into per-wave MFMA fragment
    streams (agrl_conv1x1_pack) -> uint8 tensor."""
    assert conv1x1_packed_supported(w)
    w = w.reshape(w.shape[0], -1).contiguous()
    Cout, K = w.shape
    nbytes = int(_hip.lib().agrl_conv1x1_packed_bytes(K, Cout))
    assert nbytes == 2 * w.numel()
    packed = torch.empty((nbytes,), dtype=torch.uint8, device=w.device)
    with _dev(w):
        call("agrl_conv1x1_pack", ptr(w), ptr(packed), K, Cout, _stream(w))
    return packed


def conv1x1_packed(x, packed, bias, Cout, relu=True, x2=None, duo=False):
    """act([x | x2] @ W^T + bias) over pixel rows, weights from conv1x1_pack. vmgn.py:48-50 (conv1), :56-64 with x2 (conv3 +
    downsample conv of a first block as one GEMM: x = the block input, x2 = conv2's output). -> (N,H,W,Cout) 16-bit NHWC."""
    N, H, W, K1 = x.shape
    K2 = 0 if x2 is None else x2.shape[3]
    M = N * H * W
    assert x.dtype == LP_DTYPE and x.is_contiguous() and packed.numel() == 2 * (K1 + K2) * Cout
    assert x2 is None or (x2.dtype == x.dtype and x2.is_contiguous() and tuple(x2.shape[:3]) == (N, H, W))
    out = torch.empty((N, H, W, Cout), dtype=x.dtype, device=x.device)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * M * (K1 + K2) * Cout,
                            "bytes": 2.0 * (x.numel() + (0 if x2 is None else x2.numel()) + out.numel()) + packed.numel(),
                            "conv": (1, 1, K1 + K2, Cout, H, W)}
    with _dev(x):
        if duo and x2 is not None:   # the two-workgroups-per-CU kernel (csrc/conv1x1_duo.hip), same packed weights, bit-identical
            call("agrl_conv1x1_packed_dual_duo", ptr(x), ptr(x2), ptr(packed), ptr(bias), ptr(out), M, K1, K2, Cout, 1 if relu else 0, _stream(x))
        else:
            call("agrl_conv1x1_packed_bn_act", ptr(x), ptr(x2), ptr(packed), ptr(bias), ptr(out), M, K1, K2, Cout, 1 if relu else 0, _stream(x))
    return out


def conv1x1_packed_dual_strided(x, x2, packed, bias, Cout, stride, relu=True):
    """relu(W3 x2 + b3 + Wds x[:, ::stride, ::stride] + bds) of the FIRST block of a strided layer (vmgn.py:56-64 with a stride-2
    downsample conv) as one GEMM over [x sampled | x2]: x (N,Hi,Wi,K1) the block input, x2 (N,Ho,Wo,K2) conv2's output, packed =
    conv1x1_pack([Wds | W3]), bias = bds + b3. The (N,Ho,Wo,Cout) shortcut map never exists. -> (N,Ho,Wo,Cout) 16-bit NHWC."""
    N, Hi, Wi, K1 = x.shape
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    K2 = x2.shape[3]
    assert x.dtype == LP_DTYPE and x2.dtype == LP_DTYPE and x.is_contiguous() and x2.is_contiguous()
    assert tuple(x2.shape[:3]) == (N, Ho, Wo) and packed.numel() == 2 * (K1 + K2) * Cout
    out = torch.empty((N, Ho, Wo, Cout), dtype=x.dtype, device=x.device)
    M = N * Ho * Wo
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * M * (K1 + K2) * Cout, "bytes": 2.0 * (M * K1 + x2.numel() + out.numel()) + packed.numel(),
                            "conv": (1, 1, K1 + K2, Cout, Ho, Wo)}
    with _dev(x):
        call("agrl_conv1x1_packed_dual_strided", ptr(x), ptr(x2), ptr(packed), ptr(bias), ptr(out), N, Hi, Wi, stride, K1, K2, Cout,
             1 if relu else 0, _stream(x))
    return out


def conv1x1_packed_res(x, packed, bias, Cout, residual, relu=True):
    """act(x @ W^T + bias + residual) over pixel rows, weights from conv1x1_pack: conv3 / bn3 + identity shortcut + ReLU of a
    Bottleneck (vmgn.py:56-64), or with ``residual=None`` a plain conv1 / bn1 / relu (vmgn.py:48-50), through the two-workgroups-per-CU kernel (csrc/conv1x1_duo.hip; layer 4's conv1s: 2048 -> 512 69 us against conv1x1_fat_kernel's 73 back to back; with a residual 115.6 against conv_bn_act's 122.4 us back to back, 117 / 119.5 inside a block). -> (N,H,W,Cout) 16-bit NHWC."""
    N, H, W, K = x.shape
    M = N * H * W
    assert x.dtype == LP_DTYPE and x.is_contiguous() and packed.numel() == 2 * K * Cout
    assert residual is None or (residual.dtype == x.dtype and residual.is_contiguous() and tuple(residual.shape) == (N, H, W, Cout))
    out = torch.empty((N, H, W, Cout), dtype=x.dtype, device=x.device)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * M * K * Cout,
                            "bytes": 2.0 * (x.numel() + out.numel() * (2 if residual is not None else 1)) + packed.numel(),
                            "conv": (1, 1, K, Cout, H, W)}
    with _dev(x):
        call("agrl_conv1x1_packed_res_bn_act", ptr(x), ptr(packed), ptr(bias), ptr(residual), ptr(out), M, K, Cout, 1 if relu else 0,
             _stream(x))
    return out


def conv1x1_packed_res_pool(x, packed, bias, Cout, residual, splits, mean, want_lp, relu=True):
    """conv1x1_bn_act_pool through the two-workgroups-per-CU kernel (csrc/conv1x1_duo.hip: 9 % ahead of igemm_wide_kernel's pooled form) with weights from conv1x1_pack: last conv of a layer-4 branch,
    16 x 8 frames, the 2048-channel map never written. -> pooled fp32 (F, P, Cout) [, 16-bit copy]. vmgn.py:56-64 + :298-308."""
    N, H, W, K = x.shape
    assert x.dtype == LP_DTYPE and x.is_contiguous() and (H, W) == (16, 8) and packed.numel() == 2 * K * Cout
    assert residual is None or (residual.dtype == x.dtype and residual.is_contiguous() and tuple(residual.shape) == (N, H, W, Cout))
    P = int(sum(splits))
    pooled = torch.empty((N, P, Cout), dtype=torch.float32, device=x.device)
    pooled_lp = torch.empty((N, P, Cout), dtype=LP_DTYPE, device=x.device) if want_lp else None
    arr = (C.c_int * len(splits))(*[int(s) for s in splits])
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * N * H * W * Cout * K,
                            "bytes": 2.0 * (x.numel() + (residual.numel() if residual is not None else 0)) + packed.numel() + 4.0 * pooled.numel()}
    with _dev(x):
        call("agrl_conv1x1_packed_res_pool", ptr(x), ptr(packed), ptr(bias), ptr(residual), ptr(pooled), ptr(pooled_lp),
             N, H, W, K, Cout, 1 if relu else 0, arr, len(splits), 1 if mean else 0, _stream(x))
    return pooled, pooled_lp


def bottleneck_tail_supported(y2, w3, w1_next, shortcut_conv=None):
    """The fused conv3(+residual) -> next conv1 kernel exists for the layer-1 and layer-2 shapes in bf16. ``shortcut_conv`` =
    (weight, stride) of the block's downsample conv when the residual is to be computed in the same pass."""
    if (y2.dtype == LP_DTYPE and tuple(w3.shape) == (512, 1, 1, 128) and tuple(w1_next.shape) == (128, 1, 1, 512)
            and shortcut_conv is None):
        return True  # layer-2 form (weights resident in registers)
    ok = (y2.dtype == LP_DTYPE and tuple(w3.shape) == (256, 1, 1, 64)
          and tuple(w1_next.shape) in ((64, 1, 1, 256), (128, 1, 1, 256)))
    if shortcut_conv is not None:
        ok = ok and tuple(shortcut_conv[0].shape) == (256, 1, 1, 64) and shortcut_conv[1] == 1 and w1_next.shape[0] == 64
    return ok


def bottleneck_tail(y2, w3, b3, residual, w1_next, b1_next, shortcut=None):
    """out = relu(conv3(y2) + R), z = relu(conv1_next(out)) in one pass (out never re-read from HBM); R = ``residual``
    or, with ``shortcut`` = (x, w_ds, b_ds), the block's 1x1 stride-1 downsample conv of x computed in the same pass.
    vmgn.py:57-64 (block i) + :48-50 (block i+1). -> out (N,H,W,256), z (N,H,W,64 | 128) bf16 NHWC."""
    N, H, W, Cmid = y2.shape
    Cout, Cnext = w3.shape[0], w1_next.shape[0]
    assert y2.dtype == LP_DTYPE and (residual is None) != (shortcut is None)
    xs = ws = bs = None
    Cshort = 0
    if shortcut is not None:
        xs, ws, bs = shortcut
        assert xs.shape[:3] == y2.shape[:3] and xs.dtype == y2.dtype
        Cshort = xs.shape[3]
    else:
        assert residual.shape == (N, H, W, Cout) and residual.dtype == y2.dtype
    out = torch.empty((N, H, W, Cout), dtype=y2.dtype, device=y2.device)
    z = torch.empty((N, H, W, Cnext), dtype=y2.dtype, device=y2.device)
    M = N * H * W
    if _hip.PROFILE is not None:
        rd = (residual.numel() if residual is not None else xs.numel() + ws.numel())
        _hip.PROFILE_TAG = {"flops": 2.0 * M * ((Cmid + Cshort) * Cout + Cout * Cnext),
                            "bytes": 2.0 * (y2.numel() + rd + out.numel() + z.numel() + w3.numel() + w1_next.numel())}
    with _dev(y2):
        call("agrl_bottleneck_tail", ptr(y2), ptr(w3), ptr(b3), ptr(residual), ptr(xs), ptr(ws), ptr(bs), ptr(out),
             ptr(w1_next), ptr(b1_next), ptr(z), M, Cmid, Cout, Cnext, Cshort, _stream(y2))
    return out, z


def bottleneck_block_supported(z, w2, stride, w3, w1_next, shortcut_conv=None):
    """The fused 3x3 -> conv3(+shortcut) -> next conv1 kernel exists for the layer-1 shapes in bf16 (stride-1 3x3,
    8 x 8-divisible maps). ``shortcut_conv`` as in bottleneck_tail_supported."""
    ok = (z.dtype == LP_DTYPE and stride == 1 and tuple(w2.shape) == (64, 3, 3, 64) and tuple(w3.shape) == (256, 1, 1, 64)
          and tuple(w1_next.shape) in ((64, 1, 1, 256), (128, 1, 1, 256)) and z.shape[1] % 8 == 0 and z.shape[2] % 8 == 0)
    if shortcut_conv is not None:
        ok = ok and tuple(shortcut_conv[0].shape) == (256, 1, 1, 64) and shortcut_conv[1] == 1 and w1_next.shape[0] == 64
    return ok


def bottleneck_block(z, w2, b2, w3, b3, residual, w1_next, b1_next, shortcut=None):
    """y2 = relu(conv3x3(z)), out = relu(conv3(y2) + R), z_next = relu(conv1_next(out)) in one pass: y2 never leaves the
    CU, out is written once. R = ``residual`` or, with ``shortcut`` = (x, w_ds, b_ds), the block's 1x1 stride-1
    downsample conv. vmgn.py:52-64 (block i) + :48-50 (block i+1). -> out (N,H,W,256), z_next (N,H,W,64 | 128)."""
    N, H, W, Cmid = z.shape
    Cout, Cnext = w3.shape[0], w1_next.shape[0]
    assert z.dtype == LP_DTYPE and (residual is None) != (shortcut is None)
    xs = ws = bs = None
    if shortcut is not None:
        xs, ws, bs = shortcut
        assert tuple(xs.shape) == (N, H, W, 64) and xs.dtype == z.dtype
    else:
        assert tuple(residual.shape) == (N, H, W, Cout) and residual.dtype == z.dtype
    out = torch.empty((N, H, W, Cout), dtype=z.dtype, device=z.device)
    zn = torch.empty((N, H, W, Cnext), dtype=z.dtype, device=z.device)
    M = N * H * W
    if _hip.PROFILE is not None:
        rd = residual.numel() if residual is not None else xs.numel() + ws.numel()
        _hip.PROFILE_TAG = {"flops": 2.0 * M * (9 * Cmid * Cmid + (Cmid + (64 if shortcut is not None else 0)) * Cout + Cout * Cnext),
                            "bytes": 2.0 * (z.numel() + rd + out.numel() + zn.numel() + w2.numel() + w3.numel() + w1_next.numel())}
    with _dev(z):
        call("agrl_bottleneck_block", ptr(z), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(residual), ptr(xs), ptr(ws), ptr(bs),
             ptr(out), ptr(w1_next), ptr(b1_next), ptr(zn), N, H, W, Cmid, Cout, Cnext, _stream(z))
    return out, zn


def linear_nobias(x, w):
    """(M,K) @ (N,K)^T -> fp32 (M,N). vmgn.py:148."""
    M, K = x.shape
    Nout, K2 = w.shape
    assert K == K2 and x.dtype == w.dtype
    y = torch.empty((M, Nout), dtype=torch.float32, device=x.device)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * M * K * Nout, "bytes": x.element_size() * (x.numel() + w.numel()) + 4 * y.numel()}
    with _dev(x):
        call("agrl_linear_nobias", ptr(x), ptr(w), ptr(y), M, K, Nout, _gemm_code(x.dtype), _stream(x))
    return y


def part_pool(x4_1, x4_2, splits, want_lp):
    """-> gsum (F,C), nodes (F,P,C) fp32 [, nodes_lp bf16]. vmgn.py:298-308."""
    F_, h, w, Cc = x4_1.shape
    assert x4_2.shape == x4_1.shape and x4_1.dtype == x4_2.dtype
    P = int(sum(splits))
    gsum = torch.empty((F_, Cc), dtype=torch.float32, device=x4_1.device)
    nodes = torch.empty((F_, P, Cc), dtype=torch.float32, device=x4_1.device)
    nodes_lp = torch.empty((F_, P, Cc), dtype=LP_DTYPE, device=x4_1.device) if want_lp else None
    arr = (C.c_int * len(splits))(*[int(s) for s in splits])
    with _dev(x4_1):
        call("agrl_part_pool", ptr(x4_1), ptr(x4_2), ptr(gsum), ptr(nodes), ptr(nodes_lp), F_, h, w, Cc, arr,
             len(splits), dtype_code(x4_1.dtype), _stream(x4_1))
    return gsum, nodes, nodes_lp


GRAM_CSLICE = 128

# The node counts V = parts x frames at which the GraphLayer's stages change kernel form (csrc/gcn.hip, csrc/train_tail.hip): up to
# each limit a tracklet's operands sit in one workgroup's LDS / registers, beyond it they are tiled or streamed from HBM.
GRAM_SLICE_MAX_V = 304          # agrl_graph_gram: a V x 128 fp32 slice (rows padded by 16 bytes, V rounded up to 16) in 160 KB
FINALIZE_RESIDENT_MAX_V = 256   # agrl_graph_finalize[_bits]: a row's columns in four registers per lane
PROPAGATE_TILED_MAX_V = 1024    # agrl_graph_propagate: 16 graph rows of V fp32 in 64 KB
BACKWARD_RESIDENT_MAX_V = 116   # agrl_graph_matrix_backward: three V x V fp32 images + V floats in 160 KB (its message says 115; 116 fits and ran)
PAIR_PRODUCT_MAX_V = 144        # agrl_graph_pair_product: two V x 128 fp32 slices in 160 KB


def graph_forms(V, C):
    """The kernel form each stage of a GraphLayer takes for V nodes of C channels (16-byte aligned tensors), mirrored from the
    dispatch of the entry points -> dict stage -> name:
      'gram'      'slices' (C / 128 partials, (B, C/128, V, V))          | 'tiled' (fully summed, (B, 1, V, V))
      'finalize'  'resident' (a row in registers)                       | 'rows' (two passes over the row in HBM)
      'propagate' 'stream' | 'mfma' | 'generic' | 'tiled'               | 'chunked' (16 graph rows through LDS in chunks)
      'backward'  'resident' (three V x V images in LDS)                 | 'hbm' (three passes, M as scratch)
      'pair'      'slices' (slice partials + their sum)                  | 'tiled' (no partials)
    The left-hand names are the forms every V had to fit before; each stage switches at its own limit above."""
    V, C = int(V), int(C)
    assert V >= 1 and C >= 1
    if V <= 64 and V % 4 == 0 and C % 128 == 0:
        prop = "stream"
    elif V <= 128 and C % 128 == 0:
        prop = "mfma"
    elif (V * ((V + 7) & ~7) + V * 128) * 4 <= 160 * 1024:
        prop = "generic"
    else:
        prop = "tiled" if V <= PROPAGATE_TILED_MAX_V else "chunked"
    return {"gram": "slices" if V <= GRAM_SLICE_MAX_V else "tiled",
            "finalize": "resident" if V <= FINALIZE_RESIDENT_MAX_V else "rows",
            "propagate": prop,
            "backward": "resident" if V <= BACKWARD_RESIDENT_MAX_V else "hbm",
            "pair": "slices" if V <= PAIR_PRODUCT_MAX_V else "tiled"}


def _gram_into(f):
    """The Gram of f (B,V,C) in the layout the consumers take, (B, nz, V, V): the C / 128 slice partials up to GRAM_SLICE_MAX_V
    nodes, the fully summed tiled form (nz = 1) beyond. Called inside ``_dev(f)``."""
    B, V, Cc = f.shape
    nz = Cc // GRAM_CSLICE if graph_forms(V, Cc)["gram"] == "slices" else 1
    gram = torch.empty((B, nz, V, V), dtype=torch.float32, device=f.device)
    call("agrl_graph_gram", ptr(f), ptr(gram), B, V, Cc, GRAM_CSLICE, _stream(f))
    return gram


def graph_matrix(f, adj, use_pose, learn_graph, mask_diag=False):
    """f (B,V,C) fp32, adj (B,V,V) fp32 -> G (B,V,V). vmgn.py:114-120, :155-166; ``mask_diag``: ganet.py:259-268."""
    B, V, Cc = f.shape
    G = torch.empty((B, V, V), dtype=torch.float32, device=f.device)
    gram = None
    nz = 0
    with _dev(f):
        if learn_graph:
            gram = _gram_into(f.contiguous())
            nz = gram.shape[1]
        if use_pose and adjacency_is_packed(adj):
            assert tuple(adj.shape) == (B, V, (V + 31) // 32)
            call("agrl_graph_finalize_bits", ptr(gram), nz, ptr(adj.contiguous()), ptr(G), B, V, 1, 1 if learn_graph else 0,
                 1 if mask_diag else 0, _stream(f))
            return G
        if use_pose:
            assert adj is not None and tuple(adj.shape) == (B, V, V) and adj.dtype == torch.float32
            adj = adj.contiguous()
        call("agrl_graph_finalize", ptr(gram), nz, ptr(adj) if use_pose else None, ptr(G), B, V,
             1 if use_pose else 0, 1 if learn_graph else 0, 1 if mask_diag else 0, _stream(f))
    return G


def adjacency_is_packed(adj):
    """The bit-packed adjacency is an int32 tensor (B, V, ceil(V/32)); the reference's form is fp32 (B, V, V)."""
    return adj is not None and adj.dtype == torch.int32


def adjacency_pack(adj):
    """fp32 {0,1} adjacency (B,V,V) on the device -> bit-packed int32 (B, V, ceil(V/32)): bit j & 31 of word j >> 5 of row i."""
    B, V, V2 = adj.shape
    assert V == V2 and adj.dtype == torch.float32
    bits = torch.empty((B, V, (V + 31) // 32), dtype=torch.int32, device=adj.device)
    with _dev(adj):
        call("agrl_adjacency_pack", ptr(adj.contiguous()), ptr(bits), B, V, _stream(adj))
    return bits


def adjacency_pack_host(adj):
    """The same packing on the HOST (numpy): what a loader does before the upload -- 448 bytes per 56-node tracklet cross PCIe
    instead of 12.5 KB. adj: CPU tensor / array (B,V,V) -> CPU int32 tensor (B, V, ceil(V/32))."""
    import numpy as np
    a = np.asarray(adj.detach().cpu() if hasattr(adj, "detach") else adj) != 0
    B, V, _ = a.shape
    W = (V + 31) // 32
    pad = np.zeros((B, V, W * 32), dtype=bool)
    pad[:, :, :V] = a
    words = (pad.reshape(B, V, W, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=3).astype(np.uint32)
    return torch.from_numpy(words.view(np.int32).copy())


def graph_propagate(f, h, G, bn_scale, bn_shift, gamma, slope, want_lp, keep=None):
    """out = keep f + gamma lrelu(bn(G h)); keep defaults to the reference's Python-float (1 - gamma). vmgn.py:168-172;
    ganet.py:278-283 passes keep = 1."""
    if keep is None:
        keep = 1.0 - float(gamma)
    B, V, Cc = f.shape
    out = torch.empty_like(f)
    out_lp = torch.empty((B, V, Cc), dtype=LP_DTYPE, device=f.device) if want_lp else None
    if _hip.PROFILE is not None:  # read f + read h + read G(adj-sized) + write out
        _hip.PROFILE_TAG = {"flops": 2.0 * B * V * V * Cc, "bytes": 4.0 * (3 * B * V * Cc + B * V * V)}
    with _dev(f):
        call("agrl_graph_propagate", ptr(f), ptr(h), ptr(G), ptr(bn_scale), ptr(bn_shift), float(keep), float(gamma),
             float(slope), ptr(out), ptr(out_lp), B, V, Cc, _stream(f))
    return out, out_lp


def graph_apply_presplit_supported(f):
    B, V, Cc = f.shape
    return V <= 64 and V % 4 == 0 and Cc % 128 == 0


def graph_apply_operand(G, f, out_dtype, presplit=False):
    """P = G f, (B,V,V) x (B,V,C) fp32 -> (B,V,C) in ``out_dtype`` (fp32 / bf16): the message pass applied to the layer INPUT,
    written once as the operand of ``graph_linear_mix``. vmgn.py:168 with the Linear commuted behind it. ``presplit`` ('fp16x3'): the
    fp32-sized rows hold the fp16 halves the GEMM's k-loop would form (graph_linear_mix(..., p_presplit=True))."""
    B, V, Cc = f.shape
    assert f.dtype == torch.float32 and G.dtype == torch.float32 and tuple(G.shape) == (B, V, V)
    assert not presplit or (out_dtype == torch.float32 and graph_apply_presplit_supported(f))
    if V <= 64 and V % 4 == 0 and Cc % 128 == 0:
        out = torch.empty((B, V, Cc), dtype=out_dtype, device=f.device)
        if _hip.PROFILE is not None:
            _hip.PROFILE_TAG = {"flops": 2.0 * B * V * V * Cc, "bytes": 4.0 * (B * V * Cc + B * V * V) + out.element_size() * B * V * Cc}
        with _dev(f):
            call("agrl_graph_apply", ptr(G.contiguous()), ptr(f.contiguous()), ptr(out), _hip.F32H3P if presplit else dtype_code(out_dtype), B, V, Cc,
                 _stream(f))
        return out
    # other node counts (V > 64: seq_len 16; V % 4 != 0): the general message-pass kernels with a unit BatchNorm
    key = (f.device, Cc)
    if key not in _UNIT:
        _UNIT[key] = (torch.ones((Cc,), dtype=torch.float32, device=f.device), torch.zeros((Cc,), dtype=torch.float32, device=f.device))
    one, zero = _UNIT[key]
    out, out_lp = graph_propagate(f, f, G, one, zero, 1.0, 1.0, want_lp=out_dtype == LP_DTYPE, keep=0.0)
    return out_lp if out_dtype == LP_DTYPE else out


TRACKLET_FORM_MIN_B = 224


def graph_tracklet_operand_supported(f):
    """One workgroup per tracklet needs enough tracklets to fill the chip (B >= 224: measured 90 us against 119 us for the three launches at 256 tracklets, slower below ~190) and the streaming shapes."""
    B, V, Cc = f.shape
    return B >= TRACKLET_FORM_MIN_B and V <= 64 and V % 4 == 0 and Cc % 512 == 0


def graph_tracklet_operand(f, adj, use_pose, learn_graph, out_dtype, want_graph=False, mask_diag=False):
    """graph_matrix + graph_apply_operand in one launch, one workgroup per tracklet: -> P = G f (B,V,C) in ``out_dtype``, G (B,V,V) or
    None. vmgn.py:114-120, :155-168."""
    B, V, Cc = f.shape
    assert f.dtype == torch.float32
    P = torch.empty((B, V, Cc), dtype=out_dtype, device=f.device)
    G = torch.empty((B, V, V), dtype=torch.float32, device=f.device) if want_graph else None
    packed = use_pose and adjacency_is_packed(adj)
    if use_pose:
        assert adj is not None and (tuple(adj.shape) == (B, V, (V + 31) // 32) if packed else (tuple(adj.shape) == (B, V, V) and adj.dtype == torch.float32))
        adj = adj.contiguous()
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 4.0 * B * V * V * Cc, "bytes": 4.0 * (B * V * Cc + B * V * V) + P.element_size() * B * V * Cc}
    with _dev(f):
        call("agrl_graph_tracklet_operand", ptr(f.contiguous()), ptr(adj) if use_pose else None, 1 if packed else 0, ptr(G), ptr(P),
             dtype_code(out_dtype), B, V, Cc, 1 if use_pose else 0, 1 if learn_graph else 0, 1 if mask_diag else 0, _stream(f))
    return P, G


def graph_linear_mix(p_op, w, f, bn_scale, bn_shift, gamma, slope, keep=None, p_presplit=False):
    """out = keep f + gamma lrelu(bn((G f) W^T)): the Linear of a GraphLayer as ONE GEMM over P = G f with BatchNorm1d, LeakyReLU
    and the residual mix in its epilogue (vmgn.py:148, :168-172). p_op (B,V,K) fp32 / bf16, w (N,K) same dtype, f (B,V,N) fp32."""
    if keep is None:
        keep = 1.0 - float(gamma)
    B, V, K = p_op.shape
    Nout = w.shape[0]
    assert w.shape[1] == K and p_op.dtype == w.dtype and f.dtype == torch.float32 and tuple(f.shape) == (B, V, Nout)
    out = torch.empty_like(f)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * B * V * K * Nout, "bytes": p_op.element_size() * (p_op.numel() + w.numel()) + 8.0 * f.numel()}
    code = _gemm_code(p_op.dtype)
    unscale = getattr(w, 'agrl_unscale', None)
    if unscale is not None:   # 'fp16x3': w pre-scaled by a power of two and pre-split (split16_inloop_weights); bn_scale must already carry the 2^-k
        assert p_op.dtype == torch.float32 and getattr(bn_scale, 'agrl_folded_unscale', None) == unscale and getattr(w, 'agrl_presplit', False)
        code = _hip.F32H3P if p_presplit else _hip.F32H3
    else:
        assert not p_presplit
    with _dev(f):
        call("agrl_graph_linear_mix", ptr(p_op.contiguous()), ptr(w), ptr(f.contiguous()), ptr(bn_scale), ptr(bn_shift), float(keep), float(gamma),
             float(slope), ptr(out), B * V, K, Nout, code, _stream(f))
    return out


def pam_pool(x, qk, splits):
    """ganet's position-attention part nodes, first half: x (F,h,w,C) NHWC, qk (F,h,w,2*Cq) NHWC stacked query / key conv
    output (None when the module's gamma is 0) -> xbar (F,P,C) fp32 (None without qk), xmean (F,P,C) fp32. ganet.py:98-136,
    :384-400."""
    F_, h, w, Cc = x.shape
    P = int(sum(splits))
    xmean = torch.empty((F_, P, Cc), dtype=torch.float32, device=x.device)
    xbar = None
    Cq = 0
    if qk is not None:
        assert qk.dtype == x.dtype and tuple(qk.shape[:3]) == (F_, h, w) and qk.shape[3] % 2 == 0
        Cq = qk.shape[3] // 2
        xbar = torch.empty((F_, P, Cc), dtype=torch.float32, device=x.device)
    arr = (C.c_int * len(splits))(*[int(s) for s in splits])
    with _dev(x):
        call("agrl_pam_pool", ptr(x), ptr(qk), ptr(xbar), ptr(xmean), F_, h, w, Cc, Cq, arr, len(splits), dtype_code(x.dtype),
             _stream(x))
    return xbar, xmean


def pam_combine(y, bv, xmean, gamma, want_lp):
    """nodes = gamma (y + bv) + 2 xmean (y = Wv xbar), ganet.py:394-399 -> nodes fp32 like xmean [, bf16 copy]."""
    nodes = torch.empty_like(xmean)
    nodes_lp = torch.empty(xmean.shape, dtype=LP_DTYPE, device=xmean.device) if want_lp else None
    rows, Cc = xmean.numel() // xmean.shape[-1], xmean.shape[-1]
    with _dev(xmean):
        call("agrl_pam_combine", ptr(y), ptr(bv), ptr(xmean), float(gamma), ptr(nodes), ptr(nodes_lp), rows, Cc, _stream(xmean))
    return nodes, nodes_lp


PAM_MAXL = 128   # positions a pyramid slice may hold (csrc/pam.hip); also the row length of abar


def pam_slices(splits, h):
    """[(first row, end row)] of the pyramid slices in part order: h // n rows each, remainder rows dropped (ganet.py:387-390)."""
    return [((h // int(n)) * j, (h // int(n)) * (j + 1)) for n in splits for j in range(int(n))]


def pam_pool_train(x, qk, splits):
    """pam_pool under train(): x (F,h,w,C), qk (F,h,w,2*Cq) fp32 -> xbar, xmean (F,P,C), abar (F,P,128; zero beyond a slice's
    positions). Always the attention branch: d loss / d gamma is not zero at gamma == 0."""
    F_, h, w, Cc = x.shape
    assert tuple(qk.shape[:3]) == (F_, h, w) and qk.shape[3] % 2 == 0
    P = int(sum(splits))
    xbar = torch.empty((F_, P, Cc), dtype=torch.float32, device=x.device)
    xmean = torch.empty((F_, P, Cc), dtype=torch.float32, device=x.device)
    abar = torch.empty((F_, P, PAM_MAXL), dtype=torch.float32, device=x.device)
    arr = (C.c_int * len(splits))(*[int(s) for s in splits])
    with _dev(x):
        call("agrl_pam_pool_train", ptr(x), ptr(qk), ptr(xbar), ptr(xmean), ptr(abar), F_, h, w, Cc, qk.shape[3] // 2, arr, len(splits),
             dtype_code(x.dtype), _stream(x))
    return xbar, xmean, abar


def pam_pool_backward(x, qk, dxbar, dxmean, splits, want_abar=False):
    """Backward of pam_pool_train: dxbar, dxmean (F,P,C) (dxmean = 2 dnode; the 1 / L is the kernel's) -> dx (F,h,w,C),
    dqk (F,h,w,2*Cq) [, abar (F,P,128) as recomputed on the way]. Formulas: pam_nodes_backward_reference."""
    F_, h, w, Cc = x.shape
    P = int(sum(splits))
    assert tuple(dxbar.shape) == tuple(dxmean.shape) == (F_, P, Cc) and tuple(qk.shape[:3]) == (F_, h, w)
    dx = torch.empty_like(x)
    dqk = torch.empty_like(qk)
    abar = torch.empty((F_, P, PAM_MAXL), dtype=torch.float32, device=x.device)
    arr = (C.c_int * len(splits))(*[int(s) for s in splits])
    with _dev(x):
        call("agrl_pam_pool_backward", ptr(x), ptr(qk), ptr(dxbar), ptr(dxmean), ptr(dx), ptr(dqk), ptr(abar), F_, h, w, Cc, qk.shape[3] // 2,
             arr, len(splits), dtype_code(x.dtype), _stream(x))
    return (dx, dqk, abar) if want_abar else (dx, dqk)


def pam_combine_train(y, bv, xmean, gamma):
    """nodes = gamma (y + bv) + 2 xmean with gamma a device tensor (1,) -- the nn.Parameter, never read by the host."""
    nodes = torch.empty_like(xmean)
    rows, Cc = xmean.numel() // xmean.shape[-1], xmean.shape[-1]
    with _dev(xmean):
        call("agrl_pam_combine_train", ptr(y), ptr(bv), ptr(xmean), ptr(gamma), ptr(nodes), rows, Cc, _stream(xmean))
    return nodes


def col_sum_plan(M):
    """(row chunks, rows per chunk) of agrl_col_sum / agrl_pam_combine_backward for M rows (csrc/pam.hip: pam_row_chunks)."""
    chunks = min(64, max(1, M // 32))
    return chunks, -(-M // chunks)


def _col_sum_ws(M, Cc, device):
    nbytes = int(_hip.lib().agrl_col_sum_workspace(int(M), int(Cc)))
    return torch.empty((nbytes // 4,), dtype=torch.float32, device=device), nbytes


def pam_combine_backward(dnodes, y, bv, gamma):
    """dnodes, y (rows..,C), bv (C), gamma (1,) device -> dy = gamma dnodes, dxmean = 2 dnodes, dgamma (1,), dbv (C)."""
    Cc = dnodes.shape[-1]
    rows = dnodes.numel() // Cc
    dy, dxmean = torch.empty_like(dnodes), torch.empty_like(dnodes)
    dgamma = torch.empty((1,), dtype=torch.float32, device=dnodes.device)
    dbv = torch.empty((Cc,), dtype=torch.float32, device=dnodes.device)
    ws, nbytes = _col_sum_ws(rows, Cc, dnodes.device)
    with _dev(dnodes):
        call("agrl_pam_combine_backward", ptr(dnodes), ptr(y), ptr(bv), ptr(gamma), ptr(dy), ptr(dxmean), ptr(dgamma), ptr(dbv), rows, Cc,
             ptr(ws), nbytes, _stream(dnodes))
    return dy, dxmean, dgamma, dbv


def col_sum(x2d):
    """(M,C) fp32 -> (C): column sums in a fixed order (the bias gradient of the stacked query / key conv)."""
    M, Cc = x2d.shape
    assert x2d.dtype == torch.float32
    out = torch.empty((Cc,), dtype=torch.float32, device=x2d.device)
    ws, nbytes = _col_sum_ws(M, Cc, x2d.device)
    with _dev(x2d):
        call("agrl_col_sum", ptr(x2d), ptr(out), M, Cc, ptr(ws), nbytes, _stream(x2d))
    return out


def pam_nodes_backward_reference(x, wq, bq, wk, bk, wv, bv, gamma, splits, dnodes):
    """ganet's position-attention part nodes and their gradient by the folded algebra the kernels use (csrc/pam.hip, include/
    agrl_hip.h), in plain torch on the tensors' own device and dtype (float64 in the tests): the value conv is never evaluated per
    position. x (F,h,w,C) NHWC map, wq / wk (Cq,C), bq / bk (Cq), wv (C,C), bv (C), gamma scalar tensor, dnodes (F,P,C).
    Per slice (L positions, X its (L,C) rows):
        A = softmax_rows(Q K^T), abar = mean_p A[p], xbar = X^T abar, xmean = mean_q X[q], node = gamma (Wv xbar + bv) + 2 xmean
        dgamma += dnode . (Wv xbar + bv), dbv += gamma dnode, dy = gamma dnode, dWv += dy xbar^T, dxbar = Wv^T dy
        dX += abar dxbar^T + (2 / L) 1 dnode^T, dabar = X dxbar, g = A dabar, dE = A (dabar[q] - g[p]) / L
        dQ = dE K, dK = dE^T Q, dWq += dQ^T X, dbq += sum_p dQ, dWk += dK^T X, dbk += sum_q dK (identically 0), dX += dQ Wq + dK Wk
    -> dict: nodes, xbar, xmean (F,P,C), abar (list per part of (F,L)), dx, dxbar (F,P,C), dqk (F,h,w,2*Cq; query first, before the
    conv's own data gradient), dwq, dbq, dwk, dbk, dwv, dbv, dgamma."""
    F_, h, w, Cc = x.shape
    Cq = wq.shape[0]
    g = gamma.reshape(())
    q_map = x @ wq.t() + bq
    k_map = x @ wk.t() + bk
    slices = pam_slices(splits, h)
    nodes, xbars, xmeans, abars = [], [], [], []
    dx_pool = torch.zeros_like(x)                                    # through xbar / xmean only
    dqk = x.new_zeros((F_, h, w, 2 * Cq))
    dxbars = []
    dwv, dbv_, dgamma = torch.zeros_like(wv), torch.zeros_like(bv), g.new_zeros(())
    for part, (r0, r1) in enumerate(slices):
        L = (r1 - r0) * w
        X = x[:, r0:r1].reshape(F_, L, Cc)
        Q, K = q_map[:, r0:r1].reshape(F_, L, Cq), k_map[:, r0:r1].reshape(F_, L, Cq)
        A = torch.softmax(Q @ K.transpose(1, 2), dim=2)
        abar = A.mean(dim=1)                                         # (F, L)
        xbar = torch.einsum('fq,fqc->fc', abar, X)
        xmean = X.mean(dim=1)
        yb = xbar @ wv.t() + bv
        nodes.append(g * yb + 2 * xmean)
        xbars.append(xbar), xmeans.append(xmean), abars.append(abar)
        dn = dnodes[:, part]
        dgamma = dgamma + (dn * yb).sum()
        dbv_ = dbv_ + g * dn.sum(0)
        dy = g * dn
        dwv = dwv + dy.t() @ xbar
        dxbar = dy @ wv
        dxbars.append(dxbar)
        dX = abar.unsqueeze(2) * dxbar.unsqueeze(1) + (2.0 / L) * dn.unsqueeze(1)
        dabar = torch.einsum('fqc,fc->fq', X, dxbar)
        gp = torch.einsum('fpq,fq->fp', A, dabar)
        dE = A * (dabar.unsqueeze(1) - gp.unsqueeze(2)) / L
        dQ, dK = dE @ K, dE.transpose(1, 2) @ Q
        dx_pool[:, r0:r1] += dX.reshape(F_, r1 - r0, w, Cc)
        dqk[:, r0:r1, :, :Cq] += dQ.reshape(F_, r1 - r0, w, Cq)
        dqk[:, r0:r1, :, Cq:] += dK.reshape(F_, r1 - r0, w, Cq)
    dq2, dk2, x2 = dqk[..., :Cq].reshape(-1, Cq), dqk[..., Cq:].reshape(-1, Cq), x.reshape(-1, Cc)
    return {'nodes': torch.stack(nodes, 1), 'xbar': torch.stack(xbars, 1), 'xmean': torch.stack(xmeans, 1), 'abar': abars,
            'dxbar': torch.stack(dxbars, 1), 'dx_pool': dx_pool, 'dqk': dqk,
            'dx': dx_pool + (dq2 @ wq + dk2 @ wk).reshape(x.shape),
            'dwq': dq2.t() @ x2, 'dbq': dq2.sum(0), 'dwk': dk2.t() @ x2, 'dbk': dk2.sum(0),
            'dwv': dwv, 'dbv': dbv_, 'dgamma': dgamma}


def clip_pool(feats, num_clips, mode="avg"):
    """(T*num_clips, D) fp32 -> (T, D): mean / max over each tracklet's clips. train_vidreid_xent_htri.py:471-476."""
    assert feats.dtype == torch.float32 and feats.dim() == 2 and feats.size(0) % num_clips == 0 and mode in ("avg", "max")
    feats = feats.contiguous()
    T, D = feats.size(0) // num_clips, feats.size(1)
    out = torch.empty((T, D), dtype=torch.float32, device=feats.device)
    with _dev(feats):
        call("agrl_clip_pool", ptr(feats), ptr(out), T, num_clips, D, 0 if mode == "avg" else 1, _stream(feats))
    return out


def ragged_offsets(offsets, rows):
    """Validate the segment offsets of ``clip_pool_ragged`` against ``rows`` feature rows -> contiguous int32 ndarray (T+1,): a HOST
    integer vector, strictly increasing, 0 <= offsets[0], offsets[T] <= rows. ValueError otherwise (a device tensor included)."""
    if isinstance(offsets, torch.Tensor):
        if offsets.is_cuda:
            raise ValueError("clip_pool_ragged: offsets is a host array (it is validated before the upload)")
        offsets = offsets.numpy()
    o = np.asarray(offsets)
    if o.ndim != 1 or o.size < 2 or o.dtype.kind not in "iu":
        raise ValueError("clip_pool_ragged: offsets is an integer vector of T + 1 >= 2 entries, got %s %s" % (o.dtype, o.shape))
    o = o.astype(np.int64)
    if o[0] < 0 or o[-1] > rows or not bool((np.diff(o) > 0).all()):
        raise ValueError("clip_pool_ragged: offsets must be strictly increasing within [0, %d], got %s%s" % (
            rows, o[:8].tolist(), " ..." if o.size > 8 else ""))
    return np.ascontiguousarray(o, dtype=np.int32)


def clip_pool_ragged(feats, offsets, mode="avg", nonfinite=None):
    """(N, D) fp32 clip embeddings + HOST offsets (T+1,) -> (T, D): mean / max over rows offsets[t] .. offsets[t+1]-1, every segment
    bit-identical to ``clip_pool`` on it alone (agrl_clip_pool_ragged). ``offsets`` is validated here (``ragged_offsets``) and
    uploaded non-blocking. ``nonfinite``: None or an int32 [1] tensor on the device, set to 1 when a value read is inf / NaN and never
    cleared. One launch, no synchronisation."""
    if not isinstance(feats, torch.Tensor) or feats.dtype != torch.float32 or feats.dim() != 2 or not feats.is_cuda:
        raise ValueError("clip_pool_ragged: feats are fp32 (N, D) on the GPU")
    if mode not in ("avg", "max"):
        raise ValueError("clip_pool_ragged: mode is 'avg' or 'max', got %r" % (mode,))
    N, D = feats.shape
    off = ragged_offsets(offsets, N)
    if D < 1:
        raise ValueError("clip_pool_ragged: D = 0")
    if nonfinite is not None and (nonfinite.dtype != torch.int32 or nonfinite.numel() != 1 or nonfinite.device != feats.device):
        raise ValueError("clip_pool_ragged: nonfinite is an int32 [1] tensor on %s" % (feats.device,))
    feats = feats.contiguous()
    T = off.size - 1
    out = torch.empty((T, D), dtype=torch.float32, device=feats.device)
    off_d = torch.from_numpy(off).pin_memory().to(feats.device, non_blocking=True)
    with _dev(feats):
        call("agrl_clip_pool_ragged", ptr(feats), ptr(off_d), ptr(out), ptr(nonfinite), N, T, D, 0 if mode == "avg" else 1, _stream(feats))
    if nonfinite is not None:
        written(nonfinite)
    return out


def row_sqnorm(x):
    R, Cc = x.shape
    out = torch.empty((R,), dtype=torch.float32, device=x.device)
    with _dev(x):
        call("agrl_row_sqnorm", ptr(x), ptr(out), R, Cc, dtype_code(x.dtype), _stream(x))
    return out


def attn_pool_bnneck(nodes, sqn, gsum, g_scale, g_shift, a_scale, a_shift, B, S, P, hw, want_feats=False):
    """-> out (B,2C) [, g_f, att_f (B,C)]. vmgn.py:270-278, :299-301, :313-321."""
    Cc = nodes.shape[-1]
    out = torch.empty((B, 2 * Cc), dtype=torch.float32, device=nodes.device)
    g_f = torch.empty((B, Cc), dtype=torch.float32, device=nodes.device) if want_feats else None
    att_f = torch.empty((B, Cc), dtype=torch.float32, device=nodes.device) if want_feats else None
    with _dev(nodes):
        call("agrl_attn_pool_bnneck", ptr(nodes), ptr(sqn), ptr(gsum), ptr(g_scale), ptr(g_shift), ptr(a_scale),
             ptr(a_shift), ptr(out), ptr(g_f), ptr(att_f), B, S, P, Cc, hw, _stream(nodes))
    if want_feats:
        return out, g_f, att_f
    return out


def attn_tail_supported(S, P, Cc, B=None):
    """The one-launch tail (agrl_attn_tail): C % 4 == 0 and S * P + 2 C floats within 64 KB of LDS. With ``B`` given: also whether the
    model should TAKE it -- one workgroup per tracklet fills the chip only from ~224 tracklets per GPU (measured, tools/
    attn_tail_bench.py, one launch / three launches: 37.6 / 35.7 us at 32 tracklets, 43.6 / 40.2 at 128, 53.7 / 58.2 at 256);
    AGRL_HIP_FUSE_ATTN_TAIL=1 / 0 forces it on / off."""
    ok = Cc % 4 == 0 and (((S * P + 3) & ~3) + 2 * Cc + 4) * 4 <= 64 * 1024
    if B is None or not ok:
        return ok
    force = switch('AGRL_HIP_FUSE_ATTN_TAIL', '')
    if force != '':
        return force != '0'
    return B >= int(switch('AGRL_HIP_ATTN_TAIL_MIN_B', '224'))


def attn_tail(nodes, gsum, g_scale, g_shift, a_scale, a_shift, B, S, P, hw, want_feats=False, query_dtype=None, want_node_sqn=False):
    """row_sqnorm(nodes) + attn_pool_bnneck + the distance matrix's query operand in ONE launch (bit-identical to the separate
    calls). -> out (B,2C), feats (g_f, att_f) or None, query dict or None: {'sqn': ||out||^2 (B,), 'normalized': out / ||out||
    in ``query_dtype`` (LP_DTYPE or torch.float32)}, node_sqn (B*S*P,) or None. vmgn.py:270-278, :313-321; distance.py:70-71, :86-87."""
    Cc = nodes.shape[-1]
    dev = nodes.device
    out = torch.empty((B, 2 * Cc), dtype=torch.float32, device=dev)
    g_f = torch.empty((B, Cc), dtype=torch.float32, device=dev) if want_feats else None
    att_f = torch.empty((B, Cc), dtype=torch.float32, device=dev) if want_feats else None
    node_sqn = torch.empty((B * S * P,), dtype=torch.float32, device=dev) if want_node_sqn else None
    q_lp = q_f32 = out_sqn = None
    if query_dtype is not None:
        out_sqn = torch.empty((B,), dtype=torch.float32, device=dev)
        if query_dtype == LP_DTYPE:
            q_lp = torch.empty((B, 2 * Cc), dtype=LP_DTYPE, device=dev)
        else:
            q_f32 = torch.empty((B, 2 * Cc), dtype=torch.float32, device=dev)
    with _dev(nodes):
        call("agrl_attn_tail", ptr(nodes), ptr(gsum), ptr(g_scale), ptr(g_shift), ptr(a_scale), ptr(a_shift), ptr(out), ptr(g_f),
             ptr(att_f), ptr(node_sqn), ptr(out_sqn), ptr(q_lp), ptr(q_f32), B, S, P, Cc, hw, _stream(nodes))
    query = None if query_dtype is None else {'sqn': out_sqn, 'normalized': q_lp if q_lp is not None else q_f32}
    return out, ((g_f, att_f) if want_feats else None), query, node_sqn


class QueryOperandCache:
    """What agrl_attn_tail left beside an embedding batch: its rows' squared norms and L2-normalised copy in the distance matrix's
    operand type. ``lookup(emb, dtype)`` answers only for THE tensor object the forward returned -- identity through a weak
    reference, not its address: once that tensor is freed the caching allocator may hand the same address to another (B, D) fp32
    tensor whose ``_version`` is 0 as well (raw kernels never bump it), and an address-keyed cache would then serve the previous
    batch's rows. The version is still compared so that an in-place edit of the live tensor misses."""

    def __init__(self, emb, query):
        self.ref = weakref.ref(emb)
        self.version = emb._version
        self.query = query

    def lookup(self, emb, dtype):
        if self.ref() is not emb or self.version != emb._version or self.query['normalized'].dtype != dtype:
            return None
        return self.query


def query_operands(model, emb, metric, dtype):
    """The query side of hip_distmat for one batch of embeddings ``emb`` (B,D) fp32 -> (operand, sq-norms or None): the cosine
    operand / the euclidean norms straight from the tail kernel when ``emb`` is the tensor ``model`` just returned (no extra
    launch), else agrl_row_l2_normalize / agrl_row_sqnorm. distance.py:59-89."""
    cache = getattr(model, '_hip_query', None)
    q = cache.lookup(emb, dtype) if cache is not None else None
    if metric == 'cosine':
        return (q['normalized'] if q is not None else row_l2_normalize(emb, True, dtype)), None
    qn = q['sqn'] if q is not None else row_sqnorm(emb)
    return (row_l2_normalize(emb, False, dtype) if dtype != torch.float32 else emb), qn


def k_multiple(dtype):
    """K granularity of the GEMM kernel: one 128-byte k-tile."""
    return 64 if dtype == LP_DTYPE else 32


def row_l2_normalize(x, normalize, out_dtype, pad_to=1):
    """fp32 (R,C) -> (R, Cpad) out_dtype, Cpad = C rounded up to ``pad_to``, padding columns zero."""
    R, Cc = x.shape
    assert x.dtype == torch.float32
    ld = -(-Cc // pad_to) * pad_to
    y = torch.empty((R, ld), dtype=out_dtype, device=x.device)
    with _dev(x):
        call("agrl_row_l2_normalize", ptr(x), ptr(y), R, Cc, ld, 1 if normalize else 0, dtype_code(out_dtype),
             _stream(x))
    return y


def distmat(q, g, metric, qn=None, gn=None, out=None):
    """q (m,D), g (n,D) prepared operands (see metrics.distance) -> fp32 (m,n). distance.py:59-89."""
    m, D = q.shape
    n, D2 = g.shape
    assert D == D2 and q.dtype == g.dtype
    handed = out is not None
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=q.device)
    assert out.stride(1) == 1 and out.dtype == torch.float32
    code = METRIC_EUCLIDEAN if metric == "euclidean" else METRIC_COSINE
    if _hip.PROFILE is not None:  # (m+n)*D*e + m*n*4
        _hip.PROFILE_TAG = {"flops": 2.0 * m * n * D, "bytes": q.element_size() * (m + n) * D + 4.0 * m * n}
    ws = None
    # few output tiles (one eval batch against a long gallery, or the gathered queries of an 8-GPU step against a gallery
    # shard): hand the kernel scratch for split-K partials; the m <= 64 streaming kernels ignore it
    if (-(-m // 64)) * (-(-n // 128)) < 256:
        ws = torch.empty((8 * m * n,), dtype=torch.float32, device=q.device)
    with _dev(q):
        _hip.call("agrl_distmat", ptr(q), ptr(g), ptr(qn), ptr(gn), out.data_ptr(), m, n, D, out.stride(0), code,
                  dtype_code(q.dtype), ptr(ws), 0 if ws is None else ws.numel() * 4, _stream(q))
    if handed:
        written(out)
    return out


def rank_topk(dist, k, idx_offset=0):
    """dist (m,n) fp32 -> idx int32 (m,k), val fp32 (m,k), ascending (distance, index). rank.py:170-172."""
    m, n = dist.shape
    assert dist.dtype == torch.float32 and dist.stride(1) == 1
    idx = torch.empty((m, k), dtype=torch.int32, device=dist.device)
    val = torch.empty((m, k), dtype=torch.float32, device=dist.device)
    with _dev(dist):
        _hip.call("agrl_rank_topk", dist.data_ptr(), m, n, dist.stride(0), k, idx_offset, ptr(idx), ptr(val),
                  _stream(dist))
    return idx, val


def distmat_topk(q, g, metric, k, qn=None, gn=None, idx_offset=0, workspace_bytes=None):
    """q (m,D), g (n,D) prepared operands (as for ``distmat``) -> idx int32 (m,k), val fp32 (m,k): the k nearest gallery rows
    of every query in ascending (distance, index) order, without the (m,n) matrix (distance.py:59-89 + rank.py:171-172).
    Bit-identical to ``rank_topk(distmat(q, g, ...), k)`` when ONE query block covers m (the default workspace at the MARS sizes);
    with several blocks (a small ``workspace_bytes``, very many queries) a block's row count picks the GEMM's kernel family and
    split-K, so a distance can differ from the full-matrix path in its last bit and near-ties may swap: equal up to that
    (tests/test_gpu_kernels.py::test_distmat_topk_blocks_tie_aware)."""
    m, D = q.shape
    n, D2 = g.shape
    assert D == D2 and q.dtype == g.dtype
    code = METRIC_EUCLIDEAN if metric == "euclidean" else METRIC_COSINE
    nbytes = int(_hip.lib().agrl_distmat_topk_workspace(m, n)) if workspace_bytes is None else int(workspace_bytes)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=q.device)
    rows = max(1, min(m, nbytes // (4 * (-(-n // 4) * 4))))
    gws = None
    if (-(-rows // 64)) * (-(-n // 128)) < 256:   # few output tiles per block: split-K scratch, as in ``distmat``
        gws = torch.empty((8 * rows * n,), dtype=torch.float32, device=q.device)
    idx = torch.empty((m, k), dtype=torch.int32, device=q.device)
    val = torch.empty((m, k), dtype=torch.float32, device=q.device)
    if _hip.PROFILE is not None:  # (m+n) D e in, m k 8 out
        _hip.PROFILE_TAG = {"flops": 2.0 * m * n * D, "bytes": q.element_size() * (m + n) * D + 8.0 * m * k}
    with _dev(q):
        _hip.call("agrl_distmat_topk", ptr(q), ptr(g), ptr(qn), ptr(gn), m, n, D, code, dtype_code(q.dtype), int(k), int(idx_offset),
                  ptr(idx), ptr(val), ptr(ws), ws.numel() * 4, ptr(gws), 0 if gws is None else gws.numel() * 4, _stream(q))
    return idx, val


RANK_ARGSORT_MAX_N = 16384


def rank_argsort(dist):
    """dist (m,n) fp32, n <= 16384 -> int32 (m,n): the stable ascending order of every row (NaN last). rank.py:45-47."""
    m, n = dist.shape
    assert dist.dtype == torch.float32 and dist.stride(1) == 1 and n <= RANK_ARGSORT_MAX_N
    idx = torch.empty((m, n), dtype=torch.int32, device=dist.device)
    with _dev(dist):
        _hip.call("agrl_rank_argsort", dist.data_ptr(), m, n, dist.stride(0), ptr(idx), _stream(dist))
    return idx


def rank_mars(topk_idx, q_pids, q_camids, g_pids, g_camids):
    """-> ap fp64 (m), cmc fp32 (m,k). rank.py:160-212."""
    m, k = topk_idx.shape
    n = g_pids.numel()
    ap = torch.empty((m,), dtype=torch.float64, device=topk_idx.device)
    cmc = torch.empty((m, k), dtype=torch.float32, device=topk_idx.device)
    for t in (topk_idx, q_pids, q_camids, g_pids, g_camids):
        assert t.dtype == torch.int32
    with _dev(topk_idx):
        call("agrl_rank_mars", ptr(topk_idx), ptr(q_pids), ptr(q_camids), ptr(g_pids), ptr(g_camids), m, n, k, ptr(ap),
             ptr(cmc), _stream(topk_idx))
    return ap, cmc


def pose_adjacency(poses, detected, height, num_split=4, pyramid_part=True, threshold=0.1, packed=False):
    """AlphaPose keypoints (B,S,18,3) fp32 + per-frame detection flags (B,S) -> adjacency (B,V,V) fp32 on the device, or with
    ``packed`` the bit-packed int32 (B, V, ceil(V/32)) form the graph kernels also take. dataset_loader.py:218-388
    (generate_graph + adj_graph)."""
    B, S = poses.shape[:2]
    assert poses.dtype == torch.float32 and tuple(poses.shape[2:]) == (18, 3)
    det = detected.to(torch.uint8).contiguous()
    assert tuple(det.shape) == (B, S)
    P = 2 * num_split - 1 if pyramid_part else num_split
    if packed:
        V = S * P
        bits = torch.empty((B, V, (V + 31) // 32), dtype=torch.int32, device=poses.device)
        with _dev(poses):
            call("agrl_pose_adjacency_bits", ptr(poses.contiguous()), ptr(det), ptr(bits), B, S, int(num_split), 1 if pyramid_part else 0,
                 float(height), float(threshold), _stream(poses))
        return bits
    adj = torch.empty((B, S * P, S * P), dtype=torch.float32, device=poses.device)
    with _dev(poses):
        call("agrl_pose_adjacency", ptr(poses.contiguous()), ptr(det), ptr(adj), B, S, int(num_split), 1 if pyramid_part else 0,
             float(height), float(threshold), _stream(poses))
    return adj


def rank_market1501(dist, q_pids, q_camids, g_pids, g_camids, max_rank):
    """-> ap fp64 (m) (NaN when invalid), cmc fp32 (m,max_rank), valid int32 (m). rank.py:95-150."""
    m, n = dist.shape
    assert dist.dtype == torch.float32 and dist.stride(1) == 1
    for t in (q_pids, q_camids, g_pids, g_camids):
        assert t.dtype == torch.int32
    ap = torch.empty((m,), dtype=torch.float64, device=dist.device)
    cmc = torch.empty((m, max_rank), dtype=torch.float32, device=dist.device)
    valid = torch.empty((m,), dtype=torch.int32, device=dist.device)
    with _dev(dist):
        _hip.call("agrl_rank_market1501", dist.data_ptr(), m, n, dist.stride(0), ptr(q_pids), ptr(q_camids), ptr(g_pids),
                  ptr(g_camids), max_rank, ptr(ap), ptr(cmc), ptr(valid), _stream(dist))
    return ap, cmc, valid


def re_ranking(q_g, q_q, g_g, k1=20, k2=6, lambda_value=0.3):
    """k-reciprocal re-ranking on the device: fp32 CUDA (m,n), (m,m), (n,n) -> fp32 (m,n). utils/re_ranking.py:30-95."""
    m, n = q_g.shape
    for t, shp in ((q_g, (m, n)), (q_q, (m, m)), (g_g, (n, n))):
        assert t.dtype == torch.float32 and tuple(t.shape) == shp
    q_g, q_q, g_g = q_g.contiguous(), q_q.contiguous(), g_g.contiguous()
    out = torch.empty((m, n), dtype=torch.float32, device=q_g.device)
    nbytes = int(_hip.lib().agrl_re_ranking_workspace(m, n, int(k1)))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=q_g.device)
    with _dev(q_g):
        call("agrl_re_ranking", ptr(q_g), ptr(q_q), ptr(g_g), m, n, int(k1), int(k2), float(lambda_value), ptr(out), n,
             ptr(ws), nbytes, _stream(q_g))
    return out


def triplet_hard_mine(x, pids):
    """x (n,d) fp32, pids int32 (n) -> dist_ap, dist_an fp32 (n), idx_ap, idx_an int32 (n)."""
    n, d = x.shape
    assert x.dtype == torch.float32 and pids.dtype == torch.int32
    dap = torch.empty((n,), dtype=torch.float32, device=x.device)
    dan = torch.empty((n,), dtype=torch.float32, device=x.device)
    iap = torch.empty((n,), dtype=torch.int32, device=x.device)
    ian = torch.empty((n,), dtype=torch.int32, device=x.device)
    with _dev(x):
        call("agrl_triplet_hard_mine", ptr(x), ptr(pids), n, d, ptr(dap), ptr(dan), ptr(iap), ptr(ian), _stream(x))
    return dap, dan, iap, ian


def read_stream(buf, nbytes=None, workgroups=2048):
    """Measurement yardstick (bench.py): one pure read pass over the first ``nbytes`` of ``buf`` on the current stream."""
    total = buf.numel() * buf.element_size()
    nbytes = total if nbytes is None else min(int(nbytes), total)
    sink = torch.empty((1,), dtype=torch.float32, device=buf.device)
    with _dev(buf):
        call("agrl_diag_read_stream", ptr(buf), nbytes & ~15, ptr(sink), int(workgroups), _stream(buf))
    return sink


# ---- train step of the conv trunk (include/agrl_hip.h, "train step" section) ----------------------------------------------
def _bn_ws(M, Cc, device):
    nbytes = int(_hip.lib().agrl_bn_workspace(int(M), int(Cc)))
    return torch.empty((nbytes // 8,), dtype=torch.float64, device=device), nbytes


def bn_stats(y2d):
    """(M,C) fp32 -> mean (C), biased var (C): BatchNorm2d batch statistics. vmgn.py:49-61 under model.train()."""
    M, Cc = y2d.shape
    assert y2d.dtype == torch.float32 and y2d.is_contiguous()
    mean = torch.empty((Cc,), dtype=torch.float32, device=y2d.device)
    var = torch.empty((Cc,), dtype=torch.float32, device=y2d.device)
    ws, nbytes = _bn_ws(M, Cc, y2d.device)
    with _dev(y2d):
        call("agrl_bn_stats", ptr(y2d), ptr(mean), ptr(var), M, Cc, ptr(ws), nbytes, _stream(y2d))
    return mean, var


def conv_stats(x, w_ohwi, stride, pad):
    """fp32 NHWC conv (no bias / activation) + the batch statistics of its output: -> y (N,OH,OW,Cout), mean (Cout), var (Cout,
    biased). The per-tile sums come out of the conv's epilogue; nothing re-reads y."""
    N, H, W, Cin = x.shape
    Cout, R, S, Cin2 = w_ohwi.shape
    assert Cin == Cin2 and x.dtype == torch.float32 and w_ohwi.dtype == torch.float32
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    M = N * OH * OW
    rows = -(-M // 64)
    out = torch.empty((N, OH, OW, Cout), dtype=torch.float32, device=x.device)
    partial = torch.empty((rows * 2 * Cout,), dtype=torch.float32, device=x.device)
    mean = torch.empty((Cout,), dtype=torch.float32, device=x.device)
    var = torch.empty((Cout,), dtype=torch.float32, device=x.device)
    with _dev(x):
        call("agrl_conv2d_stats", ptr(x), ptr(w_ohwi), ptr(out), ptr(partial), partial.numel() * 4, N, H, W, Cin, Cout, R, S, stride, pad,
             _gemm_code(torch.float32), _stream(x))
        ws, nbytes = _bn_ws(rows, 2 * Cout, x.device)
        call("agrl_bn_stats_from_partials", ptr(partial), rows, Cout, M, ptr(mean), ptr(var), ptr(ws), nbytes, _stream(x))
    return out, mean, var


def bn_fold_train(mean, var, gamma, beta, eps, momentum, n, running_mean=None, running_var=None, num_batches_tracked=None):
    """-> scale, shift, invstd (C): the folded BatchNorm of the batch statistics, and -- in the same launch -- the running-statistics
    update nn.BatchNorm applies in train mode (momentum, unbiased variance, num_batches_tracked += 1). vmgn.py:49-63, :169."""
    Cc = mean.numel()
    scale, shift, invstd = torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean)
    if num_batches_tracked is not None:
        assert num_batches_tracked.dtype == torch.int64
    with _dev(mean):
        call("agrl_bn_fold_train", ptr(mean), ptr(var), ptr(gamma), ptr(beta), float(eps), float(momentum), int(n), ptr(running_mean),
             ptr(running_var), ptr(num_batches_tracked), ptr(scale), ptr(shift), ptr(invstd), Cc, _stream(mean))
    running = [t for t in (running_mean, running_var, num_batches_tracked) if t is not None]
    if running:
        written(running)      # the module's buffers: the eval forward's pack is folded from them
    return scale, shift, invstd


def bn_apply(y2d, scale, shift, residual, relu, slope=0.0, want_mask=False):
    """relu: activation on; slope 0 = ReLU, > 0 = LeakyReLU(slope). -> out, mask: with ``want_mask`` (and relu) the sign bits of
    the pre-activation, one bit per element (uint8, M*C/8 bytes) -- what ``bn_backward`` needs instead of the output."""
    M, Cc = y2d.shape
    out = torch.empty_like(y2d)
    mask = torch.empty(((M * Cc + 7) // 8,), dtype=torch.uint8, device=y2d.device) if (want_mask and relu) else None
    with _dev(y2d):
        call("agrl_bn_apply", ptr(y2d), ptr(scale), ptr(shift), ptr(residual), ptr(out), ptr(mask), M, Cc, 1 if relu else 0, float(slope),
             _stream(y2d))
    return out, mask


def bn_backward(dout, out, y2d, mean, invstd, gamma, relu, want_dz, slope=0.0, mask=None):
    """-> dy (M,C), dz (M,C) or None, dgamma (C), dbeta (C). With relu either the forward output ``out`` or the sign ``mask``
    of ``bn_apply``."""
    M, Cc = y2d.shape
    dy = torch.empty_like(y2d)
    dz = torch.empty_like(y2d) if want_dz else None
    dgamma = torch.empty((Cc,), dtype=torch.float32, device=y2d.device)
    dbeta = torch.empty((Cc,), dtype=torch.float32, device=y2d.device)
    ws, nbytes = _bn_ws(M, Cc, y2d.device)
    with _dev(y2d):
        call("agrl_bn_backward", ptr(dout), ptr(out) if (relu and mask is None) else None, ptr(mask) if relu else None, ptr(y2d), ptr(mean),
             ptr(invstd), ptr(gamma), 1 if relu else 0,
             float(slope), ptr(dy), ptr(dz), ptr(dgamma), ptr(dbeta), M, Cc, ptr(ws), nbytes, _stream(y2d))
    return dy, dz, dgamma, dbeta


def im2col_t(x, R, S, stride, pad):
    """x (F,H,W,C) fp32 NHWC -> (R*S*C, Mpad) fp32, Mpad = F*OH*OW rounded up to the GEMM's k-tile (zero columns):
    tap-expanded channel-major transpose (weight-gradient operand)."""
    F_, H, W, Cc = x.shape
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    ld = -(-(F_ * OH * OW) // 32) * 32
    T = torch.empty((R * S * Cc, ld), dtype=torch.float32, device=x.device)
    with _dev(x):
        call("agrl_im2col_t", ptr(x), ptr(T), ld, F_, H, W, Cc, R, S, stride, pad, _stream(x))
    return T


def gemm_nt_splitk(x, w):
    """(M,K) @ (N,K)^T -> fp32 (M,N), K split over workgroups (weight gradients)."""
    M, K = x.shape
    Nout, K2 = w.shape
    assert K == K2 and x.dtype == w.dtype
    y = torch.empty((M, Nout), dtype=torch.float32, device=x.device)
    # enough for the split the entry point will choose: it stops at >= 1024 workgroups, i.e. at most 1024 / tiles slices
    tiles = (-(-M // 64)) * (-(-Nout // (64 if Nout <= 64 else 128)))
    ks_cap = 1
    while ks_cap < 256 and tiles * ks_cap < 1024:
        ks_cap *= 2
    ws = torch.empty((ks_cap * M * Nout,), dtype=torch.float32, device=x.device)
    with _dev(x):
        call("agrl_gemm_nt_splitk", ptr(x), ptr(w), ptr(y), M, K, Nout, _gemm_code(x.dtype), ptr(ws), ws.numel() * 4, _stream(x))
    return y


def im2col_rows(x, R, S, stride, pad, ld, nchw=False):
    """Pixel-major patches of an NHWC (or NCHW) fp32 tensor: -> (F*OH*OW, ld), columns (r, s, c), zero padded to ``ld``."""
    if nchw:
        F_, Cc, H, W = x.shape
    else:
        F_, H, W, Cc = x.shape
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    x = x.contiguous()
    P = torch.empty((F_ * OH * OW, ld), dtype=torch.float32, device=x.device)
    with _dev(x):
        call("agrl_im2col_rows", ptr(x), ptr(P), ld, F_, H, W, Cc, R, S, stride, pad, 1 if nchw else 0, _stream(x))
    return P, OH, OW


def conv_wgrad_supported(Cin, Cout):
    return Cin % 4 == 0 and Cout % 4 == 0


def conv_wgrad_plan(F_, H, W, Cin, Cout, R, S, stride, pad):
    """-> (output-channel tile, input-channel tile, pixel slices, 32-pixel k-tiles per slice) agrl_conv_wgrad runs for this shape
    in the calling thread's arithmetic mode (no launch)."""
    plan = (C.c_int * 4)()
    call("agrl_conv_wgrad_plan", F_, H, W, Cin, Cout, R, S, stride, pad, _gemm_code(torch.float32), plan)
    return tuple(int(v) for v in plan)


def conv_wgrad(x, dy, wshape, stride, pad):
    """Weight gradient of a conv from the NHWC activations: x (F,H,W,Cin), dy (F,OH,OW,Cout) fp32 -> dw (Cout,Cin,R,S) fp32
    (the nn.Conv2d.weight.grad layout); exact fp32 or, under ``f32_split``, the split-bf16 arithmetic."""
    Cout, Cin, R, S = (int(v) for v in wshape)
    F_, H, W, Cc = x.shape
    assert Cc == Cin and dy.shape[-1] == Cout and x.dtype == torch.float32 and dy.dtype == torch.float32
    x, dy = x.contiguous(), dy.contiguous()
    dw = torch.empty((Cout, Cin, R, S), dtype=torch.float32, device=x.device)
    with _dev(x):
        nbytes = _hip.lib().agrl_conv_wgrad_workspace(F_, H, W, Cin, Cout, R, S, stride, pad)
        ws = torch.empty((max(int(nbytes) // 4, 4),), dtype=torch.float32, device=x.device)
        call("agrl_conv_wgrad", ptr(x), ptr(dy), ptr(dw), F_, H, W, Cin, Cout, R, S, stride, pad, _gemm_code(torch.float32), ptr(ws),
             ws.numel() * 4, _stream(x))
    return dw


def maxpool3x3s2(x):
    F_, H, W, Cc = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((F_, OH, OW, Cc), dtype=torch.float32, device=x.device)
    idx = torch.empty((F_, OH, OW, Cc), dtype=torch.uint8, device=x.device)
    with _dev(x):
        call("agrl_maxpool3x3s2", ptr(x), ptr(out), ptr(idx), F_, H, W, Cc, _stream(x))
    return out, idx


def maxpool3x3s2_backward(dout, idx, H, W):
    F_, OH, OW, Cc = dout.shape
    dx = torch.empty((F_, H, W, Cc), dtype=torch.float32, device=dout.device)
    with _dev(dout):
        call("agrl_maxpool3x3s2_backward", ptr(dout), ptr(idx), ptr(dx), F_, H, W, Cc, _stream(dout))
    return dx


def triplet_loss(x, pids, margin, soft):
    """Batch-hard triplet loss value + feature gradient in one native call (no host sync). -> loss (1,), grad (n,d)."""
    n, d = x.shape
    assert x.dtype == torch.float32 and pids.dtype == torch.int32
    dev = x.device
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    grad = torch.empty((n, d), dtype=torch.float32, device=dev)
    dap, dan = torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev)
    iap, ian = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
    coeff = torch.empty((2 * n,), dtype=torch.float32, device=dev)
    with _dev(x):
        call("agrl_triplet_loss", ptr(x), ptr(pids), n, d, float(margin), 1 if soft else 0, ptr(loss), ptr(grad), ptr(dap), ptr(dan),
             ptr(iap), ptr(ian), ptr(coeff), _stream(x))
    return loss, grad


# ---- train step of the tail (include/agrl_hip.h, "train step of the tail" section) ------------------------------------------
def axpby(a, x, b=0.0, y=None):
    out = torch.empty_like(x)
    with _dev(x):
        call("agrl_axpby", ptr(x.contiguous()), ptr(y.contiguous()) if y is not None else None, float(a), float(b), ptr(out), x.numel(), _stream(x))
    return out


def part_pool_backward(dg, dnodes, S, h, w, splits):
    """dg (B,C) | None, dnodes (F,P,C) -> dx1 (F,h,w,C) | None, dx2 (F,h,w,C): backward of part_pool. vmgn.py:298-308."""
    F_, P, Cc = dnodes.shape
    dx2 = torch.empty((F_, h, w, Cc), dtype=torch.float32, device=dnodes.device)
    dx1 = torch.empty_like(dx2) if dg is not None else None
    arr = (C.c_int * len(splits))(*[int(v) for v in splits])
    with _dev(dnodes):
        call("agrl_part_pool_backward", ptr(dg.contiguous()) if dg is not None else None, ptr(dnodes.contiguous()), ptr(dx1), ptr(dx2), F_, S, h, w,
             Cc, arr, len(splits), _stream(dnodes))
    return dx1, dx2


def attn_pool_backward(nodes, datt):
    """nodes (B,S,P,C), datt (B,C) -> dnodes (B,S,P,C). vmgn.py:270-278, :313-317."""
    B, S, P, Cc = nodes.shape
    dn = torch.empty_like(nodes)
    with _dev(nodes):
        call("agrl_attn_pool_backward", ptr(nodes.contiguous()), ptr(datt.contiguous()), ptr(dn), B, S, P, Cc, _stream(nodes))
    return dn


def graph_gram(f):
    """f (B,V,C) fp32 -> the Gram (B, nz, V, V) (first half of graph_matrix, kept for the backward pass): the C / 128 slice
    partials up to GRAM_SLICE_MAX_V nodes, the fully summed tiled form (nz = 1) beyond."""
    with _dev(f):
        return _gram_into(f)


def graph_pair_product(a, b):
    """a, b (B,V,C) fp32 -> (B,V,V) with out[t] = a[t] b[t]^T (d loss / d G of the message pass, vmgn.py:168); beyond
    PAIR_PRODUCT_MAX_V nodes by the tiled kernel (no slice partials)."""
    B, V, Cc = a.shape
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32 and Cc % GRAM_CSLICE == 0
    out = torch.empty((B, V, V), dtype=torch.float32, device=a.device)
    with _dev(a):
        part = None   # the slice partials, only where the slices form runs
        if graph_forms(V, Cc)["pair"] == "slices":
            part = torch.empty((B, Cc // GRAM_CSLICE, V, V), dtype=torch.float32, device=a.device)
        call("agrl_graph_pair_product", ptr(a.contiguous()), ptr(b.contiguous()), ptr(part), ptr(out), B, V, Cc, _stream(a))
    return out


def graph_finalize(gram, adj, B, V, use_pose, learn_graph, mask_diag=False):
    G = torch.empty((B, V, V), dtype=torch.float32, device=(gram if gram is not None else adj).device)
    nz = gram.shape[1] if gram is not None else 0
    with _dev(G):
        call("agrl_graph_finalize", ptr(gram), nz, ptr(adj.contiguous()) if use_pose else None, ptr(G), B, V, 1 if use_pose else 0,
             1 if learn_graph else 0, 1 if mask_diag else 0, _stream(G))
    return G


def graph_matrix_backward(gram, dG, use_pose, mask_diag=False):
    """Gram partials (B,nz,V,V), dG (B,V,V) -> M (B,V,V) with d loss / d f = M f. vmgn.py:114-120, :155-166."""
    B, nz, V, _ = gram.shape
    M = torch.empty((B, V, V), dtype=torch.float32, device=gram.device)
    with _dev(gram):
        call("agrl_graph_matrix_backward", ptr(gram), nz, ptr(dG.contiguous()), ptr(M), B, V, 1 if use_pose else 0, 1 if mask_diag else 0, _stream(gram))
    return M


def graph_apply(G, h):
    """G (B,V,V) @ h (B,V,C) on the message-pass kernel (unit BatchNorm, no activation, no residual)."""
    Cc = h.shape[-1]
    key = (h.device, Cc)
    if key not in _UNIT:
        _UNIT[key] = (torch.ones((Cc,), dtype=torch.float32, device=h.device), torch.zeros((Cc,), dtype=torch.float32, device=h.device))
    one, zero = _UNIT[key]
    out, _ = graph_propagate(h, h, G, one, zero, 1.0, 1.0, want_lp=False, keep=0.0)
    return out


_UNIT = {}


def xent_label_smooth(logits, targets, eps):
    """-> loss (1,), dlogits (n,K): CrossEntropyLabelSmooth value + gradient in one call. cross_entropy_loss.py:26-37."""
    n, K = logits.shape
    loss = torch.empty((1,), dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits)
    rows = torch.empty((n,), dtype=torch.float32, device=logits.device)
    with _dev(logits):
        call("agrl_xent_label_smooth", ptr(logits), ptr(targets), n, K, float(eps), ptr(loss), ptr(dl), ptr(rows), _stream(logits))
    return loss, dl


# ---- optimiser update (include/agrl_hip.h, "optimiser update of the train step"; host side: torchreid/hip_optim.py) --------
def optim_geometry():
    """-> (elements per chunk, workgroups at most, int64 words per tensor descriptor): the library's constants."""
    chunk, grid, words = C.c_int(0), C.c_int(0), C.c_int(0)
    _hip._check("agrl_optim_geometry", _hip.lib().agrl_optim_geometry(C.byref(chunk), C.byref(grid), C.byref(words)))
    return chunk.value, grid.value, words.value


def _optim_tables(tensors, chunks):
    assert tensors.dtype == torch.int64 and tensors.dim() == 2 and chunks.dtype == torch.int32 and chunks.dim() == 2 and chunks.size(1) == 2
    assert tensors.device == chunks.device
    return ptr(tensors), tensors.size(0), ptr(chunks), chunks.size(0)


def adam_step(tensors, chunks, weight_decay, one_minus_beta1, beta2, one_minus_beta2, step_size, inv_sqrt_bc2, eps, amsgrad, zero_grad):
    """One multi-tensor Adam / AMSGrad update in place. tensors: int64 (n, words) descriptor table, chunks: int32 (n_chunks, 2), both
    on the parameters' device; the seven constants are fp32 values formed in double by the caller. optimizers.py:8-11."""
    with _dev(tensors):
        call("agrl_adam_step", *_optim_tables(tensors, chunks), float(weight_decay), float(one_minus_beta1), float(beta2),
             float(one_minus_beta2), float(step_size), float(inv_sqrt_bc2), float(eps), 1 if amsgrad else 0, 1 if zero_grad else 0,
             _stream(tensors))


def sgd_step(tensors, chunks, weight_decay, momentum, lr, has_momentum, first_step, nesterov, zero_grad):
    """One multi-tensor SGD update in place (momentum / Nesterov momentum, dampening 0). optimizers.py:12-15."""
    with _dev(tensors):
        call("agrl_sgd_step", *_optim_tables(tensors, chunks), float(weight_decay), float(momentum), float(lr), 1 if has_momentum else 0,
             1 if first_step else 0, 1 if nesterov else 0, 1 if zero_grad else 0, _stream(tensors))


def rmsprop_step(tensors, chunks, weight_decay, alpha, one_minus_alpha, eps, momentum, lr, has_momentum, zero_grad):
    """One multi-tensor RMSprop update in place (not centered; momentum optional). optimizers.py:16-17."""
    with _dev(tensors):
        call("agrl_rmsprop_step", *_optim_tables(tensors, chunks), float(weight_decay), float(alpha), float(one_minus_alpha), float(eps),
             float(momentum), float(lr), 1 if has_momentum else 0, 1 if zero_grad else 0, _stream(tensors))


def adabound_step(tensors, chunks, weight_decay, one_minus_beta1, beta2, one_minus_beta2, step_size, eps, lower, upper, amsbound, zero_grad):
    """One multi-tensor AdaBound / AMSBound update in place; step_size, lower and upper are the step's constants
    (hip_optim.adabound_constants). optimizers.py:26-138."""
    with _dev(tensors):
        call("agrl_adabound_step", *_optim_tables(tensors, chunks), float(weight_decay), float(one_minus_beta1), float(beta2),
             float(one_minus_beta2), float(step_size), float(eps), float(lower), float(upper), 1 if amsbound else 0, 1 if zero_grad else 0,
             _stream(tensors))


def radam_step(tensors, chunks, one_minus_beta1, beta2, one_minus_beta2, decay, step_size, eps, adaptive, zero_grad):
    """One multi-tensor RAdam update in place; step_size and the form (adaptive or momentum-only) are the step's constants
    (hip_optim.radam_constants). optimizers.py:141-211."""
    with _dev(tensors):
        call("agrl_radam_step", *_optim_tables(tensors, chunks), float(one_minus_beta1), float(beta2), float(one_minus_beta2),
             float(decay), float(step_size), float(eps), 1 if adaptive else 0, 1 if zero_grad else 0, _stream(tensors))


# ---- tails of the STA baselines (csrc/sta.hip) --------------------------------------------------------------------------------
STA_PARTS = 4
LINEAR_BN_RELU_MAX_M = 32   # AGRL_LINEAR_BN_RELU_MAX_M: the rows of x the kernel's LDS staging holds


def sta_bins(h):
    """[(row0, row1)] of AdaptiveAvgPool2d((4,1)) over h rows: floor(i h / 4) .. ceil((i + 1) h / 4)."""
    return [((i * h) // STA_PARTS, -((-(i + 1) * h) // STA_PARTS)) for i in range(STA_PARTS)]


def sta_frame_stats(fmap):
    """(F,h,w,C) NHWC map, fp32 or the 16-bit type -> vmean (F,4,C), nsum (F,4), nsq (F,4) fp32: the part means, per bin the sum of the
    pixels' channel norms, and the sum of their squares over the rows of the bin no later bin starts in. sta.py:213-222."""
    assert fmap.dim() == 4 and fmap.is_cuda and fmap.is_contiguous() and fmap.dtype in (torch.float32, LP_DTYPE)
    F_, h, w, Cc = fmap.shape
    assert h >= STA_PARTS and Cc % 8 == 0 and Cc <= (4096 if fmap.dtype == torch.float32 else 8192), (h, Cc)
    assert fmap.data_ptr() % 16 == 0
    vmean = torch.empty((F_, STA_PARTS, Cc), dtype=torch.float32, device=fmap.device)
    nsum = torch.empty((F_, STA_PARTS), dtype=torch.float32, device=fmap.device)
    nsq = torch.empty((F_, STA_PARTS), dtype=torch.float32, device=fmap.device)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 3.0 * fmap.numel(), "bytes": fmap.element_size() * fmap.numel() + 4 * vmean.numel()}
    with _dev(fmap):
        call("agrl_sta_frame_stats", ptr(fmap), ptr(vmean), ptr(nsum), ptr(nsq), F_, h, w, Cc, dtype_code(fmap.dtype), _stream(fmap))
    return vmean, nsum, nsq


def sta_fuse(vmean, B, S, nsum=None, nsq=None, hw=None):
    """vmean (B*S,4,C) fp32 -> f_g (B,2C) fp32, t_a (B,S,4) fp32, idx (B,4) int32: per part the first frame attaining the largest
    temporal attention, cat(mean over parts of the selected means, mean over parts of the attention-weighted sums). With ``nsum`` /
    ``nsq`` (B*S,4) and the map's ``hw``: sta's scores (the map mode); without: simple_sta's (channel norms of the part means)."""
    assert vmean.dtype == torch.float32 and vmean.is_cuda and vmean.is_contiguous() and vmean.data_ptr() % 16 == 0
    assert vmean.dim() == 3 and tuple(vmean.shape[:2]) == (B * S, STA_PARTS) and vmean.shape[2] % 4 == 0 and B > 0 and S > 0
    Cc = vmean.shape[2]
    map_mode = nsum is not None
    if map_mode:
        assert nsq is not None and hw is not None and hw[0] >= STA_PARTS and hw[1] > 0
        for t in (nsum, nsq):
            assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B * S, STA_PARTS) and t.device == vmean.device
    else:
        assert nsq is None
    f_g = torch.empty((B, 2 * Cc), dtype=torch.float32, device=vmean.device)
    t_a = torch.empty((B, S, STA_PARTS), dtype=torch.float32, device=vmean.device)
    idx = torch.empty((B, STA_PARTS), dtype=torch.int32, device=vmean.device)
    h, w = hw if map_mode else (0, 0)
    with _dev(vmean):
        call("agrl_sta_fuse", ptr(vmean), ptr(nsum), ptr(nsq), ptr(f_g), ptr(t_a), ptr(idx), B, S, Cc, int(h), int(w),
             0 if map_mode else 1, _stream(vmean))
    return f_g, t_a, idx


def linear_bn_relu(x, w, scale, shift):
    """relu(scale * (x w^T) + shift): x (M,K) fp32, w (N,K) fp32 or the 16-bit type, scale / shift (N) fp32 -> (M,N) fp32. The
    weight-streaming kernel up to LINEAR_BN_RELU_MAX_M rows; above, the tiled GEMM (linear_nobias on operands of the weight's type)
    and the epilogue in torch."""
    assert x.dim() == 2 and w.dim() == 2 and x.shape[1] == w.shape[1] and x.dtype == torch.float32 and w.dtype in (torch.float32, LP_DTYPE)
    assert x.is_cuda and x.is_contiguous() and w.is_contiguous() and w.device == x.device
    M, K = x.shape
    Nout = w.shape[0]
    for t in (scale, shift):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (Nout,) and t.device == x.device
    if M > LINEAR_BN_RELU_MAX_M:
        y = linear_nobias(x if w.dtype == torch.float32 else x.to(w.dtype), w)
        return torch.relu(y * scale + shift)
    assert K % 4 == 0 and x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
    out = torch.empty((M, Nout), dtype=torch.float32, device=x.device)
    if _hip.PROFILE is not None:
        _hip.PROFILE_TAG = {"flops": 2.0 * M * K * Nout, "bytes": w.element_size() * w.numel() + 4 * (x.numel() + out.numel())}
    with _dev(x):
        call("agrl_linear_bn_relu", ptr(x), ptr(w), ptr(scale), ptr(shift), ptr(out), M, K, Nout, dtype_code(w.dtype), _stream(x))
    return out
