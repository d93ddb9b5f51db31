"""Device-resident evaluation harness: the dataflow of the reference's ``test()``
(train_vidreid_xent_htri.py:450-542) with everything after the data loader kept on the GPU.

    reference test()                                   this harness
    ------------------------------------------------   ---------------------------------------------------------
    model(imgs, adj) per batch            (:469,:499)   same call (the HIP eval forward)
    dense/skipdense clip pooling          (:471-476)    ``pool_clips`` (mean / max over a tracklet's clips)
    features.data.cpu(); torch.cat        (:477-511)    embeddings stay in HBM; RCCL all-gather when sharded
    compute_distance_matrix on CPU        (:520)        ``agrl_distmat_topk`` against the rank's gallery shard: distance rows of
    evaluate_rank(use_metric_mars=True)   (:531)        one query block at a time + top-k; candidate merge + ``agrl_rank_mars``
    returns cmc[0], mAP                   (:542)        returns (cmc, mAP) (+ the top-k lists on request)

With ``torch.distributed`` initialised (one process per GPU) the tracklet batches and the gallery rows are sharded
over the ranks (torchreid/parallel.py); every rank returns the same (cmc, mAP).
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from torchreid import hip_ops as ops
from torchreid import parallel
from torchreid.device_transforms import eval_geometry
from torchreid.metrics.distance import hip_distmat_device, hip_distmat_topk_device


def pool_clips(features, num_clips, pool="avg"):
    """(tracklets*num_clips, D) -> (tracklets, D): mean or max over each tracklet's clips
    (reference: features.view(n, 1, -1) then mean/max over dim 0, train_vidreid_xent_htri.py:471-476)."""
    if num_clips == 1:
        return features
    if features.is_cuda:
        return ops.clip_pool(features, num_clips, "avg" if pool == "avg" else "max")
    f = features.view(-1, num_clips, features.size(-1))
    return f.mean(dim=1) if pool == "avg" else f.max(dim=1)[0]


def device_prefetch(batches, device):
    """Upload batch i+1 on a copy stream while batch i is being processed (the reference's test() uploads inside the
    loop, train_vidreid_xent_htri.py:460, and its loaders hand over pinned tensors, :222-247 ``pin_memory``): with pinned
    sources the frames of a 256-frame batch -- 100 MB as fp32, 25 MB as the uint8 a decoder produces, which the models take as
    they are -- cross PCIe under the previous batch's forward. The dtype is kept. Yields the same tuples with imgs / adj on
    ``device``; tensors already there pass through. A fifth element (the valid-extent array of a padded ragged batch,
    ``extract_features(frame_size=...)``) is passed through untouched: it stays a host array."""
    if device.type != "cuda":
        for item in batches:
            yield item
        return
    copy_stream = torch.cuda.Stream(device=device)
    main = torch.cuda.current_stream(device)

    def upload(item):
        imgs, pid, camid, adj = item[:4]
        with torch.cuda.stream(copy_stream):
            imgs_d, adj_d = imgs.to(device, non_blocking=True), adj.to(device, non_blocking=True)
            done = torch.cuda.Event()
            done.record(copy_stream)
        return (imgs_d, pid, camid, adj_d) + tuple(item[4:]), done

    pending = None
    for item in batches:
        nxt = upload(item)
        if pending is not None:
            yield _claim(pending, main)
        pending = nxt
    if pending is not None:
        yield _claim(pending, main)


def decode_batches(batches, device, decoder=None):
    """Loader items whose ``imgs`` entry is a nested list of ENCODED frames -- JPEG ``bytes``, [b][S] or [b][n][S] -- decoded on the
    device (``device_decode.DeviceJpegDecoder``: headers on the host, entropy decode / IDCT / upsampling / colour on the GPU, byte for
    byte Pillow's ``Image.open().convert('RGB')``): yields the 5-tuples (imgs uint8 (b,[n,]S,Hmax,Wmax,3) on ``device``, pids, camids,
    adj, sizes int (b,[n,]S,2)) that ``extract_features(..., frame_size=...)`` and ``extract_features_packed`` take, so
    ``evaluate(..., clip_batch=32, frame_size=...)`` on JPEG files needs no other change. Items whose imgs is already a tensor pass through.
    Files outside the decoder's subset take its Pillow fallback; ``decoder``: one to reuse (its counters run on)."""
    from torchreid.device_decode import DeviceJpegDecoder, _nested
    decoder = DeviceJpegDecoder(device) if decoder is None else decoder
    for item in batches:
        imgs, pid, camid, adj = item[:4]
        if isinstance(imgs, torch.Tensor):
            yield item
            continue
        flat, shape = _nested(imgs)
        if len(shape) not in (2, 3):
            raise ValueError("encoded imgs is a nested list [b][S] or [b][n][S] of bytes, got nesting %s" % (shape,))
        clips, sizes = decoder.decode(flat, shape)
        # the frames are on the device: the adjacency goes with them (the extractions take an item from one side or the other)
        yield (clips, pid, camid, adj.to(device, non_blocking=True) if isinstance(adj, torch.Tensor) else adj, sizes)


def _claim(pending, main):
    item, done = pending
    main.wait_event(done)
    item[0].record_stream(main)
    item[3].record_stream(main)
    return item


@torch.no_grad()
def extract_features(model, batches, pool="avg", prefetch=True, local_only=False, sync_ranks=None, frame_size=None):
    """``batches`` yields (imgs, pids, camids, adj) like the reference's loaders; imgs is (b,S,3,H,W) or, for the
    dense samplers, (b,n,S,3,H,W) with adj (b,n,V,V). Returns (features (N,D) on the model's device, pids, camids).
    imgs is fp32 (normalised by the loader's transform_test) or uint8 -- channel-first as above or channel-last, (b,S,H,W,3) /
    (b,n,S,H,W,3), straight from the decoder: a quarter of the PCIe bytes and no ToTensor / Normalize on the host; the model
    normalises inside its stem kernel (model.pixel_mean / pixel_std), bit-identical to the fp32 route.

    ``frame_size=(H, W)``: the size the model takes. uint8 channel-last batches of any other spatial size -- frames as decoded -- are
    resampled to it on the device before the model call (``hip_ops.clip_resample``: the reference's GroupResize, byte for byte
    Pillow's BILINEAR resize). A batch item may then be a 5-tuple whose last element is the int array (b,[n,]S,2) of each frame's valid
    (height, width) inside a padded container, for ragged batches; without it every frame fills its container. Batches already
    (H, W) pass through; a uint8 channel-first batch or an fp32 batch of another size raises ValueError (neither can be resampled
    here). The default ``None`` resamples nothing and takes 4-tuples only.

    Under an active process group (world > 1) the call is COLLECTIVE by default: every rank extracts its slice and then meets
    the others in ``match_and_rank``, so the non-finite flag is all-reduced (MAX) -- by every rank, whatever device its model
    is on -- and all of them raise together instead of one leaving the rest blocked in the next collective.
    ``local_only=True`` is the explicit opt-out for a call that only THIS rank makes (a rank-0-only ``evaluate``): no
    collective is issued and a non-finite embedding raises on this rank alone. (``sync_ranks``: the round-4 spelling,
    ``sync_ranks=False`` == ``local_only=True``.)"""
    device = next(model.parameters()).device
    model.eval()
    feats, pids, camids = [], [], []
    nonfinite = None
    if prefetch:
        batches = device_prefetch(batches, device)
    for item in batches:
        if len(item) not in ((4,) if frame_size is None else (4, 5)):
            raise ValueError("a batch is (imgs, pids, camids, adj)%s, got %d elements" % (
                "; a fifth element, the frames' valid extents, needs frame_size" if frame_size is None else " or that plus the valid extents",
                len(item)))
        imgs, pid, camid, adj = item[:4]
        sizes = item[4] if len(item) > 4 else None
        imgs, adj = imgs.to(device, non_blocking=True), adj.to(device, non_blocking=True)
        clips = 1
        if imgs.dim() == 6:
            b, clips = imgs.shape[:2]
            imgs = imgs.reshape((b * clips,) + tuple(imgs.shape[2:]))   # whichever layout the trailing axes have
            adj = adj.reshape((b * clips,) + tuple(adj.shape[2:]))
        if frame_size is not None:
            imgs = _to_frame_size(imgs, sizes, frame_size)
        raw = model(imgs, adj)
        if raw.is_cuda:   # accumulated on the device, read once after the last batch: no per-batch synchronisation
            bad = ~torch.isfinite(raw).all()
            nonfinite = bad if nonfinite is None else (nonfinite | bad)
        feats.append(pool_clips(raw, clips, pool))
        pids.extend(np.asarray(pid).tolist())
        camids.extend(np.asarray(camid).tolist())
    out = torch.cat(feats, 0)
    if sync_ranks is not None:
        local_only = not sync_ranks
    _raise_if_nonfinite(model, nonfinite, out.device, local_only)
    return out, np.asarray(pids), np.asarray(camids)


def _raise_if_nonfinite(model, nonfinite, device, local_only):
    """The end of an extraction: ``nonfinite`` is None (nothing was checked: the CPU path of ``extract_features``) or a one-element
    tensor, non-zero when a raw model output was inf / NaN. Read here, once; all-reduced (MAX) first when the call is collective."""
    # One check per extraction, on the RAW model outputs (before the dense samplers' clip pooling): the fp16 build stores
    # activations with a range of 65504 -- a checkpoint whose activations leave it yields inf / nan embeddings, and ranking those
    # would be silent garbage. (Nothing on this path comes near the limit with the recipe or with trained ResNet50 statistics.)
    sync = not local_only and parallel.world_size() > 1
    if nonfinite is not None or sync:
        flag = (nonfinite.to(torch.int32) if nonfinite is not None else torch.zeros((), dtype=torch.int32, device=device)).reshape(1)
        if sync:   # every rank takes part, also one whose features came from the CPU path (flag 0)
            torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MAX)
        if bool(flag.item()):
            from torchreid import _hip
            raise FloatingPointError(
                "non-finite embeddings from the %s forward (hip_precision=%r)%s" % (
                    _hip.LP_NAME if getattr(model, "hip_precision", "fp32") == _hip.LP_NAME else "HIP", getattr(model, "hip_precision", None),
                    ": activations (or BatchNorm-folded weights) left fp16's range -- set AGRL_HIP_LP16=bf16 (libagrl_hip_bf16.so) or "
                    "hip_precision='fp32'" if _hip.LP_NAME == "fp16" and getattr(model, "hip_precision", "fp32") == "fp16" else ""))


def _fits_frame_size(shape, frame_size):
    """whether clips of ``shape`` (B,S,3,H,W) / (B,S,H,W,3) already have the model's frame size"""
    H, W = int(frame_size[0]), int(frame_size[1])
    if len(shape) != 5:
        raise ValueError("clips are (b,[n,]S,3,H,W) or (b,[n,]S,H,W,3), got %s" % (tuple(shape),))
    return tuple(shape[3:]) == (H, W) if ops.frames_layout(shape) == 'nchw' else tuple(shape[2:4]) == (H, W)


def _to_frame_size(imgs, sizes, frame_size, out=None):
    """(B,S,...) clips on the device -> clips of ``frame_size``: ones already that size pass (either layout, either dtype) unless valid
    extents came with them; uint8 channel-last ones of another size, or with extents, are resampled; anything else is a ValueError.
    ``out``: uint8 (B,S,H,W,3) the resampled clips are written to (the packed route's slice of a staging buffer)."""
    H, W = int(frame_size[0]), int(frame_size[1])
    fits = _fits_frame_size(imgs.shape, frame_size)
    layout = ops.frames_layout(imgs.shape)
    if fits and sizes is None:
        return imgs if out is None else out.copy_(imgs)
    if imgs.dtype != torch.uint8 or layout != 'nhwc':
        raise ValueError("a %s channel-%s batch of %s cannot be resampled to frame_size=%s%s: hand over the decoded uint8 channel-last frames" % (
            imgs.dtype, "first" if layout == 'nchw' else "last", tuple(imgs.shape[2:]), (H, W),
            "" if sizes is None else " (valid extents were given)"))
    B, S, Hs, Ws = imgs.shape[:4]
    if sizes is None:
        sizes = np.broadcast_to(np.array([Hs, Ws], dtype=np.int64), (B, S, 2))
    else:
        sizes = np.asarray(sizes.cpu() if isinstance(sizes, torch.Tensor) else sizes)
        if sizes.size != B * S * 2:
            raise ValueError("valid extents are (b,[n,]S,2) for clips of %s, got %s" % (tuple(imgs.shape[:2]), sizes.shape))
    geometry = eval_geometry(sizes.reshape(B * S, 2))
    return ops.clip_resample(imgs.contiguous().view(B * S, Hs, Ws, 3), geometry, (H, W),
                             out=None if out is None else out.view(B * S, H, W, 3)).view(B, S, H, W, 3)


def clip_indices(num, seq_len, sample, max_len=1000):
    """The frame indices the reference's ``VideoDataset.__getitem__`` (dataset_loader.py:84-168) reads from a tracklet of ``num``
    frames, as an int64 array, for callers that hold decoded tracklets instead of the reference's loader. ``sample``: 'evenly'
    (seq_len indices), 'all' (num), 'dense' / 'skipdense' (clips of seq_len, clip after clip). Its quirks are kept: ``max_len``
    cuts the tracklet first; dense / skipdense append ``seq_len - num % seq_len`` copies of the last frame, so a length that is a
    multiple of seq_len gets one whole extra clip of it (8 frames at seq_len 4 are 3 clips); skipdense interleaves the padded list
    with stride len // seq_len (:157-168); evenly's float stride num / seq_len is truncated at use (int(index), :175)."""
    num, seq_len = min(int(num), int(max_len)), int(seq_len)
    if num < 1 or seq_len < 1:
        raise ValueError("clip_indices: num and seq_len are >= 1, got %d and %d" % (num, seq_len))
    if sample == "all":
        return np.arange(num, dtype=np.int64)
    if sample == "evenly":
        if num >= seq_len:
            num -= num % seq_len
            return np.arange(0, num, num / seq_len).astype(np.int64)
        return np.concatenate([np.arange(num), np.full(seq_len - num, num - 1)]).astype(np.int64)
    if sample in ("dense", "skipdense"):
        padded = np.concatenate([np.arange(num), np.full(seq_len - num % seq_len, num - 1)]).astype(np.int64)
        if sample == "dense":
            return padded
        skip = len(padded) // seq_len
        return padded.reshape(seq_len, skip).T.reshape(-1).copy()   # clip i = padded[i], padded[i + skip], ...
    raise KeyError("clip_indices covers 'evenly', 'all', 'dense' and 'skipdense' (the samplers without a random draw), got %r" % (sample,))


def _pool_segments(feats, offsets, mode, flag):
    """(rows, D) clip embeddings + segment offsets -> (segments, D). On the GPU one agrl_clip_pool_ragged launch, which also
    range-checks every row it reads into ``flag``; on the CPU ``pool_clips``' own expression per segment (the two routes agree bit
    for bit) and the check in torch. -> (pooled, flag)"""
    if feats.is_cuda:
        return ops.clip_pool_ragged(feats, np.asarray(offsets, dtype=np.int64), mode, nonfinite=flag), flag
    rows = []
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        seg = feats[lo:hi].view(1, hi - lo, feats.size(-1))
        rows.append(seg.mean(dim=1) if mode == "avg" else seg.max(dim=1)[0])
        flag = flag | (~torch.isfinite(seg).all()).to(torch.int32).reshape(1)
    return torch.cat(rows, 0), flag


@torch.no_grad()
def extract_features_packed(model, batches, clip_batch=32, pool="avg", prefetch=True, local_only=False, frame_size=None):
    """``extract_features`` for the dense protocols, where the clip count n differs from tracklet to tracklet (the reference's
    ``--test-sample dense`` / ``skipdense`` loaders at ``--test-batch 1`` plug in as they are): the same items -- (imgs (b,n,S,3,H,W) |
    (b,n,S,H,W,3), pids, camids, adj (b,n,V,V)), any b, n varying from item to item, 5-D imgs are n = 1, fp32 or uint8, with
    ``frame_size`` decoded uint8 frames of any size plus the optional valid extents (b,n,S,2) -- but the MODEL sees batches of exactly
    ``clip_batch`` clips (fewer only in the last call), whatever the tracklets' lengths: clips of consecutive items fill a staging
    buffer on the device, a tracklet may straddle buffers, and every tracklet is pooled (mean / max over its clips, ascending) by one
    segmented launch (``hip_ops.clip_pool_ragged``) once its last clip is embedded. All items of one extraction share dtype, layout,
    clip shape and adjacency shape. Returns (features (tracklets, D), pids, camids) in loader order; non-finite raw embeddings raise
    FloatingPointError and ``local_only`` means what it means for ``extract_features``. No host synchronisation before the end."""
    device = next(model.parameters()).device
    model.eval()
    clip_batch = int(clip_batch)
    if clip_batch < 1:
        raise ValueError("clip_batch is >= 1, got %d" % clip_batch)
    mode = "avg" if pool == "avg" else "max"
    cuda = device.type == "cuda"
    main = torch.cuda.current_stream(device) if cuda else None
    copy_stream = torch.cuda.Stream(device=device) if cuda and prefetch else main
    ahead = cuda and copy_stream is not main
    NBUF = 2
    frames, adjs, free = [], [], [None] * NBUF   # staging buffers and, per buffer, the event behind the model call that last read it
    ends, pids, camids = [], [], []               # per tracklet: where its clips end in the stream of all clips; labels

    def put(slot, at, flat, adjf, sizes):
        """clips -> rows at .. of staging buffer ``slot``: the H2D copy lands in the buffer itself; decoded frames are uploaded
        once and resampled into it."""
        dst, m = frames[slot][at:at + flat.shape[0]], flat.shape[0]
        with torch.cuda.stream(copy_stream) if cuda else contextlib.nullcontext():
            if ahead and flat.is_cuda:     # produced on the main stream: the copy stream reads it only behind that
                copy_stream.wait_stream(main)
                flat.record_stream(copy_stream)
                adjf.record_stream(copy_stream)
            if frame_size is None or (sizes is None and _fits_frame_size(flat.shape, frame_size)):
                dst.copy_(flat, non_blocking=True)
            else:
                _to_frame_size(flat.to(device, non_blocking=True), sizes, frame_size, out=dst)
            adjs[slot][at:at + m].copy_(adjf, non_blocking=True)

    def staged():
        """fills the staging buffers in rotation -> (slot, rows, event on the copy stream behind the buffer's last slice)"""
        fill, count, total = 0, 0, 0
        for item in batches:
            if len(item) not in ((4,) if frame_size is None else (4, 5)):
                raise ValueError("a batch is (imgs, pids, camids, adj)%s, got %d elements" % (
                    "; a fifth element, the frames' valid extents, needs frame_size" if frame_size is None else " or that plus the valid extents",
                    len(item)))
            imgs, pid, camid, adj = item[:4]
            if imgs.dim() not in (5, 6):
                raise ValueError("imgs is (b,S,...) or (b,n,S,...), got %s" % (tuple(imgs.shape),))
            b, n = (imgs.shape[0], imgs.shape[1]) if imgs.dim() == 6 else (imgs.shape[0], 1)
            flat = imgs.reshape((b * n,) + tuple(imgs.shape[-4:]))    # whichever layout the trailing axes have
            adjf = adj.reshape((b * n,) + tuple(adj.shape[(2 if imgs.dim() == 6 else 1):]))
            sizes = None
            if len(item) > 4 and item[4] is not None:
                sizes = np.asarray(item[4].cpu() if isinstance(item[4], torch.Tensor) else item[4])
                if sizes.size != b * n * flat.shape[1] * 2:
                    raise ValueError("valid extents are (b,[n,]S,2) for clips of %s, got %s" % (tuple(imgs.shape[:-3]), sizes.shape))
                sizes = sizes.reshape(b * n, flat.shape[1], 2)
            labels, cams = np.asarray(pid).reshape(-1).tolist(), np.asarray(camid).reshape(-1).tolist()
            if len(labels) != b or len(cams) != b:
                raise ValueError("%d tracklets with %d pids and %d camids" % (b, len(labels), len(cams)))
            resample = frame_size is not None and not (sizes is None and _fits_frame_size(flat.shape, frame_size))
            clip_shape = ((flat.shape[1], int(frame_size[0]), int(frame_size[1]), 3) if resample else tuple(flat.shape[1:]))
            clip_dtype = torch.uint8 if resample else flat.dtype
            if not frames:
                for _ in range(NBUF):
                    frames.append(torch.empty((clip_batch,) + clip_shape, dtype=clip_dtype, device=device))
                    adjs.append(torch.empty((clip_batch,) + tuple(adjf.shape[1:]), dtype=adjf.dtype, device=device))
                    if ahead:   # written on the copy stream: also when an error ends the extraction early, not reused under a copy
                        frames[-1].record_stream(copy_stream)
                        adjs[-1].record_stream(copy_stream)
            if (clip_shape, clip_dtype) != (tuple(frames[0].shape[1:]), frames[0].dtype) or \
                    (tuple(adjf.shape[1:]), adjf.dtype) != (tuple(adjs[0].shape[1:]), adjs[0].dtype):
                raise ValueError("the items of one packed extraction share clip shape, layout and dtype: %s %s with adj %s %s after %s %s with adj %s %s" % (
                    clip_dtype, clip_shape, adjf.dtype, tuple(adjf.shape[1:]), frames[0].dtype, tuple(frames[0].shape[1:]),
                    adjs[0].dtype, tuple(adjs[0].shape[1:])))
            for _ in range(b):
                total += n
                ends.append(total)
            pids.extend(labels)
            camids.extend(cams)
            k = 0
            while k < b * n:
                slot = count % NBUF
                if fill == 0 and ahead and free[slot] is not None:
                    copy_stream.wait_event(free[slot])
                m = min(b * n - k, clip_batch - fill)
                put(slot, fill, flat[k:k + m], adjf[k:k + m], None if sizes is None else sizes[k:k + m])
                fill, k = fill + m, k + m
                if fill == clip_batch:
                    yield slot, fill, _recorded(copy_stream) if ahead else None
                    fill, count = 0, count + 1
        if fill:
            yield slot, fill, _recorded(copy_stream) if ahead else None

    # Buffer rotation -- the one place this route can race. Two staging buffers; buffer k+1 is filled while the model call on buffer k
    # is still being enqueued / run (``pending`` below is always one buffer behind ``staged()``).
    #   * The copy stream may not WRITE a buffer before the model call that last read it is done: ``free[slot]`` is recorded on the
    #     main stream right behind that call, and ``staged()`` makes the copy stream wait for it before the buffer's first slice.
    #     (By the time buffer k+2 -- the same slot as k -- is begun, ``embed`` has run for buffer k: the event exists.)
    #   * The main stream may not READ a buffer before its last slice has landed: ``ready`` is recorded on the copy stream behind
    #     that slice (copy or resample), and the main stream waits for it in front of the model call.
    # With prefetch=False everything is enqueued on the one current stream and its order is the guarantee.
    # flag: zeroed once; the kernel only ever sets it; read once, at the end
    state = dict(carry=None, seen=0, done=0, flag=torch.zeros(1, dtype=torch.int32, device=device))
    pooled = []

    def embed(slot, rows, ready):
        if ready is not None:
            main.wait_event(ready)
        raw = model(frames[slot][:rows], adjs[slot][:rows])
        if ahead:
            free[slot] = _recorded(main)
        raw = raw.float()
        # the rows of a tracklet still open at the end of the previous buffer stand in front: every tracklet is pooled in ONE call,
        # its clips in ascending order, and every raw row is read by exactly one such call
        feats = raw if state["carry"] is None else torch.cat([state["carry"], raw], 0)
        state["seen"] += rows
        base = state["seen"] - feats.size(0)                   # the clip that row 0 of feats is: the first clip of tracklet ``done``
        t0 = t1 = state["done"]
        while t1 < len(ends) and ends[t1] <= state["seen"]:
            t1 += 1
        if t1 == t0:
            state["carry"] = feats
            return
        offsets = [0] + [ends[t] - base for t in range(t0, t1)]
        out, state["flag"] = _pool_segments(feats, offsets, mode, state["flag"])
        pooled.append(out)
        state["done"] = t1
        state["carry"] = feats[offsets[-1]:] if offsets[-1] < feats.size(0) else None

    pending = None
    for nxt in staged():
        if pending is not None:
            embed(*pending)
        pending = nxt
    if pending is not None:
        embed(*pending)
    if not pooled:
        raise ValueError("extract_features_packed: no batches")
    assert state["carry"] is None and state["done"] == len(ends)
    out = torch.cat(pooled, 0)
    _raise_if_nonfinite(model, state["flag"], out.device, local_only)
    return out, np.asarray(pids), np.asarray(camids)


def _recorded(stream):
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def _i32(a, device):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(device)


@torch.no_grad()
def match_and_rank(qf, q_pids, q_camids, gf, g_pids, g_camids, dist_metric="cosine", max_rank=50,
                   precision="fp32", return_topk=False, re_rank=False, local_only=False):
    """Distance matrix + MARS ranking on the device. ``qf``: ALL query embeddings (m,D); ``gf``: this rank's gallery
    rows when a process group is active (rows ``shard_bounds(n, rank, world)`` of the gallery), else the whole
    gallery. ``g_pids``/``g_camids`` always describe the WHOLE gallery. Returns (cmc ndarray (max_rank,), mAP float).
    ``local_only=True``: ``gf`` is the WHOLE gallery and only this rank calls -- no rank offset, no candidate all-gather,
    whatever process group is initialised."""
    device = qf.device
    world = 1 if local_only else parallel.world_size()
    if local_only and gf.size(0) != len(g_pids):
        raise ValueError("local_only=True needs the whole gallery: {} rows for {} labels".format(gf.size(0), len(g_pids)))
    n = len(g_pids)
    if max_rank > n:
        raise ValueError("max_rank={} exceeds the gallery size {}".format(max_rank, n))
    lo = parallel.shard_bounds(n, torch.distributed.get_rank(), world)[0] if world > 1 else 0

    def dist_fn(q, g):
        return hip_distmat_device(q, g, dist_metric, precision)

    def topk_fn(d, k):
        return ops.rank_topk(d, k)

    if re_rank:
        # the reference's --re-rank branch (train_vidreid_xent_htri.py:523-527): three distance matrices, k-reciprocal
        # re-ranking, then the ranking of the re-ranked matrix. Needs the whole gallery on one device.
        if world > 1:
            raise NotImplementedError("re-ranking works on the full (m+n)^2 matrix: gather the gallery embeddings first")
        q32, g32 = qf.float().contiguous(), gf.float().contiguous()
        dist = ops.re_ranking(dist_fn(q32, g32), dist_fn(q32, q32), dist_fn(g32, g32))
        idx, val = topk_fn(dist, max_rank)
        idx = idx.to(torch.int64)
    else:
        # distance + top-k fused (agrl_distmat_topk): the (m, n) matrix of the reference's test() is never materialised
        def match_fn(q, g, k):
            return hip_distmat_topk_device(q, g, dist_metric, k, precision)

        idx, val = parallel.sharded_topk(qf.float().contiguous(), gf.float().contiguous(), lo, max_rank, dist_fn, topk_fn,
                                         match_fn=match_fn if qf.is_cuda else None, local_only=local_only)
    ap, cmc = ops.rank_mars(idx.to(torch.int32).contiguous(), _i32(q_pids, device), _i32(q_camids, device),
                            _i32(g_pids, device), _i32(g_camids, device))
    ap = ap.cpu().numpy()
    if np.isnan(ap).any():
        raise ZeroDivisionError("query {} has no cross-camera match in the gallery".format(int(np.isnan(ap).argmax())))
    out = (np.mean(cmc.cpu().numpy().astype(np.float64), axis=0), float(np.mean(ap)))
    if return_topk:
        return out + (idx.cpu().numpy(), val.cpu().numpy())
    return out


@torch.no_grad()
def evaluate(model, query_batches, gallery_batches, dist_metric="cosine", pool="avg", max_rank=50,
             ranks=(1, 5, 10, 20), verbose=False, re_rank=False, clip_batch=None, frame_size=None):
    """Single-process form of the reference's ``test()``: returns (rank1, mAP) and, like the reference, can print the
    CMC table. This process extracts EVERY batch itself, so the gallery it ranks against is whole: all three stages run with
    ``local_only=True`` -- no collective anywhere, no rank offset -- and the call is safe on one rank of an initialised process
    group (``tests/test_parallel_gloo.py::test_rank0_only_evaluate``). For the sharded form every rank runs ``extract_features``
    on its slice and then ``match_and_rank`` (both collective by default).
    ``clip_batch``: an integer routes both extractions through ``extract_features_packed`` -- the dense protocols' ragged tracklets
    packed into model batches of that many clips; None (the default) is ``extract_features``. ``frame_size``: handed to the
    extraction, for decoded frames of any size (``decode_batches`` makes such batches out of JPEG bytes)."""
    if clip_batch is None:
        qf, q_pids, q_camids = extract_features(model, query_batches, pool, local_only=True, frame_size=frame_size)
        gf, g_pids, g_camids = extract_features(model, gallery_batches, pool, local_only=True, frame_size=frame_size)
    else:
        qf, q_pids, q_camids = extract_features_packed(model, query_batches, clip_batch, pool, local_only=True, frame_size=frame_size)
        gf, g_pids, g_camids = extract_features_packed(model, gallery_batches, clip_batch, pool, local_only=True, frame_size=frame_size)
    cmc, mAP = match_and_rank(qf, q_pids, q_camids, gf, g_pids, g_camids, dist_metric, max_rank,
                              getattr(model, "hip_precision", "fp32"), re_rank=re_rank, local_only=True)
    if verbose:
        print("Results ----------")
        print("mAP: {:.2%}".format(mAP))
        print("CMC curve")
        for r in ranks:
            print("Rank-{:<3}: {:.2%}".format(r, cmc[r - 1]))
        print("------------------")
    return cmc[0], mAP
