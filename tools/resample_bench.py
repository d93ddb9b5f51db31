#!/usr/bin/env python
"""agrl_clip_resample_u8 at 256 frames, beside the two things it stands between: a pure read stream over the same byte count
(agrl_diag_read_stream, the HBM yardstick of the streaming kernels) and Pillow doing the same resizes on 16 host threads.

    python tools/resample_bench.py [--frames 256] [--blocks 5] [--iters 200] [--out profiles/clip_resample_bench.txt]

Three cases, all to the model's 256x128: frames already that size (both passes are the identity: a copy), the training recipe's
240x120 random-crop window of a 256x128 frame, and 128x64 frames (iLIDS-VID, PRID). Device times are HIP events around ``iters``
back-to-back launches, ``blocks`` times per variant, the variants alternating; the byte count of a case is what the algorithm needs: the
source windows once plus the output once. Needs a GPU: there is no CPU fallback for a timing."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "agrl.pytorch_amd")]

OUT_HW = (256, 128)


def cases(N):
    """(name, (Hs, Ws), geometry (N, 8))"""
    rng = np.random.default_rng(0)
    whole = lambda h, w: np.array([[h, w, 0, 0, h, w, 0, 0]] * N, dtype=np.int32)
    crop = whole(256, 128)
    crop[:, 2], crop[:, 3], crop[:, 4], crop[:, 5] = rng.integers(0, 17, N), rng.integers(0, 9, N), 240, 120
    return [("256x128 -> 256x128 (identity)", (256, 128), whole(256, 128)),
            ("240x120 window -> 256x128", (256, 128), crop),
            ("128x64 -> 256x128", (128, 64), whole(128, 64))]


def device_ms(fn, blocks, iters):
    """Median over ``blocks`` of the mean time of ``iters`` back-to-back calls, HIP events on the current stream."""
    out = []
    for _ in range(blocks):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        end.synchronize()
        out.append(start.elapsed_time(end) / iters)
    return float(np.median(out)), out


def pillow_frames_per_s(frames, geometry, threads=16, repeats=3):
    try:
        from PIL import Image
    except ImportError:
        return None
    imgs = [Image.fromarray(f) for f in frames]

    def one(i):
        sh, sw, y0, x0, wh, ww = (int(v) for v in geometry[i][:6])
        img = imgs[i]
        if (x0, y0, ww, wh) != (0, 0, sw, sh):
            img = img.crop((x0, y0, x0 + ww, y0 + wh))
        return img.resize((OUT_HW[1], OUT_HW[0]), Image.BILINEAR)

    best = 0.0
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(one, range(len(imgs))))
        for _ in range(repeats):
            t0 = time.perf_counter()
            list(pool.map(one, range(len(imgs))))
            best = max(best, len(imgs) / (time.perf_counter() - t0))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_resample_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs a GPU: a timing has no CPU fallback")
    from torchreid import _hip, hip_ops as ops
    dev = torch.device("cuda:0")
    N = args.frames
    lines = ["%s, torch %s; %d frames per launch, %d blocks x %d launches per variant, alternating; HIP events" % (
        torch.cuda.get_device_name(0), torch.__version__, N, args.blocks, args.iters)]
    for name, (Hs, Ws), geo in cases(N):
        host = torch.randint(0, 256, (N, Hs, Ws, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
        frames = host.to(dev)
        out = torch.empty((N,) + OUT_HW + (3,), dtype=torch.uint8, device=dev)
        ops.clip_resample(frames, geo, OUT_HW, out=out)
        same = torch.equal(out[:4].cpu(), ops.clip_resample_reference(host[:4], geo[:4], OUT_HW))
        # the launch alone: geometry uploaded once, as a captured graph would replay it
        geo_d = torch.from_numpy(geo).to(dev)
        stream = _hip.stream_ptr(dev)
        launch = lambda: _hip.call("agrl_clip_resample_u8", frames.data_ptr(), geo_d.data_ptr(), out.data_ptr(), N, Hs, Ws,
                                   OUT_HW[0], OUT_HW[1], stream)
        wrapped = lambda: ops.clip_resample(frames, geo, OUT_HW, out=out)
        nbytes = int(geo[:, 4].astype(np.int64) @ geo[:, 5].astype(np.int64)) * 3 + out.numel()
        buf = torch.empty((max(nbytes, 1 << 20) + 15) // 16 * 4, dtype=torch.float32, device=dev).normal_()
        read = lambda: ops.read_stream(buf, nbytes)
        for fn in (launch, wrapped, read):
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        per = {k: [] for k in ("launch", "wrapped", "read")}
        for _ in range(args.blocks):   # the variants alternate block by block
            for k, fn in (("launch", launch), ("wrapped", wrapped), ("read", read)):
                per[k].extend(device_ms(fn, 1, args.iters)[1])
        res = {k: (float(np.median(v)), v) for k, v in per.items()}
        pil = pillow_frames_per_s(host.numpy(), geo)
        lines.append("%s  [first 4 frames %s the reference]" % (name, "==" if same else "!="))
        lines.append("  bytes the algorithm needs (windows + output): %.2f MB" % (nbytes / 1e6))
        for k, label in (("launch", "agrl_clip_resample_u8, the launch alone"), ("wrapped", "hip_ops.clip_resample (check + upload + launch)"),
                         ("read", "agrl_diag_read_stream over the same bytes")):
            ms, blocks = res[k]
            lines.append("  %-52s %8.4f ms (blocks %s) = %7.1f k frames/s = %6.2f TB/s algorithmic" % (
                label, ms, " ".join("%.4f" % b for b in blocks), N / ms, nbytes / ms / 1e9))
        lines.append("  the kernel takes %.1f x the read stream's time" % (res["launch"][0] / res["read"][0]))
        lines.append("  Pillow, 16 host threads: %s" % ("%.1f k frames/s" % (pil / 1e3) if pil else "not measured (PIL is not installed)"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
