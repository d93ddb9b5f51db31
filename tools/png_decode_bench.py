#!/usr/bin/env python
"""agrl_png_decode_u8 at 256 RGB frames of 64x128 (the two PNG datasets' size) and of 256x128, beside what it replaces and what it
rides along with:

  * the device decode of the batch, and its parts (inflate alone; inflate + the row filters; all three with the store);
  * the upload of the compressed bytes against the upload of the decoded frames (pinned memory, one copy each);
  * Pillow decoding the same files on 16 threads of the same host (the threads a job may use: NOT os.cpu_count());
  * agrl_diag_read_stream over the output bytes: what a kernel bound by writing the frames would be near;
  * the forward of the same frames (vmgn, the library's 16-bit mode, clips of 8).

    python tools/png_decode_bench.py [--frames 256] [--blocks 5] [--iters 10] [--out profiles/png_decode_bench.txt]

Device times are HIP events around ``iters`` back-to-back calls (operands uploaded once), ``blocks`` times per variant, the variants
alternating block by block, one process, one machine; medians of the blocks. The first 8 frames are compared with Pillow before anything
is timed. The frames are synthetic (smooth shapes plus sensor-like noise) and encoded by Pillow here at its default settings: the tool
needs Pillow and a GPU."""
import argparse
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "agrl.pytorch_amd")]

THREADS = 16


def frames_like_crops(n, H, W, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for _ in range(n):
        ph = rng.uniform(0, 6.28, 9)
        ch = [127 + 70 * np.sin(x / rng.uniform(6, 30) + ph[c]) * np.cos(y / rng.uniform(8, 40) + ph[c + 3]) +
              30 * np.sign(np.sin(x / 9 + y / 13 + ph[c + 6])) + rng.normal(0, 2.0, (H, W)) for c in range(3)]
        out.append(np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8))
    return out


def device_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_decode_bench needs a GPU: a timing has no CPU fallback")
    import PIL
    from PIL import Image
    from torchreid import device_decode as dd, hip_ops as ops, models
    dev = torch.device("cuda:0")
    N = args.frames
    assert N % 8 == 0
    lines = ["%s, torch %s, Pillow %s; %d RGB frames per batch, Pillow's default PNG encoding, %d blocks x %d calls per variant, alternating; "
             "HIP events" % (torch.cuda.get_device_name(0), torch.__version__, PIL.__version__, N, args.blocks, args.iters)]
    m = models.init_model("vmgn", num_classes=8, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1,
                          pyramid_part=True, use_pose=True, learn_graph=True).to(dev).eval()
    m.hip_precision = ops.LP_NAME
    adj = (torch.rand((N // 8, 56, 56), generator=torch.Generator().manual_seed(1)) < 0.3).float().to(dev)
    for H, W in ((64, 128), (256, 128)):
        pixels = frames_like_crops(N, H, W, 7)
        files = []
        for px in pixels:
            buf = io.BytesIO()
            Image.fromarray(px).save(buf, "PNG")
            files.append(buf.getvalue())
        plan = dd.png_batch_plan([dd.parse_png(f) for f in files])
        operands = ops.png_upload(plan, dev)
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
        status = torch.empty((N,), dtype=torch.int32, device=dev)
        desc_h = np.ascontiguousarray(plan.desc)

        def decode(stages=ops.PNG_STAGE_ALL):
            ops.call("agrl_png_decode_u8", operands[0].data_ptr(), operands[0].numel(), desc_h.ctypes.data, operands[1].data_ptr(), N,
                     out.data_ptr(), H, W, status.data_ptr(), stages, torch.cuda.current_stream(dev).cuda_stream)

        decode()
        torch.cuda.synchronize()
        want = np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files[:8]])
        exact = bool(not status.cpu().any()) and np.array_equal(out[:8].cpu().numpy(), want)   # what is timed is also right
        if (H, W) == (256, 128):
            clips = out.view(N // 8, 8, H, W, 3)
            forward = lambda: m(clips, adj)
        else:                                                       # the model's input: these frames resampled to 256x128 on the device
            from torchreid.device_transforms import DeviceClipTransform
            tf = DeviceClipTransform(256, 128)
            sizes = np.tile(np.array([H, W], dtype=np.int64), (N // 8, 8, 1))
            forward = lambda: m(tf(out.view(N // 8, 8, H, W, 3), sizes), adj)
        forward()
        torch.cuda.synchronize()
        compressed = torch.from_numpy(plan.streams).pin_memory()
        decoded = torch.from_numpy(np.stack(pixels)).pin_memory()
        c_dev, d_dev = torch.empty_like(compressed, device=dev), torch.empty_like(decoded, device=dev)
        variants = [("device decode, everything", decode), ("  inflate alone", lambda: decode(ops.PNG_STAGE_INFLATE)),
                    ("  inflate + row filters", lambda: decode(ops.PNG_STAGE_INFLATE | ops.PNG_STAGE_FILTER)),
                    ("upload of the compressed streams (%.2f MB)" % (compressed.numel() / 1e6), lambda: c_dev.copy_(compressed, non_blocking=True)),
                    ("upload of the decoded frames (%.2f MB)" % (decoded.numel() / 1e6), lambda: d_dev.copy_(decoded, non_blocking=True)),
                    ("agrl_diag_read_stream over the output bytes", lambda: ops.read_stream(out)),
                    ("forward of the same frames (%s%s)" % (ops.LP_NAME, "" if (H, W) == (256, 128) else ", resample included"), forward)]
        for _, fn in variants:
            fn()
        torch.cuda.synchronize()
        per = [[] for _ in variants]
        for _ in range(args.blocks):
            for i, (_, fn) in enumerate(variants):
                per[i].append(device_ms(fn, args.iters))
        with ThreadPoolExecutor(THREADS) as pool:
            one = lambda f: np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
            list(pool.map(one, files))
            pillow = []
            for _ in range(args.blocks):
                t0 = time.perf_counter()
                list(pool.map(one, files))
                pillow.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for _ in range(3):
            dd.png_batch_plan([dd.parse_png(f) for f in files])
        host_ms = (time.perf_counter() - t0) / 3 * 1e3
        lines.append("%dx%d: %.1f KB a file (zlib stream %.1f KB, inflated %.1f KB)  [first 8 frames %s Pillow's]" % (
            H, W, np.mean([len(f) for f in files]) / 1e3, plan.desc[:, ops.PD_LEN].mean() / 1e3, ops.png_frame_inflated(H, W, 3) / 1e3,
            "==" if exact else "!="))
        med = [float(np.median(b)) for b in per]
        for (name, _), blocks, ms in zip(variants, per, med):
            lines.append("  %-52s %9.4f ms (blocks %s) = %8.1f k frames/s" % (name, ms, " ".join("%.4f" % b for b in blocks), N / ms))
        ms = float(np.median(pillow))
        lines.append("  %-52s %9.4f ms (blocks %s) = %8.1f k frames/s  [wall clock, ThreadPoolExecutor(%d)]" % (
            "Pillow, %d threads, the same files" % THREADS, ms, " ".join("%.2f" % b for b in pillow), N / ms, THREADS))
        lines.append("  %-52s %9.4f ms = %8.1f k frames/s  [wall clock, one thread, pure Python]" % ("host side: parse_png + png_batch_plan", host_ms, N / host_ms))
        lines.append("  the device decode takes %.2f x the time of 16-thread Pillow, %.1f x the read stream's, %.2f x the forward's" % (
            med[0] / ms, med[0] / med[5], med[0] / med[6]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
