#!/usr/bin/env python
"""agrl_jpeg_decode_u8 at 256 frames of 256x128 (4:2:0, quality 75 and 95), beside what it replaces and what it rides along with:

  * the device decode of the batch, and each of its three stages alone (entropy decode, IDCT, upsampling + colour);
  * the upload of the compressed bytes against the upload of the decoded frames (pinned memory, one copy each);
  * Pillow decoding the same files on 16 threads of the same host (the threads a job may use: NOT os.cpu_count());
  * the forward of the same frames (vmgn, the library's 16-bit mode, 32 clips of 8);
  * the decode on a second stream under a running forward: what the pair takes over the forward alone.

    python tools/jpeg_decode_bench.py [--frames 256] [--blocks 5] [--iters 20] [--out profiles/jpeg_decode_bench.txt]

Device times are HIP events around ``iters`` back-to-back calls (operands uploaded once), ``blocks`` times per variant, the variants
alternating block by block, one process, one machine; medians of the blocks. The frames are synthetic (smooth shapes plus sensor-like
noise, so that a quality-75 file is the 5-10 KB of a real 256x128 crop) and encoded by Pillow here: the tool needs Pillow and a GPU."""
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

H, W = 256, 128
THREADS = 16
STEP_MS = 3.6          # the 256-frame eval step the shares are given against


def frames_like_crops(n, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for _ in range(n):
        ph = rng.uniform(0, 6.28, 9)
        ch = [127 + 70 * np.sin(x / rng.uniform(6, 30) + ph[c]) * np.cos(y / rng.uniform(8, 40) + ph[c + 3]) +
              30 * np.sign(np.sin(x / 9 + y / 13 + ph[c + 6])) + rng.normal(0, 6.0, (H, W)) for c in range(3)]
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_decode_bench needs a GPU: a timing has no CPU fallback")
    import PIL
    from PIL import Image
    from torchreid import device_decode as dd, hip_ops as ops, models
    dev = torch.device("cuda:0")
    N = args.frames
    assert N % 8 == 0
    lines = ["%s, torch %s, Pillow %s; %d frames of %dx%d 4:2:0 per batch, %d blocks x %d calls per variant, alternating; HIP events; "
             "shares of a %.1f ms step" % (torch.cuda.get_device_name(0), torch.__version__, PIL.__version__, N, H, W, args.blocks,
                                           args.iters, STEP_MS)]
    m = models.init_model("vmgn", num_classes=8, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1,
                          pyramid_part=True, use_pose=True, learn_graph=True).to(dev).eval()
    m.hip_precision = ops.LP_NAME
    adj = (torch.rand((N // 8, 56, 56), generator=torch.Generator().manual_seed(1)) < 0.3).float().to(dev)
    side = torch.cuda.Stream(device=dev)
    pixels = frames_like_crops(N, 7)
    for quality in (75, 95):
        files = []
        for px in pixels:
            buf = io.BytesIO()
            Image.fromarray(px).save(buf, "JPEG", quality=quality, subsampling=2)
            files.append(buf.getvalue())
        plan = dd.jpeg_batch_plan([dd.parse_jpeg(f) for f in files])
        operands = ops.jpeg_upload(plan, dev)
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
        ws = torch.empty((ops.jpeg_workspace_bytes(plan),), dtype=torch.uint8, device=dev)
        status = torch.empty((N,), dtype=torch.int32, device=dev)
        desc_h = np.ascontiguousarray(plan.desc)

        def decode(stages=ops.JPEG_STAGE_ALL, stream=None):
            ops.call("agrl_jpeg_decode_u8", operands[0].data_ptr(), operands[0].numel(), desc_h.ctypes.data, operands[1].data_ptr(), N,
                     operands[2].data_ptr(), operands[2].shape[0], operands[3].data_ptr(), operands[3].shape[0], ws.data_ptr(), ws.numel(),
                     out.data_ptr(), H, W, status.data_ptr(), stages, (stream or torch.cuda.current_stream(dev)).cuda_stream)

        decode()
        torch.cuda.synchronize()
        want = np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files[:8]])
        exact = bool(not status.cpu().any()) and np.array_equal(out[:8].cpu().numpy(), want)   # what is timed is also right
        clips = out.view(N // 8, 8, H, W, 3)
        forward = lambda: m(clips, adj)
        forward()
        torch.cuda.synchronize()

        def both():
            side.wait_stream(torch.cuda.current_stream(dev))
            decode(stream=side)
            forward()
            torch.cuda.current_stream(dev).wait_stream(side)

        compressed = torch.from_numpy(plan.scans).pin_memory()
        decoded = torch.from_numpy(np.stack(pixels)).pin_memory()
        c_dev, d_dev = torch.empty_like(compressed, device=dev), torch.empty_like(decoded, device=dev)
        variants = [("device decode, all three stages", decode), ("  entropy decode alone", lambda: decode(ops.JPEG_STAGE_ENTROPY)),
                    ("  IDCT alone", lambda: decode(ops.JPEG_STAGE_IDCT)), ("  upsampling + colour alone", lambda: decode(ops.JPEG_STAGE_COLOUR)),
                    ("upload of the compressed scans (%.2f MB)" % (compressed.numel() / 1e6), lambda: c_dev.copy_(compressed, non_blocking=True)),
                    ("upload of the decoded frames (%.2f MB)" % (decoded.numel() / 1e6), lambda: d_dev.copy_(decoded, non_blocking=True)),
                    ("forward of the same frames (%s)" % ops.LP_NAME, forward), ("forward + decode on a second stream", both)]
        for _, fn in variants:
            for _ in range(3):
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
            dd.jpeg_batch_plan([dd.parse_jpeg(f) for f in files])
        host_ms = (time.perf_counter() - t0) / 3 * 1e3
        lines.append("quality %d: %.1f KB a file (scan %.1f KB), %d quantisation + %d Huffman tables in the batch  [first 8 frames %s Pillow's]" % (
            quality, np.mean([len(f) for f in files]) / 1e3, plan.desc[:, ops.JD_LEN].mean() / 1e3, len(plan.quant), len(plan.huff),
            "==" if exact else "!="))
        med = [float(np.median(b)) for b in per]
        for (name, _), blocks, ms in zip(variants, per, med):
            lines.append("  %-46s %8.4f ms (blocks %s) = %8.1f k frames/s = %5.1f %% of the step" % (
                name, ms, " ".join("%.4f" % b for b in blocks), N / ms, 100 * ms / STEP_MS))
        lines.append("  %-46s %8.4f ms over the forward alone" % ("  the decode under the forward costs", med[7] - med[6]))
        ms = float(np.median(pillow))
        lines.append("  %-46s %8.4f ms (blocks %s) = %8.1f k frames/s  [wall clock, ThreadPoolExecutor(%d)]" % (
            "Pillow, %d threads, the same files" % THREADS, ms, " ".join("%.2f" % b for b in pillow), N / ms, THREADS))
        lines.append("  %-46s %8.4f ms = %8.1f k frames/s  [wall clock, one thread, pure Python]" % ("host side: parse_jpeg + jpeg_batch_plan", host_ms, N / host_ms))
        lines.append("  the device decode is %.2f x 16-thread Pillow" % (ms / med[0]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
