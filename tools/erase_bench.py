#!/usr/bin/env python
"""agrl_frames_normalize_erase_u8 at 256 frames of 256x128, beside the launch it extends: agrl_frames_normalize_u8 (unchanged: the
yardstick), the new entry with every count zero, and the new entry with the rectangles ``device_transforms.erase_geometry`` draws in
the 'all' (GroupRandomErasing: every fitting attempt of 100) and 'first' (RandomErasing: one rectangle) modes at probability 0.5 and 1.

    python tools/erase_bench.py [--frames 256] [--blocks 5] [--iters 200] [--out profiles/frames_erase_bench.txt]

Both layouts. Device times are HIP events around ``iters`` back-to-back launches of the entry point alone (the lists uploaded once, as a
captured graph would replay them), ``blocks`` times per variant, the variants alternating block by block, one process. The byte count
is what the algorithm needs: the uint8 frames once plus the fp32 output once. Needs a GPU: there is no CPU fallback for a timing."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "agrl.pytorch_amd")]

H, W = 256, 128


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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_erase_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("erase_bench needs a GPU: a timing has no CPU fallback")
    from torchreid import _hip, hip_ops as ops
    from torchreid.device_transforms import erase_geometry
    dev = torch.device("cuda:0")
    N = args.frames
    stream = _hip.stream_ptr(dev)
    table = ops._device_frame_table(dev, ops.PIXEL_MEAN, ops.PIXEL_STD)
    host = torch.randint(0, 256, (N, 3, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
    nbytes = host.numel() + 4 * out.numel()
    lists = [("every count zero", erase_geometry(N, H, W, 0, probability=0.0))]
    lists += [("'%s', probability %.1f" % (mode, p), erase_geometry(N, H, W, 0, probability=p, attempts=mode))
              for mode in ("all", "first") for p in (0.5, 1.0)]
    lines = ["%s, torch %s; %d frames of %dx%d per launch, %d blocks x %d launches per variant, alternating; HIP events" % (
        torch.cuda.get_device_name(0), torch.__version__, N, H, W, args.blocks, args.iters),
        "bytes the algorithm needs (uint8 in + fp32 out): %.2f MB" % (nbytes / 1e6)]
    for layout, code in (("nchw", _hip.FRAMES_NCHW), ("nhwc", _hip.FRAMES_NHWC)):
        frames = (host if layout == "nchw" else host.movedim(1, -1).contiguous()).to(dev)
        plain = lambda: _hip.call("agrl_frames_normalize_u8", frames.data_ptr(), table.data_ptr(), code, out.data_ptr(), N, H, W, stream)
        variants = [("agrl_frames_normalize_u8 (the yardstick)", plain, None)]
        keep = []
        for name, (rects, counts) in lists:
            r, c = ops.erase_lists(rects, counts, N, H, W)
            r_d, c_d = torch.from_numpy(r).to(dev), torch.from_numpy(c).to(dev)
            keep.append((r_d, c_d))
            fn = (lambda r_d=r_d, c_d=c_d, R=r.shape[1]: _hip.call(
                "agrl_frames_normalize_erase_u8", frames.data_ptr(), table.data_ptr(), code, r_d.data_ptr(), c_d.data_ptr(), R,
                *ops.PIXEL_MEAN, out.data_ptr(), N, H, W, stream))
            variants.append(("erase, " + name, fn, (rects, counts)))
        same = []
        for name, fn, erase in variants:   # what is timed is also right: the first 4 frames against the reference
            out.fill_(float("nan"))
            fn()
            ref = ops.frames_normalize_reference(host[:4]) if erase is None else \
                ops.frames_normalize_erase_reference(host[:4], erase[0][:4], erase[1][:4])
            same.append(torch.equal(out[:4].cpu(), ref))
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        per = [[] for _ in variants]
        for _ in range(args.blocks):   # the variants alternate block by block
            for i, (_, fn, _) in enumerate(variants):
                per[i].append(device_ms(fn, args.iters))
        base = float(np.median(per[0]))
        lines.append("%s frames" % layout)
        for (name, _, erase), blocks, ok in zip(variants, per, same):
            ms = float(np.median(blocks))
            what = "" if erase is None else "; %.1f rectangles a frame, at most %d" % (float(erase[1].mean()), int(erase[1].max()))
            lines.append("  %-44s %8.4f ms (blocks %s) = %7.1f k frames/s = %5.2f TB/s algorithmic = %5.2f x the yardstick%s  [first 4 "
                         "frames %s the reference]" % (name, ms, " ".join("%.4f" % b for b in blocks), N / ms, nbytes / ms / 1e9,
                                                      ms / base, what, "==" if ok else "!="))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
