"""The dense test protocol on a RAGGED split, the two routes of torchreid/evaluation.py in ONE process, alternating block by block:

  (t) per tracklet: ``extract_features`` on one-tracklet items (the reference's --test-sample dense at --test-batch 1): one model call
      per tracklet, on however many clips it has
  (p) packed:       ``extract_features_packed(clip_batch=32)``: the same items, the model called on 32 clips at a time

Workload: ``vmgn`` in the library's 16-bit mode, seq_len 8, uint8 channel-last frames of 256 x 128 in pinned host memory (what a decoder
hands over), all-ones adjacency. The split is SYNTHETIC and seeded: tracklet lengths L = round(exp(N(log 48, 0.7))) frames, clipped to
8 .. 400, and n = L // 8 + 1 clips (the dense sampler's count at seq_len 8, its extra clip included). MARS's real length histogram is
not available here: this distribution is ASSUMED, not measured, and the file this tool writes says so.

A block is one whole extraction (upload, forward, pooling, the one flag read at the end). Device time: one HIP event pair around the
block; host time: a clock around the block and around every model call (a call returns when its kernels are enqueued, so that part is
the host's enqueue time per step). The figure of a route is the median over --blocks blocks. GPU only: without one the script exits
non-zero.

usage: python tools/dense_eval_bench.py [--tracklets 192] [--blocks 5] [--warmup 1] [--out profiles/dense_eval_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "agrl.pytorch_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--tracklets", type=int, default=192)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--clip-batch", type=int, default=32)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_eval_bench.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("dense_eval_bench: no GPU -- this tool measures on the device and has no CPU form")

from recipe import recipe_state_dict
from torchreid import evaluation
from torchreid import hip_ops as ops
from torchreid import models

dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


S, H, W, V = 8, 256, 128, 56
rng = np.random.RandomState(args.seed)
frames = np.clip(np.rint(np.exp(rng.normal(np.log(48.0), 0.7, args.tracklets))), 8, 400).astype(np.int64)
clips = (frames // S + 1).astype(np.int64)
gen = torch.Generator().manual_seed(args.seed)
items = []
for i, n in enumerate(clips.tolist()):
    x = torch.randint(0, 256, (1, n, S, H, W, 3), generator=gen, dtype=torch.uint8).pin_memory()
    items.append((x, torch.tensor([i]), torch.tensor([i % 6]), torch.ones((1, n, V, V)).pin_memory()))
total_clips = int(clips.sum())

m = models.init_model("vmgn", num_classes=625, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1,
                      pyramid_part=True, use_pose=True, learn_graph=True)
m.load_state_dict(recipe_state_dict(m.state_dict(), seed=0))
m = m.eval().to(dev)
m.hip_precision = ops.LP_NAME

in_forward = []
plain_forward = m.forward


def timed_forward(*a, **kw):
    t = time.perf_counter()
    out = plain_forward(*a, **kw)
    in_forward.append(time.perf_counter() - t)
    return out


m.forward = timed_forward
ROUTES = {"t": lambda: evaluation.extract_features(m, items, pool="avg", local_only=True),
          "p": lambda: evaluation.extract_features_packed(m, items, clip_batch=args.clip_batch, pool="avg", local_only=True)}


def block(route, sink):
    del in_forward[:]
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.record()
    feats, _, _ = ROUTES[route]()
    e.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    if sink is not None:
        sink.append(dict(dev_ms=s.elapsed_time(e), wall_ms=wall * 1e3, steps=len(in_forward), fwd_ms=sum(in_forward) * 1e3))
    return feats


res = {"t": [], "p": []}
outs = {}
for _ in range(args.warmup):
    for route in ("t", "p"):
        block(route, None)
for _ in range(args.blocks):
    for route in ("t", "p"):
        outs[route] = block(route, res[route])
err = float((outs["t"].double() - outs["p"].double()).abs().max() / outs["t"].double().abs().max())

hist = np.bincount(clips)
say("dense protocol, ragged split: vmgn, hip_precision = %s, seq_len %d, uint8 channel-last %d x %d frames from pinned host memory" % (ops.LP_NAME, S, H, W))
say("%s, torch %s; %d blocks per route, alternating, %d warm-up block(s) each; a block = one whole extraction; one HIP event pair and one host clock per block" % (
    torch.cuda.get_device_name(0), torch.__version__, args.blocks, args.warmup))
say("split (SYNTHETIC, seed %d; the length distribution is ASSUMED -- MARS's real histogram was not available -- not measured): %d tracklets, "
    "L = round(exp(N(log 48, 0.7))) frames clipped to 8 .. 400, n = L // %d + 1 clips" % (args.seed, args.tracklets, S))
say("  clips per tracklet: min %d, median %d, mean %.2f, max %d; %d clips = %d frames in all" % (
    clips.min(), int(np.median(clips)), clips.mean(), clips.max(), total_clips, total_clips * S))
say("  histogram (clips: tracklets): " + ", ".join("%d: %d" % (n, c) for n, c in enumerate(hist.tolist()) if c))
for route, name in (("t", "(t) per tracklet (extract_features, one-tracklet items)"), ("p", "(p) packed (extract_features_packed, clip_batch=%d)" % args.clip_batch)):
    r = res[route]
    dev_ms = statistics.median(b["dev_ms"] for b in r)
    wall_ms = statistics.median(b["wall_ms"] for b in r)
    steps = r[0]["steps"]
    fwd = statistics.median(b["fwd_ms"] / b["steps"] for b in r)
    rest = statistics.median((b["wall_ms"] - b["fwd_ms"]) / b["steps"] for b in r)
    say("%-58s %9.1f frames/s | device %8.2f ms per extraction (blocks %s), host wall %8.2f ms" % (
        name, total_clips * S / dev_ms * 1e3, dev_ms, " ".join("%.2f" % b["dev_ms"] for b in r), wall_ms))
    say("%-58s %d model calls (steps); host per step: %.3f ms inside the model call (enqueue), %.3f ms around it (staging, pooling, waiting)" % (
        "", steps, fwd, rest))
t_t, t_p = statistics.median(b["dev_ms"] for b in res["t"]), statistics.median(b["dev_ms"] for b in res["p"])
say("packed / per tracklet = %.3f in device time (%s); the two routes' features differ by %.2e max-normalised (%s forwards at different batch sizes)" % (
    t_p / t_t, "packed is faster" if t_p < t_t else "packed is NOT faster", err, ops.LP_NAME))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
