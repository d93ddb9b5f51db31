"""The ``sta`` eval forward at 32 tracklets x 8 frames of 256 x 128 in the library's 16-bit mode, timed in ONE process with the two
routes alternating block by block:

  (n) the native forward: _sta_hip.hip_forward_sta (stem, conv trunk, agrl_sta_frame_stats, agrl_sta_fuse, agrl_linear_bn_relu)
  (s) the same model's stock-torch module tree on the same GPU (fp32; what the model would run without the HIP route)

and each new kernel alone at the forward's shape, one HIP event pair around each call through its wrapper: agrl_sta_frame_stats
(F = 256 frames, 16 x 8 x 2048 map of the 16-bit type: 134 MB read once) beside csrc/diag.hip's read stream over the same byte count
in the same run, agrl_sta_fuse in both modes, agrl_linear_bn_relu (32 x 4096 -> 1024, 16-bit and fp32 weight) with the bytes of its
weight stream.

Per forward one HIP event pair; a block is --steps forwards, the figure the median of the --blocks block means. GPU only: without one
the script exits non-zero.

usage: python tools/sta_bench.py [--steps 5] [--blocks 3] [--warmup 2] [--out profiles/sta_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "agrl.pytorch_amd"), os.path.join(ROOT, "tests")]
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--kernel-calls", type=int, default=30)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("sta_bench: no GPU -- this tool measures on the device and has no CPU form")

from recipe import recipe_state_dict
from torchreid import hip_ops as ops
from torchreid import models
from torchreid.models._sta_hip import hip_forward_sta

dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


B, S = 32, 8
m = models.init_model("sta", num_classes=625, loss={"xent", "htri"}, last_stride=1, pretrained=False)
m.load_state_dict(recipe_state_dict(m.state_dict(), seed=4))
m = m.eval().to(dev)
m.hip_precision = ops.LP_NAME
gen = torch.Generator(device=dev)
gen.manual_seed(4)
x = torch.randn((B, S, 3, 256, 128), device=dev, generator=gen)


def stock(frames):
    with torch.no_grad():
        return m.fc1(m.fused_feature(frames)[0])


def run(native, steps, sink):
    pairs, out = [], None
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = hip_forward_sta(m, x) if native else stock(x)
        e.record()
        pairs.append((s, e))
    torch.cuda.synchronize()
    if sink is not None:
        sink.append(sum(s.elapsed_time(e) for s, e in pairs) / steps)
    return out


times = {True: [], False: []}
outs = {}
for native in (True, False):
    run(native, args.warmup, None)
for _ in range(args.blocks):
    for native in (True, False):
        outs[native] = run(native, args.steps, times[native])
err = float((outs[True].double() - outs[False].double()).abs().max() / outs[False].double().abs().max())

say("sta eval forward: %d tracklets x %d frames of 256 x 128, hip_precision = %s against the stock-torch module tree (fp32) on the same GPU" % (
    B, S, ops.LP_NAME))
say("%s, torch %s; %d blocks x %d forwards per route, alternating, %d warm-up forwards each; one HIP event pair per forward" % (
    torch.cuda.get_device_name(0), torch.__version__, args.blocks, args.steps, args.warmup))
for native, name in ((True, "(n) native forward (_sta_hip)"), (False, "(s) stock-torch module tree")):
    say("%-34s %8.3f ms per forward (block means %s)" % (name, statistics.median(times[native]), " ".join("%.3f" % t for t in times[native])))
t_n, t_s = statistics.median(times[True]), statistics.median(times[False])
say("native / stock = %.3f (%s); outputs differ by %.2e max-normalised" % (t_n / t_s, "native is faster" if t_n < t_s else "native is NOT faster", err))


def time_calls(fn):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(args.kernel_calls):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms), min(ms), max(ms)


# ---- the new kernels alone, at the forward's shape
F_, h, w, C = B * S, 16, 8, 2048
fmap = (torch.randn((F_, h, w, C), device=dev, generator=gen).abs() * 0.5).to(ops.LP_DTYPE)
map_bytes = fmap.numel() * fmap.element_size()
vmean, nsum, nsq = ops.sta_frame_stats(fmap)
f_g, _, _ = ops.sta_fuse(vmean, B, S, nsum, nsq, (h, w))
wf = torch.randn((1024, 2 * C), device=dev, generator=gen) * 0.02
scale, shift = torch.rand(1024, device=dev, generator=gen) + 0.5, torch.randn(1024, device=dev, generator=gen)
w16 = wf.to(ops.LP_DTYPE)
rows = [
    ("agrl_sta_frame_stats", lambda: ops.sta_frame_stats(fmap), map_bytes + vmean.numel() * 4),
    ("agrl_diag_read_stream (same bytes)", lambda: ops.read_stream(fmap), map_bytes),
    ("agrl_sta_fuse (map)", lambda: ops.sta_fuse(vmean, B, S, nsum, nsq, (h, w)), vmean.numel() * 4 + f_g.numel() * 4),
    ("agrl_sta_fuse (norm)", lambda: ops.sta_fuse(vmean, B, S), vmean.numel() * 4 + f_g.numel() * 4),
    ("agrl_linear_bn_relu (16-bit weight)", lambda: ops.linear_bn_relu(f_g, w16, scale, shift), w16.numel() * 2 + f_g.numel() * 4),
    ("agrl_linear_bn_relu (fp32 weight)", lambda: ops.linear_bn_relu(f_g, wf, scale, shift), wf.numel() * 4 + f_g.numel() * 4),
]
say("kernels alone, F = %d frames, %d x %d x %d map (%s), M = %d tracklets; median of %d calls through the wrapper (allocations included)" % (
    F_, h, w, C, ops.LP_NAME, B, args.kernel_calls))
for name, fn, nbytes in rows:
    med, lo, hi = time_calls(fn)
    say("%-38s median %8.2f us (min %.2f, max %.2f) | %.2f MB algorithmic = %.2f TB/s" % (
        name, med * 1e3, lo * 1e3, hi * 1e3, nbytes / 1e6, nbytes / med / 1e9))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
