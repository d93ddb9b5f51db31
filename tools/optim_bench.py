"""The optimiser update of vmgn (702 classes, ~47 M fp32 parameters) under GradientBuckets, timed in ONE process with the variants
alternating block by block:

  (a) torch.optim.Adam, torch's default implementation, + GradientBuckets.zero_grad() (the memset of the flat buffers)
  (b) the same with fused=True, where this torch offers it
  (c) torchreid.hip_optim.HipAdam with zero_grads=True (one agrl_adam_step launch; the buckets' fill is skipped)
  (y) the yardstick of DESIGN.md section 5.4: a float4 copy (torch's fp32 tensor copy) that moves the same 32 B x elements

Every step starts from the same seeded gradient (restored outside the timed window; the step's work does not depend on the values, but
a zero gradient is not what a train step sees). Per step one HIP event pair around [optimiser step + gradient zero-fill]; a block is
--steps steps, the figure the median of --blocks block means. Two figures per variant: the lone step (host and device time together)
and the step with the host ahead (device time alone, see run()). Also printed: the host wall time to enqueue a step (no synchronise
inside), the algorithmic bytes and the share of the copy's rate. GPU only: without one the script exits non-zero.

usage: python tools/optim_bench.py [--steps 50] [--blocks 5] [--warmup 5] [--out profiles/optim_bench.txt]"""
import argparse
import copy
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "agrl.pytorch_amd"), os.path.join(ROOT, "tests")]
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("optim_bench: no GPU -- this tool measures on the device and has no CPU form")
if args.steps < 50:
    sys.exit("optim_bench: --steps must be at least 50")

from recipe import recipe_state_dict
from torchreid import models, parallel
from torchreid.hip_optim import HipAdam

dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


base = models.init_model("vmgn", num_classes=702, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1,
                         pyramid_part=True, use_pose=True, learn_graph=True, consistent_loss=True)
base.load_state_dict(recipe_state_dict(base.state_dict(), seed=4))
KW = dict(lr=3e-4, weight_decay=5e-4)          # the reference's recipe (train_vidreid_xent_htri.py: --lr 0.0003 --weight-decay 5e-04)


class Variant(object):
    def __init__(self, name, make_opt, native):
        self.name, self.native = name, native
        self.model = copy.deepcopy(base).to(dev)
        self.buckets = parallel.GradientBuckets(self.model.parameters())
        self.opt = make_opt([p for p in self.model.parameters() if p.requires_grad])
        self.block_ms, self.host_ms = [], []

    def restore(self, master):
        for (flat, _), src in zip(self.buckets.buckets, master):
            flat.copy_(src)

    def step(self):
        if self.native:
            self.opt.step(zero_grads=True)
            self.buckets.mark_clean()
        else:
            self.opt.step()
        self.buckets.zero_grad()


class CopyYardstick(object):
    name, native = "(y) float4 copy of 32 B x elements", False

    def __init__(self, elements):
        self.src = torch.randn(4 * elements, device=dev)
        self.dst = torch.empty_like(self.src)
        self.block_ms, self.host_ms = [], []

    def restore(self, master):
        pass

    def step(self):
        self.dst.copy_(self.src)


variants = [Variant("(a) torch.optim.Adam (default implementation) + bucket zero-fill", lambda ps: torch.optim.Adam(ps, **KW), False)]
try:
    fused = Variant("(b) torch.optim.Adam(fused=True) + bucket zero-fill", lambda ps: torch.optim.Adam(ps, fused=True, **KW), False)
    fused.restore([torch.zeros_like(flat) for flat, _ in fused.buckets.buckets])
    fused.step()
    torch.cuda.synchronize()
    fused = Variant(fused.name, lambda ps: torch.optim.Adam(ps, fused=True, **KW), False)     # a fresh one: every variant runs the same step count
    variants.append(fused)
except Exception as e:  # noqa: BLE001
    say("(b) torch.optim.Adam(fused=True): not offered by this torch (%s: %s)" % (type(e).__name__, e))
variants.append(Variant("(c) HipAdam(zero_grads=True), one agrl_adam_step launch", lambda ps: HipAdam(ps, **KW), True))
elements = sum(p.numel() for p in variants[0].model.parameters() if p.requires_grad)
variants.append(CopyYardstick(elements))

gen = torch.Generator(device=dev)
gen.manual_seed(4)
master = [torch.randn(flat.shape, device=dev, generator=gen) * 1e-3 for flat, _ in variants[0].buckets.buckets]


def run(v, steps, record, ahead):
    """ahead: a few yardstick copies (~3 ms of device work) are queued in front of every step's start event, so the host has the whole
    step enqueued before the device reaches it: the event pair then spans the step's DEVICE time alone -- what the update adds to a
    train step that is device-bound, as the native one is. Without it the pair spans a lone step, host time included."""
    pairs, host = [], 0.0
    for _ in range(steps):
        v.restore(master)
        if ahead:
            for _ in range(AHEAD_COPIES):
                yard.dst.copy_(yard.src)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        t0 = time.perf_counter()
        v.step()
        host += time.perf_counter() - t0
        e.record()
        pairs.append((s, e))
    torch.cuda.synchronize()
    if record:
        (v.ahead_ms if ahead else v.block_ms).append(sum(s.elapsed_time(e) for s, e in pairs) / steps)
        if not ahead:
            v.host_ms.append(host * 1e3 / steps)


AHEAD_COPIES = 10
yard = variants[-1]
for v in variants:
    v.ahead_ms = []
    run(v, args.warmup, False, False)
for _ in range(args.blocks):
    for v in variants:
        run(v, args.steps, True, False)
    for v in variants:
        run(v, args.steps, True, True)

bytes_alg = 32 * elements
say("vmgn, 702 classes: %d tensors, %d elements (%.1f MB of fp32 parameters) in %d buckets; algorithmic traffic of one Adam step with the gradient "
    "zero-fill 32 B x elements = %.3f GB" % (len(variants[0].opt.param_groups[0]["params"]), elements, elements * 4 / 1e6, len(master), bytes_alg / 1e9))
say("%s, torch %s; %d blocks x %d steps per variant, alternating; HIP events around [step + zero-fill]" % (
    torch.cuda.get_device_name(0), torch.__version__, args.blocks, args.steps))
say("lone step: the event pair spans host + device; host ahead: %d yardstick copies queued in front of each step, the pair spans the device time alone" % AHEAD_COPIES)
copy_ms = statistics.median(yard.ahead_ms)
for v in variants:
    lone, dev_ms = statistics.median(v.block_ms), statistics.median(v.ahead_ms)
    say("%-72s lone step %6.3f ms (blocks %s) | host enqueue %6.3f ms | host ahead %6.3f ms (blocks %s) = %5.2f TB/s algorithmic = %5.1f %% of the copy's rate" % (
        v.name, lone, " ".join("%.3f" % b for b in v.block_ms), statistics.median(v.host_ms), dev_ms, " ".join("%.3f" % b for b in v.ahead_ms),
        bytes_alg / dev_ms / 1e9, 100.0 * copy_ms / dev_ms))
ref, nat = variants[0], [v for v in variants if v.native][0]
worst = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(ref.model.parameters(), nat.model.parameters()))
scale = max(float(a.detach().abs().max()) for a in ref.model.parameters())
say("after %d identical steps: max |p(a) - p(c)| = %.3e (largest |p| %.3e)" % (args.warmup + 2 * args.blocks * args.steps, worst, scale))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
