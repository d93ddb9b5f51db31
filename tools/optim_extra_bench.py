"""The optimiser update of vmgn (702 classes, ~50 M fp32 parameters) under GradientBuckets for the rmsprop, adabound and radam names of
init_optim, timed by the method of tools/optim_bench.py: ONE process, the variants alternating block by block, one HIP event pair
around [optimiser step + gradient zero-fill] per step.

  per rule   native: HipRMSprop / HipAdaBound / HipRAdam with zero_grads=True (one launch; the buckets' fill is skipped)
             stock:  torch.optim.RMSprop(momentum=0.9) / the same HipAdaBound / HipRAdam class with hip_native = False (the rule as
                     per-tensor torch operations), each followed by GradientBuckets.zero_grad() (the memset of the flat buffers)
  (c)        HipAdam with zero_grads=True: the same kernel skeleton, the same 32 B x elements
  (y)        the yardstick of DESIGN.md section 5.4: a float4 copy (torch's fp32 tensor copy) that moves the same 32 B x elements

Every step starts from the same seeded gradient (restored outside the timed window). Two figures per variant: the lone step (host and
device time together) and the step with the host ahead (device time alone; see tools/optim_bench.py). The condition checked at the end:
in every block pair, lone and host-ahead, the native step is faster than its stock side; the script exits non-zero when it is not.
GPU only: without one the script exits non-zero.

usage: python tools/optim_extra_bench.py [--steps 50] [--blocks 5] [--warmup 5] [--out profiles/optim_extra_bench.txt]"""
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
    sys.exit("optim_extra_bench: no GPU -- this tool measures on the device and has no CPU form")
if args.steps < 20:
    sys.exit("optim_extra_bench: --steps must be at least 20")

from recipe import recipe_state_dict
from torchreid import models, parallel
from torchreid.hip_optim import HipAdaBound, HipAdam, HipRAdam, HipRMSprop

dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


base = models.init_model("vmgn", num_classes=702, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1,
                         pyramid_part=True, use_pose=True, learn_graph=True, consistent_loss=True)
base.load_state_dict(recipe_state_dict(base.state_dict(), seed=4))
LR, WD = 3e-4, 5e-4          # the reference's recipe (train_vidreid_xent_htri.py: --lr 0.0003 --weight-decay 5e-04)


class Variant(object):
    def __init__(self, name, make_opt, native):
        self.name, self.native = name, native
        self.model = copy.deepcopy(base).to(dev)
        self.buckets = parallel.GradientBuckets(self.model.parameters())
        self.opt = make_opt([p for p in self.model.parameters() if p.requires_grad])
        self.block_ms, self.host_ms, self.ahead_ms = [], [], []

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
        self.block_ms, self.host_ms, self.ahead_ms = [], [], []

    def restore(self, master):
        pass

    def step(self):
        self.dst.copy_(self.src)


def torch_route(cls, **kw):
    def make(ps):
        opt = cls(ps, **kw)
        opt.hip_native = False
        return opt
    return make


RULES = [
    ("rmsprop", Variant("rmsprop  stock : torch.optim.RMSprop(momentum=0.9) + bucket zero-fill", lambda ps: torch.optim.RMSprop(ps, lr=LR, momentum=0.9, weight_decay=WD), False),
     Variant("rmsprop  native: HipRMSprop(zero_grads=True), one agrl_rmsprop_step launch", lambda ps: HipRMSprop(ps, lr=LR, momentum=0.9, weight_decay=WD), True)),
    ("adabound", Variant("adabound stock : HipAdaBound, hip_native = False (per-tensor torch) + bucket zero-fill", torch_route(HipAdaBound, lr=LR, final_lr=100 * LR, weight_decay=WD), False),
     Variant("adabound native: HipAdaBound(zero_grads=True), one agrl_adabound_step launch", lambda ps: HipAdaBound(ps, lr=LR, final_lr=100 * LR, weight_decay=WD), True)),
    ("radam", Variant("radam    stock : HipRAdam, hip_native = False (per-tensor torch) + bucket zero-fill", torch_route(HipRAdam, lr=LR, weight_decay=WD), False),
     Variant("radam    native: HipRAdam(zero_grads=True), one agrl_radam_step launch", lambda ps: HipRAdam(ps, lr=LR, weight_decay=WD), True)),
]
adam = Variant("(c) HipAdam(zero_grads=True), one agrl_adam_step launch", lambda ps: HipAdam(ps, lr=LR, weight_decay=WD), True)
elements = sum(p.numel() for p in adam.model.parameters() if p.requires_grad)
yard = CopyYardstick(elements)
variants = [v for _, stock, native in RULES for v in (stock, native)] + [adam, yard]

gen = torch.Generator(device=dev)
gen.manual_seed(4)
master = [torch.randn(flat.shape, device=dev, generator=gen) * 1e-3 for flat, _ in adam.buckets.buckets]
AHEAD_COPIES = 10


def run(v, steps, record, ahead):
    """ahead: a few yardstick copies are queued in front of every step's start event, so the host has the whole step enqueued before
    the device reaches it and the event pair spans the step's DEVICE time alone; a per-tensor step whose host enqueue takes longer than
    those copies stays host-bound, and its figure says so. Without it the pair spans a lone step, host time included."""
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


for v in variants:
    run(v, args.warmup, False, False)
for _ in range(args.blocks):
    for v in variants:
        run(v, args.steps, True, False)
    for v in variants:
        run(v, args.steps, True, True)

bytes_alg = 32 * elements
say("vmgn, 702 classes: %d tensors, %d elements (%.1f MB of fp32 parameters) in %d buckets; algorithmic traffic of one step with the gradient "
    "zero-fill 32 B x elements = %.3f GB for every rule here (p and two state tensors read and written, g read and zero-filled)" % (
        len(adam.opt.param_groups[0]["params"]), elements, elements * 4 / 1e6, len(master), bytes_alg / 1e9))
say("%s, torch %s; %d blocks x %d steps per variant, alternating; HIP events around [step + zero-fill]" % (
    torch.cuda.get_device_name(0), torch.__version__, args.blocks, args.steps))
say("lone step: the event pair spans host + device; host ahead: %d yardstick copies queued in front of each step" % AHEAD_COPIES)
copy_ms, adam_ms = statistics.median(yard.ahead_ms), statistics.median(adam.ahead_ms)
for v in variants:
    lone, dev_ms = statistics.median(v.block_ms), statistics.median(v.ahead_ms)
    say("%-88s lone step %7.3f ms (blocks %s) | host enqueue %7.3f ms | host ahead %7.3f ms (blocks %s) = %5.2f TB/s algorithmic = %5.1f %% of the copy's rate, "
        "%5.1f %% of HipAdam's" % (v.name, lone, " ".join("%.3f" % b for b in v.block_ms), statistics.median(v.host_ms), dev_ms,
                                   " ".join("%.3f" % b for b in v.ahead_ms), bytes_alg / dev_ms / 1e9, 100.0 * copy_ms / dev_ms, 100.0 * adam_ms / dev_ms))
ok = True
for rule, stock, native in RULES:
    lone = [s / n for s, n in zip(stock.block_ms, native.block_ms)]
    ahead = [s / n for s, n in zip(stock.ahead_ms, native.ahead_ms)]
    faster = all(r > 1.0 for r in lone + ahead)
    ok = ok and faster
    worst = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(stock.model.parameters(), native.model.parameters()))
    scale = max(float(a.detach().abs().max()) for a in stock.model.parameters())
    say("%-8s stock / native per block pair: lone step %s | host ahead %s -> native faster in every pair: %s; after %d identical steps max |p(stock) - p(native)| "
        "= %.3e (largest |p| %.3e)" % (rule, " ".join("%.1fx" % r for r in lone), " ".join("%.1fx" % r for r in ahead), "yes" if faster else "NO",
                                       args.warmup + 2 * args.blocks * args.steps, worst, scale))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
if not ok:
    sys.exit("optim_extra_bench: a native step was not faster than its stock side in some block pair")
