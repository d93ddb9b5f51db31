"""ganet's train step at the shape of BASELINE configs[3] (16 tracklets x 16 frames of 256 x 128, 702 classes, xent + htri with the
consistent loss; forward, losses, backward -- no optimiser), timed in ONE process with the two routes alternating block by block:

  (n) the native step: model.hip_train = True  (_train_hip.forward_train_ganet, every arithmetic step a C-ABI call)
  (s) the stock step:  model.hip_train = False (the torch module tree on the same GPU, stock losses)

and the position-attention node alone at the step's shape (F = 256 frames, 16 x 8 map, C = 2048, Cq = 256, splits [4, 2, 1]):
agrl_pam_pool_train and agrl_pam_pool_backward, one HIP event pair around each call, with the bytes the algorithm has to move
(forward: the map and the query / key map once per pyramid level; backward: the same reads, dqk cleared and then read and written
once per level, dx written once) and the rate that makes of the call time.

Per step one HIP event pair around [zero_grad + forward + losses + backward]; a block is --steps steps, the figure the median of the
--blocks block means. The event pair of a lone step includes the host's share; both routes pay theirs. GPU only: without one the
script exits non-zero.

usage: python tools/ganet_train_bench.py [--steps 5] [--blocks 3] [--warmup 2] [--out profiles/ganet_train_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "agrl.pytorch_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--node-calls", type=int, default=30)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("ganet_train_bench: no GPU -- this tool measures on the device and has no CPU form")

from recipe import recipe_state_dict
from torchreid import hip_ops as ops
from torchreid import losses, models

dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


B, S, NCLS = 16, 16, 702
m = models.init_model("ganet", num_classes=NCLS, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1, knn=4,
                      pyramid_part=True, use_pose=True, learn_graph=True, consistent_loss=True, pretrained=False)
m.load_state_dict(recipe_state_dict(m.state_dict(), seed=4))
m = m.to(dev)
sd0 = {k: v.clone() for k, v in m.state_dict().items()}
gen = torch.Generator(device=dev)
gen.manual_seed(4)
x = torch.randn((B, S, 3, 256, 128), device=dev, generator=gen)
V = S * m.total_split
adj = (torch.rand((B, V, V), device=dev, generator=gen) < 0.3).float()
adj = ((adj + adj.transpose(1, 2) + torch.eye(V, device=dev)) > 0).float()
pids = torch.arange(4, device=dev).repeat_interleave(4)
ce = losses.CrossEntropyLabelSmooth(num_classes=NCLS, use_gpu=True)
htri = losses.TripletLoss(margin=0.3, soft=True)


def one_step(native):
    m.hip_train = native
    ce.hip_native = htri.hip_native = native   # the stock step uses the stock-torch losses too
    np.random.seed(1234)
    m.zero_grad(set_to_none=True)
    outs, feats = m(x, adj)
    loss = losses.DeepSupervision(ce, outs, pids) + losses.DeepSupervision(htri, feats, pids)
    loss.backward()
    return loss


def run(native, steps, sink):
    m.load_state_dict(sd0)
    m.train()
    pairs, loss = [], None
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        loss = one_step(native)
        e.record()
        pairs.append((s, e))
    torch.cuda.synchronize()
    if sink is not None:
        sink.append(sum(s.elapsed_time(e) for s, e in pairs) / steps)
    return float(loss.detach())


times = {True: [], False: []}
last = {}
for native in (True, False):
    run(native, args.warmup, None)
for _ in range(args.blocks):
    for native in (True, False):
        last[native] = run(native, args.steps, times[native])
ce.hip_native = htri.hip_native = True

say("ganet train step, BASELINE configs[3] shape: %d tracklets x %d frames of 256 x 128, %d classes, V = %d, consistent loss, fp32; "
    "[zero_grad + forward + losses + backward], no optimiser" % (B, S, NCLS, V))
say("%s, torch %s; %d blocks x %d steps per route, alternating, %d warm-up steps each; one HIP event pair per step" % (
    torch.cuda.get_device_name(0), torch.__version__, args.blocks, args.steps, args.warmup))
for native, name in ((True, "(n) native step (hip_train = True)"), (False, "(s) stock step (hip_train = False)")):
    say("%-38s %8.2f ms per step (block means %s) | last loss %.6f" % (
        name, statistics.median(times[native]), " ".join("%.2f" % t for t in times[native]), last[native]))
t_n, t_s = statistics.median(times[True]), statistics.median(times[False])
say("native / stock = %.3f (%s)" % (t_n / t_s, "native is faster" if t_n < t_s else "native is NOT faster"))

# ---- the position-attention node alone
F_, h, w, C, Cq, splits = B * S, 16, 8, 2048, 256, [4, 2, 1]
P = sum(splits)
xm = torch.randn((F_, h, w, C), device=dev, generator=gen)
qk = torch.randn((F_, h, w, 2 * Cq), device=dev, generator=gen) * 0.2
dxbar = torch.randn((F_, P, C), device=dev, generator=gen)
dxmean = torch.randn((F_, P, C), device=dev, generator=gen)


def time_calls(fn):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(args.node_calls):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms), min(ms), max(ms)


nlev = len(splits)
map_b, qk_b, node_b = F_ * h * w * C * 4, F_ * h * w * 2 * Cq * 4, F_ * P * C * 4
fwd_bytes = nlev * (map_b + qk_b) + 2 * node_b
bwd_bytes = nlev * (map_b + 2 * qk_b) + qk_b + 2 * nlev * qk_b + map_b + 2 * node_b
for name, fn, nbytes in (("agrl_pam_pool_train", lambda: ops.pam_pool_train(xm, qk, splits), fwd_bytes),
                         ("agrl_pam_pool_backward", lambda: ops.pam_pool_backward(xm, qk, dxbar, dxmean, splits), bwd_bytes)):
    med, lo, hi = time_calls(fn)
    say("%-24s F=%d %dx%d C=%d Cq=%d splits %s: median %.3f ms of %d calls (min %.3f, max %.3f), through the wrapper (allocations included) | "
        "%.1f MB algorithmic = %.2f TB/s" % (name, F_, h, w, C, Cq, splits, med, args.node_calls, lo, hi, nbytes / 1e6, nbytes / med / 1e9))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
