"""Layer 3's chained per-frame kernel (csrc/bottleneck_chain.hip) against the launches it replaces (conv3x3_packed + bottleneck_seam per
block), interleaved in one process on the bench shape (256 frames of 16 x 8, 256 / 1024 / 256 channels). The standalone conv1
(1024 -> 256) runs in front of EVERY timed call, outside the timed window, so that each arm starts cold behind a different kernel as it
does in the step. usage: chain_bench.py [rounds] [frames]
Prints for n = 1, 2, 4: median / min of each arm in us (HIP events on the launch stream) and whether the outputs are equal.
An isolated launch is not the step: this says where the time goes, tools/ab_step.sh decides."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "agrl.pytorch_amd")):
    sys.path.insert(0, p)
import torch
from torchreid import hip_ops as ops
from torchreid._hip import LP_DTYPE

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 256
dev = "cuda:0"
DIMS = (256, 1024, 256)


def rnd(*shape, scale=1.0):
    return torch.randn(shape, device=dev) * scale


w1 = [rnd(256, 1, 1, 1024, scale=1024 ** -0.5).to(LP_DTYPE) for _ in range(5)]
b1 = [rnd(256) for _ in range(5)]
blocks = []
for i in range(4):
    w2, w3 = rnd(256, 3, 3, 256, scale=(9 * 256) ** -0.5).to(LP_DTYPE), rnd(1024, 1, 1, 256, scale=256 ** -0.5).to(LP_DTYPE)
    blocks.append({"c2": (w2, rnd(256)), "c3": (w3, rnd(1024)), "c2p": ops.conv3x3_pack(w2), "seam": ops.bottleneck_seam_pack(w3, w1[i + 1]),
                   "seam_dims": DIMS, "seam_b1n": b1[i + 1], "stride": 1, "ds": None})
table = ops.bottleneck_chain_table(blocks)
a0 = rnd(frames, 16, 8, 1024).relu().to(LP_DTYPE)
work = [torch.empty_like(a0) for _ in range(3)]


def conv1():
    return ops.conv_bn_act(a0, w1[0], b1[0], 1, 0, True)


def timed(fn):
    z = conv1()   # cold start behind a different kernel; not timed
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn(z)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, out


for n in (1, 2, 4):
    def chain(z):
        return ops.bottleneck_chain(z, a0, table, n, work=work)

    def launches(z):
        a = a0
        for blk in blocks[:n]:
            y = ops.conv3x3_packed(z, blk["c2p"], blk["c2"][1], 256, True)
            a, z = ops.bottleneck_seam(y, blk["seam"], blk["c3"][1], a, blk["seam_b1n"], DIMS)
        return a, z

    for _ in range(3):
        timed(chain), timed(launches)
    tc, tl = [], []
    for _ in range(rounds):
        t, oc = timed(chain)
        tc.append(t)
        t, ol = timed(launches)
        tl.append(t)
    same = torch.equal(oc[0], ol[0]) and torch.equal(oc[1], ol[1])
    tc.sort(), tl.sort()
    flops = 2.0 * frames * 128 * n * (9 * 256 * 256 + 2 * 256 * 1024)
    print("chain n = %d, %d frames: one launch %.1f us (min %.1f)  %d launches %.1f us (min %.1f)  outputs equal: %s  chain %.0f TFLOP/s" % (
        n, frames, tc[len(tc) // 2], tc[0], 2 * n, tl[len(tl) // 2], tl[0], same, flops / tc[len(tc) // 2] * 1e-6))
