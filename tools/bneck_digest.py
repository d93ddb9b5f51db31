"""SHA-256 of every output tensor of seeded calls through agrl_bottleneck_tail and agrl_bottleneck_block: every form at the kernel
tests' shapes. Run it once per library in a fresh process (AGRL_HIP_LIB=..., AGRL_HIP_LP16=bf16 for the bfloat16 build) and diff
the outputs: a refactor of those kernels changes no line.

    python tools/bneck_digest.py > tree.txt;  AGRL_HIP_LIB=parent-build/libagrl_hip.so python tools/bneck_digest.py > parent.txt"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "agrl.pytorch_amd")):
    sys.path.insert(0, p)
import torch
from torchreid import hip_ops as ops
from torchreid._hip import LP_DTYPE
dev = "cuda:0"
TAIL = [(2, 64, 32), (1, 16, 8), (3, 10, 7), (5, 64, 32), (9, 64, 32), (7, 50, 47)]
TAIL_L2 = [(2, 32, 16), (1, 16, 8), (3, 10, 7), (40, 32, 16), (7, 50, 47)]
BLOCK = [(2, 64, 32), (1, 16, 8), (3, 8, 24), (9, 64, 32), (5, 64, 32)]


def rnd(g, shape, scale=1.0):
    return (torch.randn(shape, generator=g) / scale).to(LP_DTYPE).to(dev)


def show(name, outs):
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        h = hashlib.sha256(o.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
        print("%-62s out%d %-20s %s" % (name, i, tuple(o.shape), h))


def tail(shape, cmid, cout, cnext, cat):
    N, H, W = shape
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + cnext + cat)
    y2, res = rnd(g, (N, H, W, cmid)), rnd(g, (N, H, W, cout))
    w3, w1 = rnd(g, (cout, 1, 1, cmid), cmid ** 0.5), rnd(g, (cnext, 1, 1, cout), cout ** 0.5)
    b3, b1 = torch.randn(cout, generator=g).to(dev), torch.randn(cnext, generator=g).to(dev)
    sc = (rnd(g, (N, H, W, cmid)), rnd(g, (cout, 1, 1, cmid), cmid ** 0.5), torch.randn(cout, generator=g).to(dev)) if cat else None
    show("agrl_bottleneck_tail %s %d->%d->%d%s" % (shape, cmid, cout, cnext, " downsample" if cat else ""),
         ops.bottleneck_tail(y2, w3, b3, None if cat else res, w1, b1, shortcut=sc))


def block(shape, cnext, cat):
    N, H, W = shape
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + cnext + cat + 1)
    zin, res = rnd(g, (N, H, W, 64)), rnd(g, (N, H, W, 256))
    w2, w3, w1 = rnd(g, (64, 3, 3, 64), 24), rnd(g, (256, 1, 1, 64), 8), rnd(g, (cnext, 1, 1, 256), 16)
    b2, b3, b1 = (torch.randn(c, generator=g).to(dev) for c in (64, 256, cnext))
    sc = (rnd(g, (N, H, W, 64)), rnd(g, (256, 1, 1, 64), 8), torch.randn(256, generator=g).to(dev)) if cat else None
    show("agrl_bottleneck_block %s 64->256->%d%s" % (shape, cnext, " downsample" if cat else ""),
         ops.bottleneck_block(zin, w2, b2, w3, b3, None if cat else res, w1, b1, shortcut=sc))


if __name__ == "__main__":
    for s in TAIL:
        for cnext, cat in ((64, False), (128, False), (64, True)):
            tail(s, 64, 256, cnext, cat)
    for s in TAIL_L2:
        tail(s, 128, 512, 128, False)
    for s in BLOCK:
        for cnext, cat in ((64, False), (128, False), (64, True)):
            block(s, cnext, cat)
