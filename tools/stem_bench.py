"""The 16-bit MFMA stem (csrc/stem_mfma.hip) on the bench shape: HIP-event times over rotating inputs (3 x 100 MB of frames: no
input stays in the memory-side cache), algorithmic GB/s, for both settings of AGRL_STEM_REGPOOL in one process (the register-pool form
and the conv-tile kernel, alternating block by block), and whether the two outputs are equal. usage: stem_bench.py [rounds]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "agrl.pytorch_amd")):
    sys.path.insert(0, p)
import torch
from torchreid import _hip, hip_ops as ops
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = "cuda:0"
xs = [torch.randn((256, 3, 256, 128), device=dev) for _ in range(3)]
w = torch.randn((64, 7, 7, 3), device=dev) * 0.05
b = torch.randn(64, device=dev)
wp = ops.pack_stem_weights_lp16(w)
nbytes = xs[0].numel() * 4 + 256 * 64 * 32 * 64 * 2
FORMS = (("regpool", "1"), ("conv tile", "0"))
ts = {name: [] for name, _ in FORMS}
outs = {}
for block in range(4):       # forms alternate, so that a drift of the clocks falls on both
    for name, v in FORMS:
        os.environ["AGRL_STEM_REGPOOL"] = v
        _hip.reload_options()
        for i in range(3):
            outs[name] = ops.stem_lp16(xs[i], wp, b)
        torch.cuda.synchronize()
        for r in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = ops.stem_lp16(xs[r % 3], wp, b)
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) * 1e3)
print("outputs of the two forms equal:", torch.equal(outs["regpool"], outs["conv tile"]))
for name, _ in FORMS:
    t = sorted(ts[name])
    print("stem (%s) 256 x 3 x 256 x 128 -> 256 x 64 x 32 x 64: median %.1f us (min %.1f) over %d launches = %.2f TB/s algorithmic (%.0f MB)" % (
        name, t[len(t) // 2], t[0], len(t), nbytes / t[len(t) // 2] / 1e6, nbytes / 1e6))
