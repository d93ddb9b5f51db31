"""Times every form of the fused Bottleneck kernels (bottleneck_tail.hip, bottleneck_block.hip) against the separate launches it
replaces, at the bench step's shapes (256 frames). The library is the one torchreid loads: AGRL_HIP_LIB=path/libagrl_hip.so times
another build (a parent commit's, alternated with the tree's, for an A/B), AGRL_HIP_LP16=bf16 the bfloat16 one.

    python tools/tail_bench.py [--json] [form ...]     forms: see FORMS; default all

One line per timed function: median us over 6 windows of 10 calls (2 more windows first as warm-up), and the HBM rate of the fused
form's traffic (every operand once)."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "agrl.pytorch_amd")):
    sys.path.insert(0, p)
import torch
from torchreid import hip_ops as ops
from torchreid import _hip
from torchreid._hip import LP_DTYPE
dev = "cuda:0"
N = 256


def time_us(fn, windows=6, warm=2, calls=10):
    """median time of one call in us"""
    ts = []
    for r in range(warm + windows):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        if r >= warm:
            ts.append(s.elapsed_time(e) * 1e3 / calls)
    return statistics.median(ts)


def rnd(shape, scale=1.0):
    return (torch.randn(shape, device=dev) / scale).to(LP_DTYPE)


def tail_form(H, W, cmid, cout, cnext, cat):
    """(fused, split, bytes): conv3 + shortcut + relu and the next conv1; cat = the shortcut is the downsample conv of x0"""
    y2, res = rnd((N, H, W, cmid)), rnd((N, H, W, cout))
    w3, w1 = rnd((cout, 1, 1, cmid), cmid ** 0.5), rnd((cnext, 1, 1, cout), cout ** 0.5)
    b3, b1 = torch.randn(cout, device=dev), torch.randn(cnext, device=dev)
    x0, ws, bs = rnd((N, H, W, cmid)), rnd((cout, 1, 1, cmid), cmid ** 0.5), torch.randn(cout, device=dev)
    if cat:
        fused = lambda: ops.bottleneck_tail(y2, w3, b3, None, w1, b1, shortcut=(x0, ws, bs))
        def split():
            o = ops.conv_bn_act(y2, w3, b3, 1, 0, True, residual=ops.conv_bn_act(x0, ws, bs, 1, 0, False))
            return o, ops.conv_bn_act(o, w1, b1, 1, 0, True)
        nbytes = 2 * (y2.numel() + x0.numel() + res.numel() + N * H * W * cnext)
    else:
        fused = lambda: ops.bottleneck_tail(y2, w3, b3, res, w1, b1)
        def split():
            o = ops.conv_bn_act(y2, w3, b3, 1, 0, True, residual=res)
            return o, ops.conv_bn_act(o, w1, b1, 1, 0, True)
        nbytes = 2 * (y2.numel() + 2 * res.numel() + N * H * W * cnext)
    return fused, split, nbytes


def block_form(cnext, cat):
    """(fused, split, bytes): the whole layer-1 block behind its conv1 at 64 x 32; split = the 3x3 launch + the fused tail"""
    H, W = 64, 32
    zin, res = rnd((N, H, W, 64)), rnd((N, H, W, 256))
    w2, w3, w1 = rnd((64, 3, 3, 64), 24), rnd((256, 1, 1, 64), 8), rnd((cnext, 1, 1, 256), 16)
    b2, b3, b1 = torch.randn(64, device=dev), torch.randn(256, device=dev), torch.randn(cnext, device=dev)
    sc = (rnd((N, H, W, 64)), rnd((256, 1, 1, 64), 8), torch.randn(256, device=dev)) if cat else None
    r = None if cat else res
    fused = lambda: ops.bottleneck_block(zin, w2, b2, w3, b3, r, w1, b1, shortcut=sc)
    split = lambda: ops.bottleneck_tail(ops.conv_bn_act(zin, w2, b2, 1, 1, True), w3, b3, r, w1, b1, shortcut=sc)
    nbytes = 2 * (zin.numel() + (zin.numel() + res.numel() if cat else 2 * res.numel()) + N * H * W * cnext)
    return fused, split, nbytes


FORMS = {
    "tail":         lambda: tail_form(64, 32, 64, 256, 64, False),
    "tail_cat":     lambda: tail_form(64, 32, 64, 256, 64, True),
    "tail_cn128":   lambda: tail_form(64, 32, 64, 256, 128, False),
    "tail_l2":      lambda: tail_form(32, 16, 128, 512, 128, False),
    "block":        lambda: block_form(64, False),
    "block_cat":    lambda: block_form(64, True),
    "block_cn128":  lambda: block_form(128, False),
}

if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--json"]
    result = {"lib": _hip.LIB_PATH}
    for name in args or FORMS:
        fused, split, nbytes = FORMS[name]()
        result[name] = {"fused_us": round(time_us(fused), 2), "split_us": round(time_us(split), 2)}
        if "--json" not in sys.argv:
            us = result[name]["fused_us"]
            print("%-12s fused %7.1f us  split %7.1f us  (fused traffic %.0f MB -> %.2f TB/s)" %
                  (name, us, result[name]["split_us"], nbytes / 1e6, nbytes / (us * 1e-6) / 1e12))
    if "--json" in sys.argv:
        print(json.dumps(result))
    else:
        print("library:", _hip.LIB_PATH)
