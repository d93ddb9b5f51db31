"""uint8 ingest: what it costs and what it buys, measured in ONE call with the versions alternated on the same box.

  1. The stem launch, every precision form (exact fp32, 16-bit MFMA, split-fp16), N = 256 frames of 256 x 128: fp32 NCHW input against
     uint8 input in both layouts. Device events around single launches, warm-up first, three rotating inputs (no input stays in the
     memory-side cache). With --parent-lib (a libagrl_hip.so built from the parent commit) the parent's fp32-input launch is timed too:
     fresh child processes, parent / this tree / parent / this tree ..., each calling the library through ctypes the same way. The
     spread of the parent's own medians over its repeats is the margin the comparisons are held to.
  2. End to end: evaluation.extract_features over pinned host batches (B = 32, S = 8), fp32 against uint8, alternated, in frames/s --
     host-to-device copies included, which bench.py leaves out.

usage: ingest_bench.py [--parent-lib PATH] [--pairs 3] [--rounds 60] [--e2e-batches 64] [--precision fp16]
Every child is started with subprocess (never an exec of a process that has touched the GPU) and they run one after the other."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "agrl.pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, H, W = 256, 256, 128
FORMS = ("fp32", "lp16", "split16")
INPUTS = ("f32", "u8_nchw", "u8_nhwc")


def stem_child(lib_path, rounds):
    """Time the stem entry points of ONE library through ctypes; print one JSON line per (form, input)."""
    import torch
    from torchreid import hip_ops as ops   # host-side packers and the table only: the library under test is loaded below
    dev = "cuda:0"
    lib = C.CDLL(lib_path)
    has_u8 = hasattr(lib, "agrl_stem_split16_u8")
    p, i, f = C.c_void_p, C.c_int, C.c_float
    sig = {"agrl_stem_conv_bn_relu_maxpool": [p, p, p, p, i, i, i, i, p], "agrl_stem_conv_bn_relu_maxpool_lp16": [p, p, p, p, i, i, i, p],
           "agrl_stem_split16": [p, p, p, p, p, i, i, i, f, p]}
    if has_u8:
        sig.update({"agrl_stem_conv_bn_relu_maxpool_u8": [p, p, i, p, p, p, i, i, i, i, p],
                    "agrl_stem_conv_bn_relu_maxpool_lp16_u8": [p, p, i, p, p, p, i, i, i, p],
                    "agrl_stem_split16_u8": [p, p, i, p, p, p, p, i, i, i, f, p]})
    for name, argtypes in sig.items():
        getattr(lib, name).argtypes = argtypes
        getattr(lib, name).restype = i
    lp_dtype = torch.float16 if lib.agrl_lp16_is_f16() else torch.bfloat16
    assert lp_dtype == ops.LP_DTYPE, "set AGRL_HIP_LP16 to the 16-bit type of the library under test"

    g = torch.Generator().manual_seed(0)
    u8s = [torch.randint(0, 256, (N, 3, H, W), dtype=torch.uint8, generator=g).to(dev) for _ in range(3)]
    table = torch.zeros((3, 257))
    table[:, :256] = ops.frame_table()
    table = table.to(dev)
    xs = {"f32": [table[torch.arange(3, device=dev).view(1, 3, 1, 1), u.long()].contiguous() for u in u8s],
          "u8_nchw": u8s, "u8_nhwc": [u.permute(0, 2, 3, 1).contiguous() for u in u8s]}
    w = (torch.randn((64, 7, 7, 3), generator=g) * 0.05).to(dev)
    b = torch.randn(64, generator=g).to(dev)
    wpk = ops.pack_stem_weights_lp16(w)
    wh, wl, unscale = ops.pack_stem_weights_split16(w)
    outs = {"fp32": torch.empty((N, 64, 32, 64), device=dev), "lp16": torch.empty((N, 64, 32, 64), dtype=lp_dtype, device=dev),
            "split16": torch.empty((N, 64, 32, 64), device=dev)}
    stream = torch.cuda.current_stream().cuda_stream

    def launch(form, kind, k):
        x, out = xs[kind][k].data_ptr(), outs[form].data_ptr()
        u8 = () if kind == "f32" else (table.data_ptr(), 0 if kind == "u8_nchw" else 1)
        sfx = "" if kind == "f32" else "_u8"
        if form == "fp32":
            rc = getattr(lib, "agrl_stem_conv_bn_relu_maxpool" + sfx)(x, *u8, w.data_ptr(), b.data_ptr(), out, N, H, W, 0, stream)
        elif form == "lp16":
            rc = getattr(lib, "agrl_stem_conv_bn_relu_maxpool_lp16" + sfx)(x, *u8, wpk.data_ptr(), b.data_ptr(), out, N, H, W, stream)
        else:
            rc = getattr(lib, "agrl_stem_split16" + sfx)(x, *u8, wh.data_ptr(), wl.data_ptr(), b.data_ptr(), out, N, H, W, float(unscale), stream)
        assert rc == 0, (form, kind, rc)

    kinds = INPUTS if has_u8 else INPUTS[:1]
    ref = {}
    for form in FORMS:
        for kind in kinds:
            for k in range(3):
                launch(form, kind, k)
            torch.cuda.synchronize()
            # faster and different is not faster: every input form of one library gives the same output
            snap = outs[form].clone()
            if form in ref:
                assert torch.equal(snap, ref[form]), (form, kind)
            ref[form] = snap
    # the timed passes interleave the input forms launch by launch, so drift of the box hits all of them alike
    times = {(form, kind): [] for form in FORMS for kind in kinds}
    for form in FORMS:
        for r in range(rounds):
            for kind in kinds:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(form, kind, r % 3)
                e1.record()
                e1.synchronize()
                times[(form, kind)].append(e0.elapsed_time(e1) * 1e3)
    for (form, kind), ts in times.items():
        ts.sort()
        print(json.dumps({"stem": form, "input": kind, "lib": lib_path, "rounds": len(ts), "median_us": round(ts[len(ts) // 2], 2),
                          "min_us": round(ts[0], 2), "p90_us": round(ts[int(0.9 * (len(ts) - 1))], 2)}), flush=True)


def e2e_child(nbatches, precision, reps):
    """extract_features over pinned host batches, fp32 against uint8 (both layouts), alternated; one JSON line per run."""
    import torch
    from torchreid import evaluation, hip_ops as ops, models
    dev = "cuda:0"
    B, S = 32, 8
    m = models.init_model("vmgn", num_classes=8, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1,
                          pyramid_part=True, use_pose=True, learn_graph=True).to(dev).eval()
    m.hip_precision = precision
    g = torch.Generator().manual_seed(1)
    u8 = [torch.randint(0, 256, (B, S, 3, H, W), dtype=torch.uint8, generator=g) for _ in range(4)]   # four distinct pinned batches, cycled
    adj = (torch.rand((B, S * 7, S * 7), generator=g) < 0.3).float().pin_memory()
    host = {"f32": [ops.frames_normalize_reference(u).pin_memory() for u in u8], "u8_nchw": [u.pin_memory() for u in u8],
            "u8_nhwc": [u.permute(0, 1, 3, 4, 2).contiguous().pin_memory() for u in u8]}
    pid = list(range(B))

    def batches(kind):
        for k in range(nbatches):
            yield host[kind][k % 4], pid, pid, adj

    feats = {}
    for kind in host:   # warm-up (weight packing, code objects), and the outputs must agree bit for bit
        feats[kind] = evaluation.extract_features(m, batches(kind))[0][:4 * B].clone()
        assert torch.equal(feats[kind], feats["f32"]), kind
    torch.cuda.synchronize()
    for rep in range(reps):
        for kind in host:
            t0 = time.perf_counter()
            out = evaluation.extract_features(m, batches(kind))[0]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"e2e": "extract_features", "input": kind, "precision": precision, "rep": rep, "batches": nbatches,
                              "frames": nbatches * B * S, "seconds": round(dt, 4), "frames_per_s": round(nbatches * B * S / dt, 1),
                              "host_bytes_per_batch": host[kind][0].numel() * host[kind][0].element_size()}), flush=True)
            del out


def run_child(args, env_extra=None):
    env = dict(os.environ, **(env_extra or {}))
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=900)
    text = out.stdout.decode()
    if out.returncode != 0:   # a faulted child ends the run: nothing more is started on the device
        print(text[-4000:])
        raise SystemExit("child %s failed with status %d" % (args, out.returncode))
    rows = []
    for line in text.splitlines():
        if line.startswith("{"):
            print(line, flush=True)
            rows.append(json.loads(line))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="libagrl_hip.so built from the parent commit (same 16-bit type)")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--e2e-batches", type=int, default=64)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--precision", default=None, help="hip_precision of the end-to-end run (default: the library's 16-bit mode)")
    ap.add_argument("--stem-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--e2e-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.stem_child:
        return stem_child(a.stem_child, a.rounds)
    from torchreid import _hip
    if a.e2e_child:
        return e2e_child(a.e2e_batches, a.precision or _hip.LP_NAME, a.e2e_reps)

    new_lib = _hip.LIB_PATH
    rows = {"parent": [], "new": []}
    for pair in range(a.pairs):
        for which, path in (("parent", a.parent_lib), ("new", new_lib)):
            if path is None:
                continue
            print("# stem launches, pass %d, %s library %s" % (pair, which, path), flush=True)
            rows[which].append(run_child(["--stem-child", os.path.abspath(path), "--rounds", str(a.rounds)]))
    print("# end to end", flush=True)
    e2e = run_child(["--e2e-child", "--e2e-batches", str(a.e2e_batches), "--e2e-reps", str(a.e2e_reps)] +
                    (["--precision", a.precision] if a.precision else []))

    def medians(which, form, kind):
        return [r["median_us"] for rs in rows[which] for r in rs if r["stem"] == form and r["input"] == kind]

    print("# summary: medians of the per-pass medians, us per launch of %d x 3 x %d x %d" % (N, H, W))
    for form in FORMS:
        par = medians("parent", form, "f32")
        line = "stem %-8s" % form
        if par:
            spread = max(par) - min(par)
            line += " parent f32 %s (median %.1f, spread %.1f) |" % (par, statistics.median(par), spread)
        for kind in INPUTS:
            new = medians("new", form, kind)
            line += " new %s %s (median %.1f)" % (kind, new, statistics.median(new))
            if par:
                d = statistics.median(new) - statistics.median(par)
                line += " %+.1f vs parent: %s |" % (d, "within the parent's spread or faster" if d <= spread else "SLOWER than the parent's spread allows")
        print(line)
    for kind in INPUTS:
        fps = [r["frames_per_s"] for r in e2e if r["input"] == kind]
        print("extract_features %-8s frames/s %s (median %.0f)" % (kind, fps, statistics.median(fps)))


if __name__ == "__main__":
    main()
