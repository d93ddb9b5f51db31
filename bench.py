#!/usr/bin/env python
"""bench.py -- frames/sec of the per-tracklet forward-and-match hot path on MI355X.

Workload (BASELINE.json configs[1], the config the metric is quoted on): MARS-shaped synthetic clips, seq_len 8,
32 tracklets per GPU per step (256 frames of 256x128), VMGN eval forward (ResNet50 two-branch + 2 graph layers +
attention pooling) in the library's 16-bit type (fp16 by default, bf16 with --precision bf16: 16-bit storage and MFMA
operands, fp32 accumulation), then the cosine distance of the step's embeddings against the resident gallery
(12 180 x 4096, row-sharded over the ranks). One "step" = forward + [RCCL all-gather of embeddings, N > 1] +
distance matrix against the rank's gallery shard. Inputs are resident in HBM before the timed region.

    python bench.py                              # 1 GPU, 20 steps: the headline figure only
    python bench.py --full                       # the same, plus every secondary measurement and check listed below
    python bench.py --dump-outputs DIR           # also write the last timed step's outputs to DIR/*.npy (float32)
    python bench.py --gpus 8 --steps 20          # starts 8 ranks itself (fresh child processes, one per GPU, RCCL)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W   # the driver's form: every process is one rank

Rank 0 prints ONE JSON line: value = whole-job frames/s (all ranks) over EXACTLY --steps steps, ms_per_step = milliseconds
per timed step. A plain run sets up, warms up, times the steps, writes --dump-outputs and prints that line. With --full
the line also carries (each --no-* option drops one part)
  sustained_value : the same step repeated for >= 2 s (the chip runs at its power limit; a 74 ms burst flatters it)
  roofline        : the dominant kernel (conv1x1_duo_kernel / conv1x1_duo_persist_kernel: every 1x1 GEMM of layer 4 and the two-source
                    first blocks of layers 2 / 3; bound to this kernel in every run): algorithmic flops per launch / average launch
                    duration from HIP events on the launch stream, vs the dense MFMA peak; the 3x3 family: roofline_conv3x3
  host_issue      : wall time to ENQUEUE a step with nothing waited for, and the same in fresh children restricted to 1/8 of the
                    host's CPUs (eager and HIP-graph form)
  roofline_*      : conv family, layer-4 pointwise convs, GCN message pass (the WHOLE SURVEY 8(d) unit: sim +
                    normalise + mix + G h + BN + LeakyReLU + residual), distance matrix -- the HBM-bound ones with
                    the read-stream yardstick of this chip at the same byte count beside them
  accuracy        : Rank-1 / mAP of the 16-bit mode and exact fp32 on the 625-identity 1980 x 12180 split of tests/fullsplit.py, both held
                    against the CPU oracle's committed result for the same split (tests/golden/fullsplit_oracle.npz)
  modes           : the same step timed in exact fp32, bf16x3 and fp16x3 (round 6: the conforming mode at speed -- split-fp16 products,
                    ranking indices equal to the oracle's up to its own near-ties); index_exactness_by_mode puts their frames/s beside
                    their agreement with the oracle's ranked lists
  config5         : the full-eval distance matrix 1980 x 12180 x 4096 + top-50 + MARS AP/CMC, timed
  cpu_baseline    : the CPU oracle (oracle/vmgn_oracle.py, torch CPU kernels) on this host, B = 32, best thread count
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "agrl.pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_TFLOPS = {"fp16": 2500.0, "bf16": 2500.0, "fp32": 157.3, "bf16x3": 2500.0 / 3, "fp16x3": 2500.0 / 3}  # dense MFMA peaks, MI355X_MICROARCH.md (split mode: 3 bf16 MFMAs per product)
PEAK_HBM_GBS = 8000.0
GALLERY_ROWS = 12180  # MARS gallery of the reference tree
QUERY_ROWS = 1980
N_IDS = 625
FEATURE_DIM = 4096
GCN_UNIT_BYTES = lambda V, C: 4.0 * (3 * V * C + V * V)  # noqa: E731  SURVEY 8(d): read f + read h + read adj + write out


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32, help="tracklets per GPU per step")
    ap.add_argument("--seq-len", type=int, default=8)
    ap.add_argument("--precision", default="fp16", choices=["fp16", "bf16", "fp32", "bf16x3", "fp16x3"],
                    help="fp16 / bf16: 16-bit storage + MFMA operands, fp32 accumulation (each has its own build of the library: "
                         "libagrl_hip.so / libagrl_hip_bf16.so, selected through AGRL_HIP_LP16 before torchreid is imported)")
    ap.add_argument("--metric", default="cosine", choices=["cosine", "euclidean"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-accuracy", action="store_true", help="skip the 625-identity Rank-1 / mAP block")
    ap.add_argument("--no-config5", action="store_true", help="skip the 1980 x 12180 x 4096 full-eval timing")
    ap.add_argument("--no-config4", action="store_true", help="skip the seq_len-16 train-step timing")
    ap.add_argument("--sustain-seconds", type=float, default=2.0)
    ap.add_argument("--cpu-seconds", type=float, default=40.0, help="upper bound of the CPU-baseline thread sweep")
    ap.add_argument("--profile-steps", type=int, default=3)
    ap.add_argument("--dist-timeout", type=float, default=1800.0, help="--gpus N > 1 self-launch: seconds before the ranks are terminated")
    ap.add_argument("--no-modes", action="store_true", help="skip the fp32 / bf16x3 precision-mode timings")
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--embedding-error", action="store_true",
                    help="add the max relative error of this precision's embeddings of the timed batch against the exact-fp32 forward")
    ap.add_argument("--graph", action="store_true",
                    help="replay the forward from a captured HIP graph (host issue cost 1.2 ms -> 0.08 ms per step; GPU time "
                         "unchanged within 1.5 %%, tools/graph_probe.py)")
    ap.add_argument("--no-host-issue", action="store_true", help="skip the restricted-cores child of the host-issue measurement")
    ap.add_argument("--host-cores", type=int, default=0,
                    help="restrict this process to its first K allowed CPUs (os.sched_setaffinity at start-up, before any GPU call)")
    ap.add_argument("--host-issue-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, run every secondary measurement and check (extra blocks, host issue, sustained rate, "
                         "per-kernel rooflines, precision modes, accuracy, config5, config4, CPU baseline; the --no-* options "
                         "drop parts of it); without it the run prints the headline figure only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned on rank 0 -- the distance matrix and the embeddings it was "
                         "computed from -- as DIR/<name>.npy in float32")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """Write {name: tensor} as path/<name>.npy in float32. When they hold more than DUMP_BUDGET_BYTES together, every array
    keeps a fixed, seeded sample of its rows (the same rows from run to run for the same arguments)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    host = {name: t.detach().float().cpu().numpy() for name, t in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    for name, a in host.items():
        if total > DUMP_BUDGET_BYTES and a.ndim >= 1 and a.shape[0] > 1:
            keep = max(1, int(a.shape[0] * DUMP_BUDGET_BYTES / total))
            rows = np.sort(np.random.RandomState(0).choice(a.shape[0], keep, replace=False))
            a = a[rows]
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# N > 1 without a launcher: the parent starts one fresh child per rank BEFORE it makes any GPU call (it never does:
# no torch.cuda.* below this line in the parent) and relays rank 0's JSON line.
def launch_ranks(args, argv, script=None, poll_s=0.2):
    """Start one fresh child process per rank, watch ALL of them, relay rank 0's stdout.

    * a child that exits non-zero ends the job: the others are terminated (SIGTERM, then SIGKILL after 5 s) and the
      launcher returns that code -- a rank blocked in a collective whose partner died would otherwise wait for ever;
    * ``--dist-timeout`` seconds without completion do the same with code 124;
    * every rank's stderr tail is printed when the job fails;
    * on success rank 0's JSON line is checked: ``config.ranks == N`` and, when the children saw at least N devices,
      ``config.collective_backend == "rccl"`` (a silent gloo fallback on a real multi-GPU node is an error).
    Children are always fresh processes created before anything here touches the GPU (the parent never does)."""
    import tempfile
    script = script or os.path.abspath(__file__)
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    procs, outs, errs = [], [], []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL's intra-node transport needs it on this driver
        outs.append(tempfile.TemporaryFile())
        errs.append(tempfile.TemporaryFile())
        procs.append(subprocess.Popen([sys.executable, script] + argv, env=env, stdout=outs[-1], stderr=errs[-1]))

    def tail(f, nbytes=2000):
        f.seek(0, os.SEEK_END)
        size = f.tell()
        f.seek(max(0, size - nbytes))
        return f.read().decode(errors="replace")

    def stop_all():
        for p in procs:
            if p.poll() is None:
                p.terminate()
        t_end = time.time() + 5.0
        for p in procs:
            try:
                p.wait(timeout=max(0.1, t_end - time.time()))
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()

    deadline = time.time() + args.dist_timeout
    rc, why = 0, None
    while True:
        codes = [p.poll() for p in procs]
        bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
        if bad:
            rc, why = (abs(bad[0][1]) or 1), "rank %d exited with code %d" % bad[0]
            break
        if all(c == 0 for c in codes):
            break
        if time.time() > deadline:
            rc, why = 124, "no completion within --dist-timeout %.0f s" % args.dist_timeout
            break
        time.sleep(poll_s)
    if rc:
        stop_all()
        sys.stderr.write("bench.py launcher: %s; remaining ranks terminated\n" % why)
        for r in range(args.gpus):
            sys.stderr.write("---- rank %d (exit %s) stderr tail ----\n%s\n" % (r, procs[r].returncode, tail(errs[r])))
    else:
        for r in range(1, args.gpus):
            sys.stderr.write(tail(errs[r], 1 << 20))
    sys.stderr.write(tail(errs[0], 1 << 20))
    outs[0].seek(0)
    text = outs[0].read().decode(errors="replace")
    sys.stdout.write(text)
    sys.stdout.flush()
    if rc == 0:
        lines = [ln for ln in text.splitlines() if ln.startswith("{")]
        try:
            cfg = json.loads(lines[-1])["config"]
            if cfg.get("ranks") != args.gpus:
                rc, why = 1, "JSON line reports %r ranks, launched %d" % (cfg.get("ranks"), args.gpus)
            elif cfg.get("devices_visible", 0) >= args.gpus and cfg.get("collective_backend") != "rccl":
                rc, why = 1, "%d devices visible but the collective backend is %r, not rccl" % (cfg["devices_visible"], cfg.get("collective_backend"))
        except (IndexError, KeyError, ValueError) as e:
            rc, why = 1, "no JSON line from rank 0 (%r)" % (e,)
        if rc:
            sys.stderr.write("bench.py launcher: %s\n" % why)
    return rc


# ---------------------------------------------------------------------------------------------------------------------
def build_model(device, precision):
    from recipe import recipe_state_dict
    from torchreid import models
    m = models.init_model("vmgn", num_classes=N_IDS, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2,
                          num_scale=1, pyramid_part=True, use_pose=True, learn_graph=True, consistent_loss=False,
                          num_parts=3, bnneck=True)
    sd = recipe_state_dict(m.state_dict(), seed=0)
    m.load_state_dict(sd)
    m.eval()
    m.hip_precision = precision
    m.hip_static_weights = True
    return m.to(device), sd


def synthetic_pose_adjacency(B, S, device, gen):
    """The model's second input, built on the device by the product's own kernel (agrl_pose_adjacency)
    from synthetic AlphaPose keypoints: y uniform over the frame, confidence uniform (threshold 0.1), one frame in ten
    without a detection (its 7 x 7 blocks stay zero)."""
    import torch
    from torchreid import hip_ops as ops
    poses = torch.rand((B, S, 18, 3), device=device, generator=gen)
    poses[..., 0] *= 128.0
    poses[..., 1] *= 256.0
    detected = torch.rand((B, S), device=device, generator=gen) >= 0.1
    return ops.pose_adjacency(poses, detected, height=256.0, num_split=4, pyramid_part=True, threshold=0.1)


def _one_socket_cpus():
    """Logical CPUs of package 0, one hardware thread per physical core (sysfs topology); None when unreadable."""
    try:
        seen, cpus = set(), []
        for cpu in sorted(os.sched_getaffinity(0)):
            base = "/sys/devices/system/cpu/cpu%d/topology/" % cpu
            if int(open(base + "physical_package_id").read()) != 0:
                continue
            core = int(open(base + "core_id").read())
            if core not in seen:
                seen.add(core)
                cpus.append(cpu)
        return cpus or None
    except (OSError, ValueError, AttributeError):
        return None


def host_issue_child(args):
    """The eager step and its HIP-graph form in FRESH processes restricted to 1/8 of this host's CPUs (what a rank has to itself
    on an 8-GPU node): os.sched_setaffinity runs at the child's start-up, before it imports torch or makes any GPU call. Reports
    the enqueue time per step and the step time under the restriction."""
    ncpu = len(os.sched_getaffinity(0))
    k = max(1, ncpu // 8)
    out = {"cpus": k, "of": ncpu}
    for name, extra in (("eager", []), ("hip_graph", ["--graph"])):
        cmd = [sys.executable, os.path.abspath(__file__), "--host-issue-only", "--host-cores", str(k), "--steps", "10", "--warmup", "3",
               "--precision", args.precision, "--metric", args.metric, "--batch", str(args.batch), "--seq-len", str(args.seq_len)] + extra
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
            line = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
            out[name] = json.loads(line[-1]) if r.returncode == 0 and line else {"error": r.stderr.decode()[-300:]}
        except Exception as e:  # noqa: BLE001
            out[name] = {"error": str(e)[:200]}
    return out


def cpu_baseline_child(S, metric, budget_s):
    """Runs in a FRESH process that never touches the GPU (bench.py --cpu-baseline-only): the oracle on this host's cores,
    the same step at the same batch (32 tracklets x S frames, forward + distance matrix against the full gallery). The
    process is pinned to ONE socket, one hardware thread per physical core, before torch starts its thread pool (an
    unpinned 64- or 128-thread run across both sockets of the GPU host was slower than 32 threads), and glibc is told to
    keep freed activations (default thresholds hand every large tensor back to the kernel: 3 x slower on this oracle).
    One timed batch per thread count, best reported with the sweep."""
    cpus = _one_socket_cpus()
    pinned = False
    if cpus:
        try:
            os.sched_setaffinity(0, cpus)
            pinned = True
        except OSError:
            pass
    try:
        import ctypes
        libc = ctypes.CDLL("libc.so.6")
        libc.mallopt(-1, 1 << 30)   # M_TRIM_THRESHOLD
        libc.mallopt(-3, 1 << 30)   # M_MMAP_THRESHOLD
    except OSError:
        pass
    import torch
    from oracle import vmgn_oracle as O
    from recipe import recipe_state_dict, synthetic_adj, synthetic_clips
    from torchreid import models
    m = models.init_model("vmgn", num_classes=N_IDS, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2,
                          num_scale=1, pyramid_part=True, use_pose=True, learn_graph=True, consistent_loss=False,
                          num_parts=3, bnneck=True)
    sd = recipe_state_dict(m.state_dict(), seed=0)
    del m
    gallery_cpu = torch.randn((GALLERY_ROWS, FEATURE_DIM), generator=torch.Generator().manual_seed(7))
    bs = 32
    x, adj = synthetic_clips(bs, S, seed=123), synthetic_adj(bs, S, seed=123)
    fn = O.cosine if metric == "cosine" else O.euclidean_squared
    ncpu = len(os.sched_getaffinity(0))
    # the width that has been fastest on every box so far first (16 threads: 150-210 frames/s; 64 threads across one socket: 17-26),
    # so that a slow wide point cannot eat the budget before the representative one has run
    pref = [16, 32, 8, 64, 128]
    cands = sorted({t for t in pref if t <= ncpu} | {ncpu}, key=lambda t: pref.index(t) if t in pref else len(pref))
    sweep, t_start, frames_total = {}, time.time(), 0
    with torch.no_grad():
        for threads in cands:
            if sweep and time.time() - t_start + 1.3 * min(sweep.values()) > budget_s:
                break
            torch.set_num_threads(threads)
            O.vmgn_eval(x[:2], adj[:2], sd)  # warm the thread pool / allocator at this width
            t0 = time.time()
            emb = O.vmgn_eval(x, adj, sd)
            fn(emb, gallery_cpu)
            sweep[threads] = time.time() - t0
            frames_total += bs * S
    best = min(sweep, key=sweep.get)
    return {"value": round(bs * S / sweep[best], 2), "unit": "frames/s", "cores": best, "kind": "port",
            "sweep_frames_per_s": {str(t): round(bs * S / dt, 2) for t, dt in sweep.items()},
            "host_cpus": os.cpu_count(), "pinned_to_socket0_physical_cores": ncpu if pinned else None,
            "sample": "%d frames per thread count (one batch of %d tracklets x %d frames, fwd+GCN+%s distmat vs %d gallery rows), "
                      "%d frames in %.1f s overall, oracle/vmgn_oracle.py on torch CPU fp32, process pinned to one socket" %
                      (bs * S, bs, S, metric, GALLERY_ROWS, frames_total, time.time() - t_start)}


def cpu_baseline(S, metric, budget_s):
    """Fresh child process (affinity and allocator settings must precede torch's thread pool; the child makes no GPU call)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["HIP_VISIBLE_DEVICES"] = ""
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", "--seq-len", str(S), "--metric", metric,
                              "--cpu-seconds", str(budget_s)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             timeout=max(300.0, 8 * budget_s))
        line = [ln for ln in out.stdout.decode().splitlines() if ln.startswith("{")][-1]
        return json.loads(line)
    except Exception as e:  # noqa: BLE001
        return {"error": repr(e)[:300]}


def accuracy_block(model, device, S, metric):
    """Rank-1 / mAP on the full-size split of SURVEY 8(d) (tests/fullsplit.py: 625 identities, 1 980 queries, 12 180
    gallery tracklets with 5 % junk, 6 cameras; inputs are integer hashes, bit-identical on CPU and GPU): embedded by
    the model in the 16-bit mode (fp16 / bf16) and in exact fp32, distance + MARS ranking on the device for both, and the fp32 run held against
    what the CPU ORACLE produced for the same split in the build container (tests/golden/fullsplit_oracle.npz: Rank-1,
    mAP, the first 51 ranked gallery indices and distances of every query)."""
    import numpy as np
    import torch
    import fullsplit as FS
    from torchreid import evaluation
    from torchreid import hip_ops as ops
    from torchreid.models._vmgn_hip import hip_forward
    assert S == FS.SEQ_LEN
    q_pids, q_cams, g_pids, g_cams = FS.labels()

    def make_adj(poses, detected):
        return ops.pose_adjacency(poses, detected, height=float(FS.HEIGHT), num_split=4, pyramid_part=True, threshold=0.1)

    def batches(pids, cams, first, bs=64):
        return FS.batches(pids, cams, first, device, bs, make_adj)

    prev = model.hip_precision
    z = FS.load_oracle_fixture()
    if z is not None:
        FS.apply_calibration(model, z)   # the oracle's own BNNeck statistics: both sides normalise identically
        cal = "tests/golden/fullsplit_oracle.npz (oracle features of gallery rows 0..2047)"
    else:
        # no fixture: calibrate from the exact-fp32 forward of the same 2048 gallery tracklets
        model.hip_precision = "fp32"
        gf_, af_ = [], []
        with torch.no_grad():
            for clips, _, _, adj in batches(g_pids[:2048], g_cams[:2048], FS.QUERY_ROWS):
                _, g_f, a_f = hip_forward(model, clips, adj, return_feats=True)
                gf_.append(g_f)
                af_.append(a_f)
            for bn, f in ((model.global_bottleneck, torch.cat(gf_)), (model.att_bottleneck, torch.cat(af_))):
                bn.running_mean.copy_(f.mean(0))
                bn.running_var.copy_(f.var(0, unbiased=False).clamp(min=1e-8))
                bn.weight.fill_(1.0)
                bn.bias.zero_()
        model.invalidate_hip_cache()
        cal = "this run's fp32 forward (no oracle fixture present)"
    out = {"ids": FS.N_IDS, "n_query": FS.QUERY_ROWS, "n_gallery": FS.GALLERY_ROWS, "metric": metric, "max_rank": 50,
           "bnneck_calibration": cal}
    top = {}
    LP = ops.LP_NAME
    out["lp16"] = LP
    SPLIT = ("bf16x3", "fp16x3")
    for prec in (LP,) + SPLIT + ("fp32",):   # bf16x3 / fp16x3: the embeddings from split products, matched in exact fp32
        model.hip_precision = prec
        t0 = time.perf_counter()
        qf, _, _ = evaluation.extract_features(model, batches(q_pids, q_cams, 0), prefetch=False)
        gf, _, _ = evaluation.extract_features(model, batches(g_pids, g_cams, FS.QUERY_ROWS), prefetch=False)
        cmc, mAP, idx, val = evaluation.match_and_rank(qf, q_pids, q_cams, gf, g_pids, g_cams, metric, 50,
                                                       "fp32" if prec == "bf16x3" else prec, return_topk=True)   # (fp16x3 matches in its own split-fp16 distance matrix)
        torch.cuda.synchronize()
        out[prec] = {"rank1": round(float(cmc[0]), 6), "rank5": round(float(cmc[4]), 6), "mAP": round(float(mAP), 6),
                     "seconds": round(time.perf_counter() - t0, 2)}
        top[prec] = (idx, val, qf)
        if prec == "fp32":
            out["_embeddings"] = (qf, gf)
    model.hip_precision = prev
    model.invalidate_hip_cache()
    out["rank1_delta"] = round(out[LP]["rank1"] - out["fp32"]["rank1"], 6)
    out["mAP_delta"] = round(out[LP]["mAP"] - out["fp32"]["mAP"], 6)
    out["top1_index_agreement"] = round(float((top[LP][0][:, 0] == top["fp32"][0][:, 0]).mean()), 6)
    out["top50_index_agreement"] = round(float(np.asarray(top[LP][0] == top["fp32"][0]).mean()), 6)
    d_q = (top[LP][2] - top["fp32"][2]).double()
    out["embedding_err_%s_vs_fp32" % LP] = {
        "max_abs_over_max_abs": float("%.3g" % (d_q.abs().max() / top["fp32"][2].abs().max()).item()),
        "worst_query_rel_l2": float("%.3g" % (d_q.norm(dim=1) / top["fp32"][2].double().norm(dim=1)).max().item()),
        "note": "this split's BNNeck statistics are the oracle's (1 / sqrt(var) of near-constant feature dimensions amplifies every "
                "difference: exact fp32 against the oracle is 1.3e-5 here and 2e-7 on the recipe model of the parity tests)"}
    if z is not None and metric + "_idx" in z.files:
        o_cmc, o_map = z[metric + "_cmc"], float(z[metric + "_mAP"])
        emb = top["fp32"][2][:16].cpu().double().numpy()
        ref = z["q_emb_head"].astype(np.float64)
        out["oracle"] = {"rank1": round(float(o_cmc[0]), 6), "rank5": round(float(o_cmc[4]), 6), "mAP": round(o_map, 6),
                         "source": "tests/golden/fullsplit_oracle.npz (oracle/vmgn_oracle.py on the build container's CPU, tests/golden/make_fullsplit.py)"}
        for prec in ("fp32",) + SPLIT + (LP,):
            c = FS.compare_topk(top[prec][0], top[prec][1], z[metric + "_idx"], z[metric + "_val"])
            out[prec + "_vs_oracle"] = {"rank1_delta": round(out[prec]["rank1"] - float(o_cmc[0]), 6),
                                        "mAP_delta": round(out[prec]["mAP"] - o_map, 6),
                                        "top50_index_agreement": round(c["agreement"], 6), "top1_index_agreement": round(c["top1_agreement"], 6),
                                        "queries_with_identical_top50": round(c["rows_equal"], 6),
                                        "max_abs_distance_err": float("%.3g" % c["max_abs_val_err"]),
                                        "swapped_positions": c["swapped_positions"], "swaps_not_explained_by_a_near_tie": c["unexplained"]}
        out["fp32_vs_oracle"]["embedding_max_rel_err_first16"] = float("%.3g" % (np.abs(emb - ref).max() / np.abs(ref).max()))
    else:
        out["oracle"] = None
        out["note"] = "tests/golden/fullsplit_oracle.npz absent: fp32 = the exact-fp32 HIP mode only (run tests/golden/make_fullsplit.py in the build container)"
    return out


def modes_block(model, clips, adj, g_shard, metric, steps=3, blocks=3):
    """The same step (forward + distance matrix of the batch against the resident gallery) in the two precision modes that
    meet the north-star tolerance (1e-3 relative, ranking indices bit-exact on the test splits): exact fp32 and bf16x3
    (fp32 tensors, every conv / Linear product as three bf16 MFMAs). ``steps`` timed steps each after one warm-up, plus one
    instrumented step for the conv family's share of the respective MFMA peak."""
    import torch
    from torchreid import _hip
    from torchreid import hip_ops as ops
    prev = model.hip_precision
    B, S = clips.shape[:2]
    fam = ("agrl_conv2d_bn_act", "agrl_conv1x1_bn_act_pool", "agrl_bottleneck_tail", "agrl_bottleneck_block", "agrl_conv1x1_dual_bn_act",
           "agrl_conv2d_bn_act_split16", "agrl_conv1x1_split16", "agrl_conv1x1_split16_dual", "agrl_conv1x1_split16_pool", "agrl_conv3x3_packed_split16")
    out = {}
    if metric == "cosine":
        g_op, g_norm = ops.row_l2_normalize(g_shard, True, torch.float32), None
    else:
        g_op, g_norm = g_shard, ops.row_sqnorm(g_shard)

    def one():
        emb = model(clips, adj)
        if metric == "cosine":
            return ops.distmat(ops.row_l2_normalize(emb, True, torch.float32), g_op, "cosine")
        return ops.distmat(emb, g_op, "euclidean", ops.row_sqnorm(emb), g_norm)

    try:
        for prec in ("fp32", "bf16x3", "fp16x3"):
            model.hip_precision = prec
            one()
            torch.cuda.synchronize()
            dts = []
            for _ in range(blocks):   # median of `blocks` timed blocks of `steps` steps
                t0 = time.perf_counter()
                for _ in range(steps):
                    one()
                torch.cuda.synchronize()
                dts.append((time.perf_counter() - t0) / steps)
            dt = sorted(dts)[len(dts) // 2]
            _hip.PROFILE = []
            one()
            torch.cuda.synchronize()
            prof, _hip.PROFILE = _hip.PROFILE, None
            ms = sum(s_ev.elapsed_time(e_ev) for name, s_ev, e_ev, tag in prof if name in fam)
            fl = sum(tag["flops"] for name, s_ev, e_ev, tag in prof if name in fam and tag)
            tf = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            out[prec] = {"ms_per_step": round(1e3 * dt, 3), "frames_per_s": round(B * S / dt, 1), "steps": steps, "blocks": blocks,
                         "ms_per_step_blocks": [round(1e3 * d, 3) for d in dts],
                         "conv_family_tflops": round(tf, 1), "peak_tflops": round(PEAK_TFLOPS[prec], 1),
                         "conv_family_frac_of_peak": round(tf / PEAK_TFLOPS[prec], 4)}
    finally:
        _hip.PROFILE = None
        model.hip_precision = prev
    out["note"] = ("fp32: v_mfma_f32_16x16x4_f32, bit-compatible with an fmaf chain; bf16x3: three bf16 MFMAs per product on the high / low "
                   "halves of fp32 operands (~1e-5 per product); fp16x3 (round 6): three fp16 MFMAs per product on fp16 high / low halves, conv weights "
                   "pre-scaled by a power of two (22 significand bits per operand, ~2e-7 per product; GraphLayer / distance matrix exact fp32). All hold the whole forward within 1e-3 of the CPU oracle "
                   "(tests/test_gpu_model.py: 3e-7 / 4e-5); of the 16-bit modes fp16 is at ~2.5e-4 and bf16 at ~2e-3 (`accuracy`, `lp16_other`)")
    return out


def other_lp16_child(args):
    """The same step with the OTHER 16-bit build of the library (bf16 when this run is fp16 and vice versa): a fresh child
    process (the 16-bit type is fixed when torchreid is imported), same steps / warm-up, its one-batch embedding error against
    its own exact-fp32 forward beside it."""
    other = "bf16" if args.precision == "fp16" else "fp16"
    cmd = [sys.executable, os.path.abspath(__file__), "--precision", other, "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--batch", str(args.batch), "--seq-len", str(args.seq_len), "--metric", args.metric, "--no-cpu-baseline", "--no-accuracy",
           "--no-config5", "--no-config4", "--no-modes", "--sustain-seconds", "0", "--profile-steps", "0", "--embedding-error",
           "--full"]
    env = {k: v for k, v in os.environ.items() if k not in ("AGRL_HIP_LP16", "AGRL_HIP_LIB", "RANK", "WORLD_SIZE", "LOCAL_RANK")}
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        line = [l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1]
        j = json.loads(line)
        return {"dtype": j["dtype"], "value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"],
                "embedding_max_rel_err_vs_fp32_one_batch": j.get("embedding_max_rel_err_vs_fp32_one_batch"),
                "library": j["config"].get("library"), "how": "child process: python bench.py --precision %s, same steps / warm-up" % other}
    except Exception as e:  # noqa: BLE001
        return {"error": repr(e)[:300]}


def config5_block(device, embeddings, metric):
    """BASELINE configs[4]: the full MARS evaluation -- 1980 x 12180 x 4096 distance matrix (tiled MFMA form), top-50,
    evaluate_mars -- timed with HIP events (median of 5)."""
    import numpy as np
    import torch
    from torchreid import hip_ops as ops
    from torchreid.metrics.distance import hip_distmat_device
    if embeddings is None:
        g = torch.Generator(device=device)
        g.manual_seed(5)
        qf = torch.randn((QUERY_ROWS, FEATURE_DIM), device=device, generator=g)
        gf = torch.randn((GALLERY_ROWS, FEATURE_DIM), device=device, generator=g)
    else:
        qf, gf = embeddings
    rng = np.random.RandomState(1)
    q_pids = torch.as_tensor(rng.randint(0, N_IDS, QUERY_ROWS).astype(np.int32), device=device)
    g_pids = torch.as_tensor(rng.randint(0, N_IDS, GALLERY_ROWS).astype(np.int32), device=device)
    q_cams = torch.zeros(QUERY_ROWS, dtype=torch.int32, device=device)
    g_cams = torch.ones(GALLERY_ROWS, dtype=torch.int32, device=device)

    def timed(fn, reps=5):
        ts = []
        for _ in range(reps + 1):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn()
            e.record()
            e.synchronize()
            ts.append(s.elapsed_time(e))
        return r, float(np.median(ts[1:]))

    flops = 2.0 * QUERY_ROWS * GALLERY_ROWS * FEATURE_DIM
    out = {"m": QUERY_ROWS, "n": GALLERY_ROWS, "D": FEATURE_DIM, "metric": metric, "gflop": round(flops / 1e9, 1)}
    for prec in (ops.LP_NAME, "fp32"):
        dt = ops.LP_DTYPE if prec == ops.LP_NAME else torch.float32
        if metric == "cosine":
            (qh, gh), t_prep = timed(lambda: (ops.row_l2_normalize(qf, True, dt), ops.row_l2_normalize(gf, True, dt)))
            d, t_mm = timed(lambda: ops.distmat(qh, gh, "cosine"))
        else:
            d, t_mm = timed(lambda: hip_distmat_device(qf, gf, metric, prec))
            t_prep = 0.0
        peak = PEAK_TFLOPS[prec]
        out[prec] = {"prepare_ms": round(t_prep, 3), "distmat_ms": round(t_mm, 3),
                     "tflops": round(flops / (t_mm * 1e-3) / 1e12, 1), "peak": peak,
                     "frac_of_mfma_peak": round(flops / (t_mm * 1e-3) / 1e12 / peak, 4)}
        if metric == "cosine":   # distance + top-50 without the 96.5 MB matrix (agrl_distmat_topk: query blocks in a reused workspace)
            (idx_f, _), t_f = timed(lambda: ops.distmat_topk(qh, gh, "cosine", 50))
            out[prec]["distmat_topk50_ms"] = round(t_f, 3)
            idx_s, _ = ops.rank_topk(d, 50)
            out[prec]["distmat_topk50_equals_separate"] = bool(torch.equal(idx_f, idx_s))
        if prec == "fp32":
            (idx, _), t_topk = timed(lambda: ops.rank_topk(d, 50))
            _, t_mars = timed(lambda: ops.rank_mars(idx, q_pids, q_cams, g_pids, g_cams))
            out["topk50_ms"] = round(t_topk, 3)
            out["topk50_gbs"] = round(4.0 * QUERY_ROWS * GALLERY_ROWS / (t_topk * 1e-3) / 1e9, 1)
            out["rank_mars_ms"] = round(t_mars, 3)
            d_fp32 = d
    if metric == "cosine" and ops.split16_planes_available():
        # the conforming mode's distance matrix (round 6): the 16-bit kernels on split-fp16 plane operands -- fp32-class distances
        q32, g32 = ops.row_l2_normalize(qf, True, torch.float32), ops.row_l2_normalize(gf, True, torch.float32)
        (q3, g3), t_prep = timed(lambda: (ops.to_split16_planes(q32), ops.to_split16_weight_planes(g32, 2.0 ** 13)))
        d3, t_mm = timed(lambda: ops.distmat_split16(q3, g3, "cosine", 2.0 ** -13))
        out["fp16x3"] = {"prepare_ms": round(t_prep, 3), "distmat_ms": round(t_mm, 3), "tflops": round(flops / (t_mm * 1e-3) / 1e12, 1),
                         "peak": round(PEAK_TFLOPS["fp16x3"], 1), "frac_of_mfma_peak": round(flops / (t_mm * 1e-3) / 1e12 / PEAK_TFLOPS["fp16x3"], 4),
                         "max_abs_diff_vs_exact_fp32": float("%.3g" % (d3 - d_fp32).abs().max().item()),
                         "top50_index_agreement_with_exact_fp32": round(float((ops.rank_topk(d3, 50)[0] == ops.rank_topk(d_fp32, 50)[0]).float().mean().item()), 6)}
    return out


def config4_block(device):
    """BASELINE configs[3] on one GPU: a DukeMTMC-VideoReID-shaped xent + htri train step (seq_len 16, V = 112, 16 tracklets =
    4 identities x 4 instances, 702 classes, consistent loss, Adam) in fp32 -- forward, losses with on-GPU batch-hard
    mining, backward, optimizer step -- with the conv trunk on the native kernels, and the same step on the stock-torch
    module tree (rocBLAS / MIOpen) beside it."""
    import torch
    from recipe import recipe_state_dict
    from torchreid import losses, models
    B, S, ncls = 16, 16, 702
    m = models.init_model("vmgn", num_classes=ncls, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1,
                          pyramid_part=True, use_pose=True, learn_graph=True, consistent_loss=True)
    m.load_state_dict(recipe_state_dict(m.state_dict(), seed=4))
    m = m.to(device)
    gen = torch.Generator(device=device)
    gen.manual_seed(4)
    x = torch.randn((B, S, 3, 256, 128), device=device, generator=gen)
    adj = synthetic_pose_adjacency(B, S, device, gen)
    pids = torch.arange(4, device=device).repeat_interleave(4)
    ce = losses.CrossEntropyLabelSmooth(num_classes=ncls, use_gpu=True)
    htri = losses.TripletLoss(margin=0.3, soft=True)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    out = {"tracklets": B, "seq_len": S, "frames": B * S, "dtype": "fp32", "classes": ncls,
           "gflop_per_step": round(3 * 11.93 * B * S, 1), "timing": "median of 5 steps after one warm-up step, per variant"}

    def run(native, steps=5, precision="fp32"):
        m.load_state_dict(sd0)
        m.hip_train = native
        m.hip_train_precision = precision
        ce.hip_native = htri.hip_native = native   # the stock-torch baseline step uses the stock-torch losses too
        m.train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-4, weight_decay=5e-4)
        ts, loss = [], None
        for i in range(steps + 1):
            torch.manual_seed(1234)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs, feats = m(x, adj)
            loss = losses.DeepSupervision(ce, outs, pids) + losses.DeepSupervision(htri, feats, pids)
            opt.zero_grad()
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            if i:
                ts.append(time.perf_counter() - t0)
        return sorted(ts)[len(ts) // 2], float(loss.detach())   # median of ``steps`` timed steps (one untimed warm-up step before)
    try:
        t_nat, l_nat = run(True)
        t_x3, l_x3 = run(True, precision="bf16x3")
        t_ref, l_ref = run(False)
    except RuntimeError as e:  # noqa: BLE001  (out of memory on a small device)
        return {"error": str(e)[:200]}
    ce.hip_native = htri.hip_native = True
    fl = 3 * 11.93e9 * B * S
    # where the native step's time goes: HIP events around every C-ABI call of one more step (exact fp32)
    try:
        from torchreid import _hip as _h
        m.load_state_dict(sd0)
        m.hip_train, m.hip_train_precision = True, "fp32"
        m.train()
        _h.PROFILE = []
        torch.manual_seed(1234)
        outs, feats = m(x, adj)
        (losses.DeepSupervision(ce, outs, pids) + losses.DeepSupervision(htri, feats, pids)).backward()
        torch.cuda.synchronize()
        prof, _h.PROFILE = _h.PROFILE, None
        agg = {}
        for name, s_ev, e_ev, _tag in prof:
            agg[name] = agg.get(name, 0.0) + s_ev.elapsed_time(e_ev)
        gemm_ms = sum(v for k, v in agg.items() if k in ("agrl_conv2d_bn_act", "agrl_conv2d_stats", "agrl_linear_nobias", "agrl_conv_wgrad", "agrl_gemm_nt_splitk"))
        out["native_breakdown"] = {"entry_point_ms": {k: round(v, 2) for k, v in sorted(agg.items(), key=lambda kv: -kv[1])[:8]},
                                   "launches": len(prof), "gemm_ms": round(gemm_ms, 2), "gemm_tflops": round(fl / gemm_ms / 1e9, 1),
                                   "gemm_frac_of_fp32_mfma_peak": round(fl / gemm_ms / 1e9 / PEAK_TFLOPS["fp32"], 3),
                                   "bound": "mfma (v_mfma_f32_16x16x4_f32: 155 TFLOP/s sustained register-only, tools/mfma_peak.hip)"}
        m.zero_grad()
    except Exception as e:  # noqa: BLE001
        out["native_breakdown"] = {"error": str(e)[:200]}
    finally:
        from torchreid import _hip as _h2
        _h2.PROFILE = None
    out["native"] = {"ms_per_step": round(1e3 * t_nat, 2), "frames_per_s": round(B * S / t_nat, 1), "tflops": round(fl / t_nat / 1e12, 1),
                           "last_loss": round(l_nat, 6)}
    out["native_bf16x3"] = {"ms_per_step": round(1e3 * t_x3, 2), "frames_per_s": round(B * S / t_x3, 1),
                                  "tflops": round(fl / t_x3 / 1e12, 1), "last_loss": round(l_x3, 6)}
    out["stock_torch"] = {"ms_per_step": round(1e3 * t_ref, 2), "frames_per_s": round(B * S / t_ref, 1), "tflops": round(fl / t_ref / 1e12, 1),
                          "last_loss": round(l_ref, 6)}
    out["peak_tflops"] = PEAK_TFLOPS["fp32"]
    out["note"] = ("whole step on libagrl_hip.so: conv trunk, pooling, graph layers, attention pooling, classifiers, label-smoothed "
                   "cross entropy and batch-hard triplet as autograd nodes over C-ABI calls (exact-fp32 MFMA); optimiser = torch Adam")
    return out


def main():
    argv = sys.argv[1:]
    args = parse(argv)
    if args.cpu_baseline_only:
        print(json.dumps(cpu_baseline_child(args.seq_len, args.metric, args.cpu_seconds)), flush=True)
        return
    if args.host_cores > 0:
        # (before torch is imported: its thread pools and the HIP runtime's helper threads inherit the mask)
        os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:args.host_cores])
    if args.precision in ("fp16", "bf16"):
        os.environ["AGRL_HIP_LP16"] = args.precision   # picks the library build; must be set before torchreid is imported (ranks inherit it)
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(launch_ranks(args, argv))

    import torch
    import torch.distributed as dist
    from torchreid import _hip, parallel
    from torchreid import hip_ops as ops

    # ranks that must share GPUs (a 1-GPU development box) cannot use RCCL: fall back to gloo for the control flow
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if world_env > 1 and "AGRL_DIST_BACKEND" not in os.environ and torch.cuda.device_count() < world_env:
        os.environ["AGRL_DIST_BACKEND"] = "gloo"
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    rank, world, local_rank = parallel.init_from_env()
    assert world == args.gpus, "WORLD_SIZE=%d but --gpus %d" % (world, args.gpus)
    # the collective path: N > 1, or N = 1 with AGRL_DIST_FORCE_GROUP=1 (the RCCL branch under a real communicator on one GPU)
    multi = parallel.collectives_active()
    device = torch.device("cuda", local_rank % torch.cuda.device_count())
    torch.cuda.set_device(device)
    _hip.lib()

    B, S = args.batch, args.seq_len
    model, sd = build_model(device, args.precision)
    gen = torch.Generator(device=device)
    gen.manual_seed(0xFF + rank)
    # NCLIPS distinct clip batches rotate through the timed loop (3 x 100.7 MB at the benchmarked size: more than the 256 MiB
    # Infinity Cache, so the stem reads its input from HBM every step, as a real test() loop does); one adjacency per batch
    NCLIPS = 1 if args.graph else 3
    clip_sets = [torch.randn((B, S, 3, 256, 128), device=device, generator=gen) for _ in range(NCLIPS)]
    adj_sets = [synthetic_pose_adjacency(B, S, device, gen) for _ in range(NCLIPS)]
    clips, adj = clip_sets[0], adj_sets[0]
    step_no = [0]
    g_all = torch.Generator().manual_seed(7)
    gallery_cpu = torch.randn((GALLERY_ROWS, FEATURE_DIM), generator=g_all)
    lo, hi = parallel.shard_bounds(GALLERY_ROWS, rank, world)
    lp = args.precision == ops.LP_NAME
    dt_g = ops.LP_DTYPE if lp else torch.float32
    # resident gallery shard, prepared once (normalised rows for cosine / norms for euclidean)
    g_shard = gallery_cpu[lo:hi].to(device)
    if args.metric == "cosine":
        g_op, g_norm = ops.row_l2_normalize(g_shard, True, dt_g), None
    else:
        g_norm = ops.row_sqnorm(g_shard)
        g_op = ops.row_l2_normalize(g_shard, False, dt_g) if lp else g_shard
    dist_out = torch.empty((B * world, hi - lo), dtype=torch.float32, device=device)

    def match(emb):
        q_all = parallel.all_gather_rows(emb)         # RCCL all-gather over xGMI when world > 1
        # the query side of the distance matrix: at N = 1 the forward's tail kernel has already left the normalised rows / norms
        # beside the embeddings it returned (hip_ops.query_operands); gathered rows are normalised here
        q_op, qn = ops.query_operands(model, q_all, args.metric, dt_g)
        if args.metric == "cosine":
            return ops.distmat(q_op, g_op, "cosine", out=dist_out)
        return ops.distmat(q_op, g_op, "euclidean", qn, g_norm, out=dist_out)

    main_stream = torch.cuda.current_stream(device)
    match_stream = torch.cuda.Stream(device=device) if multi else None

    if args.graph:
        side = torch.cuda.Stream(device=device)
        side.wait_stream(main_stream)
        with torch.cuda.stream(side):
            model(clips, adj)                         # warm every lazy allocation / weight pack outside the capture
        main_stream.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            emb_static = model(clips, adj)

        def forward(eager=False):
            if eager:                                 # the instrumented steps time the same kernels launch by launch
                return model(clips, adj)
            graph.replay()
            return emb_static.clone()                 # the match stage may still read it when the next replay starts
    else:
        def forward(eager=False):
            i = step_no[0] % NCLIPS
            step_no[0] += 1
            return model(clip_sets[i], adj_sets[i])

    last_emb = [None]

    def step(eager=False):
        emb = forward(eager)                          # (B, 4096) fp32
        last_emb[0] = emb
        if match_stream is None:
            return match(emb)
        # N > 1: the exchange + match of this batch run on their own HIP stream, so the collective (and the skew
        # between ranks it absorbs) overlaps the next batch's forward instead of stalling it; every step still does
        # the same work, and the closing synchronize() waits for both streams.
        ready = torch.cuda.Event()
        ready.record(main_stream)
        with torch.cuda.stream(match_stream):
            match_stream.wait_event(ready)
            emb.record_stream(match_stream)
            return match(emb)

    def sync():
        if multi:
            dist.barrier()
        torch.cuda.synchronize()

    def reduce_max(x):
        if not multi:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.item()

    for _ in range(args.warmup):
        step()
    sync()
    if os.environ.get("AGRL_BENCH_FAULT_RANK") == str(rank):   # tests/test_gpu_configs.py: a rank that dies mid-run
        os._exit(int(os.environ.get("AGRL_BENCH_FAULT_CODE", "3")))
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last_dist = step()
    sync()
    elapsed_local = time.perf_counter() - t0
    elapsed = reduce_max(elapsed_local)
    per_rank_ms = [1e3 * elapsed_local / args.steps]
    if multi:
        t = torch.tensor([per_rank_ms[0]], dtype=torch.float64, device=device)
        allt = torch.empty((world,), dtype=torch.float64, device=device)
        dist.all_gather_into_tensor(allt, t)
        per_rank_ms = allt.tolist()
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from its last step: the distance matrix of the batch against this rank's
        # gallery shard, and the embeddings it was computed from
        dump_outputs(args.dump_outputs, {"distmat": last_dist, "embeddings": last_emb[0]})

    frames = B * S * world * args.steps
    backend = dist.get_backend() if multi else None
    result = {
        "metric": "frames/sec (fwd+GCN+distmat), MARS seq_len=8",
        "value": round(frames / elapsed, 1),
        "unit": "frames/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": args.precision,
        "data": "synthetic",
        "config": {"workload": "MARS seq_len=8 bs=32/GPU %s fwd+distmat (BASELINE configs[1]): 256x128 frames, VMGN "
                               "ResNet50x2-branch + 2 graph layers, %s distmat vs resident %d x 4096 gallery" %
                               (args.precision, args.metric, GALLERY_ROWS),
                   "global_batch": B * world, "seq_len": S, "frames_per_step": B * S * world,
                   "gallery_rows_per_gpu": hi - lo, "parallelism": "dp%d" % world, "hip_graph": bool(args.graph),
                   "ranks": world, "collective_backend": ("rccl" if backend == "nccl" else backend),
                   "devices_visible": torch.cuda.device_count(), "library": os.path.basename(_hip.LIB_PATH),
                   "per_rank_ms_per_step": [round(x, 3) for x in per_rank_ms],
                   "clip_batches_rotated": NCLIPS, "clip_bytes_rotated": NCLIPS * B * S * 3 * 256 * 128 * 4},
    }
    if not args.full and not args.host_issue_only:
        if rank == 0:
            print(json.dumps(result), flush=True)
        if multi:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- --full from here on
    # three more blocks of the same K steps (each bracketed like the first): the box-to-box and run-to-run spread of this chip
    # is larger than most kernel-level wins, so the line also carries the median block
    block_ms = []
    for _ in range(3):
        sync()
        tb = time.perf_counter()
        for _ in range(args.steps):
            step()
        sync()
        block_ms.append(1e3 * reduce_max(time.perf_counter() - tb) / args.steps)

    # host side of a step (round-5 review, multi-GPU readiness): wall time Python needs to ENQUEUE a step -- the forward's launches,
    # the match stage -- with nothing waited for. At N = 1 the step is kernel-bound; with 8 ranks sharing a host this is the first
    # thing that can break weak scaling, so the line carries it (and a child repeats it on 1/8 of the host's cores, below).
    n_issue = max(1, min(args.steps, 10))
    sync()
    ti = time.perf_counter()
    for _ in range(n_issue):
        step()
    host_issue_ms = 1e3 * (time.perf_counter() - ti) / n_issue
    sync()
    host_total_ms = 1e3 * reduce_max(time.perf_counter() - ti) / n_issue
    host_issue_ms = reduce_max(host_issue_ms)
    if args.host_issue_only:
        if rank == 0:
            print(json.dumps({"host_issue_ms_per_step": round(host_issue_ms, 3), "ms_per_step": round(1e3 * elapsed / args.steps, 3),
                              "ms_per_step_blocks": [round(x, 3) for x in block_ms], "ms_per_step_issue_block": round(host_total_ms, 3),
                              "cpus_allowed": len(os.sched_getaffinity(0)), "steps": args.steps, "hip_graph": bool(args.graph)}), flush=True)
        if multi:
            dist.barrier()
            dist.destroy_process_group()
        return

    # sustained figure: the same step for >= --sustain-seconds (all ranks run the same number of steps)
    sustained = None
    if args.sustain_seconds > 0:
        n_sus = max(args.steps, int(args.sustain_seconds / max(elapsed / args.steps, 1e-6)) + 1)
        if multi:
            t = torch.tensor([n_sus], dtype=torch.int64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            n_sus = int(t.item())
        sync()
        t0 = time.perf_counter()
        for _ in range(n_sus):
            step()
        sync()
        sus_elapsed = reduce_max(time.perf_counter() - t0)
        sustained = (n_sus, sus_elapsed)

    result.update({
        "ms_per_step_blocks": [round(x, 3) for x in block_ms],
        "host_issue_ms_per_step": round(host_issue_ms, 3),
        "host_issue": {"what": "wall time to enqueue one step (forward launches + match stage) with nothing waited for, mean of %d steps; "
                               "max over ranks" % n_issue,
                       "ms_per_step": round(host_issue_ms, 3), "frac_of_step": round(host_issue_ms / (1e3 * elapsed / args.steps), 3),
                       "cpus_allowed": len(os.sched_getaffinity(0))},
        "ms_per_step_median_of_blocks": round(sorted([1e3 * elapsed / args.steps] + block_ms)[2], 3),
    })
    if multi:
        # the ranking step of the sharded evaluation on this batch, once, outside the timed region: per-shard top-50 + candidate
        # merge (parallel.sharded_topk) against a single-process top-50 over the whole gallery on rank 0
        with torch.no_grad():
            q_all = parallel.all_gather_rows(model(clips, adj))
            q_op = ops.row_l2_normalize(q_all, True, dt_g)
            g_cos = g_op if args.metric == "cosine" else ops.row_l2_normalize(g_shard, True, dt_g)
            idx_s, val_s = parallel.sharded_topk(q_op, g_cos, lo, 50, lambda a, b: ops.distmat(a, b, "cosine"), ops.rank_topk)
            rows = torch.tensor([hi - lo], dtype=torch.int64, device=device)
            all_rows = torch.empty((world,), dtype=torch.int64, device=device)
            dist.all_gather_into_tensor(all_rows, rows)
            result["config"]["gallery_rows_all_ranks"] = all_rows.tolist()
            if rank == 0:
                g_full = ops.row_l2_normalize(gallery_cpu.to(device), True, dt_g)
                d_full = ops.distmat(q_op, g_full, "cosine")
                idx_1, val_1 = ops.rank_topk(d_full, 50)
                # tie-aware: a shard's distance columns come from another kernel family than the whole gallery's (different
                # tile shapes: last-bit differences), so a position may legitimately hold the other of two candidates whose
                # full-matrix distances differ by less than that
                tol = 4e-6 if dt_g == torch.float32 else 2e-3
                idx_s = idx_s.to(idx_1.dtype)
                differ = idx_s != idx_1
                d_s = torch.gather(d_full, 1, idx_s.long())
                d_1 = torch.gather(d_full, 1, idx_1.long())
                unexplained = int((differ & ((d_s - d_1).abs() > tol)).sum().item())
                # strict: the index lists themselves (round-5 advice: this key means equality again); the tie-aware reading has its own key
                result["config"]["sharded_top50_equals_single_process"] = bool(torch.equal(idx_s, idx_1))
                result["config"]["sharded_top50_equal_up_to_near_ties"] = bool((val_s - val_1).abs().max().item() <= tol and unexplained == 0)
                result["config"]["sharded_top50_near_tie_tolerance"] = tol
                result["config"]["sharded_top50_swapped_positions"] = int(differ.sum().item())
                result["config"]["sharded_top50_swaps_not_explained_by_a_near_tie"] = unexplained
                result["config"]["sharded_top50_max_abs_diff"] = float((val_s - val_1).abs().max().item())
                del g_full, d_full
    if (args.embedding_error or (lp and not args.no_modes)) and world == 1 and args.precision != "fp32":
        with torch.no_grad():
            e_lp = model(clips, adj).float()
            model.hip_precision = "fp32"
            e_32 = model(clips, adj).float()
            model.hip_precision = args.precision
        result["embedding_max_rel_err_vs_fp32_one_batch"] = float("%.3g" % ((e_lp - e_32).abs().max() / e_32.abs().max()).item())
    if sustained is not None:
        n_sus, sus_elapsed = sustained
        result["sustained_value"] = round(B * S * world * n_sus / sus_elapsed, 1)
        result["sustained_steps"] = n_sus
        result["sustained_seconds"] = round(sus_elapsed, 3)

    # ---- live per-kernel timing (HIP events on the launch stream). Every rank runs the extra steps (they contain
    # the collective); only rank 0 records and reports.
    nprof = max(1, args.profile_steps)
    ag_events = []
    if rank == 0:
        _hip.PROFILE = []
        if multi:
            _orig_ag = parallel.all_gather_rows

            def _timed_ag(local):
                st = torch.cuda.current_stream(device)
                s_ev, e_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s_ev.record(st)
                r = _orig_ag(local)
                e_ev.record(st)
                ag_events.append((s_ev, e_ev))
                return r
            parallel.all_gather_rows = _timed_ag
    for _ in range(nprof):
        step(eager=True)
    sync()
    if rank == 0:
        if multi:
            parallel.all_gather_rows = _orig_ag
            result["config"]["allgather_us"] = round(1e3 * sum(s.elapsed_time(e) for s, e in ag_events) / len(ag_events), 1)
            result["config"]["allgather_bytes_per_rank"] = B * FEATURE_DIM * 4
        prof, _hip.PROFILE = _hip.PROFILE, None
        agg = {}
        cls = {"dom": {"ms": 0.0, "launches": 0, "flops": 0.0}, "pw4": {"ms": 0.0, "launches": 0, "flops": 0.0},
               "duo": {"ms": 0.0, "launches": 0, "flops": 0.0, "bytes": 0.0}}
        DUO_CALLS = ("agrl_conv1x1_packed_res_bn_act", "agrl_conv1x1_packed_res_pool", "agrl_conv1x1_packed_dual_duo", "agrl_conv1x1_packed_dual_strided")
        for name, s_ev, e_ev, tag in prof:
            a = agg.setdefault(name, {"ms": 0.0, "launches": 0, "flops": 0.0, "bytes": 0.0})
            ms = s_ev.elapsed_time(e_ev)
            a["ms"] += ms
            a["launches"] += 1
            if tag:
                a["flops"] += tag["flops"]
                a["bytes"] += tag["bytes"]
                c = tag.get("conv")
                which = None
                # the 3x3 stride-1 convs of layers 3 and 4 (>= 256 input channels on 16 x 8 maps): conv3x3_fat_kernel through
                # agrl_conv3x3_packed_bn_act (conv3x3_wide_kernel through agrl_conv2d_bn_act with AGRL_HIP_CONV3X3_PACKED=0)
                if lp and c and c[0] == 3 and c[1] == 1 and c[2] >= 256:
                    which = "dom"
                elif lp and c and c[0] == 1 and max(c[2], c[3]) >= 2048:   # the pointwise convs of the layer-4 branches
                    which = "pw4"
                elif lp and name in ("agrl_conv1x1_bn_act_pool", "agrl_conv1x1_dual_bn_act", "agrl_conv1x1_packed_res_pool"):
                    which = "pw4"
                if which:
                    cls[which]["ms"] += ms
                    cls[which]["launches"] += 1
                    cls[which]["flops"] += tag["flops"]
                if lp and name in DUO_CALLS:   # every launch of conv1x1_duo_kernel (<false> + <true> in profiles/*_bench_kernel_stats.csv)
                    cls["duo"]["ms"] += ms
                    cls["duo"]["launches"] += 1
                    cls["duo"]["flops"] += tag["flops"]
                    cls["duo"]["bytes"] += tag["bytes"]
        kernels = {}
        for name, a in sorted(agg.items(), key=lambda kv: -kv[1]["ms"]):
            sec = a["ms"] * 1e-3
            kernels[name] = {"ms_per_step": round(a["ms"] / nprof, 4), "launches_per_step": a["launches"] // nprof,
                             "avg_launch_us": round(1e3 * a["ms"] / a["launches"], 2)}
            if a["flops"]:
                kernels[name]["tflops"] = round(a["flops"] / sec / 1e12, 2)
                kernels[name]["gbs"] = round(a["bytes"] / sec / 1e9, 1)
        # ---- the HBM-bound third of the step, launch by launch (review item: stem + layers 1-2 + the entry of layer 3): algorithmic
        # bytes of each call over its own duration, against the 8 TB/s roofline and against what a float4 copy of 256 MB reaches on
        # THIS chip in THIS run (the "copy ceiling": read + write bytes per second)
        if lp:
            per_step = len(prof) // nprof
            first_seam = next((i for i in range(per_step) if prof[i][0] == "agrl_bottleneck_seam"), None)
            # (with the first block of layer 3 as ONE two-source GEMM -- conv3 + the stride-2 downsample conv, round 5 -- the region
            # ends behind that launch: it then holds layer 3's first conv3 as well, which the seam launch used to carry)
            l3_dual = next((i for i in range(per_step) if prof[i][0] == "agrl_conv1x1_packed_dual_strided" and prof[i][3]
                            and tuple(prof[i][3]["conv"][4:6]) == (16, 8)), None)
            if l3_dual is not None and (first_seam is None or l3_dual < first_seam):
                first_seam = l3_dual + 1
            if first_seam is not None and all(prof[k * per_step + i][0] == prof[i][0] for k in range(nprof) for i in range(first_seam)):
                cp_src = torch.empty((64 << 20,), dtype=torch.float32, device=device)
                cp_dst = torch.empty_like(cp_src)
                best = None
                for rep in range(5):
                    s_ev, e_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s_ev.record()
                    cp_dst.copy_(cp_src)
                    e_ev.record()
                    e_ev.synchronize()
                    if rep >= 1:
                        best = s_ev.elapsed_time(e_ev) if best is None else min(best, s_ev.elapsed_time(e_ev))
                copy_gbs = 2.0 * cp_src.numel() * 4 / (best * 1e-3) / 1e9
                del cp_src, cp_dst
                rows, tot_ms, tot_b = [], 0.0, 0.0
                for i in range(first_seam):
                    name, tag = prof[i][0], prof[i][3]
                    ms = sum(prof[k * per_step + i][1].elapsed_time(prof[k * per_step + i][2]) for k in range(nprof)) / nprof
                    c = tag.get("conv") if tag else None
                    label = name.replace("agrl_", "") + (" %dx%d s%d %d->%d @%dx%d" % (c[0], c[0], c[1], c[2], c[3], c[4], c[5]) if c else "")
                    gbs = tag["bytes"] / (ms * 1e-3) / 1e9 if tag else None
                    rows.append({"call": label, "us": round(1e3 * ms, 1), "algorithmic_mb": round(tag["bytes"] / 1e6, 1) if tag else None,
                                 "gbs": round(gbs, 0) if gbs else None, "frac_of_8tbs": round(gbs / PEAK_HBM_GBS, 3) if gbs else None,
                                 "frac_of_copy": round(gbs / copy_gbs, 3) if gbs else None,
                                 "tflops": round(tag["flops"] / (ms * 1e-3) / 1e12, 0) if tag else None})
                    tot_ms += ms
                    tot_b += tag["bytes"] if tag else 0.0
                result["roofline_hbm_bound_trunk"] = {
                    "bound": "hbm", "what": ("stem + layer 1 + layer 2 + the first block of layer 3 through its conv3 + downsample GEMM" if l3_dual is not None else
                                             "stem + layer 1 + layer 2 + the first block of layer 3 (up to the first seam launch)") +
                                            ", HIP events around each C-ABI call (each carries ~2 us of launch latency)",
                    "copy_ceiling_gbs": round(copy_gbs, 0), "ms_per_step": round(tot_ms, 4), "algorithmic_mb_per_step": round(tot_b / 1e6, 1),
                    "achieved": round(tot_b / (tot_ms * 1e-3) / 1e9, 0), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                    "frac": round(tot_b / (tot_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                    "frac_of_copy": round(tot_b / (tot_ms * 1e-3) / 1e9 / copy_gbs, 4), "launches": rows}
        # the conv family: every conv launch (generic / persistent / wide implicit GEMM, 3x3 patch kernels, the fused
        # layer-1 block and layer-2 tail, the pool-fused last conv)
        a = {"ms": 0.0, "launches": 0, "flops": 0.0}
        for fam in ("agrl_conv2d_bn_act", "agrl_conv1x1_bn_act_pool", "agrl_bottleneck_tail", "agrl_bottleneck_block",
                    "agrl_conv1x1_dual_bn_act", "agrl_conv3x3_packed_bn_act", "agrl_conv1x1_packed_bn_act", "agrl_bottleneck_seam",
                    "agrl_conv1x1_packed_res_pool", "agrl_conv1x1_packed_res_bn_act", "agrl_conv1x1_packed_dual_duo",
                    "agrl_conv1x1_packed_dual_strided", "agrl_conv2d_bn_act_split16", "agrl_conv1x1_split16", "agrl_conv1x1_split16_dual",
                    "agrl_conv1x1_split16_pool", "agrl_conv3x3_packed_split16"):
            if fam in agg:
                for key in a:
                    a[key] += agg[fam][key]
        achieved = a["flops"] / (a["ms"] * 1e-3) / 1e12
        peak = PEAK_TFLOPS[args.precision]
        # HBM traffic per launch: NOT measured in this run -- PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate
        # runs of this same command, tools/collect_profiles.sh) are committed under profiles/ and quoted with their source
        traffic = fam_traffic = traffic_src = duo_traffic = None
        for tname in ("traffic_r06.json", "traffic_r05.json", "traffic_r04.json", "traffic_r03.json", "traffic_r02.json", "traffic_r01.json"):
            tpath = os.path.join(ROOT, "profiles", tname)
            if os.path.exists(tpath):
                try:
                    tj = json.load(open(tpath)).get(args.precision, {})
                    fam_traffic = tj.get("igemm_bytes_per_launch")
                    k3 = tj.get("other_kernels", {}).get("conv3x3_fat_kernel" if ops.conv3x3_packed_enabled() else "conv3x3_wide_kernel")
                    if k3:
                        traffic = k3["fetch_bytes_per_launch"] + (k3["write_bytes_per_launch"] or 0.0)
                    kd = tj.get("other_kernels", {}).get("conv1x1_duo_kernel")
                    duo_traffic = kd["fetch_bytes_per_launch"] + (kd["write_bytes_per_launch"] or 0.0) if kd else None
                    traffic_src = "profiles/%s (earlier rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, not this run)" % tname
                    break
                except Exception:
                    traffic = fam_traffic = duo_traffic = None
        family = {"bound": "mfma (layers 3-4) / hbm (layers 1-2)",
                  "kernel": "conv implicit-GEMM family (agrl_conv2d_bn_act + agrl_conv3x3_packed_bn_act + agrl_conv1x1_packed_bn_act + agrl_conv1x1_dual_bn_act + agrl_conv1x1_bn_act_pool / agrl_conv1x1_packed_res_pool + agrl_bottleneck_tail + agrl_bottleneck_block + agrl_bottleneck_seam)",
                  "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
                  "traffic": fam_traffic, "traffic_source": traffic_src, "flops_per_launch": round(a["flops"] / a["launches"], 1),
                  "avg_launch_us": round(1e3 * a["ms"] / a["launches"], 2), "ms_per_step": round(a["ms"] / nprof, 4)}
        dom = cls["dom"]
        if dom["launches"]:
            # THE dominant kernel by time (profiles/*_bench_kernel_stats.csv): conv3x3_fat_kernel<1> (layer 4) + conv3x3_half_kernel (layer 3)
            ach = dom["flops"] / (dom["ms"] * 1e-3) / 1e12
            result["roofline"] = {"bound": "mfma", "kernel": "conv3x3_fat_kernel<1> + conv3x3_half_kernel (3x3 stride-1 convs of layers 3-4: layer 4 one 16 x 8 block x 256 channels per four-wave workgroup, two workgroups per CU; layer 3 two half-width workgroups per block; csrc/conv3x3_fat.hip)" if ops.conv3x3_packed_enabled() else "conv3x3_wide_kernel<0, 128> + <0, 256> (csrc/conv3x3_wide.hip; AGRL_HIP_CONV3X3_PACKED=0)",
                                  "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                                  "traffic": traffic, "traffic_source": traffic_src,
                                  "flops_per_launch": round(dom["flops"] / dom["launches"], 1),
                                  "avg_launch_us": round(1e3 * dom["ms"] / dom["launches"], 2),
                                  "launches_per_step": dom["launches"] // nprof, "ms_per_step": round(dom["ms"] / nprof, 4)}
            result["roofline_conv_family"] = family
            # Which kernel is "the dominant one" is decided by THIS run's times: until late in round 5 the 3x3 family above; since all of
            # layer 4's 1x1 GEMMs (and the strided first blocks of layers 2 / 3) run through conv1x1_duo_kernel, its 14 launches per step
            # outweigh the 3x3 family's 11. `roofline` carries the larger one, both stay in the line under their own names.
            duo = cls["duo"]
            result["roofline_conv3x3"] = dict(result["roofline"])
            if duo["launches"]:
                ach_d = duo["flops"] / (duo["ms"] * 1e-3) / 1e12
                result["roofline_conv1x1_duo"] = {
                    "bound": "mfma", "kernel": "conv1x1_duo_kernel<false> + <true> (every 1x1 GEMM of layer 4 -- conv1s, conv3 + downsample, conv3 + residual stored / pooled -- and the two-source first blocks of layers 2 / 3: two co-resident four-wave workgroups per CU, 128 x 256 tiles; csrc/conv1x1_duo.hip)",
                    "achieved": round(ach_d, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach_d / peak, 4),
                    "traffic": duo_traffic, "traffic_source": traffic_src, "algorithmic_bytes_per_launch": round(duo["bytes"] / duo["launches"], 1),
                    "flops_per_launch": round(duo["flops"] / duo["launches"], 1), "avg_launch_us": round(1e3 * duo["ms"] / duo["launches"], 2),
                    "launches_per_step": duo["launches"] // nprof, "ms_per_step": round(duo["ms"] / nprof, 4),
                    "hbm_frac_at_8tbs": round(duo["bytes"] / (duo["ms"] * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)}
                # round-5 advice: `roofline` stays bound to ONE kernel from round to round -- conv1x1_duo_kernel, the kernel the
                # round-5 review names (14 launches per step) -- whichever family happened to be slower in this run; the 3x3 family
                # is always in the line as roofline_conv3x3
                result["roofline"] = dict(result["roofline_conv1x1_duo"])
            result["roofline"]["time_in_this_run"] = "HIP events around the C-ABI calls: %s" % (
                "conv1x1_duo_kernel %.3f ms vs the 3x3 family %.3f ms per step" % (duo["ms"] / nprof, dom["ms"] / nprof))
        else:  # fp32 / split modes: one generic kernel serves every conv
            result["roofline"] = family
        pw = cls["pw4"]
        if pw["launches"]:
            ach = pw["flops"] / (pw["ms"] * 1e-3) / 1e12
            result["roofline_pointwise_layer4"] = {
                "bound": "mfma", "kernel": "1x1 convs of the two layer-4 branches (conv1x1_duo_kernel: conv1s, conv3 + downsample, conv3 + residual, the pool-fused last conv; AGRL_HIP_CONV1X1_DUO* = 0: conv1x1_fat_kernel / igemm_wide_kernel)",
                "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                "launches_per_step": pw["launches"] // nprof, "ms_per_step": round(pw["ms"] / nprof, 4)}

        # ---- the two HBM-bound kernels the north star names, with the chip's read-stream yardstick at the same size
        scratch = torch.empty((64 << 20,), dtype=torch.float32, device=device)  # 256 MB: rotate so no pass hits a warm MALL

        def yardstick(nbytes):
            """Best single-pass read rate of this chip at this size: grid sweep, rotating through a 256 MB buffer."""
            best = None
            span = scratch.numel() * 4 - nbytes
            for wgs in (512, 1024, 2048, 4096):
                for rep in range(5):
                    off = ((rep * (48 << 20)) % max(span, 1)) // 16 * 4
                    s_ev, e_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s_ev.record()
                    ops.read_stream(scratch[off:], nbytes, workgroups=wgs)
                    e_ev.record()
                    e_ev.synchronize()
                    ms = s_ev.elapsed_time(e_ev)
                    if rep >= 1 and (best is None or ms < best):
                        best = ms
            return nbytes / (best * 1e-3) / 1e9

        V, Cc, n_layers = S * 7, 2048, 2
        esz = 2.0 if lp else 4.0

        def gcn_rooflines(agg_, B_, layers_):
            """The GraphLayer as it runs (vmgn.py:142-172). Commuted form (default): gram -> finalize -> P = G f -> ONE GEMM
            with BatchNorm1d + LeakyReLU + residual mix in its epilogue, i.e. SURVEY 8(d)'s "Linear fused in" unit: 2 V C 4 +
            V^2 4 bytes per tracklet (+ W once), 2 V C^2 + 4 V^2 C flops per tracklet, MFMA-bound; its HBM-bound part (gram +
            finalize + G f: read f, read adj, write the GEMM operand) is reported against the 8 TB/s roofline and against the
            chip's own one-pass read rate at that byte count. Round-1/2 form (AGRL_HIP_GCN_COMMUTE=0): the SURVEY's unfused
            message-pass unit (1.389 MB per tracklet-layer over gram + finalize + propagate)."""
            names_new = [n for n in ("agrl_graph_gram", "agrl_graph_finalize", "agrl_graph_apply", "agrl_graph_tracklet_operand", "agrl_graph_linear_mix") if n in agg_]
            names_old = [n for n in ("agrl_graph_message_pass", "agrl_graph_gram", "agrl_graph_finalize", "agrl_graph_propagate") if n in agg_]
            out_ = {}
            if "agrl_graph_linear_mix" in agg_:
                ms_all = sum(agg_[n]["ms"] for n in names_new)
                hbm_names = [n for n in names_new if n != "agrl_graph_linear_mix"]
                ms_hbm = sum(agg_[n]["ms"] for n in hbm_names)
                flops = (2.0 * V * Cc * Cc + 4.0 * V * V * Cc) * B_
                bytes_layer = (2.0 * V * Cc * 4 + V * V * 4) * B_ + Cc * Cc * esz
                bytes_hbm = (V * Cc * 4 + V * V * 4 + V * Cc * esz) * B_
                us_layer = 1e3 * ms_all / layers_
                tf = flops * layers_ / (ms_all * 1e-3) / 1e12
                gbs = bytes_hbm * layers_ / (ms_hbm * 1e-3) / 1e9
                ygbs = yardstick(int(bytes_hbm))
                out_["roofline_gcn_layer"] = {
                    "bound": "mfma", "achieved": round(tf, 1), "peak": PEAK_TFLOPS[args.precision], "unit": "TFLOP/s",
                    "frac": round(tf / PEAK_TFLOPS[args.precision], 4), "tracklets": B_, "us_per_layer": round(us_layer, 2),
                    "flops_per_layer": flops, "algorithmic_bytes_per_layer": bytes_layer,
                    "algorithmic_gbs": round(bytes_layer * layers_ / (ms_all * 1e-3) / 1e9, 1),
                    "kernels_us": {n: round(1e3 * agg_[n]["ms"] / agg_[n]["launches"], 2) for n in names_new},
                    "what": "whole GraphLayer, Linear fused in (SURVEY 8d: 0.930 MB + 470 MFLOP per tracklet): gram + finalize + G f + "
                            "(G f) W^T with the BatchNorm / LeakyReLU / residual epilogue"}
                out_["roofline_gcn_message_pass"] = {
                    "bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4),
                    "tracklets": B_, "bytes_per_layer": bytes_hbm, "us_per_layer": round(1e3 * ms_hbm / layers_, 2),
                    "kernels": {n: round(1e3 * agg_[n]["ms"] / agg_[n]["launches"], 2) for n in hbm_names},
                    "what": "HBM-bound part of the commuted GraphLayer: sim + normalise + mix with the pose graph + P = G f "
                            "(read f, read adj, write the GEMM operand); BatchNorm / LeakyReLU / residual ride in the GEMM's epilogue",
                    "read_stream_yardstick_gbs": round(ygbs, 1), "frac_of_yardstick": round(gbs / ygbs, 4)}
            elif names_old:
                ms = sum(agg_[n]["ms"] for n in names_old)
                unit_bytes = GCN_UNIT_BYTES(V, Cc) * B_
                gbs = unit_bytes * layers_ / (ms * 1e-3) / 1e9
                ygbs = yardstick(int(unit_bytes))
                out_["roofline_gcn_message_pass"] = {
                    "bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4),
                    "tracklets": B_, "bytes_per_layer": unit_bytes, "us_per_layer": round(1e3 * ms / layers_, 2),
                    "kernels": {n: round(1e3 * agg_[n]["ms"] / agg_[n]["launches"], 2) for n in names_old},
                    "what": "SURVEY 8(d) message-pass unit (sim + normalise + mix + G h + BN + LeakyReLU + residual; Linear excluded): "
                            "1.389 MB per tracklet-layer over the time of ALL its kernels",
                    "read_stream_yardstick_gbs": round(ygbs, 1), "frac_of_yardstick": round(gbs / ygbs, 4)}
            return out_

        result.update(gcn_rooflines(agg, B, n_layers * nprof))
        # the same layers at 256 tracklets per GPU (BASELINE configs[2]'s global batch on ONE GPU): the size at which the
        # kernels are past their launch / drain floor
        try:
            from torchreid.models import _vmgn_hip as eng
            pack = eng.pack_weights(model, device, args.precision)
            g256 = torch.Generator(device=device)
            g256.manual_seed(256)
            B2 = 256
            nodes2 = torch.rand((B2, 1, Cc), device=device, generator=g256) + 0.02 * torch.randn((B2, V, Cc), device=device, generator=g256)
            adj2 = synthetic_pose_adjacency(B2, S, device, g256)
            nodes2_lp = nodes2.to(ops.LP_DTYPE) if lp else None
            commute = eng.gcn_commute_enabled(model)
            for _ in range(2):
                eng.hip_graph_layers(nodes2, nodes2_lp, adj2, pack, commute=commute)
            torch.cuda.synchronize()
            _hip.PROFILE = []
            for _ in range(5):
                eng.hip_graph_layers(nodes2, nodes2_lp, adj2, pack, commute=commute)
            torch.cuda.synchronize()
            prof2, _hip.PROFILE = _hip.PROFILE, None
            agg2 = {}
            for name, s_ev, e_ev, tag in prof2:
                a2 = agg2.setdefault(name, {"ms": 0.0, "launches": 0})
                a2["ms"] += s_ev.elapsed_time(e_ev)
                a2["launches"] += 1
            result["gcn_at_256_tracklets"] = gcn_rooflines(agg2, B2, n_layers * 5)
            del nodes2, adj2, nodes2_lp
        except Exception as e:  # noqa: BLE001
            _hip.PROFILE = None
            result["gcn_at_256_tracklets"] = {"error": repr(e)[:300]}
        if "agrl_distmat" in agg and agg["agrl_distmat"]["bytes"]:
            names = [n for n in ("agrl_distmat", "agrl_row_l2_normalize") if n in agg]
            ms_all = sum(agg[n]["ms"] for n in names)
            gbs = agg["agrl_distmat"]["bytes"] / (agg["agrl_distmat"]["ms"] * 1e-3) / 1e9
            gbs_all = agg["agrl_distmat"]["bytes"] / (ms_all * 1e-3) / 1e9
            bytes_launch = agg["agrl_distmat"]["bytes"] / agg["agrl_distmat"]["launches"]
            ygbs = yardstick(int(bytes_launch))
            result["roofline_distmat"] = {"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                          "frac": round(gbs / PEAK_HBM_GBS, 4), "bytes_per_launch": bytes_launch,
                                          "avg_launch_us": round(1e3 * agg["agrl_distmat"]["ms"] / agg["agrl_distmat"]["launches"], 2),
                                          "achieved_incl_query_normalise": round(gbs_all, 1),
                                          "read_stream_yardstick_gbs": round(ygbs, 1), "frac_of_yardstick": round(gbs / ygbs, 4)}
            # the same kernel against an 8 x longer gallery (97 440 rows, 798 MB in bf16): at 100 MB a launch is ~6 us of ramp /
            # drain on top of ~18 us of streaming, so the fraction above is bounded by the SIZE; this one shows the kernel's rate
            try:
                if args.metric == "cosine":
                    rows8 = 8 * GALLERY_ROWS
                    g8 = g_op.repeat(-(-rows8 // g_op.shape[0]), 1)[:rows8].contiguous()   # bandwidth does not care about the values
                    q8 = ops.row_l2_normalize(torch.randn((B, FEATURE_DIM), device=device), True, g_op.dtype)
                    out8 = torch.empty((B, rows8), dtype=torch.float32, device=device)
                    ts8 = []
                    for _ in range(4):
                        s_ev, e_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s_ev.record()
                        for _i in range(4):   # back to back: the host's launch cost hides under the previous launch
                            ops.distmat(q8, g8, "cosine", out=out8)
                        e_ev.record()
                        e_ev.synchronize()
                        ts8.append(s_ev.elapsed_time(e_ev) / 4.0)
                    t8 = sorted(ts8[1:])[len(ts8[1:]) // 2]
                    b8 = g_op.element_size() * (B + rows8) * FEATURE_DIM + 4.0 * B * rows8
                    result["roofline_distmat_8x_gallery"] = {"bound": "hbm", "achieved": round(b8 / (t8 * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                                             "frac": round(b8 / (t8 * 1e-3) / 1e9 / PEAK_HBM_GBS, 4), "gallery_rows": rows8,
                                                             "bytes_per_launch": b8, "launch_us": round(1e3 * t8, 1)}
                    del g8, q8, out8
            except Exception as e:  # noqa: BLE001
                result["roofline_distmat_8x_gallery"] = {"error": repr(e)[:200]}
        del scratch
        result["kernels"] = kernels
        if world == 1:
            acc = None
            if not args.no_modes and lp:
                try:
                    result["modes"] = modes_block(model, clips, adj, g_shard, args.metric)
                except Exception as e:  # noqa: BLE001
                    result["modes"] = {"error": repr(e)[:300]}
            if not args.no_accuracy:
                acc = accuracy_block(model, device, S, args.metric)
                emb = acc.pop("_embeddings", None)
                result["accuracy"] = acc
                LPN = ops.LP_NAME
                result["rank1"] = acc[LPN]["rank1"]
                result["mAP"] = acc[LPN]["mAP"]
                result["dtype_note"] = ("%s storage and MFMA operands, fp32 accumulation (BASELINE configs[1] names bf16, configs[4] fp16: the two "
                                        "have the same MFMA rate on gfx950 and each has its own build of the library; fp16 is the default because its "
                                        "8 x smaller rounding error keeps the embeddings within the north star's 1e-3 of the exact-fp32 path: max "
                                        "|difference| / max |embedding| = %.2e on the timed batch, `embedding_max_rel_err_vs_fp32_one_batch`; %s). "
                                        "On the 625-identity split its top-1 gallery index agrees with the exact-fp32 mode for %.4f of the 1980 "
                                        "queries and the top-50 lists agree position by position for %.4f (Rank-1 / mAP deltas in `accuracy`); "
                                        "the other 16-bit build is timed in `lp16_other`, the fp32 and bf16x3 modes in `modes`"
                                        % (LPN, result.get("embedding_max_rel_err_vs_fp32_one_batch", float("nan")),
                                           "the parity tests hold fp16 to 1e-3 against the CPU oracle" if LPN == "fp16" else "bf16 does not meet 1e-3",
                                           acc["top1_index_agreement"], acc["top50_index_agreement"]))
                result["top1_index_agreement_%s_vs_fp32" % LPN] = acc["top1_index_agreement"]
                # the index-exact modes in top-level fields: frames/s of this run (`modes`) beside their agreement with the ORACLE's
                # ranked lists on the full split (tests/golden/fullsplit_oracle.npz)
                ie = {}
                for mode in ("fp32", "bf16x3", "fp16x3"):
                    vo = acc.get(mode + "_vs_oracle")
                    if vo:
                        ie[mode] = {"frames_per_s": (result.get("modes", {}).get(mode) or {}).get("frames_per_s"),
                                    "top1_index_agreement_vs_oracle": vo["top1_index_agreement"],
                                    "swaps_not_explained_by_a_near_tie": vo["swaps_not_explained_by_a_near_tie"],
                                    "queries_with_identical_top50": vo["queries_with_identical_top50"], "mAP_delta_vs_oracle": vo["mAP_delta"]}
                vo = acc.get(LPN + "_vs_oracle")
                if vo:
                    ie[LPN] = {"frames_per_s": result["value"], "top1_index_agreement_vs_oracle": vo["top1_index_agreement"],
                               "swaps_not_explained_by_a_near_tie": vo["swaps_not_explained_by_a_near_tie"],
                               "queries_with_identical_top50": vo["queries_with_identical_top50"], "mAP_delta_vs_oracle": vo["mAP_delta"]}
                result["index_exactness_by_mode"] = ie
            else:
                emb = None
            if not args.no_modes and lp:
                result["lp16_other"] = other_lp16_child(args)
            if not args.no_config5:
                result["config5"] = config5_block(device, emb, args.metric)
            if not args.no_config4:
                del model, clips
                torch.cuda.empty_cache()
                result["config4_train_step"] = config4_block(device)
            if not args.no_host_issue:
                result["host_issue"]["restricted"] = host_issue_child(args)
            if not args.no_cpu_baseline:
                result["cpu_baseline"] = cpu_baseline(S, args.metric, args.cpu_seconds)
        print(json.dumps(result), flush=True)
    if multi:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
