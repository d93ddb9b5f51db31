"""One GraphLayer (vmgn.py:142-172) at node counts past one workgroup's LDS -- the forms hip_ops.graph_forms names 'tiled', 'rows',
'chunked', 'hbm' -- against the same formulas written with torch ops (bmm, exp, normalize) on the same GPU, in the same process:
  eval   graph matrix -> P = G f -> Linear with the BatchNorm / LeakyReLU / residual epilogue, fp32
  train  forward + backward of the layer (models/_train_hip.graph_layer_train against the stock module)
HIP events, alternating blocks, two warm-up rounds, the median of the rest. Shapes: P = 15 parts at seq_len 8 and 15 (the driver's
--num-split 8 --pyramid-part), P = 7 at 146 frames, and a whole 1000-frame tracklet of --test-sample all.
usage: graph_large_bench.py [--out FILE] [--rounds N] [B V C ...]     (default FILE: profiles/graph_large_bench.txt)"""
import copy, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "agrl.pytorch_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
from torchreid import hip_ops as ops
from torchreid.models import _train_hip as T
from torchreid.models.vmgn import GraphLayer

dev = "cuda:0"
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "graph_large_bench.txt")
rounds = 8
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i:i + 2]
if "--rounds" in args:
    i = args.index("--rounds")
    rounds = int(args[i + 1])
    del args[i:i + 2]
shapes = [tuple(int(v) for v in args[i:i + 3]) for i in range(0, len(args), 3)] or [(32, 120, 2048), (32, 225, 2048), (4, 1022, 2048), (1, 7000, 2048)]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fns, reps):
    """name -> fn, run in alternating blocks of ``reps`` calls -> name -> median microseconds per call."""
    times = {k: [] for k in fns}
    for rnd in range(rounds + 2):
        for name, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            if rnd >= 2:
                times[name].append(s.elapsed_time(e) * 1000.0 / reps)
    return {k: statistics.median(v) for k, v in times.items()}


say("GraphLayer past one workgroup's LDS: native forms against the same formulas in torch ops, %s, fp32" % torch.cuda.get_device_name(0))
for B, V, C in shapes:
    g = torch.Generator().manual_seed(V)
    f = (torch.rand((B, 1, C), generator=g) * 0.2 + 0.05 * torch.randn((B, V, C), generator=g)).to(dev)
    up = torch.triu((torch.rand((B, V, V), generator=g) > 0.5).float(), diagonal=1)
    adj = (up + up.transpose(1, 2)).to(dev)
    layer = GraphLayer(C, C).to(dev)
    with torch.no_grad():
        layer.linear.weight.copy_((torch.randn((C, C), generator=g) * 0.02).to(dev))
    w = layer.linear.weight.detach()
    sc, sh = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
    dout = torch.randn((B, V, C), generator=g).to(dev)

    def native_eval():
        G = ops.graph_matrix(f, adj, True, True)
        P = ops.graph_apply_operand(G, f, torch.float32)
        return ops.graph_linear_mix(P, w, f, sc, sh, 0.1, 0.1)

    def torch_eval():
        gm = torch.bmm(f, f.transpose(1, 2))
        n = torch.diagonal(gm, dim1=1, dim2=2)
        d = (n[:, :, None] + n[:, None, :] - 2 * gm).clamp(min=1e-12).sqrt()
        sim = torch.nn.functional.normalize(2 / (torch.exp(d) + 1), p=1, dim=2)
        G = (torch.nn.functional.normalize(adj, p=1, dim=2) + sim) / 2
        y = torch.nn.functional.leaky_relu((torch.bmm(G, f) @ w.t()) * sc + sh, 0.1)
        return 0.9 * f + 0.1 * y

    nat, ref = layer.train(), copy.deepcopy(layer).train()

    def native_train():
        x = f.detach().requires_grad_(True)
        T.graph_layer_train(nat, x, adj).backward(dout)
        return x.grad

    def torch_train():
        x = f.detach().requires_grad_(True)
        ref(x, adj).backward(dout)
        return x.grad

    with torch.no_grad():
        a, b = native_eval(), torch_eval()
    ga, gb = native_train(), torch_train()
    torch.cuda.synchronize()
    e_eval = ((a - b).abs().max() / b.abs().max()).item()
    e_grad = ((ga - gb).abs().max() / gb.abs().max()).item()
    reps = max(1, min(20, int(2e11 / (2.0 * B * V * C * (C + 2 * V)))))
    with torch.no_grad():
        te = timed({"native": native_eval, "torch": torch_eval}, reps)
    tt = timed({"native": native_train, "torch": torch_train}, max(1, reps // 3))
    forms = ops.graph_forms(V, C)
    say("B=%d V=%d C=%d  forms: %s" % (B, V, C, " ".join("%s=%s" % kv for kv in sorted(forms.items()))))
    say("    eval  forward            native %10.1f us   torch %10.1f us   native / torch %5.2f   (max rel difference %.1e)" % (
        te["native"], te["torch"], te["native"] / te["torch"], e_eval))
    say("    train forward + backward native %10.1f us   torch %10.1f us   native / torch %5.2f   (d f max rel difference %.1e)" % (
        tt["native"], tt["torch"], tt["native"] / tt["torch"], e_grad))
    del f, adj, layer, nat, ref, a, b, ga, gb, dout
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
