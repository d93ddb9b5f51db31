"""The host routes of the six models as data: which C-ABI entry points a forward (and a train step's forward + backward) calls, in
order, and the SHA-256 of what comes out. Recorded once on a tree whose host path is trusted and replayed on a changed one by
tests/test_gpu_host_routes.py: a host-side refactor must give the same entry points in the same order and the same bits.

Only the public surface is used -- models.init_model, model(x, adj) / model(x), the hip_precision / hip_train_precision attributes and
a wrapper over hip_ops.call -- so the same script runs on both trees.

  eval    all six models x (fp32, the library's 16-bit type, bf16x3, fp16x3) x two frame sizes: 64 x 32 at (B, S) = (2, 4) -- the generic
          routes and agrl_part_pool -- and 256 x 128 at (1, 4): 16 x 8 layer-4 maps, a 512-pixel layer-3 map, so the seam, packed, duo,
          strided-dual, pooled-epilogue and plane routes. Three forwards each: the first (its trace includes the pack-time entry
          points), a second (which shows none) and a third on uint8 NHWC frames. Recipe weights (tests/recipe.py); ganet with
          pam_layer.gamma and every graph layer's gamma at 0.1, so that its kernels run.
  train   vmgn, gsta, ganet with consistent_loss, loss {'xent', 'htri'}, (B, S) = (2, 5), 64 x 32 frames, hip_train_precision fp32 and
          bf16x3: xent + triplet through the package's losses, backward(). Stored: the entry points across forward and backward, the
          SHA-256 of the loss and of three gradients, and the next draw of numpy's and torch's global generators.

GPU only. usage:
    python tools/record_host_routes.py --out a.json          (run it twice, in two processes)
    python tools/record_host_routes.py --merge a.json b.json tests/golden/host_routes.json
--merge fails when an entry-point list differs between the two runs, and stores null for a hash that does (a case that is not
bit-reproducible cannot serve as a criterion; its name is printed)."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "agrl.pytorch_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]
import numpy as np
import torch

DEV = "cuda:0"
KINDS = ("vmgn", "gsta", "ganet", "res50tp", "simple_sta", "sta")
TRAIN_KINDS = ("vmgn", "gsta", "ganet")
SIZES = {"64x32": (2, 4, 64, 32, 1), "256x128": (1, 4, 256, 128, 2)}      # B, S, H, W, seed
# the keyword set the reference driver passes to every architecture, plus ganet's knn
KW = dict(num_classes=5, loss={"xent", "htri"}, last_stride=1, num_parts=3, num_scale=1, num_split=4, pyramid_part=True, num_gb=2,
          use_pose=True, learn_graph=True, consistent_loss=True, bnneck=True)
_MODELS = {}


def precisions():
    from torchreid import hip_ops as ops
    return ("fp32", ops.LP_NAME, "bf16x3", "fp16x3")


def eval_cases():
    return ["%s/%s/%s" % (k, p, s) for k in KINDS for p in precisions() for s in SIZES]


def train_cases():
    return ["%s/%s" % (k, p) for k in TRAIN_KINDS for p in ("fp32", "bf16x3")]


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def model(kind):
    """(model on the device, its recipe state dict): built once per kind"""
    if kind not in _MODELS:
        from recipe import recipe_state_dict
        from torchreid import models
        m = models.init_model(kind, **dict(KW, knn=4) if kind == "ganet" else KW)
        sd = recipe_state_dict(m.state_dict(), seed=0)
        _MODELS[kind] = (m.to(DEV), sd)
        reset(kind)
    return _MODELS[kind]


def reset(kind):
    m, sd = _MODELS[kind]
    m.load_state_dict(sd)
    if kind == "ganet":
        with torch.no_grad():
            m.pam_layer.gamma.fill_(0.1)
        for layer in m.graph_layers:
            layer.gamma = 0.1
    m.zero_grad(set_to_none=True)
    m.invalidate_hip_cache()


class traced(object):
    """hip_ops.call wrapped: every entry point's name, in call order"""

    def __enter__(self):
        from torchreid import hip_ops as ops
        self.ops, self.real, self.names = ops, ops.call, []
        ops.call = lambda name, *a: (self.names.append(name), self.real(name, *a))[1]
        return self.names

    def __exit__(self, *exc):
        self.ops.call = self.real


def run_eval_case(case):
    """-> {'calls': [first, second, uint8], 'sha256': [...]}"""
    from recipe import synthetic_adj, synthetic_clips
    kind, prec, size = case.split("/")
    B, S, H, W, seed = SIZES[size]
    m, _ = model(kind)
    reset(kind)
    m.eval()
    m.hip_precision = prec
    x, adj = synthetic_clips(B, S, H=H, W=W, seed=seed).to(DEV), synthetic_adj(B, S, seed=seed).to(DEV)
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (B, S, H, W, 3), dtype=torch.uint8, generator=g).to(DEV)
    graph = kind in ("vmgn", "gsta", "ganet")
    calls, hashes = [], []
    for frames in (x, x, u8):
        with traced() as names:
            out = m(frames, adj) if graph else m(frames)
            torch.cuda.synchronize()
        calls.append(list(names))
        hashes.append(sha(out))
    m.invalidate_hip_cache()
    return {"calls": calls, "sha256": hashes}


def run_train_case(case):
    """-> {'calls': forward + backward, 'sha256': {loss, three gradients}, 'np_next', 'torch_next'}"""
    from recipe import synthetic_adj, synthetic_clips
    from torchreid import losses
    kind, prec = case.split("/")
    m, _ = model(kind)
    reset(kind)
    m.train()
    m.hip_train_precision = prec
    pids = torch.tensor([0, 1]).to(DEV)
    x = synthetic_clips(2, 5, H=64, W=32, seed=3, identities=[0, 1]).to(DEV)
    adj = synthetic_adj(2, 5, seed=3).to(DEV)
    ce = losses.CrossEntropyLabelSmooth(num_classes=KW["num_classes"], use_gpu=True)
    htri = losses.TripletLoss(margin=0.3)
    with traced() as names:
        torch.manual_seed(11)
        np.random.seed(77)
        outs, feats = m(x, adj)
        loss = losses.DeepSupervision(ce, outs, pids) + losses.DeepSupervision(htri, feats, pids)
        loss.backward()
        torch.cuda.synchronize()
    keys = [k for k, _ in m.named_parameters()]
    picked = ["conv1.weight", [k for k in keys if k.endswith("conv3.weight")][-1], [k for k in keys if k.endswith("classifier.weight")][-1]]
    params = dict(m.named_parameters())
    rec = {"calls": list(names), "sha256": dict({"loss": sha(loss)}, **{k: sha(params[k].grad) for k in picked}),
           "np_next": int(np.random.randint(1 << 30)), "torch_next": int(torch.randint(1 << 30, (1,)))}
    m.eval()
    m.hip_train_precision = "fp32"
    reset(kind)
    return rec


def first_difference(got, want):
    """None when the two entry-point lists are equal, else 'position i: got A, recorded B'"""
    for i in range(max(len(got), len(want))):
        a, b = (got[i] if i < len(got) else "<end>"), (want[i] if i < len(want) else "<end>")
        if a != b:
            return "position %d of %d / %d: got %s, recorded %s" % (i, len(got), len(want), a, b)
    return None


def encode(record):
    """entry-point names -> indices into one table (the lists are long and repeat ~120 names)"""
    table = {}

    def enc(names):
        return [table.setdefault(n, len(table)) for n in names]
    out = {"lp_name": record["lp_name"], "eval": {}, "train": {}}
    for case, r in record["eval"].items():
        out["eval"][case] = dict(r, calls=[enc(c) for c in r["calls"]])
    for case, r in record["train"].items():
        out["train"][case] = dict(r, calls=enc(r["calls"]))
    out["names"] = sorted(table, key=table.get)
    return out


def decode(stored):
    names = stored["names"]
    out = {"lp_name": stored["lp_name"], "eval": {}, "train": {}}
    for case, r in stored["eval"].items():
        out["eval"][case] = dict(r, calls=[[names[i] for i in c] for c in r["calls"]])
    for case, r in stored["train"].items():
        out["train"][case] = dict(r, calls=[names[i] for i in r["calls"]])
    return out


def load(path):
    with open(path) as f:
        return decode(json.load(f))


def merge(a, b):
    """two runs of one tree -> one record; a hash the two runs disagree on becomes None"""
    unstable = []
    for group in ("eval", "train"):
        assert sorted(a[group]) == sorted(b[group])
        for case, ra in a[group].items():
            rb = b[group][case]
            for ca, cb in zip(*([ra["calls"], rb["calls"]] if group == "eval" else [[ra["calls"]], [rb["calls"]]])):
                diff = first_difference(ca, cb)
                assert diff is None, "%s: the entry points differ between two runs of one tree: %s" % (case, diff)
            if group == "eval":
                for i, (ha, hb) in enumerate(zip(ra["sha256"], rb["sha256"])):
                    if ha != hb:
                        ra["sha256"][i] = None
                        unstable.append("%s forward %d" % (case, i))
            else:
                for k in ra["sha256"]:
                    if ra["sha256"][k] != rb["sha256"][k]:
                        ra["sha256"][k] = None
                        unstable.append("%s %s" % (case, k))
                assert (ra["np_next"], ra["torch_next"]) == (rb["np_next"], rb["torch_next"]), case
    return a, unstable


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "host_routes.json"))
    ap.add_argument("--merge", nargs=3, metavar=("A", "B", "OUT"))
    args = ap.parse_args()
    if args.merge:
        rec, unstable = merge(load(args.merge[0]), load(args.merge[1]))
        for name in unstable:
            print("not bit-reproducible, hash left out: " + name)
        out = args.merge[2]
    else:
        if not torch.cuda.is_available():
            sys.exit("record_host_routes: no GPU -- the routes are recorded on the device")
        from torchreid import hip_ops as ops
        rec = {"lp_name": ops.LP_NAME, "eval": {}, "train": {}}
        for case in eval_cases():
            rec["eval"][case] = run_eval_case(case)
            print(case, [len(c) for c in rec["eval"][case]["calls"]], flush=True)
        for case in train_cases():
            rec["train"][case] = run_train_case(case)
            print(case, len(rec["train"][case]["calls"]), flush=True)
        out = args.out
    with open(out, "w") as f:
        json.dump(encode(rec), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote %s (%d eval cases, %d train cases)" % (out, len(rec["eval"]), len(rec["train"])))


if __name__ == "__main__":
    main()
