"""Generates tests/golden/{sta,simple_sta,res50tp}_b2s4.npz by running the REFERENCE implementation (weleen/AGRL.pytorch, mounted
read-only in the build container). Run:  python tests/golden/make_sta_golden.py

The reference's model files are imported by file path, nothing in them is modified and no reference source is copied into this
repository. Two harness-side shims: a stub ``torchvision`` module (sta.py and simple_sta.py import it without using it), and
``init_pretrained_weights`` replaced by a no-op (it would download ImageNet weights). Only arrays and key names are written: weights
and clips come from seeds (tests/sta_ref.py: sta_state_dict, sta_clips).

Frame selection is only testable where it is not a coin toss: the generator walks clip seeds in order from SEED0 and takes the first
one for which every (tracklet, part) has a relative gap >= MIN_GAP between the best and the second-best temporal attention, in that
model's own score; the seed and the gaps are stored in the fixture."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("AGRL_REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)  # the reference's (empty-__init__) torchreid package; this build's package is NOT on the path

import sta_ref  # noqa: E402

SEED0, MAX_SEEDS, MIN_GAP = 0, 64, 1e-3
WEIGHT_SEED, TRAIN_SEED_OFFSET = 0, 1000
KW = dict(num_classes=5, loss={"xent", "htri"}, last_stride=1, num_parts=3, num_scale=1, num_split=4, pyramid_part=True, num_gb=2,
          use_pose=True, learn_graph=True, consistent_loss=False, bnneck=True)


def load(name, rel):
    if "torchvision" not in sys.modules:
        sys.modules["torchvision"] = types.ModuleType("torchvision")
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    mod.init_pretrained_weights = lambda *a, **k: None
    return mod


def run(model, x, tail_module):
    """eval forward with the input of the tail's first module (fc1 / bottleneck) captured -> (out, pre-tail feature)"""
    seen = []
    handle = getattr(model, tail_module).register_forward_pre_hook(lambda m, inp: seen.append(inp[0].detach().clone()))
    with torch.no_grad():
        out = model(x, None)
    handle.remove()
    return out, seen[0]


def scores_of(kind, model, x):
    """The model's own (B,S,4) temporal attention, restated on the reference's layer-4 map in float64."""
    B, S = x.shape[:2]
    with torch.no_grad():
        fm = (model.featuremaps if kind != "res50tp" else model._extract_feat)(x.view((B * S,) + tuple(x.shape[2:])))
    sd = {k: v for k, v in model.state_dict().items()}
    return sta_ref.tail_ref(kind, fm, B, S, sd)


def main():
    torch.set_num_threads(8)
    for kind, rel, factory in (("res50tp", "torchreid/models/res50tp.py", "res50tp"),
                               ("simple_sta", "torchreid/models/simple_sta.py", "simple_sta_p4"),
                               ("sta", "torchreid/models/sta.py", "sta_p4")):
        mod = load("ref_" + kind, rel)
        model = getattr(mod, factory)(**KW)
        keys = sorted(model.state_dict().keys())
        shapes = [str(tuple(model.state_dict()[k].shape)) for k in keys]
        sd = sta_ref.sta_state_dict(model.state_dict(), WEIGHT_SEED)
        model.load_state_dict(sd)
        model.eval()
        B, S = 2, 4
        # ---- the first clip seed whose frame selection is decided by >= MIN_GAP in this model's own score
        for seed in range(SEED0, SEED0 + MAX_SEEDS):
            x = sta_ref.sta_clips(B, S, seed)
            r = scores_of(kind, model, x)
            gaps = sta_ref.relative_gaps(r["t_a"])
            print("%-10s seed %d: min relative gap %.3e" % (kind, seed, float(gaps.min())))
            if kind == "res50tp" or float(gaps.min()) >= MIN_GAP:
                break
        else:
            raise SystemExit("no seed with a gap >= %g among %d" % (MIN_GAP, MAX_SEEDS))
        arrays = {"keys": np.array(keys), "shapes": np.array(shapes), "seed": np.array(seed), "gaps": gaps.numpy(),
                  "meta": np.array([B, S, seed, WEIGHT_SEED, TRAIN_SEED_OFFSET])}
        if kind != "res50tp":
            # ---- calibrate fc1.1 on the fixture batch: one scalar mean / variance of the pre-BN values
            seen = []
            handle = model.fc1[1].register_forward_pre_hook(lambda m, inp: seen.append(inp[0].detach().clone()))
            with torch.no_grad():
                model(x, None)
            handle.remove()
            calib = (float(seen[0].double().mean()), float(seen[0].double().var(unbiased=False)))
            sd = sta_ref.sta_state_dict(model.state_dict(), WEIGHT_SEED, calib=calib)
            model.load_state_dict(sd)
            arrays.update(fc1_mean=np.float64(calib[0]), fc1_var=np.float64(calib[1]), pre_std=np.float64(seen[0].std()))
        out, feat = run(model, x, "bottleneck" if kind == "res50tp" else "fc1")
        r = scores_of(kind, model, x)
        arrays.update(out=out.numpy(), t_a=r["t_a"].float().numpy())
        if kind == "res50tp":
            arrays.update(f=feat.numpy())
        else:
            arrays.update(f_g=feat.numpy(), idx=r["idx"].to(torch.int32).numpy())
            assert float((r["f_g"] - feat.double()).abs().max() / feat.double().abs().max()) < 1e-5   # the restatement IS the reference's tail
        assert float((r["out"] - out.double()).abs().max() / out.double().abs().max()) < 1e-5
        # ---- train-mode outputs at (2, 8)
        model.train()
        xt = sta_ref.sta_clips(2, 8, seed + TRAIN_SEED_OFFSET)
        y, f = model(xt, None)
        arrays.update(train_logits=y.detach().numpy(), train_feats=f.detach().numpy())
        path = os.path.join(HERE, kind + "_b2s4.npz")
        np.savez_compressed(path, **arrays)
        print("wrote %-24s %7.1f KB (seed %d, out abs-max %.3f, non-zero %.2f)" % (
            os.path.basename(path), os.path.getsize(path) / 1024, seed, float(out.abs().max()), float((out != 0).float().mean())))


if __name__ == "__main__":
    main()
