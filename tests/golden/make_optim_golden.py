"""Generates tests/golden/optim_extra.npz by running the REFERENCE's optimisers (weleen/AGRL.pytorch, mounted read-only in the build
container; root taken from AGRL_REFERENCE_ROOT). Run:  python tests/golden/make_optim_golden.py

The reference's torchreid/optimizers.py is loaded by file path (it imports only torch and math); nothing in it is modified and none
of its source is copied into this repository. Four variants -- the reference's AdaBound, AdaBound(amsbound=True) and RAdam, and
torch.optim.RMSprop(momentum=0.9) as the reference's init_optim builds it -- each step ONE parameter group of three fp32 tensors
(5, 64 and 130 elements) eight times on the CPU at lr 3e-4, weight decay 5e-4. Parameters and gradients are seeded, span several
decades and include zeros. Only arrays and names are written, per variant ``V``:

    V/p0 (199)  V/g (8,199)  V/p (8,199)  V/<state key> (8,199) for every tensor of the state  V/step (8,3)
    V/state_keys  V/group_keys  V/step_type ("int" | "tensor:<dtype>")  V/hyper: the group's scalar values, in group_keys order
    (a pair such as betas takes two entries; ``params`` is left out)

the three tensors concatenated in order; ``sizes`` holds their lengths."""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("AGRL_REFERENCE_ROOT", "/root/reference")
SIZES, STEPS, LR, WD, SEED = (5, 64, 130), 8, 3e-4, 5e-4, 20


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_optimizers", os.path.join(REF, "torchreid", "optimizers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def decades(n, gen, lo, hi, zero_share):
    x = torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * (hi - lo) + lo)
    x[torch.rand(n, generator=gen) < zero_share] = 0.0
    return x


def main():
    ref = load_reference()
    variants = (("adabound", lambda ps: ref.init_optim("adabound", ps, LR, WD)),
                ("amsbound", lambda ps: ref.AdaBound(ps, lr=LR, final_lr=100 * LR, weight_decay=WD, amsbound=True)),
                ("radam", lambda ps: ref.init_optim("radam", ps, LR, WD)),
                ("rmsprop", lambda ps: ref.init_optim("rmsprop", ps, LR, WD)))
    arrays = {"sizes": np.array(SIZES), "variants": np.array([v for v, _ in variants])}
    for vi, (name, make) in enumerate(variants):
        gen = torch.Generator().manual_seed(SEED + vi)
        params = [torch.nn.Parameter(decades(n, gen, -3.0, 1.0, 0.05)) for n in SIZES]
        opt = make(params)
        arrays[name + "/p0"] = torch.cat([p.detach() for p in params]).numpy().copy()
        rec = {"g": [], "p": [], "step": []}
        for _ in range(STEPS):
            grads = [decades(n, gen, -8.0, 2.0, 0.08) for n in SIZES]
            for p, g in zip(params, grads):
                p.grad = g.clone()
            opt.step()
            rec["g"].append(torch.cat(grads).numpy().copy())
            rec["p"].append(torch.cat([p.detach() for p in params]).numpy().copy())
            rec["step"].append([float(opt.state[p]["step"]) for p in params])
            for key, value in opt.state[params[0]].items():
                if torch.is_tensor(value) and value.dim() > 0:
                    rec.setdefault(key, []).append(torch.cat([opt.state[p][key] for p in params]).numpy().copy())
        for key, rows in rec.items():
            arrays["%s/%s" % (name, key)] = np.stack(rows) if key != "step" else np.array(rows, dtype=np.float64)
        step = opt.state[params[0]]["step"]
        group = opt.param_groups[0]
        group_keys = [k for k in group if k != "params"]
        hyper = []
        for k in group_keys:
            v = group[k]
            hyper += [float("nan") if x is None else float(x) for x in (v if isinstance(v, (tuple, list)) else (v,))]
        arrays[name + "/state_keys"] = np.array(sorted(opt.state[params[0]].keys()))
        arrays[name + "/group_keys"] = np.array(group_keys)
        arrays[name + "/hyper"] = np.array(hyper, dtype=np.float64)
        arrays[name + "/step_type"] = np.array("tensor:%s" % str(step.dtype).replace("torch.", "") if torch.is_tensor(step) else type(step).__name__)
        print("%-9s state %s, step %r after %d steps, |p| max %.3e" % (name, list(arrays[name + "/state_keys"]), step, STEPS, float(np.abs(rec["p"][-1]).max())))
    path = os.path.join(HERE, "optim_extra.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s, %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
