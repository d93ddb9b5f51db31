"""Generates tests/golden/random_erasing.npz by running the REFERENCE's random erasing (weleen/AGRL.pytorch, mounted read-only in the
build container; root taken from AGRL_REFERENCE_ROOT). Run:  python tests/golden/make_random_erasing_golden.py

The reference's torchreid/transforms.py is loaded by file path (``make_golden.load``); nothing in it is modified and none of its source
is copied into this repository. Its module-level ``from torchvision.transforms import *`` and the bases of its Group classes need seven
torchvision names: empty stand-in classes are installed for them here (torchvision is not installed; none is ever called). Its other
imports (PIL, scipy.ndimage) are installed.

Per case, seeded uint8 frames (16, 3, H, W) are normalised with this build's ``hip_ops.frames_normalize_reference`` (ToTensor +
Normalize), and the reference erases copies of that tensor:

    group : random.seed(seed); GroupRandomErasing() -- the driver's call (train_vidreid_xent_htri.py:211) -- on the list of frames, each
            wrapped in the reference's ImageData
    single: random.seed(seed + 1); RandomErasing(probability=SINGLE_P, mean=SINGLE_MEAN), frame by frame

Written, per case ``HxW``: HxW.seed, HxW.frames (uint8), HxW.group and HxW.single (fp32 (16, 3, H, W)). The 256x128 case has 4 frames
and keeps neither the frames -- torch.randint under manual_seed(HxW.seed), as ``frames`` below -- nor the fp32 outputs: only the erased
masks (every channel holds its erase value), HxW.group_mask / HxW.single_mask = np.packbits of bool (4, 256, 128). Seeds, inputs and
outputs only."""
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (puts the reference's root on sys.path; this build's package is loaded by path below)

ROOT = make_golden.ROOT
SMALL = ((16, 8), (5, 7), (4, 6), (2, 2), (1, 9))
LARGE = (256, 128)
SINGLE_P = 0.75
SINGLE_MEAN = (0.4914, 0.4822, 0.4465)   # RandomErasing's own default
GROUP_MEAN = (0.485, 0.456, 0.406)       # GroupRandomErasing's default: what GroupRandomErasing() writes


def frames(seed, n, hw):
    return torch.randint(0, 256, (n, 3) + tuple(hw), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def reference_transforms():
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tvf = types.ModuleType("torchvision.transforms.functional")
    tv.transforms, tvt.functional = tvt, tvf
    for name in ("Compose", "ToTensor", "Normalize", "Resize", "RandomCrop", "RandomHorizontalFlip", "ToPILImage"):
        setattr(tvt, name, type(name, (object,), {}))
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})
    return make_golden.load("reference_transforms", os.path.join("torchreid", "transforms.py"))


def this_build_ops():
    sys.path[:] = [p for p in sys.path if p != make_golden.REF]
    sys.path.insert(0, os.path.join(ROOT, "agrl.pytorch_amd"))
    sys.modules.pop("torchreid", None)
    from torchreid import hip_ops
    return hip_ops


def main():
    T = reference_transforms()
    ops = this_build_ops()
    table = ops.frame_table()
    for c, (g, s) in enumerate(zip(GROUP_MEAN, SINGLE_MEAN)):   # a mask read back from the values needs them to be no table entry
        assert not (table[c] == np.float32(g)).any() and not (table[c] == np.float32(s)).any()
    arrays = {"sizes": np.array(SMALL + (LARGE,)), "single_probability": np.float64(SINGLE_P), "single_mean": np.array(SINGLE_MEAN),
              "group_mean": np.array(GROUP_MEAN)}
    for i, hw in enumerate(SMALL + (LARGE,)):
        name, seed, n = "%dx%d" % hw, 100 + 10 * i, 4 if hw == LARGE else 16
        u8 = frames(seed, n, hw)
        norm = ops.frames_normalize_reference(u8)
        random.seed(seed)
        group = T.GroupRandomErasing()([T.ImageData(f.clone()) for f in norm])
        group = torch.stack([g.img for g in group])
        random.seed(seed + 1)
        erase = T.RandomErasing(probability=SINGLE_P, mean=list(SINGLE_MEAN))
        single = torch.stack([erase(f.clone()) for f in norm])
        arrays[name + ".seed"] = np.int64(seed)
        if hw == LARGE:
            for key, out, mean in (("group", group, GROUP_MEAN), ("single", single, SINGLE_MEAN)):
                fill = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
                mask = (out == fill).all(1)
                assert torch.equal(out, torch.where(mask.unsqueeze(1), fill.expand_as(out), norm))
                arrays[name + "." + key + "_mask"] = np.packbits(mask.numpy())
                print("%s %-6s erased share per frame: %s" % (name, key, [round(float(m.float().mean()), 3) for m in mask]))
        else:
            arrays.update({name + ".frames": u8.numpy(), name + ".group": group.numpy(), name + ".single": single.numpy()})
    path = os.path.join(HERE, "random_erasing.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
