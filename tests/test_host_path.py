"""The host path above the C-ABI as a structure (torchreid/models/_resnet_hip.py under the model files): what no GPU is needed for."""
import ast
import glob
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "agrl.pytorch_amd", "torchreid", "models")


def test_no_private_name_is_imported_across_the_model_files():
    """A name with a leading underscore belongs to its file: no file of torchreid/models/ imports one from another file of that
    package, by ``from .x import _name`` or ``from torchreid.models[.x] import _name`` (the shared backbone's names are public)."""
    found = []
    for path in sorted(glob.glob(os.path.join(MODELS, "*.py"))):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            if not isinstance(node, ast.ImportFrom):
                continue
            module = node.module or ""
            if node.level == 0 and module != "torchreid.models" and not module.startswith("torchreid.models."):
                continue   # not from this package
            found += ["%s:%d imports %s from %s%s" % (os.path.basename(path), node.lineno, a.name, "." * node.level, module)
                      for a in node.names if a.name.startswith("_")]
    assert len(glob.glob(os.path.join(MODELS, "*.py"))) >= 12 and not found, found


def test_drop_one_frame_draws_what_the_inline_loop_drew():
    """_train_hip.drop_one_frame, shared by the native steps and the module trees of gsta and ganet, against the loop it replaced: the
    same index tensor and the same state of numpy's global generator afterwards (B calls of np.random.randint(S), in order)."""
    from torchreid.models._train_hip import drop_one_frame
    B, S = 5, 7
    np.random.seed(77)
    keep = []
    for _ in range(B):
        idx = list(range(S))
        idx.remove(np.random.randint(S))
        keep.append(idx)
    want, want_next = torch.LongTensor(keep), np.random.randint(1 << 30)
    np.random.seed(77)
    got = drop_one_frame(B, S, torch.device("cpu"))
    assert got.dtype == torch.int64 and tuple(got.shape) == (B, S - 1) and torch.equal(got, want)
    assert np.random.randint(1 << 30) == want_next
