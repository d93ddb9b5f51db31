"""Generates tests/golden/clip_indices.npz from the REFERENCE's own ``VideoDataset`` (torchreid/dataset_loader.py:58-215 of
weleen/AGRL.pytorch, mounted read-only at /root/reference). Build container only:  python tests/golden/make_clip_indices_golden.py

``VideoDataset.__getitem__`` never returns the frame indices it draws, only the frames. So the frames carry them: tracklet frame i
is a tiny image file whose every pixel has the value i, a transform turns what the dataset read into tensors, and the index list
is read back from the pixels of what ``__getitem__`` returns. The module is loaded by file path (make_golden.load) with
``torchvision.transforms.functional`` and ``torchreid.transforms`` stubbed (make_golden.install_shims; ``ImageData`` here is a
holder with an ``img`` attribute, which is all the dataset uses of it). Only index arrays are stored:

    for every sampler in (evenly, all, dense, skipdense), seq_len S in (4, 8, 15), max_len in (7, 1000):
        "<sampler>_S<S>_M<max_len>_idx"  int64, the index lists of num = 1 .. 3 S + 1 frames, one after the other
        "<sampler>_S<S>_M<max_len>_len"  int64 (3 S + 1,), their lengths
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402

SAMPLERS = ("evenly", "all", "dense", "skipdense")
SEQ_LENS = (4, 8, 15)
MAX_LENS = (7, 1000)


class ImageData:
    def __init__(self, img):
        self.img = img


def to_tensors(items):
    for it in items:
        it.img = torch.from_numpy(np.asarray(it.img, dtype=np.uint8).copy()).permute(2, 0, 1)
    return items


def main():
    from PIL import Image
    MG.install_shims()
    sys.modules["torchreid.transforms"].ImageData = ImageData
    DL = MG.load("ref_dataset_loader", "torchreid/dataset_loader.py")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        longest = 3 * max(SEQ_LENS) + 1
        paths = []
        for i in range(longest):
            paths.append(os.path.join(tmp, "%03d.png" % i))
            Image.fromarray(np.full((2, 2, 3), i, dtype=np.uint8)).save(paths[-1])
        for sample in SAMPLERS:
            for S in SEQ_LENS:
                for max_len in MAX_LENS:
                    tracklets = [(tuple(paths[:num]), 0, 0) for num in range(1, 3 * S + 2)]
                    ds = DL.VideoDataset(tracklets, seq_len=S, sample=sample, transform=to_tensors, pose_info={}, num_split=4,
                                         num_scale=1, pyramid_part=True, enable_pose=False, max_len=max_len)
                    lists = []
                    for t in range(len(tracklets)):
                        imgs = ds[t][0]
                        frames = imgs.reshape(-1, 3, 2, 2)
                        assert bool((frames == frames[:, :1, :1, :1]).all())
                        lists.append(frames[:, 0, 0, 0].numpy().astype(np.int64))
                    tag = "%s_S%d_M%d" % (sample, S, max_len)
                    out[tag + "_idx"] = np.concatenate(lists)
                    out[tag + "_len"] = np.array([len(v) for v in lists], dtype=np.int64)
    path = os.path.join(HERE, "clip_indices.npz")
    np.savez_compressed(path, **out)
    print("wrote clip_indices.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
