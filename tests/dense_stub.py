"""A stand-in model and ragged dense loaders for the tests of the packed evaluation route (tests/test_dense_packed.py on the CPU,
tests/test_gpu_dense_packed.py on the GPU). The stub's output row is an ELEMENTWISE function of its own clip -- a slice of the clip's
pixels cast to float plus a slice of its adjacency -- so it is batch-invariant by construction: whatever batch a clip is embedded in,
its row has the same bits, and the packed route must then equal the per-tracklet route with torch.equal. What is left to go wrong is
the bookkeeping: which clip went where, in which order, pooled with which others."""
import numpy as np
import torch

S, H, W, V = 2, 8, 4, 6
CLIPS = (1, 2, 3, 5, 9, 1, 8, 2, 17, 1, 4)       # clips per tracklet: straddles 4 and 8, exceeds them, ends in a partial buffer
CLIPS_PAIRED = (2, 2, 3, 3, 3, 1, 1, 5, 4, 4)    # neighbours that share n: items with b = 2
POISON = 255                                      # a clip whose first pixel has this value embeds to inf (pixels are drawn below 200)
PIX, ADJ = 40, 8                                  # D = PIX + ADJ


class StubModel(torch.nn.Module):
    def __init__(self, poison=False):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))   # what extract_features reads the device from
        self.poison = poison
        self.calls = []                                    # clips per call, and (keep_inputs) what each call was given
        self.keep_inputs = False
        self.inputs = []

    def forward(self, imgs, adj):
        B = imgs.shape[0]
        self.calls.append(B)
        if self.keep_inputs:
            self.inputs.append((imgs.clone(), adj.clone()))
        pix = imgs.reshape(B, -1)
        out = torch.cat([pix[:, :PIX].float() * 0.25 - 3.0, adj.reshape(B, -1)[:, :ADJ].float()], 1)
        if self.poison:
            out = torch.where(pix[:, :1].float() == float(POISON), torch.full_like(out, float("inf")), out)
        return out


def tracklets(counts, seed, dtype=torch.uint8, layout="nchw", poison_clip=None):
    """-> list of one-tracklet items (imgs (1,n,S,3,H,W) | (1,n,S,H,W,3), pids (1,), camids (1,), adj (1,n,V,V)). Pixel values are
    integers below 200 in either dtype (exact in fp32); ``poison_clip``: the index, among all clips, of the one marked POISON."""
    g = torch.Generator().manual_seed(seed)
    items, k = [], 0
    for i, n in enumerate(counts):
        shape = (1, n, S, 3, H, W) if layout == "nchw" else (1, n, S, H, W, 3)
        x = torch.randint(0, 200, shape, generator=g, dtype=torch.uint8)
        if poison_clip is not None and k <= poison_clip < k + n:
            x[0, poison_clip - k].view(-1)[0] = POISON
        adj = torch.randint(0, 2, (1, n, V, V), generator=g).float() + torch.rand((1, n, V, V), generator=g)
        items.append((x.to(dtype), torch.tensor([100 + i]), torch.tensor([i % 3]), adj))
        k += n
    return items


def grouped(items, five_d=False):
    """loader items as a real loader would batch them: neighbours with the same n share an item (b = 2, never more); with ``five_d``
    single-clip tracklets come as 5-D items (b,S,...) with adj (b,V,V), the 'evenly' shape."""
    out, i = [], 0
    while i < len(items):
        group = [items[i]]
        if i + 1 < len(items) and items[i + 1][0].shape[1] == items[i][0].shape[1]:
            group.append(items[i + 1])
        i += len(group)
        x, p, c, a = group[0] if len(group) == 1 else (torch.cat([it[j] for it in group], 0) for j in range(4))   # (one: as it is, pinned or not)
        if five_d and x.shape[1] == 1:
            x, a = x[:, 0], a[:, 0]
        out.append((x, p, c, a))
    return out


def to_device(items, device):
    return [(x.to(device), p, c, a.to(device)) for x, p, c, a in items]


def expected_calls(counts, clip_batch):
    total = int(np.sum(counts))
    return [clip_batch] * (total // clip_batch) + ([total % clip_batch] if total % clip_batch else [])
