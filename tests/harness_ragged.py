"""The split of tests/harness_split.py with RAGGED tracklets, for the dense test protocol as it really is: the number of clips differs
from tracklet to tracklet. Labels are ``harness_split.make_split()``'s; tracklet i has ``CLIP_CYCLE[i % 4]`` clips of S frames, and one
gallery tracklet (``LONG_AT``) has 9 -- longer than the 8-clip model batches the packed route is tested with. The reference driver's own
``test()`` ran on these loaders (tests/golden/make_dense_ragged_harness.py -> tests/golden/test_harness_ragged.npz); both sides
rebuild the inputs from the seeds."""
import numpy as np
import torch

from harness_split import N_ID, S, _idents, make_split  # noqa: F401
from recipe import synthetic_adj, synthetic_clips

CLIP_CYCLE = (1, 2, 3, 5)
LONG_AT, LONG_CLIPS = 6, 9
Q_SEED, G_SEED = 1300, 1700     # (G_SEED: the first one tried; the generator refuses a split with more than 2 near-tied queries)


def clip_counts(num, long_at=None):
    counts = [CLIP_CYCLE[i % len(CLIP_CYCLE)] for i in range(num)]
    if long_at is not None:
        counts[long_at] = LONG_CLIPS
    return counts


def dense_loader(pids, cams, seed, long_at=None):
    """the 'dense' test sampler at --test-batch 1: ONE tracklet per item, (imgs (1,n,S,3,256,128), pids (1,), camids (1,),
    adj (1,n,V,V)), n = this tracklet's clip count"""
    idents = _idents(pids)
    for i, n in enumerate(clip_counts(len(pids), long_at)):
        x = synthetic_clips(n, S, seed=seed + 31 * i, identities=[idents[i]] * n)
        adj = synthetic_adj(n, S, seed=seed + 31 * i)
        yield x.unsqueeze(0), torch.from_numpy(pids[i:i + 1]), torch.from_numpy(cams[i:i + 1]), adj.unsqueeze(0)


def loaders():
    """-> (query loader, gallery loader), fresh generators"""
    q_pids, q_cams, g_pids, g_cams = make_split()
    return dense_loader(q_pids, q_cams, Q_SEED), dense_loader(g_pids, g_cams, G_SEED, LONG_AT)
