"""Generates tests/golden/test_harness_ragged.npz: the REFERENCE DRIVER's own ``test()`` (train_vidreid_xent_htri.py:450-542, loaded
by make_test_harness.load_driver -- nothing of it is copied) with ``--test-sample dense --test-batch 1`` on the reference's ``vmgn``,
on the CPU, over the RAGGED loaders of tests/harness_ragged.py: tracklets of 1, 2, 3, 5 and 9 clips, pooled by the reference's
``features.view(n, 1, -1)`` mean (:471-476). Build container only:  python tests/golden/make_dense_ragged_harness.py

The model is the one of tests/golden/test_harness.npz: recipe weights and that file's BNNeck calibration. Written: per metric the
distance matrix, CMC, Rank-1 and mAP that test() / evaluate_rank return, and ``<metric>_dense_exempt``: how many of the 10 queries have
two of their 51 smallest reference distances closer than 4 x 1e-5 x max|distance| -- the queries whose top-50 index list the test cannot
hold a matrix at the 1e-5 bar to. More than 2 such queries and no fixture is written: change harness_ragged.G_SEED and record it there."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_test_harness as MT  # noqa: E402
import harness_ragged as HR  # noqa: E402
from recipe import recipe_state_dict  # noqa: E402

MAX_EXEMPT = 2


def main():
    torch.set_num_threads(8)
    drv, ref_vmgn = MT.load_driver(["--use-cpu", "--test-sample", "dense", "--seq-len", str(HR.S), "--test-batch", "1",
                                    "--dist-metric", "cosine", "-a", "vmgn"])
    z = np.load(os.path.join(HERE, "test_harness.npz"))
    q_pids, q_cams, g_pids, g_cams = HR.make_split()
    model = ref_vmgn.vmgn(num_classes=HR.N_ID, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1,
                          pyramid_part=True, use_pose=True, learn_graph=True, consistent_loss=False)
    sd = recipe_state_dict(model.state_dict(), seed=0)
    for name, mean, var in (("global_bottleneck", "g_mean", "g_var"), ("att_bottleneck", "a_mean", "a_var")):
        sd[name + ".running_mean"] = torch.from_numpy(z[mean])
        sd[name + ".running_var"] = torch.from_numpy(z[var])
        sd[name + ".weight"] = torch.ones_like(sd[name + ".weight"])
        sd[name + ".bias"] = torch.zeros_like(sd[name + ".bias"])
    model.load_state_dict(sd)
    model.eval()
    ql, gl = (list(it) for it in HR.loaders())
    out = {}
    for metric in ("cosine", "euclidean"):
        drv.args.dist_metric = metric
        drv.args.test_sample = "dense"
        drv.args.re_rank = False
        distmat = np.asarray(drv.test(model, ql, gl, "avg", False, return_distmat=True), dtype=np.float32)
        cmc, mAP = sys.modules["torchreid.metrics"].evaluate_rank(distmat, q_pids, g_pids, q_cams, g_cams, use_metric_mars=True)
        gaps = np.diff(np.sort(distmat.astype(np.float64), axis=1)[:, :51], axis=1).min(axis=1)
        exempt = int((gaps <= 4 * 1e-5 * np.abs(distmat).max()).sum())
        tag = "%s_dense" % metric
        print(tag, "Rank-1 %.4f mAP %.6f, smallest top-51 gap per query / max|d|: %s, exempt %d" % (
            cmc[0], mAP, np.array2string(gaps / np.abs(distmat).max(), precision=2), exempt))
        if exempt > MAX_EXEMPT:
            raise SystemExit("%s: %d of %d queries are near-tied at the 1e-5 bar (at most %d): change harness_ragged.G_SEED" % (
                tag, exempt, len(q_pids), MAX_EXEMPT))
        out[tag + "_rank1"] = np.float64(cmc[0])
        out[tag + "_mAP"] = np.float64(mAP)
        out[tag + "_cmc"] = np.asarray(cmc, dtype=np.float64)
        out[tag + "_distmat"] = distmat
        out[tag + "_exempt"] = np.int64(exempt)
    out.update(q_pids=q_pids, q_cams=q_cams, g_pids=g_pids, g_cams=g_cams, q_seed=np.int64(HR.Q_SEED), g_seed=np.int64(HR.G_SEED),
               q_clips=np.array(HR.clip_counts(len(q_pids)), dtype=np.int64),
               g_clips=np.array(HR.clip_counts(len(g_pids), HR.LONG_AT), dtype=np.int64))
    path = os.path.join(HERE, "test_harness_ragged.npz")
    np.savez_compressed(path, **out)
    print("wrote test_harness_ragged.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
