"""agrl_re_ranking (csrc/rerank.hip, behind --re-rank) on the GPU against tests/rerank_ref.py: every output element against the float64
value of the procedure on the fp32 D the kernel must reproduce bit for bit, inside the bound derived in rerank_ref's docstring (expf
taken at its documented 1 ulp: assumed, not measured), under poisoned allocations (output and workspace are ``torch.empty``) and run
twice for bit-equal results. Per case: lambda = 0.3 on the bound; lambda = 1 bit-equal to numpy's D[:m, m:]; lambda = 0 with the
``== 1.0`` mask equal to the pairs without shared support (set membership, free of rounding) and the rest on the bound; the first 20
columns of the induced ranking differ from the exact ranking only inside near-ties. Then ldf > n, every AGRL_CHECK_ARG of the entry
point (nothing written before a rejection), and the drop-in torchreid.utils.re_ranking beyond the kernel's limits.

The cases (rerank_ref.CASES) reach: half-to-even at k1 = 5, 9, 13 on N = 256 (register top-k); k1 = 30 / k2 = 31 and k1 = 1; exact
duplicates with empty neighbour sets (4 samples with nu = 0) and the stable tie order; N = 33 with m = 1; m > n; N = 1088 (two key
vectors per thread in the top-k, row index k up to 4 in rr_jaccard); N = 671 (radix top-k, unaligned rows). The largest set is nu = 62,
the longest query row nnz = 110 (k1 = 30): the summation branches for nu > 128 of rr_kreciprocal_kernel remain unexercised.

Measured on an MI355X (profiles/rerank_bounds.txt; the fp16 and the bf16 library give identical figures, these kernels are fp32 on both):
worst |got - exact| / bound at lambda = 0.3: 0.15 on the cases with k2 <= 3 and at the limits of k1 (the fixed six-rounding tail of jac
and the blend dominates), 0.18 at N = 1088 with k2 = 1, 0.23-0.28 at k1 = 20, k2 = 6 (N = 256 with m > n, 671, 1088); at lambda = 0:
0.03-0.15. Every case: lambda = 1 bit-equal to numpy's D, the ``== 1.0`` mask equal to the pairs without shared support, the two runs
bit-equal, no ranking position outside a near-tie. The oracle's own fp32 output gives the same ratios to two digits
(tests/test_rerank_ref.py), so the kernel's chain is no longer than numpy's.

Tried on deliberately wrong builds of the library (a scratch copy): half rounded half-up fails the six odd-k1 cases and nothing else;
k2 - 1 rows in the mean fails all 20 cases with k2 > 1; ties towards the higher index in the register top-k fails the two k2 = 1
duplicates cases (and the MARS tie tests); ldf ignored in rr_jaccard fails the leading-dimension test; the parent's drop-in fails both
drop-in cases with the kernel's HipKernelError. The rejection tests were not run against a build without its checks: such a build
would launch with the very arguments the checks guard against."""
import numpy as np
import pytest
import torch

import rerank_ref as R
from bounds import check_rounded, log_record, poisoned_outputs
from oracle import vmgn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


def on_dev(arrays):
    """the shared (read-only) numpy inputs as fresh device tensors"""
    return tuple(torch.from_numpy(a.copy()).to(DEV) for a in arrays)


def ops_():
    from torchreid import hip_ops as ops
    return ops


def twice(fn):
    """fn() under poisoned allocations, twice: the output of the first run, after asserting the second gave the same bits."""
    with poisoned_outputs():
        a = fn()
    with poisoned_outputs():
        b = fn()
    torch.cuda.synchronize()
    assert torch.equal(a, b), "two runs differ"
    return a


@pytest.mark.parametrize("case", R.GRID, ids=["%s-%s-k%d_%d" % c for c in R.GRID])
def test_re_ranking_elementwise(case):
    ops = ops_()
    name, metric, k1, k2 = case
    ref = R.reference(name, metric, k1, k2)
    m = ref.m
    q_g, q_q, g_g = on_dev(R.world(name, metric))
    tag = "re_ranking %s %s k1=%d k2=%d " % case
    worst = {}
    for lam in (0.3, 0.0, 1.0):
        got = twice(lambda: ops.re_ranking(q_g, q_q, g_g, k1, k2, lam)).cpu()
        assert got.shape == (m, ref.n) and got.dtype == F32
        if lam == 1.0:
            assert torch.equal(got, torch.from_numpy(ref.D[:m, m:])), tag + "lambda 1: D is not bit-equal to numpy's"
            continue
        if lam == 0.0:
            mask = (got == 1.0).numpy()
            assert np.array_equal(mask, ref.no_overlap), tag + "lambda 0: %d pairs differ in shared support" % int((mask != ref.no_overlap).sum())
        exact, mag, n, slack = ref.bound(lam)
        worst[lam] = check_rounded(got, exact, mag, n, F32, slack=slack, name=tag + "lambda %.1f" % lam)[0]
        outside, differ = R.ranking_outside_near_ties(got.numpy(), ref, lam)
        assert outside == 0, tag + "lambda %.1f: %d of %d differing ranking positions lie outside a near-tie" % (lam, outside, differ)
    d = ref.disc
    print(tag + "worst err / bound: lambda 0.3 %.3f, lambda 0 %.3f; nu max %d, nnz max %d" % (worst[0.3], worst[0.0], d.nu.max(), d.nnz.max()))
    log_record({"name": tag + "sets", "nu_max": int(d.nu.max()), "nu_zero": int((d.nu == 0).sum()), "nnz_max": int(d.nnz.max()),
                "lambda1_bit_equal": True, "lambda0_mask_equal": True, "two_runs_bit_equal": True})


def raw_call(q_g, q_q, g_g, m, n, k1, k2, lam, out, ldf, ws, ws_bytes):
    from torchreid import _hip
    _hip.call("agrl_re_ranking", q_g.data_ptr(), q_q.data_ptr(), g_g.data_ptr(), m, n, k1, k2, float(lam), out.data_ptr(), ldf,
              ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)


def workspace_bytes(m, n, k1):
    from torchreid import _hip
    return int(_hip.lib().agrl_re_ranking_workspace(m, n, k1))


@pytest.mark.parametrize("name", ["ragged", "m_gt_n"])
def test_re_ranking_leading_dimension(name):
    """ldf = n + 5: columns n.. of the caller's buffer stay untouched, columns :n are the contiguous call's bits."""
    ops = ops_()
    k1, k2 = R.CASES[name]["settings"][0]
    q_g, q_q, g_g = on_dev(R.world(name, "euclidean"))
    m, n = q_g.shape
    dense = ops.re_ranking(q_g, q_q, g_g, k1, k2, 0.3)
    out = torch.full((m, n + 5), -7.0, dtype=F32, device=DEV)
    nbytes = workspace_bytes(m, n, k1)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
    raw_call(q_g, q_q, g_g, m, n, k1, k2, 0.3, out, n + 5, ws, nbytes)
    torch.cuda.synchronize()
    assert bool((out[:, n:] == -7.0).all()), "wrote past column n"
    assert torch.equal(out[:, :n], dense)


REJECTIONS = [   # name, (m, n, k1, k2, ldf - n, workspace shortfall), message
    ("k1=0", (4, 12, 0, 1, 0, 0), "1 <= k1 <= 30"),
    ("k1=31", (4, 40, 31, 6, 0, 0), "1 <= k1 <= 30"),
    ("k1+1>m+n", (4, 12, 16, 6, 0, 0), "k1 < m \\+ n"),
    ("k2=0", (4, 12, 8, 0, 0, 0), "1 <= k2 <= k1 \\+ 1"),
    ("k2=k1+2", (4, 12, 8, 10, 0, 0), "1 <= k2 <= k1 \\+ 1"),
    ("ldf<n", (4, 12, 8, 3, -1, 0), "bad shape"),
    ("m+n=16385", (1, 16384, 20, 6, 0, 0), "exceeds 16384"),
    ("workspace-1", (4, 12, 8, 3, 0, 1), "workspace too small"),
]


@pytest.mark.parametrize("rej", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_re_ranking_rejections_write_nothing(rej):
    """Every AGRL_CHECK_ARG of the entry point raises HipKernelError with its message BEFORE any launch: the sentinel-filled output and
    workspace are unchanged. m + n = 16385 is called with small buffers -- the check precedes every launch, nothing reads them."""
    from torchreid import _hip
    _, (m, n, k1, k2, dld, short), message = rej
    small = m + n > 16384
    g = torch.Generator().manual_seed(3)
    bm, bn = (4, 12) if small else (m, n)         # what the buffers really hold
    q_g, q_q, g_g = (torch.rand(s, generator=g).to(DEV) for s in ((bm, bn), (bm, bm), (bn, bn)))
    out = torch.full((bm, bn), -7.0, dtype=F32, device=DEV)
    nbytes = workspace_bytes(bm, bn, max(1, min(k1, 30)))
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
    claimed = workspace_bytes(m, n, max(k1, 0)) if small else nbytes - short
    with pytest.raises(_hip.HipKernelError, match=message):
        raw_call(q_g, q_q, g_g, m, n, k1, k2, 0.3, out, n + dld, ws, claimed)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ws == 0x5A).all()), "a rejected call wrote"
    with pytest.raises(_hip.HipKernelError, match="null pointer"):
        _hip.call("agrl_re_ranking", q_g.data_ptr(), q_q.data_ptr(), g_g.data_ptr(), bm, bn, 8, 3, 0.3, None, bn, ws.data_ptr(), nbytes,
                  torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("k1k2", [(40, 6), (8, 12)])
def test_drop_in_accepts_what_the_reference_accepts(k1k2):
    """torchreid.utils.re_ranking.re_ranking beyond the kernel's limits (k1 > 30; k2 > k1 + 1) on a GPU host: the reference takes any
    k1 and k2, so does the drop-in (host evaluation), numpy in -> float32 numpy out, CUDA in -> CUDA out; ops.re_ranking stays strict."""
    from torchreid import _hip
    from torchreid.utils.re_ranking import re_ranking
    k1, k2 = k1k2
    q_g, q_q, g_g = (a.copy() for a in R.world("odd_k1", "cosine"))
    ref = O.re_ranking(q_g, q_q, g_g, k1=k1, k2=k2)
    got = re_ranking(q_g, q_q, g_g, k1=k1, k2=k2)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == q_g.shape
    assert np.abs(got - ref).max() < 2e-6
    dev = re_ranking(*on_dev((q_g, q_q, g_g)), k1=k1, k2=k2)
    assert dev.is_cuda and dev.dtype == F32 and np.abs(dev.cpu().numpy() - ref).max() < 2e-6
    with pytest.raises(_hip.HipKernelError, match="k1 <= 30" if k1 > 30 else "k2 <= k1"):
        ops_().re_ranking(*on_dev((q_g, q_q, g_g)), k1=k1, k2=k2)
    # inside the limits the drop-in is the kernel: the same bits as ops.re_ranking
    inside = re_ranking(q_g, q_q, g_g, k1=9, k2=3)
    assert np.array_equal(inside, ops_().re_ranking(*on_dev((q_g, q_q, g_g)), k1=9, k2=3).cpu().numpy())
