"""The STA tail kernels on the GPU (csrc/sta.hip): agrl_sta_frame_stats, agrl_sta_fuse and agrl_linear_bn_relu, every output element
against float64 of the contract in include/agrl_hip.h on the operands the kernel sees, with the chain lengths of tests/sta_ref.py
(derived in its docstring), under NaN-poisoned allocations, and run twice for bitwise repeatability. Frame selection is tested where
it is decided: scores built with a gap of at least 5 % between the best and the second-best frame, so ``idx`` must be exact in every
arithmetic; ties and the all-zero tracklet pin the first-maximum rule and the 1e-12 clamps.

Measured on an MI355X, worst |got - exact| / bound over the cases: frame_stats vmean 0.20, nsum 0.09, nsq 0.10; fuse t_a 0.16, the selected
half of f_g 0.75 (three additions: the tightest chain), the weighted half 0.48; linear_bn_relu 0.12 (0.01 at K = 4096), the GEMM route above
the M bound 0.01."""
import pytest
import torch

import sta_ref as SR
from bounds import check_rounded, n_acc_for, poisoned_outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


def ops_():
    from torchreid import hip_ops as ops
    return ops


def lp():
    return ops_().LP_DTYPE


def twice(fn):
    """fn() under poisoned allocations, twice: the outputs of the first run, after asserting the second gave the same bits."""
    with poisoned_outputs():
        a = fn()
    with poisoned_outputs():
        b = fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two runs differ"
    return a


def channel_scales(C, seed):
    """per-channel powers of two spanning 2^-8 .. 2^8: an error confined to the small channels shows in an elementwise bound"""
    g = torch.Generator().manual_seed(900 + seed)
    return torch.pow(2.0, torch.randint(-8, 9, (C,), generator=g).float())


# ---- agrl_sta_frame_stats ---------------------------------------------------------------------------------------------------
# 16 x 8 x 2048: the model's map | overlapping bins, odd width, C no multiple of the workgroup's channel span | minimal
FS_CASES = [(3, 16, 8, 2048), (2, 7, 3, 264), (1, 4, 1, 8)]


@pytest.mark.parametrize("dtype", ["lp16", "fp32"])
@pytest.mark.parametrize("case", FS_CASES, ids=["%dx%dx%dx%d" % c for c in FS_CASES])
def test_frame_stats(case, dtype):
    ops = ops_()
    F_, h, w, C = case
    g = torch.Generator().manual_seed(F_ + 3 * h + 5 * w + C)
    x = (torch.randn((F_, h, w, C), generator=g) * channel_scales(C, C)).to(lp() if dtype == "lp16" else F32).contiguous()
    vmean, nsum, nsq = twice(lambda: ops.sta_frame_stats(x.to(DEV)))
    r = SR.frame_stats_ref(x)
    name = "frame_stats %s %s " % (case, dtype)
    worst = [check_rounded(vmean, r["vmean"], r["vmean_mag"], r["vmean_n"], F32, name=name + "vmean")[0],
             check_rounded(nsum, r["nsum"], r["nsum"], r["nsum_n"], F32, name=name + "nsum")[0],
             check_rounded(nsq, r["nsq"], r["nsq"], r["nsq_n"], F32, name=name + "nsq")[0]]
    print(name, "worst err / bound: vmean %.3f nsum %.3f nsq %.3f" % tuple(worst))
    # every pixel once: the four nsq add up to the frame's sum of squares
    total = x.double().pow(2).sum(dim=(1, 2, 3))
    assert float(((nsq.cpu().double().sum(dim=1) - total).abs() / total).max()) < (r["nsq_n"] + 4) * 2.0 ** -24
    if h % 4 == 0:   # the semantics of agrl_part_pool with splits {4}
        _, nodes, _ = ops.part_pool(x.to(DEV), x.to(DEV), [4], want_lp=False)
        check_rounded(nodes, r["vmean"], r["vmean_mag"], r["vmean_n"], F32, name=name + "part_pool")


def test_frame_stats_rejects_what_it_cannot_read():
    from torchreid import _hip
    ops = ops_()
    out = [torch.zeros(64, device=DEV) for _ in range(3)]

    def raw(x, h, C):
        _hip.call("agrl_sta_frame_stats", x.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), 1, h, 2, C, _hip.F32,
                  torch.cuda.current_stream().cuda_stream)

    x = torch.zeros(4 * 2 * 16, device=DEV)
    with pytest.raises(_hip.HipKernelError, match="multiple of 8"):
        raw(x, 4, 12)
    with pytest.raises(_hip.HipKernelError, match="at least 4"):
        raw(x, 3, 8)
    with pytest.raises(_hip.HipKernelError, match="registers"):
        raw(x, 4, 4104)
    with pytest.raises(AssertionError):
        ops.sta_frame_stats(torch.zeros((1, 4, 2, 12), device=DEV))
    with pytest.raises(AssertionError):
        ops.sta_frame_stats(torch.zeros((1, 3, 2, 8), device=DEV))
    with pytest.raises(AssertionError):
        ops.sta_frame_stats(torch.zeros((1, 4, 2, 8), device=DEV, dtype=torch.float64))


# ---- agrl_sta_fuse ------------------------------------------------------------------------------------------------------------
FUSE_BS = [(3, 1), (2, 2), (2, 5), (1, 8)]


def fuse_operands(target, C, hw, g):
    """target (B,S,4) scores -> vmean rows of that norm, and nsum / nsq that give the same scores in the map mode"""
    B, S, _ = target.shape
    v = torch.randn((B, S, 4, C), generator=g) * channel_scales(C, S)
    v = v / v.norm(dim=3, keepdim=True) * target.unsqueeze(3)
    nsq = 0.5 + torch.rand((B, S, 4), generator=g)
    npix = torch.tensor([(r1 - r0) * hw[1] for r0, r1 in SR.bins(hw[0])], dtype=torch.float32)
    nsum = target * npix * nsq.sum(dim=2, keepdim=True).sqrt()
    return v, nsum, nsq


def fuse_problem(B, S, C, seed=0, edit=None):
    """Scores 1.12^k, k a permutation of the frames per part (a 12 % gap between neighbours), optionally edited, as cpu operands:
    vmean (B*S,4,C), nsum, nsq (B*S,4), (h, w)."""
    g = torch.Generator().manual_seed(31 * B + 7 * S + C + seed)
    target = torch.stack([torch.stack([1.12 ** torch.randperm(S, generator=g).float() for _ in range(4)], dim=1) for _ in range(B)])
    if edit is not None:
        edit(target)
    hw = (16, 8) if C == 2048 else (7, 3)
    v, nsum, nsq = fuse_operands(target, C, hw, g)
    return v, nsum, nsq, hw


def flat(v, nsum, nsq):
    B, S = v.shape[:2]
    return v.reshape(B * S, 4, -1).contiguous(), nsum.reshape(B * S, 4).contiguous(), nsq.reshape(B * S, 4).contiguous()


def run_fuse(v, nsum, nsq, hw, B, S, mode):
    ops = ops_()
    if mode == "map":
        return twice(lambda: ops.sta_fuse(v.to(DEV), B, S, nsum.to(DEV), nsq.to(DEV), hw))
    return twice(lambda: ops.sta_fuse(v.to(DEV), B, S))


def check_fuse(v, nsum, nsq, hw, B, S, mode, name, min_gap=0.05):
    C = v.shape[2]
    f_g, t_a, idx = run_fuse(v, nsum, nsq, hw, B, S, mode)
    scores = SR.scores_map(nsum, nsq, *hw) if mode == "map" else SR.scores_norm(v)
    exact, mag, ta, first = SR.fuse_ref(v, scores, B, S)
    if S > 1 and min_gap:
        assert float(SR.relative_gaps(ta).min()) >= min_gap, "the test's own scores are not decided"
    assert torch.equal(idx.cpu().long(), first), (name, idx.cpu(), first)
    n = SR.fuse_chains(S, C, mode)
    worst = [check_rounded(t_a, ta, ta.abs(), n["t_a"], F32, name=name + " t_a")[0],
             check_rounded(f_g[:, :C], exact[:, :C], mag[:, :C], n["f1"], F32, name=name + " f_g[:C]")[0]]
    own, own_mag, _, _ = SR.fuse_ref(v, scores, B, S, idx=idx, t_a=t_a)     # the weighted sum on the kernel's own t_a
    worst.append(check_rounded(f_g[:, C:], own[:, C:], own_mag[:, C:], n["f2"], F32, name=name + " f_g[C:]")[0])
    print(name, "worst err / bound: t_a %.3f f1 %.3f f2 %.3f" % tuple(worst))
    return f_g, t_a, idx


@pytest.mark.parametrize("mode", ["map", "norm"])
@pytest.mark.parametrize("C", [2048, 264])
@pytest.mark.parametrize("B,S", FUSE_BS)
def test_fuse(B, S, C, mode):
    v, nsum, nsq, hw = fuse_problem(B, S, C)
    v, nsum, nsq = flat(v, nsum, nsq)
    check_fuse(v, nsum, nsq, hw, B, S, mode, "fuse B%d S%d C%d %s" % (B, S, C, mode))


@pytest.mark.parametrize("mode", ["map", "norm"])
def test_fuse_takes_the_first_of_two_identical_frames(mode):
    B, S, C = 2, 5, 264

    def largest(target):   # tracklet 0: frame 1 the largest in every part
        target[0, 1] = 3.0

    v, nsum, nsq, hw = fuse_problem(B, S, C, seed=1, edit=largest)
    for t in (v, nsum, nsq):   # ... and copied into frame 3
        t[0, 3] = t[0, 1]
    v, nsum, nsq = flat(v, nsum, nsq)
    _, t_a, idx = check_fuse(v, nsum, nsq, hw, B, S, mode, "fuse tie " + mode, min_gap=0)
    assert idx[0].tolist() == [1, 1, 1, 1] and torch.equal(t_a[0, 1], t_a[0, 3])


@pytest.mark.parametrize("mode", ["map", "norm"])
def test_fuse_all_zero_tracklet(mode):
    B, S, C = 2, 5, 264
    v, nsum, nsq, hw = fuse_problem(B, S, C, seed=2)
    for t in (v, nsum, nsq):
        t[1] = 0
    v, nsum, nsq = flat(v, nsum, nsq)
    f_g, t_a, idx = run_fuse(v, nsum, nsq, hw, B, S, mode)
    assert torch.isfinite(f_g).all() and torch.isfinite(t_a).all()
    assert float(f_g[1].abs().max()) == 0.0 and float(t_a[1].abs().max()) == 0.0 and idx[1].tolist() == [0, 0, 0, 0]
    assert float(f_g[0].abs().max()) > 0.0


def test_fuse_rejects_bad_arguments():
    from torchreid import _hip
    ops = ops_()
    v = torch.zeros((2, 4, 8), device=DEV)
    o = [torch.zeros(64, device=DEV), torch.zeros(64, device=DEV), torch.zeros(64, device=DEV, dtype=torch.int32)]
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(_hip.HipKernelError, match="mode"):
        _hip.call("agrl_sta_fuse", v.data_ptr(), None, None, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), 1, 2, 8, 0, 0, 2, st)
    with pytest.raises(_hip.HipKernelError, match="nsum"):
        _hip.call("agrl_sta_fuse", v.data_ptr(), None, None, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), 1, 2, 8, 4, 1, 0, st)
    with pytest.raises(_hip.HipKernelError, match="multiple of 4"):
        _hip.call("agrl_sta_fuse", v.data_ptr(), None, None, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), 1, 2, 6, 0, 0, 1, st)
    with pytest.raises(AssertionError):
        ops.sta_fuse(v, 1, 3)


# ---- agrl_linear_bn_relu ------------------------------------------------------------------------------------------------------
LBR_CASES = [(1, 4096, 1024), (3, 4096, 1024), (32, 4096, 1024), (5, 64, 8), (33, 4096, 1024)]   # the last: one row above the M bound


def lbr_problem(M, K, N, dtype):
    g = torch.Generator().manual_seed(M + K + N)
    x = (torch.randn((M, K), generator=g) * channel_scales(K, 1)).contiguous()
    w = (torch.randn((N, K), generator=g) * 0.05).to(lp() if dtype == "lp16" else F32).contiguous()
    scale = (0.5 + torch.rand((N,), generator=g)) * torch.where(torch.rand((N,), generator=g) < 0.25, -1.0, 1.0)
    shift = 0.3 * torch.randn((N,), generator=g)
    return x, w, scale.contiguous(), shift.contiguous()


@pytest.mark.parametrize("dtype", ["lp16", "fp32"])
@pytest.mark.parametrize("case", LBR_CASES, ids=["%dx%dx%d" % c for c in LBR_CASES])
def test_linear_bn_relu(case, dtype):
    ops = ops_()
    M, K, N = case
    assert ops.LINEAR_BN_RELU_MAX_M == 32
    x, w, scale, shift = lbr_problem(M, K, N, dtype)
    (out,) = twice(lambda: (ops.linear_bn_relu(x.to(DEV), w.to(DEV), scale.to(DEV), shift.to(DEV)),))
    if M <= ops.LINEAR_BN_RELU_MAX_M:
        exact, mag, n = SR.linear_bn_relu_ref(x, w, scale, shift)
    else:   # the tiled GEMM on operands of the weight's type, the epilogue in torch
        exact, mag, _ = SR.linear_bn_relu_ref(x.to(w.dtype), w, scale, shift)
        n = n_acc_for(K, 4 if dtype == "fp32" else 16) + 2
    assert tuple(out.shape) == (M, N)
    worst = check_rounded(out, exact, mag, n, F32, name="linear_bn_relu %s %s" % (case, dtype))[0]
    frac = float((out == 0).float().mean())
    print("linear_bn_relu", case, dtype, "worst err / bound %.3f, zeros %.2f" % (worst, frac))
    assert 0.05 < frac < 0.95   # both sides of the ReLU are exercised


def test_linear_bn_relu_entry_point_rejects_rows_above_its_bound():
    from torchreid import _hip
    x, w, scale, shift = [t.to(DEV) for t in lbr_problem(33, 64, 8, "fp32")]
    out = torch.zeros((33, 8), device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(_hip.HipKernelError, match="above the 32 rows"):
        _hip.call("agrl_linear_bn_relu", x.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(), 33, 64, 8, _hip.F32, st)
    with pytest.raises(_hip.HipKernelError, match="multiple of 4"):
        _hip.call("agrl_linear_bn_relu", x.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(), 2, 62, 8, _hip.F32, st)
    assert float(out.abs().max()) == 0.0   # nothing was launched
