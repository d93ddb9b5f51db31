"""The train-step kernels (csrc/train.hip, wgrad.hip, train_tail.hip, the fp32 / split-bf16 uses of igemm.hip, the loss kernels)
held to ELEMENTWISE float64 bounds: every output element against a float64 reference of the kernel's stated arithmetic on the
fp32 operands it reads (tests/train_ref.py: references and chain lengths, derived in their docstrings), through
bounds.check_rounded(..., out_dtype=torch.float32). test_gpu_train.py judges the same kernels with one max-normalised number
against fp32 CPU autograd; that cannot see a channel 2^-12 of the largest, an element nobody wrote, or a lost factor of a few.

Every kernel call under test runs inside poisoned_outputs() (outputs and workspaces are torch.empty: NaN-filled here), runs
twice, and the two results must be bitwise equal (the kernels promise determinism without atomics). A kernel that consumes
another kernel's fp32 output (mean, invstd, dbeta, dgamma, an index map) is referenced on THE KERNEL'S OWN values, so a legitimate
last-bit difference upstream does not loosen the bar downstream. Above the reference budget (FULL_REF_FLOPS) a deterministic
subset is bounded (bound_pixels; for weight gradients train_ref.wgrad_channels); finiteness and run-to-run equality always cover
every element.

Measured on an MI355X (AGRL_BOUNDS_LOG), worst |got - exact| / bound per kernel family, with the chain length n_acc used:
    conv forward 0.54 (ceil(K / 4) + 3)        dgrad 1x1 0.35, flipped 3x3 0.13, parity phases 0.33, fork 0.36 (same count)
    dgrad 7x7 zero insertion 0.08 (n_acc up to 395: the kernel walks all 49 taps of a dy that is 3/4 inserted zeros, and
                                   adding an exact zero product rounds nothing -- the stated chain over-counts by ~4 there)
    wgrad 0.50 (8 cps + ks; plans seen: ks 1 .. 410, cps 1 .. 33, tiles 64 / 128 both ways)     wgrad splitk fallback 0.44
    bn stats mean 0.33, var 0.19 (rows per thread 1 .. 8)      dbeta 0.46, dgamma 0.43      bn backward dy 0.37 (10)
    bn fold invstd 0.34 (5: rsqrtf allowed 2 ulp), scale 0.41, shift 0.25, running_mean 0.76 (3), running_var 0.46 (5)
    bn apply 0.65 (3)      axpby 0.93 (1 or 2)      part pool backward 0.43 / 0.66      graph pair product 0.29, gram 0.37
    graph matrix backward 0.10 (propagated bound)     attention pool backward 0.06 (5 t + 3 S + 16: the stages' worst cases
    summed, which no single element meets)      xent dlogits 0.51, loss 0.07      triplet distances 0.15, loss 0.11, grad 0.07
Relative error of the biased variance against float64 for the ``offset`` kind (|mean| / std up to 128; on record, not asserted):
1.7e-3 at 35 rows (conv_stats, 36 channels), 5.7e-4 at 7 rows, 5.9e-5 at 8192 x 128, 4.8e-6 at 135 rows x 128 (conv_stats)."""
import numpy as np
import pytest
import torch

import train_ref as R
from bounds import check_rounded, log_record, poisoned_outputs
from test_gpu_kernels import FULL_REF_FLOPS, bound_pixels, conv_exact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


def twice(fn):
    """fn() -> tensor or tuple of tensors (None allowed), called twice under poisoned allocations: every element of every
    output finite, the two runs bitwise equal. Returns the first run's outputs on the CPU."""
    runs = []
    for _ in range(2):
        with poisoned_outputs():
            o = fn()
        torch.cuda.synchronize()
        runs.append(tuple(o) if isinstance(o, (tuple, list)) else (o,))
    for k, (a, b) in enumerate(zip(*runs)):
        assert (a is None) == (b is None)
        if a is None:
            continue
        if a.is_floating_point():
            assert bool(torch.isfinite(a).all()), "output %d: %d non-finite of %d elements" % (k, int((~torch.isfinite(a)).sum()), a.numel())
        assert torch.equal(a, b), "output %d differs between two runs (%d of %d elements)" % (k, int((a != b).sum()), a.numel())
    out = tuple(None if a is None else a.detach().cpu() for a in runs[0])
    return out if len(out) > 1 else out[0]


def mode_name(split):
    return "bf16x3" if split else "fp32"


def bound(got, exact, mag, n_acc, split, name, **kw):
    """check_rounded for an fp32 output; in the split-bf16 mode every product adds C_SPLIT |x| |w|: C_SPLIT mag of slack."""
    slack = kw.pop("slack", None)
    if split:
        slack = R.C_SPLIT * mag if slack is None else slack + R.C_SPLIT * mag
    chain = n_acc if isinstance(n_acc, (int, float)) else int(n_acc.max())
    return check_rounded(got, exact, mag, n_acc, F32, slack=slack, name="%s|n_acc=%d" % (name, chain), **kw)[0]


def operands(kind, shape_x, shape_dy, seed):
    if kind == "randn":
        g = torch.Generator().manual_seed(seed)
        return torch.randn(shape_x, generator=g), torch.randn(shape_dy, generator=g)
    return R.stress_train_operands(kind, shape_x, shape_dy, seed)


# ---- conv: forward, every data-gradient route, weight gradient ---------------------------------------------------------------
def check_wgrad(dw, x, dy, R_, stride, pad, plan, split, name, seed=0):
    """dw (Cout,Cin,R,S) from agrl_conv_wgrad under ``plan`` = (bm, bn, ks, cps)."""
    F_, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    M = dy.shape[0] * dy.shape[1] * dy.shape[2]
    full = 4.0 * M * Cout * Cin * R_ * R_ <= FULL_REF_FLOPS
    co = R.wgrad_channels(Cout, full, seed)
    exact, mag = R.wgrad_ref(x, dy, R_, R_, stride, pad, co)
    bm, bn, ks, cps = plan
    assert ks >= 1 and ks * cps * 32 >= M > (ks - 1) * cps * 32, (plan, M)
    return bound(dw[co], exact, mag, R.wgrad_chain(ks, cps), split, "wgrad|%s ks=%d cps=%d tile=%dx%d" % (name, ks, cps, bm, bn))


# (N, H, W, Cin, Cout, R, stride, pad); the route each exercises in HipConv2d._backward
CONV_SMALL = [
    ("fills no tile", (1, 5, 3, 32, 32, 3, 1, 1)),
    ("1x1 through linear_nobias", (3, 16, 8, 64, 128, 1, 1, 0)),
    ("1x1, K padding for Cout=702, splitk wgrad", (1, 16, 1, 2048, 702, 1, 1, 0)),
    ("1x1, K padding for Cout=625, splitk wgrad", (1, 24, 1, 256, 625, 1, 1, 0)),
    ("strided 1x1", (5, 8, 4, 128, 256, 1, 2, 0)),
    ("strided 1x1, odd frame", (2, 9, 5, 64, 64, 1, 2, 0)),
    ("3x3 flipped filter", (4, 16, 8, 64, 64, 3, 1, 1)),
    ("3x3 flipped filter, ragged pixels", (3, 7, 5, 32, 96, 3, 1, 1)),
    ("3x3, frame smaller than the filter", (2, 2, 2, 32, 32, 3, 1, 1)),
    ("3x3 stride 2 parity phases", (4, 16, 8, 64, 96, 3, 2, 1)),
    ("3x3 stride 2 parity phases, odd frame", (2, 9, 5, 32, 64, 3, 2, 1)),
    ("7x7 stride 2 zero insertion", (2, 32, 16, 32, 64, 7, 2, 3)),
    ("7x7 stride 2 zero insertion, odd frame", (1, 9, 7, 32, 32, 7, 2, 3)),
]
# the train step's own shapes at 256 x 128 frames (_train_hip.py, vmgn.py): 64 x 32 maps in layer 1, 32 x 16 in layer 2, 16 x 8 after
CONV_REAL = [
    ("stem as 160 -> 64 over im2col_rows (no data gradient)", (1, 16 * 128 * 64, 1, 160, 64, 1, 1, 0)),
    ("layer1 conv2", (32, 64, 32, 64, 64, 3, 1, 1)),
    ("layer2.0 conv2", (16, 64, 32, 128, 128, 3, 2, 1)),
    ("layer2.0 downsample", (16, 64, 32, 256, 512, 1, 2, 0)),
    ("layer4 conv1", (16, 16, 8, 2048, 512, 1, 1, 0)),
    ("layer4 conv2", (16, 16, 8, 512, 512, 3, 1, 1)),
]
CONV_PARAMS = ([(n, c, k) for n, c in CONV_SMALL for k in ("randn", "scaled")] +
               [(n, c, k) for n, c in (CONV_SMALL[6], CONV_SMALL[9], CONV_SMALL[4]) for k in ("dead", "offset", "sparse_dout")] +
               [(n, c, "scaled") for n, c in CONV_REAL])


@pytest.mark.parametrize("split", [False, True], ids=mode_name)
@pytest.mark.parametrize("name,cfg,kind", CONV_PARAMS, ids=["%s-%s" % (n.replace(" ", "_"), k) for n, _, k in CONV_PARAMS])
def test_conv_forward_dgrad_wgrad_elementwise(name, cfg, kind, split):
    """HipConv2d forward, data gradient (each route on its own) and weight gradient, exact fp32 and split-bf16. The float64 data
    gradient is the transposed-conv sum written out (train_ref.dgrad_ref), not autograd of fp32 tensors."""
    from torchreid import hip_ops as ops
    from torchreid.models._train_hip import HipConv2d
    N, H, W, Cin, Cout, R_, stride, pad = cfg
    OH, OW = (H + 2 * pad - R_) // stride + 1, (W + 2 * pad - R_) // stride + 1
    K = Cin * R_ * R_
    x, dy = operands(kind, (N, H, W, Cin), (N, OH, OW, Cout), sum(cfg))
    g = torch.Generator().manual_seed(sum(cfg) + 1)
    w = torch.randn((Cout, Cin, R_, R_), generator=g) / np.sqrt(K)
    needs_dx = Cin != 160
    xd, wd, dyd = x.to(DEV).requires_grad_(needs_dx), w.to(DEV).requires_grad_(True), dy.to(DEV)

    def call():
        xd.grad = wd.grad = None
        with ops.f32_split(split):
            y = HipConv2d.apply(xd, wd, stride, pad)
        y.backward(dyd)                       # backward re-enters the forward's arithmetic mode
        return y.detach(), xd.grad, wd.grad
    y, dx, dw = twice(call)
    tag = "%s %s %s" % (name, kind, mode_name(split))
    # forward
    pix = bound_pixels(N * OH * OW, K, Cout)
    exact, mag, pix, coords = conv_exact(x.permute(0, 3, 1, 2), w, torch.zeros(Cout), stride, pad, pixels=pix)
    bound(y.reshape(-1, Cout)[pix], exact, mag, R.gemm_chain(K), split, "conv forward|" + tag, coords=coords)
    # data gradient
    if needs_dx:
        route = "1x1" if R_ == 1 else ("phase" if (R_, stride, pad) == (3, 2, 1) else ("flip" if stride == 1 else "zero"))
        chain = R.dgrad_chain(route, Cout, R_, R_, H, W)
        if 4.0 * N * H * W * Cout * K <= FULL_REF_FLOPS:
            exact, mag = R.dgrad_ref(dy, w, stride, pad, H, W)
            bound(dx, exact, mag, chain, split, "conv dgrad %s|%s" % (route, tag))
            if route == "1x1" and stride > 1:
                untouched = torch.ones((H, W), dtype=torch.bool)
                untouched[::stride, ::stride] = False
                assert bool((dx[:, untouched] == 0).all()), "a strided 1x1 leaves the pixels it never sampled at exactly 0"
        else:
            pin = bound_pixels(N * H * W, R_ * R_ * Cout, Cin, seed=1)
            exact, mag = R.dgrad_ref(dy, w, stride, pad, H, W, pix=pin)
            if route == "phase":
                chain = chain.reshape(H * W)[pin % (H * W)].view(-1, 1)
            bound(dx.reshape(-1, Cin)[pin], exact, mag, chain, split, "conv dgrad %s|%s" % (route, tag))
    # weight gradient
    if ops.conv_wgrad_supported(Cin, Cout):
        with ops.f32_split(split):
            plan = ops.conv_wgrad_plan(N, H, W, Cin, Cout, R_, R_, stride, pad)
        check_wgrad(dw, x, dy, R_, stride, pad, plan, split, tag, seed=sum(cfg))
    else:   # channel counts that are not multiples of 4: im2col_t + gemm_nt_splitk, K = pixels padded to 32
        M = N * OH * OW
        exact, mag = R.wgrad_ref(x, dy, R_, R_, stride, pad)
        bound(dw, exact, mag, R.splitk_chain(-(-M // 32) * 32, Cout, R_ * R_ * Cin), split, "wgrad splitk|" + tag)


FORK_CASES = [("identity", (6, 16, 8, 256, 64, None, 1)), ("downsample", (6, 16, 8, 128, 64, 256, 1)),
              ("downsample stride 2", (4, 32, 16, 128, 64, 256, 2)), ("downsample stride 2, odd frame", (2, 9, 5, 64, 32, 128, 2)),
              ("layer3.0 fork", (16, 32, 16, 512, 256, 1024, 2)), ("layer4.1 fork", (16, 16, 8, 2048, 512, None, 1))]


@pytest.mark.parametrize("split", [False, True], ids=mode_name)
@pytest.mark.parametrize("name,cfg", FORK_CASES, ids=[n.replace(" ", "_") for n, _ in FORK_CASES])
def test_conv_fork_fused_residual_data_gradient(name, cfg, split):
    """HipConvFork._backward: dx = dy1 W1 + dshortcut (identity) or dyd Wd + dy1 W1 (downsample; stride 2 lands on the sampled
    pixels) with the sum as the ``residual`` operand of the data-gradient GEMM. The second GEMM's reference takes the first's
    fp32 result as its residual only in its magnitude: the exact value is the float64 sum of both transposed convs."""
    from torchreid import hip_ops as ops
    from torchreid.models._train_hip import HipConvFork
    N, H, W, Cin, C1, Cd, sd = cfg
    g = torch.Generator().manual_seed(sum(v or 0 for v in cfg))
    x = torch.randn((N, H, W, Cin), generator=g) * R.channel_scales(Cin, 3)
    w1 = torch.randn((C1, Cin, 1, 1), generator=g) / np.sqrt(Cin)
    wdn = None if Cd is None else torch.randn((Cd, Cin, 1, 1), generator=g) / np.sqrt(Cin)
    Hd, Wd = (H - 1) // sd + 1, (W - 1) // sd + 1
    dy1 = torch.randn((N, H, W, C1), generator=g) * R.channel_scales(C1, 4)
    dsc = torch.randn((N, H, W, Cin) if Cd is None else (N, Hd, Wd, Cd), generator=g)
    xd, w1d = x.to(DEV).requires_grad_(True), w1.to(DEV).requires_grad_(True)
    wdd = None if wdn is None else wdn.to(DEV).requires_grad_(True)

    def call():
        xd.grad = w1d.grad = None
        if wdd is not None:
            wdd.grad = None
        with ops.f32_split(split):
            res = HipConvFork.apply(xd, w1d, wdd, sd)
        torch.autograd.backward([res[0], res[3]], [dy1.to(DEV), dsc.to(DEV)])
        return xd.grad, w1d.grad, (None if wdd is None else wdd.grad)
    dx, dw1, dwd = twice(call)
    tag = "%s %s" % (name, mode_name(split))
    e1, m1 = R.dgrad_ref(dy1, w1, 1, 0, H, W)
    if Cd is None:
        exact, mag, chain = e1 + dsc.double(), m1 + dsc.double().abs(), R.gemm_chain(C1)
    else:
        e2, m2 = R.dgrad_ref(dsc, wdn, sd, 0, H, W)
        exact, mag, chain = e1 + e2, m1 + m2, R.gemm_chain(C1) + R.gemm_chain(Cd)
    bound(dx, exact, mag, chain, split, "conv fork dgrad|" + tag)
    with ops.f32_split(split):
        p1 = ops.conv_wgrad_plan(N, H, W, Cin, C1, 1, 1, 1, 0)
        pd = None if Cd is None else ops.conv_wgrad_plan(N, H, W, Cin, Cd, 1, 1, sd, 0)
    check_wgrad(dw1, x, dy1, 1, 1, 0, p1, split, tag + " conv1")
    if Cd is not None:
        check_wgrad(dwd, x, dsc, 1, sd, 0, pd, split, tag + " downsample")


# ragged shapes (test_gpu_train.py's, which fill no tile) and the train step's own, one per plan: 64 / 128 tiles in both
# dimensions, ks = 1 and ks in the hundreds (layer 1: >= 65 536 pixels against one weight tile)
WGRAD_CASES = [(3, 7, 5, 36, 20, 3, 1, 1), (2, 6, 4, 8, 12, 1, 1, 0), (5, 9, 6, 68, 132, 3, 2, 1), (1, 4, 4, 4, 4, 5, 1, 2), (70, 8, 4, 192, 320, 1, 2, 0),
               (1, 3, 3, 4, 8, 1, 1, 0), (4, 16, 8, 128, 64, 3, 1, 1),
               (32, 64, 32, 64, 64, 1, 1, 0), (32, 64, 32, 64, 256, 1, 1, 0), (32, 64, 32, 256, 64, 1, 1, 0), (16, 32, 16, 512, 128, 1, 1, 0),
               (16, 16, 8, 1024, 2048, 1, 1, 0), (16, 16, 8, 256, 256, 3, 1, 1), (1, 32 * 128 * 64, 1, 160, 64, 1, 1, 0)]
WGRAD_PARAMS = [(c, "scaled") for c in WGRAD_CASES] + [(c, k) for c in (WGRAD_CASES[2], WGRAD_CASES[4]) for k in ("randn", "dead", "offset", "sparse_dout")]


@pytest.mark.parametrize("cfg,kind", WGRAD_PARAMS, ids=["%s-%s" % ("x".join(str(v) for v in c), k) for c, k in WGRAD_PARAMS])
def test_conv_wgrad_elementwise(cfg, kind):
    """agrl_conv_wgrad in both arithmetic modes on one workspace sized for the larger of the two plans: chain from the plan
    the entry point makes (agrl_conv_wgrad_plan), dW = sum_p dy[p][co] x[p + tap][ci] in float64."""
    from torchreid import hip_ops as ops
    N, H, W, Cin, Cout, R_, stride, pad = cfg
    OH, OW = (H + 2 * pad - R_) // stride + 1, (W + 2 * pad - R_) // stride + 1
    x, dy = operands(kind, (N, H, W, Cin), (N, OH, OW, Cout), sum(cfg))
    xd, dyd = x.to(DEV), dy.to(DEV)
    nbytes = int(ops._hip.lib().agrl_conv_wgrad_workspace(N, H, W, Cin, Cout, R_, R_, stride, pad))
    plans = []
    for split in (False, True):
        with ops.f32_split(split):
            plan = ops.conv_wgrad_plan(N, H, W, Cin, Cout, R_, R_, stride, pad)
            dw = twice(lambda: ops.conv_wgrad(xd, dyd, (Cout, Cin, R_, R_), stride, pad))
        plans.append(plan)
        check_wgrad(dw, x, dy, R_, stride, pad, plan, split, "%s %s %s" % ("x".join(str(v) for v in cfg), kind, mode_name(split)), seed=sum(cfg))
    assert nbytes == max(p[2] for p in plans) * Cout * R_ * R_ * Cin * 4, "the shared workspace is the larger of the two plans"


# ---- BatchNorm family --------------------------------------------------------------------------------------------------------
def check_stats(mean, var, y, n_thread, extra, name, kind):
    ref = R.bn_stats_ref(y)
    ch = R.bn_stats_chain(n_thread + extra)
    check_rounded(mean, ref["mean"][0], ref["mean"][1], ch["mean"], F32, name="bn stats mean|%s|n_acc=%d" % (name, ch["mean"]))
    check_rounded(var, ref["var"][0], ref["var"][1], ch["var"], F32, name="bn stats var|%s|n_acc=%d" % (name, ch["var"]))
    assert bool((var >= 0).all())
    if kind == "offset":     # on record, not asserted: the conditioning of sum y^2 / M - mean^2 at |mean| >> std
        v64 = y.double().var(0, unbiased=False)
        relv = ((var.double() - v64).abs() / v64.clamp(min=1e-300))[v64 > 0]
        log_record({"name": "bn stats var offset|" + name, "rel_var_err_max": float(relv.max()), "rel_var_err_median": float(relv.median())})


# (M, C, relu, slope, residual): small, ragged (C % 4 == 0 only, M odd, M C / 4 odd), the scalar path (C % 4 != 0), and the train
# step's own: reduce_lanes 16 / 32 / 64, chunks clamped at 512 (layer 1) and at 1 (M <= 16), BatchNorm1d + LeakyReLU of a graph layer
BN_CASES = [(5, 4, True, 0.0, False), (7, 12, True, 0.0, True), (45, 20, True, 0.1, False), (33, 36, False, 0.0, True), (16, 64, True, 0.0, False),
            (301, 6, True, 0.0, True), (130, 70, False, 0.0, False),
            (32 * 64 * 32, 64, True, 0.0, False), (32 * 64 * 32, 256, True, 0.0, True), (16 * 32 * 16, 128, True, 0.0, False),
            (16 * 16 * 8, 1024, True, 0.0, True), (16 * 16 * 8, 2048, False, 0.0, False), (4 * 112, 2048, True, 0.1, False)]
BN_PARAMS = [(c, "scaled") for c in BN_CASES] + [(c, k) for c in (BN_CASES[1], BN_CASES[2], BN_CASES[5], BN_CASES[9]) for k in ("randn", "dead", "offset")]


@pytest.mark.parametrize("cfg,kind", BN_PARAMS, ids=["%dx%d-%s%s%s-%s" % (c[0], c[1], "act" if c[2] else "lin", "-leaky" if c[3] else "", "-res" if c[4] else "", k)
                                                     for c, k in BN_PARAMS])
def test_batchnorm_family_elementwise(cfg, kind):
    """bn_stats -> bn_fold_train -> bn_apply (+ sign mask) -> bn_backward (MODE 1 sums, apply, masked dz), each on the previous
    kernel's own fp32 outputs."""
    from torchreid import hip_ops as ops
    M, C, relu, slope, use_res = cfg
    seed = M + 3 * C
    x, dz_src = operands(kind, (1, M, 1, C), (1, M, 1, C), seed)
    y, dout = x.view(M, C), (dz_src.view(M, C) * R.channel_scales(C, seed + 9))
    g = torch.Generator().manual_seed(seed)
    res = torch.randn((M, C), generator=g) if use_res else None
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.2 * torch.randn(C, generator=g)
    rm0, rv0 = 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    yd, name = y.to(DEV), "%dx%d %s" % (M, C, kind)
    chunks, rpc, nrl = R.reduce_plan(M, C)
    assert int(ops._hip.lib().agrl_bn_workspace(M, C)) == chunks * 2 * C * 8, "train_ref.reduce_plan mirrors train.hip's reduce_chunks"
    n_thread = R.reduce_chain(M, C)
    mean, var = twice(lambda: ops.bn_stats(yd))
    check_stats(mean, var, y, n_thread, 0, name + " chunks=%d rpc=%d lanes=%d" % (chunks, rpc, R.reduce_lanes(C)), kind)
    if kind == "dead":
        assert bool((var[1::3] == 0).all() and (mean[1::3] == 0).all())
    # fold + running statistics, at the real n and at n = 1, 2
    eps, mom = 1e-5, 0.1
    md, vd, gd, bd = mean.to(DEV), var.to(DEV), gamma.to(DEV), beta.to(DEV)
    for n in (M, 1, 2):
        nbt0 = 41

        def fold():
            rm, rv, nbt = rm0.to(DEV), rv0.to(DEV), torch.tensor(nbt0, dtype=torch.int64, device=DEV)
            return ops.bn_fold_train(md, vd, gd, bd, eps, mom, n, rm, rv, nbt) + (rm, rv, nbt)
        scale, shift, invstd, rm, rv, nbt = twice(fold)
        got = {"scale": scale, "shift": shift, "invstd": invstd, "running_mean": rm, "running_var": rv}
        for k, (exact, mag, n_acc) in R.bn_fold_ref(mean, var, gamma, beta, eps, mom, n, rm0, rv0).items():
            check_rounded(got[k], exact, mag, n_acc, F32, name="bn fold %s|%s n=%d|n_acc=%d" % (k, name, n, n_acc))
        assert int(nbt) == nbt0 + 1 and bool(torch.isfinite(invstd).all())
    sd, hd, isd = scale.to(DEV), shift.to(DEV), invstd.to(DEV)
    doutd = dout.to(DEV)
    if C % 4 == 0:
        resd = None if res is None else res.to(DEV)
        out, mask = twice(lambda: ops.bn_apply(yd, sd, hd, resd, relu, slope, want_mask=True))
        exact, mag, n_acc = R.bn_apply_ref(y, scale, shift, res, relu, slope)
        check_rounded(out, exact, mag, n_acc, F32, name="bn apply|%s|n_acc=%d" % (name, n_acc))
        if relu:
            R.check_sign_mask(mask, out, "bn apply mask " + name)
        maskd = None if mask is None else mask.to(DEV)
        forms = [("mask", None, maskd)] if relu else [("linear", None, None)]
        if relu:
            forms.append(("out", out.to(DEV), None))
    else:       # the scalar kernels: no bn_apply (C % 4 == 0 there); the backward takes the forward output
        pre = (y.double() * scale.double() + shift.double()).float() + (res if use_res else 0)
        out = torch.where(pre > 0, pre, pre * torch.tensor(slope, dtype=F32)) if relu else pre
        forms = [("out", out.to(DEV), None)]
    dz_ref = torch.where(out > 0, dout, dout * torch.tensor(slope, dtype=F32)) if relu else dout
    for form, outd, maskd in forms:
        dy, dz, dgamma, dbeta = twice(lambda: ops.bn_backward(doutd, outd, yd, md, isd, gd, relu, True, slope, mask=maskd))
        assert torch.equal(dz, dz_ref), "dz is the masked dout exactly (%s form)" % form
        sums, ch = R.bn_backward_sums_ref(dz_ref, y, mean, invstd), R.bn_backward_sums_chain(n_thread, relu and slope != 0)
        for k, got in (("dbeta", dbeta), ("dgamma", dgamma)):
            check_rounded(got, sums[k][0], sums[k][1], ch[k], F32, name="bn backward %s|%s %s|n_acc=%d" % (k, name, form, ch[k]))
        exact, mag, n_acc = R.bn_backward_ref(dz_ref, y, mean, invstd, gamma, dbeta, dgamma)
        check_rounded(dy, exact, mag, n_acc, F32, name="bn backward dy|%s %s|n_acc=%d" % (name, form, n_acc))


STATS_CASES = [(40, 16, 8, 512, 256, 1, 1, 0), (3, 9, 5, 64, 128, 3, 2, 1), (2, 64, 32, 64, 64, 3, 1, 1), (5, 7, 3, 32, 36, 1, 1, 0), (1, 3, 3, 32, 4, 1, 1, 0),
               (32, 64, 32, 64, 256, 1, 1, 0), (1, 16 * 128 * 64, 1, 160, 64, 1, 1, 0)]
STATS_PARAMS = [(c, "scaled") for c in STATS_CASES] + [(c, k) for c in (STATS_CASES[1], STATS_CASES[3]) for k in ("dead", "offset")]


@pytest.mark.parametrize("cfg,kind", STATS_PARAMS, ids=["%s-%s" % ("x".join(str(v) for v in c), k) for c, k in STATS_PARAMS])
def test_conv_epilogue_statistics_elementwise(cfg, kind):
    """agrl_conv2d_stats -> agrl_bn_stats_from_partials: the conv output bitwise agrl_conv2d_bn_act's, mean / var against float64
    sums of that output. Chain: the per-tile sums of the epilogue (train_ref.STATS_TILE_CHAIN) + the column reduction over the
    ceil(M / 64) partial rows."""
    from torchreid import hip_ops as ops
    N, H, W, Cin, Cout, R_, stride, pad = cfg
    x, _ = operands(kind, (N, H, W, Cin), (1, 1, 1, 4), sum(cfg))
    g = torch.Generator().manual_seed(sum(cfg))
    w = (torch.randn((Cout, R_, R_, Cin), generator=g) / np.sqrt(Cin * R_ * R_) * R.channel_scales(Cout, 5).view(Cout, 1, 1, 1)).to(DEV)
    xd = x.to(DEV)
    for split in (False, True):
        with ops.f32_split(split):
            y, mean, var = twice(lambda: ops.conv_stats(xd, w, stride, pad))
            y_ref = twice(lambda: ops.conv_bn_act(xd, w, None, stride, pad, False))
        assert torch.equal(y, y_ref)
        y2 = y.view(-1, Cout)
        rows = -(-y2.shape[0] // 64)
        check_stats(mean, var, y2, R.reduce_chain(rows, 2 * Cout), R.STATS_TILE_CHAIN,
                    "conv_stats %s %s %s" % ("x".join(str(v) for v in cfg), kind, mode_name(split)), kind)


# ---- max pooling: exact ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ties", [((3, 16, 8, 64), "relu"), ((2, 9, 7, 32), "relu"), ((1, 1, 1, 4), "relu"), ((2, 2, 3, 8), "levels"),
                                        ((3, 13, 6, 5), "levels"), ((16, 128, 64, 64), "relu")])
def test_maxpool_forward_backward_exact(shape, ties):
    """Value and tap index: first maximum in scan order, strict >; backward: the gather of dout through the kernel's own indices.
    Every element, ties included (post-ReLU zeros; three-level inputs tie at every value)."""
    from torchreid import hip_ops as ops
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g).relu() if ties == "relu" else torch.randint(-1, 2, shape, generator=g).float()
    xd = x.to(DEV)
    out, idx = twice(lambda: ops.maxpool3x3s2(xd))
    ref, ref_idx = R.maxpool_ref(x)
    assert torch.equal(out, ref)
    assert torch.equal(idx, ref_idx), "%d of %d tap indices differ" % (int((idx != ref_idx).sum()), idx.numel())
    dout = torch.randn(out.shape, generator=g)
    doutd, idxd = dout.to(DEV), idx.to(DEV)
    dx = twice(lambda: ops.maxpool3x3s2_backward(doutd, idxd, shape[1], shape[2]))
    assert torch.equal(dx, R.maxpool_backward_ref(dout, idx, shape[1], shape[2]))


# ---- tail and losses -------------------------------------------------------------------------------------------------------------
def test_tail_kernels_elementwise():
    """axpby, part_pool_backward, graph_pair_product, xent_label_smooth against float64 of the formulas in their header comments."""
    from torchreid import hip_ops as ops
    g = torch.Generator().manual_seed(21)
    for shape in ((5, 7, 64), (3,), (16, 112, 2048)):
        a_, b_ = torch.randn(shape, generator=g), torch.randn(shape, generator=g) * 2.0 ** -12
        ad, bd = a_.to(DEV), b_.to(DEV)
        exact, mag, n_acc = R.axpby_ref(0.9, a_, 0.1, b_)
        check_rounded(twice(lambda: ops.axpby(0.9, ad, 0.1, bd)), exact, mag, n_acc, F32, name="axpby|%s|n_acc=%d" % (shape, n_acc))
        exact, mag, n_acc = R.axpby_ref(-0.3, a_, 0.0, None)
        check_rounded(twice(lambda: ops.axpby(-0.3, ad)), exact, mag, n_acc, F32, name="axpby|%s no y|n_acc=%d" % (shape, n_acc))
    for F_, S, h, w, C, splits in ((8, 4, 16, 8, 64, (4, 2, 1)), (2, 1, 5, 3, 12, (4, 2, 1)), (64, 16, 16, 8, 2048, (4, 2, 1)), (3, 3, 7, 2, 8, (3,))):
        P = sum(splits)
        dg = torch.randn((F_ // S, C), generator=g) * R.channel_scales(C, 1)
        dn = torch.randn((F_, P, C), generator=g) * R.channel_scales(C, 2)
        dgd, dnd = dg.to(DEV), dn.to(DEV)
        dx1, dx2 = twice(lambda: ops.part_pool_backward(dgd, dnd, S, h, w, splits))
        (e1, m1, n1), (e2, m2, n2) = R.part_pool_backward_ref(dg, dn, S, h, w, splits)
        tag = "%dx%dx%dx%d" % (F_, h, w, C)
        check_rounded(dx1, e1, m1, n1, F32, name="part pool backward dx1|%s|n_acc=%d" % (tag, n1))
        check_rounded(dx2, e2, m2, n2, F32, name="part pool backward dx2|%s|n_acc=%d" % (tag, n2))
        none, dx2b = twice(lambda: ops.part_pool_backward(None, dnd, S, h, w, splits))
        assert none is None and torch.equal(dx2b, dx2)
    for B, V, C in ((16, 112, 2048), (3, 28, 256), (2, 144, 128), (5, 7, 384)):
        a_ = torch.randn((B, V, C), generator=g) * R.channel_scales(C, 3)
        b_ = torch.randn((B, V, C), generator=g)
        ad, bd = a_.to(DEV), b_.to(DEV)
        exact, mag, n_acc = R.pair_product_ref(a_, b_)
        check_rounded(twice(lambda: ops.graph_pair_product(ad, bd)), exact, mag, n_acc, F32, name="graph pair product|%dx%dx%d|n_acc=%d" % (B, V, C, n_acc))
    for n, K, scale in ((16, 702, 3.0), (4, 5, 3.0), (64, 625, 10.0), (1, 300, 0.01)):
        z = scale * torch.randn((n, K), generator=g)
        y = torch.randint(0, K, (n,), generator=g)
        zd, yd = z.to(DEV), y.to(torch.int32).to(DEV)
        loss, dl = twice(lambda: ops.xent_label_smooth(zd, yd, 0.1))
        (l64, lb), (d64, db) = R.xent_ref(z, y, 0.1)
        check_rounded(dl, d64, torch.zeros_like(d64), 0, F32, slack=db, name="xent dlogits|%dx%d" % (n, K))
        check_rounded(loss, l64, torch.zeros(1, dtype=torch.float64), 0, F32, slack=lb, name="xent loss|%dx%d" % (n, K))


def test_attention_pool_backward_elementwise():
    """agrl_attn_pool_backward against float64 of the formula in its header comment; an all-zero node passes no gradient
    through its norm (the kernel's stated convention, used by the reference too)."""
    from torchreid import hip_ops as ops
    g = torch.Generator().manual_seed(31)
    for B, S, P, C in ((3, 6, 7, 128), (4, 16, 7, 2048), (1, 1, 1, 4), (2, 3, 5, 260)):
        nodes = torch.rand((B, S, P, C), generator=g) * R.channel_scales(C, 7, -6, 2)
        nodes[B // 2, S // 2, P // 2] = 0
        datt = torch.randn((B, C), generator=g)
        nd, dd = nodes.to(DEV), datt.to(DEV)
        exact, mag, n_acc = R.attn_pool_backward_ref(nodes, datt)
        check_rounded(twice(lambda: ops.attn_pool_backward(nd, dd)), exact, mag, n_acc, F32, name="attn pool backward|%dx%dx%dx%d|n_acc=%d" % (B, S, P, C, n_acc))


@pytest.mark.parametrize("cfg", [(3, 56, 256, True, False), (2, 112, 2048, True, False), (2, 28, 512, False, False), (1, 7, 128, True, True),
                                 (4, 112, 2048, False, True)])
def test_graph_matrix_backward_elementwise(cfg):
    """agrl_graph_matrix_backward on the Gram partials agrl_graph_gram itself produced, against float64 of the formulas in its
    header comment with the rounding of every fp32 step propagated through them (train_ref.graph_matrix_backward_ref). The
    reference uses the kernel's stated convention for the diagonal: D2_ii is identically 0, E_ii = 0, no gradient passes there
    (the reference model's fp32 autograd takes sqrt' of cancellation noise at that spot)."""
    from torchreid import hip_ops as ops
    B, V, C, use_pose, mask_diag = cfg
    g = torch.Generator().manual_seed(V + C)
    f = torch.rand((B, 1, C), generator=g) * 0.2 + 0.05 * torch.randn((B, V, C), generator=g)
    dG = torch.randn((B, V, V), generator=g)
    fd, dGd = f.to(DEV), dG.to(DEV)
    gram = twice(lambda: ops.graph_gram(fd))
    gd = gram.to(DEV)
    M = twice(lambda: ops.graph_matrix_backward(gd, dGd, use_pose, mask_diag))
    exact, slack, live = R.graph_matrix_backward_ref(gram, dG, use_pose, mask_diag)
    eye = torch.eye(V, dtype=torch.bool)
    assert bool(live[:, ~eye].all()), "every off-diagonal distance is far above the clamp in this case"
    check_rounded(M, exact, torch.zeros_like(exact), 0, F32, slack=slack, name="graph matrix backward|%dx%dx%d pose=%d mask=%d" % cfg)
    # ... and the Gram partials themselves: 128-channel slices by exact-fp32 MFMA, 32 roundings each
    f64 = f.double().view(B, V, C // 128, 128).permute(0, 2, 1, 3)
    check_rounded(gram, f64 @ f64.transpose(2, 3), f64.abs() @ f64.abs().transpose(2, 3), 32 + 3, F32, name="graph gram|%dx%dx%d|n_acc=35" % (B, V, C))


@pytest.mark.parametrize("soft", [True, False], ids=["soft", "margin"])
def test_triplet_loss_elementwise(soft):
    """agrl_triplet_loss: mined distances and pairs against float64 (ties within the distance bound may go either way), the
    loss and the feature gradient against float64 of the stated formulas on the kernel's own pairs and distances."""
    from torchreid._hip import call, ptr, stream_ptr
    g = torch.Generator().manual_seed(41)
    for n, d, ids in ((16, 2048, 4), (8, 64, 2), (64, 300, 16), (4, 5, 2)):
        x = torch.randn((n, d), generator=g) * (0.05 if d > 1000 else 1.0)
        x[1] = x[0]                                        # a zero distance: at the clamp, passes no gradient
        pids = torch.arange(ids).repeat_interleave(n // ids)
        xd, pd = x.to(DEV), pids.to(torch.int32).to(DEV)

        def run():
            loss, grad = torch.empty((1,), device=DEV), torch.empty((n, d), device=DEV)
            dap, dan, coeff = torch.empty((n,), device=DEV), torch.empty((n,), device=DEV), torch.empty((2 * n,), device=DEV)
            iap, ian = torch.empty((n,), dtype=torch.int32, device=DEV), torch.empty((n,), dtype=torch.int32, device=DEV)
            call("agrl_triplet_loss", ptr(xd), ptr(pd), n, d, 0.3, 1 if soft else 0, ptr(loss), ptr(grad), ptr(dap), ptr(dan), ptr(iap), ptr(ian),
                 ptr(coeff), stream_ptr(xd.device))
            return loss, grad, dap, dan, iap, ian
        loss, grad, dap, dan, iap, ian = twice(run)
        assert bool(((iap >= 0) & (iap < n) & (ian >= 0) & (ian < n)).all())
        ref = R.triplet_ref(x, pids, 0.3, soft, dap, dan, iap, ian)
        D, dbound, same = ref["mining"]
        ar = torch.arange(n)
        assert bool(same[ar, iap.long()].all()) and not bool(same[ar, ian.long()].any())
        hardest_p = torch.where(same, D, torch.full_like(D, -1.0)).max(1).values
        hardest_n = torch.where(same, torch.full_like(D, float("inf")), D).min(1).values
        assert bool((D[ar, iap.long()] >= hardest_p - 2 * dbound.max(1).values).all()) and bool((D[ar, ian.long()] <= hardest_n + 2 * dbound.max(1).values).all())
        tag = "%dx%d %s" % (n, d, "soft" if soft else "margin")
        zero = torch.zeros(n, dtype=torch.float64)
        check_rounded(dap, ref["dist_ap"][0], zero, 0, F32, slack=ref["dist_ap"][3], name="triplet d_ap|" + tag)
        check_rounded(dan, ref["dist_an"][0], zero, 0, F32, slack=ref["dist_an"][3], name="triplet d_an|" + tag)
        check_rounded(loss, ref["loss"][0], zero[:1], 0, F32, slack=ref["loss"][3], name="triplet loss|" + tag)
        check_rounded(grad, ref["grad"][0], ref["grad"][1], ref["grad"][2], F32, name="triplet grad|%s|n_acc=%d" % (tag, ref["grad"][2]))


# ---- host-side argument checks: every case returns before any launch ---------------------------------------------------------
def test_train_entry_points_reject_bad_arguments():
    """Read off the entry points (wgrad.hip, train.hip): each of these fails an AGRL_CHECK_ARG that precedes the first launch, so
    nothing reaches the GPU with bad arguments."""
    from torchreid import hip_ops as ops
    from torchreid._hip import F32 as F32_CODE, HipKernelError, call, ptr, stream_ptr
    buf = torch.zeros(4096, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.float64, device=DEV)
    st = stream_ptr(buf.device)
    with pytest.raises(HipKernelError, match="multiples of 4"):       # Cin % 4 != 0
        call("agrl_conv_wgrad", ptr(buf), ptr(buf), ptr(buf), 1, 4, 4, 6, 8, 1, 1, 1, 0, F32_CODE, ptr(ws), ws.numel() * 8, st)
    bm, bn, ks, cps = ops.conv_wgrad_plan(1, 8, 8, 8, 8, 3, 3, 1, 1)
    need = ks * 8 * 9 * 8 * 4
    with pytest.raises(HipKernelError, match="workspace too small"):
        call("agrl_conv_wgrad", ptr(buf), ptr(buf), ptr(buf), 1, 8, 8, 8, 8, 3, 3, 1, 1, F32_CODE, ptr(ws), need - 1, st)
    need = int(ops._hip.lib().agrl_bn_workspace(64, 8))
    with pytest.raises(HipKernelError, match="workspace too small"):
        call("agrl_bn_stats", ptr(buf), ptr(buf), ptr(buf), 64, 8, ptr(ws), need - 1, st)
    with pytest.raises(HipKernelError, match="workspace too small"):
        call("agrl_bn_backward", ptr(buf), None, None, ptr(buf), ptr(buf), ptr(buf), ptr(buf), 0, 0.0, ptr(buf), None, ptr(buf), ptr(buf), 64, 8,
             ptr(ws), need - 1, st)
    with pytest.raises(HipKernelError, match="C must be even"):
        call("agrl_bn_stats_from_partials", ptr(buf), 4, 7, 256, ptr(buf), ptr(buf), ptr(ws), ws.numel() * 8, st)
    with pytest.raises(HipKernelError, match="needs the forward output or the sign mask"):
        call("agrl_bn_backward", ptr(buf), None, None, ptr(buf), ptr(buf), ptr(buf), ptr(buf), 1, 0.0, ptr(buf), None, ptr(buf), ptr(buf), 64, 8,
             ptr(ws), ws.numel() * 8, st)
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and bool((ws == 0).all()), "a rejected call writes nothing"
