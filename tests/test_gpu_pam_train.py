"""ganet's position-attention part nodes under train() on the GPU (csrc/pam.hip): agrl_pam_pool_train, agrl_pam_pool_backward,
agrl_pam_combine_train, agrl_pam_combine_backward and agrl_col_sum, every output element against float64 of the formulas in
include/agrl_hip.h with the bounds of tests/pam_train_ref.py (derived in its docstring), under NaN-poisoned allocations and run
twice (test_gpu_train_bounds.twice). Also: the autograd nodes against the direct calls, the attention pooling at ganet's
6144 channels, and the argument checks.

Inputs: the map and every gradient carry per-channel scales 2^-12 .. 2^3 (train_ref.channel_scales); the query rows alternate
between a scale of 4 and one of 2^-6 by position, so the float64 attention of one case has peaked rows (row maximum > 0.5) and flat
ones. "Flat" is a row maximum < 0.1 where the case's largest slice has more than 15 positions; the three cases whose largest
slice has 8 or 9 positions cannot go below 1 / L > 0.1, there the bar is 1.5 / L.

Measured on an MI355X, worst |got - exact| / bound over the six cases: forward abar 0.06 (propagated bound), xbar 0.35, xmean 0.38;
backward dx 0.67 (3 roundings per level on the kernel's own abar), dqk 0.04 (propagated bound: the worst cases of the energy, the
softmax and three products summed, which no single element meets), abar as the forward's, bit for bit."""
import pytest
import torch

import pam_train_ref as PR
import train_ref as R
from bounds import check_rounded, poisoned_outputs
from test_gpu_train_bounds import twice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32

# (F, h, w, C, Cq, splits): L = 128 (the LDS limit) | remainder rows, L no multiple of 8 or 64, C no multiple of 256 | the model's
# channel counts | no pyramid | one slice | a last row no slice covers
CASES = [(3, 16, 8, 256, 32, [4, 2, 1]), (2, 6, 5, 96, 32, [4, 2, 1]), (1, 16, 8, 2048, 256, [4, 2, 1]), (2, 8, 4, 128, 32, [4]),
         (2, 3, 3, 64, 32, [1]), (2, 7, 3, 64, 32, [2])]
IDS = ["%dx%dx%dx%dx%d-%s" % (c[:5] + ("".join(str(s) for s in c[5]),)) for c in CASES]

_PROBLEMS = {}


def problem(case):
    """The case's fp32 operands on the CPU, made once and shared."""
    key = IDS[CASES.index(case)]
    if key not in _PROBLEMS:
        F_, h, w, C, Cq, splits = case
        P = sum(splits)
        g = torch.Generator().manual_seed(F_ + 3 * h + 5 * w + C + Cq)
        x = torch.randn((F_, h, w, C), generator=g) * R.channel_scales(C, 1)
        rowscale = torch.where(torch.arange(h * w) % 2 == 0, torch.tensor(4.0), torch.tensor(2.0 ** -6)).view(1, h, w, 1)
        q = torch.randn((F_, h, w, Cq), generator=g) * rowscale
        k = torch.randn((F_, h, w, Cq), generator=g) / Cq ** 0.5
        _PROBLEMS[key] = dict(
            x=x.contiguous(), qk=torch.cat([q, k], 3).contiguous(),
            dxbar=(torch.randn((F_, P, C), generator=g) * R.channel_scales(C, 2)).contiguous(),
            dxmean=(torch.randn((F_, P, C), generator=g) * R.channel_scales(C, 3)).contiguous(),
            y=(torch.randn((F_, P, C), generator=g) * R.channel_scales(C, 4)).contiguous(),
            bv=torch.randn((C,), generator=g) * R.channel_scales(C, 5),
            dnodes=(torch.randn((F_, P, C), generator=g) * R.channel_scales(C, 6)).contiguous())
    return _PROBLEMS[key]


def slack_check(got, exact, slack, name):
    return check_rounded(got, exact, torch.zeros_like(exact), 0, F32, slack=slack, name=name)[0]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pam_pool_train_forward_elementwise(case):
    from torchreid import hip_ops as ops
    F_, h, w, C, Cq, splits = case
    pr = problem(case)
    xd, qkd = pr["x"].to(DEV), pr["qk"].to(DEV)
    xbar, xmean, abar = twice(lambda: ops.pam_pool_train(xd, qkd, splits))
    ref = PR.forward_ref(pr["x"], pr["qk"], splits, abar)
    rmax = torch.cat([m.reshape(-1) for m in ref["row_max"]])
    Lmax = max((r1 - r0) * w for r0, r1 in PR.slices(splits, h))
    big = torch.cat([m.reshape(-1) for m, (r0, r1) in zip(ref["row_max"], PR.slices(splits, h)) if (r1 - r0) * w == Lmax])
    assert float(rmax.max()) > 0.5 and float(big.min()) < (0.1 if Lmax > 15 else 1.5 / Lmax), (float(rmax.max()), float(big.min()), Lmax)
    tag = IDS[CASES.index(case)]
    r1_ = slack_check(abar, *ref["abar"], "pam forward abar|" + tag)
    r2_ = check_rounded(xbar, *ref["xbar"], F32, name="pam forward xbar|" + tag)[0]
    r3_ = check_rounded(xmean, *ref["xmean"], F32, name="pam forward xmean|" + tag)[0]
    print("pam forward %s: worst err / bound abar %.3f xbar %.3f xmean %.3f" % (tag, r1_, r2_, r3_))
    for part, (r0, r1) in enumerate(PR.slices(splits, h)):
        assert bool((abar[:, part, (r1 - r0) * w:] == 0).all()), "abar is zero beyond the slice's positions"
    # the eval entry point runs the same kernel: same bits
    xbar_e, xmean_e = ops.pam_pool(xd, qkd, splits)
    assert torch.equal(xbar_e.cpu(), xbar) and torch.equal(xmean_e.cpu(), xmean)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pam_pool_backward_elementwise(case):
    from torchreid import hip_ops as ops
    F_, h, w, C, Cq, splits = case
    pr = problem(case)
    xd, qkd, dbd, dmd = (pr[k].to(DEV) for k in ("x", "qk", "dxbar", "dxmean"))
    dx, dqk, abar = twice(lambda: ops.pam_pool_backward(xd, qkd, dbd, dmd, splits, want_abar=True))
    ref = PR.backward_ref(pr["x"], pr["qk"], pr["dxbar"], pr["dxmean"], splits, abar)
    tag = IDS[CASES.index(case)]
    r1_ = slack_check(abar, *ref["abar"], "pam backward abar|" + tag)
    r2_ = check_rounded(dx, *ref["dx"], F32, name="pam backward dx|" + tag)[0]
    r3_ = slack_check(dqk, *ref["dqk"], "pam backward dqk|" + tag)
    print("pam backward %s: worst err / bound abar %.3f dx %.3f dqk %.3f" % (tag, r1_, r2_, r3_))
    cov = PR.covered_rows(splits, h)
    assert bool((dx[:, ~cov] == 0).all()) and bool((dqk[:, ~cov] == 0).all()), "positions no slice covers get exactly 0"
    assert bool(cov.all()) == (case != CASES[5])
    if case == CASES[1]:   # h = 6: the four-slice level drops rows 4 and 5; the other two levels still reach them
        assert bool((dx[:, 4:] != 0).all()) and float(dqk[:, 4:].abs().max()) > 0 and float(ref["dqk"][0][:, 4:].abs().max()) > 0
    # the forward's abar and the one recomputed here come from the same code
    _, _, abar_f = ops.pam_pool_train(xd, qkd, splits)
    assert torch.equal(abar_f.cpu(), abar)
    # the bias gradient of the stacked query / key conv: column sums of the kernel's own dqk
    dqkd = dqk.to(DEV).view(-1, 2 * Cq)
    db = twice(lambda: ops.col_sum(dqkd))
    check_rounded(db, *PR.col_sum_ref(dqk.view(-1, 2 * Cq), ops.col_sum_plan(F_ * h * w)), F32, name="pam qk bias column sums|" + tag)


@pytest.mark.parametrize("gamma", [0.5, 0.0])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pam_combine_forward_backward_elementwise(case, gamma):
    from torchreid import hip_ops as ops
    F_, h, w, C, Cq, splits = case
    pr = problem(case)
    P = sum(splits)
    yd, bvd, dnd = pr["y"].to(DEV), pr["bv"].to(DEV), pr["dnodes"].to(DEV)
    xmd = pr["dxmean"].to(DEV)                                   # any (F,P,C) tensor serves as xmean here
    gd = torch.tensor([gamma], device=DEV)
    tag = "%s gamma=%g" % (IDS[CASES.index(case)], gamma)
    nodes = twice(lambda: ops.pam_combine_train(yd, bvd, xmd, gd))
    check_rounded(nodes, *PR.combine_ref(pr["y"], pr["bv"], pr["dxmean"], gamma), F32, name="pam combine|" + tag)
    dy, dxmean, dgamma, dbv = twice(lambda: ops.pam_combine_backward(dnd, yd, bvd, gd))
    ref = PR.combine_backward_ref(pr["dnodes"], pr["y"], pr["bv"], gamma, ops.col_sum_plan(F_ * P))
    for name, got in (("dy", dy), ("dxmean", dxmean), ("dgamma", dgamma), ("dbv", dbv)):
        check_rounded(got, *ref[name], F32, name="pam combine backward %s|%s" % (name, tag))
    assert float(dgamma.abs()) > 0, "d loss / d gamma is not zero at gamma == 0"


def test_pam_autograd_nodes_equal_the_direct_calls():
    """HipPamNodes / HipPamCombine through torch.autograd: bitwise the entry points called by hand."""
    from torchreid import hip_ops as ops
    from torchreid.models._train_hip import HipPamCombine, HipPamNodes
    case = CASES[1]
    F_, h, w, C, Cq, splits = case
    pr = problem(case)
    g = torch.Generator().manual_seed(5)
    bqk = torch.randn((2 * Cq,), generator=g).to(DEV).requires_grad_(True)
    xd, qk0 = pr["x"].to(DEV).requires_grad_(True), pr["qk"].to(DEV).requires_grad_(True)
    dbd, dmd = pr["dxbar"].to(DEV), pr["dxmean"].to(DEV)
    xbar, xmean = HipPamNodes.apply(xd, qk0, bqk, tuple(splits))
    torch.autograd.backward([xbar, xmean], [dbd, dmd])
    one = torch.ones((2 * Cq,), device=DEV)
    qk, _ = ops.bn_apply(qk0.detach().view(-1, 2 * Cq), one, bqk.detach(), None, False)
    qk = qk.view(qk0.shape)
    assert torch.equal(qk, qk0.detach() + bqk.detach())
    xbar_d, xmean_d, _ = ops.pam_pool_train(xd.detach(), qk, splits)
    dx_d, dqk_d = ops.pam_pool_backward(xd.detach(), qk, dbd, dmd, splits)
    assert torch.equal(xbar.detach(), xbar_d) and torch.equal(xmean.detach(), xmean_d)
    assert torch.equal(xd.grad, dx_d) and torch.equal(qk0.grad, dqk_d) and torch.equal(bqk.grad, ops.col_sum(dqk_d.view(-1, 2 * Cq)))
    yd, bvd = pr["y"].to(DEV).requires_grad_(True), pr["bv"].to(DEV).requires_grad_(True)
    xm, gm = pr["dxmean"].to(DEV).requires_grad_(True), torch.tensor([0.3], device=DEV, requires_grad=True)
    nodes = HipPamCombine.apply(yd, bvd, xm, gm)
    nodes.backward(pr["dnodes"].to(DEV))
    dy, dxm, dg, dbv = ops.pam_combine_backward(pr["dnodes"].to(DEV), yd.detach(), bvd.detach(), gm.detach())
    assert torch.equal(nodes.detach(), ops.pam_combine_train(yd.detach(), bvd.detach(), xm.detach(), gm.detach()))
    assert torch.equal(yd.grad, dy) and torch.equal(xm.grad, dxm) and torch.equal(gm.grad, dg) and torch.equal(bvd.grad, dbv)


def test_attention_pool_at_the_concatenated_width():
    """ganet pools (num_gb + 1) * 2048 = 6144 channels: agrl_row_sqnorm + agrl_attn_pool_bnneck's attention branch and
    agrl_attn_pool_backward at that width (no other test goes beyond 2048), through the node the model uses."""
    from torchreid.models._train_hip import HipAttnPool
    B, S, P, C = 2, 4, 7, 6144
    g = torch.Generator().manual_seed(61)
    nodes = torch.rand((B, S, P, C), generator=g) * R.channel_scales(C, 7, -6, 2)
    nodes[1, 2, 3] = 0
    datt = torch.randn((B, C), generator=g)
    nd, dd = nodes.to(DEV).requires_grad_(True), datt.to(DEV)

    def run():
        nd.grad = None
        att = HipAttnPool.apply(nd)
        att.backward(dd)
        return att.detach(), nd.grad
    att, dn = twice(run)
    check_rounded(att, *PR.attn_pool_forward_ref(nodes), F32, name="attn pool forward|%dx%dx%dx%d" % (B, S, P, C))
    check_rounded(dn, *R.attn_pool_backward_ref(nodes, datt), F32, name="attn pool backward|%dx%dx%dx%d" % (B, S, P, C))


def test_pam_train_entry_points_reject_bad_arguments():
    """Each of these fails an AGRL_CHECK_ARG that precedes the first launch (and the clearing of dqk): nothing is written."""
    import ctypes as C
    from torchreid._hip import F32 as F32_CODE, LP16, HipKernelError, call, ptr, stream_ptr
    buf = torch.zeros(1 << 16, device=DEV)
    st = stream_ptr(buf.device)
    b = ptr(buf)

    def arr(*v):
        return (C.c_int * len(v))(*v)

    def fwd(**kw):
        a = dict(x=b, qk=b, F=1, h=4, w=4, C=64, Cq=32, splits=arr(2, 1), n=2, dtype=F32_CODE)
        a.update(kw)
        call("agrl_pam_pool_train", a["x"], a["qk"], b, b, b, a["F"], a["h"], a["w"], a["C"], a["Cq"], a["splits"], a["n"], a["dtype"], st)

    def bwd(**kw):
        a = dict(x=b, dx=b, F=1, h=4, w=4, C=64, Cq=32, splits=arr(2, 1), n=2, dtype=F32_CODE)
        a.update(kw)
        call("agrl_pam_pool_backward", a["x"], b, b, b, a["dx"], b, b, a["F"], a["h"], a["w"], a["C"], a["Cq"], a["splits"], a["n"], a["dtype"], st)
    for fn in (fwd, bwd):
        with pytest.raises(HipKernelError, match="null pointer"):
            fn(x=None)
        with pytest.raises(HipKernelError, match="multiple of 32"):
            fn(Cq=24)
        with pytest.raises(HipKernelError, match="at most 16 parts"):
            fn(h=32, w=1, splits=arr(16, 1))
        with pytest.raises(HipKernelError, match="at most 128 supported"):
            fn(h=17, w=8, splits=arr(1), n=1)
        with pytest.raises(HipKernelError, match="bad dtype"):
            fn(dtype=LP16)
        with pytest.raises(HipKernelError, match="bad shape"):
            fn(F=0)
    with pytest.raises(HipKernelError, match="null pointer"):
        bwd(dx=None)
    with pytest.raises(HipKernelError, match="null pointer"):
        call("agrl_pam_combine_train", b, b, b, None, b, 4, 64, st)
    with pytest.raises(HipKernelError, match="workspace too small"):
        call("agrl_pam_combine_backward", b, b, b, b, b, b, b, b, 64, 64, b, (2 * 2 + 1) * 64 * 4 - 1, st)
    with pytest.raises(HipKernelError, match="workspace too small"):
        call("agrl_col_sum", b, b, 64, 64, b, (2 * 2 + 1) * 64 * 4 - 1, st)
    with pytest.raises(HipKernelError, match="bad shape"):
        call("agrl_col_sum", b, b, 0, 64, b, 1 << 16, st)
    torch.cuda.synchronize()
    assert bool((buf == 0).all()), "a rejected call writes nothing"
