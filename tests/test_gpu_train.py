"""Native train step (BASELINE config 4; reference train(), train_vidreid_xent_htri.py:397-413): the conv trunk's forward
with batch-statistics BatchNorm and its whole backward on the HIP kernels, against the SAME step computed on the CPU by the
stock-torch module tree (the reference's arithmetic: nn.Conv2d / nn.BatchNorm2d / autograd).

These 57 tests judge whole nodes and the whole step with one max-normalised number, rel() = max |a - b| / max |b|, mostly
against fp32 CPU autograd. Kernel by kernel the same train-step kernels are held to elementwise float64 bounds, NaN-poisoned
outputs and workspaces, adversarial channel scales and run-to-run bitwise equality in tests/test_gpu_train_bounds.py (references
and chain lengths: tests/train_ref.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vmgn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("cfg", [(3, 16, 8, 64, 128, 1, 1, 0), (4, 16, 8, 64, 64, 3, 1, 1), (4, 16, 8, 64, 96, 3, 2, 1), (5, 8, 4, 128, 256, 1, 2, 0),
                                 (2, 9, 5, 32, 64, 3, 2, 1), (2, 32, 16, 32, 64, 7, 2, 3), (40, 16, 8, 512, 256, 1, 1, 0),
                                 (9, 16, 8, 256, 256, 3, 1, 1)])
def test_conv_forward_dgrad_wgrad(cfg, split):
    """HipConv2d: forward, data gradient (flipped-filter conv / W^T GEMM, zero-inserted for stride 2) and weight gradient
    (agrl_conv_wgrad: contraction over the pixel axis straight from the NHWC activations, pixel axis split over workgroups;
    channel counts that are not multiples of 4 go through the transposes + NT GEMM) against F.conv2d + autograd in fp32 on the
    CPU -- in the exact-fp32 mode and in the split-bf16 mode (hip_train_precision 'bf16x3': ~1e-5 per product)."""
    from torchreid.models._train_hip import HipConv2d
    from torchreid import hip_ops
    N, H, W, Cin, Cout, R, stride, pad = cfg
    if split and (Cin % 32 or Cout % 32):
        pytest.skip("forward GEMM of the split mode: K multiple of 32")
    g = torch.Generator().manual_seed(sum(cfg))
    x = torch.randn((N, Cin, H, W), generator=g, requires_grad=True)
    w = (torch.randn((Cout, Cin, R, R), generator=g) / np.sqrt(Cin * R * R)).requires_grad_(True)
    y = F.conv2d(x, w, stride=stride, padding=pad)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    xd = x.detach().permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    wd = w.detach().to(DEV).requires_grad_(True)
    with hip_ops.f32_split(split):
        yd = HipConv2d.apply(xd, wd, stride, pad)
    yd.backward(dy.permute(0, 2, 3, 1).contiguous().to(DEV))       # backward re-enters the forward's arithmetic mode
    torch.cuda.synchronize()
    e = (rel(yd.permute(0, 3, 1, 2), y), rel(xd.grad.permute(0, 3, 1, 2), x.grad), rel(wd.grad, w.grad))
    print("conv", cfg, "split" if split else "exact", "fwd %.2e dgrad %.2e wgrad %.2e" % e)
    assert max(e) < (1e-4 if split else 1e-5)


@pytest.mark.parametrize("cfg", [(3, 3, 32, 16, 7, 2, 3, 160, True), (2, 3, 9, 7, 7, 2, 3, 148, False), (2, 8, 6, 5, 3, 1, 1, 72, False),
                                 (1, 5, 4, 4, 1, 1, 0, 8, True)])
def test_im2col_rows_matches_unfold(cfg):
    """agrl_im2col_rows (the stem conv as a pointwise layer over pixel-major patches) against F.unfold: bitwise."""
    from torchreid import hip_ops
    N, C, H, W, R, stride, pad, ld, nchw = cfg
    g = torch.Generator().manual_seed(sum(cfg[:8]))
    x = torch.randn((N, C, H, W), generator=g)
    ref = F.unfold(x, R, padding=pad, stride=stride)                                   # (N, C*R*R, L), rows (c, r, s)
    L = ref.shape[-1]
    ref = ref.view(N, C, R * R, L).permute(0, 3, 2, 1).reshape(N * L, R * R * C)        # pixel-major, columns (r, s, c)
    xd = x.to(DEV) if nchw else x.permute(0, 2, 3, 1).contiguous().to(DEV)
    P, OH, OW = hip_ops.im2col_rows(xd, R, R, stride, pad, ld, nchw=nchw)
    assert OH * OW == L and tuple(P.shape) == (N * L, ld)
    assert torch.equal(P[:, :R * R * C].cpu(), ref) and (P[:, R * R * C:] == 0).all()


@pytest.mark.parametrize("cfg", [(3, 7, 5, 36, 20, 3, 1, 1), (2, 6, 4, 8, 12, 1, 1, 0), (5, 9, 6, 68, 132, 3, 2, 1), (1, 4, 4, 4, 4, 5, 1, 2),
                                 (70, 8, 4, 192, 320, 1, 2, 0)])
def test_conv_wgrad_ragged_shapes(cfg):
    """agrl_conv_wgrad on shapes that fill no tile: channel counts that are multiples of 4 only, pixel counts that are not
    multiples of the 32-pixel k-tile, frames smaller than the filter, more slices than k-tiles -- against autograd on the CPU."""
    from torchreid import hip_ops
    N, H, W, Cin, Cout, R, stride, pad = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.zeros((Cout, Cin, R, R), requires_grad=True)
    y = F.conv2d(x, w, stride=stride, padding=pad)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    for split in (False, True):
        with hip_ops.f32_split(split):
            dw = hip_ops.conv_wgrad(x.permute(0, 2, 3, 1).contiguous().to(DEV), dy.permute(0, 2, 3, 1).contiguous().to(DEV), w.shape, stride, pad)
            dw2 = hip_ops.conv_wgrad(x.permute(0, 2, 3, 1).contiguous().to(DEV), dy.permute(0, 2, 3, 1).contiguous().to(DEV), w.shape, stride, pad)
        e = rel(dw, w.grad)
        print("wgrad", cfg, "split" if split else "exact", "%.2e" % e)
        assert e < (1e-4 if split else 1e-5)
        assert torch.equal(dw, dw2), "the slice reduce runs in a fixed order: two runs must agree bitwise"


@pytest.mark.parametrize("cfg", [(40, 16, 8, 512, 256, 1, 1, 0), (3, 9, 5, 64, 128, 3, 2, 1), (2, 64, 32, 64, 64, 3, 1, 1), (256, 16, 8, 256, 1024, 1, 1, 0),
                                 (5, 7, 3, 32, 36, 1, 1, 0)])
def test_conv_epilogue_statistics(cfg):
    """agrl_conv2d_stats: the conv output equals agrl_conv2d_bn_act's bitwise, and the batch statistics that come out of its
    epilogue (per-tile fp32 sums, reduced in double) match a float64 reduction of that output -- 64- and 128-row tiles, ragged
    pixel counts, channel counts that do not fill a tile."""
    from torchreid import hip_ops
    N, H, W, Cin, Cout, R, stride, pad = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x = torch.randn((N, H, W, Cin), generator=g).to(DEV)
    w = (torch.randn((Cout, R, R, Cin), generator=g) / np.sqrt(Cin * R * R)).to(DEV)
    for split in (False, True):
        with hip_ops.f32_split(split):
            y, mean, var = hip_ops.conv_stats(x, w, stride, pad)
            y_ref = hip_ops.conv_bn_act(x, w, None, stride, pad, False)
        assert torch.equal(y, y_ref)
        y64 = y.double().view(-1, Cout)
        e_m = ((mean.double() - y64.mean(0)).abs().max() / y64.std(0).mean()).item()
        e_v = ((var.double() - y64.var(0, unbiased=False)).abs() / y64.var(0, unbiased=False)).max().item()
        print("conv stats", cfg, "split" if split else "exact", "mean %.1e var %.1e" % (e_m, e_v))
        assert e_m < 1e-6 and e_v < 1e-5


@pytest.mark.parametrize("cfg", [(4, 16, 8, 64, True, True), (3, 9, 5, 128, False, True), (6, 4, 2, 256, True, False), (2, 64, 32, 64, False, False)])
def test_batchnorm_act_forward_backward(cfg):
    """HipBatchNormAct (batch statistics, shortcut add, ReLU) and the running-statistics update against nn.BatchNorm2d in
    train mode + autograd on the CPU."""
    from torchreid.models._train_hip import _bn_act
    N, H, W, C, use_res, relu = cfg
    g = torch.Generator().manual_seed(N + H + C)
    y = (2.0 * torch.randn((N, C, H, W), generator=g) + 0.5).requires_grad_(True)
    res = torch.randn((N, C, H, W), generator=g).requires_grad_(True) if use_res else None
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(C, generator=g))
        bn.bias.copy_(0.2 * torch.randn(C, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(C, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    import copy
    bnd = copy.deepcopy(bn).to(DEV)
    bn.train()
    bnd.train()
    out = bn(y)
    if use_res:
        out = out + res
    if relu:
        out = F.relu(out)
    dout = torch.randn(out.shape, generator=g)
    out.backward(dout)
    nh = lambda t: t.detach().permute(0, 2, 3, 1).contiguous().to(DEV)
    yd = nh(y).requires_grad_(True)
    rd = nh(res).requires_grad_(True) if use_res else None
    outd = _bn_act(bnd, yd, rd, relu)
    outd.backward(nh(dout))
    torch.cuda.synchronize()
    errs = {"out": rel(outd.permute(0, 3, 1, 2), out), "dy": rel(yd.grad.permute(0, 3, 1, 2), y.grad),
            "dgamma": rel(bnd.weight.grad, bn.weight.grad), "dbeta": rel(bnd.bias.grad, bn.bias.grad),
            "running_mean": rel(bnd.running_mean, bn.running_mean), "running_var": rel(bnd.running_var, bn.running_var)}
    if use_res:
        errs["dres"] = rel(rd.grad.permute(0, 3, 1, 2), res.grad)
    print("bn", cfg, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert max(errs.values()) < 2e-5 and int(bnd.num_batches_tracked) == 1


def test_maxpool_forward_backward():
    from torchreid.models._train_hip import HipMaxPool
    g = torch.Generator().manual_seed(5)
    for shape in ((3, 64, 16, 8), (2, 32, 9, 7), (1, 8, 128, 64)):
        x = torch.randn(shape, generator=g).relu().requires_grad_(True)   # post-ReLU maps: ties at zero are part of the case
        y = F.max_pool2d(x, 3, 2, 1)
        dy = torch.randn(y.shape, generator=g)
        y.backward(dy)
        xd = x.detach().permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
        yd = HipMaxPool.apply(xd)
        yd.backward(dy.permute(0, 2, 3, 1).contiguous().to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(yd.permute(0, 3, 1, 2).cpu(), y)
        # gradients may only differ where a window holds several equal maxima (zeros): compare where the input is positive
        pos = x.detach() > 0
        assert torch.equal(xd.grad.permute(0, 3, 1, 2).cpu()[pos], x.grad[pos])
        assert abs(xd.grad.sum().item() - x.grad.sum().item()) < 1e-3


def test_tail_nodes_forward_backward():
    """The tail's autograd nodes one by one against torch autograd on the CPU: part / global pooling, Linear (classifier
    widths 5 and 702 included), G h, attention temporal pooling, label-smoothed cross entropy, the residual mix."""
    from torchreid.models import _train_hip as T
    from torchreid import losses
    g = torch.Generator().manual_seed(11)
    # pooling: (F, h, w, C) NHWC maps, S = 4 frames per tracklet
    F_, S, h, w, C = 8, 4, 16, 8, 64
    x1 = torch.randn((F_, C, h, w), generator=g, requires_grad=True)
    x2 = torch.randn((F_, C, h, w), generator=g, requires_grad=True)
    B = F_ // S
    g_ref = x1.view(B, S, C, h * w).permute(0, 2, 1, 3).reshape(B, C, -1).mean(2)
    parts = [torch.nn.functional.adaptive_avg_pool2d(x2, (n, 1)).view(F_, C, n) for n in (4, 2, 1)]
    n_ref = torch.cat(parts, dim=2).transpose(1, 2)                                   # (F, P, C)
    wg, wn = torch.randn(g_ref.shape, generator=g), torch.randn(n_ref.shape, generator=g)
    ((g_ref * wg).sum() + (n_ref * wn).sum()).backward()
    d1 = x1.detach().permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    d2 = x2.detach().permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    g_dev, n_dev = T.HipPartPool.apply(d1, d2, S, (4, 2, 1))
    ((g_dev * wg.to(DEV)).sum() + (n_dev * wn.to(DEV)).sum()).backward()
    e = [rel(g_dev, g_ref), rel(n_dev, n_ref), rel(d1.grad.permute(0, 3, 1, 2), x1.grad), rel(d2.grad.permute(0, 3, 1, 2), x2.grad)]
    print("part pool fwd %.1e %.1e bwd %.1e %.1e" % tuple(e))
    assert max(e) < 1e-5
    # Linear
    for M, K, N in ((16, 2048, 702), (8, 2048, 5), (224, 256, 256)):
        x = torch.randn((M, K), generator=g, requires_grad=True)
        wt = (torch.randn((N, K), generator=g) / K ** 0.5).requires_grad_(True)
        y = x @ wt.t()
        dy = torch.randn(y.shape, generator=g)
        y.backward(dy)
        xd, wd = x.detach().to(DEV).requires_grad_(True), wt.detach().to(DEV).requires_grad_(True)
        yd = T.linear_train(xd, wd)
        yd.backward(dy.to(DEV))
        e = [rel(yd, y), rel(xd.grad, x.grad), rel(wd.grad, wt.grad)]
        print("linear", (M, K, N), "fwd %.1e dx %.1e dw %.1e" % tuple(e))
        assert max(e) < 1e-5
    # G h
    Bq, V, Cq = 3, 28, 256
    G = torch.rand((Bq, V, V), generator=g).requires_grad_(True)
    hh = torch.randn((Bq, V, Cq), generator=g, requires_grad=True)
    m = torch.bmm(G, hh)
    dm = torch.randn(m.shape, generator=g)
    m.backward(dm)
    Gd, hd = G.detach().to(DEV).requires_grad_(True), hh.detach().to(DEV).requires_grad_(True)
    md = T.HipGraphBmm.apply(Gd, hd)
    md.backward(dm.to(DEV))
    e = [rel(md, m), rel(Gd.grad, G.grad), rel(hd.grad, hh.grad)]
    print("graph bmm fwd %.1e dG %.1e dh %.1e" % tuple(e))
    assert max(e) < 1e-5
    # attention pooling (one all-zero node: its norm passes no gradient)
    nodes = torch.rand((3, 6, 7, 128), generator=g)
    nodes[1, 2, 3] = 0
    nodes.requires_grad_(True)
    att = torch.nn.functional.normalize(nodes.norm(p=2, dim=3, keepdim=True), p=1, dim=1)
    a_ref = (nodes * att).sum(1).mean(1)
    da = torch.randn(a_ref.shape, generator=g)
    a_ref.backward(da)
    nd = nodes.detach().to(DEV).requires_grad_(True)
    a_dev = T.HipAttnPool.apply(nd)
    a_dev.backward(da.to(DEV))
    e = [rel(a_dev, a_ref), rel(nd.grad, nodes.grad)]
    print("attention pool fwd %.1e bwd %.1e" % tuple(e))
    assert max(e) < 1e-5
    # label-smoothed cross entropy (reference arithmetic = this build's CPU path, pinned in tests/test_boundary.py)
    for n, K in ((16, 702), (4, 5)):
        z = (3 * torch.randn((n, K), generator=g)).requires_grad_(True)
        y = torch.randint(0, K, (n,), generator=g)
        l_ref = losses.CrossEntropyLabelSmooth(K, use_gpu=False)(z, y)
        (2.5 * l_ref).backward()
        zd = z.detach().to(DEV).requires_grad_(True)
        l_dev = losses.CrossEntropyLabelSmooth(K, use_gpu=True)(zd, y.to(DEV))
        (2.5 * l_dev).backward()
        assert abs(l_dev.item() - l_ref.item()) < 1e-5 * abs(l_ref.item()) and rel(zd.grad, z.grad) < 1e-5
    # residual mix
    a_, b_ = torch.randn((5, 7, 64), generator=g, requires_grad=True), torch.randn((5, 7, 64), generator=g, requires_grad=True)
    (0.9 * a_ + 0.1 * b_).backward(torch.ones(5, 7, 64))
    ad, bd = a_.detach().to(DEV).requires_grad_(True), b_.detach().to(DEV).requires_grad_(True)
    od = T.HipAxpby.apply(ad, bd, 0.9, 0.1)
    od.backward(torch.ones(5, 7, 64, device=DEV))
    assert rel(od, 0.9 * a_ + 0.1 * b_) < 1e-6 and rel(ad.grad, a_.grad) < 1e-6 and rel(bd.grad, b_.grad) < 1e-6


@pytest.mark.parametrize("cfg", [(3, 56, 256, True, True), (2, 112, 2048, True, True), (2, 28, 512, False, True)])
def test_graph_matrix_gradient_against_float64_autograd(cfg):
    """d loss / d f through the adaptive graph (sim -> row-L1 normalise -> mix): the native backward (agrl_graph_matrix_backward:
    M with d f = M f) against torch autograd of the reference formula in FLOAT64 -- in fp32 the reference's own gradient through
    the diagonal d2_ii (pure cancellation noise under a sqrt) is noise; exact arithmetic passes no gradient there, which is
    what the kernel implements."""
    from torchreid.models import _train_hip as T
    from recipe import synthetic_adj
    B, V, C, use_pose, learn_graph = cfg
    g = torch.Generator().manual_seed(V + C)
    f = torch.rand((B, 1, C), generator=g) * 0.2 + 0.05 * torch.randn((B, V, C), generator=g)
    adj = synthetic_adj(B, V // 7, seed=V)
    f64 = f.double().requires_grad_(True)
    G_ref = O.graph_matrix(f64, adj.double(), use_pose, learn_graph)
    wG = torch.randn(G_ref.shape, generator=g)
    (G_ref * wG.double()).sum().backward()
    fd = f.to(DEV).requires_grad_(True)
    G_dev = T.HipGraphMatrix.apply(fd, adj.to(DEV), use_pose, learn_graph, False)
    (G_dev * wG.to(DEV)).sum().backward()
    e_g, e_f = rel(G_dev, G_ref), rel(fd.grad, f64.grad)
    print("graph matrix", cfg, "G %.1e df %.1e (|df|max %.2e)" % (e_g, e_f, f64.grad.abs().max().item()))
    assert e_g < 1e-4 and e_f < 2e-3


@pytest.mark.parametrize("cfg", [(3, 56, 256), (2, 112, 2048)])
def test_graph_layer_train_forward_backward(cfg):
    """A whole GraphLayer in train mode (Linear, adaptive graph, G h, BatchNorm1d with batch statistics, LeakyReLU, residual
    mix) through the native nodes against the module in float64 on the CPU: output, input gradient, parameter gradients."""
    import copy
    from torchreid.models.vmgn import GraphLayer
    from torchreid.models import _train_hip as T
    from recipe import synthetic_adj
    B, V, C = cfg
    g = torch.Generator().manual_seed(B * V + C)
    layer = GraphLayer(C, C)
    with torch.no_grad():
        layer.linear.weight.copy_(torch.randn((C, C), generator=g) * 0.02)
        layer.bn.weight.copy_(0.5 + torch.rand(C, generator=g))
        layer.bn.bias.copy_(0.1 * torch.randn(C, generator=g))
    dev = copy.deepcopy(layer).to(DEV).train()
    ref = copy.deepcopy(layer).double().train()
    f = torch.rand((B, 1, C), generator=g) * 0.2 + 0.05 * torch.randn((B, V, C), generator=g)
    adj = synthetic_adj(B, V // 7, seed=V)
    f64 = f.double().requires_grad_(True)
    out = ref(f64, adj.double())
    dout = torch.randn(out.shape, generator=g)
    out.backward(dout.double())
    fd = f.to(DEV).requires_grad_(True)
    outd = T.graph_layer_train(dev, fd, adj.to(DEV))
    outd.backward(dout.to(DEV))
    errs = {"out": rel(outd, out), "df": rel(fd.grad, f64.grad), "dW": rel(dev.linear.weight.grad, ref.linear.weight.grad),
            "dgamma": rel(dev.bn.weight.grad, ref.bn.weight.grad), "dbeta": rel(dev.bn.bias.grad, ref.bn.bias.grad),
            "running_var": rel(dev.bn.running_var, ref.bn.running_var)}
    print("graph layer train", cfg, " ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) < 2e-3 and errs["out"] < 1e-5


def _problem(S, H, W, P=2, K=2, ncls=5, seed=3, consistent=True):
    from recipe import recipe_state_dict, synthetic_adj, synthetic_clips
    from torchreid import models
    kw = dict(num_classes=ncls, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1, pyramid_part=True,
              use_pose=True, learn_graph=True, consistent_loss=consistent)
    ref = models.init_model("vmgn", **kw)
    sd = recipe_state_dict(ref.state_dict(), seed=seed)
    ref.load_state_dict(sd)
    dev = models.init_model("vmgn", **kw)
    dev.load_state_dict(sd)
    pids = torch.arange(P).repeat_interleave(K)
    x = synthetic_clips(P * K, S, H=H, W=W, seed=9, identities=pids.tolist())
    adj = synthetic_adj(P * K, S, seed=9)
    return ref, dev.to(DEV), x, adj, pids, ncls


def _step(model, x, adj, y, use_gpu):
    from torchreid import losses
    ce = losses.CrossEntropyLabelSmooth(num_classes=5, use_gpu=use_gpu)
    htri = losses.TripletLoss(margin=0.3, soft=True)
    model.train()
    torch.manual_seed(1234)  # the consistent loss draws its frame subsets with torch.randperm on the host
    outs, feats = model(x, adj)
    loss = losses.DeepSupervision(ce, outs, y) + losses.DeepSupervision(htri, feats, y)
    model.zero_grad()
    loss.backward()
    return loss


@pytest.mark.parametrize("cfg", [(6, 16, 8, 256, 64, 1, False), (6, 16, 8, 128, 64, 1, True), (4, 32, 16, 128, 64, 2, True)])
def test_one_bottleneck_forward_backward(cfg):
    """One Bottleneck (vmgn.py:45-65) in train mode through the native nodes -- three convs, four BatchNorms with batch
    statistics, shortcut (identity / 1x1 downsample, stride 1 / 2), ReLUs -- against the stock module on the CPU: output, input
    gradient and every parameter gradient at 1e-4 (a single block is still well conditioned; fifty of them are not, see below)."""
    import copy
    from torchreid.models.vmgn import Bottleneck
    from torchreid.models._train_hip import bottleneck_train
    N, H, W, inplanes, planes, stride, ds = cfg
    g = torch.Generator().manual_seed(sum(cfg[:5]))
    down = None
    if ds:
        down = torch.nn.Sequential(torch.nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(planes * 4))
    blk = Bottleneck(inplanes, planes, stride, down)
    with torch.no_grad():
        for p_ in blk.parameters():
            p_.copy_(torch.randn(p_.shape, generator=g) * (0.3 if p_.dim() == 1 else (2.0 / p_[0].numel()) ** 0.5) + (1.0 if p_.dim() == 1 else 0.0))
    dev = copy.deepcopy(blk).to(DEV)
    blk.train()
    dev.train()
    x = torch.randn((N, inplanes, H, W), generator=g).relu().requires_grad_(True)
    out = blk(x)
    dout = torch.randn(out.shape, generator=g)
    out.backward(dout)
    xd = x.detach().permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    outd = bottleneck_train(dev, xd)
    outd.backward(dout.permute(0, 2, 3, 1).contiguous().to(DEV))
    torch.cuda.synchronize()
    gref = dict(blk.named_parameters())
    errs = {k: rel(p_.grad, gref[k].grad) for k, p_ in dev.named_parameters()}
    e_out, e_dx = rel(outd.permute(0, 3, 1, 2), out), rel(xd.grad.permute(0, 3, 1, 2), x.grad)
    worst = max(errs, key=errs.get)
    print("bottleneck", cfg, "out %.2e dx %.2e worst parameter gradient %.2e (%s)" % (e_out, e_dx, errs[worst], worst))
    assert e_out < 1e-5 and e_dx < 1e-4 and errs[worst] < 1e-4


@pytest.mark.parametrize("shape", [(6, 64, 32), (16, 256, 128)])
def test_trunk_backward_at_the_fp32_noise_floor(shape):
    """The native trunk in isolation: featuremaps in train mode and every trunk parameter's gradient for a fixed smooth
    functional of the two layer-4 maps. Fifty conv + batch-statistics-BatchNorm layers make these gradients sums of large
    cancelling terms (a conv weight followed by BatchNorm has no gradient along its own direction), so in fp32 they carry
    percent-level noise whatever computes them: the stock module tree on the CPU is 1e-2 (median) / 1e-1 (worst) away from the
    same computation in float64, stock torch on the GPU likewise. Asserted: the feature maps agree with
    float64 like the CPU's do, and the native gradients' error distribution against float64 is within 3 x the CPU fp32's."""
    import copy
    from torchreid.models._train_hip import featuremaps_train
    S, H, W = shape
    ref, dev, x, adj, pids, _ = _problem(S, H, W)
    frames = x.view(-1, 3, H, W)
    g = torch.Generator().manual_seed(17)
    ref64 = copy.deepcopy(ref).double()
    for m in (ref, dev, ref64):
        m.train()
    a1, a2 = ref.featuremaps(frames)
    w1, w2 = torch.randn(a1.shape, generator=g), torch.randn(a2.shape, generator=g)

    def functional(p, q):
        return ((p * w1.to(p.device, p.dtype)).sum() + (q * q * w2.to(p.device, p.dtype)).sum()) / p.numel()
    functional(a1, a2).backward()
    c1, c2 = ref64.featuremaps(frames.double())
    functional(c1, c2).backward()
    b1, b2 = featuremaps_train(dev, frames.to(DEV))
    functional(b1, b2).backward()
    torch.cuda.synchronize()
    g64 = {k: p.grad for k, p in ref64.named_parameters() if p.grad is not None}

    def dist(model):
        r = sorted(rel(p.grad, g64[k]) for k, p in model.named_parameters() if k in g64)
        return r[len(r) // 2], r[(9 * len(r)) // 10], r[-1]
    d_cpu, d_dev = dist(ref), dist(dev)
    e_cpu, e_dev = max(rel(a1, c1), rel(a2, c2)), max(rel(b1, c1), rel(b2, c2))
    bref = dict(ref.named_buffers())
    bworst = max(rel(b, bref[k]) for k, b in dev.named_buffers() if b.dtype.is_floating_point)
    print("trunk S=%d %dx%d vs float64: maps cpu %.2e native %.2e | gradients (median, p90, worst) cpu fp32 %.2e %.2e %.2e, native %.2e %.2e %.2e"
          " | running stats vs cpu %.2e" % ((S, H, W, e_cpu, e_dev) + d_cpu + d_dev + (bworst,)))
    assert len(g64) == 189 and all(p.grad is None for k, p in dev.named_parameters() if k not in g64)
    assert e_dev < 3 * e_cpu + 1e-6 and bworst < 1e-4
    for a_, b_ in zip(d_dev, d_cpu):
        assert a_ < 3 * b_ + 1e-6


@pytest.mark.parametrize("shape", [(6, 64, 32), (16, 256, 128)])
def test_train_step_loss_and_gradients_at_the_reference_noise_floor(shape):
    """One xent + htri step (consistent loss on) with the native trunk, at a small size and at BASELINE config 4's clip shape
    (seq_len 16, V = 112, 256 x 128 frames). The loss matches the CPU step to 1e-5. The per-parameter GRADIENTS of this
    model are ill-conditioned in fp32 whatever computes them: GraphLayer.get_sim_matrix takes sqrt(clamp(d2, 1e-12)) of a
    diagonal d2_ii that is pure cancellation noise (vmgn.py:114-120), and the gradient of sqrt at ~1e-4 amplifies that
    noise -- the reference's own CPU fp32 step is 1-5 % away from the same step in float64, and so is stock torch on the
    GPU. Parity is therefore asserted at that floor: against the float64 CPU step the native step's
    error distribution (median, 90th percentile, worst) must be within 3 x the CPU fp32 step's own."""
    import copy
    S, H, W = shape
    ref, dev, x, adj, pids, _ = _problem(S, H, W)
    assert dev.hip_train
    ref64 = copy.deepcopy(ref).double()
    l64 = _step(ref64, x.double(), adj.double(), pids, False)
    l_ref = _step(ref, x, adj, pids, False)
    l_dev = _step(dev, x.to(DEV), adj.to(DEV), pids.to(DEV), True)
    torch.cuda.synchronize()
    assert abs(l_ref.item() - l_dev.item()) < 1e-5 * abs(l_ref.item()) and abs(l64.item() - l_dev.item()) < 1e-5 * abs(l64.item())
    g64 = {k: p.grad for k, p in ref64.named_parameters() if p.grad is not None}

    def dist(model):
        r = sorted(rel(p.grad, g64[k]) for k, p in model.named_parameters() if k in g64)
        return r[len(r) // 2], r[(9 * len(r)) // 10], r[-1]
    d_cpu, d_dev = dist(ref), dist(dev)
    assert all(p.grad is None for k, p in dev.named_parameters() if k not in g64)
    print("train step S=%d %dx%d: loss fp64 %.7f cpu %.7f native %.7f | grad err vs fp64 (median, p90, worst): cpu fp32 %.2e %.2e %.2e, "
          "native %.2e %.2e %.2e" % ((S, H, W, l64.item(), l_ref.item(), l_dev.item()) + d_cpu + d_dev))
    for a_, b_ in zip(d_dev, d_cpu):
        assert a_ < 3 * b_ + 1e-6


def test_native_step_is_what_runs(monkeypatch):
    """The train forward on CUDA goes through the C-ABI (conv, batch-norm statistics, max pooling entry points are called),
    and AGRL_HIP_TRAIN=0 style opt-out (model.hip_train = False) gives the same loss through the stock module tree."""
    from torchreid import _hip
    ref, dev, x, adj, pids, _ = _problem(6, 64, 32, consistent=True)
    _hip.PROFILE = []
    l1 = _step(dev, x.to(DEV), adj.to(DEV), pids.to(DEV), True)
    names = {r[0] for r in _hip.PROFILE}
    _hip.PROFILE = None
    assert {"agrl_conv2d_bn_act", "agrl_bn_stats", "agrl_bn_apply", "agrl_bn_backward", "agrl_im2col_t", "agrl_gemm_nt_splitk",
            "agrl_maxpool3x3s2", "agrl_maxpool3x3s2_backward", "agrl_linear_nobias", "agrl_part_pool", "agrl_part_pool_backward",
            "agrl_graph_gram", "agrl_graph_finalize", "agrl_graph_propagate", "agrl_graph_matrix_backward", "agrl_row_sqnorm",
            "agrl_attn_pool_bnneck", "agrl_attn_pool_backward", "agrl_axpby", "agrl_xent_label_smooth", "agrl_triplet_loss"} <= names
    # ... and no stock-torch arithmetic kernel is left between the input frames and the loss: the autograd graph of the loss
    # consists of the native nodes plus views / gathers / the scalar sums of DeepSupervision
    native = ("HipConv2d", "HipConv2dStats", "HipConvFork", "HipBatchNormAct", "HipMaxPool", "HipPartPool", "HipGraphMatrix", "HipGraphBmm", "HipAxpby",
              "HipAttnPool", "HipXent", "_NativeTriplet")
    plumbing = ("View", "Reshape", "Permute", "Transpose", "Gather", "Add", "Div", "Mul", "AccumulateGrad", "Alias", "Unsafe", "Expand",
                "Squeeze", "Unsqueeze", "Clone", "T", "Select", "Slice", "Copy", "Constant", "AsStrided", "Repeat", "ToCopy", "Contiguous")
    seen, stack, foreign = set(), [l1.grad_fn], set()
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        name = type(fn).__name__
        if not (any(name.startswith(n) for n in native) or any(p_ in name for p_ in plumbing)):
            foreign.add(name)
        stack.extend(nf for nf, _ in fn.next_functions)
    assert not foreign, foreign
    dev.hip_train = False
    l2 = _step(dev, x.to(DEV), adj.to(DEV), pids.to(DEV), True)
    assert abs(l1.item() - l2.item()) < 1e-4 * abs(l2.item())


def test_native_step_against_reference_gradients():
    """The native step against gradients the REFERENCE ITSELF produced (tests/golden/vmgn_backward_b4s8.npz: its own model,
    loss.backward() of xent + htri with the consistent loss, B = 4, S = 8; train_vidreid_xent_htri.py:397-411). Loss to 1e-5;
    per named parameter the stored gradient slice (relative L2 error) and the norm of the whole gradient tensor. The bars are
    the measured errors (slices 1.4-2.9e-2 in the trunk, 1e-4 in the heads; norms <= 4.6e-3) with a 2-3 x margin: the step is
    fifty conv + batch-statistics-BatchNorm layers deep and a different (equally valid) fp32 summation order moves the trunk's
    gradients by ~1.5e-2 -- the distance at which the same step on the CPU in fp32 sits from its own float64 evaluation
    (test_train_step_loss_and_gradients_at_the_reference_noise_floor). This build's CPU module tree, which sums in the
    reference's own order, reproduces the fixture to 1.3e-5 (tests/test_oracle_golden.py)."""
    from test_oracle_golden import backward_case, gradient_errors
    z, m, loss, lx, lt = backward_case(DEV)
    torch.cuda.synchronize()
    for got, key in ((loss, "loss"), (lx, "xent"), (lt, "htri")):
        assert abs(float(got.detach()) - float(z[key])) < 1e-5 * abs(float(z[key])), key
    errs = gradient_errors(z, m)
    for key, (e_slice, e_norm, e_l2) in errs.items():
        print("%-34s slice max %.2e L2 %.2e | tensor norm %.2e" % (key, e_slice, e_l2, e_norm))
    for key, (e_slice, e_norm, e_l2) in errs.items():
        assert e_l2 < 6e-2 and e_norm < 1.5e-2, (key, e_slice, e_norm, e_l2)   # measured: <= 2.9e-2 / 4.6e-3


def test_xent_native_matches_reference_fixture_and_flags_bad_labels():
    """agrl_xent_label_smooth (value + logit gradient in one call) against the reference's CrossEntropyLabelSmooth +
    DeepSupervision (tests/golden/xent.npz: losses/cross_entropy_loss.py:26-37, losses/__init__.py:9-20), and a label outside
    [0, K): NaN loss, NaN gradient row, every other row untouched, no out-of-bounds read."""
    from test_oracle_golden import xent_case
    from torchreid import hip_ops as ops, losses
    z, logits, pids, K = xent_case()
    for eps in (0.1, 0.0, 0.3):
        tag = "eps%02d" % int(round(eps * 100))
        xs = [x.clone().to(DEV).requires_grad_(True) for x in logits]
        crit = losses.CrossEntropyLabelSmooth(num_classes=K, epsilon=eps, use_gpu=True)
        loss = losses.DeepSupervision(crit, xs, pids.to(DEV))
        loss.backward()
        assert abs(float(loss.detach()) - float(z["loss_" + tag])) < 1e-6 * abs(float(z["loss_" + tag]))
        assert abs(float(crit(xs[0].detach(), pids.to(DEV))) - float(z["single_" + tag])) < 1e-6 * abs(float(z["single_" + tag]))
        assert rel(xs[0].grad, torch.from_numpy(z["grad0_" + tag])) < 1e-5
    x = logits[0].to(DEV)
    for bad in (-1, K, K + 1000000):
        y = pids.clone()
        y[3] = bad
        loss, dl = ops.xent_label_smooth(x, y.to(torch.int32).to(DEV), 0.1)
        torch.cuda.synchronize()
        assert torch.isnan(loss).all() and torch.isnan(dl[3]).all()
        keep = torch.ones(x.shape[0], dtype=torch.bool)
        keep[3] = False
        ref = O.xent_label_smooth(logits[0].clone().requires_grad_(True), pids, 0.1)
        xr = logits[0].clone().requires_grad_(True)
        O.xent_label_smooth(xr, pids, 0.1).backward()
        assert rel(dl[keep.to(DEV)], xr.grad[keep]) < 1e-5 and torch.isfinite(ref)


@pytest.mark.parametrize("consistent", [False, True])
def test_gsta_native_train_step_matches_cpu_module(consistent):
    """The sibling ``gsta`` (one layer4 branch, one BNNeck; reference gsta.py:273-322) in train mode: the native step (same
    autograd nodes as vmgn's) against the stock-torch module tree on the CPU -- outputs, loss, gradient norms -- incl. its
    consistent loss (one frame dropped per tracklet from numpy's global RNG)."""
    from recipe import recipe_state_dict, synthetic_adj, synthetic_clips
    from torchreid import losses, models
    kw = dict(num_classes=5, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1, pyramid_part=True,
              use_pose=True, learn_graph=True, consistent_loss=consistent, pretrained=False)
    ref = models.init_model("gsta", **kw)
    sd = recipe_state_dict(ref.state_dict(), seed=5)
    ref.load_state_dict(sd)
    dev = models.init_model("gsta", **kw)
    dev.load_state_dict(sd)
    dev = dev.to(DEV)
    pids = torch.tensor([0, 0, 1, 1])
    x, adj = synthetic_clips(4, 6, H=128, W=64, seed=17, identities=pids.tolist()), synthetic_adj(4, 6, seed=17)
    htri = losses.TripletLoss(margin=0.3, soft=True)

    def step(model, x_, adj_, y_, ce):
        model.train()
        np.random.seed(77)
        outs, feats = model(x_, adj_)
        outs, feats = (outs, feats) if isinstance(outs, (list, tuple)) else ([outs], [feats])
        loss = losses.DeepSupervision(ce, outs, y_) + losses.DeepSupervision(htri, feats, y_)
        loss.backward()
        grads = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}
        return loss.item(), [o.detach().double().cpu() for o in outs], grads

    l_ref, o_ref, g_ref = step(ref, x, adj, pids, losses.CrossEntropyLabelSmooth(num_classes=5, use_gpu=False))
    l_dev, o_dev, g_dev = step(dev, x.to(DEV), adj.to(DEV), pids.to(DEV), losses.CrossEntropyLabelSmooth(num_classes=5, use_gpu=True))
    assert len(o_ref) == len(o_dev) == (2 if consistent else 1) and set(g_ref) == set(g_dev)
    for a, b in zip(o_dev, o_ref):
        assert rel(a, b) < 1e-3
    assert abs(l_ref - l_dev) < 1e-4 * abs(l_ref)
    gn_ref = torch.sqrt(sum((g ** 2).sum() for g in g_ref.values())).item()
    gn_dev = torch.sqrt(sum((g ** 2).sum() for g in g_dev.values())).item()
    print("gsta train step (consistent=%s): loss cpu %.6f gpu %.6f | grad norm cpu %.4e gpu %.4e" % (consistent, l_ref, l_dev, gn_ref, gn_dev))
    assert abs(gn_ref - gn_dev) < 2e-2 * gn_ref
    for k in ("classifier.weight", "bottleneck.weight", "graph_layers.1.linear.weight"):
        assert rel(g_dev[k], g_ref[k]) < 5e-2, k
    # running statistics moved like nn.BatchNorm's
    for k in ("bn1.running_mean", "layer4.2.bn3.running_var", "bottleneck.running_mean", "bottleneck.num_batches_tracked"):
        a, b = dev.state_dict()[k].double().cpu(), ref.state_dict()[k].double()
        assert rel(a, b) < 1e-3 if b.abs().max() > 0 else torch.equal(a, b), k


@pytest.mark.parametrize("B,V,C", [(16, 112, 2048), (3, 28, 256), (2, 144, 128), (5, 7, 384)])
def test_graph_pair_product_is_the_bmm_gradient(B, V, C):
    """agrl_graph_pair_product = d loss / d G of msg = bmm(G, h) (vmgn.py:168): dmsg[b] h[b]^T per tracklet, against
    float64 and against autograd; and the autograd function routes through it."""
    from torchreid import hip_ops as ops
    from torchreid.models._train_hip import HipGraphBmm
    g = torch.Generator().manual_seed(B * 1000 + V)
    dmsg = torch.randn((B, V, C), generator=g)
    h = torch.randn((B, V, C), generator=g)
    G = torch.rand((B, V, V), generator=g)
    ref = torch.bmm(dmsg.double(), h.double().transpose(1, 2))
    out = ops.graph_pair_product(dmsg.to(DEV), h.to(DEV))
    err = ((out.double().cpu() - ref).abs().max() / ref.abs().max()).item()
    assert err < 2e-6, err
    Gd, hd = G.to(DEV).requires_grad_(True), h.to(DEV).requires_grad_(True)
    HipGraphBmm.apply(Gd, hd).backward(dmsg.to(DEV))
    Gc, hc = G.double().requires_grad_(True), h.double().requires_grad_(True)
    torch.bmm(Gc, hc).backward(dmsg.double())
    assert ((Gd.grad.double().cpu() - Gc.grad).abs().max() / Gc.grad.abs().max()).item() < 2e-6
    assert ((hd.grad.double().cpu() - hc.grad).abs().max() / hc.grad.abs().max()).item() < 2e-6
