"""The GraphLayer beyond one workgroup's LDS: the kernel forms that take over where a tracklet's V = parts x frames nodes no longer
fit (csrc/gcn.hip: tiled Gram / pair product, row-streaming finalize, chunked message pass, pose adjacency for S > 64 frames;
csrc/train_tail.hip: the graph matrix's backward from HBM), held to the same ELEMENTWISE float64 bounds as the resident forms
(tests/graph_ref.py, tests/train_ref.py through bounds.check_rounded), then a GraphLayer in train mode, whole models in eval and
one native train step at node counts the driver reaches with --num-split 8 --pyramid-part and --test-sample all.

Every kernel call runs inside poisoned_outputs() (outputs and workspaces NaN-filled between canary bands), twice, bitwise equal.
Inputs follow the generator of test_graph_matrix_backward_elementwise: a common positive vector + 5 % noise, so every
off-diagonal D2 is ~ 2 C 0.05^2, far above the clamp (asserted: no entry is excused). Shapes are the smallest that reach each
form: the first V past each limit (hip_ops.graph_forms), several tiles with a ragged edge, more than one chunk."""
import copy

import numpy as np
import pytest
import torch

import graph_ref as GR
import train_ref as R
from bounds import U32, check_rounded, n_acc_for
from lp16 import LP16, LP_DTYPE, LP_EMBED_TOL
from oracle import vmgn_oracle as O
from recipe import recipe_state_dict, synthetic_clips
from test_gpu_train_bounds import twice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
MODES = [(True, True, False), (True, False, False), (False, True, False), (True, True, True), (False, True, True), (True, False, True)]


def ops_():
    from torchreid import hip_ops
    return hip_ops


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / ref.abs().max()).item()


def features(B, V, C, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.rand((B, 1, C), generator=g) * 0.2 + 0.05 * torch.randn((B, V, C), generator=g)
    return f, g


def random_adj(B, V, g):
    """A random symmetric zero-diagonal {0, 1} graph; row 3 of tracklet 0 has no edge at all."""
    up = torch.triu((torch.rand((B, V, V), generator=g) > 0.5).float(), diagonal=1)
    adj = up + up.transpose(1, 2)
    adj[0, 3], adj[0, :, 3] = 0, 0
    return adj


def random_poses(B, S, H, rng):
    poses = np.stack([rng.rand(B, S, 18) * 128, rng.rand(B, S, 18) * (H + 8) - 4, rng.rand(B, S, 18) * 0.5], axis=-1).astype(np.float32)
    det = rng.rand(B, S) > 0.15
    return poses, det


def assert_all_live(gram, V):
    live = GR.similarity_chain(*GR.gram_from_partials(gram))["live"]
    assert bool(live[:, ~torch.eye(V, dtype=torch.bool)].all()), "every off-diagonal distance is far above the clamp in this case"


# ---- 1. the graph matrix ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,gram_form", [((2, 257, 256), "slices"), ((1, 305, 128), "tiled"), ((2, 520, 256), "tiled")],
                         ids=lambda s: "x".join(str(v) for v in s) if isinstance(s, tuple) else s)
def test_graph_matrix_elementwise(shape, gram_form):
    """Gram + finalize past V = 256: (2,257,256) the first V of the row-streaming finalize, still on the nz = 2 slice partials;
    (1,305,128) the first V of the tiled Gram; (2,520,256) nine tiles with a ragged edge. All three modes, with and without the
    masked diagonal, fp32 and bit-packed adjacency (bitwise equal). The tiled Gram against float64 (one chain over C: C / 4
    exact-fp32 MFMA steps), bit-symmetric; G's diagonal against the reference's."""
    ops = ops_()
    B, V, C = shape
    forms = ops.graph_forms(V, C)
    assert forms["finalize"] == "rows" and forms["gram"] == gram_form
    f, g = features(B, V, C, V + C)
    adj = random_adj(B, V, g)
    fd, adjd = f.to(DEV), adj.to(DEV)
    bits = ops.adjacency_pack_host(adj)
    assert torch.equal(twice(lambda: ops.adjacency_pack(adjd)), bits)
    gram = twice(lambda: ops.graph_gram(fd))
    f64 = f.double()
    if gram_form == "tiled":
        assert tuple(gram.shape) == (B, 1, V, V)
        n = n_acc_for(C, 4)
        check_rounded(gram[:, 0], f64 @ f64.transpose(1, 2), f64.abs() @ f64.abs().transpose(1, 2), n, F32, name="graph gram tiled|%dx%dx%d|n_acc=%d" % (B, V, C, n))
        assert torch.equal(gram, gram.transpose(2, 3)), "the tiled Gram is bit-symmetric"
    else:
        assert tuple(gram.shape) == (B, C // 128, V, V)
        s64 = f64.view(B, V, C // 128, 128).permute(0, 2, 1, 3)
        check_rounded(gram, s64 @ s64.transpose(2, 3), s64.abs() @ s64.abs().transpose(2, 3), 32 + 3, F32, name="graph gram|%dx%dx%d|n_acc=35" % shape)
    assert_all_live(gram, V)
    gram_d = gram.to(DEV)
    eye = torch.eye(V, dtype=torch.bool)
    for use_pose, learn_graph, mask_diag in MODES:
        tag = "%s pose=%d learn=%d mask=%d" % (shape, use_pose, learn_graph, mask_diag)
        G = twice(lambda: ops.graph_finalize(gram_d if learn_graph else None, adjd if use_pose else None, B, V, use_pose, learn_graph, mask_diag))
        exact, slack = GR.graph_matrix_ref(gram, adj, use_pose, learn_graph, mask_diag)
        over = slack > 128 * U32 * exact.abs()
        assert not bool(over.any()), "%s: the reference's own slack exceeds 128 u |G|" % tag
        check_rounded(G, exact, torch.zeros_like(exact), 0, F32, slack=slack, name="graph_matrix|rows|" + tag)
        if learn_graph:   # the diagonal on its own: D2_ii is exactly 0 on both sides, so S_ii carries no Gram error at all
            check_rounded(G[:, eye], exact[:, eye], torch.zeros_like(exact[:, eye]), 0, F32, slack=slack[:, eye], name="graph_matrix|rows diagonal|" + tag)
        if mask_diag:
            assert bool((G[:, eye] == 0).all())
        if use_pose:
            Gb = twice(lambda: ops.graph_matrix(fd, bits.to(DEV), use_pose, learn_graph, mask_diag=mask_diag))
            assert torch.equal(Gb, G), "packed adjacency: %d of %d elements differ" % (int((Gb != G).sum()), G.numel())
            assert torch.equal(twice(lambda: ops.graph_matrix(fd, adjd, use_pose, learn_graph, mask_diag=mask_diag)), G)
    assert bool((G[0, 3] == 0).all())      # pose only, masked: the all-zero adjacency row stays zero (0 / clamp)


# ---- 2. the message pass ---------------------------------------------------------------------------------------------------------
def message_operands(B, V, C, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((B, V, C), generator=g)
    h = torch.randn((B, V, C), generator=g) * R.channel_scales(C, seed + 1, -8, 2)
    G = torch.randn((B, V, V), generator=g) / V ** 0.5
    scale, shift = torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    return f, h, G, scale, shift


@pytest.mark.parametrize("shape,mixes", [((1, 1025, 128), [(0.9, 0.1), (1.0, 0.3), (0.0, 1.0)]), ((2, 2600, 256), [(0.9, 0.1)])],
                         ids=["1x1025x128", "2x2600x256"])
def test_graph_propagate_chunked_elementwise(shape, mixes):
    """agrl_graph_propagate past V = 1024: three chunks with a one-column tail (1025), six chunks and a ragged last row block
    (2600), a real BatchNorm and LeakyReLU(0.1), the fp32 and the 16-bit output, against graph_ref.message_ref(form='tiled')
    (one running accumulator, u ascending: chain V + 5). Then P = G f through the unit-BatchNorm route of graph_apply_operand and
    graph_apply."""
    ops = ops_()
    B, V, C = shape
    assert ops.graph_forms(V, C)["propagate"] == "chunked"
    f, h, G, scale, shift = message_operands(B, V, C, V * 7 + C)
    fd, hd, Gd, sd, shd = (t.to(DEV) for t in (f, h, G, scale, shift))
    for keep, gamma in mixes:
        exact, mag, n = GR.message_ref(f, h, G, scale, shift, keep, gamma, 0.1, "tiled")
        assert n == V + 5
        tag = "graph_propagate|chunked|%s keep=%g gamma=%g" % (shape, keep, gamma)
        out, out_lp = twice(lambda: ops.graph_propagate(fd, hd, Gd, sd, shd, gamma, 0.1, want_lp=True, keep=keep))
        out1, none = twice(lambda: ops.graph_propagate(fd, hd, Gd, sd, shd, gamma, 0.1, want_lp=False, keep=keep))
        assert none is None and torch.equal(out1, out)
        check_rounded(out, exact, mag, n, F32, name=tag)
        check_rounded(out_lp, exact, mag, n, LP_DTYPE, name=tag + " out_lp")
        check_rounded(out_lp, out.double(), torch.zeros_like(exact), 0, LP_DTYPE, min_exact_frac=1.0, name=tag + " out_lp = rounded out")
    if V == 1025:
        exact, mag, n = GR.apply_ref(G, f, V + 5)
        P = twice(lambda: ops.graph_apply_operand(Gd, fd, F32))
        Plp = twice(lambda: ops.graph_apply_operand(Gd, fd, LP_DTYPE))
        check_rounded(P, exact, mag, n, F32, name="graph_apply|chunked fp32|%s" % (shape,))
        check_rounded(Plp, exact, mag, n, LP_DTYPE, name="graph_apply|chunked lp16|%s" % (shape,))
        check_rounded(twice(lambda: ops.graph_apply(Gd, fd)), exact, mag, n, F32, name="graph_apply|chunked unit BatchNorm|%s" % (shape,))


# ---- 3. the backward of the graph matrix -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(116, True, False), (117, True, False), (120, False, False), (150, True, True), (260, False, False), (305, True, False)],
                         ids=lambda c: "V%d-pose%d-mask%d" % c)
def test_graph_matrix_backward_elementwise(cfg):
    """The backward on the Gram the forward produced, against train_ref.graph_matrix_backward_ref: V = 116 (the last V the
    LDS-resident kernel takes -- its message says 115, its LDS check admits 116), 117 (the first of the HBM form), 120 and 150
    (P = 15 at seq_len 8 and 10), 260 (two slice partials into the HBM form, five 64-wide tiles with a ragged edge), 305 (the
    tiled Gram's nz = 1)."""
    ops = ops_()
    V, use_pose, mask_diag = cfg
    B, C = 2, 256
    forms = ops.graph_forms(V, C)
    assert forms["backward"] == ("resident" if V <= 116 else "hbm") and forms["gram"] == ("tiled" if V > 304 else "slices")
    f, g = features(B, V, C, V + C)
    dG = torch.randn((B, V, V), generator=g)
    fd, dGd = f.to(DEV), dG.to(DEV)
    gram = twice(lambda: ops.graph_gram(fd))
    assert gram.shape[1] == (1 if V > 304 else C // 128)
    gd = gram.to(DEV)
    M = twice(lambda: ops.graph_matrix_backward(gd, dGd, use_pose, mask_diag))
    exact, slack, live = R.graph_matrix_backward_ref(gram, dG, use_pose, mask_diag)
    assert bool(live[:, ~torch.eye(V, dtype=torch.bool)].all()), "every off-diagonal distance is far above the clamp in this case"
    check_rounded(M, exact, torch.zeros_like(exact), 0, F32, slack=slack, name="graph matrix backward|2x%dx256 pose=%d mask=%d" % cfg)


# ---- 4. the pair product ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 145, 256), (3, 260, 128)], ids=lambda s: "%dx%dx%d" % s)
def test_graph_pair_product_tiled_elementwise(shape):
    """out[b] = a[b] b[b]^T past V = 144 against the float64 bmm: one chain over all C channels, C / 4 exact-fp32 MFMA steps
    (bounds.n_acc_for(C, 4)); asymmetric operands with per-channel scales."""
    ops = ops_()
    B, V, C = shape
    assert ops.graph_forms(V, C)["pair"] == "tiled"
    g = torch.Generator().manual_seed(B * 1000 + V)
    a_ = torch.randn((B, V, C), generator=g) * R.channel_scales(C, 3)
    b_ = torch.randn((B, V, C), generator=g)
    ad, bd = a_.to(DEV), b_.to(DEV)
    exact = torch.bmm(a_.double(), b_.double().transpose(1, 2))
    mag = torch.bmm(a_.double().abs(), b_.double().abs().transpose(1, 2))
    n = n_acc_for(C, 4)
    check_rounded(twice(lambda: ops.graph_pair_product(ad, bd)), exact, mag, n, F32, name="graph pair product tiled|%dx%dx%d|n_acc=%d" % (B, V, C, n))


def test_graph_bmm_backward_runs_the_pair_kernel():
    """HipGraphBmm.backward at V = 260, B = 3: d loss / d G comes from agrl_graph_pair_product (its tiled form) -- not from one GEMM
    over all (B V)^2 rows -- and both gradients match float64 autograd."""
    from torchreid import _hip
    from torchreid.models._train_hip import HipGraphBmm
    B, V, C = 3, 260, 128
    g = torch.Generator().manual_seed(B * 1000 + V)
    dmsg, h, G = torch.randn((B, V, C), generator=g), torch.randn((B, V, C), generator=g), torch.rand((B, V, V), generator=g)
    Gd, hd = G.to(DEV).requires_grad_(True), h.to(DEV).requires_grad_(True)
    msg = HipGraphBmm.apply(Gd, hd)
    _hip.PROFILE = []
    try:
        msg.backward(dmsg.to(DEV))
        names = [r[0] for r in _hip.PROFILE]
    finally:
        _hip.PROFILE = None
    assert "agrl_graph_pair_product" in names and "agrl_linear_nobias" not in names, names
    Gc, hc = G.double().requires_grad_(True), h.double().requires_grad_(True)
    torch.bmm(Gc, hc).backward(dmsg.double())
    assert rel(Gd.grad, Gc.grad) < 2e-6 and rel(hd.grad, hc.grad) < 2e-6


# ---- 5. the pose adjacency ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [65, 150])
@pytest.mark.parametrize("num_split", [4, 8])
def test_pose_adjacency_long_tracklets(S, num_split):
    """agrl_pose_adjacency past 64 frames (S = 65: the first; 150: several workgroups per tracklet) == the oracle's restatement
    of generate_graph + adj_graph on random poses with undetected frames; the bits form == adjacency_pack of the fp32 form."""
    ops = ops_()
    B, H = 2, 256
    poses, det = random_poses(B, S, H, np.random.RandomState(S + num_split))
    assert not det.all() and det.any()
    pd, dd = torch.from_numpy(poses).to(DEV), torch.from_numpy(det).to(DEV)
    adj = twice(lambda: ops.pose_adjacency(pd, dd, H, num_split, True))
    V = S * (2 * num_split - 1)
    assert tuple(adj.shape) == (B, V, V)
    for b in range(B):
        sets = [O.pose_part_sets(poses[b, t] if det[b, t] else None, H, num_split) for t in range(S)]
        assert np.array_equal(adj[b].numpy(), O.pose_adjacency(sets, num_split, True)), (S, num_split, b)
    bits = twice(lambda: ops.pose_adjacency(pd, dd, H, num_split, True, packed=True))
    assert bits.dtype == torch.int32 and tuple(bits.shape) == (B, V, (V + 31) // 32)
    assert torch.equal(bits, twice(lambda: ops.adjacency_pack(adj.to(DEV)))) and torch.equal(bits, ops.adjacency_pack_host(adj))


# ---- 6. a GraphLayer in train mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(2, 120, 256), (2, 260, 256)], ids=lambda c: "%dx%dx%d" % c)
def test_graph_layer_train_forward_backward(cfg):
    """A whole GraphLayer in train mode through the native nodes against the module in float64 on the CPU, at V = 120 (HBM
    backward) and V = 260 (row-streaming finalize, HBM backward, tiled pair product): the bounds of the V <= 112 test."""
    from torchreid.models.vmgn import GraphLayer
    from torchreid.models import _train_hip as T
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
    adj = random_adj(B, V, g)
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


# ---- 7. models in eval -------------------------------------------------------------------------------------------------------------
def device_adjacency(B, S, H, num_split, seed):
    poses, det = random_poses(B, S, H, np.random.RandomState(seed))
    return ops_().pose_adjacency(torch.from_numpy(poses).to(DEV), torch.from_numpy(det).to(DEV), H, num_split, True)


def build_model(name, **kw):
    from torchreid import models
    cfg = dict(num_classes=5, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1, pyramid_part=True, use_pose=True,
               learn_graph=True)
    cfg.update(kw)
    m = models.init_model(name, **cfg)
    m.load_state_dict(recipe_state_dict(m.state_dict(), seed=0))
    return m


@pytest.mark.parametrize("name", ["vmgn", "ganet"])
def test_models_eval_at_280_nodes(name):
    """One clip of 40 frames of 64 x 32 with num_split 4 + pyramid (V = 280: row-streaming finalize, tiled message pass), the
    adjacency built on the device: the native forward in fp32 mode and in the default 16-bit mode against the same weights on the
    CPU module tree in fp32, at the parity bar of tests/test_gpu_model.py."""
    B, S, H, W = 1, 40, 64, 32
    m = build_model(name, **(dict(knn=4, pretrained=False) if name == "ganet" else dict(consistent_loss=False)))
    if name == "ganet":
        for layer in m.graph_layers:
            layer.gamma = 0.1
    m.eval()
    x = synthetic_clips(B, S, H=H, W=W, seed=S)
    adj = device_adjacency(B, S, H, 4, seed=S)
    assert adj.shape[1] == 280 and ops_().graph_forms(280, 2048)["finalize"] == "rows"
    with torch.no_grad():
        ref = m(x, adj.cpu())
    dev = copy.deepcopy(m).to(DEV)
    for precision, tol in (("fp32", 1e-3), (LP16, LP_EMBED_TOL)):
        dev.hip_precision = precision
        got = dev(x.to(DEV), adj)
        torch.cuda.synchronize()
        e = rel(got, ref)
        print(name, precision, "V=280 max rel err vs the CPU module tree %.3e" % e)
        assert got.shape == ref.shape and bool(torch.isfinite(got).all()) and e < tol


def test_whole_tracklet_item_through_extract_features():
    """One --test-sample all item: the whole 70-frame tracklet as one clip (V = 490), adjacency from ops.pose_adjacency, through
    evaluation.extract_features against the CPU module tree."""
    from torchreid import evaluation
    B, S, H, W = 1, 70, 64, 32
    m = build_model("vmgn", consistent_loss=False).eval()
    x = synthetic_clips(B, S, H=H, W=W, seed=S)
    adj = device_adjacency(B, S, H, 4, seed=S)
    assert adj.shape[1] == 490
    with torch.no_grad():
        ref = m(x, adj.cpu())
    dev = copy.deepcopy(m).to(DEV)
    dev.hip_precision = "fp32"
    feats, pids, camids = evaluation.extract_features(dev, [(x, np.array([3]), np.array([1]), adj.cpu())])
    e = rel(feats, ref)
    print("extract_features, 70-frame tracklet, V=490: max rel err vs the CPU module tree %.3e" % e)
    assert tuple(feats.shape) == tuple(ref.shape) and pids.tolist() == [3] and camids.tolist() == [1] and e < 1e-3


# ---- 8. a native train step ----------------------------------------------------------------------------------------------------------
def test_train_step_at_15_parts_per_frame():
    """vmgn with num_split 8 + pyramid (P = 15), four clips of 8 frames of 128 x 64 (V = 120: the graph matrix's backward from
    HBM), adjacency from ops.pose_adjacency(num_split=8): one xent + htri step. Loss within 1e-5 of the CPU fp32 and float64
    steps; the native gradients' error distribution against float64 within 3 x the CPU fp32 step's own + 1e-6 (the criterion and
    the reason of test_train_step_loss_and_gradients_at_the_reference_noise_floor)."""
    from test_gpu_train import _step
    S, H, W, P, K = 8, 128, 64, 2, 2
    kw = dict(num_split=8, consistent_loss=True)
    ref, dev = build_model("vmgn", **kw), build_model("vmgn", **kw).to(DEV)
    pids = torch.arange(P).repeat_interleave(K)
    x = synthetic_clips(P * K, S, H=H, W=W, seed=9, identities=pids.tolist())
    adjd = device_adjacency(P * K, S, H, 8, seed=9)
    adj = adjd.cpu()
    assert adj.shape[1] == 120 and dev.hip_train and ops_().graph_forms(120, 2048)["backward"] == "hbm"
    ref64 = copy.deepcopy(ref).double()
    l64 = _step(ref64, x.double(), adj.double(), pids, False)
    l_ref = _step(ref, x, adj, pids, False)
    l_dev = _step(dev, x.to(DEV), adjd, pids.to(DEV), True)
    torch.cuda.synchronize()
    g64 = {k: p.grad for k, p in ref64.named_parameters() if p.grad is not None}

    def dist(model):
        r = sorted(rel(p.grad, g64[k]) for k, p in model.named_parameters() if k in g64)
        return r[len(r) // 2], r[(9 * len(r)) // 10], r[-1]
    d_cpu, d_dev = dist(ref), dist(dev)
    print("train step P=15 S=%d %dx%d: loss fp64 %.7f cpu %.7f native %.7f | grad err vs fp64 (median, p90, worst): cpu fp32 %.2e %.2e %.2e, "
          "native %.2e %.2e %.2e" % ((S, H, W, l64.item(), l_ref.item(), l_dev.item()) + d_cpu + d_dev))
    assert abs(l_ref.item() - l_dev.item()) < 1e-5 * abs(l_ref.item()) and abs(l64.item() - l_dev.item()) < 1e-5 * abs(l64.item())
    assert all(p.grad is None for k, p in dev.named_parameters() if k not in g64)
    for a_, b_ in zip(d_dev, d_cpu):
        assert a_ < 3 * b_ + 1e-6
