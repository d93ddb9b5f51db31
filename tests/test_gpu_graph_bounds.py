"""The EVAL forward of the GraphLayer and of the attention tail held to ELEMENTWISE float64 bounds: csrc/gcn.hip (Gram finalize,
the five message-pass kernels, P = G f, the one-launch tracklet form), csrc/graph_gemm.hip and the agrl_graph_linear_mix entry of
igemm.hip, agrl_attn_pool_bnneck, agrl_clip_pool and the 16-bit form of agrl_pam_pool -- every output element against a float64
reference of the kernel's stated arithmetic on the operands it reads (tests/graph_ref.py: references, chain lengths and the
propagated slack of the graph matrix, derived in their docstrings), through bounds.check_rounded.

test_gpu_kernels.py judges the same kernels with one max-normalised number against the fp32 oracle (which pins the reference
model's order of operations and stays); that cannot see an off-diagonal graph entry several percent off, a channel 2^-10 of the
largest, an element nobody wrote or a dispatch branch no shape reaches. Here every kernel call runs inside poisoned_outputs()
(outputs are torch.empty: NaN-filled), runs twice, and the two results must be bitwise equal; every test of a dispatch branch
asserts through graph_ref.propagate_form which branch its shape takes. A kernel that consumes another kernel's fp32 output (the
Gram partials, the squared node norms, a graph) is referenced on THE KERNEL'S OWN values.

The worst |got - exact| / bound per kernel and form of a run (AGRL_BOUNDS_LOG) is on record in profiles/graph_bounds.txt."""
import numpy as np
import pytest
import torch

import graph_ref as GR
import pam_train_ref as PR
import train_ref as R
from bounds import U32, check_rounded, log_record, n_acc_for, poisoned_outputs
from lp16 import LP_DTYPE
from test_gpu_kernels import bound_pixels
from test_gpu_train_bounds import twice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
MODES = [(True, True, False), (True, False, False), (False, True, False), (True, True, True), (False, True, True), (True, False, True)]


def ops_():
    from torchreid import hip_ops
    return hip_ops


def node_features(B, V, C, seed):
    """Independent rows, |f|^2 ~ 8, d2 ~ 16: the reference's own slack stays below 128 u |G| (asserted by every test that uses them)."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((B, V, C), generator=g) * 4 / (2 * C) ** 0.5
    adj = (torch.rand((B, V, V), generator=g) > 0.5).float()
    adj[0, min(3, V - 1)] = 0                           # an all-zero adjacency row
    return f, adj


def check_graph(G, exact, slack, name, cap=True):
    if cap:   # a vacuous bound fails the test instead of passing the kernel
        over = slack > 128 * U32 * exact.abs()
        assert not bool(over.any()), "%s: the reference's own slack exceeds 128 u |G| at %d elements (max %.1f u)" % (
            name, int(over.sum()), float((slack / exact.abs().clamp(min=1e-300))[over].max() / U32))
    return check_rounded(G, exact, torch.zeros_like(exact), 0, F32, slack=slack, name=name)[0]


# ---- the graph matrix ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 56, 256), (2, 112, 2048), (2, 28, 512), (2, 20, 128), (2, 1, 128), (2, 65, 128), (1, 256, 128), (2, 33, 128)],
                         ids=lambda s: "%dx%dx%d" % s)
def test_graph_matrix_elementwise(shape):
    """agrl_graph_gram + agrl_graph_finalize in all three modes, with and without ganet's masked diagonal, fp32 and bit-packed
    adjacency (bitwise equal): model shapes, V = 1, 65 (a lane's second column), 256 (the entry's limit), 33 (V % 32 != 0 in the
    packed words); an all-zero adjacency row in every case."""
    ops = ops_()
    B, V, C = shape
    f, adj = node_features(B, V, C, V + C)
    fd, adjd = f.to(DEV), adj.to(DEV)
    bits = ops.adjacency_pack_host(adj)
    assert torch.equal(twice(lambda: ops.adjacency_pack(adjd)), bits)
    gram = twice(lambda: ops.graph_gram(fd))
    gram_d = gram.to(DEV)
    for use_pose, learn_graph, mask_diag in MODES:
        G = twice(lambda: ops.graph_finalize(gram_d if learn_graph else None, adjd if use_pose else None, B, V, use_pose, learn_graph, mask_diag))
        exact, slack = GR.graph_matrix_ref(gram, adj, use_pose, learn_graph, mask_diag)
        check_graph(G, exact, slack, "graph_matrix|finalize|%s pose=%d learn=%d mask=%d" % (shape, use_pose, learn_graph, mask_diag))
        if use_pose:
            Gb = twice(lambda: ops.graph_matrix(fd, bits.to(DEV), use_pose, learn_graph, mask_diag=mask_diag))
            assert torch.equal(Gb, G), "packed adjacency: %d of %d elements differ" % (int((Gb != G).sum()), G.numel())
            assert torch.equal(twice(lambda: ops.graph_matrix(fd, adjd, use_pose, learn_graph, mask_diag=mask_diag)), G)
        if mask_diag:
            assert bool((torch.diagonal(G, dim1=1, dim2=2) == 0).all())
    assert bool((G[0, min(3, V - 1)] == 0).all())      # pose only, masked: the all-zero adjacency row stays zero (0 / clamp)


@pytest.mark.parametrize("shape", [(3, 56, 256), (2, 112, 2048)], ids=lambda s: "%dx%dx%d" % s)
def test_graph_matrix_on_model_like_features(shape):
    """Node features as the trunk produces them (a common positive vector + 2 % noise: d2 ~ 1.6 from squared norms ~ 680): the
    similarity is ill-conditioned and the propagated slack carries that; its size relative to |G| is put on record, not asserted."""
    ops = ops_()
    B, V, C = shape
    g = torch.Generator().manual_seed(V)
    f = torch.rand((B, 1, C), generator=g) + 0.02 * torch.randn((B, V, C), generator=g)
    adj = (torch.rand((B, V, V), generator=g) > 0.5).float()
    fd, adjd = f.to(DEV), adj.to(DEV)
    gram = twice(lambda: ops.graph_gram(fd))
    G = twice(lambda: ops.graph_finalize(gram.to(DEV), adjd, B, V, True, True, False))
    exact, slack = GR.graph_matrix_ref(gram, adj, True, True, False)
    worst = check_graph(G, exact, slack, "graph_matrix|finalize|model-like %s" % (shape,), cap=False)
    log_record({"name": "graph_matrix|model-like %s slack / |G| in u" % (shape,), "max": float((slack / exact.abs().clamp(min=1e-300)).max() / U32), "ratio": worst})


# ---- the one-launch tracklet form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 4, 512), (5, 20, 1024), (5, 56, 512), (1, 64, 1024), (5, 64, 512)], ids=lambda s: "%dx%dx%d" % s)
def test_graph_tracklet_form_elementwise(shape):
    """agrl_graph_tracklet_operand: G against graph_ref.tracklet_gram_ref (eight wave partials) + the finalize propagation, P = G f
    against the kernel's own G in fp32 and the 16-bit type; G also within the two slacks of the three-launch form's."""
    ops = ops_()
    B, V, C = shape
    f, adj = node_features(B, V, C, B + V + C)
    fd, adjd = f.to(DEV), adj.to(DEV)
    gram_t = GR.tracklet_gram_ref(f)
    gram3 = twice(lambda: ops.graph_gram(fd))
    for use_pose, learn_graph, mask_diag in ((True, True, False), (False, True, True), (True, False, False)):
        tag = "%s pose=%d learn=%d mask=%d" % (shape, use_pose, learn_graph, mask_diag)
        a = adjd if use_pose else None
        P, G = twice(lambda: ops.graph_tracklet_operand(fd, a, use_pose, learn_graph, F32, want_graph=True, mask_diag=mask_diag))
        Plp, none = twice(lambda: ops.graph_tracklet_operand(fd, a, use_pose, learn_graph, LP_DTYPE, mask_diag=mask_diag))
        assert none is None and Plp.dtype == LP_DTYPE
        exact, slack = GR.graph_matrix_ref(None, adj, use_pose, learn_graph, mask_diag, gram=gram_t)
        # (no 128 u cap here: the wave partials' chain, C / 32 + 11 roundings against the finalize form's C / 128, is part of this slack)
        check_graph(G, exact, slack, "graph_matrix|tracklet|" + tag, cap=False)
        G3 = twice(lambda: ops.graph_matrix(fd, a, use_pose, learn_graph, mask_diag=mask_diag))
        exact3, slack3 = GR.graph_matrix_ref(gram3, adj, use_pose, learn_graph, mask_diag)
        check_graph(G3, exact3, slack3, "graph_matrix|finalize|" + tag)
        apart = (G.double() - G3.double()).abs() - (slack + slack3)
        assert float(apart.max()) <= 0, "%s: tracklet and three-launch graphs %.3g beyond their two slacks" % (tag, float(apart.max()))
        pe, pm, n = GR.apply_ref(G, f)
        check_rounded(P, pe, pm, n, F32, name="graph_apply|tracklet fp32|" + tag)
        check_rounded(Plp, pe, pm, n, LP_DTYPE, name="graph_apply|tracklet lp16|" + tag)


# ---- the message pass, every dispatch branch ---------------------------------------------------------------------------------------
PROPAGATE_CASES = [
    ("stream4", (2, 4, 256)), ("stream4", (2, 28, 256)), ("stream4", (1, 64, 512)),
    ("stream2", (2, 56, 128)), ("stream2", (2, 20, 384)),
    ("mfma4", (2, 1, 128)), ("mfma4", (2, 3, 256)), ("mfma4", (2, 49, 128)), ("mfma4", (2, 63, 256)),
    ("mfma8", (2, 65, 128)), ("mfma8", (1, 112, 256)), ("mfma8", (1, 128, 128)),
    # generic LDS form: C % 128 != 0; V > 128; V = 146: the last V whose graph + h slab fit 160 KB (the kernel raises its dynamic LDS)
    ("generic", (2, 20, 260)), ("generic", (1, 130, 128)), ("generic", (1, 146, 128)),
    # tiled form: from V = 147 (V (Vp + 128) 4 bytes > 160 KB, Vp = 152); 148 and 149 sit either side of where the entry's
    # comment put the limit (~125) and a count of Vp = V would (148)
    ("tiled", (1, 147, 128)), ("tiled", (1, 148, 128)), ("tiled", (1, 149, 128)), ("tiled", (2, 240, 132)),
]
MIXES = [(0.9, 0.1), (1.0, 0.3), (0.0, 1.0)]     # (keep, gamma): vmgn's 1 - gamma, ganet's keep = 1, the bare message


def message_operands(B, V, C, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((B, V, C), generator=g)
    h = torch.randn((B, V, C), generator=g) * R.channel_scales(C, seed + 1, -8, 2)
    G = torch.randn((B, V, V), generator=g) / V ** 0.5                   # random and dense: the message pass on its own
    scale, shift = torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)   # a real BatchNorm, mixed signs
    return f, h, G, scale, shift


@pytest.mark.parametrize("form,shape", PROPAGATE_CASES, ids=["%s-%dx%dx%d" % ((fm,) + s) for fm, s in PROPAGATE_CASES])
def test_graph_propagate_elementwise(form, shape):
    """agrl_graph_propagate with a real BatchNorm, LeakyReLU(0.1) and the three residual mixes, with and without the 16-bit copy,
    on the branch ``form`` (asserted against the mirrored dispatch); out_lp is bounded against float64 AND is exactly the one
    rounding of out."""
    ops = ops_()
    B, V, C = shape
    got_form, n_acc = GR.propagate_form(V, C)
    assert got_form == form, "shape %s takes the %s kernel" % (shape, got_form)
    f, h, G, scale, shift = message_operands(B, V, C, V * 7 + C)
    fd, hd, Gd, sd, shd = (t.to(DEV) for t in (f, h, G, scale, shift))
    for keep, gamma in MIXES:
        exact, mag, n = GR.message_ref(f, h, G, scale, shift, keep, gamma, 0.1, form)
        assert n == n_acc
        tag = "graph_propagate|%s|%s keep=%g gamma=%g" % (form, shape, keep, gamma)
        out, out_lp = twice(lambda: ops.graph_propagate(fd, hd, Gd, sd, shd, gamma, 0.1, want_lp=True, keep=keep))
        out1, none = twice(lambda: ops.graph_propagate(fd, hd, Gd, sd, shd, gamma, 0.1, want_lp=False, keep=keep))
        assert none is None and torch.equal(out1, out)
        check_rounded(out, exact, mag, n, F32, name=tag)
        check_rounded(out_lp, exact, mag, n, LP_DTYPE, name=tag + " out_lp")
        check_rounded(out_lp, out.double(), torch.zeros_like(exact), 0, LP_DTYPE, min_exact_frac=1.0, name=tag + " out_lp = rounded out")
    # keep defaults to the reference's Python-float 1 - gamma
    assert torch.equal(twice(lambda: ops.graph_propagate(fd, hd, Gd, sd, shd, 0.1, 0.1, want_lp=False)[0]),
                       twice(lambda: ops.graph_propagate(fd, hd, Gd, sd, shd, 0.1, 0.1, want_lp=False, keep=1.0 - 0.1)[0]))


@pytest.mark.parametrize("form,shape", PROPAGATE_CASES, ids=["%s-%dx%dx%d" % ((fm,) + s) for fm, s in PROPAGATE_CASES])
def test_graph_apply_operand_elementwise(form, shape):
    """P = G f as graph_apply_operand writes it, fp32 and 16-bit: agrl_graph_apply for the streaming shapes, the message-pass kernel
    of ``form`` behind a unit BatchNorm for the others."""
    ops = ops_()
    B, V, C = shape
    f, _, G, _, _ = message_operands(B, V, C, V * 7 + C)
    fd, Gd = f.to(DEV), G.to(DEV)
    n = n_acc_for(V, 4) if form.startswith("stream") else GR.propagate_form(V, C)[1]
    exact, mag, n = GR.apply_ref(G, f, n)
    P = twice(lambda: ops.graph_apply_operand(Gd, fd, F32))
    Plp = twice(lambda: ops.graph_apply_operand(Gd, fd, LP_DTYPE))
    assert P.dtype == F32 and Plp.dtype == LP_DTYPE
    check_rounded(P, exact, mag, n, F32, name="graph_apply|%s fp32|%s" % (form, shape))
    check_rounded(Plp, exact, mag, n, LP_DTYPE, name="graph_apply|%s lp16|%s" % (form, shape))
    if not form.startswith("stream"):     # one kernel writes both: the 16-bit copy is the one rounding of the fp32 result
        check_rounded(Plp, P.double(), torch.zeros_like(exact), 0, LP_DTYPE, min_exact_frac=1.0, name="graph_apply|%s lp16 = rounded fp32|%s" % (form, shape))
    # agrl_graph_apply's name in the train step: always the message-pass kernel of ``form`` behind the unit BatchNorm
    check_rounded(twice(lambda: ops.graph_apply(Gd, fd)), exact, mag, GR.propagate_form(V, C)[1], F32, name="graph_apply|%s unit BatchNorm|%s" % (form, shape))


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def twice_with_nans(fn):
    """twice() for outputs that hold NaNs on purpose: poisoned allocations, two runs, bitwise equal."""
    runs = []
    for _ in range(2):
        with poisoned_outputs():
            o = fn()
        torch.cuda.synchronize()
        runs.append(o.detach().cpu())
    assert bits_equal(runs[0], runs[1])
    return runs[0]


NAN_CASES = [("stream4", (2, 28, 256)), ("stream2", (2, 20, 384)), ("mfma4", (2, 49, 128)), ("mfma8", (2, 65, 128)), ("generic", (2, 20, 260)),
             ("tiled", (2, 149, 128))]


@pytest.mark.parametrize("form,shape", NAN_CASES, ids=[fm for fm, _ in NAN_CASES])
def test_graph_propagate_nan_placement(form, shape):
    """Which outputs an input reaches: a NaN at h[b,u0,c0] appears at out[b,:,c0] and nowhere else, a NaN at f[b,v0,c0] at that one
    output, and a last graph row / last node of tracklet b that is all NaN leaves tracklet b + 1 bit for bit as it was (the streaming
    form's padded fragment rows read whatever follows the graph in LDS: nothing of that may be stored)."""
    ops = ops_()
    B, V, C = shape
    assert GR.propagate_form(V, C)[0] == form and B == 2
    f, h, G, scale, shift = message_operands(B, V, C, V + C)
    sd, shd, Gd = scale.to(DEV), shift.to(DEV), G.to(DEV)
    clean = twice(lambda: ops.graph_propagate(f.to(DEV), h.to(DEV), Gd, sd, shd, 0.1, 0.1, False)[0])
    u0, v0, c0 = V - 1, V // 2, C - 3
    hn = h.clone()
    hn[0, u0, c0] = float("nan")
    out = twice_with_nans(lambda: ops.graph_propagate(f.to(DEV), hn.to(DEV), Gd, sd, shd, 0.1, 0.1, False)[0])
    want = torch.zeros((B, V, C), dtype=torch.bool)
    want[0, :, c0] = True
    assert torch.equal(torch.isnan(out), want), "NaN at h[0,%d,%d]: %d NaNs, %d expected" % (u0, c0, int(torch.isnan(out).sum()), V)
    assert bits_equal(out[~want], clean[~want])
    fn_ = f.clone()
    fn_[0, v0, c0] = float("nan")
    out = twice_with_nans(lambda: ops.graph_propagate(fn_.to(DEV), h.to(DEV), Gd, sd, shd, 0.1, 0.1, False)[0])
    want = torch.zeros((B, V, C), dtype=torch.bool)
    want[0, v0, c0] = True
    assert torch.equal(torch.isnan(out), want) and bits_equal(out[~want], clean[~want])
    hn, fn_, Gn = h.clone(), f.clone(), G.clone()
    hn[0, V - 1], fn_[0, V - 1], Gn[0, V - 1] = float("nan"), float("nan"), float("nan")
    out = twice_with_nans(lambda: ops.graph_propagate(fn_.to(DEV), hn.to(DEV), Gn.to(DEV), sd, shd, 0.1, 0.1, False)[0])
    assert bool(torch.isnan(out[0]).all()) and bits_equal(out[1], clean[1]), "tracklet 1: %d NaNs" % int(torch.isnan(out[1]).sum())


# ---- the Linear with the GraphLayer epilogue ---------------------------------------------------------------------------------------
def linear_case(M, K, N, mode, seed, keep=1.0, gamma=0.3):
    """-> the call (a closure over device operands) and the reference's operands (what the kernel multiplies, as float)."""
    ops = ops_()
    g = torch.Generator().manual_seed(seed)
    P, W = torch.randn((1, M, K), generator=g), torch.randn((N, K), generator=g) / K ** 0.5
    f = torch.randn((1, M, N), generator=g)
    scale, shift = torch.randn(N, generator=g), 0.3 * torch.randn(N, generator=g)
    fd, sd, shd = f.to(DEV), scale.to(DEV), shift.to(DEV)
    if mode == "lp16":
        Pd, Wd = P.to(LP_DTYPE).to(DEV), W.to(LP_DTYPE).to(DEV)
        P, W = Pd.float().cpu(), Wd.float().cpu()
        call = lambda: ops.graph_linear_mix(Pd, Wd, fd, sd, shd, gamma, 0.1, keep=keep)
    elif mode == "fp16x3":
        Pd, Wd = P.to(DEV), ops.split16_inloop_weights(W.to(DEV))
        assert torch.equal(ops.split16_true_weights(Wd).cpu(), W)        # the power-of-two pre-scale is exact
        sfold = (sd * Wd.agrl_unscale).contiguous()
        sfold.agrl_folded_unscale = Wd.agrl_unscale
        call = lambda: ops.graph_linear_mix(Pd, Wd, fd, sfold, shd, gamma, 0.1, keep=keep)
    else:
        Pd, Wd = P.to(DEV), W.to(DEV)

        def call():
            with ops.f32_split(mode == "bf16x3"):
                return ops.graph_linear_mix(Pd, Wd, fd, sd, shd, gamma, 0.1, keep=keep)
    return call, (P, W, f, scale, shift, keep, gamma, 0.1, mode)


def check_linear(M, K, N, mode, seed, tag, **kw):
    call, operands = linear_case(M, K, N, mode, seed, **kw)
    out = twice(call)
    rows = bound_pixels(M, K, N, seed)
    rows = None if rows.numel() == M else rows
    exact, mag, n_acc, slack = GR.linear_mix_ref(*operands, rows=rows)
    got = out.view(M, N) if rows is None else out.view(M, N)[rows]
    return check_rounded(got, exact, mag, n_acc, F32, slack=slack, name="graph_linear_mix|%s|%s M=%d K=%d N=%d" % (mode, tag, M, K, N))[0]


@pytest.mark.parametrize("mode", GR.LINEAR_MODES)
@pytest.mark.parametrize("K", [64, 128, 192, 256, 2048])
def test_graph_linear_mix_elementwise(K, mode):
    """agrl_graph_linear_mix with K != N: one, two, three and four 64-deep k-tiles (graph_linear_kernel's ring is four slots deep)
    and the model's 32; a ragged M-tile and grids of 1 .. 6 workgroups (the XCD remap); every precision mode."""
    ops = ops_()
    for N in (128, 256):
        for M in (4, 84, 129, 300):
            if mode == "lp16":
                assert -(-M // 128) * (N // 128) <= torch.cuda.get_device_properties(0).multi_processor_count   # graph_linear_kernel
            check_linear(M, K, N, mode, K + N + M, "ring" if mode == "lp16" else "igemm")
    check_linear(84, K, 128, mode, K, "vmgn mix", keep=0.9, gamma=0.1)


def test_graph_linear_mix_falls_back_when_tiles_outnumber_the_cus():
    M, K, N = 2072, 64, 2048
    assert -(-M // 128) * (N // 128) > torch.cuda.get_device_properties(0).multi_processor_count, "choose a larger M for this GPU"
    check_linear(M, K, N, "lp16", 1, "igemm fallback")


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_graph_linear_mix_ragged_channel_tile(mode):
    """N % 128 != 0 (the entry asks N % 4 == 0): the last channel tile is partial."""
    check_linear(84, 64, 132, mode, 2, "ragged N")
    check_linear(129, 192, 260, mode, 3, "ragged N")


# ---- the attention tail ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(3, 8, 7, 2048, 128), (2, 3, 5, 260, 60), (1, 9, 1, 4, 1), (2, 16, 7, 256, 128), (2, 4, 1, 512, 32)],
                         ids=lambda c: "x".join(str(v) for v in c))
def test_attention_tail_elementwise(cfg):
    """agrl_row_sqnorm + agrl_attn_pool_bnneck: the c >= C tail of the last workgroup (C = 260, 4), res50tp's P = 1, a frame whose
    nodes are all zero, a part that is zero in every frame (denominator at the clamp), per-channel scales over 12 binades."""
    ops = ops_()
    B, S, P, C, hw = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    nodes = torch.rand((B, S, P, C), generator=g) * R.channel_scales(C, S, -10, 2)
    nodes[B - 1, min(2, S - 1)] = 0
    if P > 1 or B > 1:
        nodes[0, :, P - 1] = 0
    gsum = torch.rand((B * S, C), generator=g) * hw * R.channel_scales(C, P, -10, 2)
    nd, gd = nodes.to(DEV), gsum.to(DEV)
    sqn = twice(lambda: ops.row_sqnorm(nd.view(B * S * P, C)))
    sqd = sqn.to(DEV)
    pairs = [("identity", torch.ones(C), torch.zeros(C), torch.ones(C), torch.zeros(C))]
    pairs.append(("batchnorm", torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)))
    for name, gs, gsh, as_, ash in pairs:
        out, gf, af = twice(lambda: ops.attn_pool_bnneck(nd, sqd, gd, gs.to(DEV), gsh.to(DEV), as_.to(DEV), ash.to(DEV), B, S, P, hw, want_feats=True))
        only = twice(lambda: ops.attn_pool_bnneck(nd, sqd, gd, gs.to(DEV), gsh.to(DEV), as_.to(DEV), ash.to(DEV), B, S, P, hw))
        assert torch.equal(only, out)
        ref = GR.attn_pool_ref(nodes, sqn, gsum, gs, gsh, as_, ash, hw)
        for key, t in (("out", out), ("g_f", gf), ("att_f", af)):
            check_rounded(t, *ref[key], F32, name="attn_pool_bnneck|%s %s|%s" % (key, name, cfg))
    if P == 1 and B > 1:
        assert bool((af[0] == 0).all())       # tracklet 0's only part is zero in every frame


# ---- clip pooling ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(3, 1, 4096), (2, 11, 2048), (7, 3, 1000), (1, 9, 1), (300, 2, 260)], ids=lambda c: "x".join(str(v) for v in c))
def test_clip_pool_elementwise(cfg):
    """agrl_clip_pool: the mean within n + 1 roundings, the max exact; a NaN clip stays NaN in both modes; the sign of a zero
    maximum follows torch.max on the same device."""
    ops = ops_()
    T, n, D = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x = torch.randn((T * n, D), generator=g) * R.channel_scales(D, n)
    xd = x.to(DEV)
    mean, mx = twice(lambda: ops.clip_pool(xd, n, "avg")), twice(lambda: ops.clip_pool(xd, n, "max"))
    check_rounded(mean, *GR.clip_mean_ref(x, n), F32, name="clip_pool|mean|%s" % (cfg,))
    assert torch.equal(mx, x.view(T, n, D).max(1).values)
    xn = x.clone()
    xn[n - 1, D // 2] = float("nan")                   # the last clip of tracklet 0, one channel
    want = torch.zeros((T, D), dtype=torch.bool)
    want[0, D // 2] = True
    for mode, clean in (("avg", mean), ("max", mx)):
        got = twice_with_nans(lambda: ops.clip_pool(xn.to(DEV), n, mode))
        assert torch.equal(torch.isnan(got), want) and bits_equal(got[~want], clean[~want]), mode
    if n > 1:
        z = torch.zeros((T * n, D))
        z.view(T, n, D)[:, 0::2] = -0.0                # -0, +0, -0, ..
        if T > 1:
            z.view(T, n, D)[1] = -z.view(T, n, D)[1]   # +0, -0, +0, ..
        zd = z.to(DEV)
        got = twice(lambda: ops.clip_pool(zd, n, "max"))
        assert bits_equal(got, zd.view(T, n, D).max(1).values.cpu()), "the sign of a zero maximum differs from torch.max"


# ---- ganet's position-attention pooling in eval, 16-bit maps -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 6, 4, 64, 32, [4]), (3, 12, 8, 512, 64, [4, 2, 1])], ids=["h6n4", "pyramid"])
def test_pam_pool_16_bit_map_elementwise(shape):
    """agrl_pam_pool on a 16-bit map (h = 6 with n = 4 drops remainder rows): xbar and xmean against
    hip_ops.pam_nodes_backward_reference in float64 on the rounded operands, with the softmax slack of pam_train_ref; then
    agrl_pam_combine: nodes within two roundings, nodes_lp exactly the one rounding of nodes."""
    ops = ops_()
    Fr, h, w, C, Cq, splits = shape
    g = torch.Generator().manual_seed(Fr + h + C)
    x = (0.5 * torch.randn((Fr, h, w, C), generator=g)).to(LP_DTYPE)
    qk = x[..., :2 * Cq].contiguous()
    xd, qkd = x.to(DEV), qk.to(DEV)
    xbar, xmean = twice(lambda: ops.pam_pool(xd, qkd, splits))
    none, xmean0 = twice(lambda: ops.pam_pool(xd, None, splits))
    assert none is None and torch.equal(xmean0, xmean)
    ref = GR.pam_pool_ref(x.float(), qk.float(), splits, ops.pam_nodes_backward_reference)
    e, m, n, s = ref["xbar"]
    check_rounded(xbar, e, m, n, F32, slack=s, name="pam_pool|xbar lp16 map|%s" % (shape,))
    check_rounded(xmean, *ref["xmean"], F32, name="pam_pool|xmean lp16 map|%s" % (shape,))
    P = sum(splits)
    y, bv = torch.randn((Fr * P, C), generator=g), torch.randn(C, generator=g)
    yd, bvd, xmd = y.to(DEV), bv.to(DEV), xmean.to(DEV)
    nodes, nodes_lp = twice(lambda: ops.pam_combine(yd, bvd, xmd, 0.7, want_lp=True))
    ce, cm, cn = PR.combine_ref(y.view(Fr, P, C), bv, xmean, float(np.float32(0.7)))
    check_rounded(nodes, ce, cm, cn, F32, name="pam_combine|nodes|%s" % (shape,))
    check_rounded(nodes_lp, nodes.double(), torch.zeros_like(ce), 0, LP_DTYPE, min_exact_frac=1.0, name="pam_combine|nodes_lp = rounded nodes|%s" % (shape,))
