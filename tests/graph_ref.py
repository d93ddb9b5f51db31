"""float64 references and fp32 chain lengths for the EVAL forward of the GraphLayer and of the attention tail (csrc/gcn.hip,
graph_gemm.hip, the agrl_graph_linear_mix entry of igemm.hip, agrl_attn_pool_bnneck / agrl_clip_pool of pool.hip, the 16-bit form of
agrl_pam_pool), for ``bounds.check_rounded``:

    |got - exact| <= half_ulp(|exact| + delta) + delta (+ slack),      delta = n_acc * 2^-24 * mag

``exact`` is the float64 value of the kernel's stated operation on the operands it reads, ``mag`` the same operation on their
magnitudes, ``n_acc`` the longest chain of fp32 roundings the kernel's own summation order can produce (counted in each
docstring from the code; the exact-fp32 v_mfma_f32_16x16x4_f32 counts one rounding per 4-deep step, as in bounds.n_acc_for).
Where an output sits behind sqrt / exp / a normalisation (the graph matrix) the bound is the rounding of every fp32 step
propagated to first order and handed over as ``slack``. Everything here runs on the CPU; tests/test_bounds.py holds each helper
against an fp32 emulation of the stated arithmetic and against seeded faults. A plain module (like train_ref.py)."""
import math

import numpy as np
import torch

from bounds import U32, n_acc_for

GT_WAVES = 8            # csrc/gcn.hip: waves of graph_tracklet_kernel, each owns C / GT_WAVES channels of the Gram
PROP_THREADS = 128      # channels per workgroup of the generic / tiled message pass
LDS_BYTES = 160 * 1024  # what a workgroup may raise its dynamic LDS to


def f32(x):
    """A Python float as the fp32 value a kernel argument carries."""
    return float(np.float32(x))


# ---- the graph matrix --------------------------------------------------------------------------------------------------------
def unpack_adjacency(adj, V):
    """The bit-packed adjacency (B, V, ceil(V / 32)) int32 -- bit j & 31 of word j >> 5 of row i -- as float64 {0, 1} (B,V,V);
    an fp32 / float64 (B,V,V) adjacency is passed through."""
    if adj.dtype != torch.int32:
        return adj.detach().cpu().double()
    words = adj.detach().cpu().numpy().view(np.uint32)
    j = np.arange(V)
    bits = (words[:, :, j >> 5] >> (j & 31).astype(np.uint32)) & 1
    return torch.from_numpy(bits.astype(np.float64))


def gram_from_partials(gram_part):
    """zsum: the nz slice partials (B,nz,V,V) of one element added z ascending -> g (float64), an absolute bound nz u sum_z |part|."""
    gp = gram_part.detach().cpu().double()
    return gp.sum(1), gp.shape[1] * U32 * gp.abs().sum(1)


def similarity_chain(g, a, mask_diag=False):
    """Gram g (B,V,V) float64 with the absolute bound a of the fp32 value the kernel holds -> every stage of
    graph_finalize_kernel's learned half in float64 with its first-order fp32 bound (t = ceil(V / 64) + 6: a lane's columns + the
    six steps of the wave sum):
      D2 = (n_j + n_i) - 2 g, n = diag g: those of g_ii, g_jj, 2 g_ij + 2 u (n_i + n_j + 2 |g_ij|); the diagonal is exactly 0 in
           fp32 too ((x + x) - 2 x), so it sits at the clamp 1e-12 on both sides and carries no error;
      D = sqrt(max(D2, 1e-12)): eD2 / (2 D) + u D;   S = 2 / (exp(D) + 1): |S'| eD + 4 u S (expf at 1 ulp, the sum, the quotient),
           S' = -h, h = S (1 - S / 2);   mask_diag: S_ii = 0 exactly;
      r = sum_j |S_ij|: sum_j eS + t u r;   Shat = S / max(r, 1e-12): Shat (eS / S + er / r + u).
    The D2 step is the ill-conditioned one (similar nodes: D2 << n_i + n_j); the bound carries that conditioning.
    -> dict of float64 tensors: D2, D, eD, S, h, eS, r, er, Sh, eSh and the bool masks eye, live (D2 above the clamp, off the
    diagonal)."""
    u = U32
    V = g.shape[-1]
    n, an = torch.diagonal(g, dim1=1, dim2=2), torch.diagonal(a, dim1=1, dim2=2)
    eye = torch.eye(V, dtype=torch.bool).view(1, V, V)
    D2 = n[:, :, None] + n[:, None, :] - 2 * g
    eD2 = an[:, :, None] + an[:, None, :] + 2 * a + 2 * u * (n[:, :, None] + n[:, None, :] + 2 * g.abs())
    eD2 = eD2.masked_fill(eye, 0.0)        # (g_ii + g_ii) - 2 g_ii is exactly 0 in fp32 too: the diagonal sits at the clamp in both
    D2 = D2.masked_fill(eye, 0.0)
    live = (D2 > 1e-12) & ~eye
    D = D2.clamp(min=1e-12).sqrt()
    eD = eD2 / (2 * D) + u * D
    S = 2 / (torch.exp(D) + 1)
    h = S * (1 - S / 2)
    eS = h * eD + 4 * u * S
    if mask_diag:
        S, h, eS = S.masked_fill(eye, 0.0), h.masked_fill(eye, 0.0), eS.masked_fill(eye, 0.0)
    t = -(-V // 64) + 6
    r = S.sum(2, keepdim=True)
    er = eS.sum(2, keepdim=True) + t * u * r
    rc = r.clamp(min=1e-12)
    Sh = S / rc
    eSh = Sh * (eS / S.clamp(min=1e-300) + er / rc + u)
    return {"D2": D2, "D": D, "eD": eD, "S": S, "h": h, "eS": eS, "r": r, "er": er, "Sh": Sh, "eSh": eSh, "eye": eye, "live": live}


def graph_matrix_ref(gram_part, adj, use_pose, learn_graph, mask_diag=False, gram=None):
    """agrl_graph_finalize (and phase 2 of graph_tracklet_kernel) from the kernel's own Gram partials (B,nz,V,V) -- or from
    ``gram`` = (g, a), a Gram with its absolute bound (tracklet_gram_ref) -- in float64:
        learned  Shat of similarity_chain;   pose  A_ij = adj_ij / max(sum_j |adj_ij|, 1e-12) (mask_diag: adj_ii = 0);
        G = (A + Shat) / 2 with both, else the one that is on.
    The adjacency terms are small integers: the row sum is exact, the quotient rounds once (u A). The sum A + Shat rounds once,
    the halving is exact: eG = (u A + eShat) / 2 + u |G|. ``adj``: fp32 (B,V,V) or the bit-packed int32 (B,V,ceil(V/32)).
    -> exact G, slack (B,V,V) float64."""
    u = U32
    Sh = eSh = None
    if learn_graph:
        g, a = gram_from_partials(gram_part) if gram is None else gram
        c = similarity_chain(g.double(), a.double(), mask_diag)
        Sh, eSh = c["Sh"], c["eSh"]
        V = g.shape[-1]
    if use_pose:
        if not learn_graph:
            V = adj.shape[1]
        A = unpack_adjacency(adj, V)
        if mask_diag:
            A = A.masked_fill(torch.eye(V, dtype=torch.bool).view(1, V, V), 0.0)
        A = A / A.abs().sum(2, keepdim=True).clamp(min=1e-12)
        eA = u * A.abs()
        if not learn_graph:
            return A, eA
        G = (A + Sh) / 2
        return G, (eA + eSh) / 2 + u * G.abs()
    return Sh, eSh


def tracklet_gram_ref(f):
    """The Gram f f^T (B,V,V) as graph_tracklet_kernel sums it: GT_WAVES wave partials of C / GT_WAVES channels each, one
    rounding per 4-channel step of the exact-fp32 MFMA (bounds.n_acc_for(C / GT_WAVES, 4)), the partials added in wave order
    from 0 (GT_WAVES additions). The slices partition the channels, so the chain errors add up to one chain's worth of the whole
    magnitude -> exact g, absolute bound (n_acc_for(C / GT_WAVES, 4) + GT_WAVES) u |f| |f|^T."""
    x = f.detach().cpu().double()
    C = x.shape[-1]
    assert C % GT_WAVES == 0
    n = n_acc_for(C // GT_WAVES, 4) + GT_WAVES
    return torch.bmm(x, x.transpose(1, 2)), n * U32 * torch.bmm(x.abs(), x.abs().transpose(1, 2))


# ---- the message pass --------------------------------------------------------------------------------------------------------
EPILOGUE = 5   # fmaf(acc, scale, shift), slope * y, keep * f, gamma * y, their sum: at most five roundings behind the chain


def propagate_form(V, C):
    """The kernel agrl_graph_propagate launches for 16-byte aligned tensors, mirrored from its dispatch -> (form, n_acc):
      'stream4' / 'stream2'  V <= 64, V % 4 == 0, C % 128 == 0: graph_propagate_stream_kernel, 4 waves (C % 256 == 0) or 2
      'mfma4' / 'mfma8'      V <= 128, C % 128 == 0: graph_propagate_mfma_kernel<4> (V <= 64) / <8>
      'generic'              graph + h slab in LDS: V (Vp + 128) 4 bytes <= 160 KB, Vp = V rounded up to 8 (V <= 146 at C % 128 == 0)
      'tiled'                16 graph rows per workgroup, h streamed
    n_acc: ceil(V / 4) exact-fp32 MFMA steps (stream, MFMA) or V fmas (generic, tiled), + EPILOGUE."""
    if V <= 64 and V % 4 == 0 and C % 128 == 0:
        return ("stream4" if C % 256 == 0 else "stream2"), -(-V // 4) + EPILOGUE
    if V <= 128 and C % 128 == 0:
        return ("mfma4" if V <= 64 else "mfma8"), -(-V // 4) + EPILOGUE
    Vp = (V + 7) & ~7
    if (V * Vp + V * PROP_THREADS) * 4 > LDS_BYTES:
        assert V * 16 * 4 <= 64 * 1024, "agrl_graph_propagate refuses V=%d" % V
        return "tiled", V + EPILOGUE
    return "generic", V + EPILOGUE


def form_chain(form, V):
    return (-(-V // 4) if form.startswith(("stream", "mfma")) else V) + EPILOGUE


def message_ref(f, h, G, scale, shift, keep, gamma, slope, form):
    """agrl_graph_propagate: out[b,v,c] = keep f + gamma lrelu(scale_c (sum_u G[b,v,u] h[b,u,c]) + shift_c) in float64 on the
    fp32 operands (keep, gamma, slope as the fp32 values the kernel gets) -> exact, mag, n_acc with
    mag = |keep| |f| + |gamma| (|scale| (|G| |h|) + |shift|): LeakyReLU is 1-Lipschitz (0 <= slope <= 1), so the bound of the
    pre-activation carries through whichever side of 0 the fp32 value falls. ``form``: a name of propagate_form (its chain)."""
    k, g_, s = f32(keep), f32(gamma), f32(slope)
    f64, h64, G64 = f.detach().cpu().double(), h.detach().cpu().double(), G.detach().cpu().double()
    sc, sh = scale.detach().cpu().double(), shift.detach().cpu().double()
    pre = torch.bmm(G64, h64) * sc + sh
    pmag = torch.bmm(G64.abs(), h64.abs()) * sc.abs() + sh.abs()
    y = torch.where(pre > 0, pre, pre * s)
    return k * f64 + g_ * y, abs(k) * f64.abs() + abs(g_) * pmag, form_chain(form, G.shape[-1])


def apply_ref(G, f, n_acc=None):
    """P = G f (agrl_graph_apply, the P of the tracklet form; graph_apply_operand's fall-back through the message pass with a unit
    BatchNorm multiplies by 1 and adds 0: exact) -> exact, mag, n_acc (default: ceil(V / 4) MFMA steps + 3, bounds.n_acc_for)."""
    G64, f64 = G.detach().cpu().double(), f.detach().cpu().double()
    return torch.bmm(G64, f64), torch.bmm(G64.abs(), f64.abs()), (n_acc_for(G.shape[-1], 4) if n_acc is None else n_acc)


# ---- the Linear with the GraphLayer epilogue ---------------------------------------------------------------------------------
LINEAR_MODES = ("fp32", "bf16x3", "fp16x3", "lp16")


def linear_mix_ref(P, W, f, scale, shift, keep, gamma, slope, mode, rows=None):
    """agrl_graph_linear_mix: out = keep f + gamma lrelu(scale (P W^T) + shift) on the operands the kernel multiplies (16-bit values
    as float; 'fp16x3': W and scale WITHOUT the power-of-two pre-scale, which is exact) -> exact, mag, n_acc, slack.
    n_acc = bounds.n_acc_for(K, 4 | 16) + 4: the k-chain (exact-fp32 MFMA: 4 deep; 16-bit MFMA: 16 per lane group; the two k-halves
    of graph_linear_kernel meet in one addition, inside n_acc_for's slack) and the epilogue's slope, keep f, gamma y and sum.
    Split modes: every product carries C |p| |w|: slack = C |gamma| |scale| (|P| |W|^T) with C = train_ref.C_SPLIT for 'bf16x3' (the
    bound of test_bounds.py's split recipe) and, for 'fp16x3', split16_ref.C_SPLIT16 plus that module's absolute terms for low halves
    that are not normal fp16 numbers (P split in the k-loop, W pre-scaled and split at pack time). ``rows``: optional row subset of M."""
    from train_ref import C_SPLIT
    assert mode in LINEAR_MODES
    K = P.shape[-1]
    p2, f2 = P.detach().cpu().double().reshape(-1, K), f.detach().cpu().double().reshape(-1, W.shape[0])
    if rows is not None:
        p2, f2 = p2[rows], f2[rows]
    w64, sc, sh = W.detach().cpu().double(), scale.detach().cpu().double(), shift.detach().cpu().double()
    k, g_, s = f32(keep), f32(gamma), f32(slope)
    acc, amag = p2 @ w64.t(), p2.abs() @ w64.abs().t()
    pre = acc * sc + sh
    y = torch.where(pre > 0, pre, pre * s)
    mag = abs(k) * f2.abs() + abs(g_) * (amag * sc.abs() + sh.abs())
    n_acc = n_acc_for(K, 16 if mode == "lp16" else 4) + 4
    if mode == "fp16x3":
        import split16_ref as S16
        r = S16.gemm_ref(p2, S16.pair_abs(p2), W.detach().cpu().float(), torch.zeros(W.shape[0]))
        slack = abs(g_) * sc.abs() * r[3]
    elif mode == "bf16x3":
        slack = C_SPLIT * abs(g_) * sc.abs() * amag
    else:
        slack = torch.zeros_like(mag)
    return k * f2 + g_ * y, mag, n_acc, slack


# ---- attention tail, clip pooling ----------------------------------------------------------------------------------------------
def attn_pool_ref(nodes, sqn, gsum, g_scale, g_shift, a_scale, a_shift, hw, normalise_over_parts=None):
    """agrl_attn_pool_bnneck on the kernel's own squared node norms ``sqn`` (B S P,): n = sqrt(sqn), a_sp = n_sp / max(sum_s n_sp,
    1e-12), att = (1 / P) sum_p sum_s a_sp node_sp, g = sum_s gsum_s / (S hw), out = [g g_scale + g_shift | att a_scale + a_shift]
    -> dict name -> (exact, mag, n_acc) for 'out' (B,2C; n_acc a (1,2C) tensor), 'g_f', 'att_f' (B,C).
    Roundings: sqrtf 1, the frame sum S, the quotient 1: a carries (S + 2) u; the fmaf chain over the frames S, the sum over the
    parts P, the division 1: att 2 S + P + 3. g: S additions, 1 / (S hw) rounded, the product: S + 2. The BatchNorm fmaf: + 1.
    ``normalise_over_parts`` = (b, s, p): that one weight divided by its frame's sum over the parts instead (a seeded fault)."""
    B, S, P, C = nodes.shape
    x = nodes.detach().cpu().double()
    n = sqn.detach().cpu().double().view(B, S, P, 1).sqrt()
    a = n / n.sum(1, keepdim=True).clamp(min=1e-12)
    if normalise_over_parts is not None:
        b_, s_, p_ = normalise_over_parts
        a = a.clone()
        a[b_, s_, p_] = n[b_, s_, p_] / n[b_, s_].sum().clamp(min=1e-12)
    att, amag = (a * x).sum(1).sum(1) / P, (a * x.abs()).sum(1).sum(1) / P
    gs = gsum.detach().cpu().double().view(B, S, C)
    g, gmag = gs.sum(1) / (S * hw), gs.abs().sum(1) / (S * hw)
    n_att, n_g = 2 * S + P + 3, S + 2
    gsc, gsh, asc, ash = (t.detach().cpu().double() for t in (g_scale, g_shift, a_scale, a_shift))
    out = torch.cat([g * gsc + gsh, att * asc + ash], 1)
    omag = torch.cat([gmag * gsc.abs() + gsh.abs(), amag * asc.abs() + ash.abs()], 1)
    n_out = torch.cat([torch.full((1, C), float(n_g + 1)), torch.full((1, C), float(n_att + 1))], 1).double()
    return {"out": (out, omag, n_out), "g_f": (g, gmag, n_g), "att_f": (att, amag, n_att)}


def clip_mean_ref(feats, n, denominator=None):
    """agrl_clip_pool, mode 'avg': (T n, D) -> (T, D), clips added in ascending order (n - 1 additions), one division: n + 1
    roundings allowed -> exact, mag, n_acc. ``denominator``: a seeded fault (n - 1)."""
    x = feats.detach().cpu().double().view(-1, n, feats.shape[-1])
    d = float(n if denominator is None else denominator)
    return x.sum(1) / d, x.abs().sum(1) / d, n + 1


# ---- ganet's position-attention pooling in eval, 16-bit maps --------------------------------------------------------------------
def pam_pool_ref(x, qk, splits, pam_reference):
    """agrl_pam_pool on a 16-bit map x (F,h,w,C) and its 16-bit query / key map qk (F,h,w,2Cq), both taken as the float values
    the kernel reads: xbar = X^T abar, xmean = mean_q X per pyramid slice. ``pam_reference`` = hip_ops.pam_nodes_backward_reference,
    run in float64 with selection matrices for the query / key convs so that its q / k maps ARE the given qk (needs the qk
    channels to be channels of x: qk = x[..., :2Cq], what the tests use) -> dict: xbar (exact, mag, n_acc, slack), xmean (exact,
    mag, n_acc); n_acc (1,P,1) tensors. xbar: the fmaf chain over a slice's L positions against |abar| |X| plus the softmax's
    propagated bound (pam_train_ref.attention_ref's eabar) times |X|; xmean: L additions and the quotient."""
    import pam_train_ref as PR
    F_, h, w, C = x.shape
    Cq = qk.shape[-1] // 2
    x64, qk64 = x.detach().cpu().double(), qk.detach().cpu().double()
    assert torch.equal(qk64, x64[..., :2 * Cq]), "the reference's q / k maps are selections of x"
    sel = torch.eye(C, dtype=torch.float64)
    zq = torch.zeros(Cq, dtype=torch.float64)
    P = int(sum(splits))
    ref = pam_reference(x64, sel[:Cq], zq, sel[Cq:2 * Cq], zq, torch.zeros((C, C), dtype=torch.float64), torch.zeros(C, dtype=torch.float64),
                        torch.zeros((), dtype=torch.float64), splits, torch.zeros((F_, P, C), dtype=torch.float64))
    xbm, xmm, slack = (torch.zeros((F_, P, C), dtype=torch.float64) for _ in range(3))
    nL = torch.zeros((1, P, 1), dtype=torch.float64)
    for part, (r0, r1) in enumerate(PR.slices(splits, h)):
        L = (r1 - r0) * w
        X = x64[:, r0:r1].reshape(F_, L, C)
        _, _, abar, eabar = PR.attention_ref(qk64[:, r0:r1, :, :Cq].reshape(F_, L, Cq), qk64[:, r0:r1, :, Cq:].reshape(F_, L, Cq))
        xbm[:, part] = torch.einsum('fq,fqc->fc', abar, X.abs())
        slack[:, part] = torch.einsum('fq,fqc->fc', eabar, X.abs())
        xmm[:, part] = X.abs().mean(1)
        nL[0, part, 0] = L
    return {"xbar": (ref["xbar"], xbm, nL, slack), "xmean": (ref["xmean"], xmm, nL + 1)}
