"""float64 references and fp32 chain lengths for the train-step kernels (csrc/train.hip, wgrad.hip, train_tail.hip, the fp32 /
split-bf16 uses of igemm.hip, the loss kernels of rank.hip), for ``bounds.check_rounded(..., out_dtype=torch.float32)``:

    |got - exact| <= n_acc * 2^-24 * mag (+ slack)

``exact`` is the float64 value of the kernel's stated operation on the fp32 operands it reads, ``mag`` the same operation on their
magnitudes, ``n_acc`` the longest chain of fp32 roundings the stated scheme can produce -- read off the code, derivation in
each helper's docstring. Everything here runs on the CPU; tests/test_bounds.py checks each helper against an fp32 emulation of
the stated arithmetic and against seeded faults. A plain module (like bounds.py, lp16.py): the tests import it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import graph_ref
from bounds import U32

# ---- split-bf16 products (igemm_dev.h, Frag<f32s_t>) -------------------------------------------------------------------------
# x = xh + dx, xh = x truncated to its upper 16 bits (a bf16), dx = x - xh exact in fp32, |dx| < 2^-7 |x| (bf16 keeps 8
# significand bits; truncation loses less than one unit of the last of them). xl = bf16(dx) rounded to nearest: xl = dx (1 + e),
# |e| <= 2^-8. The kernel adds xl wh + xh wl + xh wh (every product of two bf16 values is exact in the fp32 accumulator), so
#     x w - (xl wh + xh wl + xh wh) = dx dw - dx e1 wh - xh dw e2
# |dx dw| < 2^-14 |x w|; |dx e1 wh| <= 2^-7 2^-8 |x| |w| (|wh| <= |w|: truncation); the third term alike:
C_SPLIT = 2.0 ** -14 + 2 * 2.0 ** -15          # = 2^-13, per product, relative to |x| |w|


def split_bf16(v):
    """fp32 tensor -> (hi, lo) as fp32 tensors holding bf16 values: hi = upper 16 bits, lo = RNE bf16 of the exact remainder."""
    v = v.float().contiguous()
    hi = (v.view(torch.int32) & -65536).view(torch.float32)
    lo = (v - hi).to(torch.bfloat16).float()
    return hi, lo


def split_product(x, w, drop=None):
    """The three-product value xl wh + xh wl + xh wh of the split recipe in float64 (each product exact there). ``drop`` names a
    cross term to leave out ('lh' or 'hl'): the seeded fault of tests/test_bounds.py."""
    xh, xl = (t.double() for t in split_bf16(x))
    wh, wl = (t.double() for t in split_bf16(w))
    out = xh * wh
    if drop != 'lh':
        out = out + xl * wh
    if drop != 'hl':
        out = out + xh * wl
    return out


def gemm_chain(K):
    """conv_bn_act / linear_nobias / gemm_nt_splitk in fp32: one fp32 rounding per v_mfma_f32_16x16x4_f32 step of the K-deep sum
    (ceil(K / 4)) plus residual, epilogue and slack: bounds.n_acc_for(K, 4), what check_conv uses. The split mode runs three
    16-deep bf16 MFMAs per 16 values of K (3 ceil(K / 16) <= ceil(K / 4) + 3 roundings): the same count covers it."""
    return int(math.ceil(K / 4)) + 3


# ---- adversarial fp32 operands -------------------------------------------------------------------------------------------
KINDS = ("scaled", "dead", "offset", "sparse_dout")


def channel_scales(C, seed, lo=-12, hi=3):
    """Per-channel scales log-uniform over 2^lo .. 2^hi (powers of two: scaling is exact)."""
    g = torch.Generator().manual_seed(seed)
    return torch.pow(2.0, torch.randint(lo, hi + 1, (C,), generator=g).float())


def stress_train_operands(kind, shape_x, shape_dy, seed=0):
    """(x, dy) fp32 NHWC for the train kernels: x (F,H,W,Cin) an activation, dy (F,OH,OW,Cout) a gradient.
    scaled      independent per-channel scales 2^-12 .. 2^3 on x (input channels) and dy (output channels)
    dead        post-ReLU x with a third of its channels all zero (BatchNorm: var = 0, invstd = rsqrt(eps))
    offset      channels of x with mean / std in {8, 32, 128}, plus one constant channel (channel 0)
    sparse_dout dy nonzero in one frame only (the last): one pixel slice of the weight gradient carries everything"""
    g = torch.Generator().manual_seed(seed * 7919 + KINDS.index(kind))
    x = torch.randn(shape_x, generator=g)
    dy = torch.randn(shape_dy, generator=g)
    Cin, Cout = shape_x[-1], shape_dy[-1]
    if kind == "scaled":
        x = x * channel_scales(Cin, seed + 1)
        dy = dy * channel_scales(Cout, seed + 2)
    elif kind == "dead":
        x = x.relu()
        x[..., torch.arange(Cin) % 3 == 1] = 0.0
    elif kind == "offset":
        ratio = torch.tensor([8.0, 32.0, 128.0])[torch.arange(Cin) % 3]
        std = channel_scales(Cin, seed + 3, -3, 2)
        x = (x + ratio) * std
        x[..., 0] = 1.7
    elif kind == "sparse_dout":
        dy[:-1] = 0.0
    else:
        raise ValueError(kind)
    return x.contiguous(), dy.contiguous()


# ---- conv data gradient: the transposed-conv sum written out -------------------------------------------------------------
def _dgrad_sum(dy64, w64, stride, pad, H, W):
    F_, OH, OW, Cout = dy64.shape
    _, Cin, R, S = w64.shape
    hb, wb = max(H + 2 * pad, (OH - 1) * stride + R), max(W + 2 * pad, (OW - 1) * stride + S)
    buf = torch.zeros((F_, hb, wb, Cin), dtype=torch.float64)
    d2 = dy64.reshape(-1, Cout)
    for r in range(R):
        for s in range(S):
            # dx[f][oy * stride + r - pad][ox * stride + s - pad][ci] += sum_co dy[f][oy][ox][co] w[co][ci][r][s]
            buf[:, r:r + stride * OH:stride, s:s + stride * OW:stride] += (d2 @ w64[:, :, r, s]).view(F_, OH, OW, Cin)
    return buf[:, pad:pad + H, pad:pad + W]


def _dgrad_gather(dy64, w64, stride, pad, H, W, pix):
    """The same sum at the input pixels ``pix`` (flat f, iy, ix) only: per tap, the one output pixel that meets it (if any)."""
    F_, OH, OW, Cout = dy64.shape
    _, Cin, R, S = w64.shape
    f, iy, ix = pix // (H * W), pix % (H * W) // W, pix % W
    out = torch.zeros((pix.numel(), Cin), dtype=torch.float64)
    for r in range(R):
        for s in range(S):
            ty, tx = iy + pad - r, ix + pad - s
            ok = (ty >= 0) & (tx >= 0) & (ty % stride == 0) & (tx % stride == 0) & (ty // stride < OH) & (tx // stride < OW)
            g = dy64[f, (ty // stride).clamp(0, OH - 1), (tx // stride).clamp(0, OW - 1)] * ok[:, None].double()
            out += g @ w64[:, :, r, s]
    return out


def dgrad_ref(dy, w_oihw, stride, pad, H, W, residual=None, pix=None):
    """dx[f][iy][ix][ci] = sum over (oy, ox, r, s) with oy * stride + r - pad = iy, ox * stride + s - pad = ix and over co of
    dy[f][oy][ox][co] w[co][ci][r][s] (+ residual): -> exact, mag (F,H,W,Cin) float64. Pixels no output pixel reaches are exact
    zeros with mag 0 (a strided 1x1: the gradient must be exactly 0 there)."""
    if pix is not None:     # -> (len(pix), Cin): a subset of the input pixels (flat f, iy, ix), for shapes above the reference budget
        exact = _dgrad_gather(dy.double(), w_oihw.double(), stride, pad, H, W, pix)
        mag = _dgrad_gather(dy.double().abs(), w_oihw.double().abs(), stride, pad, H, W, pix)
        if residual is not None:
            r = residual.double().reshape(-1, residual.shape[-1])[pix]
            exact, mag = exact + r, mag + r.abs()
        return exact, mag
    exact = _dgrad_sum(dy.double(), w_oihw.double(), stride, pad, H, W)
    mag = _dgrad_sum(dy.double().abs(), w_oihw.double().abs(), stride, pad, H, W)
    if residual is not None:
        exact, mag = exact + residual.double(), mag + residual.double().abs()
    return exact, mag


def dgrad_chain(route, Cout, R=1, S=1, H=0, W=0):
    """fp32 roundings of each data-gradient route of HipConv2d._backward / HipConvFork._backward (one per 4-deep MFMA step, + 3
    for residual / slack as gemm_chain):
      '1x1'      linear_nobias / conv_bn_act over K = Cout (padded up to a multiple of 32 for the classifier widths)
      'flip'     stride-1 conv of dy with the flipped R x S filter: K = R S Cout
      'zero'     the same on the zero-inserted dy (7x7 / 2): the kernel still walks all R S taps
      'phase'    3x3 / 2 / 1: input pixel (iy, ix) meets 1 (even) or 2 (odd) filter rows and columns -> an (H, W, 1) tensor"""
    if route == "1x1":
        return gemm_chain(-(-Cout // 32) * 32)
    if route in ("flip", "zero"):
        return gemm_chain(R * S * Cout)
    if route == "phase":
        ty = 1 + (torch.arange(H) % 2)
        tx = 1 + (torch.arange(W) % 2)
        taps = (ty[:, None] * tx[None, :]).double()
        return (torch.ceil(taps * Cout / 4) + 3).view(1, H, W, 1)
    raise ValueError(route)


# ---- conv weight gradient ------------------------------------------------------------------------------------------------
def wgrad_ref(x, dy, R, S, stride, pad, co=None):
    """dW[co][ci][r][s] = sum over pixels p = (f, oy, ox) of dy[p][co] x[f][oy * stride + r - pad][ox * stride + s - pad][ci] in
    float64 -> exact, mag (len(co), Cin, R, S). ``co``: the output channels to evaluate (default all)."""
    F_, H, W, Cin = x.shape
    _, OH, OW, Cout = dy.shape
    co = torch.arange(Cout) if co is None else co
    xp = F.pad(x.double(), (0, 0, pad, pad, pad, pad))
    d2 = dy.double().reshape(-1, Cout)[:, co]
    d2a = d2.abs()
    exact = torch.zeros((co.numel(), Cin, R, S), dtype=torch.float64)
    mag = torch.zeros_like(exact)
    for r in range(R):
        for s in range(S):
            xs = xp[:, r:r + stride * OH:stride, s:s + stride * OW:stride].reshape(-1, Cin)
            exact[:, :, r, s] = d2.t() @ xs
            mag[:, :, r, s] = d2a.t() @ xs.abs()
    return exact, mag


def wgrad_chain(ks, cps):
    """agrl_conv_wgrad: every slice sums its cps 32-pixel k-tiles with one fp32 rounding per 4-pixel MFMA step (8 cps steps, in
    one accumulator); wgrad_reduce_kernel then adds the ks slice partials in fp32 (at most ks additions on any path: 16 lanes
    of ceil(ks / 16), then the 16 lane sums). The slices partition the pixels, so the slice errors add up to 8 cps u mag."""
    return 8 * int(cps) + int(ks)


def wgrad_channels(Cout, full, seed=0):
    """The output channels whose weight gradient is bounded: all of them when the float64 reference is within budget, otherwise
    the first and last channel of every 64- and 128-channel tile, the ragged tail past the last full 64-channel tile and a
    seeded sample of 8."""
    c = torch.arange(Cout)
    if full:
        return c
    keep = (c % 64 == 0) | (c % 64 == 63) | (c >= (Cout // 64) * 64)
    g = torch.Generator().manual_seed(seed)
    keep[torch.randint(0, Cout, (8,), generator=g)] = True
    return c[keep]


def splitk_chain(K, M, Nout):
    """agrl_gemm_nt_splitk (the weight-gradient fallback for channel counts that are not multiples of 4): K = pixels (padded to
    32) in ks slices of K / ks, ceil(K / ks / 4) roundings each, and ks - 1 additions in splitk_reduce_kernel. The slice count is
    the entry point's: doubled while ks < 256, tiles * ks < 1024, the k-tile count stays even and >= 8 per slice."""
    nk = K // 32
    tiles = (-(-M // 64)) * (-(-Nout // (64 if Nout <= 64 else 128)))
    ks = 1
    while ks < 256 and tiles * ks < 1024 and nk % (ks * 2) == 0 and nk // (ks * 2) >= 8:
        ks *= 2
    return int(math.ceil(K / ks / 4)) + ks + 3


# ---- BatchNorm reductions (colreduce_vec_kernel / colreduce_kernel + colreduce_final_kernel) ---------------------------------
def reduce_lanes(C):
    """float4 columns per block of the vectorised reduction (0: the scalar kernel) -- train.hip, reduce_lanes."""
    return 0 if C & 3 else (64 if C >= 256 else (32 if C >= 128 else 16))


def reduce_plan(M, C):
    """(chunks, rows_per_chunk, row_lanes) of train.hip's reduce_chunks: the GPU tests check ``chunks`` against the library's own
    agrl_bn_workspace(M, C) / (2 C 8 bytes)."""
    lanes = reduce_lanes(C)
    cg = -(-(C // 4) // lanes) if lanes else -(-C // 64)
    chunks = min(max(2048 // cg, 1), 512)
    rpc = (-(-M // chunks) + 15) & ~15
    return -(-M // rpc), rpc, (256 // lanes if lanes else 4)


def reduce_chain(M, C):
    """Terms a thread adds in fp32: the rows of one chunk that fall to its row lane. The four-term (or row-lane) sum and the
    partials over the chunks are double: no fp32 rounding until the result is stored."""
    _, rpc, nrl = reduce_plan(M, C)
    return -(-min(rpc, M) // nrl)


STATS_TILE_CHAIN = 128 // 16 + 4 + 4   # agrl_conv2d_stats epilogue: a lane's rows of a <= 128-row tile, 4 shuffle steps, <= 4 wave rows


def bn_stats_ref(y2d):
    """mean = sum y / M, biased var = sum y^2 / M - mean^2 of an (M, C) fp32 matrix in float64 -> dict of (exact, mag)."""
    y = y2d.double()
    M = y.shape[0]
    mean, amean = y.sum(0) / M, y.abs().sum(0) / M
    sq = (y * y).sum(0) / M
    return {"mean": (mean, amean), "var": (sq - mean * mean, sq + mean * mean)}


def bn_stats_chain(n_thread):
    """mean: n_thread fp32 additions, one rounding of the double result to fp32 (+ 1 slack). var: sum y^2 by n_thread fmas
    (error <= n_thread u sum y^2 / M); the double mean mu carries n_thread u sum |y| / M, so mu^2 carries
    2 |mu| n_thread u sum |y| / M <= 2 n_thread u sum y^2 / M (Cauchy-Schwarz); one rounding of the result: 3 n_thread + 2
    against mag = sum y^2 / M + mean^2."""
    return {"mean": n_thread + 2, "var": 3 * n_thread + 2}


def bn_backward_sums_ref(dz, y2d, mean, invstd):
    """dbeta = sum dz, dgamma = sum dz xhat, xhat = (y - mean) invstd on the kernel's own fp32 mean / invstd -> dict of (exact, mag)."""
    d, xh = dz.double(), (y2d.double() - mean.double()) * invstd.double()
    return {"dbeta": (d.sum(0), d.abs().sum(0)), "dgamma": ((d * xh).sum(0), (d * xh).abs().sum(0))}


def bn_backward_sums_chain(n_thread, leaky):
    """dbeta: n_thread additions + the final rounding (+ 1 when dz = slope dout is itself rounded). dgamma: xhat costs two
    roundings (subtract, multiply) before the fma chain of n_thread."""
    k = 1 if leaky else 0
    return {"dbeta": n_thread + 1 + k, "dgamma": n_thread + 3 + k}


RSQRT_ULPS = 2   # rsqrtf is not correctly rounded; the device-library documentation is not on the test machines: 2 ulp allowed


def bn_fold_ref(mean, var, gamma, beta, eps, momentum, n, running_mean=None, running_var=None, unbias=True):
    """bn_fold_train_kernel in float64 on the fp32 operands (eps, momentum and n / (n - 1) as the fp32 values the kernel gets):
    invstd = 1 / sqrt(var + eps), scale = gamma invstd, shift = beta - mean scale, running = (1 - m) running + m {mean,
    var n / (n - 1)}; n = 1: the kernel's convention is the factor 1 (the formula has no value there and nn.BatchNorm refuses
    such a batch). -> dict name -> (exact, mag, n_acc). ``unbias=False`` leaves the factor out (a seeded fault).
    n_acc: invstd = one rounding of var + eps (worth half of it after the square root, counted whole) + RSQRT_ULPS ulp = 2
    RSQRT_ULPS half-ulps; scale one more; shift = beta - mean scale: scale's error, the product, the difference, against
    |beta| + |mean scale|; running: 1 - m, its product, the fma (+ the rounded factor and var * factor for the variance)."""
    e32, m32 = float(np.float32(eps)), float(np.float32(momentum))
    ub = float(np.float32(float(n) / float(n - 1))) if (n > 1 and unbias) else 1.0
    mu, v, g, b = mean.double(), var.double(), gamma.double(), beta.double()
    inv = 1.0 / torch.sqrt(v + e32)
    k_inv = 1 + 2 * RSQRT_ULPS
    out = {"invstd": (inv, inv.abs(), k_inv), "scale": (g * inv, (g * inv).abs(), k_inv + 1),
           "shift": (b - mu * g * inv, b.abs() + (mu * g * inv).abs(), k_inv + 3)}
    if running_mean is not None:
        rm, rv = running_mean.double(), running_var.double()
        out["running_mean"] = ((1 - m32) * rm + m32 * mu, (1 - m32) * rm.abs() + m32 * mu.abs(), 3)
        out["running_var"] = ((1 - m32) * rv + m32 * v * ub, (1 - m32) * rv.abs() + m32 * v * ub, 5)
    return out


def bn_apply_ref(y2d, scale, shift, residual, relu, slope=0.0):
    """act(fmaf(y, scale, shift) + residual), act = identity / ReLU / LeakyReLU(slope): at most 3 roundings (fma, residual add,
    slope multiply; 0 < slope <= 1 and the activation is 1-Lipschitz, so a pre-activation whose sign differs from the exact
    one is still within the bound) -> exact, mag, n_acc."""
    pre = y2d.double() * scale.double() + shift.double()
    mag = (y2d.double() * scale.double()).abs() + shift.double().abs()
    if residual is not None:
        pre, mag = pre + residual.double(), mag + residual.double().abs()
    if relu:
        pre = torch.where(pre > 0, pre, pre * float(np.float32(slope)))
    return pre, mag, 3


def unpack_sign_mask(mask, numel):
    """agrl_bn_apply's mask: bit (i & 7) of byte (i >> 3) is set where the pre-activation of element i (linear order) is positive
    (float4 number e owns nibble e & 1 of byte e >> 1, component j its bit j) -> bool (numel,)."""
    bits = np.unpackbits(mask.detach().cpu().numpy().reshape(-1), bitorder="little")
    return torch.from_numpy(bits[:numel].astype(np.bool_))


def pack_sign_mask(positive):
    """The inverse: bool (numel,) -> uint8 ((numel + 7) // 8,), unused bits 0."""
    return torch.from_numpy(np.packbits(positive.detach().cpu().numpy().reshape(-1).astype(np.uint8), bitorder="little"))


def bn_backward_ref(dz, y2d, mean, invstd, gamma, s1, s2):
    """dy = gamma invstd (dz - s1 / M - xhat s2 / M) on the kernel's own fp32 mean, invstd, s1 = dbeta, s2 = dgamma -> exact,
    mag, n_acc. Roundings: 1 / M, s1 / M (2 on that term), xhat (2), s2 / M (2), their product (1) (5 on that term), the two
    subtractions (2), gamma invstd and the outer product (2): <= 10 against mag = |gamma invstd| (|dz| + |s1| / M + |xhat s2| / M)."""
    M = y2d.shape[0]
    xh = (y2d.double() - mean.double()) * invstd.double()
    gi = gamma.double() * invstd.double()
    exact = gi * (dz.double() - s1.double() / M - xh * (s2.double() / M))
    mag = gi.abs() * (dz.double().abs() + s1.double().abs() / M + (xh * s2.double()).abs() / M)
    return exact, mag, 10


# ---- 3x3 / stride 2 / pad 1 max pooling: exact ---------------------------------------------------------------------------
def maxpool_ref(x, last=False):
    """out, idx (F,OH,OW,C): the window maximum and its tap r * 3 + s -- the FIRST maximum in scan order (strict >; the first
    tap inside the frame always taken). ``last=True`` takes the last maximum instead (>=): a seeded fault."""
    F_, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.full((F_, 2 * OH + 1, 2 * OW + 1, C), float("-inf"), dtype=x.dtype)
    ok = torch.zeros((1, 2 * OH + 1, 2 * OW + 1, 1), dtype=torch.bool)
    xp[:, 1:H + 1, 1:W + 1] = x
    ok[:, 1:H + 1, 1:W + 1] = True
    best = torch.full((F_, OH, OW, C), float("-inf"), dtype=x.dtype)
    idx = torch.zeros((F_, OH, OW, C), dtype=torch.uint8)
    seen = torch.zeros((F_, OH, OW, C), dtype=torch.bool)
    for r in range(3):
        for s in range(3):
            v = xp[:, r:r + 2 * OH:2, s:s + 2 * OW:2]
            inside = ok[:, r:r + 2 * OH:2, s:s + 2 * OW:2].expand_as(v)
            take = inside & (~seen | ((v >= best) if last else (v > best)))
            best = torch.where(take, v, best)
            idx = torch.where(take, torch.full_like(idx, r * 3 + s), idx)
            seen = seen | inside
    return best, idx


def maxpool_backward_ref(dout, idx, H, W):
    """dx[f][ih][iw][c] = sum of dout over the windows whose recorded tap is (ih, iw), added in fp32 in the kernel's order
    (window rows ascending, then columns): bitwise what maxpool_bwd_kernel computes."""
    F_, OH, OW, C = dout.shape
    buf = torch.zeros((F_, 2 * OH + 1, 2 * OW + 1, C), dtype=torch.float32)
    for r in (2, 1, 0):           # input row ih = 2 oh - 1 + r: the larger tap row belongs to the smaller oh
        for s in (2, 1, 0):
            buf[:, r:r + 2 * OH:2, s:s + 2 * OW:2] += torch.where(idx == r * 3 + s, dout, torch.zeros_like(dout))
    return buf[:, 1:H + 1, 1:W + 1].contiguous()


# ---- tail and losses (train_tail.hip, gcn.hip gram_kernel<true>, rank.hip) -------------------------------------------------
def axpby_ref(a, x, b, y):
    """fmaf(a, x, b y) (or a x): two roundings; a, b as the fp32 values the kernel gets -> exact, mag, n_acc."""
    a, b = float(np.float32(a)), float(np.float32(b))
    if y is None:
        return a * x.double(), (a * x.double()).abs(), 1
    return a * x.double() + b * y.double(), (a * x.double()).abs() + (b * y.double()).abs(), 2


def pool_bins(splits, h):
    return [((j * h) // n, -(-((j + 1) * h) // n)) for n in splits for j in range(n)]


def part_pool_backward_ref(dg, dnodes, S, h, w, splits):
    """dx1[f][pix][c] = dg[f / S][c] / (S h w) (the reciprocal rounded once, one product: 2 roundings + 1 slack); dx2[f][pix][c] =
    sum over the parts whose row band holds pix of dnodes[f][part][c] / (rows w): one division and one addition per part ->
    (exact1, mag1, n1), (exact2, mag2, n2), NHWC float64."""
    F_, P, C = dnodes.shape
    one = None
    if dg is not None:
        e = (dg.double() / (S * h * w)).repeat_interleave(S, 0).view(F_, 1, 1, C).expand(F_, h, w, C)
        one = (e, e.abs(), 3)
    e2 = torch.zeros((F_, h, w, C), dtype=torch.float64)
    m2 = torch.zeros_like(e2)
    for p, (lo, hi) in enumerate(pool_bins(splits, h)):
        t = dnodes[:, p].double() / ((hi - lo) * w)
        e2[:, lo:hi] += t.view(F_, 1, 1, C)
        m2[:, lo:hi] += t.abs().view(F_, 1, 1, C)
    return one, (e2, m2, 2 * len(splits))


def pair_product_ref(a, b):
    """out[t] = a[t] b[t]^T: 128-channel slices by v_mfma_f32_16x16x4_f32 (32 roundings each), the C / 128 slice partials added
    in fp32 -> exact, mag, n_acc. The slice errors add up to 32 u mag (the slices partition the channels)."""
    C = a.shape[-1]
    return (torch.bmm(a.double(), b.double().transpose(1, 2)), torch.bmm(a.double().abs(), b.double().abs().transpose(1, 2)),
            32 + C // 128 + 3)


def xent_ref(logits, targets, eps):
    """loss = mean_i sum_k -q_ik log p_ik, q = (1 - eps) onehot + eps / K, dlogits = (p - q) / n in float64, and the bounds of
    xent_rows_kernel's arithmetic -> (loss, loss_bound), (dlogits, dlogits_bound) (absolute bounds, for check_rounded's slack).
    With t = ceil(K / 256) + 8 the terms a thread and the wave / block tree add: se = sum exp(z - m) carries relative
    (t + 3) u (the subtraction and expf at <= 1 ulp = 2 u each, exp(z - m) <= 1), so lse = m + log se carries
    d_lse = (t + 3) u + 2 u |log se| + u |lse| (log's derivative 1 / se, logf <= 1 ulp, the addition). p = expf(z - lse):
    |dp| <= p (d_lse + u |z - lse| + 2 u); q costs 2 u q (eps / K, the sum); the difference, 1 / n and the product one each.
    Row loss -(1 - eps)(z_y - lse) - (eps / K)(sum z - K lse): sum z carries t u sum |z|, each product / difference one more."""
    n, K = logits.shape
    z = logits.double()
    e32 = float(np.float32(eps))
    lse = torch.logsumexp(z, 1, keepdim=True)
    p = torch.exp(z - lse)
    q = torch.full_like(p, e32 / K)
    q[torch.arange(n), targets.long()] += 1 - e32
    t = -(-K // 256) + 8
    m = z.max(1, keepdim=True).values
    d_lse = U32 * ((t + 3) + 2 * (lse - m).abs() + lse.abs())
    dl = (p - q) / n
    dl_bound = (p * (d_lse + U32 * (z - lse).abs() + 2 * U32) + 2 * U32 * q + 3 * U32 * (p + q)) / n
    zy = z[torch.arange(n), targets.long()].view(n, 1)
    sz = z.sum(1, keepdim=True)
    row = -(1 - e32) * (zy - lse) - (e32 / K) * (sz - K * lse)
    row_bound = ((1 - e32) * (d_lse + 3 * U32 * (zy.abs() + lse.abs()))
                 + (e32 / K) * (t * U32 * z.abs().sum(1, keepdim=True) + K * d_lse + 4 * U32 * (sz.abs() + K * lse.abs()))
                 + 2 * U32 * row.abs())
    loss = row.mean()
    loss_bound = row_bound.mean() + (n + 1) * U32 * row.abs().mean()
    return (loss.view(1), loss_bound.view(1)), (dl, dl_bound)


def check_sign_mask(mask, out, name=""):
    """agrl_bn_apply's sign mask against ``pre-activation > 0`` recomputed from the kernel's own output (ReLU: out > 0; LeakyReLU
    with a positive slope keeps the sign): bit-exact, unused bits of the last byte zero."""
    want = pack_sign_mask(out.detach().cpu().reshape(-1) > 0)
    got = mask.detach().cpu().reshape(-1)
    assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
    bad = torch.nonzero(got != want).reshape(-1)
    assert bad.numel() == 0, "%s: %d of %d mask bytes differ from out > 0, first at byte %d (elements %d..): got 0x%02x want 0x%02x" % (
        name, bad.numel(), got.numel(), int(bad[0]), 8 * int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


def attn_pool_backward_ref(nodes, g):
    """nodes (B,S,P,C), g = d loss / d att_f (B,C): n_sp = |f_sp|, N_p = sum_s n_sp, a_sp = n_sp / N_p, u_sp = g . f_sp,
    ubar_p = sum_s a_sp u_sp,  d f_sp = (a_sp / P) g + k_sp f_sp,  k_sp = (u_sp - ubar_p) / (P N_p n_sp) -- by the kernel's
    convention k_sp = 0 where n_sp == 0 (an all-zero node: its norm passes no gradient) or N_p <= 1e-12 -> exact, mag, n_acc.
    With t = 4 ceil(C / 256) + 6 the fmas of a lane and the steps of the wave sum: n carries (t / 2 + 1) u <= (t + 2) u, u_sp
    carries t u U_sp (U = sum |g| |f|), N (t + 2 + S) u, a e_a = (2 t + S + 5) u, ubar (e_a + S u + t u) Ubar (Ubar = sum_s a
    U), the numerator of k (3 t + 2 S + 6) u (U + Ubar), its denominator (2 t + S + 8) u, the two products and the fma 2 u: at
    most (5 t + 3 S + 16) u against mag = (a / P) |g| + |f| (U + Ubar) / (P N n)."""
    B, S, P, C = nodes.shape
    f, gg = nodes.double(), g.double().view(B, 1, 1, C)
    n = f.pow(2).sum(3, keepdim=True).sqrt()
    N = n.sum(1, keepdim=True)
    live = (n > 0) & (N > 1e-12)
    a = n / N.clamp(min=1e-12)
    u, U = (gg * f).sum(3, keepdim=True), (gg * f).abs().sum(3, keepdim=True)
    ubar, Ubar = (a * u).sum(1, keepdim=True), (a * U).sum(1, keepdim=True)
    den = (P * N * n).clamp(min=1e-300)
    k = torch.where(live, (u - ubar) / den, torch.zeros_like(u))
    kmag = torch.where(live, (U + Ubar) / den, torch.zeros_like(u))
    t = 4 * (-(-C // 256)) + 6
    return a / P * gg + k * f, a / P * gg.abs() + kmag * f.abs(), 5 * t + 3 * S + 16


def triplet_ref(x, pids, margin, soft, dist_ap, dist_an, idx_ap, idx_an):
    """agrl_triplet_loss against its stated formulas (rank.hip), on the kernel's own mined pairs and distances:
      mining   d_ij = sqrt(max(|x_i|^2 + |x_j|^2 - 2 x_i . x_j, 1e-12)); the float64 distance at the kernel's hardest positive
               (negative) must be the float64 maximum (minimum) up to twice the bound of a distance, and the kernel's own
               d_ap / d_an within that bound of float64: d^2 carries (t + 3) u (|x_i|^2 + |x_j|^2 + 2 sum |x_i x_j|) with
               t = ceil(d / 64) + 6 (a lane's fmas + the wave sum), the square root halves the relative error: / (2 d)
      loss     mean_i log(1 + exp(d_ap - d_an)) (soft) or mean_i max(0, d_ap - d_an + margin): expf / logf at <= 1 ulp each
               and the difference, then n additions and the division
      gradient grad[r] = ca[r] (x_r - x_p(r)) + cn[r] (x_r - x_q(r)) - sum_{i: p(i) = r} ca[i] (x_i - x_r)
               - sum_{i: q(i) = r} cn[i] (x_i - x_r), ca = g / (n d_ap), cn = -g / (n d_an) (0 where the distance is at the
               clamp, sqrt(1e-12): a constant there), g = sigmoid(d_ap - d_an) or [L > 0]: a coefficient costs <= 8 u (difference,
               expf 2, 1 + e, quotient, n d, quotient + 1), each term one difference and one fma, at most 2 + 2 n terms.
    -> dict name -> (exact, mag or None, n_acc, slack or None)."""
    n, d = x.shape
    X = x.double()
    sq = (X * X).sum(1)
    d2 = sq[:, None] + sq[None, :] - 2 * X @ X.t()
    m2 = sq[:, None] + sq[None, :] + 2 * X.abs() @ X.abs().t()
    D = d2.clamp(min=1e-12).sqrt()
    t = -(-d // 64) + 6
    dbound = (t + 3) * U32 * m2 / (2 * D) + U32 * D
    same = pids.view(-1, 1) == pids.view(1, -1)
    ar = torch.arange(n)
    ip, iq = idx_ap.long(), idx_an.long()
    out = {"mining": (D, dbound, same), "dist_ap": (D[ar, ip], None, 0, dbound[ar, ip]), "dist_an": (D[ar, iq], None, 0, dbound[ar, iq])}
    ap, an = dist_ap.double(), dist_an.double()
    if soft:
        L = torch.log1p(torch.exp(ap - an))
        gcoef = torch.sigmoid(ap - an)
        lb = U32 * (ap.abs() + an.abs()) * gcoef + 5 * U32 * L
    else:
        m32 = float(np.float32(margin))
        L = (ap - an + m32).clamp(min=0)
        gcoef = (L > 0).double()
        lb = 2 * U32 * (ap.abs() + an.abs() + m32)
    out["loss"] = (L.mean().view(1), None, 0, (lb.mean() + (n + 1) * U32 * L.mean()).view(1))
    tiny = float(np.sqrt(np.float32(1e-12)))
    ca = torch.where(ap > tiny, gcoef / (n * ap), torch.zeros_like(ap))
    cn = torch.where(an > tiny, -gcoef / (n * an), torch.zeros_like(an))
    G, Gm = torch.zeros((n, d), dtype=torch.float64), torch.zeros((n, d), dtype=torch.float64)
    for i in range(n):
        for c, j in ((ca[i], int(ip[i])), (cn[i], int(iq[i]))):
            v = c * (X[i] - X[j])
            G[i] += v
            G[j] -= v
            Gm[i] += v.abs()
            Gm[j] += v.abs()
    out["grad"] = (G, Gm, 8 + 2 * (2 + 2 * n), None)
    return out


def graph_matrix_backward_ref(gram_part, dG, use_pose, mask_diag=False):
    """agrl_graph_matrix_backward from the kernel's own Gram partials (B,nz,V,V) and dG (B,V,V), in float64, by the formulas of
    its header comment:  g = sum_z gram_part, D2_ij = g_ii + g_jj - 2 g_ij, D = sqrt(max(D2, 1e-12)), S = 2 / (exp(D) + 1),
    r_i = sum_j S_ij, Shat = S / r_i, dShat = dG (1/2 with the pose graph), dS_ij = (dShat_ij - sum_k dShat_ik Shat_ik) / r_i,
    dD = -S (1 - S / 2) dS, E_ij = dD_ij / (2 D_ij), T = E + E^T, M = 2 (diag(rowsum T) - T). Convention (the kernel's, stated
    there): E_ii = 0 -- D2_ii is identically 0, so the diagonal passes no gradient although sqrt'(clamp) of the fp32 noise the
    reference's autograd sees there is huge -- and E_ij = 0 wherever D2_ij is at the clamp.
    -> exact M, an absolute bound for check_rounded's ``slack``. The bound is the first-order propagation of each fp32 step's
    rounding through the formulas above (t = ceil(V / 64) + 6: a lane's terms + the wave sum):
      g: nz u sum_z |part|;  D2: those of g_ii, g_jj, 2 g_ij + 2 u (g_ii + g_jj + 2 |g_ij|);  D: dD2 / (2 D) + u D;
      S: |S'| dD + 4 u S (expf at 1 ulp, the sum, the quotient), S' = -S (1 - S / 2);  r: sum_j dS_ij + t u r;
      Shat: S / r (dS / S + dr / r + u);  c_i = sum_k dShat Shat: sum |dShat| dShat_err + t u sum |dShat Shat|;
      dS: (dc + u (|dShat| + |c|)) / r + |dS| (dr / r + u);  dD: |dS| (|1 - S| dS_err + 3 u h) + h ddS + u |dD|, h = S (1 - S / 2);
      E: ddD / (2 D) + |E| (dD_err / D + 2 u);  T: dE_ij + dE_ji + u |T|;  rowsum: sum_j dT_ij + t u sum_j |T_ij|;
      M: 2 (drowsum [i = j] + dT) + u |M|.
    The D2 step is the ill-conditioned one (similar nodes: D2 << g_ii + g_jj); the bound carries that conditioning. The stages up
    to Shat are graph_ref.similarity_chain (shared with the forward reference graph_ref.graph_matrix_ref)."""
    u = U32
    V = gram_part.shape[-1]
    ch = graph_ref.similarity_chain(*graph_ref.gram_from_partials(gram_part), mask_diag=mask_diag)   # up to Shat: one copy, shared with the forward reference
    D, eD, S, h, eS, r, er, Sh, eSh, live = (ch[k] for k in ("D", "eD", "S", "h", "eS", "r", "er", "Sh", "eSh", "live"))
    t = -(-V // 64) + 6
    x = dG.double() * (0.5 if use_pose else 1.0)
    c = (x * Sh).sum(2, keepdim=True)
    ec = (x.abs() * eSh).sum(2, keepdim=True) + t * u * (x * Sh).abs().sum(2, keepdim=True)
    dS = (x - c) / r
    edS = (ec + u * (x.abs() + c.abs())) / r + dS.abs() * (er / r + u)
    dD = -h * dS
    edD = dS.abs() * ((1 - S).abs() * eS + 3 * u * h) + h * edS + u * dD.abs()
    E = torch.where(live, dD / (2 * D), torch.zeros_like(D))
    eE = torch.where(live, edD / (2 * D) + E.abs() * (eD / D + 2 * u), torch.zeros_like(D))
    T = E + E.transpose(1, 2)
    eT = eE + eE.transpose(1, 2) + u * T.abs()
    rs = T.sum(2)
    ers = eT.sum(2) + t * u * T.abs().sum(2)
    M = 2 * (torch.diag_embed(rs) - T)
    eM = 2 * (torch.diag_embed(ers) + eT) + u * M.abs()
    return M, eM, live
