"""The arithmetic contract of the split-fp16 mode (hip_precision = "fp16x3") and its element-by-element bound: float64 references
of every kernel form, the per-product error model, operand generators and a CPU emulation of the recipe with one switch per defect.

THE RECIPE (csrc/igemm_dev.h, Frag<f32h_t>; csrc/fat_dev.h, split16_pack8; hip_ops.split16_plane_weights). An fp32 value x is carried
as two fp16 halves, xh = rne16(x) and xl = rne16(x - xh) (the difference is exact in fp32: xh keeps 11 of x's 24 significand bits). A
weight is first multiplied by ONE power of two per tensor, W = w 2^k with max |W| in [2^13, 2^14) (hip_ops.split16_prescale: exact),
then split the same way; the epilogue multiplies the accumulator by 2^-k (exact). A product is three fp16 MFMAs into one fp32
accumulator, the small terms first:  xl Wh + xh Wl + xh Wh.  A product of two fp16 values is exact in fp32 (11 + 11 bits).
  In-loop kernels (agrl_conv2d_bn_act_split16, agrl_conv1x1_dual_split16, the stem) split the fp32 activations in the k-loop.
  Plane kernels read activations ALREADY split, as planes [hi | lo 2^11 | hi] (or the pair [hi | lo 2^11]) with lo 2^11 = rne16((x -
xh) 2^11), against weight columns [Wh | Wh 2^-11 | Wl] (Whs = rne16(Wh 2^-11)): xh Wh + (xl 2^11) Whs + xh Wl.

THE SPLIT OF ONE OPERAND. Let 2^E <= |x| < 2^(E+1) with E >= -14 (xh a normal fp16). fp16 numbers are 2^(E-10) apart there, so d = x - xh
has |d| <= 2^(E-11) <= 2^-11 |x|, and |xl| <= 2^-11 |x| as well (rounding is monotone and 2^(E-11) is an fp16 number). If |d| = 2^(E-11), xl =
d. Otherwise d lies in a binade below 2^(E-11), where fp16 numbers are at most 2^(E-22) apart PROVIDED d is a normal fp16 (|d| >= 2^-14):
      ex = x - xh - xl,   |ex| <= 2^(E-23) <= 2^-23 |x|        (xl normal)
Below that fp16's subnormal spacing 2^-24 takes over:  |ex| <= 2^-25 ABSOLUTE, |xl| <= |d| + 2^-25 (xl not a normal fp16; this
includes every |x| < 2^-3, the statement of igemm_dev.h). For the planes the low half is stored times 2^11, so the absolute case
starts 2^11 lower and is 2^11 smaller: 2^-36. Write  |ex| <= 2^-23 |x| + ax,  |xl| <= 2^-11 |x| + ax  with ax = 0 where xl is a
normal fp16 or d = 0, else A_LO = 2^-25 (pair_abs). The same holds for W with eW, aW.

ONE PRODUCT. (xh + xl)(Wh + Wl) = (x - ex)(W - eW); the kernel leaves out xl Wl:
      x W - (xl Wh + xh Wl + xh Wh) = ex W + x eW - ex eW + xl Wl
      |..| <= |x| |W| (2^-23 + 2^-23 + 2^-22 + 2^-46) + (1 + 2^-11 + 2^-23) (ax |W| + aW |x|) + 2 ax aW
so the relative constant is C_SPLIT16 = 2^-21 (1 + 2^-20) -- two operand splits of 2^-23 each and the dropped low x low term of 2^-22
-- and the absolute terms are (1 + 2^-10) (ax |W| + aW |x|) + 2 ax aW in the SCALED weight's units, times 2^-k in the output's. (A split
that kept only 2^-22 per operand, as a truncated high half does, would give 3 2^-22.) A plane kernel reads its activation planes, so
the reference takes the value the planes hold, xv = hi + lo 2^-11, as the operand and ex = 0 there; what remains is x eW, the dropped
term and (xl 2^11)(Whs - Wh 2^-11), which is zero where Wh 2^-11 is a normal fp16 (|Wh| >= 2^-3) and at most |x| 2^-25 otherwise: one more
A_LO in aW. The constant is kept at C_SPLIT16 for every form.
  A plane OUTPUT adds its own split: hi + lo 2^-11 reproduces the fp32 result to 2^-22 relative, 2^-36 absolute (PLANE_REL, PLANE_ABS:
the allowance the plane layout is documented with; the derivation above gives 2^-23), and |lo 2^-11| <= half an fp16 ulp of hi -- the
mark of a high half rounded to NEAREST (canonical_halves).

THE CHAIN. bounds.n_acc_for(K, 16) counts the fp32 roundings of one chain of K products through 16-deep MFMA steps, + 3 for bias,
residual and slack. Here three MFMAs per step add into the one accumulator (Frag<f32h_t>::mma: three per 16 products; mma32 and the
plane kernels' 3 K columns: three per 32, fewer), and each of the two small-term results meets the accumulator in one more rounded
addition per step: 2 ceil(K / 16) of them.  n_acc = n_acc_for(K, 16) + 2 ceil(K / 16) = 3 ceil(K / 16) + 3  (n_acc_split16).

Nothing here is fitted to a kernel's output. A plain module (like train_ref.py, graph_ref.py): the tests import it."""
import math

import torch
import torch.nn.functional as F

from bounds import check_rounded, half_ulp, n_acc_for

C_SPLIT16 = 2.0 ** -21 * (1 + 2.0 ** -20)   # per product, relative to |x| |w|
A_LO = 2.0 ** -25                           # |ex| where the low half is not a normal fp16 (in the operand's own units)
ABS_FACTOR = 1 + 2.0 ** -10
PLANE_REL, PLANE_ABS = 2.0 ** -22, 2.0 ** -36  # what a plane pair / triple loses of the fp32 value it stores
F16_MIN_NORMAL = 2.0 ** -14

KINDS = ("plain", "coherent_lo", "tiny", "small_rows", "wide_range")
DEFECTS = ("a", "b", "c", "d", "e", "f")
DEFECT_NAMES = {"a": "xh wl dropped", "b": "xl wh dropped", "c": "hi truncated, not rounded to nearest", "d": "plane lo stored without 2^11",
                "e": "weights not pre-scaled", "f": "one 128-channel slab reads hi where lo belongs"}


def n_acc_split16(K, extra=0):
    return n_acc_for(K, 16) + 2 * int(math.ceil(K / 16)) + extra


class Ref(tuple):
    """(exact, mag, n_acc, slack) in float64; ``.abs_slack`` is the part of slack made of the absolute terms alone."""
    def __new__(cls, exact, mag, n_acc, slack, abs_slack):
        self = super().__new__(cls, (exact, mag, n_acc, slack))
        self.abs_slack = abs_slack
        return self


# ---- the split itself ---------------------------------------------------------------------------------------------------------------
def rne16(v):
    return v.to(torch.float16).float()


def trunc16(v):
    """fp32 -> the fp16 value nearest to zero-wards (defect (c)), as fp32."""
    h = v.to(torch.float16)
    over = h.float().abs() > v.abs()
    bits = h.view(torch.int16) - over.to(torch.int16)     # sign-magnitude: one step towards zero
    return bits.view(torch.float16).float()


def split16(v, lo_scale=1.0, trunc=False):
    """fp32 -> (hi, lo lo_scale) as fp32 tensors holding fp16 values; the recipe's arithmetic is fp32 throughout."""
    v = v.float()
    hi = trunc16(v) if trunc else rne16(v)
    return hi, rne16((v - hi) * lo_scale)


def pair_abs(v, lo_scale=1.0):
    """float64 ax of the model: 0 where the (stored) low half of v is a normal fp16 or there is none, else A_LO / lo_scale."""
    v = v.float()
    d = (v - rne16(v)).double() * lo_scale
    return torch.where((d.abs() >= F16_MIN_NORMAL) | (d == 0), torch.zeros_like(d), torch.full_like(d, A_LO / lo_scale))


def prescale_exp(w):
    """k of hip_ops.split16_prescale."""
    amax = float(w.detach().abs().max())
    return 13 - math.frexp(amax)[1] + 1 if (amax > 0.0 and math.isfinite(amax)) else 0


def weight_abs(w, planes=False, k=None):
    """aW 2^-k per weight, float64, in the TRUE weight's units; (k, aW). ``planes``: + A_LO where Wh 2^-11 is not a normal fp16.
    ``k``: the pre-scale's exponent where the host does not take it from max |w| (the cosine distance: 13)."""
    k = prescale_exp(w) if k is None else k
    W = w.float() * 2.0 ** k
    a = pair_abs(W)
    if planes:
        a = a + torch.where((rne16(W).abs() < 2.0 ** -3) & (W != 0), torch.full_like(a, A_LO), torch.zeros_like(a))
    return k, a * 2.0 ** -k


def planes_value(hi, lo_scaled):
    return hi.double() + lo_scaled.double() * 2.0 ** -11


def canonical_halves(hi, lo, name=""):
    """The high half is the value rounded to NEAREST: the (unscaled) low half is at most half an fp16 ulp of it."""
    hi, lo = hi.detach().cpu().double(), lo.detach().cpu().double()
    hu = torch.where(hi == 0, torch.full_like(hi, 2.0 ** -25), half_ulp(hi, torch.float16))
    bad = lo.abs() > hu
    assert not bool(bad.any()), "%s: %d of %d low halves exceed half an ulp of their high half (first at flat %d)" % (
        name, int(bad.sum()), bad.numel(), int(torch.nonzero(bad.reshape(-1))[0]))


def plane_out_slack(exact):
    return PLANE_REL * exact.abs() + PLANE_ABS


def presplit_out_slack(exact):
    """An output stored PRE-SPLIT (hi, lo unscaled: the in-loop layout) is the fp32 result split as an operand is: 2^-23 relative, and
    A_LO absolute wherever its low half is not a normal fp16 (every output below 2^-3)."""
    return 2.0 ** -23 * exact.abs() + A_LO


# ---- references ---------------------------------------------------------------------------------------------------------------------
def _finish(acc, pmag, t_abs, b, res, relu, K, extra=0):
    b64 = b.detach().cpu().double()
    exact, mag = acc + b64, pmag + b64.abs()
    if res is not None:
        exact, mag = exact + res, mag + res.abs()
    if relu:
        exact = exact.relu()
    return Ref(exact, mag, n_acc_split16(K, extra), C_SPLIT16 * pmag + t_abs, t_abs)


def gemm_ref(a, ax, w, b, res=None, relu=False, planes=False, extra=0, k=None):
    """act(a w^T + b + res): a (P, K) the activation operand's values, ax (P, K) its absolute split term (zeros for planes), w (Cout, K)
    the TRUE fp32 weights, res (P, Cout) float64 or None."""
    a, ax, w64 = a.detach().cpu().double(), ax.detach().cpu().double(), w.detach().cpu().double()
    _, aw = weight_abs(w.detach().cpu(), planes, k)
    pmag = a.abs() @ w64.abs().t()
    t_abs = ABS_FACTOR * (ax @ w64.abs().t() + a.abs() @ aw.t()) + 2 * ax @ aw.t()
    return _finish(a @ w64.t(), pmag, t_abs, b, None if res is None else res.detach().cpu().double(), relu, w.shape[1], extra)


def inloop_conv_ref(x, w, b, stride=1, pad=0, res=None, relu=False, pixels=None):
    """agrl_conv2d_bn_act_split16 on fp32 NHWC x, OHWI TRUE weights w (split16_true_weights), fp32 bias, NHWC residual -> Ref of
    (P, Cout) + pixels + coords (test_gpu_kernels.conv_exact does the float64 work)."""
    from test_gpu_kernels import conv_exact
    nchw = lambda t: t.detach().cpu().permute(0, 3, 1, 2)
    xc, wc = nchw(x).float(), nchw(w).float()
    zero = torch.zeros(w.shape[0])
    rc = None if res is None else nchw(res)
    exact, mag, pix, coords = conv_exact(xc, wc, b, stride, pad, rc, relu, pixels)
    _, aw = weight_abs(wc)
    ax = pair_abs(xc)
    t1, _, _, _ = conv_exact(ax, wc.double().abs() * ABS_FACTOR + 2 * aw, zero, stride, pad, pixels=pix)
    t2, _, _, _ = conv_exact(xc.double().abs(), aw * ABS_FACTOR, zero, stride, pad, pixels=pix)
    t_abs = t1 + t2
    pmag = mag - b.detach().cpu().double().abs()
    if rc is not None:
        n, oh, ow = coords[:, 0], coords[:, 1], coords[:, 2]
        pmag = pmag - rc.double()[n, :, oh, ow].abs()
    K = w.shape[1] * w.shape[2] * w.shape[3]
    return Ref(exact, mag, n_acc_split16(K), C_SPLIT16 * pmag + t_abs, t_abs), pix, coords


def dual_inloop_ref(x, x2, w_cat, b, stride, relu=True):
    """agrl_conv1x1_dual_split16: [x sampled at the stride | x2] (fp32 NHWC) against TRUE w_cat (Cout, K1 + K2)."""
    a = torch.cat([x[:, ::stride, ::stride, :].reshape(-1, x.shape[3]), x2.reshape(-1, x2.shape[3])], dim=1).detach().cpu().float()
    return gemm_ref(a, pair_abs(a), w_cat, b, relu=relu)


def plane_gemm_ref(xvs, w, b, res_v=None, relu=True):
    """agrl_conv1x1_split16 / _dual: xvs = the values the activation planes hold (from_split16_planes), one (M, K_i) per source; w
    (Cout, sum K_i) TRUE weights; res_v (M, Cout) the residual planes' values."""
    a = torch.cat([t.detach().cpu().double() for t in xvs], dim=1)
    return gemm_ref(a, torch.zeros_like(a), w, b, res_v, relu, planes=True)


def pool_bins(splits, H):
    return [(j * H // n, (j + 1) * H // n) for n in splits for j in range(n)]


def plane_pool_ref(xv, w, b, res_v, splits, mean, N, H=16, Wd=8, relu=True):
    """agrl_conv1x1_split16_pool: the UNROUNDED fp32 activations of plane_gemm_ref pooled over whole quarter bins of rows -> (N, P,
    Cout). |relu(a) - relu(b)| <= |a - b|: the pixel bounds add. The chain grows by the pixels of the largest bin."""
    r = plane_gemm_ref([xv], w, b, res_v, relu)
    Cout = w.shape[0]
    parts = [t.view(N, H, Wd, Cout) for t in (r[0], r[1], r[3], r.abs_slack)]
    out, cnt = [[] for _ in parts], []
    for lo, hi in pool_bins(splits, H):
        c = (hi - lo) * Wd
        cnt.append(c)
        for o, t in zip(out, parts):
            o.append(t[:, lo:hi].sum((1, 2)) / (c if mean else 1))
    exact, mag, slack, t_abs = (torch.stack(o, 1) for o in out)
    return Ref(exact, mag, r[2] + max(cnt), slack, t_abs)


def plane_conv3x3_ref(xv, w, b, relu=True, pixels=None):
    """agrl_conv3x3_packed_split16: stride 1, pad 1, on the values the planes hold (N, H, W, Cin); w OHWI TRUE weights."""
    from test_gpu_kernels import conv_exact
    xc = xv.detach().cpu().double().permute(0, 3, 1, 2)
    wc = w.detach().cpu().float().permute(0, 3, 1, 2)
    exact, mag, pix, coords = conv_exact(xc, wc, b, 1, 1, None, relu, pixels)
    _, aw = weight_abs(wc, planes=True)
    t_abs, _, _, _ = conv_exact(xc.abs(), aw * ABS_FACTOR, torch.zeros(w.shape[0]), 1, 1, pixels=pix)
    pmag = mag - b.detach().cpu().double().abs()
    return Ref(exact, mag, n_acc_split16(9 * w.shape[3]), C_SPLIT16 * pmag + t_abs, t_abs), pix, coords


def stem_ref(x, w, b):
    """agrl_stem_split16: maxpool3x3/2(relu(conv7x7/2(x, w) + b)), x (N, 3, H, W) fp32 split in the loop, w (64, 7, 7, 3) TRUE weights.
    The max of a window takes the largest bound in that window (test_gpu_kernels.check_stem); the contraction is 7 rows of 32."""
    x, wc = x.detach().cpu().float(), w.detach().cpu().float().permute(0, 3, 1, 2)
    x64, w64, b64 = x.double(), wc.double(), b.detach().cpu().double()
    _, aw = weight_abs(wc)
    ax = pair_abs(x)
    conv = lambda u, v, bias=None: F.conv2d(u, v, bias=bias, stride=2, padding=3)
    pool = lambda t: F.max_pool2d(t, 3, 2, 1)
    pmag = conv(x64.abs(), w64.abs())
    t_abs = conv(ax, w64.abs() * ABS_FACTOR + 2 * aw) + conv(x64.abs(), aw * ABS_FACTOR)
    exact = pool(F.relu(conv(x64, w64, b64)))
    mag = pool(pmag + b64.abs().view(1, -1, 1, 1))
    return Ref(exact, mag, n_acc_split16(7 * 32), pool(C_SPLIT16 * pmag + t_abs), pool(t_abs))


def distmat_ref(qv, g, metric, qn=None, gn=None, rows=None):
    """agrl_distmat_split16. qv (m, D): the values the query planes hold; g (n, D): the fp32 gallery rows the weight planes were made
    of (euclidean: the rows themselves; cosine: the kernel's own normalised rows). Euclidean: qn + gn - 2 qv g^T from the fp32 norms
    the kernel is given; cosine: 1 - qv g^T. Up to 8 split-K partials meet in the reduce: + 8."""
    qv = qv.detach().cpu().double()
    if rows is not None:
        qv = qv[rows]
    r = gemm_ref(qv, torch.zeros_like(qv), g, torch.zeros(g.shape[0]), planes=True, extra=8, k=13 if metric == "cosine" else None)
    dot, pmag, slack, t_abs = r[0], r[1], r[3], r.abs_slack
    if metric == "euclidean":
        qn64, gn64 = qn.detach().cpu().double(), gn.detach().cpu().double()
        if rows is not None:
            qn64 = qn64[rows]
        base = qn64[:, None] + gn64[None, :]
        return Ref(base - 2 * dot, base.abs() + 2 * pmag, r[2], 2 * slack, 2 * t_abs)
    return Ref(1 - dot, 1 + pmag, r[2], slack, t_abs)


# ---- operand generators -------------------------------------------------------------------------------------------------------------
def _ulp16(h):
    return 2.0 * half_ulp(h, torch.float16)


def _coherent(h, sign, g):
    """h (fp16 values, float64) + sign ulp16(h) u, u in (0.1, 0.4): the low half has ONE sign whatever the sign of h."""
    u = 0.1 + 0.3 * torch.rand(h.shape, generator=g, dtype=torch.float64)
    return (h + sign * _ulp16(h) * u).float()


def activations(kind, shape, g, post_relu=True):
    """fp32 activations (..., C). ``post_relu``: non-negative with exact zeros (what a conv after a ReLU reads)."""
    lead = tuple(shape[:-1]) + (1,)
    rect = (lambda t: t.clamp(min=0)) if post_relu else (lambda t: t)
    if kind in ("plain", "small_rows"):
        # the log-normal scale of the present tests per pixel, kept above 2^-2 so that a pixel's absolute terms stay inside the cap
        x = rect(torch.randn(shape, generator=g)) * torch.exp(1.5 * torch.randn(lead, generator=g)).clamp(min=0.25)
        if kind == "small_rows":
            x[..., 8:16] *= 2.0 ** -10
        return x
    if kind == "coherent_lo":
        e = torch.randint(0, 5, shape, generator=g).double()
        h = rne16(((1 + torch.rand(shape, generator=g, dtype=torch.float64)) * 2.0 ** e).float()).double()   # [1, 32): normal low halves
        x = _coherent(h, 1.0, g)
        return x if post_relu else x * torch.where(torch.rand(lead, generator=g) < 0.25, -1.0, 1.0)
    if kind == "tiny":
        return (2.0 ** (-20 + 12 * torch.rand(shape, generator=g))).float()
    if kind == "wide_range":
        x = rect(torch.randn(shape, generator=g)) * torch.exp(2.5 * torch.randn(shape, generator=g))
        x = x.clamp(max=3.0e4) if post_relu else x.clamp(min=-3.0e4, max=3.0e4)
        flat = x.view(-1)
        idx = torch.randperm(flat.numel(), generator=g)
        n = max(flat.numel() // 16, 4)
        flat[idx[:n]] = 3.0e4 * torch.rand(n, generator=g)
        flat[idx[n:2 * n]] = 0.0
        flat[idx[2 * n:3 * n]] = -0.0
        return x
    raise ValueError(kind)


def w_unit(k):
    """The size of a generated weight: 2^-7 / K. BatchNorm-folded magnitudes (2^-13 at K = 64, 2^-18 at K = 2048): sums of K products
    keep one size at every depth, and without the pre-scale the low halves -- from K = 128 on the high halves too -- are fp16 subnormals,
    whose lost bits grow with K as fast as the chain's allowance does."""
    return 2.0 ** -7 / k


def weights(kind, cout, k, g):
    """TRUE fp32 weights (cout, k) and a bias of the size of a typical sum."""
    if kind == "coherent_lo":
        # scaled weights h 2^-27 with h across [2^10, 2^14): one sign per ROW, every fourth row negative, so all low terms of a row add up
        e = torch.randint(10, 14, (cout, k), generator=g).double()
        h = rne16(((1 + torch.rand((cout, k), generator=g, dtype=torch.float64)) * 2.0 ** e).float()).double()
        h[0, 0] = 2.0 ** 13 * 1.5                    # pins k = 27
        w = _coherent(h, 1.0, g) * 2.0 ** -27
        w = w * torch.where(torch.arange(cout) % 4 == 3, -1.0, 1.0)[:, None]
    elif kind == "tiny":
        w = torch.randn((cout, k), generator=g).abs() * w_unit(k)   # non-negative: no cancellation, the outputs stay far above the absolute terms
    else:
        w = torch.randn((cout, k), generator=g) * w_unit(k)
        if kind == "small_rows":
            w[1] *= 2.0 ** -10
            w[cout // 2] *= 2.0 ** -10
    typical = float(w.abs().mean()) * k
    b = 0.05 * typical * (torch.rand(cout, generator=g) if kind == "tiny" else torch.randn(cout, generator=g))
    return w.float().contiguous(), b.float()


# ---- CPU emulation of the recipe ----------------------------------------------------------------------------------------------------
def _chain(pairs, chunk=32):
    """sum over (A, B) of A B^T: fp32 accumulator, 32-deep steps, the pairs in order within a step (small terms first)."""
    K = pairs[0][0].shape[1]
    acc = torch.zeros((pairs[0][0].shape[0], pairs[0][1].shape[0]), dtype=torch.float32)
    for k0 in range(0, K, chunk):
        for a, w in pairs:
            acc = acc + a[:, k0:k0 + chunk] @ w[:, k0:k0 + chunk].t()
    return acc


def emulate_gemm(a, w, b, res=None, relu=False, planes=False, defects=(), out="f32", pool=None, k=None):
    """The recipe on a (P, K) fp32 activations (``planes``: first stored as planes, the kernel's input), w (Cout, K) TRUE weights, b
    (Cout,), res (P, Cout) fp32 (``planes``: stored as planes as well). ``out``: "f32" | "presplit" | "planes".
    -> dict(v = the fp32 result or the value its halves hold (float64), hi, lo = unscaled halves or None, xv, rv = what the input planes hold).
    pool = (splits, mean, N, H, W): the pooled epilogue on the fp32 values. defects: letters of DEFECTS."""
    a, w = a.float(), w.float()
    k = 0 if "e" in defects else prescale_exp(w) if k is None else k
    Wh, Wl = split16(w * 2.0 ** k)
    zero = torch.zeros_like
    xv = rv = None
    if planes:
        ah, als = split16(a, 2.0 ** 11)            # the clean planes: the kernel's input
        xv = planes_value(ah, als)
        if "f" in defects:
            als = als.clone()
            als[:, :128] = ah[:, :128]
        Whs = rne16(Wh * 2.0 ** -11)
        pairs = [(als, zero(Whs) if "b" in defects else Whs), (ah, zero(Wl) if "a" in defects else Wl), (ah, Wh)]
        if res is not None:
            rh, rls = split16(res, 2.0 ** 11)
            rv = planes_value(rh, rls)
            res = (rh + rls * 2.0 ** -11).float()   # exact in fp32: 22 bits
    else:
        ah, al = split16(a, trunc="c" in defects)
        pairs = [(zero(al) if "b" in defects else al, Wh), (ah, zero(Wl) if "a" in defects else Wl), (ah, Wh)]
    v = _chain(pairs) * 2.0 ** -k + b.float()
    if res is not None:
        v = v + res.float()
    if relu:
        v = v.relu()
    hi = lo = None
    if pool is not None:
        splits, mean, N, H, Wd = pool
        t = v.view(N, H, Wd, -1)
        v = torch.stack([t[:, lo_:hi_].sum((1, 2)) / ((hi_ - lo_) * Wd if mean else 1) for lo_, hi_ in pool_bins(splits, H)], 1)
    elif out == "presplit":
        hi, lo = split16(v, trunc="c" in defects)
        v = hi.double() + lo.double()
    elif out == "planes":
        hi, ls = split16(v, 1.0 if "d" in defects else 2.0 ** 11, trunc="c" in defects)
        v = planes_value(hi, ls)
        lo = ls * (1.0 if "d" in defects else 2.0 ** -11)
    return dict(v=v.double(), hi=hi, lo=lo, xv=xv, rv=rv)


def patches(x, R, stride, pad):
    """NHWC fp32 -> (N OH OW, R R Cin) rows in OHWI order (the emulation's own im2col, independent of conv_exact)."""
    N, H, W, C = x.shape
    cols = F.unfold(x.permute(0, 3, 1, 2).float(), R, padding=pad, stride=stride)          # (N, C R R, L), channel-major
    L = cols.shape[2]
    return cols.view(N, C, R * R, L).permute(0, 3, 2, 1).reshape(N * L, R * R * C)


def check_split16(got, ref, name="", plane_out=False, presplit_out=False, hi=None, lo=None, **kw):
    """check_rounded of an fp32 result (or of the value split halves hold) against a Ref; halves also have to be canonical."""
    exact, mag, n_acc, slack = ref
    if plane_out:
        slack = slack + plane_out_slack(exact)
    if presplit_out:
        slack = slack + presplit_out_slack(exact)
    if hi is not None:
        canonical_halves(hi, lo, name)
    return check_rounded(got, exact, mag, n_acc, torch.float32, slack=slack, name=name, **kw)[0]


# ---- the shapes both test files use (tests/test_split16_ref.py on the emulation, tests/test_gpu_split16_bounds.py on the kernels) ------
# in-loop conv: (N, H, W, Cin, Cout, R, stride, residual)
INLOOP_CASES = [(3, 10, 7, 64, 64, 1, 1, False),      # ragged M, 64-channel tile, 3-slot ring
                (2, 16, 8, 64, 256, 1, 1, True),      # conv3 + residual
                (1, 9, 5, 32, 96, 3, 1, False),       # smallest K group
                (2, 16, 8, 128, 128, 3, 2, False),    # stride 2
                (1, 4, 4, 2048, 128, 1, 1, False)]    # deepest chain
# two-source first block: (N, H, W, K1, K2, Cout, stride)
DUAL_CASES = [(1, 9, 7, 64, 96, 128, 2), (2, 16, 8, 64, 64, 256, 1), (2, 8, 4, 1024, 512, 2048, 1)]
DUAL_KINDS = ("plain", "coherent_lo", "small_rows")
# plane GEMMs: (M, K or (K1, K2), Cout, form); every M of {40, 128, 296}, K of {128, 256, (256, 128), 2048}, Cout of {256, 1024} occurs.
# A deliberate SAMPLE of the 24 combinations (each runs in four layouts on the GPU): the values are not crossed -- e.g. no dual at M = 128,
# no K = 2048 at M = 128 -- because M only decides the ragged last tile and Cout the number of channel tiles, whatever K is
PLANE_CASES = [(40, 128, 256, "plain"), (128, 256, 1024, "plain"), (296, 2048, 256, "plain"), (296, 128, 1024, "res"), (40, 2048, 1024, "res"),
               (128, 256, 256, "res"), (296, (256, 128), 256, "dual"), (40, (256, 128), 1024, "dual")]
PLANE_KINDS = ("plain", "coherent_lo", "small_rows")
# pooled last conv: (frames, K, Cout, splits, mean)
POOL_CASES = [(1, 2048, 256, [4, 2, 1], True), (5, 128, 1024, [4, 2, 1], True), (1, 256, 256, [1], False), (5, 256, 256, [1], False)]
CONV3_CASES = [(1, 16, 8, 128, 256), (3, 16, 8, 256, 256), (2, 32, 16, 128, 256)]
CONV3_KINDS = ("plain", "coherent_lo", "tiny")
STEM_CASES = [(1, 37, 23), (2, 64, 32), (2, 130, 70), (70, 64, 48)]
# distance matrix: (m, n, D); the last one is long enough for the streaming form
DISTMAT_CASES = [(7, 60, 64), (37, 101, 128), (130, 257, 2048), (260, 1523, 512), (24, 2077, 128)]
DISTMAT_KINDS = ("plain", "coherent_lo")
# the cosine metric normalises every row first, which moves the values off the fp16 grid they were built on: there are no coherent low halves
# to be had there, and coherent_lo is a euclidean kind
DISTMAT_RUNS = [(k_, m_) for k_ in DISTMAT_KINDS for m_ in ("euclidean", "cosine") if not (k_ == "coherent_lo" and m_ == "cosine")]


def seed_of(*parts):
    return sum((i + 1) * int(p) for i, p in enumerate(parts)) % (2 ** 31)


def inloop_operands(case, kind):
    N, H, W, Cin, Cout, R, stride, with_res = case
    g = torch.Generator().manual_seed(seed_of(*case[:7], KINDS.index(kind)))
    x = activations(kind, (N, H, W, Cin), g)
    w, b = weights(kind, Cout, R * R * Cin, g)
    w = w.view(Cout, R, R, Cin)
    pad = R // 2
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    res = None
    if with_res:
        res = activations(kind, (N, OH, OW, Cout), g) * float(w.abs().mean()) * R * R * Cin * 0.5
    return x, w, b, res, pad


def dual_operands(case, kind):
    N, H, W, K1, K2, Cout, stride = case
    g = torch.Generator().manual_seed(seed_of(*case, KINDS.index(kind)))
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    x, x2 = activations(kind, (N, H, W, K1), g), activations(kind, (N, OH, OW, K2), g)
    w, b = weights(kind, Cout, K1 + K2, g)
    return x, x2, w, b


def plane_operands(M, K, Cout, kind, with_res, seed=0):
    """-> list of fp32 sources (M, K_i), w (Cout, sum K_i), b, fp32 residual (M, Cout) or None."""
    Ks = list(K) if isinstance(K, tuple) else [K]
    g = torch.Generator().manual_seed(seed_of(M, sum(Ks), Cout, KINDS.index(kind), seed))
    xs = [activations(kind, (M, k_), g) for k_ in Ks]
    w, b = weights(kind, Cout, sum(Ks), g)
    res = activations(kind, (M, Cout), g) * float(w.abs().mean()) * sum(Ks) * 0.5 if with_res else None
    return xs, w, b, res


def conv3_operands(case, kind):
    N, H, W, Cin, Cout = case
    g = torch.Generator().manual_seed(seed_of(*case, KINDS.index(kind)))
    x = activations(kind, (N, H, W, Cin), g)
    w, b = weights(kind, Cout, 9 * Cin, g)
    return x, w.view(Cout, 3, 3, Cin), b


def stem_operands(shape):
    """coherent_lo pixels, coherent_lo weights with one row a thousand times smaller."""
    N, H, W = shape
    g = torch.Generator().manual_seed(seed_of(*shape))
    x = activations("coherent_lo", (N, 3, H, W), g)
    w, b = weights("coherent_lo", 64, 147, g)
    w[5] *= 1e-3
    return x, w.view(64, 7, 7, 3).contiguous(), b


def S_rne16_grid(shape, g):
    """fp16 numbers in [2^13, 2^14), float64."""
    return rne16(((1 + torch.rand(shape, generator=g, dtype=torch.float64)) * 2.0 ** 13).float()).double().clamp(max=2.0 ** 14 - 8)


def distmat_operands(shape, kind):
    m, n, D = shape
    g = torch.Generator().manual_seed(seed_of(*shape, KINDS.index(kind)))
    if kind == "coherent_lo":
        # both sides in ONE binade at the foot of fp16's normal range, [2^-14, 2^-13): the dot product weighs as much as the norms, the
        # query planes' halves are normal fp16 numbers with low halves of one sign, and an un-scaled gallery row loses its whole low half
        def rows(r):
            h = S_rne16_grid((r, D), g)
            return (_coherent(h, 1.0, g) * 2.0 ** -27).contiguous()
        return rows(m), rows(n)
    centers = torch.randn((16, D), generator=g)
    q = centers[torch.randint(0, 16, (m,), generator=g)] + 0.5 * torch.randn((m, D), generator=g)
    gal = centers[torch.randint(0, 16, (n,), generator=g)] + 0.5 * torch.randn((n, D), generator=g)
    return q, gal


def near_copies_operands():
    """Euclidean cancellation: 40 queries, 64 gallery rows of which rows 0..7 are query rows + 2^-12-relative noise and rows 8, 9 exact copies."""
    g = torch.Generator().manual_seed(77)
    q, gal = torch.randn((40, 256), generator=g), torch.randn((64, 256), generator=g)
    gal[:8] = q[:8] * (1 + 2.0 ** -12 * torch.randn((8, 256), generator=g))
    gal[8:10] = q[8:10]
    return q, gal


def distmat_form(m, n, D3, workspace=True):
    """Which form of csrc/igemm.hip::distmat_impl a 16-bit (m, n, D3) problem takes (hip_ops.distmat_split16 passes a workspace when
    there are fewer than 256 tiles): "stream" | "splitk" | "tiled". A Python COPY of that dispatch (as graph_ref.propagate_form is of its
    kernel's): it tells which form a shape reaches today; a change to the C++ dispatch does not fail an assertion made with it, and has to be
    carried over here by hand."""
    if m <= 64 and n >= 2048 and (D3 * 2) % 128 == 0:
        return "stream"
    cdiv = lambda a, b_: -(-a // b_)
    tiles, nk, ks = cdiv(m, 64) * cdiv(n, 128), D3 // 64, 1
    while ks < 8 and tiles * ks < 512 and nk % (ks * 2) == 0 and nk // (ks * 2) >= 4:
        ks *= 2
    return "splitk" if ks > 1 and workspace and tiles < 256 and D3 % 64 == 0 else "tiled"
