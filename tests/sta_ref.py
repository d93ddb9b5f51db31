"""float64 restatements of the three baseline tails (res50tp, simple_sta, sta), of the contracts of csrc/sta.hip's kernels
(agrl_sta_frame_stats, agrl_sta_fuse, agrl_linear_bn_relu) on the operands each kernel actually sees, the fp32 chain lengths for
``bounds.check_rounded(..., out_dtype=torch.float32)``, and the seeded weights / clips of the fixtures tests/golden/*_b2s4.npz
(tests/golden/make_sta_golden.py).

Chain lengths, u = 2^-24 (bounds.U32), all read off csrc/sta.hip. Every one is an upper bound on the number of fp32 roundings between
the operands and the output, relative to the sum of magnitudes handed to check_rounded as ``mag``:
  frame_stats  a lane owns cpl = ceil(C / (256 VEC)) VEC channels (VEC = 8 for 16-bit maps, 4 for fp32).
    vmean      npix - 1 additions in pixel order, 1 / npix rounded, the product:                      npix + 2,   mag = mean |x|
    n2_p       a lane's cpl fmafs, six shuffle steps, (w0 + w1) + (w2 + w3): cpl + 8 roundings of positive terms
    nsum       sqrt halves n2's relative error and rounds once, then npix additions:                  cpl + 9 + npix (an upper bound
               of (cpl + 8) / 2 + 1 + npix),                                                          mag = nsum itself
    nsq        n2 and the additions over the rows the bin owns:                                       cpl + 8 + npix_own, mag = nsq
  fuse         scores, map mode: three additions, sqrt, nsum / npix, the quotient: <= 6 each; norm mode: a lane's 4 ceil(C / 256)
               fmafs, six shuffle steps, sqrt: <= cn = 4 ceil(C / 256) + 7 each.
    t_a        a score, the S additions of |score| (each term carrying its own error), the quotient:  2 e + S + 1 with e = 6 / cn,
               mag = t_a itself
    f_g[:C]    ((v0 + v1) + v2) + v3, times 0.25 (exact):                                             3,          mag = mean_p |v|
    f_g[C:]    referenced on the kernel's OWN fp32 t_a (it returns them), so a last-bit difference upstream does not loosen the bar:
               the fmaf chain over S, three additions, times 0.25:                                    S + 3, mag = mean_p sum_s |t_a v|
  linear_bn_relu   a lane's 4 ceil(K / 256) fmafs, six shuffle steps, fmaf(acc, scale, shift):        4 ceil(K / 256) + 8,
               mag = |scale| sum_k |x w| + |shift|; ReLU is 1-Lipschitz, so the bound holds behind it
    above the M bound (hip_ops.linear_bn_relu's GEMM + torch epilogue): bounds.n_acc_for(K, 4 for fp32 / 16 for 16-bit operands, x
               rounded to the weight's type first) + 2 for the product with scale and the addition of shift.
A plain module (like pam_train_ref.py): the tests import it. Everything here runs on the CPU."""
import math

import torch

from recipe import _gen, recipe_state_dict

PARTS = 4


def bins(h):
    """[(row0, row1)] of AdaptiveAvgPool2d((4,1)): floor(i h / 4) .. ceil((i + 1) h / 4)."""
    return [((i * h) // PARTS, -((-(i + 1) * h) // PARTS)) for i in range(PARTS)]


def own_rows(h):
    """[(row0, row1)] the rows of bin i no later bin starts in: floor(i h / 4) .. floor((i + 1) h / 4)."""
    return [((i * h) // PARTS, ((i + 1) * h) // PARTS) for i in range(PARTS)]


def channels_per_lane(C, vec):
    return int(math.ceil(C / (256.0 * vec))) * vec


# ---- kernel contracts ------------------------------------------------------------------------------------------------------------
def frame_stats_ref(fmap):
    """fmap (F,h,w,C) any float dtype, NHWC -> dict of float64 (value, mag) pairs and chain lengths for agrl_sta_frame_stats."""
    x = fmap.detach().cpu().double()
    F_, h, w, C = x.shape
    vec = 4 if fmap.dtype == torch.float32 else 8
    cpl = channels_per_lane(C, vec)
    n2 = (x * x).sum(dim=3)                    # (F,h,w)
    n = n2.sqrt()
    vmean, vmag, nsum, nsq = [], [], [], []
    for (r0, r1), (o0, o1) in zip(bins(h), own_rows(h)):
        vmean.append(x[:, r0:r1].mean(dim=(1, 2)))
        vmag.append(x[:, r0:r1].abs().mean(dim=(1, 2)))
        nsum.append(n[:, r0:r1].sum(dim=(1, 2)))
        nsq.append(n2[:, o0:o1].sum(dim=(1, 2)))
    npix = max((r1 - r0) * w for r0, r1 in bins(h))
    npix_own = max((o1 - o0) * w for o0, o1 in own_rows(h))
    return {
        "vmean": torch.stack(vmean, 1), "vmean_mag": torch.stack(vmag, 1), "vmean_n": npix + 2,
        "nsum": torch.stack(nsum, 1), "nsum_n": cpl + 9 + npix,
        "nsq": torch.stack(nsq, 1), "nsq_n": cpl + 8 + npix_own,
    }


def scores_map(nsum, nsq, h, w):
    """(F,4) float64 scores of sta: (nsum / npix_p) / max(sqrt(sum_p nsq), 1e-12). sta.py:213-217."""
    npix = torch.tensor([(r1 - r0) * w for r0, r1 in bins(h)], dtype=torch.float64)
    return (nsum.double() / npix) / nsq.double().sum(dim=1, keepdim=True).sqrt().clamp(min=1e-12)


def scores_norm(vmean):
    """(F,4) float64 scores of simple_sta / res50tp: the channel norm of the part means. simple_sta.py:209."""
    return vmean.double().pow(2).sum(dim=2).sqrt()


def temporal_attention(scores, B, S):
    s = scores.double().view(B, S, PARTS)
    return s / s.abs().sum(dim=1, keepdim=True).clamp(min=1e-12)


def fuse_ref(vmean, scores, B, S, idx=None, t_a=None):
    """vmean (B*S,4,C), scores (B*S,4) -> float64 f_g (B,2C), its mag, t_a (B,S,4), idx (B,4) (first maximum). ``idx`` / ``t_a``
    given: evaluate the selection / the weighted sum with them (the device's own) instead."""
    v = vmean.detach().cpu().double().view(B, S, PARTS, -1)
    C = v.shape[-1]
    ta = temporal_attention(scores, B, S)
    first = ta.argmax(dim=1)
    # torch.argmax returns the first maximal index on the CPU; make the rule explicit all the same
    for b in range(B):
        for p in range(PARTS):
            first[b, p] = int((ta[b, :, p] == ta[b, :, p].max()).nonzero()[0])
    use_idx = first if idx is None else idx.detach().cpu().long()
    use_ta = ta if t_a is None else t_a.detach().cpu().double()
    sel = v.gather(1, use_idx.view(B, 1, PARTS, 1).expand(B, 1, PARTS, C)).view(B, PARTS, C)
    f1, f1_mag = sel.mean(dim=1), sel.abs().mean(dim=1)
    wsum = (use_ta.unsqueeze(3) * v).sum(dim=1)
    f2, f2_mag = wsum.mean(dim=1), (use_ta.abs().unsqueeze(3) * v.abs()).sum(dim=1).mean(dim=1)
    return torch.cat([f1, f2], 1), torch.cat([f1_mag, f2_mag], 1), ta, first


def fuse_chains(S, C, mode):
    e = 6 if mode == "map" else 4 * int(math.ceil(C / 256.0)) + 7
    return {"t_a": 2 * e + S + 1, "f1": 3, "f2": S + 3}


def linear_bn_relu_ref(x, w, scale, shift):
    """-> float64 relu(scale (x w^T) + shift), mag, chain length; x, w as the kernel sees them."""
    xd, wd = x.detach().cpu().double(), w.detach().cpu().double()
    sc, sh = scale.detach().cpu().double(), shift.detach().cpu().double()
    pre = (xd @ wd.t()) * sc + sh
    mag = (xd.abs() @ wd.abs().t()) * sc.abs() + sh.abs()
    return pre.clamp(min=0), mag, 4 * int(math.ceil(x.shape[1] / 256.0)) + 8


# ---- the three tails, float64, from the layer-4 map ---------------------------------------------------------------------------
def part_means(fm):
    """fm (F,c,h,w) NCHW -> (F,4,c) float64"""
    fm = fm.detach().double()
    return torch.stack([fm[:, :, r0:r1].mean(dim=(2, 3)) for r0, r1 in bins(fm.shape[2])], dim=1)


def tail_ref(kind, fm, B, S, sd, idx=None):
    """The eval tail of ``kind`` ('res50tp' / 'simple_sta' / 'sta') in float64 on the NCHW layer-4 map ``fm`` (B*S,c,h,w) with the state
    dict ``sd`` -> dict(out, t_a [, idx, f_g]). ``idx`` (B,4): select these frames instead of the first maxima."""
    fm = fm.detach().double()
    F_, c, h, w = fm.shape
    v = part_means(fm)
    if kind == "sta":
        n = fm.pow(2).sum(dim=1).sqrt()                                        # (F,h,w)
        g = n / n.view(F_, -1).pow(2).sum(dim=1).sqrt().clamp(min=1e-12).view(F_, 1, 1)
        scores = torch.stack([g[:, r0:r1].mean(dim=(1, 2)) for r0, r1 in bins(h)], dim=1)
    else:
        scores = scores_norm(v)
    eps = 1e-5
    if kind == "res50tp":
        ta = temporal_attention(scores, B, S)
        f = (ta.unsqueeze(3) * v.view(B, S, PARTS, c)).sum(dim=1).mean(dim=1)
        bn = "bottleneck."
        out = (f - sd[bn + "running_mean"].double()) / (sd[bn + "running_var"].double() + eps).sqrt() * sd[bn + "weight"].double() \
            + sd[bn + "bias"].double()
        return {"out": out, "t_a": ta, "f": f}
    f_g, _, ta, first = fuse_ref(v, scores, B, S, idx=idx)
    pre = f_g @ sd["fc1.0.weight"].double().t()
    bn = "fc1.1."
    out = (pre - sd[bn + "running_mean"].double()) / (sd[bn + "running_var"].double() + eps).sqrt() * sd[bn + "weight"].double() \
        + sd[bn + "bias"].double()
    return {"out": out.clamp(min=0), "t_a": ta, "idx": first, "f_g": f_g, "pre": pre}


def relative_gaps(t_a):
    """(B,S,4) -> (B,4): (best - second best) / best of the temporal attention over the frames."""
    top = t_a.double().topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) / top[:, 0]


# ---- fixture recipes ------------------------------------------------------------------------------------------------------------
FC1_STD = 0.02


def sta_state_dict(template, seed, calib=None):
    """tests/recipe.py's state dict for the three baselines. Where there is an ``fc1``: its Linear weight at std 0.02 (the recipe's
    0.001 makes the eval output relu(BatchNorm shift), blind to the input; at 0.02 the pre-BN values have std ~0.28), and -- with
    ``calib`` = (mean, var), two scalars measured on the fixture batch and stored in the fixture -- ``fc1.1.running_mean`` /
    ``running_var`` filled with them (a per-dimension variance over two tracklets would be degenerate)."""
    sd = recipe_state_dict(template, seed)
    key = "fc1.0.weight"
    if key in sd:
        sd[key] = torch.randn(tuple(sd[key].shape), generator=_gen(key + "#sta", seed)) * FC1_STD
        if calib is not None:
            sd["fc1.1.running_mean"] = torch.full_like(sd["fc1.1.running_mean"], float(calib[0]))
            sd["fc1.1.running_var"] = torch.full_like(sd["fc1.1.running_var"], float(calib[1]))
    return sd


def sta_clips(B, S, seed, H=256, W=128):
    """Clips whose frames differ by more than noise, so that the highest-scoring frame of a part is not a coin toss:
    (noise + pattern_s) * (1 + 0.8 cos(2 pi (y - phase_s))) * gain_s with a per-frame smooth pattern, a per-frame vertical envelope
    and a per-frame gain. (B,S,3,H,W) fp32."""
    g = torch.Generator()
    g.manual_seed(0x57A + 7919 * int(seed))
    noise = 0.5 * torch.randn((B, S, 3, H, W), generator=g)
    low = torch.randn((B * S, 3, 8, 4), generator=g)
    pattern = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False).view(B, S, 3, H, W)
    phase = torch.rand((B, S, 1, 1, 1), generator=g)
    gain = 0.6 + 0.8 * torch.rand((B, S, 1, 1, 1), generator=g)
    y = (torch.arange(H, dtype=torch.float32) / H).view(1, 1, 1, H, 1)
    return ((noise + pattern) * (1.0 + 0.8 * torch.cos(2 * math.pi * (y - phase))) * gain).contiguous()


def clips_u8(x, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """fp32 normalised clips -> the uint8 pixels a decoder would have handed over (un-normalise, round, clamp); (B,S,3,H,W) uint8."""
    m = torch.tensor(mean).view(1, 1, 3, 1, 1)
    s = torch.tensor(std).view(1, 1, 3, 1, 1)
    return ((x * s + m) * 255.0).round().clamp(0, 255).to(torch.uint8)
