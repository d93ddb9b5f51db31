"""Float64 exact evaluations of one step of the RMSprop, AdaBound / AMSBound and RAdam rules of csrc/optim.hip, in the style of
adam_exact / sgd_exact (tests/test_gpu_hip_optim.py): float64 tensors in, ``{name: (exact, magnitude)}`` out, with the host constants
formed in double and rounded once to fp32, exactly as the launch sees them. Every element of every quantity must satisfy

    |got - exact| <= n 2^-24 magnitude + 2^-149

``magnitude`` is the same chain on magnitudes (a sum of absolute values where the rule adds or subtracts), with the denominator taken
exact, as in the Adam contract: the cancellation of g + wd p that a denominator sees is the cancellation its numerator sees.

How the n tables are counted (from the contract in include/agrl_hip.h, nothing measured). Each fp32 operation adds one unit roundoff
u = 2^-24 relative to the magnitude of its result; a quantity's count c is what reaches it to first order: a sum carries the larger
count of its terms plus one, a product or quotient the sum of its factors' counts plus one, a square twice its operand's count plus
one, a square root half its operand's count plus one; max, min and the clamp add nothing (1-Lipschitz, their bounds are constants).
n = ceil(c) + 2: the two units of slack cover the second-order terms and the difference between the contract's one-constant moving
average m + (1 - b)(x - m) and the two-constant form b m + (1 - b) x of torch and of the reference (|fl(b) + fl(1 - b) - 1| <= u / 2
per unit of |m|). A contracted FMA only removes a rounding.

    gd = g + wd p                              product 1, sum 1                                            c = 2   (absent in RAdam: c = 0)

  RMSprop
    sq  = alpha sq + (1 - alpha) gd^2          gd^2: 2*2 + 1 = 5, times (1 - alpha) 6; alpha sq 1; sum     c = 7   n = 9
    den = sqrt(sq) + eps                       7 / 2 + 1 = 4.5, sum                                        c = 5.5
    d   = gd / den                             2 + 5.5 + 1                                                 c = 8.5
    buf = momentum buf + d                     momentum buf 1; d 8.5; sum                                  c = 9.5 n = 12
    p   = p - lr buf                           lr buf 10.5; sum                                            c = 11.5 n = 14
    (without momentum p = p - lr d: 8.5 + 1 + 1 = 10.5, inside the same 14)

  AdaBound / AMSBound
    m    = m + (1 - b1)(gd - m)                difference 3, product 4, sum                                c = 5   n = 7
    v    = b2 v + (1 - b2) gd^2                as sq above                                                 c = 7   n = 9   (vmax: a max, the same)
    rate = clamp(step_size / (sqrt(v) + eps))  den 5.5, quotient 6.5, clamp 0                              c = 6.5
    p    = p - rate m                          product 6.5 + 5 + 1 = 12.5; sum                             c = 13.5 n = 16

  RAdam (the gradient is an input: c = 0)
    v  = b2 v + (1 - b2) g^2                   g^2 1, times (1 - b2) 2; b2 v 1; sum                        c = 3   n = 5
    m  = m + (1 - b1)(g - m)                   difference 1, product 2, sum                                c = 3   n = 5
    pd = p - decay p                           product 1, sum                                              c = 2
    p  = pd - step_size m / (sqrt(v) + eps)    step_size m 4; den 3 / 2 + 1 + 1 = 3.5; quotient 8.5; sum   c = 9.5 n = 12
    (momentum-only form p = pd - step_size m: 4 + 1 = 5, inside the same 12)"""
import numpy as np
import torch

from torchreid.hip_optim import adabound_constants, radam_constants

N_RMSPROP = {"sq": 9, "buf": 12, "p": 14}
N_ADABOUND = {"m": 7, "v": 9, "vmax": 9, "p": 16}
N_RADAM = {"m": 5, "v": 5, "p": 12}
TINY = 2.0 ** -149


def f32(x):
    return float(np.float32(x))


def rmsprop_exact(p, g, sq, buf, lr, alpha, eps, wd, momentum):
    """buf None: no momentum. -> {name: (exact, mag)}."""
    oma = f32(1.0 - alpha)
    lr, alpha, eps, wd, momentum = (f32(c) for c in (lr, alpha, eps, wd, momentum))
    gd = g + wd * p
    mag_gd = g.abs() + wd * p.abs()
    sq2 = alpha * sq + oma * gd * gd
    den = sq2.sqrt() + eps
    d, mag_d = gd / den, mag_gd / den
    out = {"sq": (sq2, alpha * sq + oma * mag_gd * mag_gd)}
    if buf is not None:
        d, mag_d = momentum * buf + d, momentum * buf.abs() + mag_d
        out["buf"] = (d, mag_d)
    out["p"] = (p - lr * d, p.abs() + lr * mag_d)
    return out


def adabound_exact(p, g, m, v, vmax, lr, betas, eps, wd, t, final_lr, gamma, base_lr, amsbound):
    """-> {name: (exact, mag)}; ``adabound_clamp_counts`` names the clamp outcome of every element of the same step."""
    omb1, b2, omb2, step_size, lower, upper = (f32(c) for c in adabound_constants(lr, betas[0], betas[1], t, final_lr, gamma, base_lr))
    wd, eps = f32(wd), f32(eps)
    gd = g + wd * p
    mag_gd = g.abs() + wd * p.abs()
    m2 = m + omb1 * (gd - m)
    mag_m = m.abs() + omb1 * (mag_gd + m.abs())
    v2 = b2 * v + omb2 * gd * gd
    mag_v = b2 * v + omb2 * mag_gd * mag_gd
    vv = torch.maximum(vmax, v2) if amsbound else v2
    rate = (step_size / (vv.sqrt() + eps)).clamp(lower, upper)
    out = {"p": (p - rate * m2, p.abs() + rate * mag_m), "m": (m2, mag_m), "v": (v2, mag_v)}
    if amsbound:
        out["vmax"] = (vv, torch.maximum(vmax, mag_v))
    return out


def adabound_clamp_counts(v_used, lr, betas, eps, t, final_lr, gamma, base_lr):
    """Elements whose rate is raised to the lower bound, left inside, cut to the upper bound; v_used: the exact v (vmax for AMSBound)
    of the step."""
    _, _, _, step_size, lower, upper = (f32(c) for c in adabound_constants(lr, betas[0], betas[1], t, final_lr, gamma, base_lr))
    q = step_size / (v_used.sqrt() + f32(eps))
    return int((q < lower).sum()), int(((q >= lower) & (q <= upper)).sum()), int((q > upper).sum())


def radam_exact(p, g, m, v, lr, betas, eps, wd, t):
    """-> {name: (exact, mag)}; the form (adaptive or momentum-only) and the step size are radam_constants' for the count t."""
    omb1, b2, omb2, decay, step_size, adaptive = radam_constants(lr, betas[0], betas[1], t, wd)
    omb1, b2, omb2, decay, step_size, eps = (f32(c) for c in (omb1, b2, omb2, decay, step_size, eps))
    v2 = b2 * v + omb2 * g * g
    m2 = m + omb1 * (g - m)
    mag_m = m.abs() + omb1 * (g.abs() + m.abs())
    pd, mag_pd = p - decay * p, p.abs() + decay * p.abs()
    if adaptive:
        den = v2.sqrt() + eps
        p2, mag_p = pd - step_size * m2 / den, mag_pd + step_size * mag_m / den
    else:
        p2, mag_p = pd - step_size * m2, mag_pd + step_size * mag_m
    return {"p": (p2, mag_p), "m": (m2, mag_m), "v": (v2, v2)}


def radam_regime(lr, betas, t):
    """'momentum' (N <= 4), 'unrectified' (adaptive form, plain step size: 4 < N <= 5) or 'rectified' (N > 5) for the count t."""
    _, _, _, _, step_size, adaptive = radam_constants(lr, betas[0], betas[1], t, 0.0)
    if not adaptive:
        return "momentum"
    return "unrectified" if step_size == lr / (1.0 - betas[0] ** t) else "rectified"


def worst_ratio(got, exact, mag, n):
    """max over the elements of |got - exact| / (n 2^-24 mag + 2^-149) on the tensors' device (a non-finite output counts as inf)."""
    g = got.detach().double().reshape(-1)
    r = (g - exact.reshape(-1)).abs() / (n * 2.0 ** -24 * mag.reshape(-1) + TINY)
    return float(torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf"))).max())
