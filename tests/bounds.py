"""Element-by-element bounds for the kernels' arithmetic contract: 16-bit (or fp32) operands, fp32 accumulation, ONE
round-to-nearest-even rounding of each output (agrl_common.h: f32_to_lp16 / pack_lp16x2).

A max-normalised error (max |got - ref| / max |ref|) cannot see a wrong rounding mode, a second rounding, an error confined to
small channels or an output element nobody wrote. ``check_rounded`` holds every element to

    |got - exact| <= half_ulp(|exact| + delta) + delta,      delta = n_acc * 2^-24 * mag

where ``exact`` is the float64 value of the stated operation on the operands the kernel actually sees (before the output
rounding) and ``mag`` the same operation on their magnitudes; for 16-bit outputs it also asks that nearly every element IS the
correctly rounded value. ``poisoned_outputs`` fills the outputs a kernel call allocates with NaN, so an unwritten element fails.

A plain module (like lp16.py): the tests import it."""
import contextlib
import json
import math
import os

import numpy as np
import torch

U32 = 2.0 ** -24          # unit roundoff of fp32
INT_SENTINEL = -0x5A5A5A5A  # what an integer output holds until the kernel writes it

_SIG = {torch.float16: (11, -14), torch.bfloat16: (8, -126)}  # significand bits (incl. the implicit one), smallest normal exponent


def n_acc_for(K, step=16):
    """fp32 roundings on one accumulation chain of K products: one per ``step``-deep MFMA (16 x 16 x 32 16-bit MFMAs: 16 per
    lane group; the exact-fp32 v_mfma_f32_16x16x4_f32: 4) plus bias, residual and slack."""
    return int(math.ceil(K / step)) + 3


def half_ulp(x, dtype):
    """Half a unit in the last place of ``dtype`` at |x|, in float64: fp16 2^(e-11) (normal), 2^-25 below 2^-14; bf16 2^(e-8),
    2^-134 below 2^-126; fp32 outputs get no rounding term (0)."""
    x = torch.as_tensor(x).double().abs()
    if dtype == torch.float32:
        return torch.zeros_like(x)
    p, emin = _SIG[dtype]
    _, e = torch.frexp(x)                          # x = m 2^e, m in [0.5, 1): the binade exponent is e - 1
    e = torch.where(x > 0, e - 1, torch.full_like(e, emin)).clamp(min=emin)
    return torch.ldexp(torch.ones_like(x), (e - p).to(torch.int64)).double()


def _log(record):
    path = os.environ.get("AGRL_BOUNDS_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")


def log_record(record):
    """Append a measurement that is put on record, not asserted (AGRL_BOUNDS_LOG), e.g. the conditioning of a variance."""
    _log(record)


def check_rounded(got, exact, mag, n_acc, out_dtype, min_exact_frac=0.98, *, slack=None, coords=None, edge=None, name=""):
    """Assert the contract above element by element; return (worst err / bound, exact-match fraction).

    got: the kernel's output (any device / dtype); exact, mag: float64, same shape. out_dtype: the dtype the kernel rounded to
    (fp32: no rounding term, no exact-match test). slack: an optional extra float64 allowance per element (e.g. a pooled sum of
    activations that may each sit one ulp the other side of a rounding boundary). coords: optional (rows, k) int64 tensor naming
    the leading coordinates (e.g. N, H, W) of each row of a 2-D ``got``; edge: optional bool mask (broadcastable) of elements on a
    ragged tile edge. Both only make the failure message precise."""
    g = got.detach().to("cpu", torch.float64)
    exact = exact.detach().to("cpu", torch.float64)
    mag = mag.detach().to("cpu", torch.float64)
    assert g.shape == exact.shape == mag.shape, (name, tuple(g.shape), tuple(exact.shape), tuple(mag.shape))
    delta = n_acc * U32 * mag
    bound = half_ulp(exact.abs() + delta, out_dtype) + delta
    if slack is not None:
        bound = bound + slack.detach().to("cpu", torch.float64)
    err = (g - exact).abs()
    finite = torch.isfinite(g)
    ratio = torch.where(finite, err / bound.clamp(min=1e-300), torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if out_dtype == torch.float32:
        frac = 1.0
    else:
        frac = float((g == exact.to(out_dtype).double()).double().mean()) if g.numel() else 1.0
    _log({"name": name, "lp": str(out_dtype), "ratio": worst, "exact_frac": frac, "n": g.numel()})
    ok = bool(finite.all()) and worst <= 1.0 and frac >= min_exact_frac
    if not ok:
        flat = int(torch.argmax(ratio))
        idx = np.unravel_index(flat, tuple(g.shape))
        where = tuple(int(i) for i in idx)
        if coords is not None and g.dim() == 2:
            where = tuple(int(v) for v in coords[where[0]]) + (where[1],)
        on_edge = None if edge is None else bool(torch.broadcast_to(edge, g.shape).reshape(-1)[flat])
        raise AssertionError(
            "%s: worst |got - exact| / bound = %.3g at %s (ragged edge: %s): got %r exact %r bound %.3g; non-finite %d of %d; "
            "exact-match fraction %.5f (needs %.3f)" % (
                name, worst, where, on_edge, float(g.reshape(-1)[flat]), float(exact.reshape(-1)[flat]),
                float(bound.reshape(-1)[flat]), int((~finite).sum()), g.numel(), frac, min_exact_frac))
    return worst, frac


@contextlib.contextmanager
def poisoned_outputs():
    """Inside the block, torch.empty / torch.empty_like fill floating tensors with NaN and integer ones with INT_SENTINEL: an element a kernel
    does not write (or an ``empty`` buffer it reads before writing) shows up. Wrap only the kernel call, never reference code."""
    real, real_like = torch.empty, torch.empty_like

    def poison(t):
        if t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype != torch.bool:
            t.fill_(INT_SENTINEL if t.dtype in (torch.int32, torch.int64) else 0x5A)
        return t

    torch.empty = lambda *a, **kw: poison(real(*a, **kw))
    torch.empty_like = lambda *a, **kw: poison(real_like(*a, **kw))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real, real_like
