"""Element-by-element bounds for the kernels' arithmetic contract: 16-bit (or fp32) operands, fp32 accumulation, ONE
round-to-nearest-even rounding of each output (agrl_common.h: f32_to_lp16 / pack_lp16x2).

A max-normalised error (max |got - ref| / max |ref|) cannot see a wrong rounding mode, a second rounding, an error confined to
small channels or an output element nobody wrote. ``check_rounded`` holds every element to

    |got - exact| <= half_ulp(|exact| + delta) + delta,      delta = n_acc * 2^-24 * mag

where ``exact`` is the float64 value of the stated operation on the operands the kernel actually sees (before the output
rounding) and ``mag`` the same operation on their magnitudes; for 16-bit outputs it also asks that nearly every element IS the
correctly rounded value. ``poisoned_outputs`` fills the outputs a kernel call allocates with NaN, so an unwritten element fails,
and stands each of them between two canary bands, so a store outside an output fails; ``fenced`` puts an operand between two
bands of a chosen byte, so a test can ask that a result does not depend on what lies next to an operand.

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


CANARY = 0xC5               # the byte a fence band holds until something stores into it
DEFAULT_BAND = 256 * 1024   # one 256-row tile of 512 16-bit channels: the largest overhang a ragged tile could produce here


def _poison(t):
    if t.is_floating_point():
        t.fill_(float("nan"))
    elif t.dtype != torch.bool:
        t.fill_(INT_SENTINEL if t.dtype in (torch.int32, torch.int64) else 0x5A)
    return t


def _check_band(band):
    assert isinstance(band, int) and band > 0 and band % 4096 == 0, "band must be a positive multiple of 4096, not %r" % (band,)


def _carve(shape, dtype, device, band, fill, alloc=torch.empty):
    """(raw, t): ``raw`` is one uint8 allocation of band + nbytes + band bytes whose two bands hold ``fill``; ``t`` is the
    contiguous (shape, dtype) tensor over the bytes between them. The tail band starts at the first byte after ``t``; a band
    that is a multiple of 4096 leaves ``t`` on the alignment of a fresh allocation."""
    shape = tuple(int(s) for s in shape)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    raw = alloc(band + nbytes + band, dtype=torch.uint8, device=device)
    raw[:band].fill_(fill)
    raw[band + nbytes:].fill_(fill)
    return raw, raw[band:band + nbytes].view(dtype).view(shape)


def fenced(t, fill, band=DEFAULT_BAND):
    """A contiguous copy of ``t`` (any dtype) on its device, between two bands of ``band`` bytes that hold the byte ``fill``.
    Nothing is checked: a test varies ``fill`` (0x00; 0xFF: NaN / -1; 0x7C: NaN in fp16, ~5e36 in bf16 and fp32) and asks that
    a kernel's outputs do not change with what lies next to its operands."""
    _check_band(band)
    _, out = _carve(t.shape, t.dtype, t.device, band, int(fill))
    out.copy_(t)
    return out


def _band_damage(raw, lo, hi):
    """(first, last, count) of the bytes of raw[lo:hi] that are not CANARY, as offsets into raw; None when intact."""
    bad = torch.nonzero(raw[lo:hi] != CANARY).reshape(-1)
    if bad.numel() == 0:
        return None
    return lo + int(bad[0]), lo + int(bad[-1]), int(bad.numel())


@contextlib.contextmanager
def poisoned_outputs(band=DEFAULT_BAND):
    """Inside the block, torch.empty / torch.empty_like fill floating tensors with NaN and integer ones with INT_SENTINEL: an element a kernel
    does not write (or an ``empty`` buffer it reads before writing) shows up. Wrap only the kernel call, never reference code.

    Every such tensor (and every accumulator from torch.zeros / torch.zeros_like / Tensor.new_zeros, interior left zero) is also
    carved out of a larger uint8 allocation, between two bands of ``band`` bytes (a multiple of 4096) that hold CANARY; the tail
    band starts at the first byte after the tensor. On leaving the block the bands are compared with CANARY on the current
    stream, behind the kernels: a store outside an output raises AssertionError naming the tensor, the side, the byte offsets
    and the count. Pinned tensors, non-strided layouts and non-contiguous results (a ``memory_format`` other than contiguous,
    ``empty_like`` of a permuted tensor) are poisoned but not fenced. Known limit: a store farther than ``band`` bytes from
    the tensor is not seen."""
    _check_band(band)
    real, real_like, real_zeros, real_zeros_like = torch.empty, torch.empty_like, torch.zeros, torch.zeros_like
    real_new_zeros = torch.Tensor.new_zeros
    records = []   # (raw, nbytes, shape, dtype): keeps every carved allocation alive (and its memory unshared) until the check

    def fence(fn, a, kw, zero, like=None):
        """``fn(*a, **kw)`` is the real allocation. Its shape, dtype and strides come from the same call on the ``meta`` device (no
        memory, no memset), its device from the arguments: -> the carved twin, or the real tensor where a fence cannot stand."""
        def passed_through():
            t = fn(*a, **kw)
            return t if zero else _poison(t)
        if (kw.get("pin_memory") or kw.get("out") is not None or kw.get("layout") not in (None, torch.strided)
                or kw.get("memory_format") not in (None, torch.contiguous_format, torch.preserve_format)):
            return passed_through()
        m = fn(*a, **dict(kw, device="meta"))
        if kw.get("device") is not None:
            device = real(0, device=kw["device"]).device        # resolves "cuda" to the current device
        else:
            device = like.device if like is not None else real(0).device
        if not (m.layout == torch.strided and m.is_contiguous() and not m.is_quantized and device.type in ("cpu", "cuda")):
            return passed_through()
        raw, out = _carve(m.shape, m.dtype, device, band, CANARY, alloc=real)
        records.append((raw, out.numel() * out.element_size(), tuple(out.shape), out.dtype))
        out = out.zero_() if zero else _poison(out)
        return out.requires_grad_() if kw.get("requires_grad") else out

    torch.empty = lambda *a, **kw: fence(real, a, kw, False)
    torch.empty_like = lambda *a, **kw: fence(real_like, a, kw, False, like=a[0] if a else kw["input"])
    torch.zeros = lambda *a, **kw: fence(real_zeros, a, kw, True)
    torch.zeros_like = lambda *a, **kw: fence(real_zeros_like, a, kw, True, like=a[0] if a else kw["input"])
    torch.Tensor.new_zeros = lambda self, *a, **kw: fence(real_new_zeros, (self,) + a, kw, True, like=self)
    clean = False
    try:
        yield records      # ``with poisoned_outputs() as fences``: len(fences) allocations stand between bands so far
        clean = True
    finally:
        torch.empty, torch.empty_like, torch.zeros, torch.zeros_like = real, real_like, real_zeros, real_zeros_like
        torch.Tensor.new_zeros = real_new_zeros
    if not clean or not records:
        return
    # one device round trip for the whole block; the details only when a band was hit
    hit = {}
    for raw, n, _, _ in records:
        h = (raw[:band] != CANARY).any() | (raw[band + n:] != CANARY).any()
        hit[raw.device] = h if raw.device not in hit else hit[raw.device] | h
    if not any(bool(h) for h in hit.values()):
        return
    msgs = []
    for idx, (raw, n, shape, dtype) in enumerate(records):
        head, tail = _band_damage(raw, 0, band), _band_damage(raw, band + n, band + n + band)
        if head is not None:
            msgs.append("allocation %d (shape %s, %s): %d byte(s) modified BEFORE the tensor, first at %d and last at %d "
                        "bytes relative to its start" % (idx, shape, dtype, head[2], head[0] - band, head[1] - band))
        if tail is not None:
            msgs.append("allocation %d (shape %s, %s): %d byte(s) modified AFTER the tensor, first at %d and last at %d "
                        "bytes relative to its end" % (idx, shape, dtype, tail[2], tail[0] - band - n, tail[1] - band - n))
    raise AssertionError("a store left an output tensor (fence band %d bytes): " % band + "; ".join(msgs))
