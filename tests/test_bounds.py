"""CPU checks of tests/bounds.py: half_ulp against torch's own fp16 / bf16 rounding, and check_rounded accepting correctly
rounded results while rejecting the subtly wrong ones (round toward zero, double rounding, one channel off by 2^-9) that a
max-normalised error bar lets through."""
import pytest
import torch

import bounds
from bounds import INT_SENTINEL, check_rounded, fenced, half_ulp, n_acc_for, poisoned_outputs

LP_TYPES = [torch.float16, torch.bfloat16]


def _positive_finite(dtype):
    """Every positive finite value of a 16-bit type, subnormals included, ascending (the bit patterns 1 .. max)."""
    top = 0x7BFF if dtype == torch.float16 else 0x7F7F
    return torch.arange(1, top + 1, dtype=torch.int32).to(torch.int16).view(dtype)


@pytest.mark.parametrize("dtype", LP_TYPES)
def test_half_ulp_is_half_the_spacing_of_the_type(dtype):
    v = _positive_finite(dtype)
    x = v.double()
    gap = x[1:] - x[:-1]            # the spacing above each value: one ulp of its binade (subnormals: the fixed spacing)
    assert torch.equal(2 * half_ulp(x[:-1], dtype), gap)
    assert torch.equal(half_ulp(-x, dtype), half_ulp(x, dtype))
    assert float(half_ulp(torch.tensor(0.0), dtype)) == float(half_ulp(x[0], dtype))


@pytest.mark.parametrize("dtype", LP_TYPES)
def test_half_ulp_matches_torch_rounding_at_binade_edges_and_in_subnormals(dtype):
    p, emin = (11, -14) if dtype == torch.float16 else (8, -126)
    assert float(half_ulp(torch.tensor(2.0 ** emin), dtype)) == 2.0 ** (emin - p)
    assert float(half_ulp(torch.tensor(2.0 ** (emin - 3)), dtype)) == 2.0 ** (emin - p)      # subnormal
    assert float(half_ulp(torch.tensor(1.0), dtype)) == 2.0 ** -p
    assert float(half_ulp(torch.tensor(1.0 - 2.0 ** -20), dtype)) == 2.0 ** (-1 - p)        # just under a binade edge
    edges = [2.0 ** e for e in range(emin - 2, 15)] + [1.5 * 2.0 ** emin, 3.0 * 2.0 ** (emin - 3)]
    x = torch.tensor(edges, dtype=torch.float64)
    h = half_ulp(x, dtype)
    assert torch.equal(x.to(dtype).double(), x)
    # torch (RNE) keeps a value within less than half an ulp above, moves one past it to the next value (an ulp up = 2 h)
    assert torch.equal((x + 0.99 * h).float().to(dtype).double(), x)
    assert torch.equal((x + 1.01 * h).float().to(dtype).double(), x + 2 * h)
    # the tie itself goes to the even neighbour: 2^e has an even significand
    assert torch.equal((x + h).float().to(dtype).double(), x)
    # the value below a binade edge: the spacing under 2^e is half the one above it (none in the subnormal range)
    below = torch.tensor([2.0 ** e for e in range(emin + 1, 15)], dtype=torch.float64)
    assert torch.equal(half_ulp(below - 1e-3 * half_ulp(below, dtype), dtype), half_ulp(below, dtype) / 2)


def _gemm_case(dtype, seed=0, M=300, K=512, N=96):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((M, K), generator=g).to(dtype)
    w = (torch.randn((N, K), generator=g) / K ** 0.5).to(dtype)
    b = torch.randn(N, generator=g)
    r = torch.randn((M, N), generator=g).to(dtype)
    x64, w64, r64 = x.double(), w.double(), r.double()
    exact = (x64 @ w64.t() + b.double() + r64).relu()
    mag = x64.abs() @ w64.abs().t() + b.double().abs() + r64.abs()
    acc = x.float() @ w.float().t()         # fp32 accumulation of the 16-bit operands
    return acc, b, r, exact, mag, K


def _rtz(v, dtype):
    """Round toward zero to ``dtype``: the RNE result stepped one ulp back towards zero where it rounded away."""
    r = v.to(dtype)
    away = r.double().abs() > v.double().abs()
    bits = r.view(torch.int16)
    return torch.where(away, (bits - 1).view(dtype), r)    # sign-magnitude: one less in the magnitude bits


@pytest.mark.parametrize("dtype", LP_TYPES)
def test_check_rounded_accepts_fp32_accumulation_rounded_once(dtype):
    acc, b, r, exact, mag, K = _gemm_case(dtype)
    got = (acc + b + r.float()).relu().to(dtype)
    worst, frac = check_rounded(got, exact, mag, n_acc_for(K), dtype, name="correct")
    assert worst <= 1.0 and frac > 0.99
    # fp32 output: no rounding term, the accumulation bound alone
    worst, _ = check_rounded((acc + b + r.float()).relu(), exact, mag, n_acc_for(K), torch.float32, name="fp32")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", LP_TYPES)
def test_check_rounded_rejects_round_toward_zero(dtype):
    acc, b, r, exact, mag, K = _gemm_case(dtype, seed=1)
    got = _rtz((acc + b + r.float()).relu(), dtype)
    with pytest.raises(AssertionError, match="exact-match fraction"):
        check_rounded(got, exact, mag, n_acc_for(K), dtype, name="rtz")


@pytest.mark.parametrize("dtype", LP_TYPES)
def test_check_rounded_rejects_double_rounding(dtype):
    acc, b, r, exact, mag, K = _gemm_case(dtype, seed=2)
    got = ((acc + b).to(dtype).float() + r.float()).relu().to(dtype)   # acc + bias rounded, then + residual rounded again
    with pytest.raises(AssertionError):
        check_rounded(got, exact, mag, n_acc_for(K), dtype, name="double rounding")


@pytest.mark.parametrize("dtype", LP_TYPES)
def test_check_rounded_rejects_one_channel_scaled(dtype):
    acc, b, r, exact, mag, K = _gemm_case(dtype, seed=3)
    v = (acc + b + r.float()).relu()
    # fp16: 2^-9 is two to four half-ulps; bf16 has 8 significand bits, 2^-9 is below its half-ulp: 2^-6 there
    v[:, -1] *= 1 + 2.0 ** (-9 if dtype == torch.float16 else -6)
    with pytest.raises(AssertionError, match=r"at \(\d+, %d\)" % (v.shape[1] - 1)):
        check_rounded(v.to(dtype), exact, mag, n_acc_for(K), dtype, name="scaled channel")


def test_check_rounded_rejects_non_finite_and_reports_coordinates():
    acc, b, r, exact, mag, K = _gemm_case(torch.float16, seed=4, M=40)
    got = (acc + b + r.float()).relu().to(torch.float16)
    got[17, 5] = float("nan")
    coords = torch.stack([torch.arange(40) // 20, torch.arange(40) % 20 // 4, torch.arange(40) % 4], 1)
    with pytest.raises(AssertionError, match=r"at \(0, 4, 1, 5\).*non-finite 1 of"):
        check_rounded(got, exact, mag, n_acc_for(K), torch.float16, coords=coords, name="nan")


def test_poisoned_outputs_fills_and_restores():
    real = torch.empty
    with poisoned_outputs():
        f = torch.empty((3, 4), dtype=torch.float16)
        i = torch.empty(5, dtype=torch.int32)
        like = torch.empty_like(torch.zeros(2))
    assert torch.isnan(f).all() and torch.isnan(like).all() and (i == INT_SENTINEL).all()
    assert torch.empty is real
    with pytest.raises(AssertionError):   # an element nobody wrote fails any bound
        check_rounded(f, torch.zeros(3, 4, dtype=torch.float64), torch.ones(3, 4, dtype=torch.float64), 4, torch.float16)


# ---- the fences of poisoned_outputs() and fenced(): every allocation between two canary bands -------------------------------------
BAND = 4096   # the self-tests use the smallest band; the default is checked once


def _patched():
    return (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like, torch.Tensor.new_zeros)


def test_fenced_outputs_clean_use_passes_and_everything_is_restored():
    real = _patched()
    base = torch.arange(6.0)
    with poisoned_outputs(band=BAND):
        f = torch.empty((3, 5), dtype=torch.float16)
        g = torch.empty(2, 3, dtype=torch.bfloat16)
        d = torch.empty(7)                                   # the default dtype
        i = torch.empty(5, dtype=torch.int64)
        b = torch.empty((9,), dtype=torch.uint8)
        like = torch.empty_like(base, dtype=torch.float32)
        z = torch.zeros((4, 3), dtype=torch.float32)
        zl = torch.zeros_like(base)
        nz = base.new_zeros((2, 2))
        nzi = base.new_zeros(3, dtype=torch.int32)
        f[1, 2] = 1.0                                        # a store to the interior is the kernel's business
        z += 2.0
    assert _patched() == real
    for t, shape, dtype in ((f, (3, 5), torch.float16), (g, (2, 3), torch.bfloat16), (d, (7,), torch.float32),
                            (i, (5,), torch.int64), (b, (9,), torch.uint8), (like, (6,), torch.float32),
                            (z, (4, 3), torch.float32), (zl, (6,), torch.float32), (nz, (2, 2), torch.float32),
                            (nzi, (3,), torch.int32)):
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device.type == "cpu"
        assert t.data_ptr() % 64 == 0                        # the alignment of a fresh CPU allocation
        assert t.untyped_storage().nbytes() == 2 * BAND + t.numel() * t.element_size()   # carved, tail band not rounded up
    assert float(f[1, 2]) == 1.0 and int(torch.isnan(f).sum()) == 14
    assert torch.isnan(g).all() and torch.isnan(d).all() and torch.isnan(like).all()
    assert (i == INT_SENTINEL).all() and (b == 0x5A).all()
    assert (z == 2.0).all() and (zl == 0).all() and (nz == 0).all() and (nzi == 0).all()


def test_fenced_outputs_default_band_is_one_256_row_tile_of_512_16_bit_channels():
    assert bounds.DEFAULT_BAND == 256 * 512 * 2 and bounds.DEFAULT_BAND % 4096 == 0
    with poisoned_outputs():
        t = torch.empty(3, dtype=torch.float16)
    assert t.storage_offset() * 2 == bounds.DEFAULT_BAND and t.untyped_storage().nbytes() == 2 * bounds.DEFAULT_BAND + 6
    for bad in (0, 100, 4096 + 512, -4096):
        with pytest.raises(AssertionError, match="multiple of 4096"):
            with poisoned_outputs(band=bad):
                pass


def _beyond(t, first, count):
    """The fake kernel's view: ``count`` elements of t's storage starting ``first`` elements from t's start."""
    return torch.as_strided(t, (count,), (1,), t.storage_offset() + first)


def test_fenced_outputs_reject_one_element_past_the_end():
    with pytest.raises(AssertionError, match=r"allocation 1 \(shape \(3, 5\), torch.float16\): 2 byte\(s\) modified AFTER the "
                                             r"tensor, first at 0 and last at 1 bytes relative to its end"):
        with poisoned_outputs(band=BAND):
            torch.empty(4)
            t = torch.empty((3, 5), dtype=torch.float16)
            _beyond(t, 15, 1).fill_(1.0)


def test_fenced_outputs_reject_one_element_before_the_start():
    with pytest.raises(AssertionError, match=r"allocation 0 \(shape \(6,\), torch.float32\): 4 byte\(s\) modified BEFORE the "
                                             r"tensor, first at -4 and last at -1 bytes relative to its start"):
        with poisoned_outputs(band=BAND):
            t = torch.zeros(6)
            _beyond(t, -1, 1).fill_(1.0)


def test_fenced_outputs_reject_the_last_byte_of_the_tail_band():
    with pytest.raises(AssertionError, match=r"allocation 0 \(shape \(10,\), torch.uint8\): 1 byte\(s\) modified AFTER the "
                                             r"tensor, first at %d and last at %d bytes relative to its end" % (BAND - 1, BAND - 1)):
        with poisoned_outputs(band=BAND):
            t = torch.empty(10, dtype=torch.uint8)
            _beyond(t, 10 + BAND - 1, 1).fill_(0)
    # ... and a ragged overrun reports its whole extent: rows of 3 floats written 2 rows too far
    with pytest.raises(AssertionError, match=r"24 byte\(s\) modified AFTER the tensor, first at 0 and last at 23 bytes"):
        with poisoned_outputs(band=BAND):
            t = torch.empty((5, 3))
            _beyond(t, 0, 21).fill_(0.5)


def test_fenced_outputs_accept_interior_writes_and_leave_the_body_s_own_failure_alone():
    with poisoned_outputs(band=BAND):
        t = torch.empty((5, 3))
        _beyond(t, 0, 15).fill_(0.5)
        t2 = torch.empty_like(t)
        t2.copy_(t)
    assert (t == 0.5).all() and (t2 == 0.5).all()
    real = _patched()
    with pytest.raises(ZeroDivisionError):   # the block's own exception is not replaced by a fence report
        with poisoned_outputs(band=BAND):
            t = torch.empty(3)
            _beyond(t, 3, 1).fill_(1.0)
            1 / 0
    assert _patched() == real


def test_fenced_outputs_handle_zero_sized_non_contiguous_and_channels_last():
    base = torch.arange(24.0).reshape(4, 6)
    with poisoned_outputs(band=BAND):
        e = torch.empty((0, 7), dtype=torch.float16)
        e2 = torch.empty(0)
        z = torch.zeros((3, 0), dtype=torch.int32)
        nc = torch.empty_like(base.t())                                       # keeps the permuted strides: passed through
        sl = torch.empty_like(base[:, ::2])                                   # a strided slice densifies: fenced
        cl = torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)     # passed through
        zc = torch.zeros_like(base.t())
    assert tuple(e.shape) == (0, 7) and e.dtype == torch.float16 and tuple(e2.shape) == (0,) and tuple(z.shape) == (3, 0)
    assert tuple(nc.shape) == (6, 4) and torch.isnan(nc).all()
    assert tuple(sl.shape) == (4, 3) and sl.is_contiguous() and torch.isnan(sl).all()
    assert sl.untyped_storage().nbytes() == 2 * BAND + 48
    assert cl.is_contiguous(memory_format=torch.channels_last) and torch.isnan(cl).all()
    assert tuple(zc.shape) == (6, 4) and (zc == 0).all()
    with pytest.raises(AssertionError, match=r"allocation 0 \(shape \(0, 7\), torch.float16\).*AFTER the tensor, first at 0"):
        with poisoned_outputs(band=BAND):        # a zero-sized output still has its bands: any store is outside it
            e = torch.empty((0, 7), dtype=torch.float16)
            _beyond(e, 0, 1).fill_(1.0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.int32, torch.int64, torch.uint8])
@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x7C])
def test_fenced_round_trips_the_bits_between_bands_of_the_fill(dtype, fill):
    g = torch.Generator().manual_seed(5)
    src = torch.randint(0, 256, (7 * 3 * dtype.itemsize,), generator=g, dtype=torch.uint8).view(dtype).reshape(7, 3)   # NaNs too
    t = src.t()                                                              # a non-contiguous operand
    out = fenced(t, fill, band=BAND)
    assert out.shape == t.shape and out.dtype == dtype and out.is_contiguous() and out.device == t.device
    assert torch.equal(out.view(torch.uint8), t.contiguous().view(torch.uint8))
    raw = torch.empty(0, dtype=torch.uint8).set_(out.untyped_storage())
    n = out.numel() * dtype.itemsize
    assert raw.numel() == 2 * BAND + n and out.storage_offset() * dtype.itemsize == BAND
    assert (raw[:BAND] == fill).all() and (raw[BAND + n:] == fill).all()
    # what the fills mean to a kernel that reads past an operand
    if fill == 0xFF and dtype.is_floating_point:
        assert torch.isnan(raw[:dtype.itemsize].view(dtype)).all()
    if fill == 0xFF and not dtype.is_floating_point and dtype != torch.uint8:
        assert int(raw[:dtype.itemsize].view(dtype)) == -1
    if fill == 0x7C and dtype == torch.float16:
        assert torch.isnan(raw[:2].view(dtype)).all()
    if fill == 0x7C and dtype in (torch.bfloat16, torch.float32):
        assert 1e36 < float(raw[:dtype.itemsize].view(dtype)) < 1e37


def test_fenced_keeps_zero_sized_operands_and_the_default_band():
    out = fenced(torch.zeros((0, 4), dtype=torch.int32), 0xFF)
    assert tuple(out.shape) == (0, 4) and out.untyped_storage().nbytes() == 2 * bounds.DEFAULT_BAND


def test_every_launching_entry_point_has_a_fence_case():
    """tests/test_gpu_fences.py declares, family by family, the entry points its host-path calls reach (and holds that against
    the calls really made, on the GPU). Here the declaration is held against the signature table: every entry point that takes
    a stream is reached by a family, except the read yardstick; nothing is declared that the table does not have."""
    import test_gpu_fences as T
    from torchreid import _hip
    launching = T.launching_entry_points()
    assert T.NOT_FENCED == {"agrl_diag_read_stream"} and T.NOT_FENCED <= launching
    # what does not launch: size queries, plans, switches -- none of them takes a stream
    quiet = set(_hip.SIGNATURES) - launching
    assert quiet == {"agrl_jpeg_decode_workspace", "agrl_bottleneck_seam_packed_bytes", "agrl_bottleneck_chain_enabled", "agrl_conv3x3_packed_bytes",
                     "agrl_conv1x1_packed_bytes", "agrl_col_sum_workspace", "agrl_re_ranking_workspace", "agrl_distmat_topk_workspace",
                     "agrl_bn_workspace", "agrl_conv_wgrad_workspace", "agrl_conv_wgrad_plan", "agrl_optim_geometry"}, sorted(quiet)
    declared = set(T.ENTRY_POINTS)
    assert declared <= launching, "declared but not in the signature table: %s" % sorted(declared - launching)
    missing = launching - declared - T.NOT_FENCED
    assert not missing, "entry points without a fence case in tests/test_gpu_fences.py: %s" % sorted(missing)
    for name, fams in T.ENTRY_POINTS.items():
        assert fams and all(f in T.FAMILIES and name in T.FAMILIES[f].entry_points for f in fams), name
    # every family enters checks 2 and 3; only the byte kernels and the optimisers, banded by their own tests, stay out of check 1
    unfenced = {n for n, f in T.FAMILIES.items() if not f.fence_outputs}
    assert {ep for n in unfenced for ep in T.FAMILIES[n].entry_points} == {
        "agrl_frames_normalize_u8", "agrl_frames_normalize_erase_u8", "agrl_clip_resample_u8", "agrl_jpeg_decode_u8", "agrl_png_decode_u8",
        "agrl_adam_step", "agrl_sgd_step", "agrl_rmsprop_step", "agrl_adabound_step", "agrl_radam_step"}
    assert set(T.NAMES) == set(T.FAMILIES) and set(T.FENCED) == set(T.FAMILIES) - unfenced
    # only the split-fp16 plane families may skip, and only on the bf16 build
    assert {ep for f in T.FAMILIES.values() if f.fp16_only for ep in f.entry_points} <= {
        "agrl_split16_planes", "agrl_split16_weight_planes", "agrl_conv1x1_pack", "agrl_conv3x3_pack", "agrl_conv1x1_split16", "agrl_conv1x1_split16_dual",
        "agrl_conv1x1_split16_pool", "agrl_conv3x3_packed_split16", "agrl_distmat_split16", "agrl_conv1x1_dual_split16", "agrl_row_sqnorm",
        "agrl_row_l2_normalize"}


# ---- tests/train_ref.py: the float64 references of the train-step kernels -----------------------------------------------------
# Each helper against an emulation of the stated arithmetic in torch fp32 (accepted) and against seeded faults (rejected).
import numpy as np

import train_ref as R

F32 = torch.float32


def _wgrad_case(kind="scaled", seed=0, Fr=3, H=9, W=7, Cin=8, Cout=12, Rk=3, stride=1, pad=1):
    OH, OW = (H + 2 * pad - Rk) // stride + 1, (W + 2 * pad - Rk) // stride + 1
    x, dy = R.stress_train_operands(kind, (Fr, H, W, Cin), (Fr, OH, OW, Cout), seed)
    return x, dy, (Rk, stride, pad, OH, OW)


def _wgrad_emulated(x, dy, geom, cps, drop_tile=None, drop_slice=None, drop_pixel_tap=None):
    """agrl_conv_wgrad as stated: slices of ``cps`` 32-pixel k-tiles, one fp32 rounding per 4-pixel step inside a slice, the
    slice partials added in fp32 in slice order. drop_tile = (slice, k-tile), drop_slice, drop_pixel_tap = (pixel, r, s): faults."""
    Rk, stride, pad, OH, OW = geom
    Cin, Cout = x.shape[-1], dy.shape[-1]
    xp = torch.nn.functional.pad(x.double(), (0, 0, pad, pad, pad, pad))
    d2 = dy.double().reshape(-1, Cout)
    M = d2.shape[0]
    nk = -(-M // 32)
    ks = -(-nk // cps)
    dw = torch.zeros((Cout, Cin, Rk, Rk), dtype=F32)
    for r in range(Rk):
        for s in range(Rk):
            xs = xp[:, r:r + stride * OH:stride, s:s + stride * OW:stride].reshape(-1, Cin).clone()
            if drop_pixel_tap is not None and drop_pixel_tap[1:] == (r, s):
                xs[drop_pixel_tap[0]] = 0
            total = torch.zeros((Cout, Cin), dtype=F32)
            for z in range(ks):
                acc = torch.zeros((Cout, Cin), dtype=F32)
                for kt in range(z * cps, min(nk, (z + 1) * cps)):
                    if drop_tile == (z, kt):
                        continue
                    for p0 in range(kt * 32, min(M, kt * 32 + 32), 4):
                        acc = (acc.double() + d2[p0:p0 + 4].t() @ xs[p0:p0 + 4]).float()
                if drop_slice != z:
                    total = total + acc
            dw[:, :, r, s] = total
    return dw, ks


@pytest.mark.parametrize("kind", R.KINDS)
def test_wgrad_reference_accepts_the_sliced_fp32_sum_and_rejects_seeded_faults(kind):
    x, dy, geom = _wgrad_case(kind)
    Rk, stride, pad, OH, OW = geom
    exact, mag = R.wgrad_ref(x, dy, Rk, Rk, stride, pad)
    M = dy.shape[0] * OH * OW                  # 189 pixels: 6 k-tiles, the last one partial (29 pixels)
    cps = 2
    dw, ks = _wgrad_emulated(x, dy, geom, cps)
    assert ks == 3 and M % 32
    n_acc = R.wgrad_chain(ks, cps)
    worst, _ = check_rounded(dw, exact, mag, n_acc, F32, name="wgrad emulation " + kind)
    assert worst <= 1.0
    # the last, partial k-tile of the last slice dropped
    bad, _ = _wgrad_emulated(x, dy, geom, cps, drop_tile=(ks - 1, -(-M // 32) - 1))
    with pytest.raises(AssertionError):
        check_rounded(bad, exact, mag, n_acc, F32, name="last k-tile dropped")
    # one slice left out of the reduce (sparse_dout: the slice that carries everything)
    bad, _ = _wgrad_emulated(x, dy, geom, cps, drop_slice=ks - 1)
    with pytest.raises(AssertionError):
        check_rounded(bad, exact, mag, n_acc, F32, name="slice left out")
    # one filter tap dropped in one corner: tap (0, 0) of the last pixel of the last frame (reads x[OH - 2][OW - 2]: inside)
    bad, _ = _wgrad_emulated(x, dy, geom, cps, drop_pixel_tap=(M - 1, 0, 0))
    if kind != "dead":                           # (a dead input channel contributes nothing anywhere: still rejected through the live ones)
        with pytest.raises(AssertionError, match=r"0, 0\)"):
            check_rounded(bad, exact, mag, n_acc, F32, name="corner tap dropped")
    # a single small-scale output channel multiplied by 1 + 2^-12
    if kind == "scaled":
        small = int(dy.abs().amax((0, 1, 2)).argmin())
        bad = dw.clone()
        bad[small] *= 1 + 2.0 ** -12
        with pytest.raises(AssertionError, match=r"at \(%d, " % small):
            check_rounded(bad, exact, mag, n_acc, F32, name="small channel scaled")
        # ... which the max-normalised error of test_gpu_train.py's rel() does not see
        assert ((bad.double() - exact).abs().max() / exact.abs().max()) < 1e-5


@pytest.mark.parametrize("cfg", [(3, 3, 1, 1), (3, 3, 2, 1), (1, 1, 2, 0), (7, 7, 2, 3), (1, 1, 1, 0)])
def test_dgrad_reference_is_the_transposed_conv_and_rejects_a_dropped_corner_tap(cfg):
    Rk, Sk, stride, pad = cfg
    g = torch.Generator().manual_seed(Rk + stride)
    Fr, H, W, Cin, Cout = 2, 9, 7, 8, 12
    OH, OW = (H + 2 * pad - Rk) // stride + 1, (W + 2 * pad - Sk) // stride + 1
    w = torch.randn((Cout, Cin, Rk, Sk), generator=g) * R.channel_scales(Cin, 3).view(1, Cin, 1, 1)
    dy = torch.randn((Fr, OH, OW, Cout), generator=g)
    exact, mag = R.dgrad_ref(dy, w, stride, pad, H, W)
    pix = torch.tensor([0, 1, W, H * W - 1, H * W, Fr * H * W - 1, 3 * W + 2])
    e_p, m_p = R.dgrad_ref(dy, w, stride, pad, H, W, pix=pix)        # the gather form at chosen pixels: the same sums
    assert (e_p - exact.reshape(-1, Cin)[pix]).abs().max() <= 1e-12 * mag.max() and (m_p - mag.reshape(-1, Cin)[pix]).abs().max() <= 1e-12 * mag.max()
    # autograd of the same conv in float64 is the same function
    x64 = torch.zeros((Fr, Cin, H, W), dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x64, w.double(), stride=stride, padding=pad).backward(dy.double().permute(0, 3, 1, 2))
    assert (x64.grad.permute(0, 2, 3, 1) - exact).abs().max() <= 1e-12 * mag.max()
    # the fp32 emulation: autograd in fp32 (summation order unknown, chain <= taps Cout)
    x32 = torch.zeros((Fr, Cin, H, W), requires_grad=True)
    torch.nn.functional.conv2d(x32, w, stride=stride, padding=pad).backward(dy.permute(0, 3, 1, 2).contiguous())
    got = x32.grad.permute(0, 2, 3, 1).contiguous()
    n_acc = Rk * Sk * Cout
    check_rounded(got, exact, mag, n_acc, F32, name="dgrad fp32")
    if stride > 1 and Rk == 1:
        untouched = torch.ones((H, W), dtype=torch.bool)
        untouched[::stride, ::stride] = False
        assert (exact[:, untouched] == 0).all() and (mag[:, untouched] == 0).all()
        bad = got.clone()
        bad[0, 1, 1, 0] = 1e-30                  # anything at all on a pixel the conv never sampled
        with pytest.raises(AssertionError, match=r"at \(0, 1, 1, 0\)"):
            check_rounded(bad, exact, mag, n_acc, F32, name="strided 1x1 untouched pixel")
    # one tap dropped at the corner pixel (0, 0): the output pixel / tap pair (oy, ox, r, s) = (0, 0, pad, pad)
    bad = got.double() - torch.einsum("fo,oc->fc", dy[:, 0, 0].double(), w[:, :, pad, pad].double())[:, None, None, :] * \
        torch.nn.functional.one_hot(torch.tensor(0), H * W).view(1, H, W, 1)
    with pytest.raises(AssertionError, match=r"at \(\d, 0, 0, \d\)"):
        check_rounded(bad.float(), exact, mag, n_acc, F32, name="corner tap dropped")
    # the phase chain of the 3x3 / 2 route: 1, 2 or 4 taps per input pixel
    if (Rk, stride, pad) == (3, 2, 1):
        ch = R.dgrad_chain("phase", Cout, H=H, W=W)
        assert ch.shape == (1, H, W, 1) and float(ch[0, 0, 0, 0]) == 3 + 3 and float(ch[0, 1, 1, 0]) == 4 * 3 + 3
        check_rounded(got, exact, mag, ch, F32, name="dgrad fp32, phase chain")


def test_split_bf16_constant_holds_and_is_not_slack():
    """C_SPLIT against the recipe emulated in float64 (hi = truncation, lo = RNE bf16 of the exact remainder, three exact
    products) over random and edge operands: never exceeded, and approached within a factor 4. Operands between 2^-30 and 2^30:
    the low halves stay normal."""
    g = torch.Generator().manual_seed(0)
    n = 1 << 21
    mant = torch.randint(0, 1 << 23, (2, n), generator=g, dtype=torch.int32)
    expo = torch.randint(127 - 30, 127 + 30, (2, n), generator=g, dtype=torch.int32)
    sign = torch.randint(0, 2, (2, n), generator=g, dtype=torch.int32)
    rnd = ((sign << 31) | (expo << 23) | mant).view(F32)
    edges = []
    for e in range(-30, 31, 3):
        s = 2.0 ** e
        for m in (0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x10000, 0x10001, 0x7F0000, 0x7F7FFF, 0x7F8000, 0x7FFFFF, 0x00FFFF, 0x017FFF, 0x018000):
            edges.append(s * (1 + m / float(1 << 23)))          # powers of two, all-ones mantissas, either side of a bf16 boundary
    ed = torch.tensor(edges, dtype=torch.float64).float()
    ex, ew = torch.meshgrid(ed, ed, indexing="ij")
    x = torch.cat([rnd[0], ex.reshape(-1), -ex.reshape(-1)])
    w = torch.cat([rnd[1], ew.reshape(-1), ew.reshape(-1)])
    hi, lo = R.split_bf16(x)
    assert torch.equal(hi.to(torch.bfloat16).float(), hi) and torch.equal(lo.to(torch.bfloat16).float(), lo)
    assert ((x.double() - hi.double()).abs() < 2.0 ** -7 * x.double().abs()).all()
    rel = (x.double() * w.double() - R.split_product(x, w)).abs() / (x.double() * w.double()).abs()
    assert float(rel.max()) <= R.C_SPLIT, float(rel.max())
    assert float(rel.max()) >= R.C_SPLIT / 4, float(rel.max())


def test_split_mode_bound_accepts_three_products_and_rejects_a_missing_cross_term():
    g = torch.Generator().manual_seed(1)
    M, K, N = 200, 8, 24
    x, w = torch.randn((M, K), generator=g), torch.randn((N, K), generator=g)
    exact, mag = x.double() @ w.double().t(), x.double().abs() @ w.double().abs().t()
    got = R.split_product(x[:, None, :], w[None, :, :]).sum(2).float()
    n_acc = R.gemm_chain(K)
    check_rounded(got, exact, mag, n_acc, F32, slack=R.C_SPLIT * mag, name="split")
    with pytest.raises(AssertionError):          # ... and the split arithmetic is NOT inside the exact-fp32 bound
        check_rounded(got, exact, mag, n_acc, F32, name="split against the fp32 bound")
    for drop in ("lh", "hl"):
        bad = R.split_product(x[:, None, :], w[None, :, :], drop=drop).sum(2).float()
        with pytest.raises(AssertionError):
            check_rounded(bad, exact, mag, n_acc, F32, slack=R.C_SPLIT * mag, name="split, cross term %s missing" % drop)


def _colreduce_emulated(y, rpc, nrl):
    """colreduce_vec_kernel<0> + colreduce_final_kernel<0>: per chunk and row lane an fp32 sum / fma chain, then double."""
    M, C = y.shape
    sa, sb = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for r0 in range(0, M, rpc):
        for rl in range(nrl):
            a, b = torch.zeros(C), torch.zeros(C)
            for r in range(r0 + rl, min(M, r0 + rpc), nrl):
                a = a + y[r]
                b = (y[r].double() * y[r].double() + b.double()).float()      # fmaf
            sa, sb = sa + a.double(), sb + b.double()
    mu = sa / M
    return mu.float(), (sb / M - mu * mu).clamp(min=0).float()


@pytest.mark.parametrize("kind", ["scaled", "dead", "offset"])
def test_bn_statistics_reference_accepts_the_chunked_fp32_sums(kind):
    M, C = 20000, 12
    x, _ = R.stress_train_operands(kind, (1, M, 1, C), (1, M, 1, 4), seed=2)
    y = x.view(M, C)
    chunks, rpc, nrl = R.reduce_plan(M, C)
    assert (chunks, rpc, nrl) == (417, 48, 16) and R.reduce_chain(M, C) == 3 and R.reduce_plan(700, 12) == (44, 16, 16)
    assert R.reduce_plan(65536, 64) == (512, 128, 16) and R.reduce_plan(5, 4)[0] == 1 and R.reduce_plan(4096, 2048) == (256, 16, 4)
    assert R.reduce_plan(100, 702) == (7, 16, 4) and R.reduce_lanes(702) == 0      # the scalar kernel: 4 row lanes
    mean, var = _colreduce_emulated(y, rpc, nrl)
    ref, ch = R.bn_stats_ref(y), R.bn_stats_chain(R.reduce_chain(M, C))
    check_rounded(mean, ref["mean"][0], ref["mean"][1], ch["mean"], F32, name="mean " + kind)
    check_rounded(var, ref["var"][0], ref["var"][1], ch["var"], F32, name="var " + kind)
    assert (var >= 0).all()
    if kind == "dead":
        assert (var[1::3] == 0).all() and (mean[1::3] == 0).all()
    bad = mean.clone()
    c = int(y.abs().amax(0).clamp(min=1e-30).argmin()) if kind != "dead" else 0
    bad[c] *= 1 + 2.0 ** -12
    with pytest.raises(AssertionError, match=r"at \(%d,\)" % c):
        check_rounded(bad, ref["mean"][0], ref["mean"][1], ch["mean"], F32, name="mean, one channel scaled")


@pytest.mark.parametrize("n", [1, 2, 4096])
def test_bn_fold_reference_and_the_unbiased_running_variance(n):
    g = torch.Generator().manual_seed(n)
    C = 16
    mean, var = torch.randn(C, generator=g), torch.rand(C, generator=g) * R.channel_scales(C, 5, -20, 3)
    var[3] = 0.0
    gamma, beta = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    eps, mom = 1e-5, 0.1
    e32, m32 = torch.tensor(eps, dtype=F32), torch.tensor(mom, dtype=F32)
    unb = torch.tensor(n / (n - 1) if n > 1 else 1.0, dtype=torch.float64).float()
    inv = torch.rsqrt(var + e32)
    sc = gamma * inv
    got = {"invstd": inv, "scale": sc, "shift": beta - mean * sc,
           "running_mean": (m32.double() * mean.double() + (rm * (1 - m32)).double()).float(),
           "running_var": (m32.double() * (var * unb).double() + (rv * (1 - m32)).double()).float()}
    ref = R.bn_fold_ref(mean, var, gamma, beta, eps, mom, n, rm, rv)
    for k, (exact, mag, n_acc) in ref.items():
        check_rounded(got[k], exact, mag, n_acc, F32, name="%s n=%d" % (k, n))
    assert torch.isfinite(got["invstd"]).all() and float(ref["invstd"][0][3]) == pytest.approx(1 / np.sqrt(np.float32(eps)), rel=1e-12)
    if n > 1:   # n / (n - 1) missing from running_var: off by 2 at n = 2, by 2.4e-4 at n = 4096
        bad = (m32.double() * var.double() + (rv * (1 - m32)).double()).float()
        exact, mag, n_acc = ref["running_var"]
        with pytest.raises(AssertionError):
            check_rounded(bad, exact, mag, n_acc, F32, name="running_var without n / (n - 1)")
        exact, mag, n_acc = R.bn_fold_ref(mean, var, gamma, beta, eps, mom, n, rm, rv, unbias=False)["running_var"]
        check_rounded(bad, exact, mag, n_acc, F32, name="the fault against the faulty formula")


@pytest.mark.parametrize("cfg", [(7, 12, True, 0.0, True), (5, 4, True, 0.1, False), (9, 20, False, 0.0, True)])
def test_bn_apply_reference_and_the_sign_mask(cfg):
    M, C, relu, slope, use_res = cfg
    g = torch.Generator().manual_seed(M * C)
    y, res = torch.randn((M, C), generator=g), (torch.randn((M, C), generator=g) if use_res else None)
    scale, shift = torch.randn(C, generator=g) * R.channel_scales(C, 1), torch.randn(C, generator=g)
    pre = (y.double() * scale.double() + shift.double()).float()        # fmaf
    if use_res:
        pre = pre + res
    out = torch.where(pre > 0, pre, pre * torch.tensor(slope, dtype=F32)) if relu else pre
    exact, mag, n_acc = R.bn_apply_ref(y, scale, shift, res, relu, slope)
    check_rounded(out, exact, mag, n_acc, F32, name="bn_apply")
    if not relu:
        return
    assert (M * C // 4) % 2 == 1, "an odd number of float4s: the last mask byte holds one nibble"
    mask = R.pack_sign_mask(pre.reshape(-1) > 0)
    assert mask.numel() == (M * C + 7) // 8 and torch.equal(R.unpack_sign_mask(mask, M * C), pre.reshape(-1) > 0)
    R.check_sign_mask(mask, out, "mask")
    shifted = R.pack_sign_mask(torch.roll(pre.reshape(-1) > 0, 1))       # every nibble shifted by one element
    with pytest.raises(AssertionError, match="mask bytes differ"):
        R.check_sign_mask(shifted, out, "mask shifted by one element")
    one = mask.clone()
    one[-1] ^= 0x10                                                     # a bit in the unused nibble of the last byte
    with pytest.raises(AssertionError, match="mask bytes differ"):
        R.check_sign_mask(one, out, "unused nibble set")


def test_bn_backward_reference_accepts_the_fp32_formula():
    g = torch.Generator().manual_seed(4)
    M, C = 300, 12
    x, _ = R.stress_train_operands("offset", (1, M, 1, C), (1, M, 1, 4), seed=4)
    y, dz = x.view(M, C), torch.randn((M, C), generator=g) * R.channel_scales(C, 9)
    st = R.bn_stats_ref(y)
    mean, invstd = st["mean"][0].float(), (1 / torch.sqrt(st["var"][0].clamp(min=0) + 1e-5)).float()
    gamma = 0.5 + torch.rand(C, generator=g)
    xh = (y - mean) * invstd
    s1, s2 = dz.sum(0), (dz * xh).sum(0)
    sums, ch = R.bn_backward_sums_ref(dz, y, mean, invstd), R.bn_backward_sums_chain(M, False)
    check_rounded(s1, sums["dbeta"][0], sums["dbeta"][1], ch["dbeta"], F32, name="dbeta")
    check_rounded(s2, sums["dgamma"][0], sums["dgamma"][1], ch["dgamma"], F32, name="dgamma")
    inv_m = torch.tensor(1.0, dtype=F32) / torch.tensor(float(M), dtype=F32)
    dy = gamma * invstd * (dz - s1 * inv_m - xh * (s2 * inv_m))
    exact, mag, n_acc = R.bn_backward_ref(dz, y, mean, invstd, gamma, s1, s2)
    check_rounded(dy, exact, mag, n_acc, F32, name="bn_backward apply")
    bad = dy.clone()
    bad[:, 5] *= 1 + 2.0 ** -12
    with pytest.raises(AssertionError, match=r", 5\)"):
        check_rounded(bad, exact, mag, n_acc, F32, name="bn_backward, one channel scaled")


@pytest.mark.parametrize("shape", [(2, 9, 7, 5), (1, 2, 2, 3), (2, 16, 8, 4)])
def test_maxpool_reference_first_maximum_and_its_gradient(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g).relu()                           # post-ReLU: ties at zero in most windows
    out, idx = R.maxpool_ref(x)
    ref = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(out, ref)
    Fr, H, W, C = shape
    # the recorded tap holds the maximum, and no earlier tap of the window does
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1), value=float("-inf"))
    for f, oh, ow, c in [(0, 0, 0, 0), (Fr - 1, out.shape[1] - 1, out.shape[2] - 1, C - 1), (0, out.shape[1] // 2, 0, 1)]:
        win = xp[f, 2 * oh:2 * oh + 3, 2 * ow:2 * ow + 3, c].reshape(-1)
        first = int(torch.nonzero(win == win.max())[0])
        assert int(idx[f, oh, ow, c]) == first
    dout = torch.randn(out.shape, generator=g)
    dx = R.maxpool_backward_ref(dout, idx, H, W)
    assert abs(float(dx.double().sum() - dout.double().sum())) < 1e-4 and dx.shape == x.shape
    zero = torch.zeros(dx.shape, dtype=torch.float64)
    check_rounded(dx, dx.double(), zero, 0, F32, name="maxpool backward")
    # the gradient sent to the LAST maximum of a window instead of the first
    _, idx_last = R.maxpool_ref(x, last=True)
    assert not torch.equal(idx_last, idx)
    with pytest.raises(AssertionError):
        check_rounded(R.maxpool_backward_ref(dout, idx_last, H, W), dx.double(), zero, 0, F32, name="maxpool backward, last maximum")
    # where the input is positive and unique the two agree: what test_gpu_train.py's comparison was restricted to


def test_tail_references_accept_fp32_emulations():
    g = torch.Generator().manual_seed(8)
    a_, b_ = torch.randn((5, 7, 64), generator=g), torch.randn((5, 7, 64), generator=g)
    exact, mag, n_acc = R.axpby_ref(0.9, a_, 0.1, b_)
    check_rounded(torch.tensor(0.9, dtype=F32) * a_ + torch.tensor(0.1, dtype=F32) * b_, exact, mag, n_acc + 1, F32, name="axpby")
    Fr, S, h, w, C, splits = 4, 2, 6, 3, 8, (4, 2, 1)
    dg, dn = torch.randn((Fr // S, C), generator=g), torch.randn((Fr, 7, C), generator=g)
    x1 = torch.randn((Fr, C, h, w), generator=g, requires_grad=True)
    x2 = torch.randn((Fr, C, h, w), generator=g, requires_grad=True)
    gl = x1.view(Fr // S, S, C, h * w).permute(0, 2, 1, 3).reshape(Fr // S, C, -1).mean(2)
    nodes = torch.cat([torch.nn.functional.adaptive_avg_pool2d(x2, (n, 1)).view(Fr, C, n) for n in splits], 2).transpose(1, 2)
    ((gl * dg).sum() + (nodes * dn).sum()).backward()
    (e1, m1, n1), (e2, m2, n2) = R.part_pool_backward_ref(dg, dn, S, h, w, splits)
    check_rounded(x1.grad.permute(0, 2, 3, 1), e1, m1, n1, F32, name="part pool dx1")
    check_rounded(x2.grad.permute(0, 2, 3, 1), e2, m2, n2, F32, name="part pool dx2")
    A, Bm = torch.randn((2, 9, 256), generator=g), torch.randn((2, 9, 256), generator=g)
    exact, mag, n_acc = R.pair_product_ref(A, Bm)
    check_rounded(torch.bmm(A, Bm.transpose(1, 2)), exact, mag, 256, F32, name="pair product")
    assert n_acc == 32 + 2 + 3
    for n, K in ((16, 702), (4, 5)):
        z = (3 * torch.randn((n, K), generator=g)).requires_grad_(True)
        y = torch.randint(0, K, (n,), generator=g)
        logp = torch.log_softmax(z, 1)
        q = torch.zeros(n, K).scatter_(1, y[:, None], 1.0) * (1 - 0.1) + 0.1 / K
        loss = (-q * logp).mean(0).sum()
        loss.backward()
        (l64, lb), (d64, db) = R.xent_ref(z.detach(), y, 0.1)
        zero = torch.zeros_like(d64)
        check_rounded(z.grad, d64, zero, 0, F32, slack=db, name="xent dlogits")
        check_rounded(loss.detach().view(1), l64, torch.zeros(1, dtype=torch.float64), 0, F32, slack=lb, name="xent loss")
        bad = z.grad.clone()
        bad[1, int(y[1])] += 2.0 ** -12 / n * (1 - 0.1)                   # the target's q off by 2^-12 relative
        with pytest.raises(AssertionError):
            check_rounded(bad, d64, zero, 0, F32, slack=db, name="xent dlogits, q wrong")


def test_attention_pool_and_triplet_references_accept_fp32_autograd():
    g = torch.Generator().manual_seed(0)
    nodes = torch.rand((3, 6, 7, 128), generator=g)
    nodes[1, 2, 3] = 0                       # an all-zero node: by convention its norm passes no gradient
    nodes.requires_grad_(True)
    att = torch.nn.functional.normalize(nodes.norm(p=2, dim=3, keepdim=True), p=1, dim=1)
    a = (nodes * att).sum(1).mean(1)
    da = torch.randn(a.shape, generator=g)
    a.backward(da)
    exact, mag, n_acc = R.attn_pool_backward_ref(nodes.detach(), da)
    check_rounded(nodes.grad, exact, mag, n_acc, F32, name="attention pool backward")
    assert n_acc == 5 * 10 + 3 * 6 + 16 and bool((exact[1, 2, 3] == 0).all() and (mag[1, 2, 3] == 0).all())
    bad = nodes.grad.clone()
    bad[2, 5, 6] *= 1 + 2.0 ** -12
    with pytest.raises(AssertionError, match=r"at \(2, 5, 6, "):
        check_rounded(bad, exact, mag, n_acc, F32, name="attention pool backward, one node scaled")
    n, d = 16, 64
    for soft in (True, False):
        x = torch.randn((n, d), generator=g).requires_grad_(True)
        pids = torch.arange(4).repeat_interleave(4)
        dist = (x.pow(2).sum(1)[:, None] + x.pow(2).sum(1)[None, :] - 2 * x @ x.t()).clamp(min=1e-12).sqrt()
        same = pids[:, None] == pids[None, :]
        dap, iap = (dist - 1e9 * (~same)).max(1)
        dan, ian = (dist + 1e9 * same).min(1)
        loss = torch.nn.functional.softplus(dap - dan).mean() if soft else (dap - dan + 0.3).clamp(min=0).mean()
        loss.backward()
        r = R.triplet_ref(x.detach(), pids, 0.3, soft, dap.detach(), dan.detach(), iap, ian)
        zero = torch.zeros(n, dtype=torch.float64)
        check_rounded(x.grad, r["grad"][0], r["grad"][1], r["grad"][2], F32, name="triplet grad")
        check_rounded(loss.detach().view(1), r["loss"][0], zero[:1], 0, F32, slack=r["loss"][3], name="triplet loss")
        check_rounded(dap.detach(), r["dist_ap"][0], zero, 0, F32, slack=r["dist_ap"][3], name="triplet d_ap")
        check_rounded(dan.detach(), r["dist_an"][0], zero, 0, F32, slack=r["dist_an"][3], name="triplet d_an")
        bad = x.grad.clone()
        bad[int(iap[0])] += (x.detach()[0] - x.detach()[int(iap[0])]) * 2.0 ** -12 / n     # one scattered term 2^-12 too large
        if float(dap[0].detach()) > 0 and (soft or float(loss.detach()) > 0):
            with pytest.raises(AssertionError):
                check_rounded(bad, r["grad"][0], r["grad"][1], r["grad"][2], F32, name="triplet grad, one term scaled")


@pytest.mark.parametrize("cfg", [(3, 56, 256, True), (2, 28, 128, False)])
def test_graph_matrix_backward_reference_accepts_the_fp32_formulas(cfg):
    """The kernel's formulas step by step in torch fp32 stay inside the propagated bound; the same with the diagonal passing a
    gradient (sqrt'(1e-12) on E_ii, what the kernel's convention excludes) or one off-diagonal E off by 2^-10 does not."""
    B, V, C, use_pose = cfg
    g = torch.Generator().manual_seed(V + C)
    f = torch.rand((B, 1, C), generator=g) * 0.2 + 0.05 * torch.randn((B, V, C), generator=g)
    gp = torch.stack([torch.bmm(f[:, :, z:z + 128], f[:, :, z:z + 128].transpose(1, 2)) for z in range(0, C, 128)], 1)
    dG = torch.randn((B, V, V), generator=g)
    exact, slack, live = R.graph_matrix_backward_ref(gp, dG, use_pose)
    eye = torch.eye(V, dtype=torch.bool)
    assert bool(live[:, ~eye].all()) and not bool(live[:, eye].any())

    def emulate(diag_gradient=False, scale_one=False):
        gs = gp.sum(1)
        n = torch.diagonal(gs, dim1=1, dim2=2)
        d2 = ((n[:, None, :] + n[:, :, None]) - 2 * gs).clamp(min=1e-12)
        d = d2.sqrt()
        S = 2 / (torch.exp(d) + 1)
        r = S.sum(2, keepdim=True)
        x = dG * (0.5 if use_pose else 1.0)
        c = (x * (S / r)).sum(2, keepdim=True)
        dD = -S * (1 - 0.5 * S) * ((x - c) / r)
        E = dD / (2 * d)
        if not diag_gradient:
            E = torch.where(eye | ~(d2 > 1e-12), torch.zeros_like(E), E)
        if scale_one:
            E[0, 1, 2] *= 1 + 2.0 ** -10
        T = E + E.transpose(1, 2)
        return 2 * (torch.diag_embed(T.sum(2)) - T)
    zero = torch.zeros_like(exact)
    worst, _ = check_rounded(emulate(), exact, zero, 0, F32, slack=slack, name="graph matrix backward")
    assert worst > 0.01, "the propagated bound is within two orders of what fp32 does"
    for fault in ({"diag_gradient": True}, {"scale_one": True}):
        with pytest.raises(AssertionError):
            check_rounded(emulate(**fault), exact, zero, 0, F32, slack=slack, name="graph matrix backward, fault")


# ---- tests/graph_ref.py: the float64 references of the eval GraphLayer and the attention tail ------------------------------------
# Each helper against the kernel's stated arithmetic stepped in torch fp32 (accepted, and within two orders of the bound:
# worst > 0.01) and against seeded faults (rejected, at the reported coordinate where check_rounded can name it).
import graph_ref as GR


def _old_graph_matrix_backward_ref(gram_part, dG, use_pose, mask_diag=False):
    """graph_matrix_backward_ref as it stood before its stages up to Shat moved to graph_ref.similarity_chain."""
    u = R.U32
    gp = gram_part.double()
    B, nz, V, _ = gp.shape
    g, a = gp.sum(1), nz * u * gp.abs().sum(1)
    n, an = torch.diagonal(g, dim1=1, dim2=2), torch.diagonal(a, dim1=1, dim2=2)
    eye = torch.eye(V, dtype=torch.bool).view(1, V, V)
    D2 = n[:, :, None] + n[:, None, :] - 2 * g
    eD2 = an[:, :, None] + an[:, None, :] + 2 * a + 2 * u * (n[:, :, None] + n[:, None, :] + 2 * g.abs())
    eD2 = eD2.masked_fill(eye, 0.0)
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
    Sh = S / r
    eSh = Sh * (eS / S.clamp(min=1e-300) + er / r + u)
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


def _gram_partials(f):
    """agrl_graph_gram's output shape: 128-channel slice partials (B, C / 128, V, V), fp32."""
    return torch.stack([torch.bmm(f[:, :, z:z + 128], f[:, :, z:z + 128].transpose(1, 2)) for z in range(0, f.shape[-1], 128)], 1)


@pytest.mark.parametrize("mask_diag", [False, True])
@pytest.mark.parametrize("use_pose", [False, True])
def test_graph_matrix_backward_reference_is_unchanged_by_the_shared_chain(use_pose, mask_diag):
    g = torch.Generator().manual_seed(11)
    f = torch.rand((2, 1, 256), generator=g) * 0.2 + 0.05 * torch.randn((2, 28, 256), generator=g)
    gp, dG = _gram_partials(f), torch.randn((2, 28, 28), generator=g)
    for new, old in zip(R.graph_matrix_backward_ref(gp, dG, use_pose, mask_diag), _old_graph_matrix_backward_ref(gp, dG, use_pose, mask_diag)):
        assert torch.equal(new, old)


def _finalize_fp32(gp, adj, use_pose, learn_graph, mask_diag, norms=None):
    """graph_finalize_kernel step by step in fp32. ``norms``: squared norms from another sum than the Gram diagonal (a fault: the
    diagonal distance becomes fp32 cancellation noise instead of 0)."""
    B, nz, V, _ = gp.shape
    eye = torch.eye(V, dtype=torch.bool)
    if learn_graph:
        gs = torch.zeros((B, V, V))
        for z in range(nz):
            gs = gs + gp[:, z]
        n = torch.diagonal(gs, dim1=1, dim2=2) if norms is None else norms
        d2 = ((n[:, None, :] + n[:, :, None]) - 2 * gs).clamp(min=1e-12)
        sim = 2 / (torch.exp(torch.sqrt(d2)) + 1)
        if mask_diag:
            sim = sim.masked_fill(eye, 0.0)
        Sh = sim / sim.abs().sum(2, keepdim=True).clamp(min=1e-12)
    if use_pose:
        a = adj.masked_fill(eye, 0.0) if mask_diag else adj
        A = a / a.abs().sum(2, keepdim=True).clamp(min=1e-12)
        return (A + Sh) / 2 if learn_graph else A
    return Sh


def _graph_inputs(B, V, C, seed):
    """The well-conditioned node features of the GPU suite: independent rows, |f|^2 ~ 8, d2 ~ 16."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((B, V, C), generator=g) * 4 / (2 * C) ** 0.5
    adj = (torch.rand((B, V, V), generator=g) > 0.5).float()
    adj[0, min(3, V - 1)] = 0                          # an all-zero adjacency row
    return f, adj


@pytest.mark.parametrize("cfg", [(3, 56, 256, True, True, False), (2, 20, 128, False, True, False), (2, 33, 128, True, True, True),
                                 (2, 28, 512, True, False, False), (2, 1, 128, True, True, True)])
def test_graph_matrix_reference_accepts_the_fp32_formulas_and_rejects_seeded_faults(cfg):
    B, V, C, use_pose, learn_graph, mask_diag = cfg
    f, adj = _graph_inputs(B, V, C, V + C)
    gp = _gram_partials(f)
    exact, slack = GR.graph_matrix_ref(gp, adj, use_pose, learn_graph, mask_diag)
    packed, _ = GR.graph_matrix_ref(gp, _pack_bits(adj), use_pose, learn_graph, mask_diag)
    assert torch.equal(packed, exact), "the bit-packed adjacency unpacks to the same graph"
    zero = torch.zeros_like(exact)
    assert bool((slack <= 128 * R.U32 * exact.abs()).all()), "the reference alone is within 128 u |G| on these inputs"
    got = _finalize_fp32(gp, adj, use_pose, learn_graph, mask_diag)
    worst, _ = check_rounded(got, exact, zero, 0, F32, slack=slack, name="graph matrix")
    if V == 1:
        assert float(exact.abs().max()) == 0.0       # the one node masked out on both halves: 0 / clamp
        return
    assert worst > 0.01, "the propagated bound is within two orders of what fp32 does"
    if learn_graph:
        bad = got.clone()
        bad[1, 2, 5] *= 1 + 2.0 ** -12               # one off-diagonal entry: 2^12 u, against a slack of at most 128 u
        with pytest.raises(AssertionError, match=r"at \(1, 2, 5\)"):
            check_rounded(bad, exact, zero, 0, F32, slack=slack, name="graph matrix, one entry scaled")
        # ... which a 5e-4 max-normalised bar does not see
        assert float((bad.double() - exact).abs().max() / exact.abs().max()) < 5e-4
        if not mask_diag:
            noisy = _finalize_fp32(gp, adj, use_pose, learn_graph, mask_diag, norms=(f * f).sum(2))
            with pytest.raises(AssertionError):
                check_rounded(noisy, exact, zero, 0, F32, slack=slack, name="graph matrix, diagonal distance from cancellation noise")
    if use_pose and not learn_graph:
        bad = _finalize_fp32(gp, adj.transpose(1, 2).contiguous(), True, False, mask_diag)
        with pytest.raises(AssertionError):
            check_rounded(bad, exact, zero, 0, F32, slack=slack, name="adjacency transposed")


def _pack_bits(adj):
    """The bit-packed adjacency (hip_ops.adjacency_pack_host's layout) without importing the package."""
    a = adj.numpy() != 0
    B, V, _ = a.shape
    W = (V + 31) // 32
    pad = np.zeros((B, V, W * 32), dtype=bool)
    pad[:, :, :V] = a
    words = (pad.reshape(B, V, W, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=3).astype(np.uint32)
    return torch.from_numpy(words.view(np.int32).copy())


def test_tracklet_gram_reference_accepts_eight_wave_partials():
    f, adj = _graph_inputs(2, 20, 512, 5)
    C = f.shape[-1]
    cq = C // GR.GT_WAVES
    gram = torch.zeros((2, 20, 20))
    for w in range(GR.GT_WAVES):                      # wave partials of C / 8 channels, added in wave order
        part = torch.zeros((2, 20, 20))
        for c in range(w * cq, (w + 1) * cq, 4):
            part = (part.double() + torch.bmm(f[:, :, c:c + 4].double(), f[:, :, c:c + 4].double().transpose(1, 2))).float()
        gram = gram + part
    exact, bound = GR.tracklet_gram_ref(f)
    zero = torch.zeros_like(exact)
    worst, _ = check_rounded(gram, exact, zero, 0, F32, slack=bound, name="tracklet gram")
    assert worst > 0.01
    bad = gram - torch.bmm(f[:, :, -4:], f[:, :, -4:].transpose(1, 2))       # the last MFMA step of the last wave dropped
    with pytest.raises(AssertionError):
        check_rounded(bad, exact, zero, 0, F32, slack=bound, name="tracklet gram, last step dropped")
    # the finalize propagation on this Gram: the fp32 graph of the emulated Gram is inside it
    G, slack = GR.graph_matrix_ref(None, adj, True, True, False, gram=(exact, bound))
    got = _finalize_fp32(gram[:, None], adj, True, True, False)
    check_rounded(got, G, zero, 0, F32, slack=slack, name="tracklet graph")
    P, pmag, n_acc = GR.apply_ref(got, f)
    worst, _ = check_rounded(torch.bmm(got, f), P, pmag, n_acc, F32, name="P = G f")
    assert worst > 0.01 and n_acc == 5 + 3
    with pytest.raises(AssertionError):
        check_rounded(torch.bmm(got.transpose(1, 2), f), P, pmag, n_acc, F32, name="P = G^T f")


def test_propagate_form_mirrors_the_dispatch():
    want = {(4, 256): "stream4", (28, 256): "stream4", (64, 512): "stream4", (56, 128): "stream2", (20, 384): "stream2",
            (1, 128): "mfma4", (3, 256): "mfma4", (49, 128): "mfma4", (63, 128): "mfma4", (65, 128): "mfma8", (112, 256): "mfma8",
            (128, 128): "mfma8", (20, 260): "generic", (130, 128): "generic", (146, 128): "generic", (147, 128): "tiled",
            (148, 128): "tiled", (149, 128): "tiled", (240, 132): "tiled"}
    for (V, C), form in want.items():
        got, n_acc = GR.propagate_form(V, C)
        assert got == form, (V, C, got)
        assert n_acc == (-(-V // 4) if form[0] in "sm" else V) + GR.EPILOGUE == GR.form_chain(form, V)
    # the LDS-resident generic form holds V (Vp + 128) floats, Vp = V rounded up to 8: 146 fits 160 KB, 147 does not
    assert (146 * (152 + 128)) * 4 <= GR.LDS_BYTES < (147 * (152 + 128)) * 4


def _message_fp32(f, h, G, scale, shift, keep, gamma, slope, form, drop_last_row_of=None, slope_on_positive=False):
    """The message-pass kernels step by step in fp32: one rounding per 4-deep MFMA step (stream, MFMA) or per fma (generic,
    tiled), then fmaf(acc, scale, shift), the LeakyReLU, keep f + gamma y."""
    B, V, C = f.shape
    step = 4 if form[0] in "sm" else 1
    acc = torch.zeros((B, V, C))
    Gd = G.double().clone()
    if drop_last_row_of is not None:
        b, v = drop_last_row_of
        Gd[b, v, V - 1] = 0
    for u0 in range(0, V, step):
        acc = (acc.double() + torch.bmm(Gd[:, :, u0:u0 + step], h[:, u0:u0 + step].double())).float()
    y = (acc.double() * scale.double() + shift.double()).float()
    s = torch.tensor(slope, dtype=F32)
    y = torch.where((y <= 0) if slope_on_positive else (y > 0), y, s * y)
    return torch.tensor(keep, dtype=F32) * f + torch.tensor(gamma, dtype=F32) * y


def _double_rounded(v, dtype):
    """fp32 -> one significand bit more than ``dtype`` keeps -> ``dtype``: a copy rounded twice."""
    p = 11 if dtype == torch.float16 else 8
    m, e = torch.frexp(v.double())
    mid = torch.ldexp(torch.round(m * 2.0 ** (p + 1)) / 2.0 ** (p + 1), e)
    return mid.float().to(dtype)


@pytest.mark.parametrize("dtype", LP_TYPES)
@pytest.mark.parametrize("cfg", [(2, 28, 256, 0.9, 0.1), (2, 49, 128, 1.0, 0.3), (2, 20, 260, 0.0, 1.0), (1, 149, 128, 1.0, 0.3)])
def test_message_reference_accepts_each_form_and_rejects_seeded_faults(cfg, dtype):
    B, V, C, keep, gamma = cfg
    form, n_acc = GR.propagate_form(V, C)
    g = torch.Generator().manual_seed(V + C)
    f, h = torch.randn((B, V, C), generator=g), torch.randn((B, V, C), generator=g) * R.channel_scales(C, 3, -8, 2)
    G = torch.randn((B, V, V), generator=g) / V ** 0.5
    scale, shift = torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    slope = 0.1
    exact, mag, n = GR.message_ref(f, h, G, scale, shift, keep, gamma, slope, form)
    assert n == n_acc
    got = _message_fp32(f, h, G, scale, shift, keep, gamma, slope, form)
    worst, _ = check_rounded(got, exact, mag, n, F32, name="message " + form)
    assert worst > 0.01, "n_acc is within two orders of what fp32 does"
    # the last graph row u = V - 1 dropped from one output node
    bad = _message_fp32(f, h, G, scale, shift, keep, gamma, slope, form, drop_last_row_of=(B - 1, V // 2))
    with pytest.raises(AssertionError, match=r"at \(%d, %d, \d+\)" % (B - 1, V // 2)):
        check_rounded(bad, exact, mag, n, F32, name="message, last graph row dropped")
    # G used transposed
    with pytest.raises(AssertionError):
        check_rounded(_message_fp32(f, h, G.transpose(1, 2), scale, shift, keep, gamma, slope, form), exact, mag, n, F32, name="message, G^T")
    # slope applied to the positive side
    with pytest.raises(AssertionError):
        check_rounded(_message_fp32(f, h, G, scale, shift, keep, gamma, slope, form, slope_on_positive=True), exact, mag, n, F32, name="message, slope on the wrong side")
    # keep taken as fp32 1 - gamma where the host passes another keep (ganet: keep = 1; P = G f: keep = 0)
    if abs(keep - (1 - gamma)) > 1e-3:
        wrong = float(torch.tensor(1.0) - torch.tensor(gamma, dtype=F32))
        with pytest.raises(AssertionError):
            check_rounded(_message_fp32(f, h, G, scale, shift, wrong, gamma, slope, form), exact, mag, n, F32, name="message, keep = 1 - gamma")
    else:   # the reference's Python-float 1 - gamma rounded once is what the host passes: the fp32 difference may be an ulp off, inside the bound
        wrong = float(torch.tensor(1.0) - torch.tensor(gamma, dtype=F32))
        check_rounded(_message_fp32(f, h, G, scale, shift, wrong, gamma, slope, form), exact, mag, n, F32, name="message, fp32 1 - gamma")
    # the 16-bit copy: the one rounding of the fp32 output, every element; a copy rounded twice is not
    zero = torch.zeros_like(exact)
    check_rounded(got.to(dtype), got.double(), zero, 0, dtype, min_exact_frac=1.0, name="out_lp")
    check_rounded(got.to(dtype), exact, mag, n, dtype, name="out_lp against float64")
    with pytest.raises(AssertionError, match="exact-match fraction"):
        check_rounded(_double_rounded(got, dtype), got.double(), zero, 0, dtype, min_exact_frac=1.0, name="out_lp rounded twice")


@pytest.mark.parametrize("mode", GR.LINEAR_MODES)
@pytest.mark.parametrize("shape", [(84, 64, 128), (129, 192, 256)])
def test_linear_mix_reference_accepts_each_mode(shape, mode):
    M, K, N = shape
    g = torch.Generator().manual_seed(M + K)
    P, W = torch.randn((1, M, K), generator=g), torch.randn((N, K), generator=g) / K ** 0.5
    f = torch.randn((1, M, N), generator=g)
    scale, shift = torch.randn(N, generator=g), 0.3 * torch.randn(N, generator=g)
    if mode == "lp16":
        P, W = P.half().float(), W.half().float()
    exact, mag, n_acc, slack = GR.linear_mix_ref(P, W, f, scale, shift, 1.0, 0.3, 0.1, mode)
    assert n_acc == n_acc_for(K, 16 if mode == "lp16" else 4) + 4

    def emulate(k_end=K, slope_on_positive=False):
        if mode == "bf16x3":
            acc = R.split_product(P[0, :, None, :k_end], W[None, :, :k_end]).sum(2).float()
        elif mode == "fp16x3":
            ph, wh = P[0].half(), W.half()
            pl, wl = (P[0] - ph.float()).half(), (W - wh.float()).half()
            acc = (ph.double()[:, :k_end] @ wh.double()[:, :k_end].t() + pl.double()[:, :k_end] @ wh.double()[:, :k_end].t()
                   + ph.double()[:, :k_end] @ wl.double()[:, :k_end].t()).float()
        else:
            acc = P[0, :, :k_end] @ W[:, :k_end].t()
        y = (acc.double() * scale.double() + shift.double()).float()
        y = torch.where((y <= 0) if slope_on_positive else (y > 0), y, torch.tensor(0.1) * y)
        return torch.tensor(1.0) * f[0] + torch.tensor(0.3) * y
    worst, _ = check_rounded(emulate(), exact, mag, n_acc, F32, slack=slack, name="linear mix " + mode)
    assert worst > 0.01 or mode == "fp16x3"      # (fp16x3 has its own constant, split16_ref.C_SPLIT16; this emulation splits W of order
                                                 # K^-1/2 without the pre-scale, which costs 2^-25 per weight: inside the chain's allowance here)
    for fault in ({"k_end": K - 32}, {"slope_on_positive": True}):       # the last half k-tile never multiplied; slope on the wrong side
        with pytest.raises(AssertionError):
            check_rounded(emulate(**fault), exact, mag, n_acc, F32, slack=slack, name="linear mix, fault")
    rows = torch.tensor([0, M - 1])
    e2, m2, _, s2 = GR.linear_mix_ref(P, W, f, scale, shift, 1.0, 0.3, 0.1, mode, rows=rows)
    tiny = 1e-12 * float(mag.max())          # the same sums on a row subset (float64 BLAS: another blocking)
    assert float((e2 - exact[rows]).abs().max()) <= tiny and float((m2 - mag[rows]).abs().max()) <= tiny and float((s2 - slack[rows]).abs().max()) <= tiny


def _attn_pool_fp32(nodes, sqn, gsum, gs, gsh, as_, ash, hw, over_parts=None):
    """attn_pool_bnneck_kernel step by step in fp32."""
    B, S, P, C = nodes.shape
    n = torch.sqrt(sqn).view(B, S, P)
    tot = torch.zeros((B, P))
    for s in range(S):
        tot = tot + n[:, s]
    a = n / tot.clamp(min=1e-12)[:, None, :]
    if over_parts is not None:
        b_, s_, p_ = over_parts
        a[b_, s_, p_] = n[b_, s_, p_] / n[b_, s_].sum().clamp(min=1e-12)
    att = torch.zeros((B, C))
    for p in range(P):
        fuse = torch.zeros((B, C))
        for s in range(S):
            fuse = (a[:, s, p, None].double() * nodes[:, s, p].double() + fuse.double()).float()
        att = att + fuse
    att = att / torch.tensor(float(P))
    gg = torch.zeros((B, C))
    for s in range(S):
        gg = gg + gsum.view(B, S, C)[:, s]
    gg = gg * (torch.tensor(1.0) / (torch.tensor(float(S)) * torch.tensor(float(hw))))
    out = torch.cat([(gg.double() * gs.double() + gsh.double()).float(), (att.double() * as_.double() + ash.double()).float()], 1)
    return out, gg, att


@pytest.mark.parametrize("cfg", [(3, 8, 7, 256, 128), (2, 3, 5, 260, 60), (1, 9, 1, 4, 1)])
def test_attention_pool_reference_accepts_the_fp32_formulas(cfg):
    B, S, P, C, hw = cfg
    g = torch.Generator().manual_seed(S * P + C)
    nodes = torch.rand((B, S, P, C), generator=g) * R.channel_scales(C, 2, -10, 2)
    nodes[B - 1, min(2, S - 1)] = 0          # a frame whose nodes are all zero
    if P > 1:
        nodes[0, :, P - 1] = 0               # a part that is zero in every frame: the denominator sits at the clamp
    gsum = torch.rand((B * S, C), generator=g) * hw * R.channel_scales(C, 4, -10, 2)
    one, zero_ = torch.ones(C), torch.zeros(C)
    sqn = (nodes * nodes).sum(3).reshape(-1)
    ref = GR.attn_pool_ref(nodes, sqn, gsum, one, zero_, one, zero_, hw)
    out, gf, af = _attn_pool_fp32(nodes, sqn, gsum, one, zero_, one, zero_, hw)
    worst = [check_rounded(t, *ref[k], F32, name="attn pool " + k)[0] for k, t in (("out", out), ("g_f", gf), ("att_f", af))]
    assert min(worst) > 0.01, worst
    if P > 1:
        assert float(ref["att_f"][0][0].abs().max()) > 0 and bool(torch.isfinite(out).all())
        s_ = 0 if S == 1 else 1
        _, _, bad = _attn_pool_fp32(nodes, sqn, gsum, one, zero_, one, zero_, hw, over_parts=(0, s_, 0))
        with pytest.raises(AssertionError, match=r"at \(0, \d+\)"):
            check_rounded(bad, *ref["att_f"], F32, name="attention weight normalised over the parts")
        # ... and the same fault in the reference is what that output matches
        check_rounded(bad, *GR.attn_pool_ref(nodes, sqn, gsum, one, zero_, one, zero_, hw, normalise_over_parts=(0, s_, 0))["att_f"], F32, name="the fault against itself")
    # a real BatchNorm pair in the epilogue
    sc, sh = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = GR.attn_pool_ref(nodes, sqn, gsum, sc, sh, -sc, sh, hw)
    out, _, _ = _attn_pool_fp32(nodes, sqn, gsum, sc, sh, -sc, sh, hw)
    check_rounded(out, *ref["out"], F32, name="attn pool, BatchNorm")


@pytest.mark.parametrize("cfg", [(3, 1, 40), (2, 11, 64), (7, 3, 10)])
def test_clip_mean_reference(cfg):
    T, n, D = cfg
    g = torch.Generator().manual_seed(n)
    x = torch.randn((T * n, D), generator=g) * R.channel_scales(D, 6)
    acc = x.view(T, n, D)[:, 0].clone()
    for i in range(1, n):
        acc = acc + x.view(T, n, D)[:, i]
    got = acc / torch.tensor(float(n))
    exact, mag, n_acc = GR.clip_mean_ref(x, n)
    worst, _ = check_rounded(got, exact, mag, n_acc, F32, name="clip mean")
    assert n_acc == n + 1 and (worst > 0.01 or n == 1)
    if n > 1:
        with pytest.raises(AssertionError):
            check_rounded(acc / torch.tensor(float(n - 1)), exact, mag, n_acc, F32, name="mean divided by n - 1")
        check_rounded(acc / torch.tensor(float(n - 1)), *GR.clip_mean_ref(x, n, denominator=n - 1), F32, name="the fault against itself")


@pytest.mark.parametrize("dtype", LP_TYPES)
def test_pam_pool_reference_on_a_16_bit_map(dtype):
    from torchreid import hip_ops as ops
    Fr, h, w, C, Cq, splits = 2, 6, 4, 16, 4, [4]      # a short energy chain (Cq = 4): the worst-case bound grows with Cq, fp32's error with its root
    g = torch.Generator().manual_seed(6)
    x = (0.5 * torch.randn((Fr, h, w, C), generator=g)).to(dtype).float()
    qk = x[..., :2 * Cq].contiguous()
    ref = GR.pam_pool_ref(x, qk, splits, ops.pam_nodes_backward_reference)
    P = sum(splits)
    xbar, xmean = torch.zeros((Fr, P, C)), torch.zeros((Fr, P, C))
    for part, (r0, r1) in enumerate(ops.pam_slices(splits, h)):
        L = (r1 - r0) * w
        X = x[:, r0:r1].reshape(Fr, L, C)
        A = torch.softmax(X[..., :Cq] @ X[..., Cq:2 * Cq].transpose(1, 2), dim=2)
        abar = A.sum(1) / L
        xbar[:, part] = torch.einsum('fq,fqc->fc', abar, X)
        xmean[:, part] = X.sum(1) / L
    e, m, n, s = ref["xbar"]
    worst, _ = check_rounded(xbar, e, m, n, F32, slack=s, name="pam xbar")
    assert worst > 0.01
    check_rounded(xmean, *ref["xmean"], F32, name="pam xmean")
    assert float(ref["xbar"][2][0, 0, 0]) == 4 and h // 4 == 1          # h = 6, n = 4: one row per slice, two rows dropped
    bad = xbar.clone()
    bad[1, 2] = torch.einsum('fqc->fc', x[1:2, 2:3].reshape(1, w, C)) / w      # the plain mean where the attention-weighted one belongs
    with pytest.raises(AssertionError, match=r"at \(1, 2, "):
        check_rounded(bad, e, m, n, F32, slack=s, name="pam xbar, attention dropped")
