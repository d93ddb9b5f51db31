"""CPU checks of tests/bounds.py: half_ulp against torch's own fp16 / bf16 rounding, and check_rounded accepting correctly
rounded results while rejecting the subtly wrong ones (round toward zero, double rounding, one channel off by 2^-9) that a
max-normalised error bar lets through."""
import pytest
import torch

from bounds import INT_SENTINEL, check_rounded, half_ulp, n_acc_for, poisoned_outputs

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
