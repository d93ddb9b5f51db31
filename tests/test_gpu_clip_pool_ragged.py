"""agrl_clip_pool_ragged on the GPU: segmented clip pooling of a ragged dense batch. The contract is BITWISE: every segment equals
agrl_clip_pool (hip_ops.clip_pool) run on that segment alone, in both modes -- every comparison here is torch.equal on the bits; the mean
is also held to the n + 1 roundings of graph_ref.clip_mean_ref. Outputs are allocated NaN-poisoned, every call runs twice and the runs
must agree bitwise. The kernel is fp32 only, so the two 16-bit builds of the library hold the same code: the last test runs this file
under libagrl_hip_bf16.so in a fresh child, as tests/test_gpu_bf16_build.py does for the sibling's tests."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import graph_ref as GR
import train_ref as R
from bounds import check_rounded, poisoned_outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T33 = tuple((1, 2, 7, 8, 9, 17, 3, 10, 16, 1, 25)[i % 11] for i in range(33))    # mixed: below, at and above the 8 loads in flight
SEGMENTS = [(1,), (1, 2, 7, 8, 9, 17), (125, 1, 3), T33]
DIMS = [1, 5, 260, 4096]


def ops_():
    from torchreid import hip_ops
    return hip_ops


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def twice(fn):
    """fn() -> tensor, under poisoned allocations, twice: bitwise equal (NaNs included); the first run's output on the CPU."""
    runs = []
    for _ in range(2):
        with poisoned_outputs():
            o = fn()
        torch.cuda.synchronize()
        runs.append(o.detach().cpu())
    assert bits_equal(runs[0], runs[1]), "two runs differ"
    return runs[0]


def offsets_of(lens, first=0):
    return np.concatenate([[first], first + np.cumsum(lens)]).astype(np.int64)


def flag_():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def per_segment(xd, off, mode):
    """what the contract names: agrl_clip_pool on every segment alone (T = 1, n = its length)"""
    ops = ops_()
    return torch.cat([ops.clip_pool(xd[lo:hi].contiguous(), hi - lo, mode) for lo, hi in zip(off[:-1].tolist(), off[1:].tolist())], 0).cpu()


@pytest.mark.parametrize("lens", SEGMENTS, ids=lambda s: "T%d_%d" % (len(s), sum(s)))
@pytest.mark.parametrize("D", DIMS)
def test_every_segment_is_bitwise_the_sibling_on_it_alone(D, lens):
    ops = ops_()
    N = sum(lens)
    g = torch.Generator().manual_seed(D + 7 * N)
    x = torch.randn((N, D), generator=g) * R.channel_scales(D, len(lens))
    xd, off = x.to(DEV), offsets_of(lens)
    for mode in ("avg", "max"):
        flag = flag_()
        got = twice(lambda: ops.clip_pool_ragged(xd, off, mode, nonfinite=flag))
        assert got.shape == (len(lens), D) and bool(torch.isfinite(got).all())
        assert bits_equal(got, per_segment(xd, off, mode)), mode
        assert bits_equal(got, twice(lambda: ops.clip_pool_ragged(xd, off, mode))), "the flag pointer changes the result"
        assert int(flag.item()) == 0
        for t, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
            if mode == "avg":
                check_rounded(got[t:t + 1], *GR.clip_mean_ref(x[lo:hi], int(hi - lo)), F32, name="clip_pool_ragged|mean|D%d n%d" % (D, hi - lo))
            else:
                assert torch.equal(got[t], x[lo:hi].max(0).values)


@pytest.mark.parametrize("D", [5, 260])
def test_rows_outside_the_offsets_are_not_read_and_rows_behind_out_not_written(D):
    """offsets[0] > 0 and offsets[T] < N with the outside rows NaN: same output, flag 0. ``out`` is NaN-poisoned before the call and is
    the front of a larger allocation whose rows behind it hold a sentinel: intact afterwards (the entry point is called directly)."""
    from torchreid import _hip
    ops = ops_()
    lens, first, behind = (2, 9, 1, 4), 3, 5
    n_in = sum(lens)
    N = first + n_in + behind
    g = torch.Generator().manual_seed(D)
    x = torch.randn((N, D), generator=g)
    inside = x[first:first + n_in].clone()
    x[:first] = float("nan")
    x[first + n_in:] = float("nan")
    xd, off = x.to(DEV), offsets_of(lens, first)
    T = len(lens)
    for code, mode in ((0, "avg"), (1, "max")):
        flag = flag_()
        got = twice(lambda: ops.clip_pool_ragged(xd, off, mode, nonfinite=flag))
        assert int(flag.item()) == 0, "a row outside [offsets[0], offsets[T]) was read"
        assert bits_equal(got, twice(lambda: ops.clip_pool_ragged(inside.to(DEV), offsets_of(lens), mode)))
        assert bits_equal(got, per_segment(xd, off, mode))
        block = torch.full((T + 3, D), float("nan"), device=DEV)
        block[T:] = -77.0
        off_d = torch.from_numpy(off.astype(np.int32)).to(DEV)
        _hip.call("agrl_clip_pool_ragged", xd.data_ptr(), off_d.data_ptr(), block.data_ptr(), flag.data_ptr(), N, T, D, code,
                  _hip.stream_ptr(xd.device))
        torch.cuda.synchronize()
        assert bits_equal(block[:T].cpu(), got) and bool((block[T:] == -77.0).all()) and int(flag.item()) == 0


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")], ids=["inf", "-inf", "nan"])
def test_non_finite_values_set_the_flag_and_nan_propagates(bad):
    ops = ops_()
    lens, D = (3, 1, 10, 2), 260
    off = offsets_of(lens)
    g = torch.Generator().manual_seed(17)
    x = torch.randn((sum(lens), D), generator=g)
    clean = {mode: twice(lambda: ops.clip_pool_ragged(x.to(DEV), off, mode)) for mode in ("avg", "max")}
    xb = x.clone()
    xb[off[2] + 9, D // 2] = bad                      # the last clip of segment 2 (behind the first eight loads), one channel
    want = torch.zeros((len(lens), D), dtype=torch.bool)
    want[2, D // 2] = True
    for mode in ("avg", "max"):
        flag = flag_()
        got = twice(lambda: ops.clip_pool_ragged(xb.to(DEV), off, mode, nonfinite=flag))
        assert int(flag.item()) == 1, mode
        assert bits_equal(got[~want], clean[mode][~want]) and bits_equal(got, per_segment(xb.to(DEV), off, mode))
        if bad != bad:
            assert torch.equal(torch.isnan(got), want), "a NaN clip stays a NaN in both modes"
        ops.clip_pool_ragged(x.to(DEV), off, mode, nonfinite=flag)      # the kernel never stores 0: a later clean call leaves the flag
        assert int(flag.item()) == 1


def test_the_sign_of_a_zero_maximum_is_kept():
    """the first of equal maxima stands: -0 before +0 stays -0 (torch.max on the same device agrees with the sibling's rule)"""
    ops = ops_()
    lens, D = (2, 3, 9, 1), 5
    off = offsets_of(lens)
    z = torch.zeros((sum(lens), D))
    z[0::2] = -0.0
    z[off[1]:off[2]] = -z[off[1]:off[2]]
    zd = z.to(DEV)
    got = twice(lambda: ops.clip_pool_ragged(zd, off, "max"))
    assert bits_equal(got, per_segment(zd, off, "max"))
    assert bits_equal(got, torch.stack([zd[lo:hi].max(0).values for lo, hi in zip(off[:-1], off[1:])]).cpu())
    assert bool(torch.signbit(got[0]).all()) and not bool(torch.signbit(got[1]).any())


def test_rejections():
    from torchreid import _hip
    ops = ops_()
    x = torch.randn((10, 8), device=DEV)
    for off in ([0, 3, 3, 10], [0, 5, 4, 10], [0, 4, 11], [-1, 4], [4], [[0, 4]], np.array([0.0, 4.0])):
        with pytest.raises(ValueError, match="offsets"):
            ops.clip_pool_ragged(x, np.asarray(off), "avg")
    with pytest.raises(ValueError, match="host array"):
        ops.clip_pool_ragged(x, torch.tensor([0, 4, 10], dtype=torch.int32, device=DEV), "avg")
    with pytest.raises(ValueError, match="mode"):
        ops.clip_pool_ragged(x, np.array([0, 4, 10]), "sum")
    with pytest.raises(ValueError):
        ops.clip_pool_ragged(x.cpu(), np.array([0, 4, 10]), "avg")
    with pytest.raises(ValueError, match="nonfinite"):
        ops.clip_pool_ragged(x, np.array([0, 4, 10]), "avg", nonfinite=torch.zeros(1, dtype=torch.int64, device=DEV))
    assert ops.clip_pool_ragged(x, torch.tensor([0, 4, 10]), "avg").shape == (2, 8)      # a host tensor is a host array
    off_d = torch.tensor([0, 4, 10], dtype=torch.int32, device=DEV)
    out = torch.full((2, 8), 5.0, device=DEV)
    s = _hip.stream_ptr(x.device)
    good = (x.data_ptr(), off_d.data_ptr(), out.data_ptr(), None, 10, 2, 8, 0, s)
    for k in (0, 1, 2):
        with pytest.raises(_hip.HipKernelError, match="null pointer"):
            _hip.call("agrl_clip_pool_ragged", *(good[:k] + (None,) + good[k + 1:]))
    for k in (4, 5, 6):
        for v in (0, -1):
            with pytest.raises(_hip.HipKernelError, match="bad shape"):
                _hip.call("agrl_clip_pool_ragged", *(good[:k] + (v,) + good[k + 1:]))
    for v in (2, -1):
        with pytest.raises(_hip.HipKernelError, match="mode must be"):
            _hip.call("agrl_clip_pool_ragged", *(good[:7] + (v,) + good[8:]))
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())                  # nothing was launched
    _hip.call("agrl_clip_pool_ragged", *good)        # ... and the same arguments unchanged are accepted
    torch.cuda.synchronize()
    assert bits_equal(out.cpu(), ops.clip_pool_ragged(x, np.array([0, 4, 10]), "avg").cpu())


@pytest.mark.skipif(os.environ.get("AGRL_HIP_LP16", "fp16") == "bf16", reason="this process already runs the bf16 build")
def test_bf16_build_of_the_library_passes_this_file_in_a_fresh_process():
    lib = os.path.join(ROOT, "agrl.pytorch_amd", "lib", "libagrl_hip_bf16.so")
    assert os.path.exists(lib), "libagrl_hip_bf16.so is not built (make -C agrl.pytorch_amd/csrc)"
    env = dict(os.environ, AGRL_HIP_LP16="bf16")
    env.pop("AGRL_HIP_LIB", None)
    env.pop("AGRL_HIP_PRECISION", None)
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_clip_pool_ragged.py"],
                         env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    tail = out.stdout.decode()[-3000:]
    print(tail)
    assert out.returncode == 0 and " passed" in tail, tail
