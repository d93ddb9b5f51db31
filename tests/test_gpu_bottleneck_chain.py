"""Layer 3's chained per-frame kernel (csrc/bottleneck_chain.hip) against the launches it replaces: conv3x3_packed followed by
bottleneck_seam, once per Bottleneck. The chain composes those two kernels' bodies in their own order of operations, so every
comparison here is torch.equal -- no tolerance. Runs in whichever 16-bit library is loaded."""
import os

import pytest
import torch

from bounds import poisoned_outputs
from lp16 import LP_DTYPE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = (256, 1024, 256)
_CACHE = {}


def operands():
    """Weights and biases of four 256 / 1024 / 256 Bottlenecks plus the conv1 behind the last, as pack_stage-style dicts; once."""
    if "blocks" not in _CACHE:
        from torchreid import hip_ops as ops
        g = torch.Generator().manual_seed(4256)
        def rnd(*shape, scale=1.0):
            return torch.randn(shape, generator=g) * scale
        w1 = [rnd(256, 1, 1, 1024, scale=1024 ** -0.5).to(LP_DTYPE).to(DEV) for _ in range(5)]   # conv1 of blocks 1 .. 5 (OHWI)
        b1 = [rnd(256).to(DEV) for _ in range(5)]
        blocks = []
        for i in range(4):
            w2 = rnd(256, 3, 3, 256, scale=(9 * 256) ** -0.5).to(LP_DTYPE).to(DEV)
            w3 = rnd(1024, 1, 1, 256, scale=256 ** -0.5).to(LP_DTYPE).to(DEV)
            blk = {"c1": (w1[i], b1[i]), "c2": (w2, rnd(256).to(DEV)), "c3": (w3, rnd(1024).to(DEV)), "stride": 1, "ds": None,
                   "c2p": ops.conv3x3_pack(w2), "seam": ops.bottleneck_seam_pack(w3, w1[i + 1]), "seam_dims": DIMS, "seam_b1n": b1[i + 1]}
            assert ops.bottleneck_chain_block_ok(blk)
            blocks.append(blk)
        _CACHE["blocks"] = blocks
        _CACHE["table"] = ops.bottleneck_chain_table(blocks)
    return _CACHE["blocks"], _CACHE["table"]


def inputs(frames, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((frames, 16, 8, 256), generator=g).relu().to(LP_DTYPE).to(DEV)
    a = torch.randn((frames, 16, 8, 1024), generator=g).relu().to(LP_DTYPE).to(DEV)
    return z, a


def launches(z, a, n):
    """today's route: one 3x3 launch and one seam launch per block"""
    from torchreid import hip_ops as ops
    blocks, _ = operands()
    for blk in blocks[:n]:
        y = ops.conv3x3_packed(z, blk["c2p"], blk["c2"][1], 256, True)
        a, z = ops.bottleneck_seam(y, blk["seam"], blk["c3"][1], a, blk["seam_b1n"], DIMS)
    return a, z


@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("frames", [1, 3, 9])
def test_chain_is_bit_identical_to_the_launches(frames, n):
    """1 frame = a single workgroup, 3 = a multiple of nothing, 9 = more workgroups than one XCD's share of the tile map; 1, 2 and 4
    chained blocks. Output and workspace buffers start as NaN; two runs must agree bit for bit."""
    from torchreid import hip_ops as ops
    blocks, table = operands()
    z, a = inputs(frames, 100 * frames + n)
    assert ops.bottleneck_chain_supported(z, a, blocks[:n], forced=True)
    with poisoned_outputs():
        a1, z1 = ops.bottleneck_chain(z, a, table, n)
    with poisoned_outputs():
        a2, z2 = ops.bottleneck_chain(z, a, table, n)
    ar, zr = launches(z, a, n)
    torch.cuda.synchronize()
    assert not torch.isnan(a1.float()).any() and not torch.isnan(z1.float()).any()
    assert torch.equal(a1, a2) and torch.equal(z1, z2)
    assert torch.equal(a1, ar), "a_n differs: max %g" % (a1.float() - ar.float()).abs().max().item()
    assert torch.equal(z1, zr), "z_{n+1} differs: max %g" % (z1.float() - zr.float()).abs().max().item()


@pytest.mark.parametrize("border", [True, False])
def test_halo_of_the_patch_handed_over_in_lds(border):
    """z_1 large on the frame's border pixels and zero inside, and the converse: block 2's 3x3 reads a patch that GEMM 2 wrote in LDS, and
    its halo rows and columns must be zero again although y2 and X lay there in between."""
    from torchreid import hip_ops as ops
    _, table = operands()
    z, a = inputs(3, 77)
    edge = torch.zeros((16, 8), dtype=torch.bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    keep = (edge if border else ~edge).to(DEV).view(1, 16, 8, 1)
    z = (z * 8).masked_fill(~keep, 0).contiguous()
    a = a.masked_fill(~keep, 0).contiguous()
    with poisoned_outputs():
        a2, z3 = ops.bottleneck_chain(z, a, table, 2)
    ar, zr = launches(z, a, 2)
    torch.cuda.synchronize()
    assert torch.equal(a2, ar) and torch.equal(z3, zr)


def test_residual_stream_buffers_back_to_back():
    """The four residual-stream buffers carved from ONE allocation, back to back, reused by a second run with other inputs in the same
    process: a wave must read back exactly what it stored in the block before, never an older line."""
    from torchreid import hip_ops as ops
    _, table = operands()
    frames = 5
    big = torch.full((4, frames, 16, 8, 1024), float("nan"), dtype=LP_DTYPE, device=DEV)
    for seed in (11, 12):
        z, a = inputs(frames, seed)
        a4, z5 = ops.bottleneck_chain(z, a, table, 4, work=[big[0], big[1], big[2]], out=big[3])
        ar, zr = launches(z, a, 4)
        torch.cuda.synchronize()
        assert a4.data_ptr() == big[3].data_ptr()
        assert torch.equal(a4, ar) and torch.equal(z5, zr), "run with seed %d" % seed
        for i in (1, 2, 3):   # the inner maps are the launches' as well
            assert torch.equal(big[i - 1], launches(z, a, i)[0])


def test_overlapping_buffers_and_other_shapes_are_refused():
    from torchreid import _hip, hip_ops as ops
    blocks, table = operands()
    z, a = inputs(2, 5)
    with pytest.raises(_hip.HipKernelError):
        ops.bottleneck_chain(z, a, table, 2, work=[a])
    assert not ops.bottleneck_chain_supported(torch.zeros((2, 32, 16, 256), dtype=LP_DTYPE, device=DEV),
                                              torch.zeros((2, 32, 16, 1024), dtype=LP_DTYPE, device=DEV), blocks[:2], forced=True)
    assert not ops.bottleneck_chain_supported(torch.zeros((2, 16, 8, 128), dtype=LP_DTYPE, device=DEV),
                                              torch.zeros((2, 16, 8, 512), dtype=LP_DTYPE, device=DEV), blocks[:2], forced=True)
    assert not ops.bottleneck_chain_supported(z.float(), a.float(), blocks[:2], forced=True)
    assert not ops.bottleneck_chain_supported(z, a, blocks[:1] + [dict(blocks[1], seam_dims=(256, 1024, 512))], forced=True)


def _embeddings(kind, H, W, chain):
    """the eval forward of a recipe model in the 16-bit mode with AGRL_L3_CHAIN = chain -> (embeddings, entry points called)"""
    import importlib.util
    from recipe import synthetic_adj, synthetic_clips
    from torchreid import _hip, hip_ops as ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if "rec" not in _CACHE:
        spec = importlib.util.spec_from_file_location("record_host_routes", os.path.join(root, "tools", "record_host_routes.py"))
        _CACHE["rec"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_CACHE["rec"])
    R = _CACHE["rec"]
    m, _ = R.model(kind)
    R.reset(kind)
    m.eval()
    m.hip_precision = ops.LP_NAME
    x, adj = synthetic_clips(2, 2, H=H, W=W, seed=3).to(DEV), synthetic_adj(2, 2, seed=3).to(DEV)
    old = os.environ.get("AGRL_L3_CHAIN")
    os.environ["AGRL_L3_CHAIN"] = chain
    _hip.reload_options()
    try:
        with R.traced() as names:
            out = m(x, adj)
            torch.cuda.synchronize()
    finally:
        if old is None:
            del os.environ["AGRL_L3_CHAIN"]
        else:
            os.environ["AGRL_L3_CHAIN"] = old
        _hip.reload_options()
        m.invalidate_hip_cache()
    return out, list(names)


@pytest.mark.parametrize("kind", ["vmgn", "gsta"])
def test_whole_model_embeddings_do_not_change(kind):
    """B = 2, S = 2 clips of 256 x 128 (16 x 8 maps in layer 3): one chain launch for blocks 1-4, the same embeddings bit for bit.
    64 x 32 frames (4 x 2 maps) are no shape of the kernel: no chain launch either way, the same embeddings."""
    on, calls_on = _embeddings(kind, 256, 128, "1")
    off, calls_off = _embeddings(kind, 256, 128, "0")
    assert calls_on.count("agrl_bottleneck_chain") == 1 and "agrl_bottleneck_chain" not in calls_off
    assert calls_off.count("agrl_bottleneck_seam") - calls_on.count("agrl_bottleneck_seam") == 4
    assert torch.equal(on, off)
    small_on, calls_small = _embeddings(kind, 64, 32, "1")
    small_off, _ = _embeddings(kind, 64, 32, "0")
    assert "agrl_bottleneck_chain" not in calls_small
    assert torch.equal(small_on, small_off)


@pytest.mark.skipif(os.environ.get("AGRL_HIP_LP16", "fp16") == "bf16", reason="this process already runs the bf16 build")
def test_bf16_build_in_a_fresh_process():
    """The 16-bit type is fixed when torchreid is imported: the kernel tests above once more on libagrl_hip_bf16.so, in a fresh child
    interpreter (tests/test_gpu_bf16_build.py's pattern)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AGRL_HIP_LP16="bf16")
    for k in ("AGRL_HIP_LIB", "AGRL_HIP_PRECISION", "AGRL_L3_CHAIN"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "not whole_model",
                          "tests/test_gpu_bottleneck_chain.py"], env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    tail = out.stdout.decode()[-3000:]
    print(tail)
    assert out.returncode == 0 and " passed" in tail and "1 skipped" in tail, tail
