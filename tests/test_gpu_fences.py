"""Three properties of every kernel entry point that no arithmetic bound sees, one registry of kernel families, exact checks:

1. stores stay inside the outputs: the call runs under ``poisoned_outputs()``, whose allocations stand between canary bands;
2. results do not depend on bytes outside the operands: every operand is a ``fenced()`` copy between bands of 0x00, 0xFF (NaN /
   -1) and 0x7C (NaN in fp16, ~5e36 in bf16 and fp32) -- a load past a ragged edge that is masked by a multiplication with zero, or
   only in the epilogue, changes the bits;
3. the entry point honours the stream it is given: the call on a side stream, behind a producer that takes a few milliseconds and
   the copies that fill NaN / -1 operand buffers, gives the bits of the default-stream run.

A registry entry builds its seeded operands on the CPU (``make``) and makes one host-path call on device copies of them (``run``).
Where the call needs buffers that another launch or a packer makes (packed weight streams, planes, normalised rows, Gram partials,
statistics), ``run`` makes them too and hands each on through ``mid``: in check 2 every such intermediate stands between bands of
the fill like the seeded operands, so each launch of a chain has varied bytes around everything it reads. What one hip_ops call
allocates and reads back inside itself (the Gram partials of graph_matrix, the tile sums of conv_stats, split-K scratch) cannot be
wrapped from outside; those buffers are fenced as outputs in check 1. ENTRY_POINTS declares which
entry points each family reaches: tests/test_bounds.py holds it against torchreid._hip.SIGNATURES (a new entry point without a
fence case fails there, without a GPU) and check 1 holds it against the calls the family really makes. Shapes: the smallest
ragged cases of the families' own tests. Comparisons: torch.equal on integer views, nothing looser."""
import contextlib
import os
import time

import numpy as np
import pytest
import torch

import bounds
from bounds import INT_SENTINEL, fenced, poisoned_outputs
from lp16 import LP16, LP_DTYPE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
FP16_BUILD = LP16 == "fp16"
FILLS = (0x00, 0xFF, 0x7C)


class Family(object):
    def __init__(self, name, entry_points, make, run, env=None, fp16_only=False, fence_outputs=True, poison_ok=()):
        self.name, self.entry_points, self.make, self.run = name, tuple(entry_points), make, run
        self.env = dict(env or {})                # AGRL_* switches that force a tile form, applied as the family's own test does
        self.fp16_only = fp16_only                # the split-fp16 plane kernels exist in the fp16 build only
        self.fence_outputs = fence_outputs        # False: in-place / byte kernels whose own tests already band their outputs
        self.poison_ok = tuple(poison_ok)         # indices of outputs that may legitimately hold the poison value (documented)


FAMILIES = {}


def family(name, entry_points, make, **kw):
    def register(run):
        assert name not in FAMILIES, name
        FAMILIES[name] = Family(name, entry_points, make, run, **kw)
        return run
    return register


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rn(g, *shape, s=1.0, dt=F32):
    return (torch.randn(shape, generator=g) * s).to(dt)


def ru(g, *shape, s=1.0, dt=F32):
    return (torch.rand(shape, generator=g) * s).to(dt)


def ops_():
    from torchreid import hip_ops
    return hip_ops


def dt_name(dt):
    return "fp32" if dt == F32 else "lp16"


_RIDERS = ("agrl_unscale", "agrl_presplit", "agrl_scaled", "agrl_folded_unscale")     # what the packers let ride on a weight tensor


def mid(o, *ts):
    """An intermediate of ``run``: a buffer that one launch (or a torch packer) wrote and a later launch reads -- packed weight
    streams, planes, normalised rows, Gram partials, statistics. Checks 1 and 3 pass it on as it is; check 2 sets o["mid"] and
    every intermediate becomes a fenced() copy between bands of the fill, like the seeded operands."""
    wrap, out = o.get("mid"), []
    for t in ts:
        if wrap is not None and t is not None:
            w = wrap(t)
            for a in _RIDERS:
                if hasattr(t, a):
                    setattr(w, a, getattr(t, a))
            t = w
        out.append(t)
    return out[0] if len(out) == 1 else tuple(out)


# ---- convs on the implicit-GEMM kernels ----------------------------------------------------------------------------------------------
def conv_operands(case, dt, res):
    N, H, W, Cin, Cout, R, stride = case
    g = gen(sum(case))
    pad = R // 2
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    o = {"x": rn(g, N, H, W, Cin, dt=dt), "w": rn(g, Cout, R, R, Cin, s=(R * R * Cin) ** -0.5, dt=dt), "b": rn(g, Cout)}
    if res:
        o["res"] = rn(g, N, OH, OW, Cout, dt=dt)
    return o


for _case, _res in (((3, 10, 7, 64, 64, 1, 1), False), ((1, 9, 5, 512, 200, 3, 1), True), ((2, 16, 8, 128, 128, 3, 2), False)):
    for _dt in (F32, LP_DTYPE):
        @family("conv_bn_act-%s-%s" % ("x".join(str(v) for v in _case), dt_name(_dt)), ["agrl_conv2d_bn_act"],
                lambda c=_case, d=_dt, r=_res: conv_operands(c, d, r))
        def _run(o, c=_case):
            return (ops_().conv_bn_act(o["x"], o["w"], o["b"], c[6], c[5] // 2, True, residual=o.get("res")),)

for _tile in ("2", "3"):
    @family("conv_bn_act-wide-tile%s-3x10x7x256x256" % _tile, ["agrl_conv2d_bn_act"],
            lambda: conv_operands((3, 10, 7, 256, 256, 1, 1), LP_DTYPE, False), env={"AGRL_IGEMM_WIDE": _tile})
    def _run(o):
        return (ops_().conv_bn_act(o["x"], o["w"], o["b"], 1, 0, True),)


# ---- 1x1 / 3x3 convs on packed weight streams ----------------------------------------------------------------------------------------
def packed1x1_operands(N, H, W, K1, K2, Cout, res=False, Ho=None, Wo=None, positive=False):
    g = gen(N + H + W + K1 + K2 + Cout)
    Ho, Wo = H if Ho is None else Ho, W if Wo is None else Wo
    x = rn(g, N, H, W, K1)
    o = {"x": (x.relu() if positive else x).to(LP_DTYPE), "w": rn(g, Cout, K1 + K2, s=(K1 + K2) ** -0.5, dt=LP_DTYPE), "b": rn(g, Cout)}
    if K2:
        o["x2"] = rn(g, N, Ho, Wo, K2).relu().to(LP_DTYPE)
    if res:
        o["res"] = rn(g, N, Ho, Wo, Cout, dt=LP_DTYPE)
    return o


@family("conv1x1_packed-3x10x6x256x0x512", ["agrl_conv1x1_pack", "agrl_conv1x1_packed_bn_act"], lambda: packed1x1_operands(3, 10, 6, 256, 0, 512))
def _run(o):
    ops = ops_()
    packed = mid(o, ops.conv1x1_pack(o["w"]))
    return packed, ops.conv1x1_packed(o["x"], packed, o["b"], 512, False)


for _duo in (False, True):
    @family("conv1x1_packed-two-source-2x16x8x256x128x256-%s" % ("duo" if _duo else "fat"),
            ["agrl_conv1x1_pack", "agrl_conv1x1_packed_dual_duo" if _duo else "agrl_conv1x1_packed_bn_act"],
            lambda: packed1x1_operands(2, 16, 8, 256, 128, 256))
    def _run(o, duo=_duo):
        ops = ops_()
        return (ops.conv1x1_packed(o["x"], mid(o, ops.conv1x1_pack(o["w"])), o["b"], 256, True, x2=o["x2"], duo=duo),)


@family("conv1x1_packed_res-3x10x6x128x256", ["agrl_conv1x1_pack", "agrl_conv1x1_packed_res_bn_act"],
        lambda: packed1x1_operands(3, 10, 6, 128, 0, 256, res=True, positive=True))
def _run(o):
    ops = ops_()
    return (ops.conv1x1_packed_res(o["x"], mid(o, ops.conv1x1_pack(o["w"])), o["b"], 256, o["res"], False),)


@family("conv1x1_packed_dual_strided-3x7x5x128x128x256s2", ["agrl_conv1x1_pack", "agrl_conv1x1_packed_dual_strided"],
        lambda: packed1x1_operands(3, 7, 5, 128, 128, 256, Ho=4, Wo=3, positive=True))
def _run(o):
    ops = ops_()
    return (ops.conv1x1_packed_dual_strided(o["x"], o["x2"], mid(o, ops.conv1x1_pack(o["w"])), o["b"], 256, 2, True),)


@family("conv1x1_dual-3x16x8x1024x512x2048", ["agrl_conv1x1_dual_bn_act"], lambda: packed1x1_operands(3, 16, 8, 1024, 512, 2048))
def _run(o):
    ops = ops_()
    assert ops.conv1x1_dual_supported(o["x"], o["x2"], o["w"])
    return (ops.conv1x1_dual(o["x"], o["x2"], o["w"], o["b"], True),)


@family("conv1x1_packed_res_pool-3x128x256-421", ["agrl_conv1x1_pack", "agrl_conv1x1_packed_res_pool"],
        lambda: packed1x1_operands(3, 16, 8, 128, 0, 256, res=True, positive=True))
def _run(o):
    ops = ops_()
    return ops.conv1x1_packed_res_pool(o["x"], mid(o, ops.conv1x1_pack(o["w"])), o["b"], 256, o["res"], [4, 2, 1], True, True)


@family("conv1x1_bn_act_pool-3x128x256-421", ["agrl_conv1x1_bn_act_pool"], lambda: packed1x1_operands(3, 16, 8, 128, 0, 256, res=True, positive=True))
def _run(o):
    return ops_().conv1x1_bn_act_pool(o["x"], o["w"].view(256, 1, 1, 128), o["b"], o["res"], [4, 2, 1], True, True)


def conv3x3_operands(N, H, W, Cin, Cout):
    g = gen(N + H + W + Cin + Cout)
    return {"x": rn(g, N, H, W, Cin, dt=LP_DTYPE), "w": rn(g, Cout, 3, 3, Cin, s=(9 * Cin) ** -0.5, dt=LP_DTYPE), "b": rn(g, Cout)}


@family("conv3x3_packed-1x16x8x128x256", ["agrl_conv3x3_pack", "agrl_conv3x3_packed_bn_act"], lambda: conv3x3_operands(1, 16, 8, 128, 256))
def _run(o):
    ops = ops_()
    packed = mid(o, ops.conv3x3_pack(o["w"]))
    return packed, ops.conv3x3_packed(o["x"], packed, o["b"], 256, True)


# ---- fused Bottleneck kernels --------------------------------------------------------------------------------------------------------
def tail_operands(N, H, W, cmid, cout, cnext, shortcut=False, block=False):
    g = gen(N * H + cnext + cmid)
    o = {"y2": rn(g, N, H, W, cmid, dt=LP_DTYPE), "w3": rn(g, cout, 1, 1, cmid, s=cmid ** -0.5, dt=LP_DTYPE), "b3": rn(g, cout),
         "w1": rn(g, cnext, 1, 1, cout, s=cout ** -0.5, dt=LP_DTYPE), "b1": rn(g, cnext)}
    if shortcut:
        o.update(x0=rn(g, N, H, W, 64, dt=LP_DTYPE), ws=rn(g, cout, 1, 1, 64, s=0.125, dt=LP_DTYPE), bs=rn(g, cout))
    else:
        o["res"] = rn(g, N, H, W, cout, dt=LP_DTYPE)
    if block:
        o.update(w2=rn(g, 64, 3, 3, 64, s=1 / 24, dt=LP_DTYPE), b2=rn(g, 64))
    return o


def run_tail(o):
    ops = ops_()
    sc = (o["x0"], o["ws"], o["bs"]) if "x0" in o else None
    assert ops.bottleneck_tail_supported(o["y2"], o["w3"], o["w1"], None if sc is None else (o["ws"], 1))
    return ops.bottleneck_tail(o["y2"], o["w3"], o["b3"], o.get("res"), o["w1"], o["b1"], shortcut=sc)


family("bottleneck_tail-3x10x7-cnext64", ["agrl_bottleneck_tail"], lambda: tail_operands(3, 10, 7, 64, 256, 64))(run_tail)
family("bottleneck_tail-3x10x7-cnext64-shortcut", ["agrl_bottleneck_tail"], lambda: tail_operands(3, 10, 7, 64, 256, 64, shortcut=True))(run_tail)
family("bottleneck_tail-layer2-3x10x7", ["agrl_bottleneck_tail"], lambda: tail_operands(3, 10, 7, 128, 512, 128))(run_tail)


def run_block(o):
    ops = ops_()
    sc = (o["x0"], o["ws"], o["bs"]) if "x0" in o else None
    assert ops.bottleneck_block_supported(o["y2"], o["w2"], 1, o["w3"], o["w1"], None if sc is None else (o["ws"], 1))
    return ops.bottleneck_block(o["y2"], o["w2"], o["b2"], o["w3"], o["b3"], o.get("res"), o["w1"], o["b1"], shortcut=sc)


family("bottleneck_block-3x8x24", ["agrl_bottleneck_block"], lambda: tail_operands(3, 8, 24, 64, 256, 64, block=True))(run_block)
family("bottleneck_block-3x8x24-shortcut", ["agrl_bottleneck_block"], lambda: tail_operands(3, 8, 24, 64, 256, 64, shortcut=True, block=True))(run_block)


@family("bottleneck_seam-3-frames-256x1024x256", ["agrl_bottleneck_seam_pack", "agrl_bottleneck_seam"], lambda: tail_operands(3, 16, 8, 256, 1024, 256))
def _run(o):
    ops = ops_()
    assert ops.bottleneck_seam_supported(o["w3"], o["w1"], 3 * 128)
    packed = mid(o, ops.bottleneck_seam_pack(o["w3"], o["w1"]))
    return (packed,) + ops.bottleneck_seam(o["y2"], packed, o["b3"], o["res"], o["b1"], (256, 1024, 256))


def chain_operands(frames, n):
    g = gen(4256 + frames)
    o = {"z": rn(g, frames, 16, 8, 256).relu().to(LP_DTYPE), "a": rn(g, frames, 16, 8, 1024).relu().to(LP_DTYPE)}
    for i in range(n + 1):
        o["w1_%d" % i], o["b1_%d" % i] = rn(g, 256, 1, 1, 1024, s=1024 ** -0.5, dt=LP_DTYPE), rn(g, 256)
    for i in range(n):
        o["w2_%d" % i], o["b2_%d" % i] = rn(g, 256, 3, 3, 256, s=(9 * 256) ** -0.5, dt=LP_DTYPE), rn(g, 256)
        o["w3_%d" % i], o["b3_%d" % i] = rn(g, 1024, 1, 1, 256, s=256 ** -0.5, dt=LP_DTYPE), rn(g, 1024)
    return o


@family("bottleneck_chain-3-frames-n2", ["agrl_conv3x3_pack", "agrl_bottleneck_seam_pack", "agrl_bottleneck_chain"], lambda: chain_operands(3, 2))
def _run(o):
    ops = ops_()
    blocks = []
    for i in range(2):
        blk = {"c1": (o["w1_%d" % i], o["b1_%d" % i]), "c2": (o["w2_%d" % i], o["b2_%d" % i]), "c3": (o["w3_%d" % i], o["b3_%d" % i]),
               "stride": 1, "ds": None, "c2p": mid(o, ops.conv3x3_pack(o["w2_%d" % i])), "seam": mid(o, ops.bottleneck_seam_pack(o["w3_%d" % i], o["w1_%d" % (i + 1)])),
               "seam_dims": (256, 1024, 256), "seam_b1n": o["b1_%d" % (i + 1)]}
        blocks.append(blk)
    assert ops.bottleneck_chain_supported(o["z"], o["a"], blocks, forced=True)
    table = mid(o, ops.bottleneck_chain_table(blocks))
    out = ops.bottleneck_chain(o["z"], o["a"], table, 2)
    o["_keep"] = (blocks, table)      # the table points into the packs: alive until the caller has synchronised
    return out


# ---- stems ---------------------------------------------------------------------------------------------------------------------------
def stem_operands(u8):
    g = gen(5)
    x = torch.randint(0, 256, (1, 37, 29, 3), generator=g, dtype=torch.uint8) if u8 else rn(g, 1, 3, 37, 29)
    return {"x": x, "w": rn(g, 64, 7, 7, 3, s=0.1), "b": rn(g, 64, s=0.1)}


for _u8 in (False, True):
    _sfx = "-u8" if _u8 else ""
    for _dt in (F32, LP_DTYPE):
        @family("stem-1x37x29-%s%s" % (dt_name(_dt), _sfx), ["agrl_stem_conv_bn_relu_maxpool" + ("_u8" if _u8 else "")], lambda u=_u8: stem_operands(u))
        def _run(o, d=_dt):
            return (ops_().stem(o["x"], o["w"], o["b"], d),)

    @family("stem_lp16-1x37x29%s" % _sfx, ["agrl_stem_conv_bn_relu_maxpool_lp16" + ("_u8" if _u8 else "")], lambda u=_u8: stem_operands(u))
    def _run(o):
        ops = ops_()
        return (ops.stem_lp16(o["x"], mid(o, ops.pack_stem_weights_lp16(o["w"])), o["b"]),)

    @family("stem_split16-1x37x29%s" % _sfx, ["agrl_stem_split16" + ("_u8" if _u8 else "")], lambda u=_u8: stem_operands(u))
    def _run(o):
        ops = ops_()
        wh, wl, u = ops.pack_stem_weights_split16(o["w"])
        return (ops.stem_split16(o["x"], mid(o, wh), mid(o, wl), u, o["b"]),)


# ---- split-fp16 convs and distance matrix ----------------------------------------------------------------------------------------------
def wide_range(g, *shape):
    """non-negative activations with rows of very different scale, as the split-fp16 tests use"""
    return rn(g, *shape).clamp(min=0) * torch.exp(1.5 * rn(g, *(shape[:-1] + (1,))))


@family("conv_bn_act-split16-inloop-3x10x7x64x64", ["agrl_conv2d_bn_act_split16"], lambda: conv_operands((3, 10, 7, 64, 64, 1, 1), F32, False))
def _run(o):
    ops = ops_()
    return (ops.conv_bn_act(o["x"], mid(o, ops.split16_inloop_weights(o["w"])), o["b"], 1, 0, True),)


@family("split16_weights_inloop-24x3x3x96", ["agrl_split16_weights_inloop"], lambda: {"w": rn(gen(5), 24, 3, 3, 96)})
def _run(o):
    from torchreid import _hip
    ops = ops_()
    ws = mid(o, ops.split16_prescale(o["w"]))
    got = torch.empty_like(ws)
    with torch.cuda.device(ws.device):
        _hip.call("agrl_split16_weights_inloop", ws.data_ptr(), got.data_ptr(), ws.numel() // 96, 96, _hip.stream_ptr(ws.device))
    return (got,)


def dual_split_operands():
    g = gen(7 + 64 + 96 + 128)
    return {"x": wide_range(g, 1, 9, 7, 64), "x2": wide_range(g, 1, 5, 4, 96), "w": rn(g, 128, 160, s=160 ** -0.5), "b": rn(g, 128, s=0.1)}


for _planes in (0, 3):
    @family("conv1x1_dual_split16-1x9x7x64x96x128s2-planes%d" % _planes, ["agrl_conv1x1_dual_split16"], dual_split_operands, fp16_only=_planes != 0)
    def _run(o, p=_planes):
        ops = ops_()
        return (ops.conv1x1_dual_split16(o["x"], o["x2"], mid(o, ops.split16_inloop_weights(o["w"])), o["b"], 2, True, out_planes=p),)


def plane_operands(M, Ks, Cout, res=False):
    g = gen(M + Cout + sum(Ks))
    o = {"w": rn(g, Cout, sum(Ks), s=0.7 * sum(Ks) ** -0.5), "b": rn(g, Cout, s=0.1)}
    for i, k in enumerate(Ks):
        o["x%d" % i] = wide_range(g, M, k)
    if res:
        o["res"] = rn(g, M, Cout)
    return o


@family("conv1x1_split16-40x128x256", ["agrl_split16_planes", "agrl_conv1x1_pack", "agrl_conv1x1_split16"], lambda: plane_operands(40, [128], 256, res=True),
        fp16_only=True)
def _run(o):
    ops = ops_()
    x3, r3 = mid(o, ops.to_split16_planes(o["x0"]), ops.to_split16_planes(o["res"]))
    w3, unscale = ops.split16_plane_weights(o["w"])
    return x3, ops.conv1x1_split16(x3.view(1, 40, 1, -1), mid(o, ops.conv1x1_pack(mid(o, w3))), unscale, o["b"], 256, residual3=r3.view(1, 40, 1, -1))


@family("conv1x1_split16_dual-40x128+128x256", ["agrl_split16_planes", "agrl_conv1x1_pack", "agrl_conv1x1_split16_dual"],
        lambda: plane_operands(40, [128, 128], 256), fp16_only=True)
def _run(o):
    ops = ops_()
    x3, y3 = mid(o, ops.to_split16_planes(o["x0"]), ops.to_split16_planes(o["x1"]))
    w3, unscale = ops.split16_plane_weights(o["w"], segments=[128, 128])
    return (ops.conv1x1_split16(x3.view(1, 40, 1, -1), mid(o, ops.conv1x1_pack(mid(o, w3))), unscale, o["b"], 256, x2=y3.view(1, 40, 1, -1)),)


@family("conv1x1_split16_pool-1x256x256", ["agrl_split16_planes", "agrl_conv1x1_pack", "agrl_conv1x1_split16_pool"],
        lambda: plane_operands(128, [256], 256, res=True), fp16_only=True)
def _run(o):
    ops = ops_()
    x3, r3 = mid(o, ops.to_split16_planes(o["x0"]), ops.to_split16_planes(o["res"]))
    w3, unscale = ops.split16_plane_weights(o["w"])
    return (ops.conv1x1_split16_pool(x3.view(1, 16, 8, -1), mid(o, ops.conv1x1_pack(mid(o, w3))), unscale, o["b"], 256, r3.view(1, 16, 8, -1), [1], False),)


def conv3_split_operands():
    g = gen(1 + 16 + 8 + 128 + 256)
    return {"x": wide_range(g, 1, 16, 8, 128), "w": rn(g, 256, 3, 3, 128, s=0.7 * (9 * 128) ** -0.5), "b": rn(g, 256, s=0.1)}


@family("conv3x3_split16-1x16x8x128x256", ["agrl_split16_planes", "agrl_conv3x3_pack", "agrl_conv3x3_packed_split16"], conv3_split_operands, fp16_only=True)
def _run(o):
    ops = ops_()
    w3, unscale = ops.split16_plane_weights(o["w"])
    return (ops.conv3x3_split16(mid(o, ops.to_split16_planes(o["x"])), mid(o, ops.conv3x3_pack(mid(o, w3))), unscale, o["b"], 256),)


def distmat_operands(m, n, D):
    g = gen(m + n)
    centers = rn(g, 16, D)
    return {"q": centers[torch.randint(0, 16, (m,), generator=g)] + 0.5 * rn(g, m, D),
            "g": centers[torch.randint(0, 16, (n,), generator=g)] + 0.5 * rn(g, n, D)}


def distance_operands(o, metric, prec):
    """The launches of metrics.distance.hip_distmat_device in its order, made one by one so that every buffer the distance kernel
    reads is an intermediate of ``run`` (mid): -> (q operand, g operand, q norms, g norms, 2^-k of the gallery planes or None)."""
    import math
    ops = ops_()
    q, g = o["q"], o["g"]
    if prec == "fp16x3":
        assert ops.split16_planes_available() and q.size(1) % 64 == 0
        if metric == "euclidean":
            qn, gn = mid(o, ops.row_sqnorm(q), ops.row_sqnorm(g))
            k = 13 - math.frexp(float(g.abs().max()))[1] + 1
        else:
            qn = gn = None
            q, g = mid(o, ops.row_l2_normalize(q, True, F32), ops.row_l2_normalize(g, True, F32))
            k = 13
        return mid(o, ops.to_split16_planes(q)), mid(o, ops.to_split16_weight_planes(g, 2.0 ** k)), qn, gn, 2.0 ** -k
    dt = LP_DTYPE if ops.is_lp16(prec) else F32
    km = ops.k_multiple(dt)
    if metric == "euclidean":
        qn, gn = mid(o, ops.row_sqnorm(q), ops.row_sqnorm(g))
        if dt != F32 or q.size(1) % km:
            q, g = mid(o, ops.row_l2_normalize(q, False, dt, km), ops.row_l2_normalize(g, False, dt, km))
        return q, g, qn, gn, None
    q, g = mid(o, ops.row_l2_normalize(q, True, dt, km), ops.row_l2_normalize(g, True, dt, km))
    return q, g, None, None, None


def same_as_host_path(o, got, want):
    """the chain above is the host path's: checked where nothing is wrapped (checks 1 and 3)"""
    if o.get("mid") is None:
        assert all(torch.equal(a, b) for a, b in zip(got, want)), "the chained launches differ from the host path's result"
    return got


for _metric in ("euclidean", "cosine"):
    @family("distmat_split16-37x101x128-%s" % _metric,
            ["agrl_split16_planes", "agrl_split16_weight_planes", "agrl_distmat_split16", "agrl_row_sqnorm" if _metric == "euclidean" else "agrl_row_l2_normalize"],
            lambda: distmat_operands(37, 101, 128), fp16_only=True)
    def _run(o, metric=_metric):
        from torchreid.metrics.distance import hip_distmat_device
        q3, g3, qn, gn, unscale = distance_operands(o, metric, "fp16x3")
        got = (ops_().distmat_split16(q3, g3, metric, unscale, qn, gn),)
        return same_as_host_path(o, got, (hip_distmat_device(o["q"], o["g"], metric, "fp16x3"),))


# ---- pooling, attention tail -----------------------------------------------------------------------------------------------------------
for _dt in (F32, LP_DTYPE):
    @family("part_pool-1x3x14x7x512-421-%s" % dt_name(_dt), ["agrl_part_pool"],
            lambda d=_dt: {"x1": ru(gen(11), 3, 14, 7, 512, dt=d), "x2": ru(gen(12), 3, 14, 7, 512, dt=d)})
    def _run(o):
        return ops_().part_pool(o["x1"], o["x2"], [4, 2, 1], True)

    @family("pam_pool-2x6x4x64x32-4-%s" % dt_name(_dt), ["agrl_pam_pool"],
            lambda d=_dt: {"x": rn(gen(72), 2, 6, 4, 64, dt=d), "qk": rn(gen(73), 2, 6, 4, 64, s=0.3, dt=d)})
    def _run(o):
        return ops_().pam_pool(o["x"], o["qk"], [4])


@family("pam_pool-2x6x4x64-4-no-attention", ["agrl_pam_pool"], lambda: {"x": rn(gen(72), 2, 6, 4, 64)})
def _run(o):
    return (ops_().pam_pool(o["x"], None, [4])[1],)


@family("pam_combine-2x4x64", ["agrl_pam_combine"], lambda: {"y": rn(gen(1), 2, 4, 64), "bv": rn(gen(2), 64, s=0.1), "xmean": rn(gen(3), 2, 4, 64)})
def _run(o):
    return ops_().pam_combine(o["y"], o["bv"], o["xmean"], 0.7, True)


for _mode in ("avg", "max"):
    @family("clip_pool-7x3x1000-%s" % _mode, ["agrl_clip_pool"], lambda: {"f": rn(gen(5), 21, 1000)})
    def _run(o, mode=_mode):
        return (ops_().clip_pool(o["f"], 3, mode),)

for _D, _mode in ((5, "avg"), (260, "max")):
    @family("clip_pool_ragged-T6_44-D%d-%s" % (_D, _mode), ["agrl_clip_pool_ragged"],
            lambda D=_D: {"f": rn(gen(D), 47, D), "flag": torch.zeros(1, dtype=torch.int32), "offsets": np.cumsum([2, 1, 2, 7, 8, 9, 17]).astype(np.int64)})
    def _run(o, mode=_mode):
        return ops_().clip_pool_ragged(o["f"], o["offsets"], mode, nonfinite=o["flag"]), o["flag"]


def attn_operands(B, S, P, C, hw):
    g = gen(B * 7 + S)
    nodes = ru(g, B, S, P, C)
    if S > 2:
        nodes[B // 2, 2] = 0      # a frame whose nodes are all zero
    return {"nodes": nodes, "gsum": ru(g, B * S, C, s=hw), "gs": 0.8 + 0.4 * ru(g, C), "gsh": rn(g, C, s=0.1), "as": 0.8 + 0.4 * ru(g, C),
            "ash": rn(g, C, s=0.1)}


@family("attn_pool_bnneck-1x1x7x256x128", ["agrl_row_sqnorm", "agrl_attn_pool_bnneck"], lambda: attn_operands(1, 1, 7, 256, 128))
def _run(o):
    ops = ops_()
    sqn = mid(o, ops.row_sqnorm(o["nodes"].view(7, 256)))
    return (sqn,) + ops.attn_pool_bnneck(o["nodes"], sqn, o["gsum"], o["gs"], o["gsh"], o["as"], o["ash"], 1, 1, 7, 128, want_feats=True)


for _q in (F32, LP_DTYPE):
    @family("attn_tail-5x4x3x512x60-query-%s" % dt_name(_q), ["agrl_attn_tail"], lambda: attn_operands(5, 4, 3, 512, 60))
    def _run(o, q=_q):
        ops = ops_()
        assert ops.attn_tail_supported(4, 3, 512)
        out, feats, query, node_sqn = ops.attn_tail(o["nodes"], o["gsum"], o["gs"], o["gsh"], o["as"], o["ash"], 5, 4, 3, 60, want_feats=True,
                                                    query_dtype=q, want_node_sqn=True)
        return out, feats[0], feats[1], query["sqn"], query["normalized"], node_sqn


# ---- graph layer -----------------------------------------------------------------------------------------------------------------------
def graph_operands(B, V, C, packed=False):
    g = gen(B * 1000 + V + C)
    f = ru(g, B, 1, C) + 0.02 * rn(g, B, V, C)
    adj = (ru(g, B, V, V) > 0.5).float()
    adj[0, 3] = 0      # an all-zero row
    o = {"f": f, "adj": ops_().adjacency_pack_host(adj) if packed else adj, "w": rn(g, C, C, s=0.02), "scale": 0.8 + 0.4 * ru(g, C),
         "shift": rn(g, C, s=0.1)}
    Gm = ru(g, B, V, V) * adj
    o["G"] = Gm / Gm.sum(2, keepdim=True).clamp(min=1e-6)
    return o


for _mode in ((True, True), (True, False), (False, True)):
    @family("graph_matrix-V20-pose%d-learn%d" % _mode, (["agrl_graph_gram"] if _mode[1] else []) + ["agrl_graph_finalize"], lambda: graph_operands(3, 20, 2048))
    def _run(o, mode=_mode):
        return (ops_().graph_matrix(o["f"], o["adj"], mode[0], mode[1]),)

for _mode in ((True, True), (True, False)):
    @family("graph_matrix-V20-packed-adjacency-learn%d" % _mode[1], (["agrl_graph_gram"] if _mode[1] else []) + ["agrl_graph_finalize_bits"],
            lambda: graph_operands(3, 20, 2048, packed=True))
    def _run(o, mode=_mode):
        return (ops_().graph_matrix(o["f"], o["adj"], True, mode[1], mask_diag=True),)

for _shape in ((3, 20, 2048), (3, 49, 512)):
    _sn = "%dx%dx%d" % _shape

    @family("graph_propagate-%s" % _sn, ["agrl_linear_nobias", "agrl_graph_propagate"], lambda s=_shape: graph_operands(*s))
    def _run(o):
        ops = ops_()
        B, V, C = o["f"].shape
        h = mid(o, ops.linear_nobias(o["f"].view(B * V, C), o["w"])).view(B, V, C)
        return (h,) + ops.graph_propagate(o["f"], h, o["G"], o["scale"], o["shift"], 0.1, 0.1, want_lp=True)

    for _dt in (F32, LP_DTYPE):
        @family("graph_apply_operand+linear_mix-%s-%s" % (_sn, dt_name(_dt)),
                ["agrl_graph_apply" if _shape[1] % 4 == 0 else "agrl_graph_propagate", "agrl_graph_linear_mix"], lambda s=_shape: graph_operands(*s))
        def _run(o, d=_dt):
            ops = ops_()
            P = mid(o, ops.graph_apply_operand(o["G"], o["f"], d))
            return P, ops.graph_linear_mix(P, o["w"] if d == F32 else mid(o, o["w"].to(d)), o["f"], o["scale"], o["shift"], 0.1, 0.1)

    @family("graph_linear_mix-%s-bf16x3" % _sn, ["agrl_graph_apply" if _shape[1] % 4 == 0 else "agrl_graph_propagate", "agrl_graph_linear_mix"],
            lambda s=_shape: graph_operands(*s))
    def _run(o):
        ops = ops_()
        with ops.f32_split():
            P = mid(o, ops.graph_apply_operand(o["G"], o["f"], F32))
            return P, ops.graph_linear_mix(P, o["w"], o["f"], o["scale"], o["shift"], 0.1, 0.1)

    for _pre in ((False, True) if _shape[1] % 4 == 0 else (False,)):
        @family("graph_linear_mix-%s-fp16x3%s" % (_sn, "-presplit" if _pre else ""),
                ["agrl_graph_apply" if _shape[1] % 4 == 0 else "agrl_graph_propagate", "agrl_graph_linear_mix"], lambda s=_shape: graph_operands(*s))
        def _run(o, pre=_pre):
            ops = ops_()
            w = mid(o, ops.split16_inloop_weights(o["w"]))
            scale = (o["scale"] * w.agrl_unscale).contiguous()
            scale.agrl_folded_unscale = w.agrl_unscale
            P = mid(o, ops.graph_apply_operand(o["G"], o["f"], F32, presplit=pre))
            return P, ops.graph_linear_mix(P, w, o["f"], mid(o, scale), o["shift"], 0.1, 0.1, p_presplit=pre)


@family("graph_finalize+graph_apply-V20", ["agrl_graph_gram", "agrl_graph_finalize", "agrl_graph_propagate"], lambda: graph_operands(3, 20, 2048))
def _run(o):
    ops = ops_()
    gram = mid(o, ops.graph_gram(o["f"]))
    G = mid(o, ops.graph_finalize(gram, o["adj"], 3, 20, True, True))
    return gram, G, ops.graph_apply(G, o["f"])


for _name, _shape, _mode, _packed in (("3x64x512-learned", (3, 64, 512), (False, True), False), ("4x20x1024-pose-packed", (4, 20, 1024), (True, False), True),
                                      ("4x20x1024-pose-learned", (4, 20, 1024), (True, True), False)):
    for _dt in (F32, LP_DTYPE):
        @family("graph_tracklet_operand-%s-%s" % (_name, dt_name(_dt)), ["agrl_graph_tracklet_operand"], lambda s=_shape, p=_packed: graph_operands(*s, packed=p))
        def _run(o, mode=_mode, d=_dt):
            return ops_().graph_tracklet_operand(o["f"], o["adj"], mode[0], mode[1], d, want_graph=True)


def pose_operands(B, S, H):
    rng = np.random.RandomState(17)
    poses = np.stack([rng.rand(B, S, 18) * 128, rng.rand(B, S, 18) * (H + 8) - 4, rng.rand(B, S, 18) * 0.5], axis=-1).astype(np.float32)
    return {"poses": torch.from_numpy(poses), "det": torch.from_numpy((rng.rand(B, S) > 0.15).astype(np.uint8))}


for _packed in (False, True):
    @family("pose_adjacency-2x6-h100-split2%s" % ("-bits" if _packed else ""), ["agrl_pose_adjacency_bits" if _packed else "agrl_pose_adjacency"],
            lambda: pose_operands(2, 6, 100))
    def _run(o, packed=_packed):
        return (ops_().pose_adjacency(o["poses"], o["det"], 100, 2, True, packed=packed),)


@family("adjacency_pack-4x35", ["agrl_adjacency_pack"], lambda: {"adj": (ru(gen(3), 4, 35, 35) > 0.5).float()})
def _run(o):
    return (ops_().adjacency_pack(o["adj"]),)


# ---- distance matrix and ranking -------------------------------------------------------------------------------------------------------
for _dt in (F32, LP_DTYPE):
    @family("row_sqnorm-64x7-%s" % dt_name(_dt), ["agrl_row_sqnorm"], lambda d=_dt: {"x": rn(gen(71), 64, 7, dt=d)})
    def _run(o):
        return (ops_().row_sqnorm(o["x"]),)

for _shape, _norm, _dt in (((5, 2048, 1), True, LP_DTYPE), ((37, 100, 64), True, F32), ((37, 100, 64), False, LP_DTYPE)):
    @family("row_l2_normalize-%dx%d-pad%d-%s-%s" % (_shape + ("unit" if _norm else "copy", dt_name(_dt))), ["agrl_row_l2_normalize"],
            lambda s=_shape: {"x": rn(gen(sum(s)), s[0], s[1])})
    def _run(o, s=_shape, norm=_norm, d=_dt):
        return (ops_().row_l2_normalize(o["x"], norm, d, s[2]),)

for _shape in ((5, 300, 96), (64, 4099, 128)):
    for _metric in ("euclidean", "cosine"):
        for _prec in ("fp32", LP16):
            @family("distmat-%dx%dx%d-%s-%s" % (_shape + (_metric, "fp32" if _prec == "fp32" else "lp16")),
                    ["agrl_distmat"] + (["agrl_row_sqnorm"] if _metric == "euclidean" else []) + (
                        [] if (_metric == "euclidean" and _prec == "fp32") else ["agrl_row_l2_normalize"]), lambda s=_shape: distmat_operands(*s))
            def _run(o, metric=_metric, prec=_prec):
                from torchreid.metrics.distance import hip_distmat_device
                q, g, qn, gn, _ = distance_operands(o, metric, prec)
                got = (ops_().distmat(q, g, metric, qn, gn),)
                return same_as_host_path(o, got, (hip_distmat_device(o["q"], o["g"], metric, prec),))

for _prec in ("fp32", LP16):
    @family("distmat_topk-130x517x64-%s" % ("fp32" if _prec == "fp32" else "lp16"), ["agrl_distmat_topk", "agrl_row_sqnorm"] + ([] if _prec == "fp32" else ["agrl_row_l2_normalize"]),
            lambda: distmat_operands(130, 517, 64))
    def _run(o, prec=_prec):
        from torchreid.metrics.distance import hip_distmat_topk_device
        q, g, qn, gn, _ = distance_operands(o, "euclidean", prec)
        got = ops_().distmat_topk(q, g, "euclidean", 50, qn, gn)
        return same_as_host_path(o, got, hip_distmat_topk_device(o["q"], o["g"], "euclidean", 50, prec))


def topk_operands(m, n, k):
    """the rows of tests/test_gpu_kernels.py::test_rank_topk_single_pass_form: equal values, NaN, +-inf, -0.0 -- the values (output 1) hold
    NaN where the distances do"""
    rng = np.random.RandomState(m * n + k)
    d = rng.randn(m, n).astype(np.float32)
    d[0] = np.float32(0.5)
    d[1, ::7], d[1, 3], d[1, 11 % n] = np.nan, -np.inf, np.inf
    d[2, : n // 2], d[2, n // 2:] = np.float32(-0.0), np.float32(0.0)
    d[3] = np.sort(d[3])
    d[4, k // 2:] = np.nan
    return {"d": torch.from_numpy(d)}


for _shape in ((6, 37, 30), (5, 1023, 20)):
    @family("rank_topk-%dx%dx%d" % _shape, ["agrl_rank_topk"], lambda s=_shape: topk_operands(*s), poison_ok=(1,))
    def _run(o, k=_shape[2]):
        return ops_().rank_topk(o["d"], k)


def unaligned_operands():
    wide = torch.zeros((6, 40))
    wide[:, 1:38] = topk_operands(6, 37, 30)["d"]
    return {"wide": wide}


@family("rank_topk-6x37x30-unaligned-view", ["agrl_rank_topk"], unaligned_operands, poison_ok=(1,))
def _run(o):
    return ops_().rank_topk(o["wide"][:, 1:38], 30)       # base pointer + 4 bytes, rows 160 bytes apart


def argsort_operands():
    d = np.random.RandomState(39).randn(6, 33).astype(np.float32)
    d[0, ::3] = np.float32(0.25)
    d[1, 5], d[1, 7], d[1, 2] = np.nan, -np.inf, np.inf
    d[2, :16], d[2, 16:] = np.float32(-0.0), np.float32(0.0)
    return {"d": torch.from_numpy(d)}


@family("rank_argsort-6x33", ["agrl_rank_argsort"], argsort_operands)
def _run(o):
    return (ops_().rank_argsort(o["d"]),)


def protocol_operands(m, n, absent=2):
    """``absent``: identities among the queries that the gallery does not hold"""
    rng = np.random.RandomState(m + n)
    d = rng.rand(m, n).astype(np.float32)
    d[:, 5] = d[:, 3]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
    return {"d": torch.from_numpy(d), "q_pids": i32(rng.randint(0, 4 + absent, m)), "g_pids": i32(rng.randint(0, 4, n)), "q_cam": i32(rng.randint(0, 6, m)),
            "g_cam": i32(rng.randint(0, 6, n))}


# ap is NaN for a query without a valid gallery match (tests/test_gpu_kernels.py::test_rank_market1501_device): output 0 may hold NaN
@family("rank_market1501-7x64", ["agrl_rank_market1501"], lambda: protocol_operands(7, 64), poison_ok=(0,))
def _run(o):
    return ops_().rank_market1501(o["d"], o["q_pids"], o["q_cam"], o["g_pids"], o["g_cam"], 50)


@family("rank_mars-7x64", ["agrl_rank_topk", "agrl_rank_mars"], lambda: protocol_operands(7, 64, absent=0))
def _run(o):
    ops = ops_()
    idx, val = ops.rank_topk(o["d"], 64)      # the whole gallery: every query meets its matches
    idx = mid(o, idx)
    return (idx, val) + ops.rank_mars(idx, o["q_pids"], o["q_cam"], o["g_pids"], o["g_cam"])


def rerank_operands():
    import rerank_ref as R
    name, metric, k1, k2 = min(R.GRID, key=lambda c: R.CASES[c[0]]["m"] * R.CASES[c[0]]["n"])      # m = 1, n = 32: one ragged tile
    qg, qq, gg = R.world(name, metric)
    return {"qg": torch.from_numpy(np.array(qg)), "qq": torch.from_numpy(np.array(qq)), "gg": torch.from_numpy(np.array(gg)), "k1": k1, "k2": k2}


@family("re_ranking-smallest-world", ["agrl_re_ranking"], rerank_operands)
def _run(o):
    return (ops_().re_ranking(o["qg"], o["qq"], o["gg"], k1=o["k1"], k2=o["k2"], lambda_value=0.3),)


# ---- train step ------------------------------------------------------------------------------------------------------------------------
for _cfg in ((1, 4, 4, 4, 4, 5, 1, 2), (3, 7, 5, 36, 20, 3, 1, 1)):
    def _make(c=_cfg):
        F_, H, W, Cin, Cout, R, stride, pad = c
        g = gen(sum(c))
        OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
        return {"x": rn(g, F_, H, W, Cin), "dy": rn(g, F_, OH, OW, Cout)}

    for _split in (False, True):
        @family("conv_wgrad-%s%s" % ("x".join(str(v) for v in _cfg), "-bf16x3" if _split else ""), ["agrl_conv_wgrad"], _make)
        def _run(o, c=_cfg, split=_split):
            ops = ops_()
            assert ops.conv_wgrad_supported(c[3], c[4])
            with ops.f32_split(split):
                return (ops.conv_wgrad(o["x"], o["dy"], (c[4], c[3], c[5], c[5]), c[6], c[7]),)


@family("conv_stats-3x9x5x64x128k3s2", ["agrl_conv2d_stats", "agrl_bn_stats_from_partials"], lambda: conv_operands((3, 9, 5, 64, 128, 3, 2), F32, False))
def _run(o):
    return ops_().conv_stats(o["x"], o["w"], 2, 1)


def bn_operands():
    g = gen(128)
    return {"y": rn(g, 135, 128) * (0.5 + ru(g, 128)) + rn(g, 128), "gamma": 0.8 + 0.4 * ru(g, 128), "beta": rn(g, 128, s=0.1), "res": rn(g, 135, 128),
            "dout": rn(g, 135, 128), "rm": rn(g, 128, s=0.1), "rv": 0.5 + ru(g, 128), "nbt": torch.tensor(3, dtype=torch.int64)}


@family("bn_stats+fold+apply+backward-3x9x5x128", ["agrl_bn_stats", "agrl_bn_fold_train", "agrl_bn_apply", "agrl_bn_backward"], bn_operands)
def _run(o):
    ops = ops_()
    mean, var = mid(o, *ops.bn_stats(o["y"]))
    scale, shift, invstd = mid(o, *ops.bn_fold_train(mean, var, o["gamma"], o["beta"], 1e-5, 0.1, 135, o["rm"], o["rv"], o["nbt"]))
    out, mask = ops.bn_apply(o["y"], scale, shift, o["res"], True, want_mask=True)
    mask = mid(o, mask)
    dy, dz, dgamma, dbeta = ops.bn_backward(o["dout"], None, o["y"], mean, invstd, o["gamma"], True, True, mask=mask)
    out2, _ = ops.bn_apply(o["y"], scale, shift, None, True, slope=0.1)
    out2 = mid(o, out2)
    dy2, _, dgamma2, dbeta2 = ops.bn_backward(o["dout"], out2, o["y"], mean, invstd, o["gamma"], True, False, slope=0.1)
    return mean, var, scale, shift, invstd, o["rm"], o["rv"], o["nbt"], out, mask, dy, dz, dgamma, dbeta, out2, dy2, dgamma2, dbeta2


@family("im2col_rows-2x3x9x7-k7s2-ld148", ["agrl_im2col_rows"], lambda: {"x": rn(gen(28), 2, 9, 7, 3)})
def _run(o):
    return (ops_().im2col_rows(o["x"], 7, 7, 2, 3, 148)[0],)


# the GEMM's K is a whole number of 32-value k-tiles: the patches padded to 160 columns; 40 rows and 20 channels, ragged in both
@family("im2col_rows+gemm_nt_splitk-2x3x9x7-k7s2-ld160", ["agrl_im2col_rows", "agrl_gemm_nt_splitk"],
        lambda: {"x": rn(gen(28), 2, 3, 9, 7), "w": rn(gen(29), 20, 160, s=0.1)})
def _run(o):
    ops = ops_()
    P, OH, OW = ops.im2col_rows(o["x"], 7, 7, 2, 3, 160, nchw=True)
    P = mid(o, P)
    return P, ops.gemm_nt_splitk(P, o["w"])


@family("im2col_rows-nhwc-2x8x6x5-k3", ["agrl_im2col_rows"], lambda: {"x": rn(gen(30), 2, 8, 6, 5)})
def _run(o):
    return (ops_().im2col_rows(o["x"], 3, 3, 1, 1, 72)[0],)


@family("im2col_t-3x7x5x36-k3", ["agrl_im2col_t"], lambda: {"x": rn(gen(31), 3, 7, 5, 36)})
def _run(o):
    return (ops_().im2col_t(o["x"], 3, 3, 1, 1),)


@family("graph_gram+pair_product-5x7x384", ["agrl_graph_gram", "agrl_graph_pair_product"], lambda: {"a": rn(gen(32), 5, 7, 384), "b": rn(gen(33), 5, 7, 384)})
def _run(o):
    ops = ops_()
    return ops.graph_gram(o["a"]), ops.graph_pair_product(o["a"], o["b"])


def triplet_operands():
    x = rn(gen(1), 9, 256)
    x[4] = x[3]
    return {"x": x, "pids": torch.tensor([0, 0, 1, 1, 1, 2, 3, 3, 3], dtype=torch.int32)}


for _soft in (True, False):
    @family("triplet_loss-9x256-tied-%s" % ("soft" if _soft else "margin"), ["agrl_triplet_loss"], triplet_operands)
    def _run(o, soft=_soft):
        return ops_().triplet_loss(o["x"], o["pids"], 0.3, soft)


@family("triplet_hard_mine-9x256-tied", ["agrl_triplet_hard_mine"], triplet_operands)
def _run(o):
    return ops_().triplet_hard_mine(o["x"], o["pids"])


def relu_levels(g, *shape):
    return (rn(g, *shape).relu() * 4).round() / 4       # many exact ties and zeros: the first maximum decides


@family("maxpool3x3s2-2x9x7x32", ["agrl_maxpool3x3s2", "agrl_maxpool3x3s2_backward"], lambda: {"x": relu_levels(gen(34), 2, 9, 7, 32), "dout": rn(gen(35), 2, 5, 4, 32)})
def _run(o):
    ops = ops_()
    out, idx = ops.maxpool3x3s2(o["x"])
    idx = mid(o, idx)
    return out, idx, ops.maxpool3x3s2_backward(o["dout"], idx, 9, 7)


for _dt, _split in ((F32, False), (F32, True), (LP_DTYPE, False)):
    @family("linear_nobias-37x100x%s%s" % (dt_name(_dt), "-bf16x3" if _split else ""), ["agrl_linear_nobias"],
            lambda d=_dt: {"x": rn(gen(36), 37, 192, dt=d), "w": rn(gen(37), 100, 192, s=0.07, dt=d)})
    def _run(o, split=_split):
        ops = ops_()
        with ops.f32_split(split):
            return (ops.linear_nobias(o["x"], o["w"]),)


@family("xent_label_smooth-7x625", ["agrl_xent_label_smooth"], lambda: {"logits": rn(gen(38), 7, 625, s=3.0),
                                                                        "targets": torch.randint(0, 625, (7,), generator=gen(39), dtype=torch.int32)})
def _run(o):
    return ops_().xent_label_smooth(o["logits"], o["targets"], 0.1)


@family("part_pool_backward-3x14x7x96-421", ["agrl_part_pool_backward"], lambda: {"dg": rn(gen(40), 1, 96), "dnodes": rn(gen(41), 3, 7, 96)})
def _run(o):
    return ops_().part_pool_backward(o["dg"], o["dnodes"], 3, 14, 7, [4, 2, 1])


@family("attn_pool_backward-2x3x5x260", ["agrl_attn_pool_backward"], lambda: {"nodes": ru(gen(42), 2, 3, 5, 260), "datt": rn(gen(43), 2, 260)})
def _run(o):
    return (ops_().attn_pool_backward(o["nodes"], o["datt"]),)


@family("graph_matrix_backward-1x7x128", ["agrl_graph_gram", "agrl_graph_matrix_backward"], lambda: {"f": ru(gen(44), 1, 1, 128) + 0.02 * rn(gen(45), 1, 7, 128),
                                                                                                     "dG": rn(gen(46), 1, 7, 7)})
def _run(o):
    ops = ops_()
    gram = mid(o, ops.graph_gram(o["f"]))
    return gram, ops.graph_matrix_backward(gram, o["dG"], True, mask_diag=True)


@family("axpby-1001", ["agrl_axpby"], lambda: {"x": rn(gen(47), 7, 143), "y": rn(gen(48), 7, 143)})
def _run(o):
    ops = ops_()
    return ops.axpby(0.5, o["x"], -2.0, o["y"]), ops.axpby(3.0, o["x"])


@family("col_sum-135x66", ["agrl_col_sum"], lambda: {"x": rn(gen(49), 135, 66)})
def _run(o):
    return (ops_().col_sum(o["x"]),)


def pam_train_operands():
    g = gen(96)
    return {"x": rn(g, 2, 6, 5, 96), "qk": rn(g, 2, 6, 5, 64, s=0.3), "dxbar": rn(g, 2, 7, 96), "dxmean": rn(g, 2, 7, 96), "y": rn(g, 2, 7, 96),
            "bv": rn(g, 96, s=0.1), "gamma": torch.tensor([0.5]), "dnodes": rn(g, 2, 7, 96)}


@family("pam_pool_train+backward-2x6x5x96x32-421", ["agrl_pam_pool_train", "agrl_pam_pool_backward"], pam_train_operands)
def _run(o):
    ops = ops_()
    return ops.pam_pool_train(o["x"], o["qk"], [4, 2, 1]) + ops.pam_pool_backward(o["x"], o["qk"], o["dxbar"], o["dxmean"], [4, 2, 1], want_abar=True)


@family("pam_combine_train+backward-2x7x96", ["agrl_pam_combine_train", "agrl_pam_combine_backward"], pam_train_operands)
def _run(o):
    ops = ops_()
    return (ops.pam_combine_train(o["y"], o["bv"], o["dxmean"], o["gamma"]),) + ops.pam_combine_backward(o["dnodes"], o["y"], o["bv"], o["gamma"])


# ---- STA tails -------------------------------------------------------------------------------------------------------------------------
for _dt in (F32, LP_DTYPE):
    @family("sta_frame_stats-2x7x3x264-%s" % dt_name(_dt), ["agrl_sta_frame_stats"], lambda d=_dt: {"x": rn(gen(300), 2, 7, 3, 264, dt=d)})
    def _run(o):
        return ops_().sta_frame_stats(o["x"])

    @family("linear_bn_relu-5x64x8-%s" % dt_name(_dt), ["agrl_linear_bn_relu"],
            lambda d=_dt: {"x": rn(gen(301), 5, 64), "w": rn(gen(302), 8, 64, s=0.125, dt=d), "scale": 0.8 + 0.4 * ru(gen(303), 8), "shift": rn(gen(304), 8, s=0.1)})
    def _run(o):
        return (ops_().linear_bn_relu(o["x"], o["w"], o["scale"], o["shift"]),)


def fuse_operands():
    g = gen(31 * 2 + 7 * 5 + 264)
    target = torch.stack([torch.stack([1.12 ** torch.randperm(5, generator=g).float() for _ in range(4)], dim=1) for _ in range(2)])
    v = rn(g, 2, 5, 4, 264)
    v = v / v.norm(dim=3, keepdim=True) * target.unsqueeze(3)
    nsq = 0.5 + ru(g, 2, 5, 4)
    npix = torch.tensor([(r1 - r0) * 3 for r0, r1 in ops_().sta_bins(7)], dtype=F32)
    nsum = target * npix * nsq.sum(dim=2, keepdim=True).sqrt()
    return {"v": v.reshape(10, 4, 264).contiguous(), "nsum": nsum.reshape(10, 4).contiguous(), "nsq": nsq.reshape(10, 4).contiguous()}


for _mode in ("map", "norm"):
    @family("sta_fuse-2x5x264-%s" % _mode, ["agrl_sta_fuse"], fuse_operands)
    def _run(o, mode=_mode):
        ops = ops_()
        return ops.sta_fuse(o["v"], 2, 5, o["nsum"], o["nsq"], (7, 3)) if mode == "map" else ops.sta_fuse(o["v"], 2, 5)


# ---- byte kernels and optimisers: their own tests already stand their outputs between sentinel bands; checks 2 and 3 only ---------------
def frames_operands():
    g = gen(77)
    rects = np.array([[[1, 2, 5, 7], [0, 0, 3, 3]], [[10, 4, 27, 20], [0, 0, 1, 1]], [[36, 28, 1, 1], [5, 5, 9, 9]]], dtype=np.int64)
    return {"u8": torch.randint(0, 256, (3, 37, 29, 3), generator=g, dtype=torch.uint8), "rects": rects, "counts": np.array([2, 1, 0], dtype=np.int64)}


@family("frames_normalize-3x37x29", ["agrl_frames_normalize_u8"], frames_operands, fence_outputs=False)
def _run(o):
    return (ops_().frames_normalize(o["u8"]),)


@family("frames_normalize_erase-3x37x29", ["agrl_frames_normalize_erase_u8"], frames_operands, fence_outputs=False)
def _run(o):
    return (ops_().frames_normalize_erase(o["u8"], o["rects"], o["counts"]),)


@family("clip_resample-3x37x29-to-16x8", ["agrl_clip_resample_u8"],
        lambda: dict(frames_operands(), geometry=np.array([[37, 29, 0, 0, 37, 29, 0, 0], [30, 20, 3, 2, 25, 17, 1, 0], [37, 29, 5, 5, 16, 8, 0, 0]], dtype=np.int64)),
        fence_outputs=False)
def _run(o):
    return (ops_().clip_resample(o["u8"], o["geometry"], (16, 8)),)


# agrl_resample_taps_u8 reads no device memory (two sizes in, two tables out): ``where`` only names the device. Check 1 (the tables
# stay inside their tensors) and the stream half of check 3 are what hold it; check 2 has no operand to put bytes around.
@family("resample_taps-37-to-16", ["agrl_resample_taps_u8"], lambda: {"where": torch.zeros(1)})
def _run(o):
    return ops_().resample_taps_device(37, 16, o["where"].device)


def jpeg_operands():
    import jpeg_cases as J
    from torchreid import device_decode as dd
    ops = ops_()
    plan = dd.jpeg_batch_plan([dd.parse_jpeg(J.fixture()[J.names((17, 9), "420")[0]][0])])
    scans, desc, quant, huff = ops.jpeg_upload(plan, torch.device("cpu"))
    return {"plan": plan, "scans": scans.clone(), "desc": desc.clone(), "quant": quant.clone(), "huff": huff.clone()}


@family("jpeg_decode-17x9-420", ["agrl_jpeg_decode_u8"], jpeg_operands, fence_outputs=False)
def _run(o):
    return ops_().jpeg_decode(o["plan"], operands=(o["scans"], o["desc"], o["quant"], o["huff"]))


def png_operands():
    import png_cases as P
    from torchreid import device_decode as dd
    ops = ops_()
    plan = dd.png_batch_plan([dd.parse_png(P.fixture()["7x9_rgb_smooth_f4"][0])])
    streams, desc = ops.png_upload(plan, torch.device("cpu"))
    return {"plan": plan, "streams": streams.clone(), "desc": desc.clone()}


@family("png_decode-7x9-rgb", ["agrl_png_decode_u8"], png_operands, fence_outputs=False)
def _run(o):
    return ops_().png_decode(o["plan"], operands=(o["streams"], o["desc"]))


def optim_operands():
    g = gen(2024)
    o = {}
    for i, n in enumerate((5, 4099, 64)):      # below one vector, a ragged second chunk, a whole vector count
        o["p%d" % i], o["g%d" % i] = rn(g, n), rn(g, n, s=0.1)
        o["s0_%d" % i], o["s1_%d" % i], o["s2_%d" % i] = rn(g, n, s=0.01), ru(g, n, s=0.01), ru(g, n, s=0.02)
    return o


def optim_tables(o, states):
    from torchreid import hip_optim as H
    rows = [tuple(o[k % i].data_ptr() for k in ("p%d", "g%d")) + tuple(o["s%d_%d" % (s, i)].data_ptr() if s < states else 0 for s in range(3))
            + (o["p%d" % i].numel(),) for i in range(3)]
    dev = o["p0"].device
    tensors = mid(o, torch.from_numpy(H.build_descriptors(rows)).to(dev))
    chunks = mid(o, torch.from_numpy(H.build_chunk_table([r[5] for r in rows])).to(dev))
    return tensors, chunks, tuple(o[k] for k in sorted(o) if isinstance(o[k], torch.Tensor))


@family("adam_step-amsgrad-5+4099+64", ["agrl_adam_step"], optim_operands, fence_outputs=False)
def _run(o):
    from torchreid import hip_optim as H
    t, c, outs = optim_tables(o, 3)
    ops_().adam_step(t, c, 5e-4, *H.adam_constants(3e-4, 0.9, 0.999, 3), 1e-8, True, True)
    return outs


@family("sgd_step-nesterov-5+4099+64", ["agrl_sgd_step"], optim_operands, fence_outputs=False)
def _run(o):
    t, c, outs = optim_tables(o, 1)
    ops_().sgd_step(t, c, 5e-4, 0.9, 0.01, True, False, True, False)
    return outs


@family("rmsprop_step-momentum-5+4099+64", ["agrl_rmsprop_step"], optim_operands, fence_outputs=False)
def _run(o):
    t, c, outs = optim_tables(o, 2)
    ops_().rmsprop_step(t, c, 5e-4, 0.99, 0.01, 1e-8, 0.9, 0.01, True, True)
    return outs


@family("adabound_step-amsbound-5+4099+64", ["agrl_adabound_step"], optim_operands, fence_outputs=False)
def _run(o):
    from torchreid import hip_optim as H
    t, c, outs = optim_tables(o, 3)
    omb1, beta2, omb2, step_size, lower, upper = H.adabound_constants(1e-3, 0.9, 0.999, 3, 0.1, 1e-3, 1e-3)
    ops_().adabound_step(t, c, 5e-4, omb1, beta2, omb2, step_size, 1e-8, lower, upper, True, False)
    return outs


for _adaptive in (True, False):
    @family("radam_step-%s-5+4099+64" % ("adaptive" if _adaptive else "momentum-only"), ["agrl_radam_step"], optim_operands, fence_outputs=False)
    def _run(o, adaptive=_adaptive):
        t, c, outs = optim_tables(o, 2)
        ops_().radam_step(t, c, 0.1, 0.999, 0.001, 1.0 - 1e-3 * 5e-4, 2e-3, 1e-8, adaptive, True)
        return outs


# ---- the declared map: entry point -> the families that reach it (held against _hip.SIGNATURES by tests/test_bounds.py) -----------------
NOT_FENCED = {"agrl_diag_read_stream"}      # the bench's read yardstick: one sink element, no result anyone reads
ENTRY_POINTS = {}
for _f in FAMILIES.values():
    for _ep in _f.entry_points:
        ENTRY_POINTS.setdefault(_ep, []).append(_f.name)


def launching_entry_points():
    """The entry points of torchreid._hip.SIGNATURES that launch: every one takes the stream as its last (pointer) argument; the size
    queries, the plans and the switches do not."""
    import ctypes
    from torchreid import _hip
    return {name for name, argtypes in _hip.SIGNATURES.items() if len(argtypes) > 1 and argtypes[-1] is ctypes.c_void_p}


# ---- harness ---------------------------------------------------------------------------------------------------------------------------
_OPERANDS = {}


def operands(fam):
    """the family's seeded operands on the device, built once and never written: every call gets copies"""
    if fam.name not in _OPERANDS:
        _OPERANDS[fam.name] = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in fam.make().items()}
        torch.cuda.synchronize()
    return _OPERANDS[fam.name]


def copies(ops_dict, copy):
    return {k: (copy(v) if isinstance(v, torch.Tensor) else v) for k, v in ops_dict.items()}


@contextlib.contextmanager
def switches(fam):
    """The family's AGRL_* switches in the environment and in the library, as its own test sets them; the autouse fixture of
    conftest.py puts the library back on the restored environment afterwards."""
    from torchreid import _hip
    old = {k: os.environ.get(k) for k in fam.env}
    os.environ.update(fam.env)
    if fam.env:
        _hip.reload_options()
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if fam.env:
            _hip.reload_options()


def tensors_of(outs):
    assert isinstance(outs, tuple), type(outs)
    return [t for t in outs if t is not None]


def bits(t):
    t = t.contiguous()
    if t.is_floating_point():
        return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def first_difference(name, what, got, want):
    assert len(got) == len(want), (name, what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        if not same_bits(a, b):
            d = (bits(a) != bits(b)).reshape(-1) if a.shape == b.shape and a.dtype == b.dtype else None
            n = int(d.sum()) if d is not None else -1
            at = int(torch.nonzero(d)[0]) if n > 0 else -1
            return "%s: output %d (%s %s) %s: %d of %d elements differ, the first at flat index %d" % (
                name, i, tuple(a.shape), a.dtype, what, n, a.numel(), at)
    return None


def skip_other_build(fam):
    if fam.fp16_only and not FP16_BUILD:
        pytest.skip("split-fp16 plane kernels: fp16 build only")


@contextlib.contextmanager
def recorded_calls():
    """names of the entry points called inside the block (hip_ops binds ``call`` by name: both bindings are wrapped)"""
    from torchreid import _hip, hip_ops
    names, real = [], _hip.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    _hip.call = hip_ops.call = call
    try:
        yield names
    finally:
        _hip.call = hip_ops.call = real


def check_outputs_stay_inside(fam):
    o = copies(operands(fam), torch.clone)
    with switches(fam), recorded_calls() as called:
        with poisoned_outputs() as fences:      # raises on leaving the block when a band was hit
            outs = tensors_of(fam.run(o))
            count = len(fences)
        torch.cuda.synchronize()
    name = fam.name
    bounds.log_record({"name": "fences|%s" % name, "fenced_allocations": count, "entry_points": sorted(set(called))})
    assert count > 0, "%s: no allocation of the call went through the fence" % name
    assert set(fam.entry_points) <= set(called), "%s declares %s but called %s" % (name, sorted(fam.entry_points), sorted(set(called)))
    for i, t in enumerate(outs):
        if i in fam.poison_ok:
            continue
        if t.is_floating_point():
            assert not bool(torch.isnan(t).any()), "%s: output %d (%s %s) holds %d NaN: unwritten, or NaN from an unwritten buffer" % (
                name, i, tuple(t.shape), t.dtype, int(torch.isnan(t).sum()))
        elif t.dtype in (torch.int32, torch.int64):
            assert not bool((t == INT_SENTINEL).any()), "%s: output %d (%s %s) holds the integer sentinel" % (name, i, tuple(t.shape), t.dtype)


def check_neighbour_independence(fam):
    runs = []
    with switches(fam), recorded_calls() as called:
        for fill in FILLS:
            o = copies(operands(fam), lambda t, fill=fill: fenced(t, fill))
            o["mid"] = lambda t, fill=fill: fenced(t, fill)      # ... and every buffer that one launch of run() hands to the next
            runs.append([t.clone() for t in tensors_of(fam.run(o))])
            torch.cuda.synchronize()
    # the families that stay out of check 1 have their declaration held against the calls here
    assert set(fam.entry_points) <= set(called), "%s declares %s but called %s" % (fam.name, sorted(fam.entry_points), sorted(set(called)))
    for fill, outs in zip(FILLS[1:], runs[1:]):
        msg = first_difference(fam.name, "changes when the bytes around the operands are 0x%02X instead of 0x00" % fill, outs, runs[0])
        assert msg is None, msg


_SCRATCH = []


def slow_producer():
    """a few milliseconds of work on the current stream: a chain of elementwise passes over 256 MiB"""
    if not _SCRATCH:
        _SCRATCH.append(torch.zeros(1 << 26, dtype=F32, device=DEV))
    s = _SCRATCH[0]
    for _ in range(12):
        s.add_(1.0)
        s.mul_(0.5)
    return s


def hollow(t):
    """an operand buffer holding NaN, or -1 for integers: what a launch that does not wait for the copies reads"""
    return torch.full_like(t, float("nan")) if t.is_floating_point() else torch.full_like(t, 0xFF if t.dtype == torch.uint8 else -1)


def check_side_stream(fam):
    src = operands(fam)
    with switches(fam):
        want = [t.clone() for t in tensors_of(fam.run(copies(src, torch.clone)))]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            o = copies(src, hollow)
            slow_producer()
            for k, v in o.items():
                if isinstance(v, torch.Tensor):
                    v.copy_(src[k], non_blocking=True)
            got = [t.clone() for t in tensors_of(fam.run(o))]
        side.synchronize()
        torch.cuda.synchronize()
    msg = first_difference(fam.name, "differs between the side stream and the default stream", got, want)
    assert msg is None, msg


NAMES = list(FAMILIES)
FENCED = [n for n in NAMES if FAMILIES[n].fence_outputs]


@pytest.mark.parametrize("name", FENCED)
def test_outputs_stay_inside_their_tensors(name):
    skip_other_build(FAMILIES[name])
    check_outputs_stay_inside(FAMILIES[name])


@pytest.mark.parametrize("name", NAMES)
def test_outputs_do_not_depend_on_bytes_outside_the_operands(name):
    skip_other_build(FAMILIES[name])
    check_neighbour_independence(FAMILIES[name])


@pytest.mark.parametrize("name", NAMES)
def test_side_stream_run_equals_the_default_stream_run(name):
    skip_other_build(FAMILIES[name])
    check_side_stream(FAMILIES[name])


# ---- the three checks can tell: torch "kernels" with the defect each one is there for (no library code, nothing outside the test's
# own allocations is touched) ---------------------------------------------------------------------------------------------------
def _one_past(t):
    """the element behind ``t`` in its own storage: a band of a fenced tensor"""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + t.numel())


def _fake(name, run):
    return Family("selftest-" + name, [], lambda: {"x": rn(gen(9), 37, 5)}, run)


def test_the_checks_reject_an_overrun_an_over_read_and_a_launch_on_the_wrong_stream():
    def overrun(o):
        out = torch.empty_like(o["x"])
        out.copy_(o["x"])
        _one_past(out).fill_(1.0)
        return (out,)

    def over_read_masked_by_zero(o):
        return (o["x"] * 2 + _one_past(o["x"]) * 0,)

    def over_read_of_an_intermediate(o):
        t = mid(o, o["x"] * 2)
        return (t + _one_past(t) * 0,)

    def default_stream_whatever_the_caller_says(o):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return (o["x"] * 2,)

    def sound(o):
        out = torch.empty_like(o["x"])
        torch.mul(o["x"], 2, out=out)
        return (out,)

    with pytest.raises(AssertionError, match=r"shape \(37, 5\), torch.float32\): 4 byte\(s\) modified AFTER the tensor, first at 0 and last at 3"):
        check_outputs_stay_inside(_fake("overrun", overrun))
    with pytest.raises(AssertionError, match="changes when the bytes around the operands are 0xFF instead of 0x00"):
        check_neighbour_independence(_fake("over-read", over_read_masked_by_zero))
    with pytest.raises(AssertionError, match="changes when the bytes around the operands are 0xFF instead of 0x00"):
        check_neighbour_independence(_fake("over-read-intermediate", over_read_of_an_intermediate))
    with pytest.raises(AssertionError, match="differs between the side stream and the default stream"):
        check_side_stream(_fake("wrong-stream", default_stream_whatever_the_caller_says))
    for check in (check_outputs_stay_inside, check_neighbour_independence, check_side_stream):
        check(_fake("sound", sound))


@pytest.mark.skipif(os.environ.get("AGRL_HIP_LP16", "fp16") == "bf16", reason="this process already runs the bf16 build")
def test_bf16_build_in_a_fresh_process():
    """The 16-bit type is fixed when torchreid is imported: this file once more on libagrl_hip_bf16.so, in a fresh child interpreter
    (tests/test_gpu_bf16_build.py's pattern); only the split-fp16 plane families skip there."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AGRL_HIP_LP16="bf16")
    for k in ("AGRL_HIP_LIB", "AGRL_HIP_PRECISION", "AGRL_IGEMM_WIDE"):
        env.pop(k, None)
    t0 = time.time()
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_fences.py"], env=env,
                         cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    tail = out.stdout.decode()[-3000:]
    print(tail)
    print("bf16 child: %.1f s" % (time.time() - t0))
    plane = sum(1 for f in FAMILIES.values() if f.fp16_only)
    skipped = 3 * plane + 1       # the plane families in each of the three checks, and this test
    assert out.returncode == 0 and " passed" in tail and "%d skipped" % skipped in tail, tail
