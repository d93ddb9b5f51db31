"""The split-fp16 (hip_precision = "fp16x3") kernels held to element-by-element float64 bounds.

Every kernel call runs inside poisoned_outputs(), runs twice and must repeat bit for bit; every output element goes through
bounds.check_rounded against the references and the per-product error model of tests/split16_ref.py (C_SPLIT16 = 2^-21 relative, the
absolute terms of low halves that are not normal fp16 numbers, three MFMA chains in one accumulator), on the operands the kernel
actually reads. Plane outputs are decoded with hip_ops.from_split16_planes, get the plane half-ulp as slack and must be canonical
(the low half at most half an ulp of the high half). tests/test_split16_ref.py proves on a CPU that these checks fail for a dropped
or mis-paired cross term, a truncated high half, a low plane without its 2^11, weights that were not pre-scaled and a slab that reads
hi for lo. AGRL_BOUNDS_LOG records the worst err / bound per check (profiles/split16_bounds.txt)."""
import pytest
import torch

import split16_ref as S
from bounds import U32, log_record
from lp16 import LP16
from test_gpu_kernels import bound_pixels
from test_gpu_graph_bounds import twice_with_nans
from test_gpu_train_bounds import twice
from torchreid import _hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def fp16_build_only():
    if LP16 != "fp16":
        pytest.skip("fp16 build only")


def record(form, kind, ref):
    exact, mag, _, slack = ref
    log_record({"name": "split16|%s|%s|slack/mag" % (form, kind), "slack_over_mag_u": float((slack / mag.clamp(min=1e-300)).max() / U32)})


def presplit_host(t):
    """fp32 (..., K) -> the pre-split layout of agrl_split16_weights_inloop (same shape and bytes): per 32-value k-tile the fp16 high
    halves of lane groups c = 0..3 (k 4c..4c+3, 16+4c..16+4c+3), then the low halves in the same order."""
    K = t.shape[-1]
    v = t.reshape(-1, K // 32, 2, 4, 4).permute(0, 1, 3, 2, 4)
    hi = v.to(torch.float16)
    lo = (v - hi.float()).to(torch.float16)
    return torch.stack([hi, lo], dim=2).contiguous().view(torch.float32).view(t.shape)


def presplit_decode(t):
    """The inverse: a pre-split tensor (on the CPU) -> (hi, lo) fp32 (rows, K)."""
    K = t.shape[-1]
    v = t.contiguous().view(torch.float16).view(-1, K // 32, 2, 4, 2, 4).permute(2, 0, 1, 4, 3, 5).reshape(2, -1, K).float()
    return v[0], v[1]


def planes_decode(out, Cout, nplanes):
    """planes on the CPU (rows, nplanes Cout) -> value (hip_ops.from_split16_planes), hi, unscaled lo; a triple's third plane is its first."""
    from torchreid import hip_ops as ops
    out = out.reshape(-1, nplanes * Cout)
    if nplanes == 3:
        assert torch.equal(out[:, :Cout], out[:, 2 * Cout:])
    return ops.from_split16_planes(out, nplanes).double(), out[:, :Cout].float(), out[:, Cout:2 * Cout].float() * 2.0 ** -11


def edge_mask(rows, M, Cout, tile=128):
    return (rows >= (M // tile) * tile)[:, None] | (torch.arange(Cout) >= (Cout // tile) * tile)[None, :]


# ---- agrl_conv2d_bn_act_split16 -----------------------------------------------------------------------------------------------------
def run_inloop(case, kind, tag=""):
    from torchreid import hip_ops as ops
    N, H, W, Cin, Cout, R, stride, with_res = case
    x, w, b, res, pad = S.inloop_operands(case, kind)
    ref, pix, coords = S.inloop_conv_ref(x, w, b, stride, pad, res, relu=True)
    record("inloop", kind, ref)
    xd, bd = x.to(DEV), b.to(DEV)
    rd = None if res is None else res.to(DEV)
    wp = ops.split16_inloop_weights(w.to(DEV))
    assert torch.equal(ops.split16_true_weights(wp).cpu(), w)
    xp = presplit_host(xd)
    edge = edge_mask(pix, pix.numel(), Cout, 64)
    outs = []
    for x_pre in (False, True):                    # each flag on and off; a pre-split output takes no residual
        for out_pre in ((False,) if with_res else (False, True)):
            name = "split16|inloop|%s|%s x_presplit=%d out_presplit=%d%s" % (kind, case, x_pre, out_pre, tag)
            got = twice(lambda: ops.conv_bn_act(xp if x_pre else xd, wp, bd, stride, pad, True, residual=rd, x_presplit=x_pre, out_presplit=out_pre))
            if out_pre:
                hi, lo = presplit_decode(got)
                S.check_split16(hi.double() + lo.double(), ref, name.replace("|inloop|", "|inloop_presplit_out|"), presplit_out=True, hi=hi, lo=lo,
                                coords=coords, edge=edge)
                assert torch.equal(got.view(torch.int32), presplit_host(outs[0]).view(torch.int32))   # the halves of the fp32 output
            else:
                outs.append(got)
                S.check_split16(got.reshape(-1, Cout), ref, name, coords=coords, edge=edge)
    assert torch.equal(outs[0], outs[1])     # pre-split activations are the halves the k-loop forms


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("case", S.INLOOP_CASES)
def test_inloop_conv(case, kind):
    run_inloop(case, kind)


@pytest.mark.parametrize("ns", ["2", "3"])
def test_inloop_conv_ring_depth(ns, monkeypatch):
    """AGRL_SPLIT16_NS forces the LDS ring depth of the in-loop GEMM (unset: 3 slots for 64-channel tiles, else 2)."""
    monkeypatch.setenv("AGRL_SPLIT16_NS", ns)
    _hip.reload_options()
    for kind in ("plain", "coherent_lo"):
        run_inloop(S.INLOOP_CASES[0], kind, " ns=" + ns)


# ---- agrl_conv1x1_dual_split16 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_planes", [0, 2, 3])
@pytest.mark.parametrize("kind", S.DUAL_KINDS)
@pytest.mark.parametrize("case", S.DUAL_CASES)
def test_dual_inloop(case, kind, out_planes):
    from torchreid import hip_ops as ops
    if out_planes:
        fp16_build_only()
    N, H, W, K1, K2, Cout, stride = case
    x, x2, w, b = S.dual_operands(case, kind)
    ref = S.dual_inloop_ref(x, x2, w, b, stride)
    record("dual_inloop", kind, ref)
    xd, x2d, bd = x.to(DEV), x2.to(DEV), b.to(DEV)
    wp = ops.split16_inloop_weights(w.to(DEV))
    M = ref[0].shape[0]
    edge = edge_mask(torch.arange(M), M, Cout)
    name = "split16|dual_inloop|%s|%s out_planes=%d" % (kind, case, out_planes)
    results = []
    for pre in (False, True):
        src = presplit_host(x2d) if pre else x2d
        got = twice(lambda: ops.conv1x1_dual_split16(xd, src, wp, bd, stride, True, x2_presplit=pre, out_planes=out_planes))
        results.append(got)
        if out_planes:
            v, hi, lo = planes_decode(got, Cout, out_planes)
            S.check_split16(v, ref, name, plane_out=True, hi=hi, lo=lo, edge=edge)
        else:
            S.check_split16(got.reshape(-1, Cout), ref, name, edge=edge)
    assert torch.equal(results[0], results[1])


# ---- agrl_conv1x1_split16 / _dual / _pool -------------------------------------------------------------------------------------------
def device_planes(x):
    """fp32 CPU (M, C) -> (triple, pair) on the device, made under poisoned allocations, and the value they hold on the CPU."""
    from torchreid import hip_ops as ops
    xd = x.to(DEV)
    t3 = twice(lambda: ops.to_split16_planes(xd))
    t2 = twice(lambda: ops.to_split16_planes(xd, 2))
    C = x.shape[-1]
    assert torch.equal(t2, t3[..., :2 * C].contiguous())
    v, hi, lo = planes_decode(t3, C, 3)
    assert torch.equal(hi, x.half().float().reshape(-1, C))
    x64 = x.double().reshape(-1, C)
    assert bool(((v - x64).abs() <= S.PLANE_REL * x64.abs() + S.PLANE_ABS).all())      # the planes hold x to the plane half-ulp
    t3, t2 = t3.to(DEV), t2.to(DEV)
    S.canonical_halves(hi, lo, "agrl_split16_planes")
    return t3, t2, v


@pytest.mark.parametrize("kind", S.PLANE_KINDS)
@pytest.mark.parametrize("case", S.PLANE_CASES)
def test_plane_gemm(case, kind):
    """Triple and pair layouts: layout bit 0 = the first source is a plane pair (weights from split16_plane_weights(pair_first=True)),
    bit 1 = the residual and the result are pairs."""
    from torchreid import hip_ops as ops
    fp16_build_only()
    M, K, Cout, form = case
    xs, w, b, res = S.plane_operands(M, K, Cout, kind, form == "res")
    Ks = [t.shape[1] for t in xs]
    planes = [device_planes(t) for t in xs]
    rp = device_planes(res) if res is not None else None
    ref = S.plane_gemm_ref([p[2] for p in planes], w, b, None if rp is None else rp[2])
    record("plane_" + form, kind, ref)
    wd, bd = w.to(DEV), b.to(DEV)
    segs = Ks if len(Ks) > 1 else None
    edge = edge_mask(torch.arange(M), M, Cout)
    shape4 = lambda t: t.view(1, M, 1, -1)
    for layout in range(4):
        w3, unscale = ops.split16_plane_weights(wd, segments=segs, pair_first=bool(layout & 1))
        pk = ops.conv1x1_pack(w3)
        xin = shape4(planes[0][1] if layout & 1 else planes[0][0])
        r_in = None if rp is None else shape4(rp[1] if layout & 2 else rp[0])
        x2 = shape4(planes[1][0]) if len(planes) > 1 else None
        got = twice(lambda: ops.conv1x1_split16(xin, pk, unscale, bd, Cout, residual3=r_in, relu=True, x2=x2, layout=layout))
        v, hi, lo = planes_decode(got, Cout, 2 if layout & 2 else 3)
        S.check_split16(v, ref, "split16|plane_%s|%s|%s layout=%d" % (form, kind, case, layout), plane_out=True, hi=hi, lo=lo, edge=edge)


@pytest.mark.parametrize("kind", S.PLANE_KINDS)
@pytest.mark.parametrize("case", S.POOL_CASES)
def test_plane_pool(case, kind):
    from torchreid import hip_ops as ops
    fp16_build_only()
    N, K, Cout, splits, mean = case
    xs, w, b, res = S.plane_operands(N * 128, K, Cout, kind, True, seed=1)
    x3, _, xv = device_planes(xs[0])
    r3, r2, rv = device_planes(res)
    ref = S.plane_pool_ref(xv, w, b, rv, splits, mean, N)
    record("plane_pool", kind, ref)
    w3, unscale = ops.split16_plane_weights(w.to(DEV))
    pk, bd = ops.conv1x1_pack(w3), b.to(DEV)
    for layout in (0, 2):
        r_in = (r2 if layout & 2 else r3).view(N, 16, 8, -1)
        got = twice(lambda: ops.conv1x1_split16_pool(x3.view(N, 16, 8, -1), pk, unscale, bd, Cout, r_in, splits, mean, layout=layout))
        S.check_split16(got, ref, "split16|plane_pool|%s|%s layout=%d" % (kind, case, layout))


# ---- agrl_conv3x3_packed_split16 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.CONV3_KINDS)
@pytest.mark.parametrize("case", S.CONV3_CASES)
def test_plane_conv3x3(case, kind):
    from torchreid import hip_ops as ops
    fp16_build_only()
    N, H, W, Cin, Cout = case
    x, w, b = S.conv3_operands(case, kind)
    x3, _, xv = device_planes(x.view(-1, Cin))
    ref, pix, coords = S.plane_conv3x3_ref(xv.view(N, H, W, Cin), w, b, pixels=bound_pixels(N * H * W, 9 * Cin, Cout))
    record("plane_conv3x3", kind, ref)
    w3, unscale = ops.split16_plane_weights(w.to(DEV))
    pk, bd = ops.conv3x3_pack(w3), b.to(DEV)
    got = twice(lambda: ops.conv3x3_split16(x3.view(N, H, W, 3 * Cin), pk, unscale, bd, Cout))
    v, hi, lo = planes_decode(got, Cout, 3)
    S.check_split16(v[pix], ref, "split16|plane_conv3x3|%s|%s" % (kind, case), plane_out=True, hi=hi[pix], lo=lo[pix], coords=coords,
                    edge=edge_mask(pix, N * H * W, Cout))


# ---- agrl_stem_split16 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.STEM_CASES)
def test_stem(shape):
    """Image borders, ragged tiles, a weight row a thousand times smaller, coherent low halves; (70, 64, 48) makes more tiles than
    CUs: the persistent loop."""
    from torchreid import hip_ops as ops
    x, w, b = S.stem_operands(shape)
    ref = S.stem_ref(x, w, b)
    record("stem", "coherent_lo", ref)
    wh, wl, u = ops.pack_stem_weights_split16(w.to(DEV))
    xd, bd = x.to(DEV), b.to(DEV)
    got = twice(lambda: ops.stem_split16(xd, wh, wl, u, bd))
    S.check_split16(got.permute(0, 3, 1, 2), ref, "split16|stem|coherent_lo|%s" % (shape,))


# ---- agrl_distmat_split16 -----------------------------------------------------------------------------------------------------------
def run_distmat(q, gal, metric, name, kind="plain"):
    """hip_distmat_device(..., "fp16x3") against distmat_ref on what the kernel is given: euclidean the fp32 norms of the rows and the
    planes of q; cosine the planes of the kernel's own normalised rows."""
    from torchreid import hip_ops as ops
    from torchreid.metrics.distance import hip_distmat_device
    qd, gd = q.to(DEV), gal.to(DEV)
    got = twice(lambda: hip_distmat_device(qd, gd, metric, "fp16x3"))
    m, n = got.shape
    rows = bound_pixels(m, q.shape[1], n)
    # what the kernel is given, made by the same kernels the host path calls, under the same rule (poisoned, twice, bitwise equal)
    planes_of = lambda t: ops.from_split16_planes(twice(lambda: ops.to_split16_planes(t)))
    if metric == "euclidean":
        qn, gn = twice(lambda: ops.row_sqnorm(qd)), twice(lambda: ops.row_sqnorm(gd))
        ref = S.distmat_ref(planes_of(qd), gal, metric, qn, gn, rows=rows)
    else:
        qh, gh = twice(lambda: ops.row_l2_normalize(qd, True, torch.float32)), twice(lambda: ops.row_l2_normalize(gd, True, torch.float32))
        ref = S.distmat_ref(planes_of(qh.to(DEV)), gh, metric, rows=rows)
    record("distmat_" + metric, kind, ref)
    edge = (rows >= (m // 64) * 64)[:, None] | (torch.arange(n) >= (n // 128) * 128)[None, :]
    S.check_split16(got[rows], ref, name, edge=edge)
    return got, ref


@pytest.mark.parametrize("kind,metric", S.DISTMAT_RUNS)
@pytest.mark.parametrize("shape", S.DISTMAT_CASES)
def test_distmat(shape, kind, metric):
    fp16_build_only()
    q, gal = S.distmat_operands(shape, kind)
    run_distmat(q, gal, metric, "split16|distmat_%s|%s|%s %s" % (metric, kind, shape, S.distmat_form(shape[0], shape[1], 3 * shape[2])), kind)


def test_distmat_shapes_reach_every_form(monkeypatch):
    """The streaming, split-K and tiled forms of distmat_impl are all among the shapes above (split16_ref.distmat_form mirrors the
    dispatch), and the streaming shape forced through the tiled kernel (AGRL_DISTMAT_TILED) holds the same bound."""
    fp16_build_only()
    forms = {s: S.distmat_form(s[0], s[1], 3 * s[2]) for s in S.DISTMAT_CASES}
    assert set(forms.values()) == {"stream", "splitk", "tiled"}, forms
    shape = [s for s, f in forms.items() if f == "stream"][0]
    q, gal = S.distmat_operands(shape, "coherent_lo")
    run_distmat(q, gal, "euclidean", "split16|distmat_euclidean|coherent_lo|%s stream" % (shape,), "coherent_lo")
    monkeypatch.setenv("AGRL_DISTMAT_TILED", "1")
    _hip.reload_options()
    run_distmat(q, gal, "euclidean", "split16|distmat_euclidean|coherent_lo|%s forced tiled" % (shape,), "coherent_lo")


def test_distmat_near_copies():
    """Euclidean cancellation: gallery rows 0..7 are query rows with 2^-12-relative noise, rows 8 and 9 exact copies. The bound is in
    mag, so it stays meaningful: a copy's distance is held to the bound itself, ~1e-5 of |q|^2, not to something small against max |ref|."""
    fp16_build_only()
    q, gal = S.near_copies_operands()
    got, ref = run_distmat(q, gal, "euclidean", "split16|distmat_euclidean|near_copies|(40, 64, 256)", "near_copies")
    exact, mag, n_acc, slack = ref
    bound = n_acc * U32 * mag + slack
    for i in (8, 9):
        print("copy %d: d = %.3e, float64 of the given operands %.3e, bound %.3e, |q|^2 %.3e" % (i, float(got[i, i]), float(exact[i, i]),
                                                                                             float(bound[i, i]), float((q[i] ** 2).sum())))
        assert abs(float(got[i, i]) - float(exact[i, i])) <= float(bound[i, i]) and float(bound[i, i]) < 1e-4 * float(mag[i, i])
    for i in range(8):
        assert abs(float(got[i, i]) - float(exact[i, i])) <= float(bound[i, i])


# ---- NaN propagation ----------------------------------------------------------------------------------------------------------------
def nan_reach(N, H, W, at):
    import torch.nn.functional as F
    hit = torch.zeros((N, 1, H, W))
    hit[at[0], 0, at[1], at[2]] = 1
    return (F.conv2d(hit, torch.ones((1, 1, 3, 3)), padding=1) > 0).permute(0, 2, 3, 1)      # (N, H, W, 1)


def test_nan_reaches_exactly_its_receptive_field_inloop():
    """One NaN activation through the in-loop 3x3 conv: NaN in every channel of the nine pixels that read it, every other output equal
    bit for bit to the run without it (ReLU keeps the NaN)."""
    from torchreid import hip_ops as ops
    case = (2, 9, 5, 32, 96, 3, 1, False)
    x, w, b, _, pad = S.inloop_operands(case, "plain")
    wp, bd = ops.split16_inloop_weights(w.to(DEV)), b.to(DEV)
    bad = x.clone()
    bad[1, 4, 2, 7] = float("nan")
    xd, bad_d = x.to(DEV), bad.to(DEV)
    clean = twice(lambda: ops.conv_bn_act(xd, wp, bd, 1, pad, True))
    got = twice_with_nans(lambda: ops.conv_bn_act(bad_d, wp, bd, 1, pad, True))
    reach = nan_reach(2, 9, 5, (1, 4, 2)).expand(2, 9, 5, 96)
    assert torch.equal(torch.isnan(got).cpu(), reach) and not bool(torch.isnan(clean).any())
    assert torch.equal(got.cpu()[~reach], clean.cpu()[~reach])


def test_nan_reaches_exactly_its_receptive_field_planes():
    """The same through the plane 3x3 conv: both result planes are NaN where the NaN reaches, the rest is bit-identical."""
    from torchreid import hip_ops as ops
    fp16_build_only()
    case = (1, 16, 8, 128, 256)
    x, w, b = S.conv3_operands(case, "plain")
    w3, unscale = ops.split16_plane_weights(w.to(DEV))
    pk, bd = ops.conv3x3_pack(w3), b.to(DEV)
    bad = x.clone()
    bad[0, 15, 0, 100] = float("nan")      # a corner: the window is cut by two borders
    x3 = twice(lambda: ops.to_split16_planes(x.to(DEV))).to(DEV)
    bad3 = twice_with_nans(lambda: ops.to_split16_planes(bad.to(DEV))).to(DEV)
    clean = twice(lambda: ops.conv3x3_split16(x3, pk, unscale, bd, 256))
    got = twice_with_nans(lambda: ops.conv3x3_split16(bad3, pk, unscale, bd, 256))
    reach = nan_reach(1, 16, 8, (0, 15, 0)).expand(1, 16, 8, 768)
    assert torch.equal(torch.isnan(got).cpu(), reach) and not bool(torch.isnan(clean).any())
    assert torch.equal(got.cpu()[~reach], clean.cpu()[~reach])
