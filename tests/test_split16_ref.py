"""CPU proof that tests/test_gpu_split16_bounds.py can fail: the split-fp16 recipe emulated in torch (split16_ref.emulate_gemm) is
inside the bound of split16_ref on EVERY element at the GPU file's shapes and operand kinds, each defect of the recipe
((a) xh wl dropped, (b) xl wh dropped, (c) hi truncated, (d) plane lo without its 2^11, (e) weights not pre-scaled, (f) a 128-channel
slab reading hi for lo) puts elements outside it, and the bound's slack is capped against the magnitude so that it cannot grow vacuous.

Every defect is tried on every shape and kind. A missing cross term of random sign grows like sqrt(K) against a chain allowance that
grows like K, so at the deepest shapes only the coherent_lo kind shows it: those (form, defect, kind, shape) cases are listed in EXEMPT
with their reason, coherent_lo is never among them, and what no operands could show is listed in DOES_NOT_APPLY."""
import pytest
import torch

import split16_ref as S
from bounds import U32

F32 = torch.float32

# Every defect is tried on EVERY shape and kind. (form, defect, kind) -> (shapes, or None for every shape of the form; reason): the pairs
# that cannot show. coherent_lo is never among them: it is caught at every shape (expect_caught asserts that no entry names it).
RANDOM_SIGN = ("a missing cross term (or a lost low half) of random sign adds up like sqrt(K) while the chain's allowance, 3 ceil(K / 16) + 3 "
               "roundings of mag, grows like K: from K ~ 1000 on the sum is inside the allowance")
DEEP_INLOOP = [(2, 16, 8, 128, 128, 3, 2, False), (1, 4, 4, 2048, 128, 1, 1, False)]          # K = 1152, 2048
DEEP_POOL = [(1, 2048, 256, (4, 2, 1), True)]
POOLED = "; the pooled sum over up to 128 pixels averages such errors once more while its chain grows by the bin's pixels"
DEEP_DISTMAT = [(130, 257, 2048)]
EXEMPT = {
    ("inloop", "a", "tiny"): (DEEP_INLOOP, RANDOM_SIGN),
    ("inloop", "b", "tiny"): (DEEP_INLOOP, RANDOM_SIGN + "; activations below 2^-8 have low halves of a few units of 2^-24 at most"),
    ("plane_conv3x3", "a", "tiny"): ([(3, 16, 8, 256, 256)], RANDOM_SIGN + " (K = 2304)"),
    ("plane_conv3x3", "b", "tiny"): ([(3, 16, 8, 256, 256)], RANDOM_SIGN + " (K = 2304)"),
    ("plane_pool", "a", "plain"): (DEEP_POOL, RANDOM_SIGN + POOLED),
    ("plane_pool", "a", "small_rows"): (DEEP_POOL, RANDOM_SIGN + POOLED),
    ("plane_pool", "b", "plain"): (DEEP_POOL + [(1, 256, 256, (1,), False)], RANDOM_SIGN + POOLED),
    ("plane_pool", "b", "small_rows"): (DEEP_POOL + [(1, 256, 256, (1,), False)], RANDOM_SIGN + POOLED),
    ("distmat_euclidean", "a", "plain"): (DEEP_DISTMAT, RANDOM_SIGN),
    ("distmat_euclidean", "b", "plain"): (DEEP_DISTMAT, RANDOM_SIGN),
    ("distmat_euclidean", "e", "plain"): (None, "features of order one: a gallery row's low halves lose 2^-25 absolute, random in sign, with or without the "
                                                "pre-scale -- inside the chain's allowance at every D"),
    ("distmat_cosine", "a", "plain"): (DEEP_DISTMAT, RANDOM_SIGN),
    ("distmat_cosine", "b", "plain"): (DEEP_DISTMAT, RANDOM_SIGN),
    ("distmat_cosine", "f", "plain"): (DEEP_DISTMAT, "one slab of sixteen, of random sign after the normalisation"),
}
# (form, defect[, shape]) -> reason: a defect that is no defect of that form, or that no operands whatever could show there
DOES_NOT_APPLY = {
    ("distmat_cosine", "e"): "the host scales UNIT rows by a fixed 2^13: entries are ~ D^-1/2, and what an un-scaled row loses, 2^-25 absolute per "
                             "entry, is below 2^-24 of a distance of order one at every D",
    ("plane_pool", "f", (1, 2048, 256, (4, 2, 1), True)):
        "one slab of sixteen is at most 2^-11 / 16 = 2^-15 of the products; the chain of K = 2048 and the 128 pixels of the whole-frame bin allow "
        "(387 + 128) 2^-24 = 2^-15 of mag, which the residual makes 1.5 x the products: inside the bound whatever the operands",
    ("distmat_euclidean", "f", (130, 257, 2048)):
        "one slab of sixteen is at most 2^-11 / 16 = 2^-15 of the dot product, so 2^-14 of it in the distance; the chain allows 395 2^-24 = 2^-15.4 of "
        "mag = |q|^2 + |g|^2 + 2 |q||g| >= 4 x the dot product: 0.63 of the bound at the very best, whatever the operands",
}


def expect_caught(fn, form, defect, kind, shape, name):
    """Every defect is tried on EVERY shape; what is not listed in EXEMPT for this very shape has to leave the bound."""
    if (form, defect) in DOES_NOT_APPLY or (form, defect, shape) in DOES_NOT_APPLY:
        return
    ex = EXEMPT.get((form, defect, kind))
    if ex is not None and (ex[0] is None or shape in ex[0]):
        assert kind != "coherent_lo"
        return
    import os
    if os.environ.get("SPLIT16_EXPLORE"):
        try:
            fn()
            print("ESCAPE", form, defect, kind, shape)
        except AssertionError:
            pass
        return
    with pytest.raises(AssertionError):
        fn()
    print("caught  (%s) %-45s %-12s %s" % (defect, S.DEFECT_NAMES[defect], kind, name))


def cap(ref, kind, name):
    """The bound is not vacuous: slack <= 16 2^-24 mag (C_SPLIT16 is 8 of the 16); tiny: the absolute terms stay below the smallest output."""
    exact, mag, _, slack = ref
    if kind == "tiny":
        nz = exact.abs()[exact != 0]
        assert nz.numel() and float(ref.abs_slack.max()) < float(nz.min()), (name, float(ref.abs_slack.max()), float(nz.min()))
    else:
        worst = float((slack / mag.clamp(min=1e-300)).max())
        assert worst <= 16 * U32, (name, worst / U32)


# ---- the split and its constant -----------------------------------------------------------------------------------------------------
def test_split16_constant_holds_and_is_approached():
    """C_SPLIT16 and A_LO against the recipe on single products over random and edge operands, in float64."""
    g = torch.Generator().manual_seed(0)
    n = 1 << 20
    mant = torch.randint(0, 1 << 23, (2, n), generator=g, dtype=torch.int32)
    expo = torch.randint(127 - 24, 127 + 14, (2, n), generator=g, dtype=torch.int32)
    v = ((expo << 23) | mant).view(torch.float32)
    x, W = v[0], v[1].clamp(max=2.0 ** 14 - 1)
    (xh, xl), (Wh, Wl) = S.split16(x), S.split16(W)
    ax, aW = S.pair_abs(x), S.pair_abs(W)
    ex = (x.double() - xh.double() - xl.double()).abs()
    assert bool((ex <= 2.0 ** -23 * x.double().abs() + ax).all())
    assert bool((xl.double().abs() <= 2.0 ** -11 * x.double().abs() + ax).all())
    got = xl.double() * Wh.double() + xh.double() * Wl.double() + xh.double() * Wh.double()
    err = (x.double() * W.double() - got).abs()
    bound = S.C_SPLIT16 * (x.double() * W.double()).abs() + S.ABS_FACTOR * (ax * W.double().abs() + aW * x.double().abs()) + 2 * ax * aW
    assert bool((err <= bound).all())
    normal = (ax == 0) & (aW == 0)
    rel = (err / (x.double() * W.double()).abs())[normal]
    assert float(rel.max()) >= S.C_SPLIT16 / 4, float(rel.max())
    # the planes: hi + lo 2^-11 to 2^-22 relative, 2^-36 absolute, and canonical; a truncated high half is not
    hi, ls = S.split16(x, 2.0 ** 11)
    assert bool(((S.planes_value(hi, ls) - x.double()).abs() <= S.PLANE_REL * x.double().abs() + S.PLANE_ABS).all())
    S.canonical_halves(hi, ls * 2.0 ** -11)
    th, tl = S.split16(x, trunc=True)
    assert bool((th.abs() <= x.abs()).all()) and bool((th != S.rne16(x)).any())
    with pytest.raises(AssertionError):
        S.canonical_halves(th, tl)


# ---- in-loop conv -------------------------------------------------------------------------------------------------------------------
INLOOP_DEFECTS = ("a", "b", "c", "e")


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("case", S.INLOOP_CASES)
def test_inloop_conv(case, kind):
    N, H, W, Cin, Cout, R, stride, with_res = case
    x, w, b, res, pad = S.inloop_operands(case, kind)
    ref, _, _ = S.inloop_conv_ref(x, w, b, stride, pad, res, relu=True)
    a = S.patches(x, R, stride, pad)
    r2 = None if res is None else res.reshape(-1, Cout)
    name = "in-loop conv %s %s" % (case, kind)

    def run(defects=(), out="f32"):
        e = S.emulate_gemm(a, w.view(Cout, -1), b, r2, True, defects=defects, out=out)
        return S.check_split16(e["v"], ref, name + " " + out + " " + "".join(defects), presplit_out=out == "presplit", hi=e["hi"], lo=e["lo"])

    run()
    run(out="presplit")       # the stored halves hold the fp32 result to 22 bits and are canonical
    cap(ref, kind, name)
    for d in INLOOP_DEFECTS:
        if d == "c" and with_res:
            continue          # a pre-split output takes no residual
        expect_caught(lambda: run((d,), "presplit" if d == "c" else "f32"), "inloop", d, kind, case, name)


# ---- two-source first block ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.DUAL_KINDS)
@pytest.mark.parametrize("case", S.DUAL_CASES)
def test_dual_inloop(case, kind):
    N, H, W, K1, K2, Cout, stride = case
    x, x2, w, b = S.dual_operands(case, kind)
    ref = S.dual_inloop_ref(x, x2, w, b, stride)
    a = torch.cat([x[:, ::stride, ::stride].reshape(-1, K1), x2.reshape(-1, K2)], 1)
    name = "dual in-loop %s %s" % (case, kind)

    def run(defects=(), out="f32"):
        e = S.emulate_gemm(a, w, b, None, True, defects=defects, out=out)
        return S.check_split16(e["v"], ref, name + " " + out, plane_out=out == "planes", hi=e["hi"], lo=e["lo"])

    run()
    run(out="planes")
    cap(ref, kind, name)
    for d in ("a", "b", "c", "d", "e"):
        expect_caught(lambda: run((d,), "planes" if d in "cd" else "f32"), "dual_inloop", d, kind, case, name)


# ---- plane GEMMs --------------------------------------------------------------------------------------------------------------------
def plane_emulated(xs, w, b, res, defects=(), pool=None):
    e = S.emulate_gemm(torch.cat(xs, 1), w, b, res, True, planes=True, defects=defects, out="planes", pool=pool)
    off, xvs = 0, []
    for t in xs:
        xvs.append(e["xv"][:, off:off + t.shape[1]])
        off += t.shape[1]
    return e, xvs


@pytest.mark.parametrize("kind", S.PLANE_KINDS)
@pytest.mark.parametrize("case", S.PLANE_CASES)
def test_plane_gemm(case, kind):
    M, K, Cout, form = case
    xs, w, b, res = S.plane_operands(M, K, Cout, kind, form == "res")
    e, xvs = plane_emulated(xs, w, b, res)
    ref = S.plane_gemm_ref(xvs, w, b, e["rv"])
    name = "plane gemm %s %s" % (case, kind)
    S.check_split16(e["v"], ref, name, plane_out=True, hi=e["hi"], lo=e["lo"])
    cap(ref, kind, name)
    for d in S.DEFECTS:
        def run():
            bad, _ = plane_emulated(xs, w, b, res, (d,))
            S.check_split16(bad["v"], ref, name + d, plane_out=True, hi=bad["hi"], lo=bad["lo"])
        expect_caught(run, "plane_gemm", d, kind, case, name)


@pytest.mark.parametrize("kind", S.PLANE_KINDS)
@pytest.mark.parametrize("case", S.POOL_CASES)
def test_plane_pool(case, kind):
    N, K, Cout, splits, mean = case
    xs, w, b, res = S.plane_operands(N * 128, K, Cout, kind, True, seed=1)
    pool = (splits, mean, N, 16, 8)
    e, xvs = plane_emulated(xs, w, b, res, pool=pool)
    ref = S.plane_pool_ref(xvs[0], w, b, e["rv"], splits, mean, N)
    name = "plane pool %s %s" % (case, kind)
    S.check_split16(e["v"], ref, name)
    cap(ref, kind, name)
    for d in ("a", "b", "e", "f"):
        def run():
            bad, _ = plane_emulated(xs, w, b, res, (d,), pool=pool)
            S.check_split16(bad["v"], ref, name + d)
        expect_caught(run, "plane_pool", d, kind, (N, K, Cout, tuple(splits), mean), name)


@pytest.mark.parametrize("kind", S.CONV3_KINDS)
@pytest.mark.parametrize("case", S.CONV3_CASES)
def test_plane_conv3x3(case, kind):
    N, H, W, Cin, Cout = case
    x, w, b = S.conv3_operands(case, kind)
    xh, xls = S.split16(x, 2.0 ** 11)
    ref, _, _ = S.plane_conv3x3_ref(S.planes_value(xh, xls), w, b)
    a = S.patches(x, 3, 1, 1)
    name = "plane conv3x3 %s %s" % (case, kind)

    def run(defects=()):
        e = S.emulate_gemm(a, w.view(Cout, -1), b, None, True, planes=True, defects=defects, out="planes")
        return S.check_split16(e["v"], ref, name + "".join(defects), plane_out=True, hi=e["hi"], lo=e["lo"])

    run()
    cap(ref, kind, name)
    for d in ("a", "b", "c", "d", "e"):
        expect_caught(lambda: run((d,)), "plane_conv3x3", d, kind, case, name)


# ---- stem ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.STEM_CASES)
def test_stem(shape):
    import torch.nn.functional as F
    N, H, W = shape
    x, w, b = S.stem_operands(shape)
    ref = S.stem_ref(x, w, b)
    a = S.patches(x.permute(0, 2, 3, 1).contiguous(), 7, 2, 3)
    CH, CW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    name = "stem %s" % (shape,)

    def run(defects=()):
        e = S.emulate_gemm(a, w.view(64, -1), b, None, True, defects=defects)
        v = F.max_pool2d(e["v"].view(N, CH, CW, 64).permute(0, 3, 1, 2), 3, 2, 1)
        return S.check_split16(v, ref, name + "".join(defects))

    run()
    cap(ref, "coherent_lo", name)
    for d in ("a", "b", "e"):
        expect_caught(lambda: run((d,)), "stem", d, "coherent_lo", shape, name)


# ---- distance matrix ----------------------------------------------------------------------------------------------------------------
def distmat_emulated(q, gal, metric, defects=()):
    """hip_distmat_device(..., "fp16x3") on the CPU: fp32 norms / normalised rows, query planes, pre-scaled gallery triples, fp32 epilogue."""
    if metric == "cosine":
        q, gal = (t / t.norm(dim=1, keepdim=True).clamp(min=1e-12) for t in (q, gal))
    qn, gn = (q * q).sum(1), (gal * gal).sum(1)
    e = S.emulate_gemm(q, gal, torch.zeros(gal.shape[0]), planes=True, defects=defects, k=13 if metric == "cosine" else None)
    dot = e["v"].float()
    got = (qn[:, None] + gn[None, :]) - 2 * dot if metric == "euclidean" else 1 - dot
    return got, S.distmat_ref(e["xv"], gal, metric, qn, gn)


@pytest.mark.parametrize("kind,metric", S.DISTMAT_RUNS)
@pytest.mark.parametrize("shape", S.DISTMAT_CASES)
def test_distmat(shape, kind, metric):
    q, gal = S.distmat_operands(shape, kind)
    got, ref = distmat_emulated(q, gal, metric)
    name = "distmat %s %s %s" % (shape, kind, metric)
    S.check_split16(got, ref, name)
    cap(ref, kind, name)
    form = "distmat_" + metric
    for d in ("a", "b", "e", "f"):
        expect_caught(lambda: S.check_split16(distmat_emulated(q, gal, metric, (d,))[0], ref, name + d), form, d, kind, shape, name)


def test_distmat_near_copies_keep_a_meaningful_bound():
    """Euclidean cancellation: the bound is in mag, so an exact copy's distance is held to ~1e-5 of |q|^2, not to max |ref|."""
    q, gal = S.near_copies_operands()
    got, ref = distmat_emulated(q, gal, "euclidean")
    S.check_split16(got, ref, "distmat near copies")
    exact, mag, n_acc, slack = ref
    bound = n_acc * U32 * mag + slack
    for i in (8, 9):
        assert abs(float(got[i, i])) <= float(bound[i, i]) + abs(float(exact[i, i])) and float(bound[i, i]) < 1e-4 * float(mag[i, i])
    with pytest.raises(AssertionError):
        S.check_split16(distmat_emulated(q, gal, "euclidean", ("a",))[0], ref, "distmat near copies, (a)")


def test_distmat_forms_are_all_reached():
    forms = {s: S.distmat_form(s[0], s[1], 3 * s[2]) for s in S.DISTMAT_CASES}
    assert set(forms.values()) == {"stream", "splitk", "tiled"}, forms


# ---- graph_ref.linear_mix_ref borrows this constant ---------------------------------------------------------------------------------
def test_linear_mix_ref_uses_the_fp16_constant():
    import graph_ref as GR
    g = torch.Generator().manual_seed(3)
    P, W = S.activations("coherent_lo", (40, 64), g), S.weights("coherent_lo", 32, 64, g)[0]
    f = torch.randn((40, 32), generator=g)
    scale, shift = 0.8 + 0.4 * torch.rand(32, generator=g), 0.1 * torch.randn(32, generator=g) * float(W.abs().mean()) * 64
    exact, mag, n_acc, slack = GR.linear_mix_ref(P, W, f * 0, scale, shift, 0.0, 1.0, 0.1, "fp16x3")
    amag = P.double().abs() @ W.double().abs().t()
    assert float((slack / (scale.double().abs() * amag)).max()) < 2.0 ** -20       # 2^-21 and the absolute terms, not bf16's 2^-13

    def run(defects=()):
        acc = S.emulate_gemm(P, W, torch.zeros(32), defects=defects)["v"].float()
        pre = acc * scale + shift
        from bounds import check_rounded
        check_rounded(torch.where(pre > 0, pre, pre * 0.1), exact, mag, n_acc, F32, slack=slack, name="linear mix fp16x3")

    run()
    for d in ("a", "b"):
        with pytest.raises(AssertionError):
            run((d,))
