"""The register-pool form of the 16-bit stem (csrc/stem_mfma.hip, stem_regpool_kernel; AGRL_STEM_REGPOOL): the 3x3/2 maximum is taken on
the fp32 accumulators, then + bias, ReLU and one rounding per pooled value. a -> round16(relu(a + b)) is non-decreasing, so on finite inputs
the outputs are those of the conv-tile kernel (AGRL_STEM_REGPOOL=0) BIT FOR BIT; every case launches both and also holds the result to
the element-by-element fp64 bound of the rounded-operand reference (bounds.check_rounded, as test_gpu_kernels.check_stem).

The form takes frames whose pooled row is 17..32 wide (W 65..128), any height; a tile is 8 pooled rows x the whole width, four waves of
two pooled rows each, two 16-column groups per row. Shapes below: the smallest it takes, the bench frame (both groups full: the
lane 15 -> lane 0 hand-over between them), 9 frames (one XCD owns two), odd conv heights / widths (conv row CH and conv column CW enter
no maximum), a second group that is partly empty, and a launch of 1040 tiles over the 512 persistent workgroups (some walk three)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from bounds import check_rounded, n_acc_for, poisoned_outputs
from lp16 import LP_DTYPE
from torchreid import _hip

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = "AGRL_STEM_REGPOOL"


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp(min=1e-30)).item()


def check_stem(out_nhwc, x, w, b, out_dtype, n_acc, name):
    """maxpool3x3/2(ReLU(conv7x7/2(x, w) + b)) in float64 on the operands the kernel multiplies, then one RNE rounding; the bound of a
    max is the largest bound in its window (test_gpu_kernels.check_stem)."""
    x64, w64 = x.double(), w.double()
    exact = F.max_pool2d(F.relu(F.conv2d(x64, w64, bias=b.double(), stride=2, padding=3)), 3, 2, 1)
    mag = F.max_pool2d(F.conv2d(x64.abs(), w64.abs(), bias=b.double().abs(), stride=2, padding=3), 3, 2, 1)
    return check_rounded(out_nhwc.permute(0, 3, 1, 2), exact, mag, n_acc, out_dtype, name=name)


def both_forms(monkeypatch, run):
    """run() with the option unset (the register-pool form where it applies) and with AGRL_STEM_REGPOOL=0 (the conv-tile kernel)."""
    monkeypatch.delenv(OPT, raising=False)
    _hip.reload_options()
    new = run()
    torch.cuda.synchronize()
    monkeypatch.setenv(OPT, "0")
    _hip.reload_options()
    try:
        old = run()
        torch.cuda.synchronize()
    finally:
        monkeypatch.delenv(OPT)
        _hip.reload_options()
    return new, old


def operands(seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((64, 3, 7, 7), generator=g) * 0.1
    b = torch.randn((64,), generator=g) * 0.1
    return g, w, b


SHAPES = [
    (1, 7, 65),       # the smallest: conv 4 x 33, pooled 2 x 17 -- one tile, one wave with rows, group 1 holds one column, odd CW
    (2, 256, 128),    # the bench frame: pooled 64 x 32, both groups full
    (9, 64, 72),      # nine frames: frame 8 shares XCD 0 with frame 0; pooled width 18
    (1, 61, 125),     # odd conv map 31 x 63: the last pooled row's window has two conv rows, the last column's two conv columns
    (3, 45, 97),      # conv 23 x 49, pooled 12 x 25: a ragged second tile (4 of 8 rows), group 1 partly empty
    (520, 39, 65),    # 2 tiles per frame (8 + 2 rows), 1040 tiles on 512 persistent workgroups: three tiles for some, ragged last
]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_regpool_equals_conv_tile_kernel_and_fp64_bound(shape, monkeypatch):
    from torchreid import hip_ops as ops
    N, H, W = shape
    g, w, b = operands(N + H + W)
    x = torch.randn((N, 3, H, W), generator=g)
    xr, wr = x.to(LP_DTYPE).float(), w.to(LP_DTYPE).float()
    ref = F.max_pool2d(F.relu(F.conv2d(xr, wr, bias=b, stride=2, padding=3)), 3, 2, 1)
    wpk = ops.pack_stem_weights_lp16(w.permute(0, 2, 3, 1).contiguous().to(DEV))
    dx, db = x.to(DEV), b.to(DEV)

    def run():
        with poisoned_outputs():
            return ops.stem_lp16(dx, wpk, db)

    new, old = both_forms(monkeypatch, run)
    again = ops.stem_lp16(dx, wpk, db)   # option unset again
    torch.cuda.synchronize()
    e = rel_err(new.float().permute(0, 3, 1, 2), ref)
    print("stem regpool", shape, "rel err %.3e" % e, "differ from the conv-tile kernel: %d of %d" % (int((new != old).sum()), new.numel()))
    assert e < 5e-3
    assert torch.equal(new, old)
    assert torch.equal(new, again)
    check_stem(new.cpu(), xr, wr, b, LP_DTYPE, n_acc_for(224), "stem regpool %s" % (shape,))


@pytest.mark.gpu
def test_regpool_excludes_positions_outside_the_conv_map(monkeypatch):
    """Positive pixels, negative weights, bias 6: a conv position computed from zero padding (row -1, column -1) has fewer taps than any
    real one and exceeds every real position of its window, so a kernel that lets it into the maximum changes every element of the first
    pooled row and the first pooled column (checked below on the CPU) -- and no other."""
    from torchreid import hip_ops as ops
    N, H, W = 1, 64, 96
    g = torch.Generator().manual_seed(3)
    x = (1 + 0.1 * torch.randn((N, 3, H, W), generator=g).abs()).to(LP_DTYPE).float()
    w = (-0.05 * (1 + 0.1 * torch.randn((64, 3, 7, 7), generator=g).abs())).to(LP_DTYPE).float()
    b = torch.full((64,), 6.0)
    ref = F.max_pool2d(F.relu(F.conv2d(x, w, bias=b, stride=2, padding=3)), 3, 2, 1)
    # the wrong answer: conv positions -1 .. CH, -1 .. CW from zero padding (padding 5), pooled without padding
    wrong = F.max_pool2d(F.relu(F.conv2d(x, w, bias=b, stride=2, padding=5)), 3, 2, 0)[:, :, :ref.shape[2], :ref.shape[3]]
    differs = wrong != ref
    assert differs[:, :, 0, :].all() and differs[:, :, :, 0].all() and not differs[:, :, 1:, 1:].any()
    wpk = ops.pack_stem_weights_lp16(w.permute(0, 2, 3, 1).contiguous().to(DEV))
    dx, db = x.to(DEV), b.to(DEV)

    def run():
        with poisoned_outputs():
            return ops.stem_lp16(dx, wpk, db)

    new, old = both_forms(monkeypatch, run)
    got = new.float().permute(0, 3, 1, 2).cpu()
    print("stem regpool border: first row max |got - ref| %.3e, |got - wrong| %.3e" % (
        float((got - ref)[:, :, 0].abs().max()), float((got - wrong)[:, :, 0].abs().max())))
    assert torch.equal(new, old)
    check_stem(new.cpu(), x, w, b, LP_DTYPE, n_acc_for(224), "stem regpool border")


@pytest.mark.gpu
def test_regpool_nan_reaches_exactly_its_windows(monkeypatch):
    """One NaN pixel: the outputs whose windows it reaches are NaN in both forms (the payload is free), the others equal bit for bit."""
    from torchreid import hip_ops as ops
    N, H, W = 2, 64, 128
    g, w, b = operands(17)
    x = torch.randn((N, 3, H, W), generator=g)
    x[1, 1, 31, 63] = float("nan")     # conv rows 14..17, columns 30..33: on the seam between the two column groups
    wpk = ops.pack_stem_weights_lp16(w.permute(0, 2, 3, 1).contiguous().to(DEV))
    dx, db = x.to(DEV), b.to(DEV)
    new, old = both_forms(monkeypatch, lambda: ops.stem_lp16(dx, wpk, db))
    nan_new, nan_old = torch.isnan(new), torch.isnan(old)
    hit = torch.zeros((N, 1, H, W))
    hit[1, 0, 31, 63] = 1
    reach = F.max_pool2d(F.conv2d(hit, torch.ones((1, 1, 7, 7)), stride=2, padding=3), 3, 2, 1) > 0   # (N,1,PH,PW)
    assert torch.equal(nan_new, nan_old)
    assert torch.equal(nan_new.cpu(), reach.permute(0, 2, 3, 1).expand_as(nan_new))
    assert torch.equal(new[~nan_new], old[~nan_old])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_regpool_u8_frames_equal_the_fp32_launch(layout, monkeypatch):
    """uint8 frames in both layouts through the register-pool form = its fp32 launch on the table-normalised tensor, bit for bit (the
    contract of test_gpu_u8_ingest.test_stem_lp16_u8_equals_its_fp32_launch), and = the conv-tile kernel."""
    from torchreid import hip_ops as ops
    u8 = torch.randint(0, 256, (2, 3, 256, 128), dtype=torch.uint8, generator=torch.Generator().manual_seed(21))
    _, w, b = operands(11)
    wpk = ops.pack_stem_weights_lp16(w.permute(0, 2, 3, 1).contiguous().to(DEV))
    db = b.to(DEV)
    x32 = ops.frames_normalize_reference(u8).to(DEV)
    d = (u8.contiguous() if layout == "nchw" else u8.movedim(-3, -1).contiguous()).to(DEV)

    def run_u8():
        with poisoned_outputs():
            return ops.stem_lp16(d, wpk, db)

    def run_f32():
        with poisoned_outputs():
            return ops.stem_lp16(x32, wpk, db)

    new_u8, old_u8 = both_forms(monkeypatch, run_u8)
    new_f32, old_f32 = both_forms(monkeypatch, run_f32)
    assert torch.isfinite(new_f32).all() and float(new_f32.float().abs().max()) > 0
    assert torch.equal(new_u8, new_f32)
    assert torch.equal(new_u8, old_u8) and torch.equal(new_f32, old_f32)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 37, 29), (3, 64, 64), (2, 40, 129)])
def test_shapes_the_regpool_form_does_not_take(shape, monkeypatch):
    """Pooled rows of at most 16 or more than 32 columns go to the conv-tile kernel whatever the option says."""
    from torchreid import hip_ops as ops
    N, H, W = shape
    g, w, b = operands(N * H + W)
    x = torch.randn((N, 3, H, W), generator=g)
    xr, wr = x.to(LP_DTYPE).float(), w.to(LP_DTYPE).float()
    wpk = ops.pack_stem_weights_lp16(w.permute(0, 2, 3, 1).contiguous().to(DEV))
    dx, db = x.to(DEV), b.to(DEV)

    def run():
        with poisoned_outputs():
            return ops.stem_lp16(dx, wpk, db)

    new, old = both_forms(monkeypatch, run)
    assert torch.equal(new, old)
    check_stem(new.cpu(), xr, wr, b, LP_DTYPE, n_acc_for(224), "stem 16-bit %s" % (shape,))


def test_regpool_adds_no_pack_entry_point():
    """The register-pool form reads pack_stem_weights_lp16's tensor as it is: (64, 240) 16-bit, and the C header declares no weight
    packing for a stem."""
    from torchreid import hip_ops as ops
    w = torch.arange(64 * 7 * 7 * 3, dtype=torch.float32).reshape(64, 7, 7, 3) / 1024
    p = ops.pack_stem_weights_lp16(w)
    assert p.dtype == LP_DTYPE and tuple(p.shape) == (64, 240) and p.is_contiguous()
    r = p.view(64, 30, 8).float()            # 30 sixteen-byte slots a row: 7 filter rows x 4 slots (8 taps x 4 channels), 2 of padding
    assert torch.equal(r[:, :28].reshape(64, 7, 8, 4)[:, :, :7, :3], w.to(LP_DTYPE).float())
    assert float(r[:, 28:].abs().max()) == 0 and float(r[:, :28].reshape(64, 7, 8, 4)[:, :, 7].abs().max()) == 0
    assert float(r[:, :28].reshape(64, 7, 8, 4)[:, :, :, 3].abs().max()) == 0
    with open(os.path.join(ROOT, "include", "agrl_hip.h")) as f:
        names = set(re.findall(r"\bagrl_\w+", f.read()))
    assert not [n for n in names if "pack" in n and "stem" in n]
    assert not [n for n in names if "regpool" in n]
