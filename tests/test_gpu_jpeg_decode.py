"""agrl_jpeg_decode_u8 on the GPU: baseline JPEG frames decoded BITWISE as Pillow decodes them. Every comparison is torch.equal against
the fixture's Pillow pixels (tests/golden/jpeg_decode.npz) inside the valid extents; everything runs under poisoned allocations, and
twice for equal bits. The broken scans are inputs the kernels survive by construction (every index they form is range-checked): their
status must be the restatement's, the rest of the batch exact and the sentinel bands around output and workspace untouched."""
import numpy as np
import pytest
import torch

import dense_stub as DS
import jpeg_cases as J
from bounds import poisoned_outputs
from torchreid import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 4096     # sentinel bytes on either side of the output and of the workspace


def mods():
    from torchreid import device_decode as dd, hip_ops as ops
    return dd, ops


def plan_of(names, damage=None):
    dd, _ = mods()
    frames = [dd.parse_jpeg(J.fixture()[n][0]) for n in names]
    for k, kind in (damage or {}).items():
        frames[k] = J.broken(frames[k], kind)
    return dd.jpeg_batch_plan(frames)


def run(plan, **kw):
    _, ops = mods()
    with poisoned_outputs():
        clip, status = ops.jpeg_decode(plan, device=torch.device(DEV), **kw)
    torch.cuda.synchronize()
    return clip, status


def check(names, what):
    """the batch decoded twice == Pillow's pixels in every valid extent, zeros outside, status 0 -> the device clip"""
    plan = plan_of(names)
    want, sizes = J.container([J.fixture()[n][1] for n in names])
    clip, status = run(plan)
    assert clip.dtype == torch.uint8 and tuple(clip.shape) == want.shape and status.dtype == torch.int32 and np.array_equal(plan.sizes, sizes)
    assert not status.cpu().any(), (what, status.cpu().tolist())
    got = clip.cpu()
    bad = got != torch.from_numpy(want)
    assert not bad.any(), "%s: %d of %d bytes differ from Pillow's, first at (frame, y, x, c) %s = %s" % (
        what, int(bad.sum()), want.size, bad.nonzero()[0].tolist(), names[int(bad.nonzero()[0][0])])
    again, status2 = run(plan)
    assert torch.equal(again, clip) and torch.equal(status2, status)
    return clip


# ---- Pillow's bytes, shape by shape ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", J.SAMPLINGS)
@pytest.mark.parametrize("shape", J.SHAPES, ids=["%dx%d" % s for s in J.SHAPES])
def test_kernel_equals_pillow_fixture(shape, sampling):
    names = J.names(shape, sampling)
    assert names
    if shape == (256, 128):      # four frames: the sampling's own and the three others around it
        names = names + [n for n in J.names(shape) if n not in names]
        assert len(names) == 4
    else:
        assert [n for n in names if "_q30_" in n] and [n for n in names if "_q100_" in n] and [n for n in names if "_opt" in n]
        assert [n for n in names if "_saturated" in n]
    for n in names:              # each alone (its own container), then all of the shape in one launch
        check([n], n)
    check(names, "%dx%d %s" % (shape + (sampling,)))


@pytest.mark.parametrize("sampling", J.SAMPLINGS)
def test_restart_intervals(sampling):
    names = [n for n in J.names(sampling=sampling) if "_rst" in n]
    assert len(names) == 3
    dd, ops = mods()
    assert sorted({dd.parse_jpeg(J.fixture()[n][0]).restart_interval for n in names})[0] == 3
    check(names, "restart intervals, " + sampling)


def mixed_names():
    """everything of the small shapes interleaved: sizes, samplings, tables and restart intervals change from frame to frame"""
    small = [n for n in J.fixture() if not n.startswith("256x128")]
    order = np.random.default_rng(4).permutation(len(small)).tolist()
    return [small[i] for i in order] + ["256x128_420_q75_smooth"]


def banded(nbytes, fill):
    buf = torch.full((BAND + nbytes + BAND,), fill, dtype=torch.uint8, device=DEV)
    return buf, buf[BAND:BAND + nbytes]


def bands_intact(buf, nbytes, fill):
    host = buf.cpu()
    return bool((host[:BAND] == fill).all()) and bool((host[BAND + nbytes:] == fill).all())


def test_one_mixed_batch_in_one_launch_between_sentinels():
    _, ops = mods()
    names = mixed_names()
    plan = plan_of(names)
    assert len(plan.quant) > 4 and len(plan.huff) > 8 and len(set(map(tuple, plan.sizes.tolist()))) >= 6
    want, sizes = J.container([J.fixture()[n][1] for n in names])
    F, Hc, Wc = want.shape[:3]
    obuf, out = banded(want.size, 0xA5)
    need = ops.jpeg_workspace_bytes(plan)
    assert need == plan.ws_blocks * 192
    wbuf, ws = banded(need, 0x3C)
    clip, status = run(plan, out=out.view(F, Hc, Wc, 3), workspace=ws)
    assert clip.data_ptr() == out.data_ptr()
    assert not status.cpu().any() and torch.equal(clip.cpu(), torch.from_numpy(want)), "frame order or content"
    assert bands_intact(obuf, want.size, 0xA5) and bands_intact(wbuf, need, 0x3C)
    first = clip.clone()
    clip2, status2 = run(plan, out=out.view(F, Hc, Wc, 3), workspace=ws)
    assert torch.equal(clip2, first) and not status2.cpu().any()


@pytest.mark.parametrize("name", ["33x47_420_q75_noise_rst3", "33x47_444_q100_noise", "256x128_420_q75_smooth"])
def test_broken_scans_inside_a_good_batch(name):
    """a scan cut at half its length and one with a fixed-seed byte pattern over its middle third, between good frames: the device's
    status is the restatement's, every other frame is still exact, nothing outside the output and the workspace is written"""
    _, ops = mods()
    names = ["17x9_422_q30_noise", name, "16x16_420_q100_noise", name, "33x47_gray_q85_noise_opt", "8x8_444_q30_noise"]
    plan = plan_of(names, damage={1: "cut", 3: "noise"})
    ref_clip, ref_status = ops.jpeg_decode_reference(plan)
    assert ref_status[1] != 0 and ref_status[3] != 0
    want, sizes = J.container([J.fixture()[n][1] for n in names])
    F, Hc, Wc = want.shape[:3]
    obuf, out = banded(want.size, 0xA5)
    need = ops.jpeg_workspace_bytes(plan)
    wbuf, ws = banded(need, 0x3C)
    clip, status = run(plan, out=out.view(F, Hc, Wc, 3), workspace=ws)
    assert status.cpu().tolist() == ref_status.tolist()
    good = [0, 2, 4, 5]
    assert torch.equal(clip.cpu()[good], torch.from_numpy(want)[good])
    assert torch.equal(clip.cpu(), ref_clip)      # the broken frames too: what the coefficients decoded so far give
    assert bands_intact(obuf, want.size, 0xA5) and bands_intact(wbuf, need, 0x3C)
    clip2, status2 = run(plan, out=out.view(F, Hc, Wc, 3), workspace=ws)
    assert torch.equal(clip2.cpu(), ref_clip) and torch.equal(status2, status)


# ---- the C ABI's own checks ----------------------------------------------------------------------------------------------------------
def raw_args(plan, operands, out_t, ws_t, status_t, desc_host=None, **over):
    """the entry point's arguments in order; ``over`` replaces some by name (desc_host: an int32 (F,16) array)"""
    _, ops = mods()
    scans_d, desc_d, quant_d, huff_d = operands
    a = dict(scans=scans_d.data_ptr(), scan_bytes=scans_d.numel(), desc_host=(plan.desc if desc_host is None else desc_host).ctypes.data,
             desc=desc_d.data_ptr(), F=plan.desc.shape[0], quant=quant_d.data_ptr(), NQ=quant_d.shape[0], huff=huff_d.data_ptr(),
             NH=huff_d.shape[0], ws=ws_t.data_ptr(), ws_bytes=ws_t.numel(), out=out_t.data_ptr(), Hc=out_t.shape[1], Wc=out_t.shape[2],
             status=status_t.data_ptr(), stages=ops.JPEG_STAGE_ALL)
    assert set(over) <= set(a), over
    a.update(over)
    return tuple(a.values()) + (_hip.stream_ptr(out_t.device),)


def test_cabi_rejections_write_nothing():
    """Every AGRL_CHECK_ARG of the entry point raises with its message BEFORE any launch: output, workspace and status keep their
    sentinels. The descriptor rows are checked on the host copy."""
    _, ops = mods()
    names = ["17x9_420_q30_noise", "16x16_444_q100_noise", "33x47_gray_q30_noise"]
    plan = plan_of(names)
    operands = ops.jpeg_upload(plan, torch.device(DEV))
    F, (Hc, Wc) = 3, plan.container
    out = torch.full((F, Hc, Wc, 3), 0xA5, dtype=torch.uint8, device=DEV)
    ws = torch.full((ops.jpeg_workspace_bytes(plan),), 0x3C, dtype=torch.uint8, device=DEV)
    status = torch.full((F,), -7, dtype=torch.int32, device=DEV)

    def row(f, col, value):
        d = plan.desc.copy()
        d[f, col] = value
        return d

    cases = [
        (dict(scans=None), "null pointer"), (dict(out=None), "null pointer"), (dict(status=None), "null pointer"), (dict(ws=None), "null pointer"),
        (dict(F=0), "F=0 frames"), (dict(Hc=0), "container 0x"), (dict(Wc=4097), "container %dx4097" % Hc), (dict(stages=0), "stage mask 0"),
        (dict(stages=8), "stage mask 8"), (dict(NQ=0), "bad sizes"), (dict(scans=operands[0].data_ptr() + 1), "misaligned pointer"),
        (dict(ws=ws.data_ptr() + 8, ws_bytes=ws.numel() - 8), "misaligned pointer"),
        (dict(desc_host=row(1, ops.JD_OFF, plan.scans.size)), "descriptor 1 is outside its buffers"),
        (dict(desc_host=row(1, ops.JD_OFF, 4)), "descriptor 1 is outside its buffers"),
        (dict(desc_host=row(2, ops.JD_LEN, plan.desc[2, ops.JD_LEN] + 64)), "descriptor 2 is outside its buffers"),
        (dict(desc_host=row(0, ops.JD_LEN, -1)), "descriptor 0 is outside its buffers"),
        (dict(desc_host=row(2, ops.JD_H, Hc + 1)), "descriptor 2 is outside its buffers"),
        (dict(desc_host=row(0, ops.JD_W, 0)), "descriptor 0 is outside its buffers"),
        (dict(desc_host=row(0, ops.JD_SAMP, 4)), "descriptor 0 is outside its buffers"),
        (dict(desc_host=row(0, ops.JD_RI, -2)), "descriptor 0 is outside its buffers"),
        (dict(desc_host=row(1, ops.JD_Q0 + 2, len(plan.quant))), "descriptor 1 is outside its buffers"),
        (dict(desc_host=row(1, ops.JD_DC0, -1)), "descriptor 1 is outside its buffers"),
        (dict(desc_host=row(1, ops.JD_AC0 + 1, len(plan.huff))), "descriptor 1 is outside its buffers"),
        (dict(desc_host=row(2, ops.JD_WS, plan.desc[2, ops.JD_WS] + 1)), "descriptor 2 is outside its buffers"),
        (dict(desc_host=row(1, ops.JD_WS, 0)), "descriptor 1's workspace slice .* overlaps"),
        (dict(ws_bytes=ws.numel() - 192), "descriptor 2 is outside its buffers"),
        (dict(Hc=Hc - 1), "descriptor 2 is outside its buffers"),
    ]
    for over, message in cases:
        with pytest.raises(_hip.HipKernelError, match=message):
            _hip.call("agrl_jpeg_decode_u8", *raw_args(plan, operands, out, ws, status, **over))
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((ws == 0x3C).all()) and bool((status == -7).all()), "a rejected call wrote"
    assert _hip.lib().agrl_jpeg_decode_workspace(0) == 0 and _hip.lib().agrl_jpeg_decode_workspace(-3) == 0
    # and the same operands, untouched, decode
    _hip.call("agrl_jpeg_decode_u8", *raw_args(plan, operands, out, ws, status))
    torch.cuda.synchronize()
    want, _ = J.container([J.fixture()[n][1] for n in names])
    assert torch.equal(out.cpu(), torch.from_numpy(want)) and not status.cpu().any()
    # the wrapper's own checks
    with pytest.raises(ValueError, match="out must be contiguous uint8"):
        ops.jpeg_decode(plan, out=out[:, :, :-1])
    with pytest.raises(ValueError, match="workspace must be contiguous uint8 of at least"):
        ops.jpeg_decode(plan, out=out, workspace=ws[:-1])


def test_a_device_descriptor_the_host_copy_does_not_match_is_skipped_with_status_5():
    """the kernels check the DEVICE copy of every row again: a row that fails there is skipped -- status 5, its slot zeroed, nothing else
    touched -- and the other frames decode"""
    _, ops = mods()
    names = ["17x9_420_q30_noise", "16x16_444_q100_noise", "33x47_gray_q30_noise"]
    plan = plan_of(names)
    bad = plan.desc.copy()
    bad[1, ops.JD_WS] = 2 ** 23            # far outside the workspace
    operands = ops.jpeg_upload(plan._replace(desc=bad), torch.device(DEV))
    want, _ = J.container([J.fixture()[n][1] for n in names])
    want[1] = 0
    F, (Hc, Wc) = 3, plan.container
    obuf, out = banded(want.size, 0xA5)
    wbuf, ws = banded(ops.jpeg_workspace_bytes(plan), 0x3C)
    status = torch.full((F,), -7, dtype=torch.int32, device=DEV)
    _hip.call("agrl_jpeg_decode_u8", *raw_args(plan, operands, out.view(F, Hc, Wc, 3), ws, status))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, ops.JPEG_ERR_DESC, 0]
    assert torch.equal(out.view(F, Hc, Wc, 3).cpu(), torch.from_numpy(want))
    assert bands_intact(obuf, want.size, 0xA5) and bands_intact(wbuf, ws.numel(), 0x3C)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_decoder_then_resample_equals_pillow_then_resample():
    dd, ops = mods()
    from torchreid.device_transforms import DeviceClipTransform, eval_geometry
    names = ["256x128_420_q75_smooth", "33x47_422_q30_noise", "17x9_444_q100_noise", "256x128_gray_q30_smooth", "48x48_420_q75_smooth_opt_rstrow",
             "33x47_420_q95_noise_rstrow", "16x16_gray_q85_noise_opt", "8x8_420_q30_noise"]
    dec = dd.DeviceJpegDecoder(DEV)
    with poisoned_outputs():
        imgs, sizes = dec.decode([J.fixture()[n][0] for n in names], shape=(2, 4))
        got = DeviceClipTransform(256, 128)(imgs, sizes)
    torch.cuda.synchronize()
    box, want_sizes = J.container([J.fixture()[n][1] for n in names])
    assert imgs.is_cuda and imgs.shape == (2, 4, 256, 128, 3) and np.array_equal(sizes.reshape(-1, 2), want_sizes)
    assert dec.frames == 8 and dec.fallback_frames == 0
    want = ops.clip_resample_reference(torch.from_numpy(box), eval_geometry(want_sizes), (256, 128))
    assert torch.equal(got.view(8, 256, 128, 3).cpu(), want)


def test_decoder_falls_back_for_files_outside_the_subset_and_broken_scans(caplog):
    """one launch for the frames inside the subset; the others come from the host decode, in their slots"""
    import logging
    dd, ops = mods()
    fx = J.fixture()
    rst = fx["33x47_420_q75_noise_rst3"][0]
    at = rst.index(bytes(dd.parse_jpeg(rst).scan))
    renumbered = rst[:at] + rst[at:].replace(b"\xff\xd0", b"\xff\xd3", 1)    # status 4 on the device; libjpeg resynchronises
    decoded = {}

    def host_decode(data):
        decoded[len(decoded)] = data
        return fx["33x47_420_q75_noise_rst3"][1] if data is renumbered else np.full((9, 70, 3), 200, dtype=np.uint8)

    unsupported = fx["17x9_420_q30_noise"][0].replace(b"\xff\xc0", b"\xff\xc2", 1)
    dec = dd.DeviceJpegDecoder(DEV)
    real, dd.pillow_decode = dd.pillow_decode, host_decode
    try:
        with caplog.at_level(logging.WARNING, logger="torchreid.device_decode"), poisoned_outputs():
            imgs, sizes = dec.decode([fx["16x16_444_q30_noise"][0], unsupported, renumbered, fx["8x8_gray_q100_noise"][0]])
    finally:
        dd.pillow_decode = real
    assert list(decoded.values()) == [unsupported, renumbered] and dec.fallback_frames == 2 and "2 of 4 frames took the Pillow fallback" in caplog.text
    assert imgs.shape == (4, 33, 70, 3) and sizes.tolist() == [[16, 16], [9, 70], [33, 47], [8, 8]]
    host = imgs.cpu().numpy()
    assert np.array_equal(host[0, :16, :16], fx["16x16_444_q30_noise"][1]) and (host[1, :9, :70] == 200).all()
    assert np.array_equal(host[2, :33, :47], fx["33x47_420_q75_noise_rst3"][1]) and np.array_equal(host[3, :8, :8], fx["8x8_gray_q100_noise"][1])


TRACKLET_CLIPS = (1, 3, 2, 5, 1)


@pytest.mark.parametrize("prefetch", [True, False], ids=["prefetch", "one_stream"])
def test_packed_extraction_from_jpeg_bytes_equals_the_decoded_frames_route(prefetch):
    """JPEG bytes -> decode_batches -> extract_features_packed(frame_size=...) on the batch-invariant stub == the same tracklets handed
    over as Pillow-decoded frames with their valid extents"""
    from torchreid import evaluation
    fx = J.fixture()
    pool = [n for n in fx if not n.startswith("256x128")]
    S = DS.S
    g = torch.Generator().manual_seed(2)
    encoded, decoded, k = [], [], 0
    for t, n in enumerate(TRACKLET_CLIPS):
        chosen = [[pool[(k + c * S + s) * 5 % len(pool)] for s in range(S)] for c in range(n)]
        k += n * S
        adj = torch.rand((1, n, DS.V, DS.V), generator=g)
        pid, cam = torch.tensor([100 + t]), torch.tensor([t % 3])
        encoded.append(([[[fx[name][0] for name in clip] for clip in chosen]], pid, cam, adj))
        box, sizes = J.container([fx[name][1] for clip in chosen for name in clip])
        full = np.zeros((n * S, 48, 48, 3), dtype=np.uint8)        # one container shape for every item of the extraction
        full[:, :box.shape[1], :box.shape[2]] = box
        decoded.append((torch.from_numpy(full).view(1, n, S, 48, 48, 3), pid, cam, adj, sizes.reshape(1, n, S, 2)))
    model = DS.StubModel().to(DEV)
    want, want_pids, want_cams = evaluation.extract_features_packed(model, decoded, clip_batch=4, frame_size=(16, 8), prefetch=prefetch)
    model.calls = []
    with poisoned_outputs():
        got, pids, cams = evaluation.extract_features_packed(model, evaluation.decode_batches(encoded, torch.device(DEV)), clip_batch=4,
                                                             frame_size=(16, 8), prefetch=prefetch)
    torch.cuda.synchronize()
    assert got.shape == (len(TRACKLET_CLIPS), DS.PIX + DS.ADJ) and torch.equal(got, want)
    assert np.array_equal(pids, want_pids) and np.array_equal(cams, want_cams) and model.calls == DS.expected_calls(TRACKLET_CLIPS, 4)
