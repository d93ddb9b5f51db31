"""agrl_png_decode_u8 on the GPU: 8-bit grey / RGB PNG frames decoded BITWISE as Pillow decodes them. Every comparison is torch.equal
against the restatement (hip_ops.png_decode_reference, run once: png_cases.reference) and the fixture's Pillow pixels
(tests/golden/png_decode.npz); output and status lie between sentinel bands, and everything runs twice for equal bits. The broken
streams are inputs the kernel survives by construction (every index it forms is range-checked): their status must be the restatement's,
their slot zero, the rest of the batch exact and the sentinels untouched."""
import numpy as np
import pytest
import torch

import dense_stub as DS
import jpeg_cases as J
import png_cases as P
from bounds import poisoned_outputs
from torchreid import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 4096     # sentinel bytes on either side of the output and of the status


def mods():
    from torchreid import device_decode as dd, hip_ops as ops
    return dd, ops


def banded(nbytes, fill):
    buf = torch.full((BAND + nbytes + BAND,), fill, dtype=torch.uint8, device=DEV)
    return buf, buf[BAND:BAND + nbytes]


def bands_intact(buf, nbytes, fill):
    host = buf.cpu()
    return bool((host[:BAND] == fill).all()) and bool((host[BAND + nbytes:] == fill).all())


def raw_args(plan, operands, out_t, status_t, desc_host=None, **over):
    """the entry point's arguments in order; ``over`` replaces some by name (desc_host: an int32 (F,8) array)"""
    _, ops = mods()
    streams_d, desc_d = operands
    a = dict(streams=streams_d.data_ptr(), stream_bytes=streams_d.numel(), desc_host=(plan.desc if desc_host is None else desc_host).ctypes.data,
             desc=desc_d.data_ptr(), F=plan.desc.shape[0], out=out_t.data_ptr(), Hc=out_t.shape[1], Wc=out_t.shape[2],
             status=status_t.data_ptr(), stages=ops.PNG_STAGE_ALL)
    assert set(over) <= set(a), over
    a.update(over)
    return tuple(a.values()) + (_hip.stream_ptr(out_t.device),)


def run_between_sentinels(plan):
    """the plan decoded through the C ABI into banded output and status, twice -> (clip, status) on the host"""
    _, ops = mods()
    F, (Hc, Wc) = plan.desc.shape[0], plan.container
    operands = ops.png_upload(plan, torch.device(DEV))
    results = []
    for _ in range(2):
        obuf, out = banded(F * Hc * Wc * 3, 0xA5)
        sbuf, st = banded(4 * F, 0x3C)
        status = st.view(torch.int32)
        _hip.call("agrl_png_decode_u8", *raw_args(plan, operands, out.view(F, Hc, Wc, 3), status))
        torch.cuda.synchronize()
        assert bands_intact(obuf, F * Hc * Wc * 3, 0xA5) and bands_intact(sbuf, 4 * F, 0x3C), "a byte outside the output or the status was written"
        results.append((out.view(F, Hc, Wc, 3).cpu(), status.cpu()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), "two runs differ"
    return results[0]


# ---- Pillow's bytes ----------------------------------------------------------------------------------------------------------------------
def test_every_decodable_case_in_one_batch_equals_the_restatement_and_pillow():
    order, plan, ref_clip, ref_status, _ = P.reference()
    want, _ = P.container([P.fixture()[n][1] for n in order])
    clip, status = run_between_sentinels(plan)
    assert status.tolist() == ref_status.tolist() == [0] * len(order)
    bad = clip != ref_clip
    assert not bad.any(), "%d bytes differ from the restatement's, first at (frame, y, x, c) %s = %s" % (
        int(bad.sum()), bad.nonzero()[0].tolist(), order[int(bad.nonzero()[0][0])])
    assert torch.equal(clip, torch.from_numpy(want))      # Pillow's pixels in every valid extent, zeros in the rest of every slot


@pytest.mark.parametrize("shape", P.SHAPES, ids=["%dx%d" % s for s in P.SHAPES])
def test_each_shape_in_its_own_container(shape):
    """the container is exactly the frames' size: no slot remainder, row strides of 3, 21, 27 and 384 bytes"""
    dd, ops = mods()
    names = P.names(shape)
    assert [n for n in names if "_grey_" in n] and [n for n in names if "_rgb_" in n]
    plan = dd.png_batch_plan([dd.parse_png(P.fixture()[n][0]) for n in names])
    assert plan.container == shape
    clip, status = run_between_sentinels(plan)
    assert not status.any() and torch.equal(clip, torch.from_numpy(np.stack([P.fixture()[n][1] for n in names])))
    with poisoned_outputs():                               # and through the wrapper, which allocates for itself
        clip2, status2 = ops.png_decode(plan, device=torch.device(DEV))
    torch.cuda.synchronize()
    assert torch.equal(clip2.cpu(), clip) and not status2.cpu().any()


@pytest.mark.parametrize("name", sorted(P.broken()))
def test_broken_stream_between_good_frames(name):
    plan, ref_clip, ref_status, want = P.broken_batch(name)
    assert ref_status[1] != 0
    clip, status = run_between_sentinels(plan)
    assert status.tolist() == ref_status.tolist()
    assert torch.equal(clip, ref_clip) and torch.equal(clip, torch.from_numpy(want))     # good frames exact, the broken slot zero


# ---- the C ABI's own checks ----------------------------------------------------------------------------------------------------------
def small_plan():
    dd, _ = mods()
    names = ["7x9_rgb_smooth_f4", "1x7_grey_smooth_f3", "7x1_rgb_smooth_mixed_fixed"]
    return names, dd.png_batch_plan([dd.parse_png(P.fixture()[n][0]) for n in names])


def test_cabi_rejections_write_nothing():
    """every AGRL_CHECK_ARG of the entry point raises with its message BEFORE the launch: output and status keep their sentinels. The
    descriptor rows are checked on the host copy."""
    _, ops = mods()
    names, plan = small_plan()
    operands = ops.png_upload(plan, torch.device(DEV))
    F, (Hc, Wc) = 3, plan.container
    out = torch.full((F, Hc, Wc, 3), 0xA5, dtype=torch.uint8, device=DEV)
    status = torch.full((F,), -7, dtype=torch.int32, device=DEV)

    def row(f, col, value):
        d = plan.desc.copy()
        d[f, col] = value
        return d

    cases = [
        (dict(streams=None), "null pointer"), (dict(out=None), "null pointer"), (dict(status=None), "null pointer"), (dict(F=0), "F=0 frames"),
        (dict(Hc=0), "container 0x"), (dict(Wc=4097), "container %dx4097" % Hc), (dict(stages=0), "stage mask 0"), (dict(stages=8), "stage mask 8"),
        (dict(stages=6), "stage mask 6"), (dict(stream_bytes=0), "bad sizes"), (dict(streams=operands[0].data_ptr() + 1), "misaligned pointer"),
        (dict(desc_host=row(1, ops.PD_OFF, plan.streams.size)), "descriptor 1 is outside its buffers"),
        (dict(desc_host=row(1, ops.PD_OFF, 4)), "descriptor 1 is outside its buffers"),
        (dict(desc_host=row(2, ops.PD_LEN, plan.desc[2, ops.PD_LEN] + 64)), "descriptor 2 is outside its buffers"),
        (dict(desc_host=row(0, ops.PD_LEN, -1)), "descriptor 0 is outside its buffers"),
        (dict(desc_host=row(0, ops.PD_H, Hc + 1)), "descriptor 0 is outside its buffers"),
        (dict(desc_host=row(0, ops.PD_W, 0)), "descriptor 0 is outside its buffers"),
        (dict(desc_host=row(1, ops.PD_CH, 2)), "descriptor 1 is outside its buffers"),
        (dict(desc_host=row(1, ops.PD_CH, 4)), "descriptor 1 is outside its buffers"),
        (dict(Hc=Hc - 1), "descriptor 0 is outside its buffers"),
        (dict(stream_bytes=plan.streams.size - 32), "descriptor 2 is outside its buffers"),
    ]
    for over, message in cases:
        with pytest.raises(_hip.HipKernelError, match=message):
            _hip.call("agrl_png_decode_u8", *raw_args(plan, operands, out, status, **over))
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((status == -7).all()), "a rejected call wrote"
    # a frame over the size bound: a container that would hold it, a row that says so
    big = plan.desc.copy()
    big[0, ops.PD_H], big[0, ops.PD_W] = 300, 200
    wide = torch.full((F, 300, 200, 3), 0xA5, dtype=torch.uint8, device=DEV)
    with pytest.raises(_hip.HipKernelError, match="descriptor 0 is outside its buffers .* at most %d inflated bytes" % ops.PNG_MAX_INFLATED):
        _hip.call("agrl_png_decode_u8", *raw_args(plan, operands, wide, status, desc_host=big))
    torch.cuda.synchronize()
    assert bool((wide == 0xA5).all()) and bool((status == -7).all())
    # and the same operands, untouched, decode
    _hip.call("agrl_png_decode_u8", *raw_args(plan, operands, out, status))
    torch.cuda.synchronize()
    want, _ = P.container([P.fixture()[n][1] for n in names])
    assert torch.equal(out.cpu(), torch.from_numpy(want)) and not status.cpu().any()
    with pytest.raises(ValueError, match="out must be contiguous uint8"):
        ops.png_decode(plan, out=out[:, :, :-1])


def test_a_device_descriptor_the_host_copy_does_not_match_is_skipped_with_status_5():
    """the kernel checks the DEVICE copy of every row again: a row that fails there is skipped -- status 5, its slot zeroed, nothing else
    touched -- and the other frames decode"""
    _, ops = mods()
    names, plan = small_plan()
    want, _ = P.container([P.fixture()[n][1] for n in names])
    F, (Hc, Wc) = 3, plan.container
    for col, value in ((ops.PD_OFF, 2 ** 30), (ops.PD_H, 4000), (ops.PD_CH, 7), (ops.PD_LEN, -5)):
        bad = plan.desc.copy()
        bad[1, col] = value
        operands = ops.png_upload(plan._replace(desc=bad), torch.device(DEV))
        obuf, out = banded(want.size, 0xA5)
        status = torch.full((F,), -7, dtype=torch.int32, device=DEV)
        _hip.call("agrl_png_decode_u8", *raw_args(plan, operands, out.view(F, Hc, Wc, 3), status))
        torch.cuda.synchronize()
        expect = want.copy()
        expect[1] = 0
        assert status.cpu().tolist() == [0, ops.PNG_ERR_DESC, 0]
        assert torch.equal(out.view(F, Hc, Wc, 3).cpu(), torch.from_numpy(expect)) and bands_intact(obuf, want.size, 0xA5)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_device_decoders_on_the_gpu_equal_their_cpu_results():
    dd, ops = mods()
    px, jx, un, br = P.fixture(), J.fixture(), P.unsupported(), P.broken()
    pngs = [px["7x9_rgb_smooth_f4"][0], un["palette"][0], px["64x128_grey_smooth_paeth_w9"][0], br["inflated_too_long"][0],
            px[P.LARGE][0], px["7x9_rgb_dynamic_deep"][0], px["1x1_grey_smooth_pillow"][0], px["64x128_rgb_smooth_flushes"][0]]
    cpu, gpu = dd.DevicePngDecoder("cpu"), dd.DevicePngDecoder(DEV)
    want, want_sizes = cpu.decode(pngs, shape=(2, 4))
    with poisoned_outputs():
        got, sizes = gpu.decode(pngs, shape=(2, 4))
    torch.cuda.synchronize()
    assert got.is_cuda and got.shape == (2, 4, 256, 128, 3) and torch.equal(got.cpu(), want) and np.array_equal(sizes, want_sizes)
    assert (gpu.frames, gpu.fallback_frames) == (cpu.frames, cpu.fallback_frames) == (8, 2)
    mixed = [jx["17x9_422_q30_noise"][0], pngs[0], pngs[2], jx["33x47_gray_q85_noise_opt"][0], pngs[1], jx["16x16_420_q100_noise"][0],
             px["1x7_grey_smooth_f3"][0], jx["8x8_444_q30_noise"][0]]
    cpu, gpu = dd.DeviceImageDecoder("cpu"), dd.DeviceImageDecoder(DEV)
    want, want_sizes = cpu.decode(mixed, shape=(2, 2, 2))
    with poisoned_outputs():
        got, sizes = gpu.decode(mixed, shape=(2, 2, 2))
    torch.cuda.synchronize()
    assert got.shape == (2, 2, 2, 64, 128, 3) and torch.equal(got.cpu(), want) and np.array_equal(sizes, want_sizes)
    assert (gpu.frames, gpu.fallback_frames) == (cpu.frames, cpu.fallback_frames) == (8, 1)
    for f, data in enumerate(mixed):
        ref = dd.pillow_decode(data)
        assert np.array_equal(got.view(8, 64, 128, 3)[f, :ref.shape[0], :ref.shape[1]].cpu().numpy(), ref), f


TRACKLET_CLIPS = (1, 3, 2, 5, 1)


def test_packed_extraction_from_png_and_jpeg_bytes_equals_the_decoded_frames_route():
    """PNG and JPEG bytes interleaved -> decode_batches(decoder=DeviceImageDecoder) -> extract_features_packed(frame_size=...) on the
    batch-invariant stub == the same tracklets handed over as Pillow-decoded frames with their valid extents"""
    dd, _ = mods()
    from torchreid import evaluation
    px, jx = P.fixture(), J.fixture()
    pool = [(px[n][0], px[n][1]) for n in px if not n.startswith(("64x128", "256x128"))]
    pool += [(jx[n][0], jx[n][1]) for n in list(jx)[:len(pool)] if not n.startswith("256x128")]
    S = DS.S
    g = torch.Generator().manual_seed(2)
    encoded, decoded, k = [], [], 0
    for t, n in enumerate(TRACKLET_CLIPS):
        chosen = [[pool[(k + c * S + s) * 5 % len(pool)] for s in range(S)] for c in range(n)]
        k += n * S
        adj = torch.rand((1, n, DS.V, DS.V), generator=g)
        pid, cam = torch.tensor([100 + t]), torch.tensor([t % 3])
        encoded.append(([[[item[0] for item in clip] for clip in chosen]], pid, cam, adj))
        box, sizes = P.container([item[1] for clip in chosen for item in clip])
        full = np.zeros((n * S, 48, 48, 3), dtype=np.uint8)        # one container shape for every item of the extraction
        full[:, :box.shape[1], :box.shape[2]] = box
        decoded.append((torch.from_numpy(full).view(1, n, S, 48, 48, 3), pid, cam, adj, sizes.reshape(1, n, S, 2)))
    model = DS.StubModel().to(DEV)
    want, want_pids, want_cams = evaluation.extract_features_packed(model, decoded, clip_batch=4, frame_size=(16, 8))
    model.calls = []
    decoder = dd.DeviceImageDecoder(torch.device(DEV))
    with poisoned_outputs():
        got, pids, cams = evaluation.extract_features_packed(model, evaluation.decode_batches(encoded, torch.device(DEV), decoder=decoder),
                                                             clip_batch=4, frame_size=(16, 8))
    torch.cuda.synchronize()
    assert got.shape == (len(TRACKLET_CLIPS), DS.PIX + DS.ADJ) and torch.equal(got, want)
    assert np.array_equal(pids, want_pids) and np.array_equal(cams, want_cams) and model.calls == DS.expected_calls(TRACKLET_CLIPS, 4)
    assert decoder.frames == sum(TRACKLET_CLIPS) * S and decoder.png.frames > 0 and decoder.jpeg.frames > 0 and decoder.fallback_frames == 0
