"""GPU: the device JPEG decoder (edgehip_jpeg_decode_images / edgehip_upload_jpeg, rebvo_amd/csrc/jpeg_decode.hip) against PIL's pixels of
tests/golden/jpeg_decode and against the host reader rebvo_decode_jpeg, bit for bit.  tests/test_jpeg_decode_cpu.py holds the same walk and
pixel functions to the same files on the CPU and shows the walk in bounds on corrupt streams.  No PIL, no reference here."""
import ctypes as C

import numpy as np
import pytest

from rebvo_amd import edgehip, synth
from tests import jpeg_decode_fixtures as fx

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4
W, H = 256, 192
DEC = fx.decodable()


@pytest.fixture(scope="module")
def tool_ctx():
    """a small context that only lends its stream to edgehip_jpeg_decode_images"""
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=1, nslots=2)
    yield eh
    eh.close()


def frames3():
    """three different 256x192 frames: a ramp, noise, a billboard scene"""
    bill = next(iter(synth.billboard_sequence(W, H, 1)))[0].reshape(H, W, 3)
    noise = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    ramp = np.stack([x, 255 - y, (x + y) // 2], -1).astype(np.uint8)
    return np.ascontiguousarray(np.stack([ramp, noise, bill]))


@pytest.fixture(scope="module")
def streams3(tool_ctx):
    """the device encoder's streams of frames3() (4:2:0, no DRI, Annex-K tables), and what the host reader makes of them"""
    jp = [g[0] for g in tool_ctx.jpeg_encode_images(frames3(), 90)]
    return jp, [fx.host_decode(s) for s in jp]


@pytest.mark.parametrize("name", sorted(DEC))
def test_image_alone_equals_pil(tool_ctx, name):
    """every fixture alone: the sizes 1x1 .. 150x200 (partial MCUs right and bottom, odd chroma widths), grey / 4:4:4 / 4:2:2 / 4:2:0,
    q 1 .. 100, optimised and Annex-K tables, restart intervals 1, 3, 7 and one MCU row, five groups of 32 intervals"""
    f = DEC[name]
    h, w = f["rgb"].shape[:2]
    got = tool_ctx.jpeg_decode_images([f["jpeg"]], w, h)
    assert np.array_equal(got[0], f["rgb"]), (name, np.argwhere(got[0] != f["rgb"])[:4])


@pytest.mark.parametrize("size", [(24, 40), (50, 70)])
def test_ragged_batches_and_guard_bytes(tool_ctx, size):
    """3 and 7 different streams of one size (different samplings, tables, qualities, restart intervals, lengths) in one call: every
    image as it is alone; the output sits at an odd offset inside a larger tensor whose other bytes stay as they were."""
    import torch
    w, h = size
    names = fx.of_size(w, h)
    assert len(names) >= 7 and len({DEC[n]["sampling"] for n in names[:7]}) >= 3
    for count in (3, 7):
        pick = names[:count] if count == 7 else names[2:5]
        nb = count * w * h * 3
        out = torch.full((nb + 64,), 0xC3, dtype=torch.uint8, device="cuda")
        tool_ctx.jpeg_decode_images([DEC[n]["jpeg"] for n in pick], w, h, out=out, offset=21)
        got = out.cpu().numpy()
        assert (got[:21] == 0xC3).all() and (got[21 + nb:] == 0xC3).all()
        for k, n in enumerate(pick):
            assert np.array_equal(got[21 + k * w * h * 3:21 + (k + 1) * w * h * 3].reshape(h, w, 3), DEC[n]["rgb"]), (count, n)


def test_corrupt_streams_report_and_leave_the_neighbour(tool_ctx):
    """One truncated stream and one with an inverted entropy byte — both walked in bounds by the CPU guard program
    (tests/test_jpeg_decode_cpu.py::test_chain_walk_guard) — in a batch of three: their status is nonzero, the third image exact, the
    context usable afterwards."""
    import torch
    truncated, flipped = fx.corrupt_pair()
    good = DEC[fx.CORRUPT_SOURCE]
    h, w = good["rgb"].shape[:2]
    out = torch.zeros(3 * w * h * 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(edgehip.EdgeHipError) as e:
        tool_ctx.jpeg_decode_images([truncated, flipped, good["jpeg"]], w, h, out=out)
    assert e.value.code == ERR_ARG
    r = e.value.reasons
    assert r[0] == edgehip.JPEG_REASON_WALK + 2 and r[1] > edgehip.JPEG_REASON_WALK and r[2] == 0, r
    assert r[1] == edgehip.JPEG_REASON_WALK + fx.staged(flipped, good["rgb"].shape)[1]          # the host walk's status
    assert np.array_equal(out.cpu().numpy()[2 * w * h * 3:].reshape(h, w, 3), good["rgb"])
    assert np.array_equal(tool_ctx.jpeg_decode_images([good["jpeg"]], w, h)[0], good["rgb"])


def test_images_arguments(tool_ctx):
    f = DEC["noise_24x40_420_q90"]
    with pytest.raises(edgehip.EdgeHipError) as e:                       # not the size asked for; a progressive file
        tool_ctx.jpeg_decode_images([f["jpeg"], DEC["noise_50x70_422_q90"]["jpeg"], fx.fixtures()["smooth_17x33_progressive"]["jpeg"]], 24, 40)
    assert e.value.code == ERR_ARG and e.value.reasons == [0, fx.SIZE, fx.PROGRESSIVE]
    lib, z = tool_ctx.lib, C.c_void_p(16)
    for count, w, h in ((0, 24, 40), (1, 0, 40), (1, 24, 0), (1, 20000, 40)):
        assert lib.edgehip_jpeg_decode_images(tool_ctx.ctx, z, z, count, w, h, z, None) == ERR_ARG
    assert lib.edgehip_jpeg_decode_images(tool_ctx.ctx, None, z, 1, 24, 40, z, None) == ERR_ARG
    assert lib.edgehip_jpeg_decode_images(tool_ctx.ctx, z, z, 1, 24, 40, None, None) == ERR_ARG
    assert edgehip.jpeg_probe(f["jpeg"])["reason"] == 0 and edgehip.jpeg_probe(b"")["reason"] == fx.TRUNCATED
    assert edgehip.jpeg_probe(f["jpeg"]) == fx.probe(f["jpeg"])


def test_round_trip_through_slots(streams3):
    """edgehip_jpeg_encode of three frames, download, upload_jpeg into another slot: the slot holds what the host reader decodes."""
    fr = frames3()
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=3, nslots=3)
    try:
        eh.jpeg_enable(90)
        eh.jpeg_decode_enable()
        eh.upload_rgb(0, fr)
        eh.jpeg_encode(0)
        jp = eh.jpeg_download_batch([0, 1, 2])
        for a, b in zip(jp, streams3[0]):
            assert np.array_equal(a, b)
        eh.upload_jpeg(1, jp)
        assert eh.jpeg_decode_status(1).tolist() == [0, 0, 0]
        for s in range(3):
            got = eh.download_frame(s, 1)
            assert got.shape == (H, W, 3) and np.array_equal(got, streams3[1][s]), s
            assert np.array_equal(eh.download_frame(s, 0), fr[s])          # the raw slot is what was uploaded
        # a sub-range, in another order: sequences 1 and 2 take streams 0 and 1, sequence 0 keeps its frame
        eh.upload_jpeg(1, [jp[0], jp[1]], seq_first=1)
        assert np.array_equal(eh.download_frame(0, 1), streams3[1][0])
        assert np.array_equal(eh.download_frame(1, 1), streams3[1][0]) and np.array_equal(eh.download_frame(2, 1), streams3[1][1])
    finally:
        eh.close()


def stage_a_of(feed):
    """a fresh context (the detector's threshold state moves with every stage A), `feed` fills slot 0 -> KeyLines and masks of stage A"""
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=3, nslots=2)
    try:
        eh.jpeg_decode_enable()
        feed(eh)
        eh.stage_a(0)
        return [(kl.tobytes(), mask.tobytes()) for kl, mask in (eh.download_keylines(s, 0) for s in range(3))]
    finally:
        eh.close()


def test_slot_path_equals_raw_upload(streams3):
    """upload_jpeg followed by stage A gives the KeyLines of upload_rgb of the host-decoded pixels, bit for bit."""
    jp, px = streams3
    want = stage_a_of(lambda eh: eh.upload_rgb(0, np.stack(px)))
    got = stage_a_of(lambda eh: eh.upload_jpeg(0, jp))
    assert got == want and len(want[2][0]) > 100 * 168


def test_grey8_slot_path_and_status():
    """One-component streams with format grey8: the slot holds the 8-bit plane, stage A's KeyLines are those of upload_grey8 of the
    host-decoded plane — and of the same streams decoded to RGB24.  One stream has an MCU row per restart interval (24 intervals, one
    group).  Then a stream cut in its entropy-coded segment (walked in bounds by the CPU guard program first) between two good ones:
    its status says out of data, the neighbours' frames are exact, and the context decodes again afterwards."""
    a, b = DEC["mosaic_256x192_grey_q90"], DEC["mosaic_256x192_grey_q90_drirow"]
    jp = [a["jpeg"], b["jpeg"], a["jpeg"]]
    planes = np.ascontiguousarray(np.stack([a["rgb"], b["rgb"], a["rgb"]])[:, :, :, 0])
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=3, nslots=3)
    try:
        want = stage_a_of(lambda e: e.upload_grey8(0, planes))
        assert stage_a_of(lambda e: e.upload_jpeg(0, jp, fmt=edgehip.FRAME_GREY8)) == want and len(want[0][0]) > 100 * 168
        assert stage_a_of(lambda e: e.upload_jpeg(0, jp)) == want             # the same streams as RGB24: r = g = b = Y
        eh.jpeg_decode_enable()
        eh.upload_jpeg(1, jp, fmt=edgehip.FRAME_GREY8)
        for s in range(3):
            got = eh.download_frame(s, 1)
            assert got.shape == (H, W) and np.array_equal(got, planes[s]), s
        eh.upload_jpeg(2, jp)
        assert np.array_equal(eh.download_frame(1, 2), b["rgb"])
        eh.upload_jpeg(1, [b["jpeg"], fx.corrupt_slot_stream(), a["jpeg"]], fmt=edgehip.FRAME_GREY8)
        assert eh.jpeg_decode_status(1).tolist() == [0, 2, 0]
        assert np.array_equal(eh.download_frame(0, 1), planes[1]) and np.array_equal(eh.download_frame(2, 1), planes[0])
        eh.upload_jpeg(1, jp, fmt=edgehip.FRAME_GREY8)
        assert eh.jpeg_decode_status(1).tolist() == [0, 0, 0] and np.array_equal(eh.download_frame(1, 1), planes[1])
    finally:
        eh.close()


def test_all_or_nothing_and_errors(streams3):
    jp, px = streams3
    fr = frames3()
    small = DEC["noise_24x40_420_q90"]["jpeg"]
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=3, nslots=2)
    lib, ctx = eh.lib, eh.ctx
    try:
        st = np.zeros(3, np.int32)
        with pytest.raises(edgehip.EdgeHipError) as e:                   # decoder off
            eh.upload_jpeg(0, jp)
        assert e.value.code == ERR_STATE
        assert lib.edgehip_read_jpeg_decode_status(ctx, 0, st.ctypes.data_as(C.c_void_p)) == ERR_STATE
        assert lib.edgehip_jpeg_decode_enable(ctx, 0, C.c_uint32(1000)) == ERR_ARG
        assert lib.edgehip_jpeg_decode_enable(ctx, 4, C.c_uint32(1000)) == ERR_ARG       # more streams than sequences
        assert lib.edgehip_jpeg_decode_enable(None, 3, C.c_uint32(1000)) == ERR_ARG
        eh.jpeg_decode_enable()
        eh.upload_grey8(0, np.ascontiguousarray(fr[:, :, :, 1]))
        eh.sync()
        before = [eh.download_frame(s, 0) for s in range(3)]
        assert before[0].shape == (H, W)
        # one wrong-size stream: nothing is enqueued, the slot keeps storage and format
        with pytest.raises(edgehip.EdgeHipError) as e:
            eh.upload_jpeg(0, [jp[0], small, jp[2]])
        assert e.value.code == ERR_ARG and e.value.reasons == [0, fx.SIZE, 0]
        for s in range(3):
            assert np.array_equal(eh.download_frame(s, 0), before[s])
        with pytest.raises(edgehip.EdgeHipError) as e:                   # colour into grey8
            eh.upload_jpeg(0, jp, fmt=edgehip.FRAME_GREY8)
        assert e.value.code == ERR_ARG and e.value.reasons == [0, 0, 0]
        assert eh.download_frame(0, 0).shape == (H, W)
        for slot, first, n in ((-1, 0, 3), (2, 0, 3), (0, 1, 3), (0, -1, 1)):
            with pytest.raises(edgehip.EdgeHipError) as e:
                eh.upload_jpeg(slot, jp[:n], seq_first=first)
            assert e.value.code == ERR_ARG
        eh.jpeg_decode_enable(cap_bytes=len(jp[1]) - 700)                # cap_bytes below the longest segment
        with pytest.raises(edgehip.EdgeHipError) as e:
            eh.upload_jpeg(0, jp)
        assert e.value.code == ERR_ARG and e.value.reasons[1] == fx.TOO_LONG and e.value.reasons[0] == e.value.reasons[2] == 0
        eh.jpeg_decode_enable(cap_bytes=0)                               # disable, re-enable with fewer streams
        with pytest.raises(edgehip.EdgeHipError) as e:
            eh.upload_jpeg(0, jp)
        assert e.value.code == ERR_STATE
        eh.jpeg_decode_enable(max_streams=2)
        with pytest.raises(edgehip.EdgeHipError) as e:
            eh.upload_jpeg(0, jp)
        assert e.value.code == ERR_ARG
        eh.upload_jpeg(0, jp[:2], seq_first=1)
        assert eh.jpeg_decode_status(0).tolist() == [0, 0, 0]
        assert np.array_equal(eh.download_frame(2, 0), px[1])
    finally:
        eh.close()


def test_frame_path_unchanged_with_decoder_enabled():
    """edgehip_read_nav and the KeyLines of a 4-frame replay are the same with the decoder enabled but unused."""
    seq = [f for f, _, _ in synth.billboard_sequence(W, H, 4)]
    runs = []
    for with_dec in (False, True):
        eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=2, nslots=3)
        try:
            if with_dec:
                eh.jpeg_decode_enable()
            log = []
            for k, f in enumerate(seq):
                eh.upload_rgb(eh.next_slot(), np.stack([f.reshape(H, W, 3), seq[-1 - k].reshape(H, W, 3)]))
                eh.process_frame(0.05 * k)
                kls = [eh.download_keylines(s, eh.cur_slot()) for s in range(2)]
                log.append((b"".join(bytes(n) for n in eh.read_nav()), [(kl.tobytes(), mask.tobytes()) for kl, mask in kls]))
            runs.append(log)
        finally:
            eh.close()
    assert runs[0] == runs[1]
    assert len(runs[0][-1][1][0][0]) > 100 * 168   # KeyLines were found
