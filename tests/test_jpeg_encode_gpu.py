"""GPU: the device JPEG encoder (edgehip_jpeg_encode / edgehip_jpeg_encode_images, rebvo_amd/csrc/jpeg_encode.hip) against libjpeg's files
of tests/golden/jpeg_encode and against the host encoder rebvo_encode_jpeg, byte for byte.  tests/test_jpeg_encode_cpu.py holds the host
encoder equal to the same files.  No PIL, no reference here: fixtures and the host encoder only."""
import ctypes as C

import numpy as np
import pytest

from rebvo_amd import edgehip, synth
from tests import jpeg_encode_fixtures as fx

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4
W, H = 256, 192
FIX = fx.fixtures()


@pytest.fixture(scope="module")
def tool_ctx():
    """a small context that only lends its stream to edgehip_jpeg_encode_images"""
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=1, nslots=2)
    yield eh
    eh.close()


def frames3():
    """three different 256x192 frames: a billboard scene, noise (the longest stream), a ramp"""
    bill = next(iter(synth.billboard_sequence(W, H, 1)))[0].reshape(H, W, 3)
    noise = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    ramp = np.stack([x, 255 - y, (x + y) // 2], -1).astype(np.uint8)
    return np.ascontiguousarray(np.stack([ramp, noise, bill]))


def whole_store(eh):
    import torch
    stride = (eh.jpeg_cap + 15) & ~15
    b = torch.empty((eh.nseq, stride), dtype=torch.uint8, device="cuda")
    s = torch.empty((eh.nseq, 2), dtype=torch.int32, device="cuda")
    eh.jpeg_device(b, s)
    return b.cpu().numpy(), s.cpu().numpy()


def check(got, want, what):
    stream, size, overflow = got
    assert size == len(want) and not overflow, (what, size, len(want), overflow)
    assert np.array_equal(stream, want), (what,) + fx.first_difference(stream, want)


@pytest.mark.parametrize("name", sorted(n for n in FIX if FIX[n]["comment"] is None))
def test_image_alone_equals_libjpeg(tool_ctx, name):
    f = FIX[name]
    check(tool_ctx.jpeg_encode_images(f["rgb"][None], f["quality"])[0], f["jpeg"], name)


@pytest.mark.parametrize("size", [(1, 1), (8, 8), (17, 33), (24, 40), (50, 70), (150, 200)])
def test_batches_of_one_size(tool_ctx, size):
    """The same bytes alone and inside any batch: three images of one size in one launch, and seven with seven different contents (the
    fixtures of the size, and images derived from them — flipped, channels rotated, values shifted — held to the host encoder)."""
    w, h = size
    names = [f"{k}_{w}x{h}_q90" for k in ("noise", "smooth", "saturated")]
    if size == (24, 40):
        names += [f"batch{i}_24x40_q90" for i in range(6)]
    got = tool_ctx.jpeg_encode_images(np.stack([FIX[n]["rgb"] for n in names[:3]]), 90)
    assert len(got) == 3
    for g, n in zip(got, names[:3]):
        check(g, FIX[n]["jpeg"], (n, 3))
    if len(names) >= 9:
        seven = [(FIX[n]["rgb"], FIX[n]["jpeg"]) for n in names[3:9] + names[:1]]
    else:
        base = [FIX[n]["rgb"] for n in names]
        imgs = [base[2], base[0][::-1, ::-1], np.roll(base[1], 1, axis=2), (base[0].astype(np.int32) + 37).astype(np.uint8),
                base[1][:, ::-1] ^ 0x55, 255 - base[2], np.roll(base[0], 2, axis=2) ^ 0xA0]
        seven = [(np.ascontiguousarray(im), fx.host_encode(im, 90)[0]) for im in imgs]
    assert len({im.tobytes() for im, _ in seven}) == 7                # seven different contents, at every size
    got = tool_ctx.jpeg_encode_images(np.stack([im for im, _ in seven]), 90)
    assert len(got) == 7
    for k, (g, (_, want)) in enumerate(zip(got, seven)):
        check(g, want, (size, 7, k))


def test_images_cap_and_arguments(tool_ctx):
    """A cap below the stream: true size, flag, the prefix, and nothing behind the region (the next image's region starts there)."""
    f = FIX["noise_50x70_q90"]
    n = len(f["jpeg"])
    cap = (n - 40) & ~15
    got = tool_ctx.jpeg_encode_images(np.stack([f["rgb"], FIX["smooth_50x70_q90"]["rgb"]]), 90, cap=cap)
    assert got[0][1] == n and got[0][2] and np.array_equal(got[0][0], f["jpeg"][:cap])
    check(got[1], FIX["smooth_50x70_q90"]["jpeg"], "the neighbour behind an overflowing image")
    lib, z = tool_ctx.lib, C.c_void_p(16)
    for w, h, count, q, cap in ((0, 4, 1, 90, 1024), (4, 4, 0, 90, 1024), (4, 4, 1, 0, 1024), (4, 4, 1, 101, 1024), (4, 4, 1, 90, 1000),
                                (4, 4, 1, 90, 608)):
        assert lib.edgehip_jpeg_encode_images(tool_ctx.ctx, z, w, h, count, q, z, C.c_uint32(cap), z) == ERR_ARG, (w, h, count, q, cap)
    assert lib.edgehip_jpeg_encode_images(tool_ctx.ctx, None, 4, 4, 1, 90, z, C.c_uint32(1024), z) == ERR_ARG


def test_context_slots_rgb_grey8_bound():
    """What the slot holds — RGB24, 8-bit mono, frames of a bound pool — through the accessors stage A uses; the comment segment."""
    import torch
    fr = frames3()
    grey = np.ascontiguousarray(fr[:, :, :, 1])
    text = b"CREATOR: gd-jpeg v1.0 (using IJG JPEG v62), quality = 90\n"
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=3, nslots=3)
    try:
        eh.jpeg_enable(90, comment=text)
        assert eh.jpeg_cap == edgehip.jpeg_bound(W, H, len(text))
        eh.upload_rgb(0, fr)
        eh.jpeg_encode(0)
        for s, g in enumerate(eh.jpeg_download_batch([0, 1, 2], with_record=True)):
            check(g, fx.host_encode(fr[s], 90, text)[0], ("rgb24", s))
        eh.upload_grey8(1, grey)
        eh.jpeg_encode(1)
        for s in range(3):
            want = fx.host_encode(np.repeat(grey[s][:, :, None], 3, 2), 90, text)[0]
            check(eh.jpeg_download(s, with_record=True), want, ("grey8", s))
        pool = torch.zeros(5 * H * W * 3 + 16, dtype=torch.uint8, device="cuda")
        order = [4, 0, 2]
        for s, k in enumerate(order):
            pool[k * H * W * 3:(k + 1) * H * W * 3] = torch.from_numpy(fr[s].reshape(-1)).cuda()
        torch.cuda.synchronize()
        eh.bind_rgb_indexed(2, pool.data_ptr(), 5, order)
        eh.jpeg_encode(2)
        for s in range(3):
            check(eh.jpeg_download(s, with_record=True), fx.host_encode(fr[s], 90, text)[0], ("bound", s))
        # without the comment the billboard frame is the fixture's file
        eh.jpeg_enable(90)
        eh.jpeg_encode(0)
        check(eh.jpeg_download(2, with_record=True), FIX["billboard_256x192_q90"]["jpeg"], "billboard fixture")
    finally:
        eh.close()


def test_context_undistorted():
    """With UseUndistort the undistorted frame is encoded (PipeBuffer::imgc): the host encoder on edgehip_download_undistorted."""
    fr = frames3()
    eh = edgehip.EdgeHip(edgehip.tum_params(W, H, use_undistort=1), nseq=3, nslots=2)
    try:
        eh.jpeg_enable(90)
        eh.upload_rgb(0, fr)
        eh.upload_grey8(1, np.ascontiguousarray(fr[:, :, :, 0]))
        for slot in (0, 1):
            eh.jpeg_encode(slot)
            got = eh.jpeg_download_batch([0, 1, 2], with_record=True)
            for s in range(3):
                und = eh.download_undistorted(s, slot)
                assert not np.array_equal(und, fr[s])          # the map moves pixels
                check(got[s], fx.host_encode(und, 90)[0], ("undistorted", slot, s))
    finally:
        eh.close()


def test_select_cap_and_guards():
    fr = frames3()
    want = [fx.host_encode(f, 90)[0] for f in fr]
    assert len(want[1]) > max(len(want[0]), len(want[2]))
    cap = len(want[1]) - 1                                   # one byte short of sequence 1's frame, and no multiple of 16
    assert cap % 16 != 0
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=3, nslots=2)
    try:
        eh.jpeg_enable(90, cap)
        eh.upload_rgb(0, fr)
        eh.upload_rgb(1, fr[::-1])
        eh.jpeg_encode(0)
        store, rec = whole_store(eh)
        assert rec.tolist() == [[len(want[0]), 0], [len(want[1]), 1], [len(want[2]), 0]]
        for s in range(3):
            n = min(len(want[s]), cap)
            assert np.array_equal(store[s, :n], want[s][:n]), s
            assert not store[s, n:].any(), s                 # behind the stream, and the guard bytes between cap and the stride
        stream, size, overflow = eh.jpeg_download(1, with_record=True)
        assert size == len(want[1]) and overflow and np.array_equal(stream, want[1][:cap])
        # the select mask: sequences 0 and 2 keep region and record while sequence 1 takes the other slot's (shorter) frame
        eh.jpeg_select([0, 1, 0])
        eh.jpeg_encode(1)
        store2, rec2 = whole_store(eh)
        assert np.array_equal(store2[[0, 2]], store[[0, 2]]) and np.array_equal(rec2[[0, 2]], rec[[0, 2]])
        assert rec2[1].tolist() == [len(want[1]), 1]          # slot 1 holds the frames in reverse order: sequence 1's is the same
        eh.jpeg_select([1, 0, 0])
        eh.jpeg_encode(1)
        store3, rec3 = whole_store(eh)
        assert rec3[0].tolist() == [len(want[2]), 0] and np.array_equal(store3[0, :len(want[2])], want[2])
        assert np.array_equal(store3[1:], store2[1:]) and np.array_equal(rec3[1:], rec2[1:])
        eh.jpeg_select(None)
        eh.jpeg_encode(0)
        assert np.array_equal(whole_store(eh)[1], rec)
    finally:
        eh.close()


def test_frame_path_unchanged():
    """edgehip_read_nav and the KeyLines of a 6-frame replay are the same with an encode behind every frame."""
    seq = [f for f, _, _ in synth.billboard_sequence(W, H, 6)]
    runs = []
    for with_jpeg in (False, True):
        eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=2, nslots=3)
        try:
            if with_jpeg:
                eh.jpeg_enable(90)
            log = []
            for k, f in enumerate(seq):
                slot = eh.next_slot()
                eh.upload_rgb(slot, np.stack([f.reshape(H, W, 3), seq[-1 - k].reshape(H, W, 3)]))
                eh.process_frame(0.05 * k)
                if with_jpeg:
                    eh.jpeg_encode(eh.cur_slot())
                nav = eh.read_nav()
                kls = [eh.download_keylines(s, eh.cur_slot()) for s in range(2)]
                log.append((b"".join(bytes(n) for n in nav), [(len(kl), kl.tobytes(), mask.tobytes()) for kl, mask in kls]))
                if with_jpeg:
                    for s, src in enumerate((f, seq[-1 - k])):
                        check(eh.jpeg_download(s, with_record=True), fx.host_encode(src.reshape(H, W, 3), 90)[0], ("replay", k, s))
            runs.append(log)
        finally:
            eh.close()
    assert runs[0] == runs[1]
    assert runs[0][-1][1][0][0] > 100   # KeyLines were found


def test_errors_and_reenable():
    fr = frames3()
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=3, nslots=2)
    lib, ctx = eh.lib, eh.ctx
    try:
        assert lib.edgehip_jpeg_encode(ctx, 0) == ERR_STATE             # store off
        assert lib.edgehip_jpeg_select(ctx, None) == ERR_STATE
        assert lib.edgehip_download_jpeg(ctx, 0, None, C.c_uint32(0), None) == ERR_STATE
        assert lib.edgehip_jpeg_device(ctx, 0, 1, None, None) == ERR_STATE
        for q in (0, 101, -5):
            assert lib.edgehip_jpeg_enable(ctx, q, C.c_uint32(100000), None) == ERR_ARG
        assert lib.edgehip_jpeg_enable(ctx, 90, C.c_uint32(fx.HEADER_BYTES + 1), None) == ERR_ARG      # below header + EOI
        assert lib.edgehip_jpeg_enable(ctx, 90, C.c_uint32(fx.HEADER_BYTES + 2 + 4), b"abcdefgh") == ERR_ARG   # the comment counts
        assert lib.edgehip_jpeg_enable(None, 90, C.c_uint32(100000), None) == ERR_ARG
        assert lib.edgehip_jpeg_encode(ctx, 0) == ERR_STATE             # a refused enable leaves the store off
        eh.jpeg_enable(90)
        assert lib.edgehip_jpeg_encode(ctx, -1) == ERR_ARG and lib.edgehip_jpeg_encode(ctx, 2) == ERR_ARG
        assert lib.edgehip_download_jpeg(ctx, 3, None, C.c_uint32(0), None) == ERR_ARG
        assert lib.edgehip_jpeg_device(ctx, 2, 2, None, None) == ERR_ARG
        eh.upload_rgb(0, fr)
        eh.jpeg_encode(0)
        check(eh.jpeg_download(1, with_record=True), fx.host_encode(fr[1], 90)[0], "q90")
        eh.jpeg_enable(cap_bytes=0)                                     # disable
        assert lib.edgehip_jpeg_encode(ctx, 0) == ERR_STATE
        eh.jpeg_enable(35, 40000)                                       # another quality and cap
        eh.jpeg_encode(0)
        for s in (0, 2):
            check(eh.jpeg_download(s, with_record=True), fx.host_encode(fr[s], 35)[0], ("q35", s))
        want = fx.host_encode(fr[1], 35)[0]
        stream, size, overflow = eh.jpeg_download(1, with_record=True)
        assert size == len(want) and overflow == (len(want) > 40000) and np.array_equal(stream, want[:40000])
    finally:
        eh.close()


def test_export_ring_with_tickets_in_flight():
    """edgehip_jpeg_export: three tickets out at once over two slots, sequences by request (another order, a subset), fetched and waited
    for afterwards: every stream equals the host encoder's; the store's own regions are not touched; four tickets are the limit."""
    fr = frames3()
    want = [fx.host_encode(f, 90)[0] for f in fr]
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=3, nslots=2)
    lib, ctx = eh.lib, eh.ctx
    try:
        t = C.c_int(0)
        seqs = np.array([0], np.int32)
        assert lib.edgehip_jpeg_export(ctx, 0, 1, seqs.ctypes.data_as(C.c_void_p), C.byref(t)) == ERR_STATE      # store off
        eh.jpeg_enable(90, 70000)
        before = whole_store(eh)
        eh.upload_rgb(0, fr)
        eh.upload_rgb(1, fr[::-1])
        tickets = [eh.jpeg_export(0, [2, 0, 1]), eh.jpeg_export(1, [1, 2]), eh.jpeg_export(0, [1])]
        expect = [[want[2], want[0], want[1]], [want[1], want[0]], [want[1]]]
        got = [eh.jpeg_export_fetch(tk) for tk in tickets]
        for tk in tickets:
            eh.jpeg_export_wait(tk)
        for (bufs, rec), exp in zip(got, expect):
            assert len(bufs) == len(exp)
            for b, r, w_ in zip(bufs, rec, exp):
                assert int(r[0]) == len(w_) and int(r[1]) == (len(w_) > 70000) and np.array_equal(b, w_[:70000])
        after = whole_store(eh)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        out = [eh.jpeg_export(0, [0]) for _ in range(4)]
        assert lib.edgehip_jpeg_export(ctx, 0, 1, seqs.ctypes.data_as(C.c_void_p), C.byref(t)) == ERR_STATE      # four outstanding
        for tk in out:
            eh.jpeg_export_wait(tk)                                   # never fetched: released behind their encoders
        assert lib.edgehip_jpeg_export_wait(ctx, out[0][0]) == ERR_ARG
        assert lib.edgehip_jpeg_export(ctx, 5, 1, seqs.ctypes.data_as(C.c_void_p), C.byref(t)) == ERR_ARG
        bad = np.array([3], np.int32)
        assert lib.edgehip_jpeg_export(ctx, 0, 1, bad.ctypes.data_as(C.c_void_p), C.byref(t)) == ERR_ARG
    finally:
        eh.close()
