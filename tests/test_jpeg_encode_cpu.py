"""CPU: the host JPEG encoder (rebvo_encode_jpeg, rebvo_amd/host/src/jpeg_encode.cpp) against libjpeg's own files, byte for byte, header
included.  The files are PIL's (libjpeg-turbo) at the settings gd's gdImageJpegPtr leaves libjpeg with — what the reference's MJPEGEncoder
writes — and live in tests/golden/jpeg_encode (tools/make_jpeg_encode_golden.py).  tests/test_jpeg_encode_gpu.py holds the device encoder
to the same files."""
import numpy as np
import pytest

from rebvo_amd import edgehip
from tests import jpeg_encode_fixtures as fx

FIX = fx.fixtures()


def test_fixture_set():
    """The sizes, contents and qualities the encoder's rules need: padding in both directions, odd sizes, an even height off the MCU
    grid (chroma rows are replicated after the downsampling), every quality regime."""
    sizes = {f["rgb"].shape[:2][::-1] for f in FIX.values()}
    assert {(1, 1), (8, 8), (17, 33), (24, 40), (50, 70), (150, 200), (256, 192)} <= sizes
    for w, h in ((1, 1), (8, 8), (17, 33), (24, 40), (50, 70), (150, 200)):
        for kind in ("noise", "smooth", "saturated"):
            assert f"{kind}_{w}x{h}_q90" in FIX
    assert {f["quality"] for f in FIX.values()} == {1, 10, 50, 90, 100}
    assert sum(f["comment"] is not None for f in FIX.values()) == 1
    assert any(w & 1 for w, _ in sizes) and any(h & 1 for _, h in sizes) and any(h % 2 == 0 and h % 16 for _, h in sizes)


@pytest.mark.parametrize("name", sorted(FIX))
def test_host_encoder_equals_libjpeg(name):
    f = FIX[name]
    got, stats = fx.host_encode(f["rgb"], f["quality"], f["comment"])
    assert np.array_equal(got, f["jpeg"]), fx.first_difference(got, f["jpeg"])
    assert stats == f["stats"]          # the populations the tool counted, recomputed
    h, w = f["rgb"].shape[:2]
    assert edgehip.jpeg_bound(w, h, len(f["comment"] or b"")) >= len(f["jpeg"])


def test_populations():
    """What the streams exercise, so that equality means something: stuffed bytes, ZRL, a block that ends without EOB, the largest DC and
    AC categories, dummy blocks right of and below the image."""
    top = {k: max(f["stats"][k] for f in FIX.values()) for k in fx.STATS}
    assert top["stuffed"] >= 20 and top["zrl"] >= 1 and top["no_eob"] >= 1
    assert top["max_dc_cat"] == 11 and top["max_ac_cat"] == 10
    assert top["dummy_right"] >= 1 and top["dummy_bottom"] >= 1
    # the stuffed pairs are really in the file: count them behind SOS
    best = max(FIX.values(), key=lambda f: f["stats"]["stuffed"])
    body = best["jpeg"][fx.HEADER_BYTES:-2]
    assert int(np.sum((body[:-1] == 0xFF) & (body[1:] == 0))) == best["stats"]["stuffed"]


def test_header_layout():
    f = FIX["smooth_17x33_q90"]
    j = f["jpeg"].tobytes()
    assert j[:4] == b"\xff\xd8\xff\xe0" and j[6:11] == b"JFIF\0" and j[11:20] == bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])
    assert j[20:22] == b"\xff\xdb"                                   # no COM: DQT follows APP0
    assert j[fx.HEADER_BYTES - 14:fx.HEADER_BYTES - 12] == b"\xff\xda" and j[fx.HEADER_BYTES - 3:fx.HEADER_BYTES] == bytes([0, 63, 0])
    sof = j.index(b"\xff\xc0")
    assert j[sof + 4:sof + 19] == bytes([8, 0, 33, 0, 17, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert [j[i + 4] for i in range(len(j) - 1) if j[i:i + 2] == b"\xff\xc4" and i < fx.HEADER_BYTES] == [0x00, 0x10, 0x01, 0x11]
    # the COM segment sits directly behind APP0 and moves everything else by its length
    c = FIX["comment_17x33_q90"]
    jc, text = c["jpeg"].tobytes(), c["comment"]
    assert jc[20:24] == b"\xff\xfe" + (len(text) + 2).to_bytes(2, "big") and jc[24:24 + len(text)] == text
    assert jc[24 + len(text):24 + len(text) + 2] == b"\xff\xdb"
    got, _ = fx.host_encode(c["rgb"], 90, text)
    assert len(got) == len(jc) and got.tobytes()[:fx.HEADER_BYTES + len(text) + 4] == jc[:fx.HEADER_BYTES + len(text) + 4]


def test_bound_and_bad_arguments():
    lib = fx.host_lib()
    assert edgehip.jpeg_bound(1, 1) == 623 + 2 * ((6 * 1660 + 7) // 8) + 2
    assert edgehip.jpeg_bound(752, 480) == 623 + 2 * ((8460 * 1660 + 7) // 8) + 2
    assert edgehip.jpeg_bound(17, 33, 10) == edgehip.jpeg_bound(17, 33) + 14
    assert edgehip.jpeg_bound(0, 5) == 0
    px = np.zeros((4, 4, 3), np.uint8)
    for w, h, q in ((0, 4, 90), (4, 0, 90), (4, 4, 0), (4, 4, 101)):
        assert lib.rebvo_encode_jpeg(px.ctypes.data, w, h, q, None, None, 0, None) == -1


@pytest.mark.parametrize("name", sorted(FIX))
def test_own_reader_decodes_the_stream(name):
    """The project's own reader (jpeg_reader.cpp) takes what the encoder writes; its pixels are libjpeg's where PIL is there to say."""
    f = FIX[name]
    got, _ = fx.host_encode(f["rgb"], f["quality"], f["comment"])
    mine = fx.host_decode(got)
    assert mine.shape == f["rgb"].shape
    try:
        import io
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(mine, np.asarray(Image.open(io.BytesIO(f["jpeg"].tobytes())).convert("RGB")))


# ---- the wire packet: net_packet_hdr + kline_num records of 15 B + the picture (rebvo_third_t.cpp:189-234) ----
import ctypes as C  # noqa: E402

HDR = fx.HDR


def _packet_lib():
    lib = fx.host_lib()
    lib.rebvo_build_net_packet.argtypes = [C.c_void_p] * 4
    lib.rebvo_build_net_packet.restype = C.c_longlong
    lib.rebvo_net_packet_ring_new.argtypes = [C.c_uint]
    lib.rebvo_net_packet_ring_new.restype = C.c_void_p
    lib.rebvo_net_packet_ring_push.argtypes = [C.c_void_p] * 5 + [C.c_longlong]
    lib.rebvo_net_packet_ring_push.restype = C.c_longlong
    lib.rebvo_net_packet_ring_free.argtypes = [C.c_void_p]
    return lib


def test_packet_layout():
    """The header is the reference's packed struct, field for field; records and picture follow it back to back."""
    assert HDR.itemsize == 108
    assert [HDR.fields[n][1] for n in HDR.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40]
    assert [HDR["nav"].fields[n][1] for n in HDR["nav"].names] == [0, 12, 24, 36, 48, 60, 64]
    lib = _packet_lib()
    h = np.zeros(1, HDR)
    h["w"], h["h"], h["encoder_type"], h["kline_num"], h["km_num"], h["k"], h["max_rho"], h["jpeg_size"] = 752, 480, 1, 3, 2, 1.5, 20.0, 7
    h["nav"]["Pos"], h["nav"]["dt"] = (1, 2, 3), 0.05
    rec = np.arange(45, dtype=np.uint8)
    pic = np.arange(200, 207, dtype=np.uint8)
    out = np.zeros(108 + 45 + 7, np.uint8)
    assert lib.rebvo_build_net_packet(h.ctypes.data, rec.ctypes.data, pic.ctypes.data, out.ctypes.data) == len(out)
    got = out[:108].view(HDR)[0]
    assert got["data_size"] == len(out) and got["jpeg_size"] == 7 and got["kline_num"] == 3 and got["w"] == 752 and got["h"] == 480
    assert got["k"] == np.float32(1.5) and got["max_rho"] == 20 and got["nav"]["Pos"].tolist() == [1, 2, 3] and got["nav"]["dt"] == np.float32(0.05)
    assert np.array_equal(out[108:153], rec) and np.array_equal(out[153:], pic)


@pytest.mark.parametrize("delay", [0, 2])
def test_packet_edge_map_delay(delay):
    """Five frames of fake records and pictures: the records of frame n (and their count, km_num, k) are in the packet that carries the
    picture (and size, nav data) of frame n + delay; the first `delay` packets carry no records."""
    lib = _packet_lib()
    ring = lib.rebvo_net_packet_ring_new(delay)
    try:
        packets = []
        for n in range(5):
            h = np.zeros(1, HDR)
            h["w"], h["h"], h["encoder_type"], h["max_rho"] = 64, 48, 1, 20.0
            h["kline_num"], h["km_num"], h["k"], h["jpeg_size"] = n + 1, 10 + n, 1.0 + n, 20 + n
            h["nav"]["dt"] = 0.01 * (n + 1)
            rec = np.full(15 * (n + 1), 100 + n, np.uint8)
            pic = np.full(20 + n, 200 + n, np.uint8)
            out = np.zeros(4096, np.uint8)
            size = lib.rebvo_net_packet_ring_push(ring, h.ctypes.data, rec.ctypes.data, pic.ctypes.data, out.ctypes.data, len(out))
            packets.append(out[:size].copy())
        for n, p in enumerate(packets):
            h = p[:108].view(HDR)[0]
            m = n - delay                                   # whose records travel with picture n
            nrec = m + 1 if m >= 0 else 0
            assert h["kline_num"] == nrec and h["jpeg_size"] == 20 + n and h["data_size"] == len(p) == 108 + 15 * nrec + 20 + n
            assert h["nav"]["dt"] == np.float32(0.01 * (n + 1)) and h["w"] == 64 and h["encoder_type"] == 1
            assert (p[108:108 + 15 * nrec] == 100 + m).all() and (p[108 + 15 * nrec:] == 200 + n).all()
            if m >= 0:
                assert h["km_num"] == 10 + m and h["k"] == np.float32(1.0 + m) and h["max_rho"] == 20
            else:
                assert h["km_num"] == 0 and h["k"] == 0
    finally:
        lib.rebvo_net_packet_ring_free(ring)
