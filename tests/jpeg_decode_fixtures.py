"""Shared by the JPEG decoder's tests: the fixtures of tools/make_jpeg_decode_golden.py (a stream as PIL wrote it, the pixels PIL decodes
it to, its sampling, the populations the tool counted), the CPU form of the device decoder in librebvohost.so (rebvo_jpeg_probe,
rebvo_jpeg_decode_staged) and the two corrupt streams both the CPU guard program and the device test use."""
import ctypes as C
import functools
import glob
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "jpeg_decode")
HOST = os.path.join(ROOT, "rebvo_amd", "lib", "librebvohost.so")
STATS = ("long_codes", "zrl", "no_eob", "max_dc_cat", "max_ac_cat", "blocks", "stuffed", "groups")
INFO = np.dtype([("w", "<i4"), ("h", "<i4"), ("components", "<i4"), ("hsamp", "<i4"), ("vsamp", "<i4"), ("restart_interval", "<i4"),
                 ("entropy_offset", "<u4"), ("entropy_length", "<u4"), ("reason", "<i4")])
SAMPLING = {"grey": (1, 1, 1), "444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2)}   # components, hsamp, vsamp
SIZES = ((1, 1), (8, 8), (17, 33), (24, 40), (50, 70), (150, 200))
# the parser's reason codes (rebvo/jpeg_decode.h)
OK, TRUNCATED, PROGRESSIVE, CODING, PRECISION, COMPONENTS, SAMPLING_REASON, MULTISCAN, COLOURSPACE, TABLE, HEADER, SIZE, TOO_LONG = range(13)


@functools.lru_cache(maxsize=None)
def fixtures():
    """-> {name: dict(jpeg (uint8), rgb (h, w, 3) as PIL decodes it, sampling, stats {name: count})}, read once, read-only."""
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLD, "*.npz"))):
        z = np.load(path)
        for a in (z["rgb"], z["jpeg"]):
            a.setflags(write=False)
        out[os.path.basename(path)[:-4]] = dict(jpeg=z["jpeg"], rgb=z["rgb"], sampling=z["sampling"].tobytes().decode(),
                                                stats=dict(zip(STATS, (int(v) for v in z["stats"]))))
    return out


def decodable():
    """the fixtures the device takes (all but the progressive one)"""
    return {n: f for n, f in fixtures().items() if f["sampling"] in SAMPLING}


def of_size(w, h):
    return sorted(n for n, f in decodable().items() if f["rgb"].shape[:2] == (h, w))


@functools.lru_cache(maxsize=None)
def host_lib():
    lib = C.CDLL(HOST)
    lib.rebvo_jpeg_probe.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p]
    lib.rebvo_jpeg_probe_expect.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_uint, C.c_void_p]
    lib.rebvo_jpeg_decode_staged.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong] + [C.c_void_p] * 5
    lib.rebvo_decode_jpeg.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    return lib


def probe(stream, expect=None, cap=0):
    """the shared parser -> dict of INFO's fields; expect = (w, h), cap: with the size and cap check every caller with a frame size of
    its own applies (jpegdec::expect, as edgehip_upload_jpeg does)"""
    stream = np.ascontiguousarray(stream, np.uint8)
    info = np.zeros((), INFO)
    if expect is None:
        rc = host_lib().rebvo_jpeg_probe(stream.ctypes.data if stream.size else None, len(stream), info.ctypes.data)
    else:
        rc = host_lib().rebvo_jpeg_probe_expect(stream.ctypes.data if stream.size else None, len(stream), int(expect[0]), int(expect[1]),
                                                C.c_uint(int(cap)), info.ctypes.data)
    assert rc == int(info["reason"])
    return {k: int(info[k]) for k in INFO.names}


def staged(stream, shape):
    """parser + host chain walk + the pixel stage's restatement -> (reason, status, rgb (h, w, 3), groups)"""
    stream = np.ascontiguousarray(stream, np.uint8)
    rgb = np.zeros(tuple(shape[:2]) + (3,), np.uint8)
    status, groups = C.c_int(-1), C.c_int(0)
    reason = host_lib().rebvo_jpeg_decode_staged(stream.ctypes.data, len(stream), rgb.ctypes.data, rgb.size, None, None, C.addressof(status), None,
                                                 C.addressof(groups))
    return reason, status.value, rgb, groups.value


def host_decode(stream):
    """the library's own JPEG reader (rebvo_decode_jpeg) -> (h, w, 3) uint8"""
    stream = np.ascontiguousarray(stream, np.uint8)
    w, h = C.c_int(0), C.c_int(0)
    assert host_lib().rebvo_decode_jpeg(stream.ctypes.data, len(stream), None, 0, C.byref(w), C.byref(h)) == 0
    out = np.zeros((h.value, w.value, 3), np.uint8)
    assert host_lib().rebvo_decode_jpeg(stream.ctypes.data, len(stream), out.ctypes.data, out.size, None, None) == 0
    return out


CORRUPT_SOURCE = "noise_50x70_422_q90"


@functools.lru_cache(maxsize=None)
def corrupt_pair():
    """(truncated, flipped): CORRUPT_SOURCE cut in the middle of its entropy-coded segment, and with one byte of the segment inverted —
    the first byte from a third of the segment on whose inversion the host chain walk notices (many do not: Huffman codes resynchronise).
    tests/test_jpeg_decode_cpu.py puts both through tools/jpeg_entropy_guard.cpp (in bounds, nonzero status) before any device sees them."""
    f = fixtures()[CORRUPT_SOURCE]
    s = f["jpeg"]
    info = probe(s)
    cut = info["entropy_offset"] + info["entropy_length"] // 2
    for at in range(info["entropy_offset"] + info["entropy_length"] // 3, cut):
        flipped = s.copy()
        flipped[at] ^= 0xFF
        reason, status, _, _ = staged(flipped, f["rgb"].shape)
        if reason == 0 and status != 0 and flipped[at] != 0xFF:   # (an FF would be a marker: that is the truncated case again)
            return s[:cut].copy(), flipped
    raise AssertionError("no inverted byte is noticed")


def corrupt_slot_stream():
    """a one-component stream of the tests' context size cut in the middle of its entropy-coded segment (the guard program walks it too)"""
    s = fixtures()["mosaic_256x192_grey_q90"]["jpeg"]
    info = probe(s)
    return s[:info["entropy_offset"] + info["entropy_length"] // 2].copy()


def sampling_440_of(stream_422):
    """a 4:2:2 file's frame header rewritten to 4:4:0 (no encoder at hand writes one): for the parser's reason code only"""
    s = np.array(stream_422, np.uint8)
    b = s.tobytes()
    at = b.index(b"\xff\xc0")
    assert s[at + 11] == 0x21   # Y: h = 2, v = 1
    s[at + 11] = 0x12
    return s
