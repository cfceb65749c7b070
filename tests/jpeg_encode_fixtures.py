"""Shared by the JPEG encoder's tests: the fixtures of tools/make_jpeg_encode_golden.py (input RGB, quality, comment, libjpeg's complete
file as PIL wrote it, the populations the tool counted) and the host encoder rebvo_encode_jpeg of librebvohost.so."""
import ctypes as C
import functools
import glob
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "jpeg_encode")
HOST = os.path.join(ROOT, "rebvo_amd", "lib", "librebvohost.so")
STATS = ("stuffed", "zrl", "no_eob", "max_dc_cat", "max_ac_cat", "dummy_right", "dummy_bottom", "blocks")
HEADER_BYTES = 623
# the reference's net_packet_hdr (include/CommLib/net_keypoint.h:64-78, packed) with its compressed_nav_pkg
NAV = [("Pos", "<f4", (3,)), ("Pose", "<f4", (3,)), ("Rot", "<f4", (3,)), ("Vel", "<f4", (3,)), ("G", "<f4", (3,)), ("K", "<f4"), ("dt", "<f4")]
HDR = np.dtype([("data_size", "<i4"), ("w", "<i4"), ("h", "<i4"), ("key_num", "<i4"), ("jpeg_size", "<i4"), ("encoder_type", "<i4"),
                ("kline_num", "<i4"), ("km_num", "<i4"), ("k", "<f4"), ("max_rho", "<f4"), ("nav", NAV)])


@functools.lru_cache(maxsize=None)
def fixtures():
    """-> {name: dict(rgb (h, w, 3), quality, jpeg (uint8), comment (bytes or None), stats {name: count})}, read once."""
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLD, "*.npz"))):
        z = np.load(path)
        comment = z["comment"].tobytes()
        for a in (z["rgb"], z["jpeg"]):
            a.setflags(write=False)
        out[os.path.basename(path)[:-4]] = dict(rgb=z["rgb"], quality=int(z["quality"]), jpeg=z["jpeg"], comment=comment or None,
                                                stats=dict(zip(STATS, (int(v) for v in z["stats"]))))
    return out


@functools.lru_cache(maxsize=None)
def host_lib():
    lib = C.CDLL(HOST)
    lib.rebvo_encode_jpeg.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.rebvo_encode_jpeg.restype = C.c_longlong
    lib.rebvo_decode_jpeg.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    lib.rebvo_decode_jpeg.restype = C.c_int
    return lib


def host_encode(rgb, quality, comment=None):
    """rebvo_encode_jpeg -> (stream as uint8 array, {population: count})"""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    st = np.zeros(8, np.int64)
    n = host_lib().rebvo_encode_jpeg(rgb.ctypes.data, w, h, int(quality), comment, None, 0, st.ctypes.data)
    assert n > 0, (w, h, quality)
    out = np.zeros(n, np.uint8)
    assert host_lib().rebvo_encode_jpeg(rgb.ctypes.data, w, h, int(quality), comment, out.ctypes.data, n, None) == n
    return out, dict(zip(STATS, (int(v) for v in st)))


def host_decode(stream):
    """the library's own JPEG reader on a stream in memory -> (h, w, 3) uint8"""
    stream = np.ascontiguousarray(stream, np.uint8)
    w, h = C.c_int(0), C.c_int(0)
    assert host_lib().rebvo_decode_jpeg(stream.ctypes.data, len(stream), None, 0, C.byref(w), C.byref(h)) == 0
    out = np.zeros((h.value, w.value, 3), np.uint8)
    assert host_lib().rebvo_decode_jpeg(stream.ctypes.data, len(stream), out.ctypes.data, out.size, None, None) == 0
    return out


def first_difference(a, b):
    """for assertion messages: (len a, len b, index of the first differing byte or None)"""
    n = min(len(a), len(b))
    d = np.flatnonzero(np.asarray(a[:n]) != np.asarray(b[:n]))
    return len(a), len(b), (int(d[0]) if len(d) else None)
