#!/usr/bin/env python3
"""Fixtures of the JPEG decoder (tests/golden/jpeg_decode/*.npz): a stream as PIL (libjpeg-turbo) wrote it, the pixels PIL decodes it to,
and the name of its sampling.  Needs PIL and the built host library (rebvo_amd/lib/librebvohost.so); run from anywhere:
    python tools/make_jpeg_decode_golden.py

The tool refuses to write a set in which the host reader (rebvo_decode_jpeg) differs from PIL on any file, and one that lacks a
population the tests rely on; it counts the populations with the host instantiation of the device's chain walk
(rebvo_jpeg_decode_staged), whose pixels it holds to PIL as well."""
import ctypes as C
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_decode")
STATS = ("long_codes", "zrl", "no_eob", "max_dc_cat", "max_ac_cat", "blocks", "stuffed", "groups")
SAMPLING = {"grey": None, "444": 0, "422": 1, "420": 2}
SIZES = ((1, 1), (8, 8), (17, 33), (24, 40), (50, 70), (150, 200))


def host():
    lib = C.CDLL(os.path.join(ROOT, "rebvo_amd", "lib", "librebvohost.so"))
    lib.rebvo_decode_jpeg.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    lib.rebvo_jpeg_decode_staged.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong] + [C.c_void_p] * 5
    return lib


def staged(lib, stream, w, h):
    """the three stages on the CPU -> (reason, status, rgb, {population: count})"""
    stream = np.ascontiguousarray(stream, np.uint8)
    rgb = np.zeros((h, w, 3), np.uint8)
    st, status, groups = np.zeros(6, np.int64), C.c_int(-1), C.c_int(0)
    reason = lib.rebvo_jpeg_decode_staged(stream.ctypes.data, len(stream), rgb.ctypes.data, rgb.size, None, None, C.addressof(status),
                                          st.ctypes.data, C.addressof(groups))
    pop = dict(zip(STATS, [int(v) for v in st] + [stream.tobytes().count(b"\xff\x00"), groups.value]))
    return reason, status.value, rgb, pop


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth(w, h, seed):
    y, x = np.mgrid[0:h, 0:w]
    ch = [(x * 255) // max(w - 1, 1), 255 - (y * 255) // max(h - 1, 1), ((x + 2 * y) // 3 + 37 * seed) % 256]
    return np.stack(ch, -1).astype(np.uint8)


def saturated(w, h, seed):
    rng = np.random.default_rng(100 + seed)
    widths = rng.integers(1, 6, w + h + 8)
    col = np.repeat(rng.integers(0, 8, len(widths)), widths)[: w + h + 8]
    idx = col[(np.arange(w)[None, :] + (np.arange(h)[:, None] // 3)) % len(col)]
    return np.stack([(idx & 1) * 255, ((idx >> 1) & 1) * 255, ((idx >> 2) & 1) * 255], -1).astype(np.uint8)


def mosaic(w, h, seed):
    """16 x 16 tiles of random colours on the MCU grid: the decoded image deflates well, which the largest size needs"""
    rng = np.random.default_rng(200 + seed)
    t = rng.integers(0, 256, ((h + 15) // 16, (w + 15) // 16, 3), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(t, 16, 0), 16, 1)[:h, :w])


def checker(w, h):
    y, x = np.mgrid[0:h, 0:w]
    v = (((x // 8) + (y // 8)) & 1) * 255
    return np.stack([v, v, v], -1).astype(np.uint8)


def stripes2(w, h):
    y, x = np.mgrid[0:h, 0:w]
    v = (x & 1) * 255
    return np.stack([v, v, v], -1).astype(np.uint8)


def main():
    from PIL import Image, features
    if not features.check_feature("libjpeg_turbo"):
        sys.exit("PIL without libjpeg-turbo: its pixels are not the ones these fixtures pin down")
    lib = host()
    cases = []   # (name, rgb, sampling, save keywords)
    makers = (noise, saturated, smooth)
    for k, (w, h) in enumerate(SIZES):
        for j, samp in enumerate(SAMPLING):
            f = makers[(k + j) % 3] if (w, h) != (150, 200) else (saturated if samp == "422" else mosaic)
            cases.append((f"{f.__name__}_{w}x{h}_{samp}_q90", f(w, h, k + j), samp, dict(quality=90)))
    for q, samp in ((1, "420"), (10, "422"), (50, "444"), (100, "420"), (100, "grey")):
        cases.append((f"noise_24x40_{samp}_q{q}", noise(24, 40, 30 + q), samp, dict(quality=q)))
    for samp in SAMPLING:   # optimised Huffman tables (the others carry Annex K's)
        cases.append((f"saturated_50x70_{samp}_q90_opt", saturated(50, 70, 9), samp, dict(quality=90, optimize=True)))
    cases.append(("noise_24x40_420_q50_opt", noise(24, 40, 41), "420", dict(quality=50, optimize=True)))
    # restart intervals: 1, 3 (20 MCUs: it does not divide them), 7, one MCU row; 130 intervals of one MCU make five groups of 32
    cases.append(("noise_50x70_420_q90_dri1", noise(50, 70, 50), "420", dict(quality=90, restart_marker_blocks=1)))
    cases.append(("noise_50x70_420_q90_dri3", noise(50, 70, 51), "420", dict(quality=90, restart_marker_blocks=3)))
    cases.append(("noise_50x70_444_q90_dri7", noise(50, 70, 52), "444", dict(quality=90, restart_marker_blocks=7)))
    cases.append(("noise_50x70_422_q90_drirow", noise(50, 70, 53), "422", dict(quality=90, restart_marker_rows=1)))
    cases.append(("saturated_50x70_grey_q90_dri3", saturated(50, 70, 54), "grey", dict(quality=90, restart_marker_blocks=3)))
    cases.append(("mosaic_150x200_420_q90_dri1", mosaic(150, 200, 55), "420", dict(quality=90, restart_marker_blocks=1)))
    cases.append(("mosaic_150x200_420_q90_drirow", mosaic(150, 200, 56), "420", dict(quality=90, restart_marker_rows=1, optimize=True)))
    cases.append(("checker_48x40_420_q100", checker(48, 40), "420", dict(quality=100)))
    cases.append(("stripes2_40x24_420_q100", stripes2(40, 24), "420", dict(quality=100)))
    cases.append(("stripes2_40x24_grey_q100", stripes2(40, 24), "grey", dict(quality=100)))
    # the size of the tests' contexts, one component: the 8-bit slot path (one stream without DRI, one with an MCU row per interval)
    cases.append(("mosaic_256x192_grey_q90", mosaic(256, 192, 57), "grey", dict(quality=90)))
    cases.append(("mosaic_256x192_grey_q90_drirow", mosaic(256, 192, 58), "grey", dict(quality=90, restart_marker_rows=1)))
    cases.append(("mosaic_256x192_progressive", mosaic(256, 192, 59), "progressive", dict(quality=90, progressive=True)))
    cases.append(("smooth_17x33_progressive", smooth(17, 33, 3), "progressive", dict(quality=90, progressive=True)))

    os.makedirs(OUT, exist_ok=True)
    total, pop, bad = 0, {k: 0 for k in STATS}, []
    have = set()
    for name, rgb, samp, kw in cases:
        h, w = rgb.shape[:2]
        buf = io.BytesIO()
        if samp == "grey":
            Image.fromarray(rgb, "RGB").convert("L").save(buf, "JPEG", **kw)
        else:
            Image.fromarray(rgb, "RGB").save(buf, "JPEG", subsampling=SAMPLING.get(samp, 2), **kw)
        stream = np.frombuffer(buf.getvalue(), np.uint8)
        ref = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")))
        mine = np.zeros_like(ref)
        if lib.rebvo_decode_jpeg(stream.ctypes.data, len(stream), mine.ctypes.data, mine.size, None, None) != 0 or not np.array_equal(mine, ref):
            bad.append(name + ": host reader")
        reason, status, px, st = staged(lib, stream, w, h)
        if samp == "progressive":
            if reason != 2:
                bad.append(name + f": reason {reason}")
        else:
            if reason or status or not np.array_equal(px, ref):
                bad.append(name + f": staged decoder (reason {reason}, status {status})")
            for k in STATS:
                pop[k] = max(pop[k], st[k])
            have.add((samp, w, h))
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, jpeg=stream, rgb=ref, sampling=np.frombuffer(samp.encode(), np.uint8),
                            stats=np.array([st[k] for k in STATS], np.int64))
        total += os.path.getsize(path)
    print(f"{len(cases)} fixtures, {total} bytes; largest per file: {pop}")
    assert not bad, bad
    assert all((s, w, h) in have for s in SAMPLING for w, h in SIZES)
    assert pop["stuffed"] >= 5 and pop["long_codes"] >= 1 and pop["zrl"] >= 1 and pop["no_eob"] >= 1, pop
    assert pop["max_dc_cat"] == 11 and pop["max_ac_cat"] == 10, pop
    assert pop["groups"] >= 4, pop
    assert total < 400 * 1024, total


if __name__ == "__main__":
    main()
