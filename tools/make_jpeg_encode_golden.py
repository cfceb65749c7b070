#!/usr/bin/env python3
"""Fixtures of the JPEG encoder (tests/golden/jpeg_encode/*.npz): input RGB, quality, comment and the complete file libjpeg writes for
them, taken from PIL (libjpeg-turbo) at the settings gd's gdImageJpegPtr leaves libjpeg with: baseline, 4:2:0, Annex-K Huffman tables,
the islow DCT.  Needs PIL and the built host library (rebvo_amd/lib/librebvohost.so); run from anywhere:  python tools/make_jpeg_encode_golden.py

The tool also counts, with the host encoder's own pass over its symbols, what the streams exercise, and refuses to write a set that
lacks one of the populations the tests rely on (stuffed bytes, ZRL, a block without EOB, the largest categories, dummy blocks, odd sizes)."""
import ctypes as C
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_encode")
STATS = ("stuffed", "zrl", "no_eob", "max_dc_cat", "max_ac_cat", "dummy_right", "dummy_bottom", "blocks")


def host_encoder():
    lib = C.CDLL(os.path.join(ROOT, "rebvo_amd", "lib", "librebvohost.so"))
    lib.rebvo_encode_jpeg.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.rebvo_encode_jpeg.restype = C.c_longlong

    def encode(rgb, quality, comment=None):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        h, w = rgb.shape[:2]
        st = np.zeros(8, np.int64)
        n = lib.rebvo_encode_jpeg(rgb.ctypes.data, w, h, quality, comment, None, 0, st.ctypes.data)
        assert n > 0, (w, h, quality)
        out = np.zeros(n, np.uint8)
        assert lib.rebvo_encode_jpeg(rgb.ctypes.data, w, h, quality, comment, out.ctypes.data, n, None) == n
        return out, dict(zip(STATS, (int(v) for v in st)))
    return encode


def noise(w, h, seed):
    """uniform noise; the largest size in 16 levels only (half the bytes after deflate: the fixture set has a size budget)"""
    rng = np.random.default_rng(seed)
    if w * h > 10000:
        return (rng.integers(0, 16, (h, w, 3)) * 17).astype(np.uint8)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth(w, h, seed):
    """integer ramps along x, along y and along a diagonal"""
    y, x = np.mgrid[0:h, 0:w]
    ch = [(x * 255) // max(w - 1, 1), 255 - (y * 255) // max(h - 1, 1), ((x + 2 * y) // 3 + 37 * seed) % 256]
    return np.stack(ch, -1).astype(np.uint8)


def saturated(w, h, seed):
    """stripes of the eight corner colours, 1 to 5 px wide, turned by the row"""
    rng = np.random.default_rng(100 + seed)
    widths = rng.integers(1, 6, w + h + 8)
    col = np.repeat(rng.integers(0, 8, len(widths)), widths)[: w + h + 8]
    idx = col[(np.arange(w)[None, :] + (np.arange(h)[:, None] // 3)) % len(col)]
    return np.stack([(idx & 1) * 255, ((idx >> 1) & 1) * 255, ((idx >> 2) & 1) * 255], -1).astype(np.uint8)


def checker(w, h):
    """8x8 blocks alternately 0 and 255: DC differences of the largest category at quality 100"""
    y, x = np.mgrid[0:h, 0:w]
    v = (((x // 8) + (y // 8)) & 1) * 255
    return np.stack([v, v, v], -1).astype(np.uint8)


def stripes2(w, h):
    """period-2 stripes: the whole energy of a block in one AC coefficient (category 10 at quality 100)"""
    y, x = np.mgrid[0:h, 0:w]
    v = (x & 1) * 255
    return np.stack([v, v, v], -1).astype(np.uint8)


def main():
    from PIL import Image, features
    if not features.check_feature("libjpeg_turbo"):
        sys.exit("PIL without libjpeg-turbo: its stream is not the one these fixtures pin down")
    from rebvo_amd import synth
    encode = host_encoder()
    cases = []   # (name, rgb, quality, comment)
    makers = (("noise", noise), ("smooth", smooth), ("saturated", saturated))
    for k, (w, h) in enumerate(((1, 1), (8, 8), (17, 33), (24, 40), (50, 70), (150, 200))):
        for name, f in makers:
            cases.append((f"{name}_{w}x{h}_q90", f(w, h, k), 90, None))
    for w, h, name, f in ((24, 40, "noise", noise), (150, 200, "saturated", saturated)):
        for q in (1, 10, 50, 100):
            cases.append((f"{name}_{w}x{h}_q{q}", f(w, h, 7), q, None))
    # further contents of the sizes above, for batches of one size with different images (3 and 7)
    for i in range(6):
        cases.append((f"batch{i}_24x40_q90", (noise, smooth, saturated)[i % 3](24, 40, 20 + i), 90, None))
    frame = next(iter(synth.billboard_sequence(256, 192, 1)))[0]
    cases.append(("billboard_256x192_q90", np.ascontiguousarray(frame.reshape(192, 256, 3)), 90, None))
    cases.append(("checker_48x40_q100", checker(48, 40), 100, None))
    cases.append(("stripes2_40x24_q100", stripes2(40, 24), 100, None))
    cases.append(("comment_17x33_q90", smooth(17, 33, 3), 90, b"CREATOR: gd-jpeg v1.0 (using IJG JPEG v62), quality = 90\n"))

    os.makedirs(OUT, exist_ok=True)
    total, pop, agree = 0, {k: 0 for k in STATS}, 0
    sizes = set()
    for name, rgb, q, comment in cases:
        h, w = rgb.shape[:2]
        buf = io.BytesIO()
        kw = {"comment": comment} if comment else {}
        Image.fromarray(rgb, "RGB").save(buf, "JPEG", quality=q, subsampling=2, optimize=False, **kw)
        ref = np.frombuffer(buf.getvalue(), np.uint8)
        mine, st = encode(rgb, q, comment)
        agree += int(np.array_equal(ref, mine))
        if not np.array_equal(ref, mine):
            print(f"  {name}: host encoder differs from PIL ({len(mine)} vs {len(ref)} bytes)")
        for k in STATS:
            pop[k] = max(pop[k], st[k])
        sizes.add((w, h))
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, rgb=rgb, quality=np.int32(q), jpeg=ref, comment=np.frombuffer(comment or b"", np.uint8),
                            stats=np.array([st[k] for k in STATS], np.int64))
        total += os.path.getsize(path)
    print(f"{len(cases)} fixtures, {total} bytes, host encoder equal to PIL on {agree}; largest per file: {pop}")
    # the populations the tests rely on, on the reference stream (the host encoder's symbol pass counts them; it equals PIL's bytes)
    assert agree == len(cases), "the host encoder must reproduce every stream before its symbol counts mean anything"
    assert pop["stuffed"] >= 20 and pop["zrl"] >= 1 and pop["no_eob"] >= 1, pop
    assert pop["max_dc_cat"] == 11 and pop["max_ac_cat"] == 10, pop
    assert pop["dummy_right"] >= 1 and pop["dummy_bottom"] >= 1, pop
    assert any(w & 1 for w, _ in sizes) and any(h & 1 for _, h in sizes)
    assert any(h % 2 == 0 and h % 16 != 0 for _, h in sizes)
    assert total < 400 * 1024, total


if __name__ == "__main__":
    main()
