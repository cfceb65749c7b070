#!/usr/bin/env python3
"""Generate tests/golden/depth_surface/*.npz from the REFERENCE's own depth_filler (src/visualizer/depth_filler.cpp).

Build machine only (needs the reference tree and oracle/_ref/libreforacle.so from `make -C oracle`):
    python tools/make_depth_surface_golden.py [--ref /path/to/reference]

The reference's depth_filler.cpp is compiled in place, together with tools/depth_surface_ref_driver.cpp, into a temporary directory
outside the repository, with the flags and prelude of tools/make_depth_fill_golden.py.  The KeyLine lists and fill cases are the
ones stored in tests/golden/depth_fill/*.npz; the camera is edgehip.euroc_params(w, h)'s (what the GPU tests' contexts use).
Per case a fixture (tests/golden/depth_surface/<w>x<h>_case<i>.npz, case i of the depth_fill fixture) stores point, dist, min_dist, normal and area (a NaN sentinel marks the cells the reference never writes).
Depth images (getImgRho and getImgRhoTriInterp, rho and s_rho): whole for two 376x240 cases, and for 752x480 a seeded sample of
pixels plus the four border rows and columns.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rebvo_amd import edgehip  # noqa: E402
from tools.make_depth_fill_golden import FIELDS, PRELUDE  # noqa: E402

SENTINEL64 = 0x7FF4DEADBEEF0001   # tools/depth_surface_ref_driver.cpp
SENTINEL32 = 0x7FA0DEAD
IMAGE_CASES_SMALL = (0, 2)        # 10x10 blocks; 7x7 blocks (partial column and row)


def build_driver(ref, tmp):
    inc = os.path.join(ROOT, "oracle", "_ref", "inc")
    lib = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(lib, "libreforacle.so")):
        raise SystemExit("oracle/_ref/libreforacle.so is missing: run `make -C oracle` first")
    pre = os.path.join(tmp, "prelude.h")
    with open(pre, "w") as f:
        f.write(PRELUDE)
    exe = os.path.join(tmp, "ds_driver")
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-access-control", "-w", "-include", pre,
           "-I" + inc, "-I" + os.path.join(ref, "include"), "-I" + ref,
           os.path.join(ROOT, "tools", "depth_surface_ref_driver.cpp"), os.path.join(ref, "src", "visualizer", "depth_filler.cpp"),
           "-L" + lib, "-Wl,-rpath," + lib, "-lreforacle", "-lm", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def camera(w, h):
    p = edgehip.euroc_params(w, h)
    return np.array([p.ppx, p.ppy, p.zfx, p.zfy], np.float32)


def to_records(fields):
    kl = np.zeros(len(fields["rho"]), edgehip.KEYLINE_DTYPE)
    for f in FIELDS:
        kl[f] = fields[f]
    return kl


def run_ref(exe, kl, w, h, bw, bh, iter_num, mode, discard, v_thresh, m_num_t, pix):
    hdr = np.array([w, h, bw, bh, iter_num, mode, discard, m_num_t], np.int32).tobytes()
    pix = np.ascontiguousarray(pix, np.int32).reshape(-1, 2)
    payload = (hdr + np.float64(v_thresh).tobytes() + camera(w, h).tobytes() + np.int32(len(kl)).tobytes()
               + np.ascontiguousarray(kl).tobytes() + np.int32(len(pix)).tobytes() + pix.tobytes())
    out = subprocess.run([exe], input=payload, check=True, capture_output=True).stdout
    gw, gh = w // bw, h // bh
    n, m = gw * gh, len(pix)
    assert len(out) == 8 * (7 * n + 1) + 4 * n + 32 * m, (len(out), n, m)
    o = 0

    def take(dtype, count, shape):
        nonlocal o
        a = np.frombuffer(out, dtype, count, o).reshape(shape).copy()
        o += np.dtype(dtype).itemsize * count
        return a

    rec = dict(point=take(np.float64, 3 * n, (gh, gw, 3)), dist=take(np.float64, n, (gh, gw)), min_dist=take(np.float64, 1, ())[()],
               normal=take(np.float64, 3 * n, (gh, gw, 3)), area=take(np.float32, n, (gh, gw)))
    img = take(np.float64, 4 * m, (4, m))
    assert np.array_equal(img.astype(np.float32).astype(np.float64), img, equal_nan=True)   # float results: exact in float32
    rec["image"] = img.astype(np.float32)   # rho1, s_rho1, rho2, s_rho2 at the pixels
    return rec


def sample_pixels(w, h, n, seed):
    rng = np.random.default_rng(seed)
    px = rng.integers(0, w, n)
    py = rng.integers(0, h, n)
    xs, ys = np.arange(w), np.arange(h)
    border = np.concatenate([np.stack([xs, np.zeros_like(xs)], 1), np.stack([xs, np.full_like(xs, h - 1)], 1),
                             np.stack([np.zeros_like(ys), ys], 1), np.stack([np.full_like(ys, w - 1), ys], 1)])
    return np.concatenate([np.stack([px, py], 1), border]).astype(np.int32)


def write(gold, exe, src, full_image_cases, n_sample):
    """One file per case, <res>_case<i>.npz, and one per whole image and mode, <res>_case<i>_image<mode>.npz: each stays under the
    size limit of a committed file."""
    z = np.load(src)
    w, h = int(z["w"]), int(z["h"])
    sample = sample_pixels(w, h, n_sample, seed=w * h)
    for i, (lst, bw, bh, it, mode, disc, m) in enumerate(z["cases"]):
        kl = to_records({f: z[f"kl{chr(lst)}_{f}"] for f in FIELDS})
        full = i in full_image_cases
        pix = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2) if full else sample
        r = run_ref(exe, kl, w, h, int(bw), int(bh), int(it), int(mode), int(disc), float(z[f"case{i}_thresh_rel_rho"]), int(m), pix)
        rec = {"w": np.int32(w), "h": np.int32(h), "cam": camera(w, h), "case": np.int32(i)}
        for k in ("point", "dist", "min_dist", "normal", "area"):
            rec[k] = r[k]
        if not full and n_sample:
            rec["sample"], rec["image"] = sample, r["image"]
        base = os.path.join(gold, f"{w}x{h}_case{i}")
        np.savez_compressed(base + ".npz", **rec)
        sizes = [os.path.getsize(base + ".npz")]
        if full:
            img = r["image"].reshape(4, h, w)
            for md in (1, 2):
                np.savez_compressed(f"{base}_image{md}.npz", rho=img[2 * md - 2], s_rho=img[2 * md - 1])
                sizes.append(os.path.getsize(f"{base}_image{md}.npz"))
        unwritten = int((r["area"].view(np.uint32) == SENTINEL32).sum())
        print(f"{w}x{h} case {i}: grid {w // bw}x{h // bh}, min_dist {r['min_dist']:.6g}, {unwritten} cells without area, "
              f"{'whole image' if full else f'{len(pix)} pixels'}; bytes {sizes}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF", "/root/reference"))
    a = ap.parse_args()
    src = os.path.join(ROOT, "tests", "golden", "depth_fill")
    gold = os.path.join(ROOT, "tests", "golden", "depth_surface")   # a subdirectory: tests/golden/*.npz are the pipeline fixtures
    os.makedirs(gold, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="depth_surface_ref_") as tmp:
        exe = build_driver(a.ref, tmp)
        write(gold, exe, os.path.join(src, "376x240.npz"), IMAGE_CASES_SMALL, 0)
        write(gold, exe, os.path.join(src, "752x480.npz"), (), 4000)


if __name__ == "__main__":
    main()
