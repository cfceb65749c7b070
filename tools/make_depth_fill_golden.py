#!/usr/bin/env python3
"""Generate tests/golden/depth_fill/*.npz from the REFERENCE's own depth_filler (src/visualizer/depth_filler.cpp).

Build machine only (needs the reference tree and oracle/_ref/libreforacle.so from `make -C oracle`):
    python tools/make_depth_fill_golden.py [--ref /path/to/reference]

The reference's depth_filler.cpp is compiled in place, together with tools/depth_fill_ref_driver.cpp, into a temporary directory
outside the repository (nothing is written under oracle/, no reference source is copied).  The KeyLine lists are what the reference
oracle's own replay of synth.billboard_sequence leaves in its newest slot after 9+ frames (a real share of them reach m_num >= 5).
Each fixture stores the fields the fill reads (c_p, rho, s_rho, rho0, m_num, p_id, n_id) and, per case, the parameters and the
reference's output grids (rho, s_rho, fixed).
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402
from rebvo_amd import synth  # noqa: E402

FIELDS = ("c_p", "rho", "s_rho", "rho0", "m_num", "p_id", "n_id")
# A pre-included header: depth_filler.h's inline interpolation helpers (not on the fill path) call std::max(float, double), which
# this C++ library does not resolve on its own.
PRELUDE = "#include <algorithm>\nnamespace std { inline double max(float a, double b) { return max((double)a, b); } }\n"

# (list, bw, bh, iter_num, bound_mode, discard, thresh_rel_rho, thresh_match_num)
CASES_SMALL = [
    ("A", 10, 10, 10, 0, 1, 1.0, 5),   # the visualizer's blocks; 376 % 10 != 0: a partial column (x == gw wraps to the next row)
    ("A", 5, 5, 10, 0, 1, 1.0, 5),     # the key-frame viewer's blocks
    ("A", 7, 7, 10, 0, 1, 1.0, 5),     # partial column and partial row (the last row's overflow is dropped)
    ("A", 10, 10, 10, 1, 1, 1.0, 5),
    ("A", 10, 10, 10, 2, 0, 1.0, 5),
    ("A", 5, 5, 1, 2, 0, 1.0, 5),
    ("A", 10, 10, 0, 1, 0, 1.0, 5),
    ("A", 5, 5, 10, 1, 0, 2.0, 2),
    ("B", 10, 5, 10, 0, 1, 1.0, 5),
    ("B", 8, 8, 10, 2, 1, 1.0, 5),
    ("B", 10, 10, 10, 0, 1, 0.5, 0),
    ("B", 5, 5, 10, 1, 0, 1.0, 5),
    ("E", 10, 10, 10, 0, 1, 1.0, 5),   # empty list: rho 1, s_rho 40 everywhere
    ("E", 5, 5, 10, 2, 0, 1.0, 5),
]
CASES_LARGE = [
    ("C", 10, 10, 10, 0, 1, 1.0, 5),
    ("C", 5, 5, 10, 0, 1, 1.0, 5),
]


def build_driver(ref, tmp):
    inc = os.path.join(ROOT, "oracle", "_ref", "inc")
    lib = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(lib, "libreforacle.so")):
        raise SystemExit("oracle/_ref/libreforacle.so is missing: run `make -C oracle` first")
    pre = os.path.join(tmp, "prelude.h")
    with open(pre, "w") as f:
        f.write(PRELUDE)
    exe = os.path.join(tmp, "df_driver")
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-access-control", "-w", "-include", pre,
           "-I" + inc, "-I" + os.path.join(ref, "include"), "-I" + ref,
           os.path.join(ROOT, "tools", "depth_fill_ref_driver.cpp"), os.path.join(ref, "src", "visualizer", "depth_filler.cpp"),
           "-L" + lib, "-Wl,-rpath," + lib, "-lreforacle", "-lm", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run_ref(exe, kl, w, h, bw, bh, iter_num, mode, discard, v_thresh, m_num_t):
    hdr = np.array([w, h, bw, bh, iter_num, mode, discard, m_num_t], np.int32).tobytes()
    payload = hdr + np.float64(v_thresh).tobytes() + np.int32(len(kl)).tobytes() + np.ascontiguousarray(kl).tobytes()
    out = subprocess.run([exe], input=payload, check=True, capture_output=True).stdout
    gw, gh = w // bw, h // bh
    n = gw * gh
    assert len(out) == 17 * n, (len(out), n)
    rho = np.frombuffer(out, np.float64, n, 0).reshape(gh, gw)
    s_rho = np.frombuffer(out, np.float64, n, 8 * n).reshape(gh, gw)
    fixed = np.frombuffer(out, np.uint8, n, 16 * n).reshape(gh, gw)
    return rho.copy(), s_rho.copy(), fixed.copy()


def replay_lists(w, h, frames_at):
    """KeyLine lists of the reference oracle's newest slot after the frames numbered in frames_at."""
    orc = oracle.Oracle("ref", oracle.euroc_params(w, h))
    out = {}
    for k, (f, _, _) in enumerate(synth.billboard_sequence(w, h, max(frames_at) + 1)):
        orc.process_frame(f, 0.05 * k)
        if k in frames_at:
            out[k] = orc.keylines(orc.cur_slot()).copy()
    orc.close()
    return out


def write(path, exe, w, h, lists, cases):
    rec = {"w": np.int32(w), "h": np.int32(h)}
    for name, kl in lists.items():
        for f in FIELDS:
            rec[f"kl{name}_{f}"] = np.ascontiguousarray(kl[f])
    params = []
    for i, (name, bw, bh, it, mode, disc, v, m) in enumerate(cases):
        rho, s_rho, fixed = run_ref(exe, lists[name], w, h, bw, bh, it, mode, disc, v, m)
        rec[f"case{i}_rho"], rec[f"case{i}_s_rho"], rec[f"case{i}_fixed"] = rho, s_rho, fixed
        params.append((ord(name), bw, bh, it, mode, disc, m))
        rec[f"case{i}_thresh_rel_rho"] = np.float64(v)
        print(f"{os.path.basename(path)} case {i}: list {name} ({len(lists[name])} KeyLines) block {bw}x{bh} iter {it} mode {mode} "
              f"discard {disc}: {int(fixed.sum())} fixed of {fixed.size}")
    rec["cases"] = np.array(params, np.int32)   # list (ord), bw, bh, iter_num, bound_mode, discard, thresh_match_num
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF", "/root/reference"))
    a = ap.parse_args()
    gold = os.path.join(ROOT, "tests", "golden", "depth_fill")   # (a directory of its own: tests/golden/*.npz are the pipeline fixtures)
    with tempfile.TemporaryDirectory(prefix="depth_fill_ref_") as tmp:
        exe = build_driver(a.ref, tmp)
        small = replay_lists(376, 240, (9, 12))
        empty = small[9][:0]
        write(os.path.join(gold, "376x240.npz"), exe, 376, 240, {"A": small[9], "B": small[12], "E": empty}, CASES_SMALL)
        large = replay_lists(752, 480, (9,))
        write(os.path.join(gold, "752x480.npz"), exe, 752, 480, {"C": large[9]}, CASES_LARGE)


if __name__ == "__main__":
    main()
