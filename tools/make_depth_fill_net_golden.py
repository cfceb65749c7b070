#!/usr/bin/env python3
"""Generate tests/golden/depth_fill_net/*.npz from the REFERENCE's own depth_filler, net_keyline overload
(src/visualizer/depth_filler.cpp:59-104), fed with records from the reference's own packer (src/CommLib/net_keypoint.cpp).

Build machine only (needs the reference tree and oracle/_ref/libreforacle.so from `make -C oracle`):
    python tools/make_depth_fill_net_golden.py [--ref /path/to/reference]

The reference's depth_filler.cpp is compiled in place, together with tools/depth_fill_net_ref_driver.cpp, into a temporary directory
outside the repository (nothing is written under oracle/, no reference source is copied).  The records are what ref_copy_net_keyline +
ref_copy_net_keyline_nextid pack from the reference oracle's newest slot after 10 frames of synth.billboard_sequence.  Each fixture is
data only: the records (kn x 15 bytes), the parameters, p_off and the reference's output grids (rho, s_rho, fixed).
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402
from rebvo_amd import synth  # noqa: E402
from tools.make_depth_fill_golden import PRELUDE  # noqa: E402

# name: (list, bw, bh, iter_num, bound_mode, discard, thresh_rel_rho, thresh_match_num, p_off)
FIXTURES = {
    "1_376x240_lds": ("S", 10, 10, 10, 0, 1, 1.0, 5, (0.0, 0.0)),          # the visualizer's call; grid in LDS
    "2_752x480_hbm": ("L", 5, 5, 10, 0, 1, 1.0, 5, (0.0, 0.0)),            # 14 400 cells: grid in HBM
    "3_376x240_offset_keep": ("S", 10, 10, 10, 0, 0, 1.0, 5, (7.5, 26.0)),  # discard = 0; p_off puts the lowest records past the grid
    "4_376x240_all_unmatched": ("S", 10, 10, 10, 0, 1, 1.0, 256, (0.0, 0.0)),   # m_num_t = 256: every record fails the match gate
    "5_376x240_empty": ("E", 10, 10, 10, 0, 1, 1.0, 5, (0.0, 0.0)),        # kn = 0: rho 1, s_rho 40 everywhere
}


def build_driver(ref, tmp):
    inc = os.path.join(ROOT, "oracle", "_ref", "inc")
    lib = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(lib, "libreforacle.so")):
        raise SystemExit("oracle/_ref/libreforacle.so is missing: run `make -C oracle` first")
    pre = os.path.join(tmp, "prelude.h")
    with open(pre, "w") as f:
        f.write(PRELUDE)
    exe = os.path.join(tmp, "dfn_driver")
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-access-control", "-w", "-include", pre,
           "-I" + inc, "-I" + os.path.join(ref, "include"), "-I" + ref,
           os.path.join(ROOT, "tools", "depth_fill_net_ref_driver.cpp"), os.path.join(ref, "src", "visualizer", "depth_filler.cpp"),
           "-L" + lib, "-Wl,-rpath," + lib, "-lreforacle", "-lm", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run_ref(exe, rec, w, h, bw, bh, iter_num, mode, discard, v_thresh, m_num_t, p_off):
    hdr = np.array([w, h, bw, bh, iter_num, mode, discard, m_num_t], np.int32).tobytes()
    payload = (hdr + np.float64(v_thresh).tobytes() + np.array(p_off, np.float32).tobytes() + np.int32(len(rec)).tobytes() +
               np.ascontiguousarray(rec, np.uint8).tobytes())
    out = subprocess.run([exe], input=payload, check=True, capture_output=True).stdout
    gw, gh = w // bw, h // bh
    n = gw * gh
    assert len(out) == 17 * n, (len(out), n)
    rho = np.frombuffer(out, np.float64, n, 0).reshape(gh, gw)
    s_rho = np.frombuffer(out, np.float64, n, 8 * n).reshape(gh, gw)
    fixed = np.frombuffer(out, np.uint8, n, 16 * n).reshape(gh, gw)
    return rho.copy(), s_rho.copy(), fixed.copy()


def replay_records(w, h, frames):
    """The reference packer's records of the reference oracle's newest slot after `frames` frames."""
    orc = oracle.Oracle("ref", oracle.euroc_params(w, h))
    for k, (f, _, _) in enumerate(synth.billboard_sequence(w, h, frames)):
        orc.process_frame(f, 0.05 * k)
    s = orc.cur_slot()
    kn = orc.kn(s)
    L = orc.lib
    L.ref_copy_net_keyline.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double]
    L.ref_copy_net_keyline_nextid.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    rec = np.zeros((kn, 15), np.uint8)
    n = L.ref_copy_net_keyline(orc.ctx, s, -1, rec.ctypes.data, kn, 1.0)
    assert n == kn
    L.ref_copy_net_keyline_nextid(orc.ctx, s, rec.ctypes.data, kn)
    orc.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF", "/root/reference"))
    a = ap.parse_args()
    gold = os.path.join(ROOT, "tests", "golden", "depth_fill_net")
    os.makedirs(gold, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="depth_fill_net_ref_") as tmp:
        exe = build_driver(a.ref, tmp)
        small = replay_records(376, 240, 10)
        lists = {"S": (376, 240, small), "L": (752, 480, replay_records(752, 480, 10)), "E": (376, 240, small[:0])}
        for name, (lst, bw, bh, it, mode, disc, v, m, p_off) in FIXTURES.items():
            w, h, rec = lists[lst]
            rho, s_rho, fixed = run_ref(exe, rec, w, h, bw, bh, it, mode, disc, v, m, p_off)
            path = os.path.join(gold, name + ".npz")
            np.savez_compressed(path, w=np.int32(w), h=np.int32(h), records=rec,
                                params=np.array([bw, bh, it, mode, disc, m], np.int32),   # bw, bh, iter_num, bound_mode, discard, thresh_match_num
                                thresh_rel_rho=np.float64(v), p_off=np.array(p_off, np.float32), rho=rho, s_rho=s_rho, fixed=fixed)
            print(f"{name}: {len(rec)} records, block {bw}x{bh}, discard {disc}, m_num_t {m}, p_off {p_off}: {int(fixed.sum())} fixed of "
                  f"{fixed.size}; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
