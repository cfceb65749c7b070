#!/usr/bin/env python3
"""Generate tests/golden/ros_edgemap/crafted.npz from the REFERENCE's own arithmetic for the ROS nodelet's per-KeyLine output.

Build machine only (needs the reference tree and oracle/_ref/inc from `make -C oracle`):
    python tools/make_ros_edgemap_golden.py [--ref /path/to/reference]

The nodelet itself (ros/src/rebvo_ros/src/rebvo_nodelet.cpp:176-212) needs ROS; tools/ros_edgemap_ref_driver.cpp stands in for its loop
with the reference's KeyLine, cam_model::unprojectHomCordVec and TooN included in place, and is compiled into oracle/_ref/ (kept out of
the repository; no reference source is copied).  The fixture is data only: the crafted KeyLine lists of tests/ros_edgemap_crafted.py
(lengths 0, 1, 37, 128), their K, the camera's zfm and the bytes the reference's operations give."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rebvo_amd import edgehip  # noqa: E402
from tests import ros_edgemap_crafted as crafted  # noqa: E402


def build_driver(ref):
    out = os.path.join(ROOT, "oracle", "_ref")
    inc = os.path.join(out, "inc")
    if not os.path.exists(os.path.join(inc, "TooN", "TooN.h")):
        raise SystemExit("oracle/_ref/inc/TooN is missing: run `make -C oracle` first")
    exe = os.path.join(out, "ros_edgemap_ref_driver")
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-access-control", "-w", "-I" + inc, "-I" + os.path.join(ref, "include"),
           "-I" + ref, os.path.join(ROOT, "tools", "ros_edgemap_ref_driver.cpp"), "-lm", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run_ref(exe, kl, K, zfx, zfy):
    kn = len(kl)
    payload = np.int32(kn).tobytes() + np.float64(K).tobytes() + np.array([zfx, zfy], np.float32).tobytes() + np.ascontiguousarray(kl).tobytes()
    out = subprocess.run([exe], input=payload, check=True, capture_output=True).stdout
    assert len(out) == 8 + 64 * kn, (len(out), kn)
    zfm = float(np.frombuffer(out, np.float64, 1, 0)[0])
    pts = np.frombuffer(out, np.uint8, 12 * kn, 8).reshape(kn, 12).copy()
    recs = np.frombuffer(out, np.uint8, 52 * kn, 8 + 12 * kn).reshape(kn, 52).copy()
    return zfm, pts, recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF", "/root/reference"))
    a = ap.parse_args()
    gold = os.path.join(ROOT, "tests", "golden", "ros_edgemap")
    os.makedirs(gold, exist_ok=True)
    exe = build_driver(a.ref)
    p = edgehip.euroc_params(crafted.W, crafted.H)
    lists = crafted.crafted_lists(max(crafted.MAX_POINTS))
    arrays = {"K": np.array(crafted.K_PROF, np.float64), "zf": np.array([p.zfx, p.zfy], np.float32)}
    for s, kl in enumerate(lists):
        zfm, pts, recs = run_ref(exe, kl, crafted.K_PROF[s], p.zfx, p.zfy)
        assert zfm == crafted.ZFM, (zfm, crafted.ZFM)
        arrays[f"keylines_{s}"] = np.ascontiguousarray(kl).view(np.uint8).reshape(len(kl), 168)
        arrays[f"points_{s}"] = pts
        arrays[f"records_{s}"] = recs
    arrays["zfm"] = np.float64(crafted.ZFM)
    path = os.path.join(gold, "crafted.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: lists of {[len(k) for k in lists]} KeyLines, zfm {crafted.ZFM!r}, {crafted.populations(lists)}; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
