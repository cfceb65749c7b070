#!/usr/bin/env python3
"""Time of the cross-view surface integration on the device and in the reference, on the same inputs.

    python tools/surface_integrate_timing.py device    [--reps 20] [--check] [--out FILE]     (GPU machine)
    python tools/surface_integrate_timing.py reference [--ref /path/to/reference] [--out FILE] (build machine, one core)

Two scenes: the 752x480 fixture (tests/golden/surface_integrate/752x480_b10.npz: 8 views, its own voxel grid) and a synthetic ring of
64 views at 752x480 / 10-px blocks in a 500 x 500 x 500 grid (tools/make_surface_integrate_golden.ring_views, seed 64; the box is
analizeSpaceSize's, widened to the camera centres and padded).  `device` brackets edgehip_surface_integrate (all views cast: the clear
of the plane, the rays and the test) with HIP events on the context's stream, after three warm-up calls, and separately the clear
alone (an integrate with an empty casting list: clear + test against an empty plane).  `reference` runs
tools/surface_integrate_ref_driver.cpp — OcGrid, fillKFList, rayCutSurface(kf_list) — and reports its own clock around the two calls.
--check compares the device's flags with the numpy port.  Prints one JSON line per measurement; --out appends them to a file.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import surface_integrate_port as port  # noqa: E402
from tools import make_surface_integrate_golden as gen  # noqa: E402


def scenes():
    g = np.load(os.path.join(ROOT, "tests", "golden", "surface_integrate", "752x480_b10.npz"))
    views = [port.view(g["rho"][k], g["s_rho"][k], g["Pose"][k], g["Pos"][k], g["K"][k]) for k in range(len(g["K"]))]
    yield "752x480 fixture", views, g["origin"], g["size"], tuple(int(v) for v in g["n"])
    cam = port.camera(*gen.camera(752, 480))
    ring = gen.ring_views(75, 48, 64, 64)
    o, s = gen.padded_box(ring, 10, 10, cam)
    yield "64-view ring", ring, o, s, (500, 500, 500)


def describe(name, views, o, s, n):
    return {"scene": name, "views": len(views), "w": 752, "h": 480, "block": 10, "grid": [75, 48], "voxels": list(n),
            "box_origin": [float(v) for v in o], "box_size": [float(v) for v in s]}


def device(a):
    from rebvo_amd import edgehip
    hip = C.CDLL("libamdhip64.so")
    eh = edgehip.EdgeHip(edgehip.euroc_params(752, 480), nseq=1, nslots=2)
    eh.depth_fill_enable(10, 1)
    stream = C.c_void_p(eh.lib.edgehip_stream(eh.ctx))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

    def timed(o, s, cast):
        for _ in range(3):
            eh.surface_integrate(o, s, cast)
        eh.sync()
        ms = []
        for _ in range(a.reps):
            hip.hipEventRecord(ev0, stream)
            eh.surface_integrate(o, s, cast)
            hip.hipEventRecord(ev1, stream)
            hip.hipEventSynchronize(ev1)
            t = C.c_float(0)
            hip.hipEventElapsedTime(C.byref(t), ev0, ev1)
            ms.append(t.value)
        return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": a.reps}

    lines = []
    for name, views, o, s, n in scenes():
        eh.surface_views_enable(len(views), n)
        for k, v in enumerate(views):
            eh.surface_view_upload(k, v["rho"], v["s_rho"], v["Pose"], v["Pos"], v["K"])
        rec = dict(describe(name, views, o, s, n), leg="device: clear + rays of all views + test", **timed(o, s, None))
        vis = eh.download_surface_visibility(list(range(len(views))))
        rec["hidden"] = float(1 - np.mean(vis))
        if a.check:
            want, st = port.integrate(views, o, s, n, 10, 10, port.camera(*gen.camera(752, 480)))
            rec["flags_equal_port"] = bool(all(np.array_equal(x, y) for x, y in zip(vis, want)))
            rec["voxels_marked"], rec["samples"] = st["voxels_marked"], st["samples"]
            rec["outside"] = st["ray_steps_outside"] + st["samples_outside"]
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        rec = dict(describe(name, views, o, s, n), leg="device: clear + test, nobody casts", **timed(o, s, []))
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    eh.close()
    return lines


def reference(a):
    lines = []
    with tempfile.TemporaryDirectory(prefix="surface_integrate_ref_") as tmp:
        exe = gen.build_driver(a.ref, tmp)
        for name, views, o, s, n in scenes():
            r = gen.run_ref(exe, tmp, 752, 480, 10, 10, gen.camera(752, 480), views, o, s, n, [(1, None)])
            rec = dict(describe(name, views, o, s, n), leg="reference, one core: OcGrid + fillKFList + rayCutSurface(kf_list)",
                       fill_s=float(r["secs"][0]), raycut_s=float(r["secs"][1]), total_ms=float(1e3 * r["secs"].sum()),
                       blocks_filled=r["blocks_filled"], hidden=float(1 - r["vis"][0].mean()))
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["device", "reference"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF", "/root/reference"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = device(a) if a.leg == "device" else reference(a)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
