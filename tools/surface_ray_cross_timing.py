#!/usr/bin/env python3
"""Time of the exhaustive cross-view ray check on the device and in the reference, on the same inputs, and its agreement with the
OcGrid cut.

    python tools/surface_ray_cross_timing.py device    [--reps 20] [--out FILE]                (GPU machine)
    python tools/surface_ray_cross_timing.py reference [--ref /path/to/reference] [--out FILE] (build machine, one core)

752x480 at 10-px blocks (75 x 48 = 3600 cells a view): one pair and every ordered pair of the fixture's eight views
(tests/golden/surface_integrate/752x480_b10.npz), and every ordered pair of a synthetic ring of 64 views
(tools/make_surface_integrate_golden.ring_views, seed 64).  `device` brackets edgehip_surface_ray_cross (after a reset: the memset of
the flags, the copy of the pair list and the kernel) with HIP events on the context's stream, after three warm-up calls.  `reference`
runs tools/surface_ray_cross_ref_driver.cpp — checkDFRayCrossExaustive per pair — and reports its own clock around the calls; of the
64-view ring it runs the 63 pairs that have view 0 as their target and scales by 64 (every pair costs the same loops; the whole ring
would take most of an hour).  For information `device` also prints the share of cells on which the exhaustive flags and the OcGrid
flags differ, in each direction, at the fixture's voxel grid and at 500^3.  Prints one JSON line per measurement; --out appends them.
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
from tests import surface_integrate_port as iport  # noqa: E402
from tools import make_surface_integrate_golden as igen  # noqa: E402

PAIR = (0, 7)


def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "surface_integrate", "752x480_b10.npz"))
    views = [iport.view(g["rho"][k], g["s_rho"][k], g["Pose"][k], g["Pos"][k], g["K"][k]) for k in range(len(g["K"]))]
    return g, views


def ring():
    return igen.ring_views(75, 48, 64, 64)


def device(a):
    from rebvo_amd import edgehip
    hip = C.CDLL("libamdhip64.so")
    eh = edgehip.EdgeHip(edgehip.euroc_params(752, 480), nseq=1, nslots=2)
    eh.depth_fill_enable(10, 1)
    stream = C.c_void_p(eh.lib.edgehip_stream(eh.ctx))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

    def timed(pairs):
        for _ in range(3):
            eh.surface_ray_cross(pairs)
        eh.sync()
        ms = []
        for _ in range(a.reps):
            hip.hipEventRecord(ev0, stream)
            eh.surface_ray_cross(pairs)
            hip.hipEventRecord(ev1, stream)
            hip.hipEventSynchronize(ev1)
            t = C.c_float(0)
            hip.hipEventElapsedTime(C.byref(t), ev0, ev1)
            ms.append(t.value)
        return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": a.reps}

    def load(views, n):
        eh.surface_views_enable(len(views), n)
        for k, v in enumerate(views):
            eh.surface_view_upload(k, v["rho"], v["s_rho"], v["Pose"], v["Pos"], v["K"])

    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    g, views = fixture()
    load(views, 1)
    rec = dict(leg="device", scene="752x480 fixture, one pair", pairs=1, **timed([PAIR]))
    rec["hidden_target"] = float(1 - eh.download_surface_visibility(PAIR[0]).mean())
    emit(rec)
    rec = dict(leg="device", scene="752x480 fixture, every ordered pair of 8 views", pairs=56, **timed(None))
    exhaustive = np.stack(eh.download_surface_visibility(list(range(8))))
    rec["ms_per_pair"], rec["hidden"] = rec["ms_median"] / 56, float(1 - exhaustive.mean())
    emit(rec)
    for n in (tuple(int(v) for v in g["n"]), (500, 500, 500)):   # agreement with the voxel cut, for information
        load(views, n)
        eh.surface_integrate(g["origin"], g["size"])
        oc = np.stack(eh.download_surface_visibility(list(range(8))))
        emit(dict(leg="agreement", scene="752x480 fixture, 8 views", voxels=list(n), hidden_exhaustive=float(1 - exhaustive.mean()),
                  hidden_ocgrid=float(1 - oc.mean()), share_hidden_by_exhaustive_only=float((~exhaustive & oc).mean()),
                  share_hidden_by_ocgrid_only=float((exhaustive & ~oc).mean())))
    views = ring()
    load(views, 1)
    rec = dict(leg="device", scene="64-view ring, every ordered pair", pairs=64 * 63, **timed(None))
    rec["ms_per_pair"] = rec["ms_median"] / (64 * 63)
    rec["hidden"] = float(1 - np.mean(eh.download_surface_visibility(list(range(64)))))
    emit(rec)
    eh.close()
    return lines


def reference(a):
    from tools import make_surface_ray_cross_golden as gen
    lines = []
    cam32 = igen.camera(752, 480)
    with tempfile.TemporaryDirectory(prefix="surface_ray_cross_ref_") as tmp:
        exe = gen.build_driver(a.ref, tmp)
        _, views = fixture()
        vis, secs = gen.run_ref(exe, tmp, 752, 480, 10, 10, cam32, views, [(1, [PAIR], None), (1, None, None)])
        lines.append(dict(leg="reference, one core", scene="752x480 fixture, one pair", pairs=1, ms=float(1e3 * secs[0]),
                          hidden_target=float(1 - vis[0, PAIR[0]].mean())))
        lines.append(dict(leg="reference, one core", scene="752x480 fixture, every ordered pair of 8 views", pairs=56,
                          ms=float(1e3 * secs[1]), ms_per_pair=float(1e3 * secs[1] / 56), hidden=float(1 - vis[1].mean())))
        views = ring()
        vis, secs = gen.run_ref(exe, tmp, 752, 480, 10, 10, cam32, views, [(1, [(0, h) for h in range(1, 64)], None)])
        lines.append(dict(leg="reference, one core", scene="64-view ring, the 63 pairs with target 0, x 64", pairs_run=63,
                          ms_run=float(1e3 * secs[0]), ms_per_pair=float(1e3 * secs[0] / 63), ms_scaled_to_4032_pairs=float(64e3 * secs[0])))
        for rec in lines:
            print(json.dumps(rec), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["device", "reference"])
    ap.add_argument("--reps", type=int, default=20)
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
