#!/usr/bin/env python3
"""Generate tests/golden/surface_ray_cross/*.npz from the REFERENCE's own SurfaceInt::checkDFRayCrossExaustive
(src/visualizer/surface_integrator.cpp:70-116).

Build machine only (needs the reference tree and oracle/_ref/libreforacle.so from `make -C oracle`):
    python tools/make_surface_ray_cross_golden.py [--ref /path/to/reference]

The reference's surface_integrator.cpp, depth_filler.cpp and mtracklib/keyframe.cpp are compiled in place, together with
tools/surface_ray_cross_ref_driver.cpp, into a temporary directory outside the repository, with the flags and prelude of
tools/make_depth_fill_golden.py (nothing is written under oracle/, no reference source is copied).

The views of the three scenes are those of tests/golden/surface_integrate/*.npz, read and not stored again: a fixture here holds the
steps and the reference's flags after each.  A step is (start, absent, pairs): start 1 resets every visibility first, 0 keeps the
flags of the step before, 2 starts from the flags the OcGrid cut left (cut 0 of the surface_integrate fixture); absent is a view whose
slot is empty during the step (-1: none); pairs are (target, hidder), None = every ordered pair.  The fourth fixture, `crafted`, holds
its own small views (made by crafted_views below) for the IEEE branches: cells with rho zero, negative, NaN and infinite, a hidder whose
centre coincides with the target's, and a view with K = 1.  Before a file is written the generator asserts that the numpy port
(tests/surface_ray_cross_port.py) equals the reference on every flag, and that the file is no larger than the largest one under
tests/golden/depth_surface/.
"""
import argparse
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import surface_ray_cross_port as port  # noqa: E402
from tools.make_depth_fill_golden import PRELUDE  # noqa: E402
from tools.make_surface_integrate_golden import camera, rotx, roty, wall  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "surface_ray_cross")
SRC = os.path.join(ROOT, "tests", "golden", "surface_integrate")
# scene -> the pair whose hidden share the estimate put inside [0.05, 0.95] (target, hidder)
SCENES = {"376x240_b10": (0, 3), "376x240_b7": (0, 1), "752x480_b10": (0, 7)}


def build_driver(ref, tmp):
    inc = os.path.join(ROOT, "oracle", "_ref", "inc")
    lib = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(lib, "libreforacle.so")):
        raise SystemExit("oracle/_ref/libreforacle.so is missing: run `make -C oracle` first")
    pre = os.path.join(tmp, "prelude.h")
    with open(pre, "w") as f:
        f.write(PRELUDE)
    exe = os.path.join(tmp, "rc_driver")
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-access-control", "-w", "-include", pre,
           "-I" + inc, "-I" + os.path.join(ref, "include"), "-I" + ref,
           os.path.join(ROOT, "tools", "surface_ray_cross_ref_driver.cpp"),
           os.path.join(ref, "src", "visualizer", "surface_integrator.cpp"), os.path.join(ref, "src", "visualizer", "depth_filler.cpp"),
           os.path.join(ref, "src", "mtracklib", "keyframe.cpp"),
           "-L" + lib, "-Wl,-rpath," + lib, "-lreforacle", "-lm", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run_ref(exe, tmp, w, h, bw, bh, cam, views, steps):
    """steps: [(start, pairs or None, flags or None)]; flags [nviews](gh, gw) for start == 2.  views may hold None (no grid).
    -> (vis [nsteps][nviews](gh, gw) bool, seconds [nsteps])."""
    gw, gh = w // bw, h // bh
    G = gw * gh
    payload = [np.array([w, h, bw, bh, len(views), len(steps)], np.int32).tobytes(), np.asarray(cam, np.float32).tobytes()]
    some = next(v for v in views if v is not None)
    for v in views:
        p = some if v is None else v
        payload += [p["Pose"].tobytes(), p["Pos"].tobytes(), np.float64(p["K"]).tobytes(), np.int32(v is not None).tobytes()]
        if v is not None:
            payload += [np.ascontiguousarray(v["rho"]).tobytes(), np.ascontiguousarray(v["s_rho"]).tobytes()]
    for start, pairs, flags in steps:
        ids = [] if pairs is None else [int(x) for p in pairs for x in p]
        payload.append(np.array([int(start), -1 if pairs is None else len(pairs), *ids], np.int32).tobytes())
        if start == 2:
            payload.append(np.stack([np.zeros((gh, gw), np.uint8) if f is None else np.asarray(f, np.uint8) for f in flags]).tobytes())
    fin, fout = os.path.join(tmp, "rc_in.bin"), os.path.join(tmp, "rc_out.bin")
    with open(fin, "wb") as f:
        f.write(b"".join(payload))
    subprocess.run([exe, fin, fout], check=True, capture_output=True, text=True)
    out = open(fout, "rb").read()
    assert len(out) == len(steps) * len(views) * G + 8 * len(steps), len(out)
    vis = np.frombuffer(out, np.uint8, len(steps) * len(views) * G).reshape(len(steps), len(views), gh, gw).astype(bool)
    return vis, np.frombuffer(out[-8 * len(steps):], np.float64).copy()


def scene_steps(a, b, nviews):
    """The steps of a scene whose populated pair is (a, b); c is a third view."""
    c = next(k for k in range(nviews) if k not in (a, b))
    return [(1, -1, None),                       # every ordered pair after a reset
            (1, -1, [(a, b)]),                   # one pair ...
            (0, -1, [(b, a), (a, c), (c, b)]),   # ... and an accumulating step on top of it
            (1, -1, [(b, a)]),                   # the other direction alone
            (2, -1, [(a, b), (c, a)]),           # on top of the OcGrid cut's flags
            (1, c, [(a, b), (a, c), (c, b), (b, a)])]   # a list that names an empty slot


def reference_steps(exe, tmp, w, h, bw, bh, cam32, views, steps, ocgrid):
    """Runs of the driver (one per set of absent views, the steps of a run in order) -> (vis [nsteps][nviews](gh, gw), seconds)."""
    vis, secs = [None] * len(steps), np.zeros(len(steps))
    for absent in sorted({s[1] for s in steps}):
        idx = [i for i, s in enumerate(steps) if s[1] == absent]
        vv = [None if k == absent else v for k, v in enumerate(views)]
        r, t = run_ref(exe, tmp, w, h, bw, bh, cam32, vv, [(steps[i][0], steps[i][2], ocgrid) for i in idx])
        for j, i in enumerate(idx):
            vis[i], secs[i] = r[j], t[j]
    return np.stack(vis), secs


def port_steps(views, steps, bw, bh, cam, ocgrid):
    """The same through the numpy port -> [nsteps][nviews] (gh, gw) bool or None."""
    out, prev = [], None
    for start, absent, pairs in steps:
        vv = [None if k == absent else v for k, v in enumerate(views)]
        base = {0: prev, 1: None, 2: ocgrid}[start]
        prev = port.ray_cross(vv, pairs, bw, bh, cam, base)
        out.append(prev)
    return out


def pack_steps(steps):
    width = 3 + 2 * max(len(p) for _, _, p in steps if p is not None)
    arr = np.full((len(steps), width), -2, np.int32)   # start, absent, n (-1 = every ordered pair), (t, h) ...
    for i, (start, absent, pairs) in enumerate(steps):
        ids = [] if pairs is None else [int(x) for p in pairs for x in p]
        arr[i, :3 + len(ids)] = [start, absent, -1 if pairs is None else len(pairs), *ids]
    return arr


def check_and_write(exe, tmp, name, w, h, bw, bh, views, steps, ocgrid, limit, extra):
    cam32 = camera(w, h)
    cam = port.camera(*cam32)
    ref, secs = reference_steps(exe, tmp, w, h, bw, bh, cam32, views, steps, ocgrid)
    got = port_steps(views, steps, bw, bh, cam, ocgrid)
    for i, (_, absent, _) in enumerate(steps):
        for k in range(len(views)):
            if k != absent:
                assert np.array_equal(got[i][k], ref[i, k]), (name, i, k, int((got[i][k] != ref[i, k]).sum()))
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, steps=pack_steps(steps), vis=np.packbits(ref, axis=None), **extra)
    assert os.path.getsize(path) <= limit, (path, os.path.getsize(path), limit)
    print(f"{name}: {len(views)} views, grid {w // bw}x{h // bh}, hidden per step "
          f"{[round(1 - float(ref[i].mean()), 3) for i in range(len(steps))]}, reference {secs.sum():.3f} s "
          f"(all pairs {secs[0]:.3f} s), {os.path.getsize(path)} bytes")


def crafted_views(gw=37, gh=24):
    """Three small views on the 376x240 camera with 10-px blocks.  View 0 has K = 1 and cells with rho 0, negative, NaN and infinite;
    view 1 stands in view 0's centre, turned a little (ray_orig is exactly zero between them, the ray vectors are not); view 2 looks
    back at both from the other side, with K != 1."""
    rng = np.random.default_rng(11)
    rho0, s0 = wall(gw, gh, 2.0, 0.1, 0.3)
    rho0 = rho0.copy()
    rho0[5, 7], rho0[5, 8], rho0[6, 7], rho0[6, 8] = 0.0, -0.4, np.nan, np.inf
    rho0[15, 20], rho0[16, 30] = -np.inf, -0.0
    rho1, s1 = wall(gw, gh, 2.05, 0.25, 1.7)      # in front of view 0's wall in places, behind it in others
    rho1 = rho1.copy()
    rho1[10, 12], rho1[11, 12] = np.nan, 0.0
    rho2, s2 = wall(gw, gh, 2.6, 0.3, 4.0)       # its rays end before view 0's wall in places, pass it in others
    pos0 = np.array([0.1, -0.05, -2.0])
    views = [port.view(rho0, s0, np.eye(3), pos0, 1.0),
             port.view(rho1, s1, roty(0.06) @ rotx(-0.04), pos0, 0.93),
             port.view(rho2, s2, roty(np.pi + 0.1) @ rotx(0.05), np.array([0.2, 0.1, 2.1]) + rng.uniform(-0.05, 0.05, 3), 0.9)]
    return views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF", "/root/reference"))
    ap.add_argument("--only", default=None, help="write this fixture alone")
    a = ap.parse_args()
    os.makedirs(GOLD, exist_ok=True)
    limit = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "depth_surface", "*.npz")))
    with tempfile.TemporaryDirectory(prefix="surface_ray_cross_ref_") as tmp:
        exe = build_driver(a.ref, tmp)
        for name, (ta, hb) in SCENES.items():
            if a.only not in (None, name):
                continue
            g = np.load(os.path.join(SRC, name + ".npz"))
            nv = len(g["K"])
            views = [port.view(g["rho"][k], g["s_rho"][k], g["Pose"][k], g["Pos"][k], g["K"][k]) for k in range(nv)]
            gh, gw = g["rho"].shape[1:]
            oc = np.unpackbits(g["vis"])[:nv * gh * gw].reshape(nv, gh, gw).astype(bool)   # cut 0: the all-views OcGrid cut
            check_and_write(exe, tmp, name, int(g["w"]), int(g["h"]), int(g["bw"]), int(g["bh"]), views, scene_steps(ta, hb, nv),
                            list(oc), limit, {})
        if a.only not in (None, "crafted"):
            return
        views = crafted_views()
        steps = [(1, -1, None), (1, -1, [(0, 1)]), (0, -1, [(1, 0)]), (1, -1, [(0, 2), (2, 0)]), (1, 1, [(0, 1), (2, 0), (1, 2)])]
        check_and_write(exe, tmp, "crafted", 376, 240, 10, 10, views, steps, None, limit,
                        dict(w=np.int32(376), h=np.int32(240), bw=np.int32(10), bh=np.int32(10), cam=camera(376, 240),
                             rho=np.stack([v["rho"] for v in views]), s_rho=np.stack([v["s_rho"] for v in views]),
                             Pose=np.stack([v["Pose"] for v in views]), Pos=np.stack([v["Pos"] for v in views]),
                             K=np.array([v["K"] for v in views])))


if __name__ == "__main__":
    main()
