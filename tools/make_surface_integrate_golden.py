#!/usr/bin/env python3
"""Generate tests/golden/surface_integrate/*.npz from the REFERENCE's own surface integrator (src/visualizer/surface_integrator.cpp).

Build machine only (needs the reference tree and oracle/_ref/libreforacle.so from `make -C oracle`):
    python tools/make_surface_integrate_golden.py [--ref /path/to/reference]

The reference's surface_integrator.cpp, depth_filler.cpp and mtracklib/keyframe.cpp are compiled in place, together with
tools/surface_integrate_ref_driver.cpp, into a temporary directory outside the repository, with the flags and prelude of
tools/make_depth_fill_golden.py (nothing is written under oracle/, no reference source is copied).

A scene is a ring of cameras that look at a common centre through each other's surfaces.  View 0's grid (and view 1's where there is
one) is the reference's fill of a KeyLine list (tests/golden/depth_fill/*.npz); the others are analytic walls with ripples.  The box
is analizeSpaceSize's, widened to hold the camera centres and padded.  Per fixture: the views (grids, poses, K), camera, block size,
box, voxel dimensions, the cuts (reset flag + casting views, -1 = all) and the reference's visibility of every view after each cut,
and its analizeSpaceSize result.  Before a file is written the generator asserts, on the CPU: no fill sample and no ray step outside
the box (counted by tests/surface_integrate_port.py on the same inputs, and no "Out of" message from the reference), every rho / K
finite and positive, 5 % .. 95 % of the cells hidden after the all-views cut with at least one view showing both states, the port equal
to the reference on every flag, and the file no larger than the largest one under tests/golden/depth_surface/.
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
from rebvo_amd import edgehip  # noqa: E402
from tests import surface_integrate_port as port  # noqa: E402
from tools.make_depth_fill_golden import PRELUDE  # noqa: E402


def build_driver(ref, tmp):
    inc = os.path.join(ROOT, "oracle", "_ref", "inc")
    lib = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(lib, "libreforacle.so")):
        raise SystemExit("oracle/_ref/libreforacle.so is missing: run `make -C oracle` first")
    pre = os.path.join(tmp, "prelude.h")
    with open(pre, "w") as f:
        f.write(PRELUDE)
    exe = os.path.join(tmp, "si_driver")
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-access-control", "-w", "-include", pre,
           "-I" + inc, "-I" + os.path.join(ref, "include"), "-I" + ref,
           os.path.join(ROOT, "tools", "surface_integrate_ref_driver.cpp"),
           os.path.join(ref, "src", "visualizer", "surface_integrator.cpp"), os.path.join(ref, "src", "visualizer", "depth_filler.cpp"),
           os.path.join(ref, "src", "mtracklib", "keyframe.cpp"),
           "-L" + lib, "-Wl,-rpath," + lib, "-lreforacle", "-lm", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def camera(w, h):
    p = edgehip.euroc_params(w, h)
    return np.array([p.ppx, p.ppy, p.zfx, p.zfy], np.float32)


def run_ref(exe, tmp, w, h, bw, bh, cam, views, origin, size, n, cuts):
    """-> dict(space_origin, space_size, blocks_filled, vis [ncuts][nviews](gh, gw) bool, secs [1 + ncuts], stdout)."""
    gw, gh = w // bw, h // bh
    G = gw * gh
    payload = [np.array([w, h, bw, bh, len(views), *n, len(cuts)], np.int32).tobytes(), np.asarray(cam, np.float32).tobytes(),
               np.asarray(origin, np.float64).tobytes(), np.asarray(size, np.float64).tobytes()]
    for v in views:
        payload += [v["Pose"].tobytes(), v["Pos"].tobytes(), np.float64(v["K"]).tobytes(),
                    np.ascontiguousarray(v["rho"]).tobytes(), np.ascontiguousarray(v["s_rho"]).tobytes()]
    for reset, cast in cuts:
        ids = [] if cast is None else list(cast)
        payload.append(np.array([int(reset), -1 if cast is None else len(ids), *ids], np.int32).tobytes())
    fin, fout = os.path.join(tmp, "si_in.bin"), os.path.join(tmp, "si_out.bin")
    with open(fin, "wb") as f:
        f.write(b"".join(payload))
    r = subprocess.run([exe, fin, fout], check=True, capture_output=True, text=True)
    out = open(fout, "rb").read()
    assert len(out) == 48 + 4 + len(cuts) * len(views) * G + 8 * (1 + len(cuts)), len(out)
    sp = np.frombuffer(out, np.float64, 6, 0)
    vis = np.frombuffer(out, np.uint8, len(cuts) * len(views) * G, 52).reshape(len(cuts), len(views), gh, gw).astype(bool)
    return dict(space_origin=sp[:3].copy(), space_size=sp[3:].copy(), blocks_filled=int(np.frombuffer(out, np.uint32, 1, 48)[0]),
                vis=vis, secs=np.frombuffer(out[-8 * (1 + len(cuts)):], np.float64).copy(), stdout=r.stdout)


def roty(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rotx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def wall(gw, gh, depth, ripple, phase):
    """A wall at `depth` with ripples, as a grid of inverse depths and uncertainties."""
    y, x = np.mgrid[0:gh, 0:gw]
    z = depth * (1 + ripple * np.sin(6.0 * x / gw + phase) * np.cos(5.0 * y / gh - phase))
    rho = 1.0 / z
    return rho, rho * (0.04 + 0.03 * np.cos(3.0 * x / gw + 2.0 * y / gh + phase) ** 2)


def ring_views(gw, gh, nviews, seed, first=()):
    """nviews cameras on a ring (and a little above and below it) that look at the origin; the grids in `first` for the first views, walls
    that pass near the origin for the rest."""
    rng = np.random.default_rng(seed)
    views = []
    for k in range(nviews):
        K = float(rng.uniform(0.8, 1.3))
        d = float(rng.uniform(1.6, 2.4))                       # world distance of the camera from the centre
        R = roty(2 * np.pi * k / nviews + rng.uniform(-0.1, 0.1)) @ rotx(rng.uniform(-0.25, 0.25))
        pos = -R @ np.array([0, 0, d]) + rng.uniform(-0.1, 0.1, 3)
        if k < len(first):
            rho, s_rho = first[k]
        else:
            rho, s_rho = wall(gw, gh, d / K * rng.uniform(0.9, 1.2), 0.12, float(rng.uniform(0, 6)))
        views.append(port.view(rho, s_rho, R, pos, K))
    return views


def padded_box(views, bw, bh, cam, pad=0.04):
    """analizeSpaceSize's box, widened to hold the camera centres and padded by `pad` of its size on every side."""
    o, s = port.space(views, bw, bh, cam)
    lo, hi = o.copy(), o + s
    for v in views:
        lo, hi = np.minimum(lo, v["Pos"]), np.maximum(hi, v["Pos"])
    ext = hi - lo
    return lo - pad * ext, ext * (1 + 2 * pad)


def check_and_pack(exe, tmp, name, w, h, bw, bh, views, n, cuts, limit):
    cam32 = camera(w, h)
    cam = port.camera(*cam32)
    for v in views:
        q = v["rho"] / v["K"]
        assert np.isfinite(q).all() and (q > 0).all(), name
    origin, size = padded_box(views, bw, bh, cam)
    ref = run_ref(exe, tmp, w, h, bw, bh, cam32, views, origin, size, n, cuts)
    assert "Out of" not in ref["stdout"], (name, ref["stdout"][-400:])
    po, ps = port.space(views, bw, bh, cam)
    assert po.tobytes() == ref["space_origin"].tobytes() and ps.tobytes() == ref["space_size"].tobytes(), name
    vis = None
    for c, (reset, cast) in enumerate(cuts):
        vis, stats = port.integrate(views, origin, size, n, bw, bh, cam, cast, None if reset else vis)
        assert stats["ray_steps_outside"] == 0 and stats["samples_outside"] == 0, (name, c, stats)
        for k in range(len(views)):
            assert np.array_equal(vis[k], ref["vis"][c, k]), (name, c, k, int((vis[k] != ref["vis"][c, k]).sum()))
    hid = 1.0 - ref["vis"][0].mean()
    assert 0.05 <= hid <= 0.95, (name, hid)
    assert any(0 < ref["vis"][0, k].sum() < ref["vis"][0, k].size for k in range(len(views))), name
    cut_arr = np.full((len(cuts), 2 + len(views)), -2, np.int32)   # reset, n (-1 = all), ids
    for c, (reset, cast) in enumerate(cuts):
        ids = [] if cast is None else list(cast)
        cut_arr[c, :2 + len(ids)] = [int(reset), -1 if cast is None else len(ids), *ids]
    rec = dict(w=np.int32(w), h=np.int32(h), bw=np.int32(bw), bh=np.int32(bh), cam=cam32, n=np.asarray(n, np.int32),
               origin=origin, size=size, rho=np.stack([v["rho"] for v in views]), s_rho=np.stack([v["s_rho"] for v in views]),
               Pose=np.stack([v["Pose"] for v in views]), Pos=np.stack([v["Pos"] for v in views]), K=np.array([v["K"] for v in views]),
               cuts=cut_arr, vis=np.packbits(ref["vis"], axis=None), space_origin=ref["space_origin"], space_size=ref["space_size"])
    path = os.path.join(ROOT, "tests", "golden", "surface_integrate", name + ".npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) <= limit, (path, os.path.getsize(path), limit)
    print(f"{name}: {len(views)} views, grid {w // bw}x{h // bh}, voxels {tuple(n)}, hidden after the all-views cut {hid:.3f} "
          f"(per cut {[round(1 - float(ref['vis'][c].mean()), 3) for c in range(len(cuts))]}), {ref['blocks_filled']} blocks filled, "
          f"reference {ref['secs'].sum():.3f} s, {os.path.getsize(path)} bytes")


def fill_grid(res, case):
    z = np.load(os.path.join(ROOT, "tests", "golden", "depth_fill", f"{res}.npz"))
    return z[f"case{case}_rho"], z[f"case{case}_s_rho"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF", "/root/reference"))
    a = ap.parse_args()
    os.makedirs(os.path.join(ROOT, "tests", "golden", "surface_integrate"), exist_ok=True)
    limit = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "depth_surface", "*.npz")))
    # main.cpp:192 then :201 (all key frames, then one more on top); a single view after a reset, then another on top; a subset
    cuts = [(1, None), (0, [1]), (1, [0]), (0, [2]), (1, [1, 3])]
    with tempfile.TemporaryDirectory(prefix="surface_integrate_ref_") as tmp:
        exe = build_driver(a.ref, tmp)
        check_and_pack(exe, tmp, "376x240_b10", 376, 240, 10, 10,
                       ring_views(37, 24, 4, 1, [fill_grid("376x240", 0), fill_grid("376x240", 10)]), (64, 60, 72), cuts, limit)
        check_and_pack(exe, tmp, "376x240_b7", 376, 240, 7, 7,
                       ring_views(53, 34, 5, 2, [fill_grid("376x240", 2)]), (60, 64, 68), cuts, limit)
        check_and_pack(exe, tmp, "752x480_b10", 752, 480, 10, 10,
                       ring_views(75, 48, 8, 3, [fill_grid("752x480", 0)]), (136, 128, 144), cuts + [(1, [2, 5, 7])], limit)


if __name__ == "__main__":
    main()
