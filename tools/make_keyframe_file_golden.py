#!/usr/bin/env python3
"""Generate tests/golden/keyframe_file/crafted.npz from the REFERENCE's own key-frame file code (src/mtracklib/keyframe.cpp).

Build machine only (needs the reference tree and oracle/_ref/libreforacle.so from `make -C oracle`):
    python tools/make_keyframe_file_golden.py [--ref /path/to/reference]

tools/keyframe_file_ref_driver.cpp is compiled into a temporary directory outside the repository, with the reference's keyframe.cpp and
depth_filler.cpp in place (nothing is written under oracle/, no reference source is copied).  Three key frames at 64 x 48 with kn = 0, 1
and a few hundred, every field of the 168-byte records random but valid for the depth fill.  The fixture records
  (a) the bytes the reference's keyframe::saveKeyframes2File wrote for them, and a mask of the bytes that mean something, built from the
      driver's offsetof / sizeof (the reference writes whatever its heap holds into the records' padding);
  (b) the bytes rebvo_amd.edgehip.write_keyframe_file wrote for the same input;
  (c) what the reference's keyframe::loadKeyframesFromFile read back from (b), every field;
  (d) the grids of the reference's initDepthFiller({8, 8}, IterNum, ThreshRelRho, ThreshMatchNum, BOUND_NONE, discart) on each key
      frame loaded from (b).
Before anything is written: (a) == (b) under the mask, the mask's holes are exactly bytes 36..39 of every record, (c) == the input.
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

GOLD = os.path.join(ROOT, "tests", "golden", "keyframe_file")
SIZE_LIMIT = 919829   # the largest file under tests/golden/depth_surface/
PRELUDE = "#include <algorithm>\nnamespace std { inline double max(float a, double b) { return max((double)a, b); } }\n"
W, H = 64, 48
FILL = dict(bw=8, bh=8, iter_num=5, thresh_rel_rho=0.5, thresh_match_num=5, discard=1)
PACKED = np.dtype([(n, edgehip.KEYLINE_DTYPE[n]) for n in edgehip.KEYLINE_DTYPE.names if n != "_pad0"])   # every field, no padding
HEAD = 256 + 8 + 72 + 4   # pose block, max_r, cam_model, kn


def build_driver(ref, tmp):
    inc = os.path.join(ROOT, "oracle", "_ref", "inc")
    lib = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(lib, "libreforacle.so")):
        raise SystemExit("oracle/_ref/libreforacle.so is missing: run `make -C oracle` first")
    pre = os.path.join(tmp, "prelude.h")
    with open(pre, "w") as f:
        f.write(PRELUDE)
    exe = os.path.join(tmp, "kf_file_driver")
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-access-control", "-w", "-include", pre,
           "-I" + inc, "-I" + os.path.join(ref, "include"), "-I" + ref,
           os.path.join(ROOT, "tools", "keyframe_file_ref_driver.cpp"), os.path.join(ref, "src", "mtracklib", "keyframe.cpp"),
           os.path.join(ref, "src", "visualizer", "depth_filler.cpp"),
           "-L" + lib, "-Wl,-rpath," + lib, "-lreforacle", "-lm", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def crafted_records(rs, n):
    kl = np.zeros(n, edgehip.KEYLINE_DTYPE)
    ang = rs.uniform(0, 2 * np.pi, n)
    kl["n_m"] = rs.uniform(1, 50, n).astype(np.float32)
    kl["u_m"] = np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
    kl["m_m"] = kl["u_m"] * kl["n_m"][:, None]
    kl["c_p"] = (rs.uniform(0, 1, (n, 2)) * [W - 1, H - 1]).astype(np.float32)
    kl["p_inx"] = kl["c_p"][:, 1].astype(np.int32) * W + kl["c_p"][:, 0].astype(np.int32)
    for f in ("p_m", "p_m_0", "m_m0"):
        kl[f] = rs.uniform(-40, 40, (n, 2)).astype(np.float32)
    for f in ("rho", "s_rho", "rho_nr", "s_rho_nr", "rho0", "s_rho0", "n_m0", "stereo_rho", "stereo_s_rho"):
        kl[f] = rs.uniform(0.01, 5, n)
    kl["score"] = rs.uniform(0, 1, n).astype(np.float32)
    kl["m_num"] = rs.randint(0, 12, n)            # ThreshMatchNum = 5: both sides
    for f in ("m_id", "m_id_f", "m_id_kf", "p_id", "n_id", "net_id", "stereo_m_id"):
        kl[f] = rs.randint(-1, max(n, 1), n)
    return kl


def crafted_pose(rs):
    q = edgehip.KfPose()
    q.t, q.K = rs.uniform(0, 100), rs.uniform(0.5, 2)
    for f, n in (("Rot", 9), ("RotLie", 3), ("Vel", 3), ("Pose", 9), ("PoseLie", 3), ("Pos", 3)):
        getattr(q, f)[:] = list(rs.uniform(-3, 3, n))
    return q


def driver_input(path, kfs, params):
    """The driver's own `save` input: pose block, max_r, pp, zf, Kc, w, h, kn, records (the camera as the configuration gives it)."""
    with open(path, "wb") as f:
        f.write(np.int32(len(kfs)).tobytes())
        for pose, kl in kfs:
            f.write(bytes(pose) + np.float64(params.search_range).tobytes())
            f.write(np.array([params.ppx, params.ppy, params.zfx, params.zfy], np.float32).tobytes())
            f.write(np.array(list(params.kc), np.float64).tobytes())
            f.write(np.array([params.w, params.h, len(kl)], np.int32).tobytes())
            f.write(kl.tobytes())


def parse_layout(text):
    lay = {}
    for line in text.splitlines():
        parts = line.split()
        if len(parts) == 3 and "." in parts[0]:
            lay[parts[0]] = (int(parts[1]), int(parts[2]))
    return lay


def file_mask(lay, kns):
    """1 for every byte of the file that a field of the reference's structs covers."""
    rec = np.zeros(168, np.uint8)
    for name, (off, size) in lay.items():
        if name.startswith("KeyLine.") and name != "KeyLine.sizeof":
            rec[off:off + size] = 1
    cam = np.zeros(72, np.uint8)
    for name, (off, size) in lay.items():
        if name.startswith("cam_model.") and name != "cam_model.sizeof":
            cam[off:off + size] = 1
    assert lay["KeyLine.sizeof"][1] == 168 and lay["cam_model.sizeof"][1] == 72
    parts = [np.ones(4, np.uint8)]
    for kn in kns:
        parts += [np.ones(256 + 8, np.uint8), cam, np.ones(4, np.uint8), np.tile(rec, kn)]
    return np.concatenate(parts), rec, cam


def parse_dump(out, n_expected):
    at = 0

    def take(dt, count=1):
        nonlocal at
        a = np.frombuffer(out, dt, count, at)
        at += a.nbytes
        return a

    n = int(take("<i4")[0])
    assert n == n_expected
    kfs = []
    for _ in range(n):
        pose = take("<f8", 32).copy()
        cam = dict(pp=take("<f4", 2).copy(), zf=take("<f4", 2).copy(), zfm=take("<f8")[0], Kc=take("<f8", 5).copy(), wh=take("<i4", 2).copy())
        kn = int(take("<i4")[0])
        kl = take(PACKED, kn).copy()
        kfs.append((pose, cam, kl))
    assert at == len(out)
    return kfs


def parse_grids(out, n_expected):
    at = 0
    n = int(np.frombuffer(out, "<i4", 1, at)[0]); at += 4
    assert n == n_expected
    grids = []
    for _ in range(n):
        gw, gh = (int(v) for v in np.frombuffer(out, "<i4", 2, at)); at += 8
        rho = np.frombuffer(out, "<f8", gw * gh, at).reshape(gh, gw).copy(); at += 8 * gw * gh
        s_rho = np.frombuffer(out, "<f8", gw * gh, at).reshape(gh, gw).copy(); at += 8 * gw * gh
        fixed = np.frombuffer(out, np.uint8, gw * gh, at).reshape(gh, gw).copy(); at += gw * gh
        grids.append((rho, s_rho, fixed))
    assert at == len(out)
    return grids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF", "/root/reference"))
    a = ap.parse_args()
    os.makedirs(GOLD, exist_ok=True)
    rs = np.random.RandomState(20)
    params = edgehip.euroc_params(W, H, zfx=420.0, zfy=421.5)     # zfx != zfy: zfm's float mean shows
    kns = [0, 1, 333]
    kfs = [(crafted_pose(rs), crafted_records(rs, kn)) for kn in kns]
    with tempfile.TemporaryDirectory(prefix="keyframe_file_ref_") as tmp:
        exe = build_driver(a.ref, tmp)
        lay = parse_layout(subprocess.run([exe, "layout"], check=True, capture_output=True, text=True).stdout)
        mask, rec_mask, cam_mask = file_mask(lay, kns)
        assert np.flatnonzero(rec_mask == 0).tolist() == [36, 37, 38, 39], np.flatnonzero(rec_mask == 0)
        assert cam_mask.all()
        # (a) the reference's writer
        din, fa, fb = (os.path.join(tmp, n) for n in ("in.bin", "a.kf", "b.kf"))
        driver_input(din, kfs, params)
        subprocess.run([exe, "save", din, fa], check=True, capture_output=True)
        bytes_a = np.fromfile(fa, np.uint8)
        # (b) ours
        edgehip.write_keyframe_file(fb, kfs, params)
        bytes_b = np.fromfile(fb, np.uint8)
        assert len(bytes_a) == len(bytes_b) == len(mask) == 4 + sum(HEAD + 168 * kn for kn in kns), (len(bytes_a), len(bytes_b), len(mask))
        diff = np.flatnonzero((bytes_a != bytes_b) & (mask != 0))
        assert diff.size == 0, ("the reference's file and ours differ in meaningful bytes", diff[:20])
        # (c) the reference's reader on ours
        loaded = parse_dump(subprocess.run([exe, "load", fb], check=True, capture_output=True).stdout, len(kfs))
        cam = edgehip.keyframe_file_camera(params)
        rec = {}
        for i, ((pose, kl), (lpose, lcam, lkl)) in enumerate(zip(kfs, loaded)):
            assert lpose.tobytes() == bytes(pose), i
            assert lcam["pp"].tobytes() == cam["pp"].tobytes() and lcam["zf"].tobytes() == cam["zf"].tobytes(), i
            assert lcam["zfm"] == cam["zfm"] and lcam["Kc"].tobytes() == cam["Kc"].tobytes() and list(lcam["wh"]) == [W, H], i
            for f in PACKED.names:
                assert lkl[f].tobytes() == kl[f].tobytes(), (i, f)
            rec[f"kf{i}_pose"] = np.frombuffer(bytes(pose), np.float64).copy()
            rec[f"kf{i}_kl"] = kl.view(np.uint8).reshape(-1, 168).copy()
            rec[f"kf{i}_loaded_pose"] = lpose
            rec[f"kf{i}_loaded_kl"] = lkl.view(np.uint8).reshape(-1, PACKED.itemsize).copy()
            rec[f"kf{i}_loaded_cam"] = np.concatenate([lcam["pp"], lcam["zf"], [lcam["zfm"]], lcam["Kc"], lcam["wh"]]).astype(np.float64)
        # (d) the reference's fill on ours
        grids = parse_grids(subprocess.run([exe, "fill", fb, str(FILL["bw"]), str(FILL["bh"]), str(FILL["iter_num"]), str(FILL["thresh_rel_rho"]),
                                            str(FILL["thresh_match_num"]), str(FILL["discard"])], check=True, capture_output=True).stdout, len(kfs))
        for i, (rho, s_rho, fixed) in enumerate(grids):
            assert rho.shape == (H // FILL["bh"], W // FILL["bw"])
            rec[f"kf{i}_grid_rho"], rec[f"kf{i}_grid_s_rho"], rec[f"kf{i}_grid_fixed"] = rho, s_rho, fixed
            print(f"key frame {i}: kn {kns[i]}, fixed cells {int(fixed.sum())} of {fixed.size}")
        assert grids[2][2].any() and not grids[2][2].all()
    rec.update(n=np.int32(len(kfs)), w=np.int32(W), h=np.int32(H), zfx=np.float64(params.zfx), zfy=np.float64(params.zfy),
               max_r=np.float64(params.search_range), ref_bytes=bytes_a, our_bytes=bytes_b, mask=mask,
               **{f"fill_{k}": np.float64(v) for k, v in FILL.items()})
    path = os.path.join(GOLD, "crafted.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= SIZE_LIMIT, size


if __name__ == "__main__":
    main()
