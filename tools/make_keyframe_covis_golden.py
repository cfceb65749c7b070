#!/usr/bin/env python3
"""Generate tests/golden/keyframe_covis/*.npz from the REFERENCE's own key-frame pair scoring (kfvo::countMatches, kfvo::kls_on_fov,
global_tracker::build_field).

Build machine only (needs the reference tree and oracle/_ref/libreforacle.so from `make -C oracle`):
    python tools/make_keyframe_covis_golden.py [--ref /path/to/reference]

tools/keyframe_covis_ref_driver.cpp is compiled into a temporary directory outside the repository, with the reference's kfvo.cpp and
global_tracker.cpp included in place (nothing is written under oracle/, no reference source is copied).  A fixture holds, per KeyLine, only
the eleven numbers the rules read (p_m, c_p, u_m, m_m, n_m as float32; rho, s_rho as float64, the record's own type), the poses, the
camera, the arguments, the reference's counts and fields and its seconds.  Before anything is written the plain-numpy port
(tests/keyframe_covis_port.py) must equal the reference on every count and every field cell; the branch populations come from the
port's run and are stored (for crafted.npz they are asserted non-zero).

  crafted.npz   5 key frames of 0, 1, 65, 257 and 600 KeyLines at 70x50 (no multiple of a tile either way), poses and scales that put
                KeyLines outside each border, behind the camera, on empty cells, through each rejection, over max_r (max_r below the
                field radius) and into matches of either sign; fields with ties, overlaps and samples off every border; a second run
                with min_mod filtering
  chained.npz   5 consecutive frames of synth.billboard_sequence (256x192) through the reference oracle's own pipeline on the CPU, each
                taken as a key frame with the pose and scale the pipeline had for it; every third KeyLine is kept (from a start that
                moves with the frame), for the file's size
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import keyframe_covis_port as port  # noqa: E402
from rebvo_amd import synth  # noqa: E402
from rebvo_amd.edgehip import KEYLINE_DTYPE  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "keyframe_covis")
SIZE_LIMIT = 919829   # the largest file under tests/golden/depth_surface/
PRELUDE = "#include <algorithm>\nnamespace std { inline double max(float a, double b) { return max((double)a, b); } }\n"

REQUIRED = ("out_left", "out_top", "out_right", "out_bottom", "behind", "empty_cell", "rej_angle", "rej_mod", "rej_rho",
            "matched_over_max_r", "match_negative_fi", "match_positive_fi", "kls_x_0", "kls_x_w_minus_1",
            "field_tie_cells", "field_overlap_cells", "field_off_left", "field_off_right", "field_off_top", "field_off_bottom")


def build_driver(ref, tmp):
    inc = os.path.join(ROOT, "oracle", "_ref", "inc")
    lib = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(lib, "libreforacle.so")):
        raise SystemExit("oracle/_ref/libreforacle.so is missing: run `make -C oracle` first")
    pre = os.path.join(tmp, "prelude.h")
    with open(pre, "w") as f:
        f.write(PRELUDE)
    exe = os.path.join(tmp, "kf_covis_driver")
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-access-control", "-w", "-include", pre,
           "-I" + inc, "-I" + os.path.join(ref, "include"), "-I" + ref,
           os.path.join(ROOT, "tools", "keyframe_covis_ref_driver.cpp"), os.path.join(ref, "src", "mtracklib", "keyframe.cpp"),
           os.path.join(ref, "src", "visualizer", "depth_filler.cpp"),
           "-L" + lib, "-Wl,-rpath," + lib, "-lreforacle", "-lm", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def camera(w, h, ppx, ppy, zfx, zfy):
    """cam_model's members: pp and zf as float, zfm = (double)((zf.x + zf.y) / 2) computed in float (cam_model.h:51-52)."""
    zfm = np.float64(np.float32((np.float32(zfx) + np.float32(zfy)) / np.float32(2)))
    return dict(w=np.int32(w), h=np.int32(h), ppx=np.float32(ppx), ppy=np.float32(ppy), zfx=np.float32(zfx), zfy=np.float32(zfy), zfm=zfm)


def records(kf):
    kl = np.zeros(len(kf["n_m"]), KEYLINE_DTYPE)
    for k in port.FIELDS:
        kl[k] = kf[k]
    for k in ("m_id", "m_id_f", "m_id_kf", "p_id", "n_id", "net_id", "stereo_m_id"):
        kl[k] = -1
    return kl


def run_ref(exe, kfs, cam, a):
    M, w, h = len(kfs), int(cam["w"]), int(cam["h"])
    payload = np.array([M, w, h, a["field_radius"]], np.int32).tobytes()
    payload += np.array([a["field_min_mod"], a["match_mod"], a["match_ang"], a["rho_tol"], a["max_r"], cam["ppx"], cam["ppy"], cam["zfx"],
                         cam["zfy"]], np.float32).tobytes()
    for kf in kfs:
        payload += np.array([len(kf["n_m"]), 0], np.int32).tobytes()
        payload += np.concatenate([kf["Pose"].ravel(), kf["Pos"], [kf["K"]]]).astype(np.float64).tobytes()
        payload += records(kf).tobytes()
    out = subprocess.run([exe], input=payload, check=True, capture_output=True).stdout
    assert len(out) == 8 + 16 + 12 * M * M + 8 * w * h * M, (len(out), M, w, h)
    cos_width = int(np.frombuffer(out, np.int32, 1, 0)[0])
    sec = np.frombuffer(out, np.float64, 2, 8).copy()
    cnt = np.frombuffer(out, np.int32, 3 * M * M, 24).reshape(M, M, 3).copy()
    fld = np.frombuffer(out, np.int32, 2 * w * h * M, 24 + 12 * M * M).reshape(M, h, w, 2).copy()
    assert cos_width == 4, "kfvo.cpp's cos(match_ang) no longer binds to the float overload: the port and the device use cosf"
    return cnt, fld, sec


def check(exe, kfs, cam, a, name):
    """port == reference on every count and every field cell -> (counts [M][M][4] with guard 0, fields, stats, seconds)."""
    cnt, fld, sec = run_ref(exe, kfs, cam, a)
    st, fields = port.Stats(), []
    got = port.covisibility(kfs, cam, a["field_radius"], a["match_mod"], a["match_ang"], a["rho_tol"], a["max_r"], a["field_min_mod"], st, fields)
    assert not got[..., 3].any(), (name, "guard")
    for m, (dist, ikl) in enumerate(fields):
        assert np.array_equal(ikl, fld[m, :, :, 1]), (name, "field ikl", m, int((ikl != fld[m, :, :, 1]).sum()))
        assert np.array_equal(dist, fld[m, :, :, 0]), (name, "field dist", m, int((dist != fld[m, :, :, 0]).sum()))
    assert np.array_equal(got[..., :3], cnt), (name, "counts", got[..., :3].tolist(), cnt.tolist())
    return got, fld, st, sec


def rot(ax, ay, az):
    return synth._so3_exp(np.array([ax, ay, az], np.float64))


def crafted_keyframe(rs, kn, cam, Pose, Pos, K):
    w, h = int(cam["w"]), int(cam["h"])
    c_p = np.stack([rs.uniform(-0.4, w - 0.6, kn), rs.uniform(-0.4, h - 0.6, kn)], 1).astype(np.float32)   # (rounds into the image)
    ang = rs.uniform(0, 2 * np.pi, kn)
    # a few fixed directions among the random ones: axis-aligned segments of neighbouring KeyLines meet on whole pixels with equal |t|
    fixed = rs.rand(kn) < 0.4
    ang[fixed] = rs.choice([0.0, np.pi / 2, np.pi, 3 * np.pi / 2], fixed.sum())
    u_m = np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
    n_m = rs.uniform(3, 12, kn).astype(np.float32)
    m_m = (u_m * n_m[:, None]).astype(np.float32)
    p_m = (c_p - np.array([cam["ppx"], cam["ppy"]], np.float32)).astype(np.float32)
    rho = rs.uniform(0.3, 1.5, kn)
    s_rho = rs.uniform(0.02, 0.4, kn)
    kf = dict(p_m=p_m, c_p=c_p, u_m=u_m, m_m=m_m, n_m=n_m, rho=rho.astype(np.float64), s_rho=s_rho.astype(np.float64))
    kf.update(Pose=np.asarray(Pose, np.float64), Pos=np.asarray(Pos, np.float64), K=np.float64(K))
    return kf


def crafted(exe):
    w, h = 70, 50
    cam = camera(w, h, 34.3, 25.6, 60.0, 62.0)
    a = dict(field_radius=5, field_min_mod=0.0, match_mod=0.5, match_ang=0.9, rho_tol=1.5, max_r=3.0)
    kns = [0, 1, 65, 257, 600]
    # small motions between the large lists (matches), a sideways look and a camera that has walked past the scene (behind, borders)
    poses = [(rot(0, 0, 0), [0, 0, 0], 1.0), (rot(0.02, -0.03, 0.01), [0.1, 0, 0.05], 1.2), (rot(0, 0.5, 0.1), [0.6, -0.2, 0.1], 0.8),
             (rot(0.03, 0.05, -0.04), [-0.15, 0.1, 1.4], 1.1), (rot(-0.02, 0.01, 0.03), [0.05, -0.05, 0.0], 0.9)]
    for seed in range(100):
        rs = np.random.RandomState(seed)
        kfs = [crafted_keyframe(rs, kn, cam, *p) for kn, p in zip(kns, poses)]
        got, fld, st, sec = check(exe, kfs, cam, a, f"crafted seed {seed}")
        if all(st.get(k, 0) > 0 for k in REQUIRED):
            break
    else:
        raise SystemExit(f"crafted: no seed populates every branch; last stats {dict(st)}")
    missing = [k for k in REQUIRED if st.get(k, 0) == 0]
    assert not missing, missing
    b = dict(a, field_min_mod=7.5)
    got_b, fld_b, st_b, _ = check(exe, kfs, cam, b, "crafted min_mod")
    assert st_b["field_min_mod_skipped"] > 0 and st["field_min_mod_skipped"] == 0 and not np.array_equal(got_b, got)
    rec = pack(kfs, cam, a, got, fld, st, sec)
    rec.update(seed=np.int32(seed), min_mod_b=np.float32(b["field_min_mod"]), counts_b=got_b[..., :3].copy(),
               field_dist_b=fld_b[..., 0].astype(np.int8), field_ikl_b=fld_b[..., 1].astype(np.int16),
               stat_b_names=np.array(sorted(st_b)), stat_b_values=np.array([st_b[k] for k in sorted(st_b)], np.int64))
    print(f"crafted: seed {seed} counts\n{got[..., :3].transpose(2, 0, 1)}\nstats {dict(st)}\nmin_mod stats {dict(st_b)}")
    return rec


def pack(kfs, cam, a, got, fld, st, sec):
    rec = {f"cam_{k}": np.asarray(v) for k, v in cam.items()}
    rec.update({f"arg_{k}": np.asarray(v, np.int32 if k == "field_radius" else np.float32) for k, v in a.items()})
    rec["n_kf"] = np.int32(len(kfs))
    for m, kf in enumerate(kfs):
        for k, v in kf.items():
            rec[f"kf{m}_{k}"] = np.asarray(v)
    keys = sorted(st)
    rec.update(counts=got[..., :3].copy(), field_dist=fld[..., 0].astype(np.int8), field_ikl=fld[..., 1].astype(np.int16),
               stat_names=np.array(keys), stat_values=np.array([st[k] for k in keys], np.int64), ref_seconds=sec)
    assert fld[..., 0].max() < 128 and fld[..., 1].max() < 32768
    return rec


def chained(exe, w=256, h=192, n_frames=7, keep=5, thin=3):
    from oracle import oracle
    params = oracle.euroc_params(w, h)
    orc = oracle.Oracle("ref", params)
    kfs = []
    for k, (f, _, _) in enumerate(synth.billboard_sequence(w, h, n_frames)):
        orc.process_frame(f, 0.05 * k)
        st = orc.seq_state()
        kl = orc.keylines(orc.cur_slot()).copy()
        kfs.append(port.keyframe(kl[k % thin::thin], np.array(st.Pose[:]).reshape(3, 3), np.array(st.Pos[:]), st.K))
    orc.close()
    kfs = kfs[n_frames - keep:]
    cam = camera(w, h, params.ppx, params.ppy, params.zfx, params.zfy)
    a = dict(field_radius=int(params.search_range), field_min_mod=0.0, match_mod=float(params.match_thresh_module),
             match_ang=float(np.float32(np.deg2rad(params.match_thresh_angle))), rho_tol=3.0, max_r=float(params.search_range))
    got, fld, st, sec = check(exe, kfs, cam, a, "chained")
    assert all(len(kf["n_m"]) > 100 for kf in kfs) and got[..., 1].min() > 0, "the chained key frames should see each other"
    print(f"chained: kn {[len(kf['n_m']) for kf in kfs]} counts\n{got[..., :3].transpose(2, 0, 1)}\nref seconds {sec} stats {dict(st)}")
    return pack(kfs, cam, a, got, fld, st, sec)


def write(path, rec):
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= SIZE_LIMIT, (path, size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF", "/root/reference"))
    a = ap.parse_args()
    os.makedirs(GOLD, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="keyframe_covis_ref_") as tmp:
        exe = build_driver(a.ref, tmp)
        write(os.path.join(GOLD, "crafted.npz"), crafted(exe))
        write(os.path.join(GOLD, "chained.npz"), chained(exe))


if __name__ == "__main__":
    main()
