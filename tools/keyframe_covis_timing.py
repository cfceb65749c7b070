#!/usr/bin/env python3
"""Device time of edgehip_keyframe_covisibility for a batch of sequences against the reference's one-core time for one sequence.

    python tools/keyframe_covis_timing.py --reference [--ref /path/to/reference] --ref-json FILE     (build machine: no GPU needed)
    python tools/keyframe_covis_timing.py --ref-json FILE [--out profiles/keyframe_covis_timing.txt]  (GPU)

Two shapes at 752x480 with --kn KeyLines per key frame: 64 sequences x 8 key frames (list capacity 7) and 1024 sequences x 2 (capacity 1).
Every sequence holds the same synthetic key frames (random KeyLines over the image, poses a few centimetres and degrees apart, so that
most KeyLines land on every other key frame's image): the work per sequence is the same as the reference's run of that one sequence.
  --reference   tools/keyframe_covis_ref_driver.cpp on one core: build_field of every key frame (what keyframe::loadFromBinaryFile does
                serially) and countMatches + kls_on_fov of every ordered pair; the seconds and the counts go to --ref-json
  GPU           the device's counts must equal the reference's; HIP-event time of the call split into field build (with the one read of
                the key frames) and pair pass, per call and per sequence, and the ratio to the reference's seconds for one sequence.
                Only the compact-SoA pair pass exists; a record-reading one was not built.
Prints one JSON line per shape; --out appends them to a file.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import keyframe_covis_port as port  # noqa: E402

SHAPES = ((64, 8), (1024, 2))
ARGS = dict(field_radius=40, field_min_mod=0.0, match_mod=1.0, match_ang=float(np.float32(np.deg2rad(45.0))), rho_tol=3.0, max_r=40.0)


def key_frames(m, kn, cam):
    import make_keyframe_covis_golden as gen
    rs = np.random.RandomState(100 + m)
    return [gen.crafted_keyframe(rs, kn, cam, gen.rot(*(0.01 * rs.randn(3))), 0.03 * rs.randn(3), 1.0 + 0.05 * j) for j in range(m)]


def camera(w, h):
    import make_keyframe_covis_golden as gen
    from rebvo_amd import edgehip
    p = edgehip.euroc_params(w, h)
    return gen.camera(w, h, p.ppx, p.ppy, p.zfx, p.zfy), p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF", "/root/reference"))
    ap.add_argument("--ref-json", required=True)
    ap.add_argument("--kn", type=int, default=16000)
    ap.add_argument("--w", type=int, default=752)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cam, params = camera(a.w, a.h)
    if a.reference:
        import make_keyframe_covis_golden as gen
        rec = {}
        with tempfile.TemporaryDirectory(prefix="keyframe_covis_ref_") as tmp:
            exe = gen.build_driver(a.ref, tmp)
            for _, m in SHAPES:
                kfs = key_frames(m, a.kn, cam)
                runs = [gen.run_ref(exe, kfs, cam, ARGS) for _ in range(3)]
                sec = np.median([r[2] for r in runs], axis=0)
                rec[str(m)] = dict(counts=runs[0][0].tolist(), field_s=float(sec[0]), pairs_s=float(sec[1]))
                print(f"reference, {m} key frames x {a.kn} KeyLines at {a.w}x{a.h}: fields {sec[0]:.4f} s, pairs {sec[1]:.4f} s")
        with open(a.ref_json, "w") as f:
            json.dump(rec, f)
        return
    from rebvo_amd import edgehip
    with open(a.ref_json) as f:
        ref = json.load(f)
    lines = []
    for nseq, m in SHAPES:
        kfs = key_frames(m, a.kn, cam)
        p = edgehip.euroc_params(a.w, a.h, max_points=a.kn)
        eh = edgehip.EdgeHip(p, nseq=nseq, nslots=2)
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        eh.keyframe_list_enable(m - 1)
        recs = [port.records(k, edgehip.KEYLINE_DTYPE) for k in kfs]
        poses = [eh.kf_pose(k["Pose"], k["Pos"], K=float(k["K"])) for k in kfs]
        for s in range(nseq):
            for j in range(m):
                eh.upload_keyframe(s, recs[j], poses[j])
        ms = []
        for _ in range(a.reps + 1):
            got, info = eh.keyframe_covisibility(**ARGS)
            ms.append(eh.keyframe_covisibility_ms())
        eh.close()
        want = np.array(ref[str(m)]["counts"], np.int32)
        for n, name in enumerate(("kl_on_fov", "kl_match", "kls_on_fov")):
            assert (got[name] == want[None, :, :, n]).all(), name
        assert not got["guard"].any()
        fld, prs = (float(np.median([x[i] for x in ms[1:]])) for i in (0, 1))   # (the first call allocates the scratch)
        ref_s = ref[str(m)]["field_s"] + ref[str(m)]["pairs_s"]
        dev_s = (fld + prs) * 1e-3 / nseq
        lines.append(dict(leg="edgehip_keyframe_covisibility, every ordered pair of every sequence (compact-SoA pair pass), counts equal to the reference's",
                          nseq=nseq, key_frames=m, kn=a.kn, w=a.w, h=a.h, args=ARGS,
                          field_ms=[round(x[0], 3) for x in ms], pair_ms=[round(x[1], 3) for x in ms], field_ms_median=fld, pair_ms_median=prs,
                          device_s_per_sequence=dev_s, reference_one_core_s_field=ref[str(m)]["field_s"], reference_one_core_s_pairs=ref[str(m)]["pairs_s"],
                          reference_one_core_s_per_sequence=ref_s, reference_over_device=ref_s / dev_s,
                          reprojections_per_s=nseq * m * m * a.kn / (prs * 1e-3)))
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
