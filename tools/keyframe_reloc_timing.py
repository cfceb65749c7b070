#!/usr/bin/env python3
"""Time of one edgehip_keyframe_relocalize call against the route the library offered before it, for the same pairs, in the same run.

    python tools/keyframe_reloc_timing.py [--out profiles/keyframe_reloc_timing.txt]        (GPU)

Two shapes at 752x480 with --kn KeyLines per key frame: 64 sequences x 8 key frames (list capacity 7) and 1024 sequences x 2 (capacity 1),
iter_max = 5.  Every sequence holds the same synthetic key frames (tools/make_keyframe_covis_golden.py's random KeyLines over the image, the
same set in every key frame, under poses a few centimetres and degrees apart); the query in ring slot 0 is the newest key frame's KeyLines under its own pose.  The pairs that
are timed are (query, list entry) for every list entry — what the older route can reach without a host copy:
  new     one edgehip_keyframe_relocalize with a to_mask that selects the list's positions: wall-clock time of the call (it synchronises) and
          its HIP-event times, prepare and solve
  before  per list position: edgehip_keyframe_list_restore into ring slot 1, then edgehip_minimizer_rv_kf (which rebuilds the field and
          synchronises) with the request the caller computes on the host (tests/keyframe_reloc_port.request); wall-clock time of the two calls,
          summed over the positions.  The host finish of that route (optimizeScale and the pose, per pair) is NOT in the time: it is
          numpy here and would dominate.
X of every pair must agree between the two (rtol 1e-9 + atol 1e-12) and mnum must be equal.  Prints one JSON line per shape; --out appends
them to a file.  The two routes alternate, --reps times; the first round is not counted (allocations)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import keyframe_covis_port as cport  # noqa: E402
import keyframe_reloc_port as port  # noqa: E402

SHAPES = ((64, 8), (1024, 2))
ARGS = dict(field_radius=40, field_min_mod=0.0, iter_max=5, rew_dis=2.0, rho_tol=3.0)
ANG = 30.0 * np.pi / 180.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kn", type=int, default=16000)
    ap.add_argument("--w", type=int, default=752)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="64x8,1024x2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import make_keyframe_covis_golden as gen
    from rebvo_amd import edgehip
    p0 = edgehip.euroc_params(a.w, a.h)
    cam = gen.camera(a.w, a.h, p0.ppx, p0.ppy, p0.zfx, p0.zfy)
    lines = []
    for nseq, m in [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]:
        rs = np.random.RandomState(100 + m)
        kfs = [gen.crafted_keyframe(rs, a.kn, cam, gen.rot(*(0.01 * rs.randn(3))), 0.03 * rs.randn(3), 1.0 + 0.05 * j) for j in range(m)]
        for k in kfs[1:]:                                    # one set of KeyLines under m poses: the minimiser has edges to match and a way to go
            for n in cport.FIELDS:
                k[n] = kfs[0][n]
        p = edgehip.euroc_params(a.w, a.h, max_points=a.kn, search_range=ARGS["field_radius"])
        eh = edgehip.EdgeHip(p, nseq=nseq, nslots=2)
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        eh.keyframe_list_enable(m - 1)
        recs = [cport.records(k, edgehip.KEYLINE_DTYPE) for k in kfs]
        poses = [eh.kf_pose(k["Pose"], k["Pos"], K=float(k["K"])) for k in kfs]
        for s in range(nseq):
            for j in range(m):
                eh.upload_keyframe(s, recs[j], poses[j])
            eh.upload_keylines(s, 0, recs[m - 1])
        qpose = [poses[m - 1]] * nseq
        mask = np.ones((nseq, m), np.uint8)
        mask[:, m - 1] = 0                                   # the list's positions: the pairs the older route reaches by a restore
        s_rho_q = 1e3
        new_wall, new_ms, old_wall = [], [], []
        first = None
        for _ in range(a.reps + 1):                          # the two routes alternate: the same neighbours on a shared machine
            t0 = time.perf_counter()
            got, info = eh.keyframe_relocalize(0, s_rho_q, poses=qpose, to_mask=mask, **ARGS)
            new_wall.append((time.perf_counter() - t0) * 1e3)
            new_ms.append(eh.keyframe_relocalize_ms())
            first = info["first"].astype(np.int32)
            tot = 0.0
            for j in range(m - 1):
                qp = (kfs[m - 1]["Pose"], kfs[m - 1]["Pos"], float(kfs[m - 1]["K"]))
                kp = (kfs[j]["Pose"], kfs[j]["Pos"], float(kfs[j]["K"]))
                X0, Kr = port.request(*qp, *kp)
                t0 = time.perf_counter()
                eh.keyframe_list_restore(1, first + j)
                r = eh.minimizer_rv_kf(1, 0, X0, Kr, s_rho_q, 5.0, ANG, ARGS["rho_tol"], ARGS["iter_max"], ARGS["rew_dis"], 0)
                tot += (time.perf_counter() - t0) * 1e3
                assert np.allclose(got["X"][:, j], r["X"], rtol=1e-9, atol=1e-12), j
                assert np.array_equal(got["mnum"][:, j], r["mnum"]), j
            old_wall.append(tot)
        eh.close()
        nw, ow = float(np.median(new_wall[1:])), float(np.median(old_wall[1:]))
        lines.append(dict(leg="edgehip_keyframe_relocalize (one call, list positions selected) against restore + edgehip_minimizer_rv_kf per position "
                              "(host finish of the older route not timed); X and mnum of every pair agree",
                          nseq=nseq, key_frames=m, pairs=nseq * (m - 1), kn=a.kn, w=a.w, h=a.h, args=ARGS,
                          new_wall_ms=[round(x, 3) for x in new_wall], new_prepare_ms=[round(x[0], 3) for x in new_ms],
                          new_solve_ms=[round(x[1], 3) for x in new_ms], before_wall_ms=[round(x, 3) for x in old_wall],
                          new_wall_ms_median=nw, new_device_ms_median=float(np.median([x[0] + x[1] for x in new_ms[1:]])),
                          before_wall_ms_median=ow, before_over_new=ow / nw, mnum_median=int(np.median(got["mnum"][:, :m - 1]))))
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
