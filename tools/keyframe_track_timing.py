#!/usr/bin/env python3
"""Device time of the key-frame tracking (TrackKeyFrames) for a batch of sequences: the three repair steps and an insertion through the
stage-level entry points, and edgehip_process_frame with the feature on beside the same frames with it off (HIP events on the context's
stream), next to the reference's own one-core seconds, which the fixture generator recorded.

    python tools/keyframe_track_timing.py [--nseq 1024] [--w 752 --h 480] [--frames 8] [--out FILE]
    EDGEHIP_KF_LDS=0 python tools/keyframe_track_timing.py ...      # phase 2 with its label / key arrays in HBM instead of LDS

The KeyLines are real: the sequences run synth.billboard_sequence.  Context S keeps the key-frame store for the stage-level calls alone
(its frames are the feature-less frames); after every frame pair the three steps are timed one by one on the newest slot with the frame's
integrated pose, and the criterion's insertions follow.  Contexts ON and OFF run the same frames with the feature in the frame driver and
without it.  Prints one JSON line per leg; --out appends them to a file.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rebvo_amd import edgehip, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=1024)
    ap.add_argument("--w", type=int, default=752)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--kf-save-percent", type=float, default=0.985)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    hip = C.CDLL("libamdhip64.so")
    w, h, nseq, frames = a.w, a.h, a.nseq, a.frames
    mono = np.stack([np.ascontiguousarray(f[:, :, 0]) for f, _, _ in synth.billboard_sequence(w, h, frames + 2)])
    pool = torch.empty(mono.size + 16, dtype=torch.uint8, device="cuda")
    pool[:mono.size] = torch.from_numpy(mono.reshape(-1)).cuda()
    p = edgehip.euroc_params(w, h)
    S, ON, OFF = (edgehip.EdgeHip(p, nseq=nseq, nslots=3) for _ in range(3))
    S.keyframe_track_enable(True, a.kf_save_percent, True, in_frame_driver=False)
    ON.keyframe_track_enable(True, a.kf_save_percent, True)
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

    def timed(eh, call):
        stream = C.c_void_p(eh.lib.edgehip_stream(eh.ctx))
        eh.sync()
        hip.hipEventRecord(ev0, stream)
        r = call()
        hip.hipEventRecord(ev1, stream)
        hip.hipEventSynchronize(ev1)
        t = C.c_float(0)
        hip.hipEventElapsedTime(C.byref(t), ev0, ev1)
        return t.value, r

    ms = {k: [] for k in ("insert", "build_forward_match", "forward_correct", "back_correct", "frame_on", "frame_off")}
    counts = []
    for k in range(frames):
        idx = np.array([k + (s % 3) for s in range(nseq)], np.int32)
        t = np.full(nseq, 0.05 * k)
        if k == 1:   # the first key frame: the old frame
            ms["insert"].append(timed(S, lambda: S.keyframe_insert(S.cur_slot(), None, [S.kf_pose() for _ in range(nseq)]))[0])
        for eh in (S, ON, OFF):
            eh.bind_grey8_indexed(eh.next_slot(), pool.data_ptr(), frames + 2, idx)
        S.process_frame(t)
        S.sync()   # (the timed frames below have the device to themselves)
        t_on, t_off = timed(ON, lambda: ON.process_frame(t))[0], timed(OFF, lambda: OFF.process_frame(t))[0]
        if k < 2:
            continue
        ms["frame_on"].append(t_on); ms["frame_off"].append(t_off)
        nav = S.read_nav()
        Pose, Pos = np.array([n.Pose[:] for n in nav]), np.array([n.Pos[:] for n in nav])
        sn = S.cur_slot()
        t0, c0 = timed(S, lambda: S.keyframe_build_forward_match(sn))
        t1, c1 = timed(S, lambda: S.keyframe_forward_correct(sn, Pose, Pos))
        t2, c2 = timed(S, lambda: S.keyframe_back_correct(sn, Pose, Pos))
        ms["build_forward_match"].append(t0); ms["forward_correct"].append(t1); ms["back_correct"].append(t2)
        kn = np.array([n.kn for n in nav])
        ins = c2 < np.minimum(p.track_points, kn) * a.kf_save_percent
        counts.append({"frame": k, "kn_mean": float(kn.mean()), "fow_m0": float(c0.mean()), "fow_m": float(c1.mean()), "back_m": float(c2.mean()),
                       "inserting": int(ins.sum())})
        if ins.any():
            ms["insert"].append(timed(S, lambda: S.keyframe_insert(sn, ins, None))[0])
    guard = int(S.read_keyframe_track()["guard"].any()) | int(ON.read_keyframe_track()["guard"].any())
    rec_on = ON.read_keyframe_track()
    for eh in (S, ON, OFF):
        eh.close()
    base = {"nseq": nseq, "w": w, "h": h, "frames_timed": frames - 2, "kf_lds": os.environ.get("EDGEHIP_KF_LDS", "1"), "guard": guard}
    lines = []
    for leg in ("insert", "build_forward_match", "forward_correct", "back_correct"):
        v = ms[leg]
        lines.append(dict(base, leg=f"edgehip_keyframe_{leg}, all sequences in one launch set (ms include the counts' read-back)",
                          ms_median=float(np.median(v)), ms_min=float(np.min(v)), ms_max=float(np.max(v)), calls=len(v)))
    on, off = np.array(ms["frame_on"]), np.array(ms["frame_off"])
    steps = np.median(ms["build_forward_match"]) + np.median(ms["forward_correct"]) + np.median(ms["back_correct"])
    lines.append(dict(base, leg="edgehip_process_frame, feature on beside feature off (same frames, two contexts)", ms_on_median=float(np.median(on)),
                      ms_off_median=float(np.median(off)), ms_on_per_frame=[float(x) for x in on], ms_off_per_frame=[float(x) for x in off],
                      enabled_share_of_step=float((np.median(on) - np.median(off)) / np.median(on)), three_steps_ms=float(steps),
                      kf_count_mean=float(rec_on["kf_count"].mean())))
    lines.append(dict(base, leg="what the steps counted (means over the sequences)", per_frame=counts))
    gold = os.path.join(ROOT, "tests", "golden", "keyframe_track")
    if os.path.exists(os.path.join(gold, "chained.npz")):
        z, zc = np.load(os.path.join(gold, "chained.npz")), np.load(os.path.join(gold, "crafted.npz"))
        ref = [{"case": f"chained frame {k} ({len(z[f'f{k}_new_p_id'])} KeyLines)", "seconds_3_steps": [float(x) for x in z[f"f{k}_ref_seconds"]]}
               for k in range(1, int(z["n_frames"]))]
        ref.append({"case": f"crafted BIG ({len(zc['BIG_new_p_id'])} KeyLines)", "seconds_3_steps": [float(x) for x in zc["BIG_ref_seconds"]]})
        lines.append({"leg": "reference kfvo.cpp, one sequence on one CPU core (recorded by tools/make_keyframe_track_golden.py)", "cases": ref})
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
