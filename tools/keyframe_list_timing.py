#!/usr/bin/env python3
"""Device time of the key-frame list (edgehip_keyframe_list_enable) for a batch of sequences, HIP events on the context's stream.

    python tools/keyframe_list_timing.py [--nseq 1024] [--kn 16000] [--w 752 --h 480] [--frames 10] [--out profiles/keyframe_list_timing.txt]

  retire   every sequence holds a key frame of --kn KeyLines and a slot list of --kn KeyLines; edgehip_keyframe_insert of all sequences
           in a context WITHOUT the list (k_kf_decide + k_kf_copy: what the insertion cost before the list existed) and in a context
           WITH it (the same two kernels and k_kf_retire between them), alternating.  retire = with - without; the bound asked of it is
           1.5 x the time without (bytes alone: 304 B against 256 B per KeyLine, x 1.19).
  frames   edgehip_process_frame with tracking on: two contexts without the list against each other (the spread of the measurement), and a
           context with the list (capacity 4) against them, alternating, on frames that insert nothing (saving off after the first key
           frame): the list's cost there is one launch of empty workgroups per hook.
  batch    edgehip_download_keyframe_list_batch of 64 entries (a PCIe copy of 64 x kn x 168 B into pageable memory).
Prints one JSON line per leg; --out appends them to a file.
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
    ap.add_argument("--kn", type=int, default=16000)
    ap.add_argument("--w", type=int, default=752)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hip = C.CDLL("libamdhip64.so")
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

    def timed(eh, call):
        stream = C.c_void_p(eh.lib.edgehip_stream(eh.ctx))
        eh.sync()
        hip.hipEventRecord(ev0, stream)
        call()
        hip.hipEventRecord(ev1, stream)
        hip.hipEventSynchronize(ev1)
        t = C.c_float(0)
        hip.hipEventElapsedTime(C.byref(t), ev0, ev1)
        return t.value

    lines = []
    base = {"nseq": a.nseq, "w": a.w, "h": a.h}
    # ---- retire ----
    rs = np.random.RandomState(1)
    kl = np.zeros(a.kn, edgehip.KEYLINE_DTYPE)
    for f in ("m_m", "u_m", "c_p", "p_m", "p_m_0", "m_m0"):
        kl[f] = rs.uniform(-100, 100, (a.kn, 2)).astype(np.float32)
    for f in ("rho", "s_rho", "rho_nr", "s_rho_nr", "rho0", "s_rho0", "n_m0"):
        kl[f] = rs.uniform(0.01, 5, a.kn)
    for f in ("m_id", "m_id_f", "m_id_kf", "p_id", "n_id"):
        kl[f] = rs.randint(-1, a.kn, a.kn)
    kl["net_id"], kl["stereo_m_id"], kl["stereo_rho"], kl["stereo_s_rho"] = -1, -1, 1.0, 20.0
    p = edgehip.euroc_params(a.w, a.h, max_points=a.kn)
    OFF, ON = (edgehip.EdgeHip(p, nseq=a.nseq, nslots=2) for _ in range(2))
    for eh in (OFF, ON):
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        for s in range(a.nseq):
            eh.upload_keylines(s, 0, kl)
    ON.keyframe_list_enable(2)
    poses = [OFF.kf_pose() for _ in range(a.nseq)]
    for eh in (OFF, ON):
        eh.keyframe_insert(0, None, poses)          # the first key frame: nothing retires
    t_off, t_on = [], []
    for _ in range(a.reps):
        t_off.append(timed(OFF, lambda: OFF.keyframe_insert(0, None, poses)))
        t_on.append(timed(ON, lambda: ON.keyframe_insert(0, None, poses)))
    info = ON.keyframe_list_info()
    assert (info["kf_count"] == a.reps + 1).all() and (info["held"] == 2).all()
    got = ON.download_keyframe_list(a.nseq - 1, int(info["first"][-1]))[0]
    cur = OFF.download_keyframe(a.nseq - 1)[0]
    assert got.tobytes() == cur.tobytes()           # (every insertion copies the same slot list)
    off, on = float(np.median(t_off)), float(np.median(t_on))
    retire = on - off
    lines.append(dict(base, leg="edgehip_keyframe_insert of every sequence: without the list (k_kf_decide + k_kf_copy) and with it (+ k_kf_retire), alternating",
                      kn=a.kn, ms_without=[round(x, 4) for x in t_off], ms_with=[round(x, 4) for x in t_on], ms_without_median=off, ms_with_median=on,
                      retire_ms=retire, retire_over_copy=retire / off, bound=1.5,
                      copy_GBps=256.0 * a.kn * a.nseq / (off * 1e-3) / 1e9, retire_GBps=304.0 * a.kn * a.nseq / (retire * 1e-3) / 1e9))
    # ---- batch download ----
    n = min(64, a.nseq)
    seqs, ords = list(range(n)), [int(info["first"][s]) for s in range(n)]
    import time
    ON.sync()
    tb = []
    for _ in range(3):
        t0 = time.perf_counter()
        ON.download_keyframe_list(seqs, ords)
        tb.append((time.perf_counter() - t0) * 1e3)
    lines.append(dict(base, leg=f"edgehip_download_keyframe_list_batch of {n} entries of {a.kn} KeyLines (wall clock, pageable destinations, the wrapper's copies included)",
                      ms=[round(x, 3) for x in tb], MB=n * a.kn * 168 / 1e6))
    OFF.close(); ON.close()
    # ---- frames that insert nothing ----
    import torch
    mono = np.stack([np.ascontiguousarray(f[:, :, 0]) for f, _, _ in synth.billboard_sequence(a.w, a.h, a.frames + 2)])
    pool = torch.empty(mono.size + 16, dtype=torch.uint8, device="cuda")
    pool[:mono.size] = torch.from_numpy(mono.reshape(-1)).cuda()
    p = edgehip.euroc_params(a.w, a.h)
    P0, P1, L = (edgehip.EdgeHip(p, nseq=a.nseq, nslots=3) for _ in range(3))
    for eh in (P0, P1, L):
        eh.keyframe_track_enable(True, 0.985, False)     # saving off: the first key frame, then no insertion
    L.keyframe_list_enable(4)
    ms = {"p0": [], "p1": [], "list": []}
    for k in range(a.frames):
        idx = np.array([k + (s % 3) for s in range(a.nseq)], np.int32)
        t = np.full(a.nseq, 0.05 * k)
        order = [("p0", P0), ("list", L), ("p1", P1)] if k % 2 == 0 else [("p1", P1), ("list", L), ("p0", P0)]
        for name, eh in order:
            eh.bind_grey8_indexed(eh.next_slot(), pool.data_ptr(), a.frames + 2, idx)
            v = timed(eh, lambda: eh.process_frame(t))
            if k >= 3:
                ms[name].append(v)
    assert (L.read_keyframe_track()["kf_count"] == 1).all() and not L.keyframe_list_info()["held"].any()
    for eh in (P0, P1, L):
        eh.close()
    m = {k: float(np.median(v)) for k, v in ms.items()}
    lines.append(dict(base, leg="edgehip_process_frame, tracking on, no insertion: two contexts without the list (spread) and one with it (capacity 4), alternating",
                      frames_timed=len(ms["list"]), ms_without_a=[round(x, 3) for x in ms["p0"]], ms_without_b=[round(x, 3) for x in ms["p1"]],
                      ms_with=[round(x, 3) for x in ms["list"]], median_without_a=m["p0"], median_without_b=m["p1"], median_with=m["list"],
                      spread_ms=abs(m["p0"] - m["p1"]), list_cost_ms=m["list"] - 0.5 * (m["p0"] + m["p1"])))
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
