#!/usr/bin/env python3
"""Device time of edgehip_depth_surface for a batch of sequences (HIP events around the launch on the context's stream).

    python tools/depth_surface_timing.py [--nseq 1024] [--w 752 --h 480] [--blocks 10,5] [--reps 20] [--out FILE]

The grids are real: the sequences run seven frames of synth.billboard_sequence through edgehip_process_frame, then one
edgehip_depth_fill of the newest slot.  Per block size it times the per-cell surface alone (k_depth_surface), the image alone in
both modes (k_depth_image) and reports the image's store rate: 8 B per pixel (two fp32 planes) over its time.  For per-kernel
times run it under `rocprofv3 --kernel-trace --stats -- python tools/depth_surface_timing.py`, in a run of its own.
Prints one JSON line per measurement; --out appends them to a file.
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
    ap.add_argument("--blocks", default="10,5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    hip = C.CDLL("libamdhip64.so")
    w, h, nseq, frames = a.w, a.h, a.nseq, 7
    mono = np.stack([np.ascontiguousarray(f[:, :, 0]) for f, _, _ in synth.billboard_sequence(w, h, frames + 2)])
    pool = torch.empty(mono.size + 16, dtype=torch.uint8, device="cuda")
    pool[:mono.size] = torch.from_numpy(mono.reshape(-1)).cuda()
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=nseq, nslots=3)
    for k in range(frames):
        idx = np.array([k + (s % 3) for s in range(nseq)], np.int32)
        eh.bind_grey8_indexed(eh.next_slot(), pool.data_ptr(), frames + 2, idx)
        eh.process_frame(np.full(nseq, 0.05 * k))
    eh.sync()
    stream = C.c_void_p(eh.lib.edgehip_stream(eh.ctx))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

    def timed():
        for _ in range(3):
            eh.depth_surface()
        eh.sync()
        ms = []
        for _ in range(a.reps):
            hip.hipEventRecord(ev0, stream)
            eh.depth_surface()
            hip.hipEventRecord(ev1, stream)
            hip.hipEventSynchronize(ev1)
            t = C.c_float(0)
            hip.hipEventElapsedTime(C.byref(t), ev0, ev1)
            ms.append(t.value)
        return ms

    lines = []
    for block in (int(b) for b in a.blocks.split(",")):
        gw, gh = eh.depth_fill_enable(block, 10, 1.0, 5, 0, 1)
        eh.depth_fill(eh.cur_slot())
        for surface, mode in ((True, 0), (False, 1), (False, 2)):
            eh.depth_surface_enable(surface, mode)
            ms = timed()
            rec = {"nseq": nseq, "w": w, "h": h, "block": block, "grid": [gw, gh], "part": "surface" if surface else f"image{mode}",
                   "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": a.reps}
            if mode:
                rec["image_bytes"] = 8 * nseq * w * h
                rec["store_TBps_median"] = rec["image_bytes"] / (rec["ms_median"] * 1e-3) / 1e12
            else:
                rec["min_dist_seq0"] = eh.download_depth_surface(0)["min_dist"]
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        eh.depth_surface_enable(None)
    eh.close()
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
