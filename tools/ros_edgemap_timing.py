#!/usr/bin/env python3
"""Device time of edgehip_ros_pack (k_ros_pack) for a batch of sequences, for each record kind, and the host-side time until 8 and 64
sequences' point clouds are in host memory, beside edgehip_download_keylines_batch (the 168-byte KeyLine records) for the same
sequences in the same run.

    python tools/ros_edgemap_timing.py [--nseq 1024] [--w 752 --h 480] [--reps 20] [--out FILE]

The KeyLines are real: the sequences run seven frames of synth.billboard_sequence through edgehip_process_frame first, and everything
reads the OLD slot of the last frame (what an output callback gets).  Kernel legs: HIP events around the call on the context's stream.
Host legs: wall clock around pack + download (the cloud) and around the batch download (the KeyLine lists), each ending with the data
in host memory.  Prints one JSON line per leg; --out appends them to a file.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rebvo_amd import edgehip, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=1024)
    ap.add_argument("--w", type=int, default=752)
    ap.add_argument("--h", type=int, default=480)
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
    slot = (eh.cur_slot() - 1) % 3
    kn = eh.get_kn(slot)
    stream = C.c_void_p(eh.lib.edgehip_stream(eh.ctx))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

    def timed(call):
        ms = []
        for i in range(a.reps + 3):
            hip.hipEventRecord(ev0, stream)
            call()
            hip.hipEventRecord(ev1, stream)
            hip.hipEventSynchronize(ev1)
            t = C.c_float(0)
            hip.hipEventElapsedTime(C.byref(t), ev0, ev1)
            if i >= 3:
                ms.append(t.value)
        return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": a.reps}

    def wall(call):
        ms = []
        for i in range(a.reps + 3):
            eh.sync()
            t0 = time.perf_counter()
            call()
            if i >= 3:
                ms.append(1e3 * (time.perf_counter() - t0))
        return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": a.reps}

    lines = []
    base = {"nseq": nseq, "w": w, "h": h, "kn_mean": float(np.mean(kn)), "keylines": int(np.sum(kn))}
    for what, name, per in ((1, "points", 12), (2, "Keyline.msg records", 52), (3, "points + records", 64)):
        eh.ros_enable(what)
        rec = dict(base, leg=f"edgehip_ros_pack (k_ros_pack), {name}, all sequences in one launch", what=what, bytes_per_keyline=per,
                   bytes_written=int(np.sum(kn)) * per, **timed(lambda: eh.ros_pack(slot)))
        rec["GB_per_s_written"] = rec["bytes_written"] / rec["ms_median"] / 1e6
        lines.append(rec)
    eh.ros_enable(1)
    for n in (8, 64):
        if n > nseq:
            continue
        seqs = np.arange(n, dtype=np.int32) * (nseq // n)
        pts = [np.zeros(eh.cap, edgehip.ROS_POINT_DTYPE) for _ in range(n)]
        kls = [np.zeros(eh.cap, edgehip.KEYLINE_DTYPE) for _ in range(n)]
        for b in pts + kls:   # page-locked destinations for both, as a batch group gives its callbacks
            eh._ck(eh.lib.edgehip_register_host(C.c_void_p(b.ctypes.data), C.c_size_t(b.nbytes)))
        pp = (C.c_void_p * n)(*[b.ctypes.data for b in pts])
        pk = (C.c_void_p * n)(*[b.ctypes.data for b in kls])
        kno = np.zeros(n, np.int32)
        ps = seqs.ctypes.data_as(C.c_void_p)

        def cloud():
            eh.ros_pack(slot)
            eh._ck(eh.lib.edgehip_download_ros_edgemaps_batch(eh.ctx, n, ps, pp, None, kno.ctypes.data_as(C.c_void_p)))

        def aos():
            eh._ck(eh.lib.edgehip_download_keylines_batch(eh.ctx, slot, n, ps, pk, kno.ctypes.data_as(C.c_void_p)))
        kn_n = int(np.sum(kn[seqs]))
        lines.append(dict(base, leg=f"edgehip_ros_pack (whole batch) + edgehip_download_ros_edgemaps_batch: clouds of {n} sequences on the host",
                          sequences=n, bytes_to_host=kn_n * 12, **wall(cloud)))
        lines.append(dict(base, leg=f"edgehip_download_keylines_batch: 168-byte KeyLine lists of {n} sequences on the host",
                          sequences=n, bytes_to_host=kn_n * 168, **wall(aos)))
        for b in pts + kls:
            eh._ck(eh.lib.edgehip_unregister_host(C.c_void_p(b.ctypes.data)))
    eh.close()
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
