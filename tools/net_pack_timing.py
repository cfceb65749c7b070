#!/usr/bin/env python3
"""Device time of edgehip_net_pack for a batch of sequences, beside the 168-byte KeyLine export of the same lists
(edgehip_export_keylines: k_pack_keylines), the reference's own packer on one CPU core, and the fill from the records beside
edgehip_depth_fill (HIP events around each call on the context's stream).

    python tools/net_pack_timing.py [--nseq 1024] [--w 752 --h 480] [--reps 20] [--out FILE]

The KeyLines are real: the sequences run seven frames of synth.billboard_sequence through edgehip_process_frame first, and everything
reads the OLD slot of the last frame (what the reference's third thread gets).  The reference leg needs oracle/_ref/libreforacle.so and
is left out without it.  Prints one JSON line per leg; --out appends them to a file.
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


def reference_leg(w, h, frames, reps):
    from oracle import oracle
    if not oracle.available("ref"):
        return None
    orc = oracle.Oracle("ref", oracle.euroc_params(w, h))
    for k, (f, _, _) in enumerate(synth.billboard_sequence(w, h, frames)):
        orc.process_frame(f, 0.05 * k)
    s = (orc.cur_slot() + 7) % 8
    kn = orc.kn(s)
    L = orc.lib
    L.ref_copy_net_keyline.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double]
    L.ref_copy_net_keyline_nextid.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    out = np.zeros((kn, 15), np.uint8)
    ms = []
    for _ in range(reps + 3):
        t0 = time.perf_counter()
        L.ref_copy_net_keyline(orc.ctx, s, -1, out.ctypes.data, kn, 1.0)
        L.ref_copy_net_keyline_nextid(orc.ctx, s, out.ctypes.data, kn)
        ms.append(1e3 * (time.perf_counter() - t0))
    orc.close()
    ms = ms[3:]
    return {"leg": "reference copy_net_keyline + _nextid, one sequence on one CPU core", "kn": kn, "ms_median": float(np.median(ms)),
            "ms_min": float(np.min(ms)), "reps": reps}


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

    def timed(call, after=None):
        ms = []
        for i in range(a.reps + 3):
            hip.hipEventRecord(ev0, stream)
            r = call()
            hip.hipEventRecord(ev1, stream)
            hip.hipEventSynchronize(ev1)
            t = C.c_float(0)
            hip.hipEventElapsedTime(C.byref(t), ev0, ev1)
            if after:
                after(r)
            if i >= 3:
                ms.append(t.value)
        return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": a.reps}

    lines = []
    base = {"nseq": nseq, "w": w, "h": h, "kn_mean": float(np.mean(kn)), "keylines": int(np.sum(kn))}
    eh.net_enable(eh.cap)
    rec = dict(base, leg="edgehip_net_pack (k_net_pack), all sequences in one launch", bytes_per_keyline=15,
               bytes_written=int(np.sum(kn)) * 15, **timed(lambda: eh.net_pack(slot)))
    rec["GB_per_s_written"] = rec["bytes_written"] / rec["ms_median"] / 1e6
    lines.append(rec)
    seqs = list(range(nseq))
    rec = dict(base, leg="edgehip_export_keylines (k_pack_keylines, 168-byte records), all sequences in one launch", bytes_per_keyline=168,
               bytes_written=int(np.sum(kn)) * 168, **timed(lambda: eh.export_keylines(seqs), eh.export_drop))
    rec["GB_per_s_written"] = rec["bytes_written"] / rec["ms_median"] / 1e6
    lines.append(rec)
    eh.depth_fill_enable(10, 10, 1.0, 5, 0, 1)
    lines.append(dict(base, leg="edgehip_depth_fill (tracker list), 10-px blocks, IterNum 10", **timed(lambda: eh.depth_fill(slot))))
    eh.net_pack(slot)
    lines.append(dict(base, leg="edgehip_depth_fill_net (wire records), 10-px blocks, IterNum 10", **timed(lambda: eh.depth_fill_net())))
    eh.close()
    ref = reference_leg(w, h, frames, a.reps)
    if ref:
        lines.append(ref)
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
