#!/usr/bin/env python3
"""Device time of edgehip_jpeg_encode for a batch of 752x480 sequences at quality 90, beside what a caller pays without it: the plain
device-to-host copy of the same raw RGB24 frames (into page-locked memory), and libjpeg on one host core (PIL, when it is installed).

    python tools/jpeg_encode_timing.py [--nseq 64 1024] [--w 752 --h 480] [--reps 10] [--out FILE] [--pil-only]

The frames are the ones bench.py replays (synth.billboard_sequence, seed 11), bound as a device pool and only read: sequence s encodes
pool frame s % 8.  HIP events around each call on the context's stream.  Prints one JSON line per leg; --out appends them to a file.
--pil-only runs the host leg alone (no GPU needed), for a machine that has PIL when the GPU machine has not.
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rebvo_amd import edgehip, synth  # noqa: E402

POOL = 8


def pil_leg(frames, reps):
    try:
        from PIL import Image
    except ImportError:
        return None
    ms, nbytes = [], 0
    for i in range(reps + 2):
        f = frames[i % len(frames)]
        im = Image.fromarray(f, "RGB")
        buf = io.BytesIO()
        t0 = time.perf_counter()
        im.save(buf, "JPEG", quality=90, subsampling=2, optimize=False)
        ms.append(1e3 * (time.perf_counter() - t0))
        nbytes = len(buf.getvalue())
    ms = ms[2:]
    return {"leg": "PIL (libjpeg-turbo) quality 90, 4:2:0, one frame on one host core", "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)),
            "bytes_last_frame": nbytes, "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--w", type=int, default=752)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cap", type=int, default=512 * 1024, help="bytes per sequence in the store")
    ap.add_argument("--out", default=None)
    ap.add_argument("--pil-only", action="store_true")
    a = ap.parse_args()
    w, h = a.w, a.h
    frames = np.stack([f.reshape(h, w, 3) for f, _, _ in synth.billboard_sequence(w, h, POOL, seed=11)])
    lines = []
    if not a.pil_only:
        import torch
        hip = C.CDLL("libamdhip64.so")
        fb = w * h * 3
        pool = torch.empty(POOL * fb + 16, dtype=torch.uint8, device="cuda")
        pool[:POOL * fb] = torch.from_numpy(frames.reshape(-1)).cuda()
        ev0, ev1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
        for nseq in a.nseq:
            eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=nseq, nslots=2)
            stream = C.c_void_p(eh.lib.edgehip_stream(eh.ctx))
            eh.bind_rgb_indexed(0, pool.data_ptr(), POOL, np.arange(nseq, dtype=np.int32) % POOL)
            eh.jpeg_enable(90, a.cap)
            ms = []
            for i in range(a.reps + 3):
                hip.hipEventRecord(ev0, stream)
                eh.jpeg_encode(0)
                hip.hipEventRecord(ev1, stream)
                hip.hipEventSynchronize(ev1)
                t = C.c_float(0)
                hip.hipEventElapsedTime(C.byref(t), ev0, ev1)
                if i >= 3:
                    ms.append(t.value)
            rec = torch.empty((nseq, 2), dtype=torch.int32, device="cuda")
            eh.jpeg_device(None, rec)
            rec = rec.cpu().numpy()
            assert not rec[:, 1].any(), "a frame did not fit: raise --cap"
            out_bytes = int(rec[:, 0].sum())
            lines.append({"leg": "edgehip_jpeg_encode (k_jpeg_encode), all sequences in one launch", "nseq": nseq, "w": w, "h": h, "quality": 90,
                          "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": a.reps,
                          "bytes_out": out_bytes, "bytes_in": nseq * fb, "ratio": out_bytes / (nseq * fb)})
            eh.close()
            # what the caller pays today: the raw frames over PCIe into page-locked memory
            dev = torch.empty((nseq, fb), dtype=torch.uint8, device="cuda")
            for s in range(nseq):
                dev[s] = pool[(s % POOL) * fb:(s % POOL + 1) * fb]
            host = torch.empty((nseq, fb), dtype=torch.uint8).pin_memory()
            ms = []
            for i in range(a.reps + 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                host.copy_(dev, non_blocking=True)
                e1.record()
                e1.synchronize()
                if i >= 2:
                    ms.append(e0.elapsed_time(e1))
            lines.append({"leg": "device-to-host copy of the same raw RGB24 frames (page-locked destination)", "nseq": nseq, "bytes": nseq * fb,
                          "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": a.reps,
                          "GB_per_s": nseq * fb / float(np.median(ms)) / 1e6})
            del dev, host
    p = pil_leg(frames, a.reps)
    lines.append(p if p else {"leg": "PIL is not installed here: the host leg was not run"})
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
