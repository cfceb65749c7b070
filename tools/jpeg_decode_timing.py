#!/usr/bin/env python3
"""What a batch of compressed camera frames costs on its way into a slot, beside the raw upload of the same frames and the host reader:

    python tools/jpeg_decode_timing.py [--nseq 64 1024] [--w 752 --h 480] [--reps 5] [--out FILE]

The frames are the ones bench.py replays (synth.billboard_sequence, seed 11); PIL writes them at quality 90 as colour 4:2:0 and as grey,
without DRI and with one MCU row per restart interval; sequence s takes stream s % 8.  Per workload and batch:
  - edgehip_upload_jpeg from the call until the slot is ready (host clock around the call and edgehip_upload_wait: parsing, the copy
    into page-locked memory, the transfer, the three kernels), the bytes that cross the bus, and the kernels' own times
    (edgehip_jpeg_decode_ms);
  - edgehip_upload_rgb_pinned / edgehip_upload_grey8_pinned of the decoded frames, the same way;
  - the host reader (rebvo_decode_jpeg) over the batch on 16 threads.
Prints one JSON line per leg; --out appends them to a file.  Needs PIL and a GPU."""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rebvo_amd import edgehip, synth  # noqa: E402

POOL = 8


def med(v):
    return {"ms_median": float(np.median(v)), "ms_min": float(np.min(v)), "ms_max": float(np.max(v))}


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--w", type=int, default=752)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = a.w, a.h
    frames = [f.reshape(h, w, 3) for f, _, _ in synth.billboard_sequence(w, h, POOL, seed=11)]
    host = C.CDLL(os.path.join(ROOT, "rebvo_amd", "lib", "librebvohost.so"))
    host.rebvo_decode_jpeg.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    workloads = {}
    for colour in (True, False):
        for dri in (False, True):
            streams = []
            for f in frames:
                buf = io.BytesIO()
                im = Image.fromarray(f, "RGB")
                kw = dict(restart_marker_rows=1) if dri else {}
                (im if colour else im.convert("L")).save(buf, "JPEG", quality=90, **(dict(subsampling=2) if colour else {}), **kw)
                streams.append(np.frombuffer(buf.getvalue(), np.uint8))
            workloads[("colour 4:2:0" if colour else "grey") + (", one MCU row per restart interval" if dri else ", no DRI")] = (colour, streams)
    lines = []
    for nseq in a.nseq:
        eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=nseq, nslots=2)
        eh.profile_enable(True)   # upload_jpeg records the events around its kernels
        eh.jpeg_decode_enable(cap_bytes=max(len(s) for _, ss in workloads.values() for s in ss))
        pin = C.c_void_p()
        assert eh.lib.edgehip_alloc_pinned(C.c_size_t(nseq * w * h * 3), C.byref(pin)) == 0
        pinned = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_uint8)), (nseq * w * h * 3,))
        for what, (colour, streams) in workloads.items():
            batch = [streams[s % POOL] for s in range(nseq)]
            fmt = edgehip.FRAME_RGB24 if colour else edgehip.FRAME_GREY8
            wall, kern = [], []
            keep, data, size = edgehip._stream_args(batch)   # the argument arrays once: the clock sees the C call alone
            for i in range(a.reps + 2):
                eh.sync()
                t0 = time.perf_counter()
                eh._ck(eh.lib.edgehip_upload_jpeg(eh.ctx, 0, data, size, 0, nseq, fmt, None))
                eh._ck(eh.lib.edgehip_upload_wait(eh.ctx, 0))
                wall.append(1e3 * (time.perf_counter() - t0))
                kern.append(eh.jpeg_decode_ms())
            assert not eh.jpeg_decode_status(0).any()
            kern = np.array(kern[2:])
            info = [edgehip.jpeg_probe(s) for s in batch]
            lines.append({"leg": "edgehip_upload_jpeg, call to slot ready", "workload": what, "nseq": nseq, "w": w, "h": h, **med(wall[2:]),
                          "bytes_entropy": int(sum(i["entropy_length"] for i in info)), "bytes_moved": int(kern[0, 3]),
                          "ms_k_jpeg_entropy": float(np.median(kern[:, 0])), "ms_k_jpeg_idct": float(np.median(kern[:, 1])),
                          "ms_k_jpeg_pixels": float(np.median(kern[:, 2])), "reps": a.reps})
            # the raw upload of the same frames, decoded beforehand
            px = [np.zeros((h, w, 3), np.uint8) for _ in range(POOL)]
            for f, s in zip(px, streams):
                assert host.rebvo_decode_jpeg(s.ctypes.data, len(s), f.ctypes.data, f.size, None, None) == 0
            bpp = 3 if colour else 1
            for s in range(nseq):
                pinned[s * w * h * bpp:(s + 1) * w * h * bpp] = (px[s % POOL] if colour else px[s % POOL][:, :, 0]).reshape(-1)
            raw = []
            for i in range(a.reps + 2):
                eh.sync()
                t0 = time.perf_counter()
                (eh.lib.edgehip_upload_rgb_pinned if colour else eh.lib.edgehip_upload_grey8_pinned)(eh.ctx, 0, pin, 0, nseq)
                eh._ck(eh.lib.edgehip_upload_wait(eh.ctx, 0))
                raw.append(1e3 * (time.perf_counter() - t0))
            lines.append({"leg": "edgehip_upload_rgb_pinned" if colour else "edgehip_upload_grey8_pinned", "workload": what, "nseq": nseq,
                          **med(raw[2:]), "bytes": nseq * w * h * bpp, "reps": a.reps})
            # the host reader on 16 threads
            out = [np.zeros((h, w, 3), np.uint8) for _ in range(16)]

            def work(k):
                for s in range(k, nseq, 16):
                    host.rebvo_decode_jpeg(batch[s].ctypes.data, len(batch[s]), out[k].ctypes.data, out[k].size, None, None)
            cpu = []
            with ThreadPoolExecutor(16) as ex:
                for i in range(3):
                    t0 = time.perf_counter()
                    list(ex.map(work, range(16)))
                    cpu.append(1e3 * (time.perf_counter() - t0))
            lines.append({"leg": "host reader (rebvo_decode_jpeg) on 16 threads", "workload": what, "nseq": nseq, **med(cpu[1:]), "reps": 2})
        eh.lib.edgehip_free_pinned(pin)
        eh.close()
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
