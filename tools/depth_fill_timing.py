#!/usr/bin/env python3
"""Device time of edgehip_depth_fill for a batch of sequences (HIP events around the launch on the context's stream).

    python tools/depth_fill_timing.py [--nseq 1024] [--w 752 --h 480] [--blocks 10,5] [--iters 10] [--reps 20] [--out FILE]

The KeyLines are real: the sequences run seven frames of synth.billboard_sequence through edgehip_process_frame first (KeyLines
reach m_num >= 5), and the fill reads the OLD slot of the last frame (what an output callback gets).  --iters takes a list: IterNum 0
times the binning, fusion and coarse-fine alone.  --surface N also times N rebvo::REBVO objects of one batch group with output callbacks
through rebvo_amd/lib/surface_replay (752x480), with &DepthFiller (PixelBlockSize 10) and without: frames per second through the surface.  Prints one JSON line per block size; --out appends them to a file.
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


def surface_leg(n_obj, n_fr, w, h):
    import subprocess
    import tempfile
    from rebvo_amd.config import write_global_config
    exe = os.path.join(ROOT, "rebvo_amd", "lib", "surface_replay")
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        frames = [f for f, _, _ in synth.billboard_sequence(w, h, 8)]
        np.stack(frames).tofile(os.path.join(tmp, "frames.rgb24"))
        for fill in (False, True):
            cfg = os.path.join(tmp, f"cfg{int(fill)}")
            write_global_config(cfg, edgehip.euroc_params(w, h), gpu=dict(group=f"t{int(fill)}", size=n_obj))
            if fill:
                with open(cfg, "a") as f:
                    f.write("\n&DepthFiller\nPixelBlockSize=10\nThreshRelRho=1\nThreshMatchNum=5\nIterNum=10\n")
            r = subprocess.run([exe, cfg, os.path.join(tmp, "frames.rgb24"), str(len(frames)), str(n_obj), str(n_fr), "1.0", "0.05",
                                "--group", f"t{int(fill)}", "--callback", "--warmup", "5"], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(r.stdout[-2000:] + r.stderr[-2000:])
            js = json.loads(r.stdout.strip().splitlines()[-1])
            rec = {"leg": "surface_replay", "objects": n_obj, "frames_per_object": n_fr, "w": w, "h": h, "depth_fill": fill,
                   "fps": js["fps"], "callbacks": js["callbacks"]}
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=1024)
    ap.add_argument("--w", type=int, default=752)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--blocks", default="10,5")
    ap.add_argument("--iters", default="10,0")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--surface", type=int, default=8)
    ap.add_argument("--surface-frames", type=int, default=60)
    a = ap.parse_args()
    import torch
    hip = C.CDLL("libamdhip64.so")
    w, h, nseq, frames = a.w, a.h, a.nseq, 7
    mono = np.stack([np.ascontiguousarray(f[:, :, 0]) for f, _, _ in synth.billboard_sequence(w, h, frames + 2)])
    pool = torch.empty(mono.size + 16, dtype=torch.uint8, device="cuda")
    pool[:mono.size] = torch.from_numpy(mono.reshape(-1)).cuda()
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=nseq, nslots=3)
    for k in range(frames):
        idx = np.array([k + (s % 3) for s in range(nseq)], np.int32)   # frames + 2 in the pool
        eh.bind_grey8_indexed(eh.next_slot(), pool.data_ptr(), frames + 2, idx)
        eh.process_frame(np.full(nseq, 0.05 * k))
    eh.sync()
    slot = (eh.cur_slot() - 1) % 3
    kn = np.array([n.kn for n in eh.read_nav()])
    stream = C.c_void_p(eh.lib.edgehip_stream(eh.ctx))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    lines = []
    for block, iters in ((int(b), int(i)) for b in a.blocks.split(",") for i in a.iters.split(",")):
        gw, gh = eh.depth_fill_enable(block, iters, 1.0, 5, 0, 1)
        for _ in range(3):
            eh.depth_fill(slot)
        eh.sync()
        ms = []
        for _ in range(a.reps):
            hip.hipEventRecord(ev0, stream)
            eh.depth_fill(slot)
            hip.hipEventRecord(ev1, stream)
            hip.hipEventSynchronize(ev1)
            t = C.c_float(0)
            hip.hipEventElapsedTime(C.byref(t), ev0, ev1)
            ms.append(t.value)
        fixed = int(eh.download_depth_grid(0)[2].sum())
        rec = {"nseq": nseq, "w": w, "h": h, "block": block, "grid": [gw, gh], "iter_num": iters, "kn_mean": float(kn.mean()),
               "fixed_cells_seq0": fixed, "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)),
               "reps": a.reps}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    eh.close()
    if a.surface > 0:
        lines += surface_leg(a.surface, a.surface_frames, w, h)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
