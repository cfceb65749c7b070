#!/usr/bin/env python3
"""Device time of edgehip_edgemap_compress per stage for a batch of sequences, its bytes out beside the 15-byte wire records of the same
lists (k_net_pack), and the compiled reference's compress_edgemap on one CPU core for one of the lists.

    python tools/edgemap_compress_timing.py [--nseq 1024 64] [--w 752 --h 480] [--reps 20] [--out profiles/edgemap_compress_timing.txt]

The KeyLines are real: the sequences run seven frames of synth.billboard_sequence through edgehip_process_frame first, and everything
reads the OLD slot of the last frame.  Stage times come from edgehip_edgemap_ms (HIP events, under edgehip_profile_enable, which runs
labelling and sort as two launches): component labelling, key sort, walks and fits (counting pass, scan, fitting pass), placement.
The reference leg needs oracle/_ref/edgemap_ref_driver (built by tools/make_edgemap_golden.py) and is left out without it."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rebvo_amd import edgehip, synth  # noqa: E402
from tests import edgemap_crafted as crafted  # noqa: E402

P = dict(min_line_len=3, max_line_len=50, max_angle=0.3, match_n_t=1, rho_rel_max=2.0, scale=1.0)


def reference_leg(kl, params, reps):
    ref = os.path.join(ROOT, "oracle", "_ref")
    exe = os.path.join(ref, "edgemap_ref_driver")
    if not os.path.exists(exe):
        return None
    hdr = np.array([len(kl), P["min_line_len"], P["max_line_len"], P["match_n_t"], 10, 0, params.w, params.h], np.int32)
    payload = hdr.tobytes() + np.array([P["scale"], P["max_angle"], P["rho_rel_max"]], np.float64).tobytes() + \
        np.array([params.ppx, params.ppy, params.zfx, params.zfy], np.float32).tobytes() + crafted.NAV.tobytes() + np.ascontiguousarray(kl).tobytes()
    env = dict(os.environ, LD_LIBRARY_PATH=ref + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, str(reps)], input=payload, check=True, capture_output=True, env=env)
    count = int(np.frombuffer(r.stdout, np.int32, 1)[0])
    return {"leg": "reference compress_edgemap, one sequence on one CPU core", "kn": len(kl), "records": count,
            "ms_mean": float(r.stderr.decode().split()[-1]), "reps": reps}


def one_batch(nseq, a, lines):
    import torch
    w, h, frames = a.w, a.h, 7
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
    eh.edgemap_enable(2 * eh.cap)
    eh.profile_enable(True)
    q = crafted.params_struct(P)
    ms = []
    for i in range(a.reps + 3):
        eh.edgemap_compress(slot, q)
        if i >= 3:
            ms.append(eh.edgemap_ms())
    ms = np.array(ms)
    cnt = torch.empty((nseq,), dtype=torch.int32, device="cuda")
    eh.edgemap_into(None, cnt)
    cnt = cnt.cpu().numpy()
    med = np.median(ms, 0)
    lines.append({"leg": "edgehip_edgemap_compress, all sequences in one call", "nseq": nseq, "w": w, "h": h, "kn_mean": float(np.mean(kn)),
                  "keylines": int(np.sum(kn)), "max_line_len": P["max_line_len"], "records_mean": float(np.mean(cnt)),
                  "ms_labelling_median": float(med[0]), "ms_sort_median": float(med[1]), "ms_walks_median": float(med[2]),
                  "ms_placement_median": float(med[3]),
                  "ms_total_median": float(np.median(ms.sum(1))), "ms_total_min": float(ms.sum(1).min()), "ms_total_max": float(ms.sum(1).max()),
                  "bytes_out": int(np.sum(cnt)) * 5, "bytes_net_keyline": int(np.sum(kn)) * 15, "bytes_keyline": int(np.sum(kn)) * 168,
                  "reps": a.reps})
    kl = eh.download_keylines(0, slot, want_mask=False)[0]
    params = eh.p
    eh.close()
    return kl, params


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, nargs="+", default=[1024, 64])
    ap.add_argument("--w", type=int, default=752)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for nseq in a.nseq:
        kl, params = one_batch(nseq, a, lines)
    ref = reference_leg(kl, params, a.reps)
    if ref:
        lines.append(ref)
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:   # (a profile's commented head is written by hand above these lines)
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
