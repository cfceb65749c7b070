#!/usr/bin/env python3
"""Device time of the compressed edge map's receiving side per stage for a batch of sequences — edgehip_edgemap_decode,
edgehip_edgemap_hide_visible, and edgehip_depth_fill_segments (the item pass and the fill) — and the compiled reference's Decode,
HideVisible and fillDepthMap chain on one CPU core for one of the lists.

    python tools/edgemap_decode_timing.py [--nseq 1024 64] [--w 752 --h 480] [--reps 20] [--out profiles/edgemap_decode_timing.txt]

The records are real: the sequences run seven frames of synth.billboard_sequence through edgehip_process_frame, edgehip_edgemap_compress
packs the OLD slot of the last frame, and the decoder reads the store it leaves (records and rho_scale) without a host round trip.
Stage times come from edgehip_edgemap_decode_ms (HIP events, under edgehip_profile_enable).  The reference leg needs
oracle/_ref/edgemap_decode_ref_driver (built by tools/make_edgemap_decode_golden.py) and is left out without it."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rebvo_amd import edgehip, synth  # noqa: E402
from tests import edgemap_crafted  # noqa: E402
from tests import edgemap_decode_crafted as crafted  # noqa: E402
from tests import edgemap_decode_port as port  # noqa: E402

P = dict(min_line_len=3, max_line_len=50, max_angle=0.3, match_n_t=1, rho_rel_max=2.0, scale=1.0)
BLOCK, ITER_NUM, V_THRESH, A_THRESH = 10, 10, 1.0, 45.0
VIEW = crafted.nav(p=(0.1, 0.0, 0.2), w=(0.0, 0.3, 0.0))


def reference_leg(rec, params, reps):
    ref = os.path.join(ROOT, "oracle", "_ref")
    exe = os.path.join(ref, "edgemap_decode_ref_driver")
    if not os.path.exists(exe):
        return None
    zfm = float(np.float32((np.float32(params.zfx) + np.float32(params.zfy)) / np.float32(2)))
    payload = crafted.payload(rec, P["scale"], V_THRESH, A_THRESH, size=(params.w, params.h), block=(BLOCK, BLOCK),
                              cam=(params.ppx, params.ppy, params.zfx, params.zfy, zfm), em_nav=crafted.nav(), views=(VIEW,), iter_num=ITER_NUM,
                              reps=reps)
    env = dict(os.environ, LD_LIBRARY_PATH=ref + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe], input=payload, check=True, capture_output=True, env=env)
    t = [float(v) for v in r.stderr.decode().split()[-4:]]
    return {"leg": "reference edgemap_com_decoder, one sequence on one CPU core", "records": len(rec),
            "segments": int(np.frombuffer(r.stdout, np.int32, 1)[0]), "ms_decode_mean": t[0], "ms_hide_visible_mean": t[1],
            "ms_fill_depth_map_mean": t[2], "ms_fill_and_chain_mean": t[3], "reps": reps}


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
    eh.edgemap_enable(a.cap_records)
    eh.edgemap_compress(slot, edgemap_crafted.params_struct(P))
    recs = eh.download_edgemaps([0, nseq - 1])
    assert all(st == 0 for _, st in recs), "the record store overflowed: raise --cap-records"
    eh.edgemap_decode_enable(a.cap_records, a.cap_items)
    eh.depth_fill_enable(BLOCK, ITER_NUM)
    DPose, DPos, _ = port.update_pos(crafted.nav(), VIEW)
    views = [(DPose, DPos, 1.0, 1.0)] * nseq
    eh.profile_enable(True)
    ms = []
    for i in range(a.reps + 3):
        eh.edgemap_decode()
        eh.edgemap_hide_visible(views)
        eh.depth_fill_segments(V_THRESH, A_THRESH)
        if i >= 3:
            ms.append(eh.edgemap_decode_ms())
    ms = np.array(ms)
    out = eh.download_edgemap_segments(list(range(nseq)))
    assert all(st == 0 for _, _, st in out), "the decoder overflowed: raise --cap-records / --cap-items"
    fixed = np.mean([g[2].sum() for g in eh.download_depth_grids(list(range(min(nseq, 8))))])
    med = np.median(ms, 0)
    lines.append({"leg": "edgemap decode + hide_visible + depth_fill_segments, all sequences in one call each", "nseq": nseq, "w": w, "h": h,
                  "block": BLOCK, "iter_num": ITER_NUM, "records_mean": float(np.mean([len(r) for r, _ in recs])),
                  "segments_mean": float(np.mean([len(s) for s, _, _ in out])), "hidden_mean": float(np.mean([(f == 0).sum() for _, f, _ in out])),
                  "fixed_cells_mean": float(fixed),
                  "ms_decode_median": float(med[0]), "ms_hide_visible_median": float(med[1]), "ms_items_median": float(med[2]),
                  "ms_fill_chain_median": float(med[3]), "ms_total_median": float(np.median(ms.sum(1))), "ms_total_min": float(ms.sum(1).min()),
                  "ms_total_max": float(ms.sum(1).max()), "reps": a.reps})
    rec, params = recs[0][0], eh.p
    eh.close()
    return rec, params


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, nargs="+", default=[1024, 64])
    ap.add_argument("--w", type=int, default=752)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cap-records", type=int, default=4096)
    ap.add_argument("--cap-items", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for nseq in a.nseq:
        rec, params = one_batch(nseq, a, lines)
    ref = reference_leg(rec, params, a.reps)
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
