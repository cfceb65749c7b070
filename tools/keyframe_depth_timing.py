#!/usr/bin/env python3
"""Device time of the key-frame depth calls for a batch of sequences against the reference's one-core time for one sequence.

    python tools/keyframe_depth_timing.py [--out profiles/keyframe_depth_timing.txt]      (GPU)

Two shapes at 752x480, 16 000 KeyLines per list of which about 80 % are linked: 64 and 1024 sequences.  Every sequence holds the same
synthetic pair and the same list of 8 key frames (tools/make_keyframe_depth_golden.py: timing_inputs — the crafted lists' noise and dropped
links), so the work per sequence is the reference's run of that one input; the reference's seconds (each function alone, the median of 3
runs on one core of the build machine) are stored in tests/golden/keyframe_depth/crafted.npz.  Legs: edgehip_keyframe_map_depth,
edgehip_keyframe_translate_depth (direction 0 without and with optim_scale, direction 1), and edgehip_keyframe_list_translate_depth over
8 positions with iters = 3.  The first call of a leg runs on freshly seeded lists and must equal the port (which the fixture generator
held against the reference) bit for bit on sequences 0, nseq / 2 and nseq - 1 (with optim_scale: K within 1e-9) before a time is
reported; the timed calls that follow run on the lists as the calls before left them (the same links, other depths).  HIP-event time of
the call (edgehip_keyframe_depth_ms), the median of --reps calls after the first; what is NOT in it: the host's copy of the poses in
and of the results out.  bytes_per_keyline is BY COUNT: the walked list's link, and for a linked KeyLine the walked fields read, the
gathered partner's fields and the written fields (the list pass counts the same fields although its records are 168-byte AoS).
Prints one JSON line per shape and leg; --out appends them to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import keyframe_depth_port as port  # noqa: E402

SHAPES = (64, 1024)
# bytes by count: (per walked KeyLine, per linked KeyLine)
#   map         link 4 | own p_m 8 + rho 8 + s_rho 8, partner p_m 8 + u_m 8, written rho 8 + s_rho 8
#   f2kf        link 4 | partner p_m 8 + rho 8 + s_rho 8, written rho 8 + s_rho 8, m_num read and written 8
#   f2kf_optim  two passes: link 4 + 4 | sums: partner 24 + own rho 8 + s_rho 8; rewrite: as f2kf 48
#   kf2f        link 4 | partner 24, written 16
BYTES = dict(map=(4, 56), f2kf=(4, 48), f2kf_optim=(8, 88), kf2f=(4, 40), list=(4, 48))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(str(s) for s in SHAPES))
    a = ap.parse_args()
    import make_keyframe_depth_golden as gen
    from rebvo_amd import edgehip
    T = gen.TIMING
    z = np.load(os.path.join(gen.GOLD, "crafted.npz"))
    assert int(z["timing_kn"]) == T["kn"]
    pair, chain, cam = gen.timing_inputs(edgehip.euroc_params(T["w"], T["h"]))
    kf = port.records(pair["kf"], edgehip.KEYLINE_DTYPE, dict(m_id_f=pair["kf"]["m_id_f"]))
    fr = port.records(pair["fr"], edgehip.KEYLINE_DTYPE, dict(m_id_kf=pair["fr"]["m_id_kf"]))
    chain_rec = [port.records(k["kl"], edgehip.KEYLINE_DTYPE, dict(m_id_f=k["kl"]["m_id_f"])) for k in chain]
    cap = max([len(fr)] + [len(r) for r in chain_rec])
    P, Tr, K = pair["Pose"], pair["Pos"], float(pair["K"])
    legs = [("map", lambda eh: eh.keyframe_map_depth(0, *gen.MAP_ARGS[1], P, Tr), lambda: port.map_depth(pair, *gen.MAP_ARGS[1])[:2], 0),
            ("f2kf", lambda eh: eh.keyframe_translate_depth(0, 0, False, P, Tr, K), lambda: port.translate(pair, 0), 0),
            ("f2kf_optim", lambda eh: eh.keyframe_translate_depth(0, 0, True, P, Tr, K), lambda: port.translate(pair, 0, True), 0),
            ("kf2f", lambda eh: eh.keyframe_translate_depth(0, 1, False, P, Tr, K), lambda: port.translate(pair, 1), 1)]
    lines = []
    for nseq in (int(s) for s in a.shapes.split(",")):
        probe = sorted({0, nseq // 2, nseq - 1})
        p = edgehip.euroc_params(T["w"], T["h"], max_points=cap)
        eh = edgehip.EdgeHip(p, nseq=nseq, nslots=2)
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        pose = eh.kf_pose(pair["kf_Pose"], pair["kf_Pos"], K=float(pair["kf_K"]))
        for tag, run, want, to_slot in legs:
            for s in range(nseq):
                eh.upload_keyframe(s, kf, pose)
                eh.upload_keylines(s, 0, fr)
            ms = []
            for r in range(a.reps + 1):
                got = run(eh)
                ms.append(eh.keyframe_depth_ms())
                if r:
                    continue
                w = want()
                w = dict(rho=w[0], s_rho=w[1]) if isinstance(w, tuple) else w
                for s in probe:
                    kl = eh.download_keylines(s, 0, want_mask=False)[0] if to_slot else eh.download_keyframe(s)[0]
                    if tag == "f2kf_optim":
                        assert abs(got["K"][s] - w["K"]) <= 1e-9 * abs(w["K"]) and np.allclose(kl["rho"], w["rho"], rtol=1e-9, atol=0, equal_nan=True), (tag, s)
                    else:
                        assert port.same_bits(kl["rho"], w["rho"]) and port.same_bits(kl["s_rho"], w["s_rho"]), (tag, s)
                assert not got["guard"].any() and (got["count"] == got["count"][0]).all()
            lines.append(line(tag, nseq, T, ms, int(got["count"][0]), T["kn"], float(z["timing_ref_seconds_" + tag]), 1))
        eh.close()
        # the list pass: 8 positions (a ring of 7 and the current key frame), iters = 3
        eh = edgehip.EdgeHip(p, nseq=nseq, nslots=2)
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        eh.keyframe_list_enable(len(chain) - 1)
        for s in range(nseq):
            for k, rec in zip(chain, chain_rec):
                eh.upload_keyframe(s, rec, eh.kf_pose(k["Pose"], k["Pos"], K=float(k["K"])))
        ms = []
        for r in range(a.reps + 1):
            got = eh.keyframe_list_translate_depth(T["iters"])
            ms.append(eh.keyframe_depth_ms())
            if r:
                continue
            w, count, _ = port.list_translate(chain, T["iters"], float(cam["zfm"]))
            assert (got["count"] == count).all() and not got["guard"].any()
            for s in probe:
                for i in (0, len(chain) - 2):
                    kl = eh.download_keyframe_list(s, i)[0]
                    assert port.same_bits(kl["rho"], w[i]["kl"]["rho"]) and port.same_bits(kl["s_rho"], w[i]["kl"]["s_rho"]), ("list", s, i)
        walked = sum(len(r) for r in chain_rec[:-1])
        lines.append(line("list", nseq, T, ms, int(got["count"][0]), walked, float(z["timing_ref_seconds_list"]), T["iters"]))
        eh.close()
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


def line(tag, nseq, T, ms, linked, walked, ref_s, passes):
    med = float(np.median(ms[1:]))
    per_walked, per_linked = BYTES[tag]
    nbytes = passes * (per_walked * walked + per_linked * linked)
    dev_s = med * 1e-3 / nseq
    return dict(leg=tag, nseq=nseq, w=T["w"], h=T["h"], kn=T["kn"], walked_keylines=walked, linked=linked, passes=passes, ms=[round(x, 4) for x in ms],
                ms_median=med, device_s_per_sequence=dev_s, reference_one_core_s_per_sequence=ref_s, reference_over_device=ref_s / dev_s,
                bytes_per_keyline_by_count=nbytes / (passes * walked), GBps_by_count=nbytes * nseq / (med * 1e-3) / 1e9)


if __name__ == "__main__":
    main()
