#!/usr/bin/env python3
"""Device time of edgehip_keyframe_constraint for a batch of sequences against the reference's one-core time for one sequence.

    python tools/keyframe_constraint_timing.py [--out profiles/keyframe_constraint_timing.txt]      (GPU)

Two shapes at 752x480, 16 000 KeyLines per list, iter_max = 10, k_huber = 2: 64 and 1024 sequences, either direction.  Every sequence
holds the same synthetic pair (tools/make_keyframe_constraint_golden.py: timing_pair — the crafted lists' noise, outliers and dropped links),
so the work per sequence is the reference's run of that one pair; the reference's seconds (kfvo::OptimizeRelContraint alone, the median
of 3 runs on one core of the build machine) and its X, E/E0 and link count are stored in tests/golden/keyframe_constraint/crafted.npz.
The device's result must equal the reference's within the tests' tolerances before a time is reported.  HIP-event time of the call, split
into the link gather and the solve (one launch: iter_max + 2 evaluations, the scale pass, the 6x6 algebra), the median of --reps calls
after the allocating one; what is NOT in it: the host's copy of the poses in and of the results out.  Only the one-launch solve exists;
a launch-chain form was not built.
Prints one JSON line per shape and direction; --out appends them to a file.
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
import keyframe_constraint_port as port  # noqa: E402

SHAPES = (64, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import make_keyframe_constraint_golden as gen
    from rebvo_amd import edgehip
    T = gen.TIMING
    z = np.load(os.path.join(gen.GOLD, "crafted.npz"))
    assert int(z["timing_kn"]) == T["kn"]
    params = edgehip.euroc_params(T["w"], T["h"])
    pair, cam = gen.timing_pair(params)
    kf = port.records(pair["kf"], edgehip.KEYLINE_DTYPE, dict(m_id_f=pair["kf"]["m_id_f"]))
    fr = port.records(pair["fr"], edgehip.KEYLINE_DTYPE, dict(m_id_kf=pair["fr"]["m_id_kf"]))
    lines = []
    for nseq in SHAPES:
        p = edgehip.euroc_params(T["w"], T["h"], max_points=len(fr))
        eh = edgehip.EdgeHip(p, nseq=nseq, nslots=2)
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        pose = eh.kf_pose(pair["kf_Pose"], pair["kf_Pos"], K=float(pair["kf_K"]))
        for s in range(nseq):
            eh.upload_keyframe(s, kf, pose)
            eh.upload_keylines(s, 0, fr)
        for d in (0, 1):
            ms = []
            for _ in range(a.reps + 1):
                got = eh.keyframe_constraint(0, d, T["iter_max"], T["k_huber"], pair["Pose"], pair["Pos"], float(pair["K"]))
                ms.append(eh.keyframe_constraint_ms())
            X, ratio = z[f"timing_ref_X_dir{d}"], float(z[f"timing_ref_ratio_dir{d}"])
            assert (got["links"] == int(z[f"timing_ref_links_dir{d}"])).all() and not got["guard"].any()
            assert (np.abs(got["X"] - X) <= 1e-9 * np.abs(X) + 1e-12).all() and (np.abs(got["ratio"] - ratio) <= 1e-9 * ratio).all()
            assert all(got[k].tobytes() == np.repeat(got[k][:1], nseq, 0).tobytes() for k in ("X", "W_X", "R_X", "ratio"))   # every sequence the same bits
            gat, sol = (float(np.median([x[i] for x in ms[1:]])) for i in (0, 1))   # (the first call allocates the scratch)
            ref_s = float(z[f"timing_ref_seconds_dir{d}"])
            dev_s = (gat + sol) * 1e-3 / nseq
            evals = int(got["evals"][0])
            lines.append(dict(leg="edgehip_keyframe_constraint (gather + one-launch solve), results equal to the reference's within the tests' tolerances",
                              nseq=nseq, direction=d, kn=T["kn"], links=int(got["links"][0]), w=T["w"], h=T["h"], iter_max=T["iter_max"],
                              k_huber=T["k_huber"], evals=evals, gather_ms=[round(x[0], 3) for x in ms], solve_ms=[round(x[1], 3) for x in ms],
                              gather_ms_median=gat, solve_ms_median=sol, device_s_per_sequence=dev_s, reference_one_core_s_per_sequence=ref_s,
                              reference_over_device=ref_s / dev_s, rows_per_s=nseq * (evals + d) * T["kn"] / (sol * 1e-3)))
        eh.close()
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
