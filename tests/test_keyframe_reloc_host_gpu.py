"""GPU: rebvo::REBVO::keyframeRelocalize on a two-object batch group (rebvo_amd/host/examples/keyframe_replay.cpp --relocalize) against
the C ABI: the same frames go through a context of two sequences with the key-frame tracking in the frame driver (the path
tests/test_keyframe_host_gpu.py shows to equal the mirror's byte for byte), and edgehip_keyframe_relocalize of that context's newest slot,
with the call's default pose (the newest nav record's, the running K) and seq_state's s_rho_q, gives the numbers the mirror printed, digit
for digit."""
import os
import subprocess

import numpy as np
import pytest

from rebvo_amd import config, edgehip, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rebvo_amd", "lib", "keyframe_replay")
W, H, NOBJ, NFRAMES = 256, 192, 2, 7
KF_SAVE_PERCENT = 0.985
T0, DT = 1.0, 0.05
START, END = 2, 6
CAPACITY = 4          # BatchGroup::kKfListCapacity
INTS = ("mnum", "evals", "accepted", "guard")


def test_mirror_relocalize_equals_the_c_abi(tmp_path):
    if not os.path.exists(EXE):
        pytest.fail("keyframe_replay not built — a broken snapshot: run __graft_entry__.build()")
    frames = [list(f for f, _, _ in synth.billboard_sequence(W, H, NFRAMES, seed=11 + s, traj_seed=13 + s)) for s in range(NOBJ)]
    np.stack([frames[s][k] for s in range(NOBJ) for k in range(NFRAMES)]).tofile(tmp_path / "frames.rgb24")
    p = edgehip.euroc_params(W, H)
    cfg = tmp_path / "cfg"
    config.write_global_config(cfg, p, keyframes=KF_SAVE_PERCENT)
    r = subprocess.run([EXE, str(cfg), str(tmp_path / "frames.rgb24"), str(NOBJ), str(NFRAMES), str(T0), str(DT), str(tmp_path) + "/",
                        "--group", "rl", "--start", str(START), "--end", str(END), "--relocalize", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    rows, every = {}, {}
    for line in r.stdout.splitlines():
        if line.startswith("relocalize ") and " frame " in line:          # every 2nd frame: mnum, score_ratio, Kp per position the object has
            head, _, body = line.partition(":")
            _, i, _, k, _, t = head.split()
            v = body.split()
            assert len(v) == 3, line
            every[(int(i), int(k), int(t))] = (int(v[0]), float(v[1]), float(v[2]))
        elif line.startswith("relocalize "):
            head, _, body = line.partition(":")
            _, i, _, t = head.split()
            v = body.split()
            assert len(v) == 4 + 21, line
            rows[(int(i), int(t))] = ([int(x) for x in v[:4]], [float(x) for x in v[4:]])
    assert sorted(rows) == [(i, t) for i in range(NOBJ) for t in range(CAPACITY + 1)], r.stdout[-2000:]

    eh = edgehip.EdgeHip(p, nseq=NOBJ, nslots=3, device=0)
    try:
        eh.keyframe_track_enable(True, KF_SAVE_PERCENT, False)
        eh.keyframe_list_enable(CAPACITY)
        for k in range(NFRAMES):
            eh.keyframe_set_save(START <= k < END)
            eh.upload_rgb(eh.next_slot(), np.stack([frames[s][k] for s in range(NOBJ)]))
            eh.process_frame(np.full(NOBJ, T0 + DT * k))
        q = np.array([eh.get_state(s).s_rho_q for s in range(NOBJ)])
        got, info = eh.keyframe_relocalize(eh.cur_slot(), q, int(p.search_range), 5, 2.0, 3.0)
    finally:
        eh.close()
    served = 0
    for i in range(NOBJ):
        n = int(info["held"][i]) + (1 if info["kf_count"][i] > 0 else 0)
        for t in range(CAPACITY + 1):
            it, fl = rows[(i, t)]
            g = got[i, t]
            assert [int(g[k]) for k in INTS] == it, (i, t)
            mine = [float(g["score_ratio"]), float(g["Kp"]), float(g["K"])] + list(g["X"]) + list(g["Pose"]) + list(g["Pos"])
            assert [float("%.17g" % x) for x in mine] == fl or np.array_equal(np.array(mine), np.array(fl), equal_nan=True), (i, t, mine, fl)
            if t < n:
                served += 1
                assert it[0] >= 30 and it[1] == 6 and it[3] == 0 and np.isfinite(fl).all() and fl[1] > 0      # a real re-localisation
            else:
                assert it == [-1, -1, -1, -1]
            if t < n:                                     # the last frame's periodic line saw the same state as the final print
                assert every[(i, NFRAMES - 1, t)] == (it[0], fl[0], fl[1]), (i, t)
            else:
                assert (i, NFRAMES - 1, t) not in every
    assert {4, 6} <= {k for _, k, _ in every} <= {2, 4, 6} and all(m >= 0 for m, _, _ in every.values())
    assert served >= NOBJ + 1                             # a key frame was taken while saving was on: a list position is among them
