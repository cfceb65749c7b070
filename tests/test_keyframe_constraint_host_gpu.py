"""GPU: rebvo::REBVO::keyframeConstraint on a two-object batch group (rebvo_amd/host/examples/keyframe_replay.cpp --constraint) against
the C ABI: the same frames go through a context of two sequences with the key-frame tracking in the frame driver (the path
tests/test_keyframe_host_gpu.py shows to equal the mirror's byte for byte), and edgehip_keyframe_constraint of that context's newest slot,
with the newest nav record's pose and the running K, gives the numbers the mirror printed, digit for digit."""
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
FLOATS = ("ratio", "E", "E0", "Kp", "W_Kp")
INTS = ("links", "inliers", "evals", "accepted", "guard")


def test_mirror_constraint_equals_the_c_abi(tmp_path):
    if not os.path.exists(EXE):
        pytest.fail("keyframe_replay not built — a broken snapshot: run __graft_entry__.build()")
    frames = [list(f for f, _, _ in synth.billboard_sequence(W, H, NFRAMES, seed=11 + s, traj_seed=13 + s)) for s in range(NOBJ)]
    np.stack([frames[s][k] for s in range(NOBJ) for k in range(NFRAMES)]).tofile(tmp_path / "frames.rgb24")
    p = edgehip.euroc_params(W, H)
    cfg = tmp_path / "cfg"
    config.write_global_config(cfg, p, keyframes=KF_SAVE_PERCENT)
    r = subprocess.run([EXE, str(cfg), str(tmp_path / "frames.rgb24"), str(NOBJ), str(NFRAMES), str(T0), str(DT), str(tmp_path) + "/",
                        "--group", "kc", "--start", str(START), "--end", str(END), "--constraint"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    rows = {}
    for line in r.stdout.splitlines():
        if line.startswith("constraint "):
            head, _, body = line.partition(":")
            _, i, _, d = head.split()
            v = body.split()
            assert len(v) == 16, line
            rows[(int(i), int(d))] = ([float(x) for x in v[:11]], [int(x) for x in v[11:]])
    assert sorted(rows) == [(i, d) for i in range(NOBJ) for d in (0, 1)], r.stdout[-2000:]

    eh = edgehip.EdgeHip(p, nseq=NOBJ, nslots=3, device=0)
    try:
        eh.keyframe_track_enable(True, KF_SAVE_PERCENT, False)
        eh.keyframe_list_enable(4)
        for k in range(NFRAMES):
            eh.keyframe_set_save(START <= k < END)
            eh.upload_rgb(eh.next_slot(), np.stack([frames[s][k] for s in range(NOBJ)]))
            eh.process_frame(np.full(NOBJ, T0 + DT * k))
        nav = eh.read_nav()
        Pose = np.array([list(n.Pose) for n in nav]).reshape(NOBJ, 3, 3)
        Pos = np.array([list(n.Pos) for n in nav])
        K = np.array([eh.get_state(s).K for s in range(NOBJ)])
        for d in (0, 1):
            got = eh.keyframe_constraint(eh.cur_slot(), d, 10, 2.0, Pose, Pos, K)
            for i in range(NOBJ):
                fl, it = rows[(i, d)]
                mine = list(got["X"][i]) + [float(got[k][i]) for k in FLOATS]
                assert [float("%.17g" % x) for x in mine] == fl or np.array_equal(np.array(mine), np.array(fl), equal_nan=True), (i, d, mine, fl)
                assert [int(got[k][i]) for k in INTS] == it, (i, d)
                assert it[0] >= 30 and it[2] == 12 and it[4] == 0          # a real constraint: links, every evaluation ran, no guard
                assert np.isfinite(fl).all() and 0 < fl[6] <= 1 and (fl[9] > 0) == (d == 1)
    finally:
        eh.close()
