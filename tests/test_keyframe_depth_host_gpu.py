"""GPU: rebvo::REBVO::keyframeMapDepth and keyframeTranslateDepth on a two-object batch group (rebvo_amd/host/examples/keyframe_replay.cpp
--depth) against the C ABI: the same frames go through a context of two sequences with the key-frame tracking in the frame driver (the
path tests/test_keyframe_host_gpu.py shows to equal the mirror's byte for byte); edgehip_keyframe_map_depth of the newest slot after every
frame, and edgehip_keyframe_translate_depth in both directions at the end, with the newest nav record's pose and the running K, give the
numbers the mirror printed, digit for digit, and the current key frame's median s_rho the example prints."""
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


def frame_pose(eh):
    nav = eh.read_nav()
    Pose = np.array([list(n.Pose) for n in nav]).reshape(NOBJ, 3, 3)
    Pos = np.array([list(n.Pos) for n in nav])
    K = np.array([eh.get_state(s).K for s in range(NOBJ)])
    return Pose, Pos, K


def test_mirror_depth_calls_equal_the_c_abi(tmp_path):
    if not os.path.exists(EXE):
        pytest.fail("keyframe_replay not built — a broken snapshot: run __graft_entry__.build()")
    frames = [list(f for f, _, _ in synth.billboard_sequence(W, H, NFRAMES, seed=11 + s, traj_seed=13 + s)) for s in range(NOBJ)]
    np.stack([frames[s][k] for s in range(NOBJ) for k in range(NFRAMES)]).tofile(tmp_path / "frames.rgb24")
    p = edgehip.euroc_params(W, H)
    cfg = tmp_path / "cfg"
    config.write_global_config(cfg, p, keyframes=KF_SAVE_PERCENT)
    r = subprocess.run([EXE, str(cfg), str(tmp_path / "frames.rgb24"), str(NOBJ), str(NFRAMES), str(T0), str(DT), str(tmp_path) + "/",
                        "--group", "kd", "--start", str(START), "--end", str(END), "--depth"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    mapped, moved, median = {}, {}, {}
    for line in r.stdout.splitlines():
        v = line.replace(":", " ").split()
        if line.startswith("mapdepth "):
            mapped[(int(v[1]), int(v[3]))] = int(v[4])
        elif line.startswith("translate "):
            moved[(int(v[1]), int(v[3]))] = ([int(v[4]), int(v[5])], [float(x) for x in v[6:9]])
        elif line.startswith("depth "):
            median[int(v[1])] = (float(v[4]), int(v[6]))
    assert sorted(mapped) == [(i, k) for i in range(NOBJ) for k in range(1, NFRAMES)], r.stdout[-2000:]
    assert sorted(moved) == [(i, d) for i in range(NOBJ) for d in (0, 1)] and sorted(median) == list(range(NOBJ)), r.stdout[-2000:]

    eh = edgehip.EdgeHip(p, nseq=NOBJ, nslots=3, device=0)
    try:
        eh.keyframe_track_enable(True, KF_SAVE_PERCENT, False)
        eh.keyframe_list_enable(4)
        for k in range(NFRAMES):
            eh.keyframe_set_save(START <= k < END)
            eh.upload_rgb(eh.next_slot(), np.stack([frames[s][k] for s in range(NOBJ)]))
            eh.process_frame(np.full(NOBJ, T0 + DT * k))
            if k == 0:
                continue
            Pose, Pos, _ = frame_pose(eh)
            got = eh.keyframe_map_depth(eh.cur_slot(), 1e-3, 5e-2, 2.0, Pose, Pos)
            assert [int(c) for c in got["count"]] == [mapped[(i, k)] for i in range(NOBJ)], k
        assert sum(mapped.values()) > 1000                                   # real updates: the key frames had links
        Pose, Pos, K = frame_pose(eh)
        for d in (0, 1):
            got = eh.keyframe_translate_depth(eh.cur_slot(), d, d == 0, Pose, Pos, K)
            for i in range(NOBJ):
                ints, fl = moved[(i, d)]
                assert [int(got["count"][i]), int(got["guard"][i])] == ints and ints[0] > 100 and ints[1] == 0, (i, d)
                mine = [float(got[k][i]) for k in ("K", "rTr", "rTr0")]
                assert [float("%.17g" % x) for x in mine] == fl, (i, d, mine, fl)
                assert (fl[1] > 0 and fl[2] > 0 and fl[0] == fl[1] / fl[2]) if d == 0 else fl[1:] == [0.0, 0.0]
        for i in range(NOBJ):
            s = np.sort(eh.download_keyframe(i)[0]["s_rho"])
            assert (float("%.17g" % s[len(s) // 2]), len(s)) == median[i], i
    finally:
        eh.close()
