"""GPU: rebvo::REBVO::keyframeCovisibility on a two-object batch group (rebvo_amd/host/examples/keyframe_replay.cpp --covis) against the
C ABI: the key frames the objects end with (their key-frame files) are put into a context of two sequences with upload_keyframe, and
edgehip_keyframe_covisibility of that context gives the rows the mirror printed, count for count."""
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
CAPACITY = 4          # BatchGroup::kKfListCapacity


def test_mirror_rows_equal_the_c_abi(tmp_path):
    if not os.path.exists(EXE):
        pytest.fail("keyframe_replay not built — a broken snapshot: run __graft_entry__.build()")
    frames = [list(f for f, _, _ in synth.billboard_sequence(W, H, NFRAMES, seed=11 + s, traj_seed=13 + s)) for s in range(NOBJ)]
    np.stack([frames[s][k] for s in range(NOBJ) for k in range(NFRAMES)]).tofile(tmp_path / "frames.rgb24")
    p = edgehip.euroc_params(W, H)
    cfg = tmp_path / "cfg"
    config.write_global_config(cfg, p, keyframes=KF_SAVE_PERCENT)
    r = subprocess.run([EXE, str(cfg), str(tmp_path / "frames.rgb24"), str(NOBJ), str(NFRAMES), "1.0", "0.05", str(tmp_path) + "/",
                        "--group", "covis", "--start", "2", "--end", "6", "--covis"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    rows = {}
    for line in r.stdout.splitlines():
        if line.startswith("covis "):
            head, _, body = line.partition(":")
            _, i, _, m = head.split()
            rows[int(i)] = np.array(body.split(), np.int32).reshape(int(m), int(m), 4)
    assert sorted(rows) == list(range(NOBJ)), r.stdout[-2000:]
    lists = [edgehip.read_keyframe_file(str(tmp_path / f"kf_{i}.kf")) for i in range(NOBJ)]
    assert any(len(l) >= 2 for l in lists)            # the criterion took a key frame while saving was on: pairs off the diagonal exist
    eh = edgehip.EdgeHip(p, nseq=NOBJ, nslots=2, device=0)
    try:
        eh.keyframe_track_enable(True, KF_SAVE_PERCENT, True, in_frame_driver=False)
        eh.keyframe_list_enable(CAPACITY)
        for i, l in enumerate(lists):
            for kf in l:
                eh.upload_keyframe(i, kf["kl"], kf["pose"])
        got, info = eh.keyframe_covisibility(int(p.search_range), float(p.match_thresh_module),
                                             float(np.float32(p.match_thresh_angle * np.pi / 180.0)), 3.0, float(p.search_range))
    finally:
        eh.close()
    for i, l in enumerate(lists):
        n = min(len(l), CAPACITY + 1)
        mine = np.stack([got[i][f] for f in ("kl_on_fov", "kl_match", "kls_on_fov", "guard")], -1)
        assert rows[i].shape == (CAPACITY + 1, CAPACITY + 1, 4)
        assert np.array_equal(rows[i], mine), (i, rows[i][..., 1], mine[..., 1])
        assert (rows[i][:n, :n] >= 0).all() and (rows[i][n:] == -1).all() and (rows[i][:, n:] == -1).all()
        assert (np.diagonal(rows[i][:n, :n, 1]) > 0).all()    # a key frame matches itself
