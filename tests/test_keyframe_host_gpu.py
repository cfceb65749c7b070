"""GPU: REBVO::kf_list, startKeyFrames / endKeyFrames and the key-frame file behind the rebvo::REBVO surface
(rebvo_amd/host/examples/keyframe_replay.cpp), against the same frames through the ctypes path: every kf_<i>.kf equals, byte for byte, the
file rebvo_amd.edgehip.write_keyframe_file writes from the device's list."""
import os
import subprocess

import numpy as np
import pytest

from rebvo_amd import config, edgehip, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rebvo_amd", "lib", "keyframe_replay")
W, H, NSEQ, NFRAMES = 256, 192, 3, 7          # the frames of tests/test_keyframe_track_gpu.py::driven
KF_SAVE_PERCENT = 0.985
T0, DT = 1.0, 0.05
START, END = 2, 6


@pytest.fixture(scope="module")
def frames():
    return [list(f for f, _, _ in synth.billboard_sequence(W, H, NFRAMES, seed=11 + s, traj_seed=13 + s)) for s in range(NSEQ)]


def python_files(frames, seqs, start, end, out_dir):
    """The same sequences as one ctypes batch with tracking and the list, the save flag as startKeyFrames / endKeyFrames set it."""
    p = edgehip.euroc_params(W, H)
    eh = edgehip.EdgeHip(p, nseq=len(seqs), nslots=3, device=0)
    try:
        eh.keyframe_track_enable(True, KF_SAVE_PERCENT, False)
        eh.keyframe_list_enable(8)
        for k in range(NFRAMES):
            eh.keyframe_set_save(start is not None and start <= k < (NFRAMES if end is None else end))
            eh.upload_rgb(eh.next_slot(), np.stack([frames[s][k] for s in seqs]))
            eh.process_frame(np.full(len(seqs), T0 + DT * k))
        info = eh.keyframe_list_info()
        assert (info["overwritten"] == 0).all()
        out = []
        for i in range(len(seqs)):
            kfs = [eh.download_keyframe_list(i, j) for j in range(info["first"][i], info["first"][i] + info["held"][i])]
            cur = eh.download_keyframe(i)
            path = os.path.join(out_dir, f"py_{i}.kf")
            edgehip.write_keyframe_file(path, [(pose, kl) for kl, pose in kfs] + [(cur[1], cur[0])], p)
            out.append((open(path, "rb").read(), len(kfs) + 1))
        return out
    finally:
        eh.close()


def replay(tmp_path, frames, seqs, extra, expect=0):
    if not os.path.exists(EXE):
        pytest.fail("keyframe_replay not built — a broken snapshot: run __graft_entry__.build()")
    np.stack([frames[s][k] for s in seqs for k in range(NFRAMES)]).tofile(tmp_path / "frames.rgb24")
    cfg = tmp_path / "cfg"
    config.write_global_config(cfg, edgehip.euroc_params(W, H), keyframes=KF_SAVE_PERCENT)
    r = subprocess.run([EXE, str(cfg), str(tmp_path / "frames.rgb24"), str(len(seqs)), str(NFRAMES), str(T0), str(DT), str(tmp_path) + "/"] + extra,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == expect, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("seqs, extra", [([0], []), ([0, 1, 2], ["--group", "kf"])])
def test_key_frame_files_equal_the_device_list(tmp_path, frames, seqs, extra):
    replay(tmp_path, frames, seqs, extra + ["--start", str(START), "--end", str(END)])
    want = python_files(frames, seqs, START, END, str(tmp_path))
    assert any(n >= 2 for _, n in want)            # the criterion took a key frame while saving was on
    for i in range(len(seqs)):
        got = open(tmp_path / f"kf_{i}.kf", "rb").read()
        assert got == want[i][0], (i, len(got), len(want[i][0]))


def test_without_start_the_file_holds_the_first_key_frame_alone(tmp_path, frames):
    out = replay(tmp_path, frames, [0, 1, 2], ["--group", "kf1"])
    want = python_files(frames, [0, 1, 2], None, None, str(tmp_path))
    for i in range(NSEQ):
        assert f"object {i}: 1 key frames" in out
        got = open(tmp_path / f"kf_{i}.kf", "rb").read()
        assert got == want[i][0] and want[i][1] == 1
        assert len(edgehip.read_keyframe_file(str(tmp_path / f"kf_{i}.kf"))) == 1


def test_a_group_with_disagreeing_track_key_frames_is_refused(tmp_path, frames):
    out = replay(tmp_path, frames, [0, 1], ["--group", "kf2", "--disagree"], expect=4)
    assert "object 1: Init failed" in out and "TrackKeyFrames" in out


def test_map_prints_one_count_per_key_frame(tmp_path, frames):
    out = replay(tmp_path, frames, [0], ["--start", str(START), "--end", str(END), "--map"])
    n = len(edgehip.read_keyframe_file(str(tmp_path / "kf_0.kf")))
    views = [l for l in out.splitlines() if l.startswith("view ")]
    assert n >= 1 and len(views) == n, out[-2000:]
    assert all(" cells hidden" in l for l in views)
