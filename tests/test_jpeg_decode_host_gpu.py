"""GPU: compressed camera frames through the mirror library (rebvo_amd/host/examples/mjpeg_replay.cpp): a two-object batch group fed
from .mjpeg files through REBVO::pushCustomCamJpeg with &GPU CompressedUpload = 1 — the frames cross the bus as JPEG and the device decodes
them — against the same frames decoded by the host reader and fed through requestCustomCamBuffer (--raw): the nav records digit for
digit.  A step with a member the device does not take (a progressive file) falls back to the host reader and still matches."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from rebvo_amd import edgehip, synth
from tests import jpeg_decode_fixtures as fx

pytestmark = pytest.mark.gpu
W, H = 256, 192
T0, DT = 1.0, 0.05
N_OBJ, N_FR, POOL = 2, 6, 4
REPLAY = os.path.join(fx.ROOT, "rebvo_amd", "lib", "mjpeg_replay")


@pytest.fixture(scope="module")
def streams():
    """the pool's frames as the device encoder writes them (what video_replay saves): 4:2:0, no DRI"""
    frames = np.stack([f.reshape(H, W, 3) for f, _, _ in synth.billboard_sequence(W, H, POOL)])
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=1, nslots=2)
    try:
        return [g[0] for g in eh.jpeg_encode_images(frames, 90)]
    finally:
        eh.close()


def run(tmp_path, tag, files, *extra):
    from tests.helpers import write_global_config
    if not os.path.exists(REPLAY):
        pytest.fail("mjpeg_replay not built — a broken snapshot: run __graft_entry__.build()")
    cfg = tmp_path / f"cfg_{tag}"
    write_global_config(cfg, edgehip.euroc_params(W, H))
    paths = []
    for i, frames in enumerate(files):
        paths.append(str(tmp_path / f"{tag}_{i}.mjpeg"))
        np.concatenate(frames).tofile(paths[-1])
    r = subprocess.run([REPLAY, str(cfg), str(N_OBJ), str(N_FR), str(T0), str(DT), *extra, *paths], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, REBVO_GROUP_TIMING="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    js = json.loads(lines[-1])
    nav = [ln for ln in lines if ln.startswith("nav ")]
    assert len(nav) == N_OBJ and js["objects"] == N_OBJ and js["frames_per_object"] == N_FR
    m = re.search(r"(\d+) steps \(.*; (\d+) steps went up compressed", r.stdout)
    assert m, r.stdout[-2000:]
    return nav, js, int(m.group(1)), int(m.group(2))


def test_compressed_against_raw(tmp_path, streams):
    """object 0 reads the pool forwards, object 1 backwards; with a callback PipeBuffer::imgc is the host reader's frame either way"""
    files = [streams, streams[::-1]]
    nav_c, js_c, steps_c, comp_c = run(tmp_path, "c", files, "--callback")
    nav_r, js_r, steps_r, comp_r = run(tmp_path, "r", files, "--raw", "--callback")
    assert nav_c == nav_r                                   # 17 significant digits of t, Pos, Vel, RotLie, PoseLie per object
    assert float(nav_c[0].split()[2]) == pytest.approx(T0 + DT * (N_FR - 1))
    assert steps_c == steps_r == N_FR and comp_c == N_FR and comp_r == 0 and js_c["raw"] == 0 and js_r["raw"] == 1
    assert js_c["callbacks"] == js_r["callbacks"] > 0 and js_c["imgc_sum"] == js_r["imgc_sum"] > 0
    assert any(abs(float(v)) > 1e-9 for v in nav_c[0].split()[3:])   # something was tracked


def test_a_progressive_member_falls_back(tmp_path, streams):
    """object 1's second and fifth frames are progressive files: those steps go up raw (object 0's frame by the host reader on the group's
    thread, object 1's at the push), the others compressed, and the records still equal the raw run's"""
    prog = fx.fixtures()["mosaic_256x192_progressive"]["jpeg"]
    assert edgehip.jpeg_probe(prog)["reason"] == fx.PROGRESSIVE and edgehip.jpeg_probe(prog)["w"] == 0   # (SOF2: refused before the size is read)
    files = [streams, [streams[1], prog, streams[2], streams[3]]]
    nav_c, _, steps_c, comp_c = run(tmp_path, "pc", files)
    nav_r, _, steps_r, comp_r = run(tmp_path, "pr", files, "--raw")
    assert nav_c == nav_r
    assert steps_c == steps_r == N_FR and comp_c == N_FR - 2 and comp_r == 0   # frames 1 and 5 (k % 4 == 1) are the progressive one


def test_raw_video_of_a_compressed_step_is_the_host_decoded_frame(tmp_path, streams):
    """VideoSave with EncoderType 0 on compressed steps: the saved raw frames are the host reader's decode of the frames pushed, in order
    (the ring entry holds no pixels on such a step until the host reader is asked for them)."""
    files = [streams, streams[::-1]]
    video = tmp_path / "rawvideo"
    _, _, steps, comp = run(tmp_path, "v", files, "--rawvideo", str(video))
    assert steps == comp == N_FR
    want = [fx.host_decode(s) for s in streams]
    for i, order in enumerate((want, want[::-1])):
        saved = np.fromfile(f"{video}.{i}.rgb24", np.uint8)
        assert saved.size == N_FR * H * W * 3, (i, saved.size)
        for k, fr in enumerate(saved.reshape(N_FR, H, W, 3)):
            assert np.array_equal(fr, order[k % POOL]), (i, k)
