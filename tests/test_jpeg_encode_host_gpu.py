"""GPU: the video half of the mirror library's output path on a two-object batch group (rebvo_amd/host/examples/video_replay.cpp): with
VideoSave = 1 every frame is compressed on the device and appended to the object's buffer, which is written to VideoSaveFile when the
object stops; PipeBuffer::jpeg inside the output callback has the same bytes, and with VideoNetEnabled PipeBuffer::net_packet is the
packet the reference's third thread would send.  Every frame is held to EdgeHip.jpeg_download of that frame."""
import json
import os
import subprocess

import numpy as np
import pytest

from rebvo_amd import edgehip, synth
from tests import jpeg_encode_fixtures as fx

pytestmark = pytest.mark.gpu
HDR = fx.HDR
W, H = 256, 192
T0, DT = 1.0, 0.05
N_OBJ, N_FR, POOL = 2, 5, 4
REPLAY = os.path.join(fx.ROOT, "rebvo_amd", "lib", "video_replay")


def tri(k, n):
    p = 2 * (n - 1)
    k %= p
    return k if k < n else p - k


@pytest.fixture(scope="module")
def scene():
    """the pool's frames and each one's JPEG from the C ABI (edgehip_jpeg_encode + download), once"""
    frames = np.stack([f.reshape(H, W, 3) for f, _, _ in synth.billboard_sequence(W, H, POOL)])
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=POOL, nslots=2)
    try:
        eh.jpeg_enable(90)
        eh.upload_rgb(0, frames)
        eh.jpeg_encode(0)
        jpegs = eh.jpeg_download_batch(list(range(POOL)))
    finally:
        eh.close()
    for k in range(POOL):
        assert np.array_equal(jpegs[k], fx.host_encode(frames[k], 90)[0])
    return frames, jpegs


def run(tmp_path, frames, tag, *extra):
    from tests.helpers import write_global_config
    if not os.path.exists(REPLAY):
        pytest.fail("video_replay not built — a broken snapshot: run __graft_entry__.build()")
    frames.tofile(tmp_path / "frames.rgb24")
    cfg = tmp_path / f"cfg_{tag}"
    write_global_config(cfg, edgehip.euroc_params(W, H))
    video, dump = tmp_path / f"{tag}_video", tmp_path / f"{tag}_cb"
    r = subprocess.run([REPLAY, str(cfg), str(tmp_path / "frames.rgb24"), str(POOL), str(N_OBJ), str(N_FR), str(T0), str(DT),
                        "--video", str(video), "--dump", str(dump), *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    js = json.loads(r.stdout.strip().splitlines()[-1])
    files = [np.fromfile(f"{video}.{i}.mjpeg", np.uint8) for i in range(N_OBJ)]
    calls = []
    for i in range(N_OBJ):
        raw, at, mine = open(f"{dump}.{i}.cb", "rb").read(), 0, []
        while at < len(raw):
            p_id, nj, npk = (int(v) for v in np.frombuffer(raw, np.int32, 3, at))
            at += 12
            jpg = np.frombuffer(raw, np.uint8, nj, at)
            at += nj
            pk = np.frombuffer(raw, np.uint8, npk, at) if npk >= 0 else None
            at += max(npk, 0)
            mine.append((p_id, jpg, pk))
        calls.append(mine)
    return js, files, calls


def split_frames(stream):
    """cut an MJPEG stream at SOI / EOI (inside a frame FF is followed by 00 or a marker that is neither)"""
    s = stream.tobytes()
    out, at = [], 0
    while at < len(s):
        assert s[at:at + 2] == b"\xff\xd8", at
        end = s.index(b"\xff\xd9", at) + 2
        out.append(np.frombuffer(s[at:end], np.uint8))
        at = end
    return out


def test_video_save_and_callbacks(tmp_path, scene):
    frames, jpegs = scene
    js, files, calls = run(tmp_path, frames, "save", "--net")
    assert js["callbacks"] == N_OBJ * (N_FR - 1)
    for i in range(N_OBJ):
        got = split_frames(files[i])
        assert len(got) == N_FR                                       # as many frames as were pushed
        for k in range(N_FR):
            assert np.array_equal(got[k], jpegs[tri(k + i, POOL)]), (i, k)
        assert len(calls[i]) == N_FR - 1                              # the last frame is never delivered
        for j, (p_id, jpg, pk) in enumerate(calls[i]):
            assert p_id == j and np.array_equal(jpg, jpegs[tri(j + i, POOL)]), (i, j)
            h = pk[:108].view(HDR)[0]
            assert h["w"] == W and h["h"] == H and h["encoder_type"] == 1 and h["jpeg_size"] == len(jpg) and h["max_rho"] == 20
            assert h["data_size"] == len(pk) == 108 + 15 * h["kline_num"] + len(jpg)
            assert h["kline_num"] > 100 and np.array_equal(pk[108 + 15 * h["kline_num"]:], jpg)


def test_edge_map_delay_moves_the_records(tmp_path, scene):
    frames, _ = scene
    _, _, now = run(tmp_path, frames, "d0", "--net")
    _, _, late = run(tmp_path, frames, "d2", "--net", "--delay", "2")
    for i in range(N_OBJ):
        for j in range(N_FR - 1):
            a, b = late[i][j][2], now[i][j][2]
            ha, hb = a[:108].view(HDR)[0], b[:108].view(HDR)[0]
            assert ha["jpeg_size"] == hb["jpeg_size"] and np.array_equal(a[-ha["jpeg_size"]:], b[-hb["jpeg_size"]:])   # the picture is this frame's
            if j < 2:
                assert ha["kline_num"] == 0
            else:                                                     # the records are those of two frames before
                src = now[i][j - 2][2]
                hs = src[:108].view(HDR)[0]
                assert ha["kline_num"] == hs["kline_num"] and ha["km_num"] == hs["km_num"]
                assert np.array_equal(a[108:108 + 15 * ha["kline_num"]], src[108:108 + 15 * hs["kline_num"]])


def test_buffer_that_ends_inside_frame_3(tmp_path, scene):
    frames, jpegs = scene
    want = [np.concatenate([jpegs[tri(k + i, POOL)] for k in range(N_FR)]) for i in range(N_OBJ)]
    size = len(jpegs[tri(0, POOL)]) + len(jpegs[tri(1, POOL)]) + len(jpegs[tri(2, POOL)]) // 2
    _, files, calls = run(tmp_path, frames, "cut", "--buffersize", str(size))
    assert len(files[0]) == size and np.array_equal(files[0], want[0][:size])   # frame 3 cut at the buffer's end, nothing behind it
    assert np.array_equal(files[1], want[1][:size])
    for i in range(N_OBJ):                                            # the callbacks still get whole frames
        assert [len(c[1]) for c in calls[i]] == [len(jpegs[tri(j + i, POOL)]) for j in range(N_FR - 1)]


def test_raw_frames_for_encoder_type_0(tmp_path, scene):
    frames, _ = scene
    _, files, calls = run(tmp_path, frames, "raw", "--encoder", "0")
    for i in range(N_OBJ):
        assert np.array_equal(files[i], np.concatenate([frames[tri(k + i, POOL)].reshape(-1) for k in range(N_FR)]))
        assert all(np.array_equal(c[1], frames[tri(j + i, POOL)].reshape(-1)) for j, c in enumerate(calls[i]))


def test_encoder_type_2_is_refused(tmp_path, scene):
    """The MFC hardware encoder does not exist here: an object built from parameters with EncoderType 2 does not initialise."""
    frames, _ = scene
    from tests.helpers import write_global_config
    frames.tofile(tmp_path / "frames.rgb24")
    write_global_config(tmp_path / "cfg", edgehip.euroc_params(W, H))
    r = subprocess.run([REPLAY, str(tmp_path / "cfg"), str(tmp_path / "frames.rgb24"), str(POOL), "1", "2", str(T0), str(DT),
                        "--video", str(tmp_path / "v"), "--encoder", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and "EncoderType 2 is not available" in r.stdout, r.stdout[-2000:]
