"""The reference's key-frame file (keyframe::saveKeyframes2File / loadKeyframesFromFile) in plain numpy, against the fixture the
reference's own writer and reader produced (tests/golden/keyframe_file, made by tools/make_keyframe_file_golden.py).  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from rebvo_amd import edgehip

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_file", "crafted.npz")


@pytest.fixture(scope="module")
def fixture():
    z = np.load(GOLD)
    params = edgehip.euroc_params(int(z["w"]), int(z["h"]), zfx=float(z["zfx"]), zfy=float(z["zfy"]))
    kfs = [(edgehip.KfPose.from_buffer_copy(z[f"kf{i}_pose"].tobytes()),
            np.ascontiguousarray(z[f"kf{i}_kl"]).view(edgehip.KEYLINE_DTYPE).reshape(-1)) for i in range(int(z["n"]))]
    return z, params, kfs


def test_writer_reproduces_the_reference_file(fixture, tmp_path):
    z, params, kfs = fixture
    assert [len(kl) for _, kl in kfs] == [0, 1, 333]
    path = str(tmp_path / "ours.kf")
    edgehip.write_keyframe_file(path, kfs, params)
    ours = np.fromfile(path, np.uint8)
    assert ours.tobytes() == z["our_bytes"].tobytes()                       # the bytes the reference's reader was given
    ref, mask = z["ref_bytes"], z["mask"]
    assert len(ours) == len(ref) == len(mask) == 4 + sum(256 + 8 + 72 + 4 + 168 * len(kl) for _, kl in kfs)
    assert np.array_equal(ours[mask != 0], ref[mask != 0])                  # the reference's own file, wherever a field lies
    # the mask's holes are the records' padding, bytes 36..39, and nothing else; there we write zeros
    holes = np.flatnonzero(mask == 0)
    at, want = 4, []
    for _, kl in kfs:
        at += 256 + 8 + 72 + 4
        want += [at + 168 * i + b for i in range(len(kl)) for b in (36, 37, 38, 39)]
        at += 168 * len(kl)
    assert holes.tolist() == want and not ours[holes].any()


def test_reader_returns_the_input(fixture, tmp_path):
    z, params, kfs = fixture
    path = str(tmp_path / "ref.kf")
    z["ref_bytes"].tofile(path)                                             # the reference's file, its heap bytes in the padding
    back = edgehip.read_keyframe_file(path)
    cam = edgehip.keyframe_file_camera(params)
    assert len(back) == len(kfs)
    for i, (kf, (pose, kl)) in enumerate(zip(back, kfs)):
        assert bytes(kf["pose"]) == bytes(pose) and kf["max_r"] == float(z["max_r"]) == params.search_range
        assert kf["camera"].tobytes() == cam.tobytes()
        assert cam["zfm"] == np.float32((np.float32(params.zfx) + np.float32(params.zfy)) / np.float32(2))
        for f in edgehip.KEYLINE_DTYPE.names:
            if f != "_pad0":
                assert kf["kl"][f].tobytes() == kl[f].tobytes(), (i, f)
        # and what the reference's loader read from OUR file is the same input, every field
        assert z[f"kf{i}_loaded_pose"].tobytes() == bytes(pose)
        packed = np.dtype([(n, edgehip.KEYLINE_DTYPE[n]) for n in edgehip.KEYLINE_DTYPE.names if n != "_pad0"])
        loaded = np.ascontiguousarray(z[f"kf{i}_loaded_kl"]).view(packed).reshape(-1)
        for f in packed.names:
            assert loaded[f].tobytes() == kl[f].tobytes(), (i, f)


def test_empty_list_is_a_four_byte_file(tmp_path, fixture):
    path = str(tmp_path / "empty.kf")
    edgehip.write_keyframe_file(path, [], fixture[1])
    assert open(path, "rb").read() == b"\0\0\0\0"
    assert edgehip.read_keyframe_file(path) == []


@pytest.mark.parametrize("cut", [0, 3, 4, 100, 4 + 256 + 8 + 72 + 2, -1, -169])
def test_truncated_file_fails_cleanly(fixture, tmp_path, cut):
    data = fixture[0]["our_bytes"].tobytes()
    path = str(tmp_path / "cut.kf")
    with open(path, "wb") as f:
        f.write(data[:cut])
    with pytest.raises(ValueError):
        edgehip.read_keyframe_file(path)


# ---- the mirror library's reader and writer (rebvo/keyframe.h, header only) through a small host-only program ----------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kf_host") / "keyframe_file_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "rebvo_amd", "host", "include"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "keyframe_file_host_check.cpp"), "-o", exe], check=True, timeout=120)
    return exe


def run_check(exe, src, dst):
    return subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=30)


@pytest.mark.parametrize("which", ["ref_bytes", "our_bytes"])
def test_cpp_reader_and_writer_round_trip(fixture, host_check, tmp_path, which):
    """loadKeyframesFromFile of the reference's file (heap bytes in the padding) and of ours, saveKeyframes2File of what was read: our
    bytes exactly, so the reference's under the mask."""
    z = fixture[0]
    src, dst = str(tmp_path / "in.kf"), str(tmp_path / "out.kf")
    z[which].tofile(src)
    r = run_check(host_check, src, dst)
    assert r.returncode == 0 and r.stdout.split() == ["3", "0", "1", "333"], (r.returncode, r.stdout, r.stderr)
    out = np.fromfile(dst, np.uint8)
    assert out.tobytes() == z["our_bytes"].tobytes()
    assert np.array_equal(out[z["mask"] != 0], z["ref_bytes"][z["mask"] != 0])


def test_cpp_empty_list_is_a_four_byte_file(host_check, tmp_path):
    src, dst = str(tmp_path / "in.kf"), str(tmp_path / "out.kf")
    with open(src, "wb") as f:
        f.write(b"\0\0\0\0")
    r = run_check(host_check, src, dst)
    assert r.returncode == 0 and r.stdout.split() == ["0"]
    assert open(dst, "rb").read() == b"\0\0\0\0"


@pytest.mark.parametrize("cut", [0, 3, 4, 100, 4 + 256 + 8 + 72 + 2, -1, -169])
def test_cpp_truncated_file_fails_cleanly(fixture, host_check, tmp_path, cut):
    src, dst = str(tmp_path / "cut.kf"), str(tmp_path / "out.kf")
    with open(src, "wb") as f:
        f.write(fixture[0]["our_bytes"].tobytes()[:cut])
    r = run_check(host_check, src, dst)
    assert r.returncode == 3 and "load failed" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert not os.path.exists(dst)
