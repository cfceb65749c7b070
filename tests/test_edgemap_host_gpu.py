"""GPU: the compressed edge map through the mirror library (&EdgeMapOutput CompressedEdgeMap, PipeBuffer::edge_map_compressed): the
records a callback receives equal rebvo_compress_edgemap of the callback's own KeyLine list, for members of a batch group (the third
instance of the export ring) and for an object alone; members that disagree on the keys are refused at Init()."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rebvo_amd import edgehip, synth
from tests import edgemap_crafted as crafted

pytestmark = pytest.mark.gpu
W, H = 376, 240
HOST = os.path.join(crafted.ROOT, "rebvo_amd", "lib", "librebvohost.so")
REPLAY = os.path.join(crafted.ROOT, "rebvo_amd", "lib", "ros_output_replay")
P = dict(min_line_len=3, max_line_len=40, max_angle=0.3, match_n_t=1, rho_rel_max=2.0, scale=1.0)
SECTION = "\n&EdgeMapOutput\nCompressedEdgeMap=1\nMinLineLen=3\nMaxLineLen=40\nMaxAngle=0.3\nMatchNumThresh=1\nRhoRelMax=2.0\n"


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return crafted.build_host_tool(tmp_path_factory.mktemp("edgemap_host"))


def _camera():
    p = edgehip.euroc_params(W, H)
    ppx, ppy, zfx, zfy = (np.float32(v) for v in (p.ppx, p.ppy, p.zfx, p.zfy))
    return float(ppx), float(ppy), float(zfx), float(zfy), float((zfx + zfy) / np.float32(2))


def _replay(tmp_path, n_obj, n_fr, extra):
    from tests.helpers import write_global_config
    from tests.test_batch_group_gpu import T0, DT
    if not os.path.exists(REPLAY):
        pytest.fail("ros_output_replay not built — a broken snapshot: run __graft_entry__.build()")
    frames = [f for f, _, _ in synth.billboard_sequence(W, H, 6)]
    np.stack(frames).tofile(tmp_path / "frames.rgb24")
    cfg = tmp_path / "cfg"
    write_global_config(cfg, edgehip.euroc_params(W, H))
    with open(cfg, "a") as f:
        f.write(SECTION)
    prefix = tmp_path / "out"
    r = subprocess.run([REPLAY, str(cfg), str(tmp_path / "frames.rgb24"), str(len(frames)), str(n_obj), str(n_fr), str(T0), str(DT),
                        "--compressed", str(prefix)] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    out = []
    for i in range(n_obj):
        raw, at, calls = open(f"{prefix}.{i}.cem", "rb").read(), 0, []
        while at < len(raw):
            p_id, kn, count, status, em_id = (int(v) for v in np.frombuffer(raw, np.int32, 5, at))
            scale = float(np.frombuffer(raw, np.float32, 1, at + 20)[0])
            at += 24
            kl = np.frombuffer(raw, edgehip.KEYLINE_DTYPE, kn, at).copy()
            at += 168 * kn
            rec = np.frombuffer(raw, np.uint8, 5 * max(count, 0), at).reshape(-1, 5)
            at += 5 * max(count, 0)
            calls.append((p_id, kl, count, status, em_id, scale, rec))
        out.append(calls)
    return r.stdout, out


def _check(tool, stdout, out, n_fr):
    cam = _camera()
    fitted = 0
    for i, calls in enumerate(out):
        assert len(calls) >= n_fr - 2, (i, len(calls))
        with_map = [c for c in calls if c[2] >= 0]
        assert len(with_map) >= n_fr - 2
        assert [c[4] for c in with_map] == list(range(1, len(with_map) + 1))        # the running edgemap_id
        for p_id, kl, count, status, em_id, scale, rec in with_map:
            assert len(kl) > 1000 and status == 0 and scale == 1.0
            want = crafted.host_run(tool, kl, P, 2 * len(kl) + 2, cam)
            assert want["status"] == 0 and want["count"] > 50
            assert count == want["count"] and np.array_equal(rec, want["records"]), (i, p_id, count, want["count"])
            assert f"object {i} frame {p_id}: {count} records, {5 * count} bytes (KeyLine list: {len(kl)}, {168 * len(kl)} bytes)" in stdout
            fitted += int((rec[:, 4] < 255).sum())
    assert fitted > 0


def test_group_callbacks_get_the_compressed_edge_map(tool, tmp_path):
    stdout, out = _replay(tmp_path, 2, 6, [])
    _check(tool, stdout, out, 6)


def test_an_object_alone_gets_the_compressed_edge_map(tool, tmp_path):
    stdout, out = _replay(tmp_path, 1, 5, ["--single"])
    _check(tool, stdout, out, 5)


def test_group_refuses_members_with_other_compressed_edge_map_keys(tmp_path):
    from tests.helpers import write_global_config
    cfg = tmp_path / "cfg"
    write_global_config(cfg, edgehip.euroc_params(W, H))
    host = C.CDLL(HOST)
    assert host.rebvo_group_compressed_edgemap_selftest(str(cfg).encode()) == 0
