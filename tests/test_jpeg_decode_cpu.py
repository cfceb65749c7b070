"""CPU: the device JPEG decoder's parts that run on the host — the shared marker parser (rebvo/jpeg_decode.h), the host instantiation of
the chain walk (csrc/jpeg_entropy.h) with the pixel stage's restatement over the kernels' own functions (csrc/jpeg_pixels.h), and the
walk's bounds under corruption (tools/jpeg_entropy_guard.cpp, a stand-alone program built here with the host compiler).  The yardstick
is PIL's decode, stored in tests/golden/jpeg_decode by tools/make_jpeg_decode_golden.py.  No GPU, no PIL."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import jpeg_decode_fixtures as fx
from tests import jpeg_encode_fixtures as enc

FIX = fx.fixtures()
DEC = fx.decodable()


def test_fixture_set_covers_the_populations():
    assert len(FIX) == 48 and len(DEC) == 46
    for samp in fx.SAMPLING:
        for w, h in fx.SIZES:
            assert any(f["sampling"] == samp for n, f in DEC.items() if n in fx.of_size(w, h)), (samp, w, h)
    top = {k: max(f["stats"][k] for f in DEC.values()) for k in fx.STATS}
    assert top["stuffed"] >= 5 and top["long_codes"] >= 1 and top["zrl"] >= 1 and top["no_eob"] >= 1, top
    assert top["max_dc_cat"] == 11 and top["max_ac_cat"] == 10 and top["groups"] >= 4, top
    assert sum(os.path.getsize(os.path.join(fx.GOLD, n + ".npz")) for n in FIX) < 400 * 1024


@pytest.mark.parametrize("name", sorted(DEC))
def test_parser_on_fixture(name):
    f = DEC[name]
    info = fx.probe(f["jpeg"])
    h, w = f["rgb"].shape[:2]
    assert info["reason"] == fx.OK
    assert (info["w"], info["h"]) == (w, h)
    assert (info["components"], info["hsamp"], info["vsamp"]) == fx.SAMPLING[f["sampling"]]
    b = f["jpeg"].tobytes()
    sos = b.index(b"\xff\xda")
    assert info["entropy_offset"] == sos + 4 + (b[sos + 2] << 8 | b[sos + 3]) - 2
    assert info["entropy_offset"] + info["entropy_length"] == len(b) - 2 and b[-2:] == b"\xff\xd9"   # up to EOI
    dri = b.find(b"\xff\xdd")
    assert info["restart_interval"] == (0 if dri < 0 else b[dri + 4] << 8 | b[dri + 5])
    assert ("dri" in name) == (info["restart_interval"] > 0)


def test_parser_on_the_encoder_streams():
    """the 36 streams of tests/golden/jpeg_encode: our own encoder's output form (4:2:0, no DRI, Annex-K tables, one with a comment)"""
    streams = enc.fixtures()
    assert len(streams) == 36
    for name, f in streams.items():
        info = fx.probe(f["jpeg"])
        h, w = f["rgb"].shape[:2]
        assert (info["reason"], info["w"], info["h"], info["components"], info["hsamp"], info["vsamp"], info["restart_interval"]) == \
               (fx.OK, w, h, 3, 2, 2, 0), name
        assert info["entropy_offset"] == enc.HEADER_BYTES + (len(f["comment"]) + 4 if f["comment"] else 0), name
        assert info["entropy_offset"] + info["entropy_length"] == len(f["jpeg"]) - 2, name


def test_parser_reason_codes():
    prog = FIX["smooth_17x33_progressive"]["jpeg"]
    assert fx.probe(prog)["reason"] == fx.PROGRESSIVE
    s422 = DEC["noise_24x40_422_q10"]["jpeg"]
    assert fx.probe(fx.sampling_440_of(s422))["reason"] == fx.SAMPLING_REASON
    good = DEC["noise_50x70_422_q90"]["jpeg"]
    off = fx.probe(good)["entropy_offset"]
    for cut in (0, 1, 2, 3, 4, 20, 160, 300, off - 1):          # every header cut is a reason code, never a crash
        assert fx.probe(good[:cut])["reason"] in (fx.TRUNCATED, fx.HEADER), cut
    assert fx.probe(good[:off])["reason"] == fx.OK and fx.probe(good[:off])["entropy_length"] == 0
    assert fx.probe(np.zeros(64, np.uint8))["reason"] == fx.TRUNCATED            # not a JPEG
    # the wrong size: the shared check every caller applies to the descriptor (size first, then the segment's cap)
    assert fx.probe(good, expect=(50, 70))["reason"] == fx.OK
    assert fx.probe(good, expect=(256, 192))["reason"] == fx.SIZE and fx.probe(good, expect=(70, 50))["reason"] == fx.SIZE
    assert fx.probe(good, expect=(50, 70), cap=fx.probe(good)["entropy_length"] - 1)["reason"] == fx.TOO_LONG
    assert fx.probe(prog, expect=(17, 33))["reason"] == fx.PROGRESSIVE          # an earlier reason stays
    b = bytearray(good.tobytes())
    sof = bytes(b).index(b"\xff\xc0")
    b[sof + 4] = 12                                              # 12-bit samples
    assert fx.probe(np.frombuffer(bytes(b), np.uint8))["reason"] == fx.PRECISION
    b[sof + 4], b[sof + 1] = 8, 0xC9                             # arithmetic coding
    assert fx.probe(np.frombuffer(bytes(b), np.uint8))["reason"] == fx.CODING
    b[sof + 1], b[sof + 9] = 0xC0, 4                             # four components
    assert fx.probe(np.frombuffer(bytes(b), np.uint8))["reason"] == fx.COMPONENTS


@pytest.mark.parametrize("name", sorted(DEC))
def test_host_walk_and_pixel_stage_equal_pil(name):
    f = DEC[name]
    reason, status, rgb, groups = fx.staged(f["jpeg"], f["rgb"].shape)
    assert (reason, status) == (0, 0)
    assert groups == f["stats"]["groups"]
    assert np.array_equal(rgb, f["rgb"]), np.argwhere(rgb != f["rgb"])[:4]


def test_chain_walk_guard(tmp_path):
    """tools/jpeg_entropy_guard.cpp on every fixture and on seeded corruptions of them, and on the three corrupt streams of the device tests"""
    exe = tmp_path / "jpeg_entropy_guard"
    inc = [os.path.join(fx.ROOT, *p) for p in (("rebvo_amd", "host", "include"), ("include",), ("rebvo_amd", "csrc"))]
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall"] + ["-I" + i for i in inc] +
                   [os.path.join(fx.ROOT, "tools", "jpeg_entropy_guard.cpp"), os.path.join(fx.ROOT, "rebvo_amd", "host", "src", "jpeg_reader.cpp"),
                    "-o", str(exe)], check=True)
    files = []
    for name, f in sorted(DEC.items()):
        files.append(str(tmp_path / (name + ".jpg")))
        f["jpeg"].tofile(files[-1])
    bad = []
    for tag, s in zip(("truncated", "flipped", "slot"), fx.corrupt_pair() + (fx.corrupt_slot_stream(),)):
        bad.append(str(tmp_path / (tag + ".jpg")))
        s.tofile(bad[-1])
    # four processes side by side, the large files dealt round (each file's corruptions are seeded by its place in its own process)
    by_size = sorted(files, key=os.path.getsize, reverse=True)
    procs = [subprocess.Popen([str(exe)] + by_size[k::4] + (["--corrupt"] + bad if k == 0 else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True) for k in range(4)]
    out = {}
    for p in procs:
        stdout, stderr = p.communicate()
        print(stdout, stderr[-2000:])
        assert p.returncode == 0, stderr[-2000:]
        for k, v in json.loads(stdout.strip().splitlines()[-1]).items():
            out[k] = out.get(k, 0) + v
    assert out["failures"] == 0 and out["files"] == len(files) + 3
    assert out["runs"] > 3000 and out["nonzero_status"] > 1000 and out["host_reader_errors"] > 50 and out["behind_last_read"] > 10, out
