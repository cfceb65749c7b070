"""CPU-only: the compressed edge map on the host (rebvo_amd/host/include/rebvo/edgemap_com.h on csrc/edgemap_fit.h) against the compiled
reference's records, packets and decoded segments (tests/golden/edgemap/, written by tools/make_edgemap_golden.py), the receiving side's
acceptance rules, the error returns, and the walk guard (tools/edgemap_walk_guard.cpp) under the address and undefined-behaviour
sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from rebvo_amd import edgehip
from tests import edgemap_crafted as crafted

GOLD = os.path.join(crafted.ROOT, "tests", "golden", "edgemap")
FIELDS = ("c_p", "u_m", "rho", "s_rho", "m_num", "p_id", "n_id")
PKEYS = ("min_line_len", "max_line_len", "max_angle", "match_n_t", "rho_rel_max", "scale")


def fixture_case(g, tag):
    """-> (KeyLine list from the fields the fixture keeps, parameters)"""
    n = len(g[f"{tag}__rho"])
    kl = np.zeros(n, edgehip.KEYLINE_DTYPE)
    for f in FIELDS:
        kl[f] = g[f"{tag}__{f}"]
    v = g[f"{tag}__params"]
    p = dict(zip(PKEYS, v.tolist()))
    for k in ("min_line_len", "max_line_len", "match_n_t"):
        p[k] = int(p[k])
    return kl, p


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return crafted.build_host_tool(tmp_path_factory.mktemp("edgemap"))


@pytest.fixture(scope="module")
def gold():
    return {k: np.load(os.path.join(GOLD, k + ".npz")) for k in ("crafted", "billboard")}


def _check(tool, g, tag, cam):
    kl, p = fixture_case(g, tag)
    r = crafted.host_run(tool, kl, p, 2 * len(kl) + 2, cam)
    want = g[f"{tag}__records"]
    assert r["status"] == 0
    assert r["count"] == len(want), (tag, r["count"], len(want))
    assert np.array_equal(r["records"], want.reshape(-1, 5)), tag
    assert np.array_equal(r["packet"], g[f"{tag}__packet"]), tag          # header with both CRCs, then the records
    assert r["segments"].tobytes() == g[f"{tag}__segments"].tobytes(), tag
    assert np.array_equal(r["trace"][:, 2:5], g[f"{tag}__dirs"]), tag      # tx, ty, zfo of every fit, as float bit patterns


def test_crafted_lists_are_the_fixtures_inputs(gold):
    g = gold["crafted"]
    assert list(g["names"]) == crafted.names()
    assert tuple(g["camera"]) == crafted.camera()
    for name in crafted.names():
        kl, p = crafted.case(name)
        fk, fp = fixture_case(g, name)
        for f in FIELDS:
            assert np.array_equal(kl[f], fk[f]), (name, f)
        assert fp == {k: p[k] for k in PKEYS}, name


@pytest.mark.parametrize("name", crafted.names())
def test_host_restatement_equals_reference_on_crafted(tool, gold, name):
    _check(tool, gold["crafted"], name, tuple(gold["crafted"]["camera"]))


def test_host_restatement_equals_reference_on_billboard_frames(tool, gold):
    g = gold["billboard"]
    assert len(g["frames"]) >= 3
    for k in g["frames"]:
        _check(tool, g, f"frame{int(k)}", tuple(g["camera"]))


def _recv(tool, keyline_max, packets):
    payload = np.array([keyline_max, len(packets)], np.int32).tobytes()
    for brecv, pkt in packets:
        payload += np.array([brecv, len(pkt)], np.int32).tobytes() + np.asarray(pkt, np.uint8).tobytes()
    out = subprocess.run([tool, "recv"], input=payload, check=True, capture_output=True).stdout
    flags = np.frombuffer(out, np.int32, 2 * len(packets)).reshape(-1, 2)
    at = 8 * len(packets)
    kl_num, em_id = (int(v) for v in np.frombuffer(out, np.int32, 2, at))
    rho_scale = float(np.frombuffer(out, np.float32, 1, at + 8)[0])
    recs = np.frombuffer(out, np.uint8, 5 * kl_num, at + 12).reshape(kl_num, 5)
    return flags, kl_num, em_id, rho_scale, recs


def test_check_recv_pak_rules(tool, gold):
    g = gold["crafted"]
    pkt = g["mixed__packet"].copy()
    want = g["mixed__records"].reshape(-1, 5)
    sent = (len(pkt) - 92) // 5
    assert 0 < sent < len(want)                      # a partial packet: kl_num < kl_total
    # a good packet: accepted, a new edge map begins, its records land at kl_id
    flags, kl_num, em_id, rho_scale, recs = _recv(tool, 1000, [(len(pkt), pkt)])
    assert flags.tolist() == [[1, 1]] and kl_num == len(want) and em_id == 1 and rho_scale == 1.0
    assert np.array_equal(recs[:sent], want[:sent]) and not recs[sent:].any()
    # a flipped byte in the header: the header CRC rejects the packet
    bad = pkt.copy()
    bad[20] ^= 0x40
    flags, kl_num, em_id, _, _ = _recv(tool, 1000, [(len(bad), bad)])
    assert flags.tolist() == [[0, 0]] and kl_num == 0 and em_id == 0
    # a flipped byte in the data: the packet is accepted, its records are left out
    bad = pkt.copy()
    bad[92 + 7] ^= 0x01
    flags, kl_num, em_id, _, recs = _recv(tool, 1000, [(len(bad), bad)])
    assert flags.tolist() == [[1, 1]] and kl_num == len(want) and em_id == 1 and not recs.any()
    # the wrong size, and a kl_total beyond the receiver's KEYLINE_MAX
    flags, kl_num, _, _, _ = _recv(tool, 1000, [(len(pkt) - 5, pkt)])
    assert flags.tolist() == [[0, 0]] and kl_num == 0
    flags, kl_num, _, _, _ = _recv(tool, len(want) - 1, [(len(pkt), pkt)])
    assert flags.tolist() == [[0, 0]] and kl_num == 0
    # the same edge map again is accepted without beginning a new one
    flags, _, em_id, _, recs = _recv(tool, 1000, [(len(pkt), pkt), (len(pkt), pkt)])
    assert flags.tolist() == [[1, 1], [1, 0]] and em_id == 1 and np.array_equal(recs[:sent], want[:sent])


def test_crc16_is_the_reflected_a001_polynomial(gold):
    """the fixture's packets carry the reference's CRCs: recompute both here, bit by bit"""
    def crc(b):
        c = 0xFFFF
        for x in bytes(b):
            c ^= x
            for _ in range(8):
                c = (c >> 1) ^ 0xA001 if c & 1 else c >> 1
        return c
    pkt = gold["crafted"]["mixed__packet"]
    assert int(pkt[88:90].copy().view("<u2")[0]) == crc(pkt[92:])
    assert int(pkt[90:92].copy().view("<u2")[0]) == crc(pkt[:90])


def test_error_returns(tool):
    kl, p = crafted.case("mixed")
    full = crafted.host_run(tool, kl, p, 2 * len(kl))
    assert full["count"] > 1 and full["status"] == 0
    # a span one record too small: count 0 and the overflow status (the reference's `return kl_num=0`)
    small = crafted.host_run(tool, kl, p, full["count"] - 1)
    assert small["count"] == 0 and small["status"] == edgehip.EDGEMAP_OVERFLOW
    # links out of range read as -1 and set the status bit
    bad = kl.copy()
    bad["n_id"][3], bad["p_id"][20] = len(kl) + 4, -7
    r = crafted.host_run(tool, bad, p, 2 * len(kl))
    assert r["status"] == edgehip.EDGEMAP_BAD_LINK
    # parameters the rule does not cover, and a packet that does not fit the 16-bit paket_size
    for over, code in ((dict(min_line_len=-1), 5), (dict(max_line_len=0), 5)):
        q = dict(p)
        q.update(over)
        with pytest.raises(subprocess.CalledProcessError) as e:
            crafted.host_run(tool, kl, q, 2 * len(kl))
        assert e.value.returncode == code
    assert crafted.host_run(tool, kl, p, 2 * len(kl), max_kl_num=(65535 - 92) // 5)["sent"] == full["count"]
    with pytest.raises(subprocess.CalledProcessError) as e:
        crafted.host_run(tool, kl, p, 2 * len(kl), max_kl_num=(65535 - 92) // 5 + 1)
    assert e.value.returncode == 6


def test_config_parser_reads_the_compressed_edge_map_keys(tmp_path):
    """&EdgeMapOutput CompressedEdgeMap, MinLineLen, MaxLineLen, MaxAngle, MatchNumThresh, RhoRelMax; absent keys keep their defaults
    (off; 3, 50, 0.3 and the reference's default arguments match_n_t = 0, rho_rel_max = 1e10)."""
    import ctypes as C
    from tests.helpers import write_global_config
    host = C.CDLL(os.path.join(crafted.ROOT, "rebvo_amd", "lib", "librebvohost.so"))

    def parsed(section):
        cfg = tmp_path / "cfg"
        write_global_config(cfg, edgehip.euroc_params(376, 240))
        with open(cfg, "a") as f:
            f.write(section)
        ints, reals = (C.c_int * 4)(-1, -1, -1, -1), (C.c_double * 2)(-1, -1)
        assert host.rebvo_compressed_edgemap_config(str(cfg).encode(), ints, reals) == 0
        return list(ints), list(reals)
    assert parsed("") == ([0, 3, 50, 0], [0.3, 1e10])
    assert parsed("\n&EdgeMapOutput\nCompressedEdgeMap=1\n") == ([1, 3, 50, 0], [0.3, 1e10])
    assert parsed("\n&EdgeMapOutput\nCompressedEdgeMap=1\nMinLineLen=5\nMaxLineLen=33\nMaxAngle=0.25\nMatchNumThresh=2\nRhoRelMax=1.5\n") == \
        ([1, 5, 33, 2], [0.25, 1.5])


def test_walk_guard_under_sanitizers(tmp_path):
    """tools/edgemap_walk_guard.cpp: the component-wise execution in a shuffled order against the serial loop on random link graphs, with
    checked indices, canary bands and the step bound, built with -fsanitize=address,undefined"""
    exe = tmp_path / "edgemap_walk_guard"
    inc = [os.path.join(crafted.ROOT, *q) for q in (("rebvo_amd", "host", "include"), ("include",), ("rebvo_amd", "csrc"))]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                   ["-I" + i for i in inc] + [os.path.join(crafted.ROOT, "tools", "edgemap_walk_guard.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "graphs ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
