"""CPU-only: the receiving side of the compressed edge map on the host — the local decode rule, update_pos, hide_visible and
fill_depth_map of rebvo/edgemap_com.h (through tools/edgemap_decode_host_check.cpp) and the numpy port tests/edgemap_decode_port.py —
against the fixtures tools/make_edgemap_decode_golden.py wrote from the compiled reference, bit for bit."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from rebvo_amd import edgehip
from tests import edgemap_crafted
from tests import edgemap_decode_crafted as crafted
from tests import edgemap_decode_port as port

ROOT = crafted.ROOT


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return crafted.build_host_tool(tmp_path_factory.mktemp("emdec"))


def _fixture_cases():
    out = []
    for which in crafted.SETS:
        meta, cases = crafted.load(which)
        for tag, c in cases.items():
            geo = c["geometry"] if "geometry" in c else meta["geometry"]
            out.append((which, tag, meta, c, [int(v) for v in geo]))
    return out


FIXTURES = _fixture_cases()


def _records(c):
    return np.frombuffer(np.ascontiguousarray(c["records"]).tobytes(), edgehip.COMPRESSED_KL_DTYPE)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the local rule against the cursor walk --------------------------------------------------------------------------------------------
ENUM_SRC = r"""
#include <cstdio>
#include <vector>
#include "rebvo/edgemap_com.h"
using namespace rebvo::edgemap;
int main() {
    long lists = 0, bad = 0;
    for (int n = 0; n <= 10; n++) {
        long total = 1;
        for (int i = 0; i < n; i++) total *= 3;
        for (long code = 0; code < total; code++) {
            std::vector<compressed_kl> k((size_t)n + 1);
            long c = code;
            for (int i = 0; i < n; i++, c /= 3) { k[i].x = (uint8_t)(3 * i + 1); k[i].y = (uint8_t)(5 * i + 2); k[i].rho = (int16_t)((c % 3 - 1) * (100 + i)); k[i].s_rho = (uint8_t)(i % 4); }
            // the walk: which record is k0 and which is k1 of every pair, from the cursor
            std::vector<int> w0, w1;
            int inx = 0;
            uncompressed_kl a, b;
            for (;;) {
                int at = inx;
                for (; at < n - 1 && k[at].rho == 0; at++) {}
                if (!get_pair(k.data(), n, 1.f, &inx, &a, &b)) break;
                w0.push_back(at);
                w1.push_back((k[at + 1].rho == 0 || k[at].rho < 0) ? at : at + 1);
            }
            std::vector<int> l0, l1;
            for (int i = 0; i < n; i++)
                if (seg_starts(i >= 1 ? k[i - 1].rho : 0, k[i].rho, i, n)) { l0.push_back(i); l1.push_back(seg_partner_is_self(k[i].rho, k[i + 1].rho) ? i : i + 1); }
            std::vector<uncompressed_segment> s_walk, s_local;
            decode(k.data(), n, 1.f, &s_walk, 1 << 30);
            decode_local(k.data(), n, 1.f, &s_local, 1 << 30);
            bool same = w0 == l0 && w1 == l1 && s_walk.size() == s_local.size() && s_walk.size() == w0.size();
            for (size_t j = 0; same && j < s_walk.size(); j++)
                same = !memcmp(&s_walk[j].k0, &s_local[j].k0, 16) && !memcmp(&s_walk[j].k1, &s_local[j].k1, 16);
            lists++;
            if (!same) bad++;
        }
    }
    printf("%ld %ld\n", lists, bad);
    return 0;
}
"""


def test_local_rule_equals_cursor_walk_on_every_sign_pattern(tmp_path):
    """Every list of up to 10 records with rho in {-, 0, +}: 88 573 lists.  The records that start a segment, their partners and the
    segments themselves are those of get_pair's walk."""
    src = tmp_path / "enum.cpp"
    src.write_text(ENUM_SRC)
    exe = tmp_path / "enum"
    inc = [os.path.join(ROOT, *q) for q in (("rebvo_amd", "host", "include"), ("include",), ("rebvo_amd", "csrc"))]
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off"] + ["-I" + i for i in inc] + [str(src), "-o", str(exe)], check=True)
    lists, bad = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert lists == sum(3 ** n for n in range(11)) == 88573
    assert bad == 0


def test_port_walk_equals_local_rule_on_sign_patterns():
    """The numpy port's cursor walk against the rule, on every pattern up to length 6."""
    for n in range(7):
        for signs in itertools.product((-1, 0, 1), repeat=n):
            rec = np.zeros(n, edgehip.COMPRESSED_KL_DTYPE)
            rec["rho"] = [s * (100 + i) for i, s in enumerate(signs)]
            rec["x"], rec["y"], rec["s_rho"] = np.arange(n) + 1, 2 * np.arange(n) + 1, np.arange(n) % 3
            segs, _ = port.decode(rec, 1.0)
            rho = rec["rho"].astype(int)
            starts = [i for i in range(n - 1) if rho[i] != 0 and not (rho[i] < 0 and i >= 1 and rho[i - 1] > 0)]
            assert len(segs) == len(starts), signs
            assert [int(round(float(x) * 0.5)) for x in segs[:, 0]] == [int(rec["x"][i]) for i in starts], signs


# ---- host and port against every fixture -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,tag,meta,c,geo", FIXTURES, ids=[f"{f[0]}-{f[1]}" for f in FIXTURES])
def test_host_and_port_equal_the_reference(tool, which, tag, meta, c, geo):
    w, h, bw, bh, iters, mode = geo
    rec = _records(c)
    rho_scale, v_thresh, a_thresh = (float(v) for v in c["params"])
    cam = tuple(float(v) for v in meta["camera"])
    views = list(meta["views"])
    host = crafted.host_run(tool, rec, rho_scale, v_thresh, a_thresh, size=(w, h), block=(bw, bh), cam=cam, em_nav=meta["em_nav"], views=views,
                            iter_num=iters, bound_mode=mode)
    assert _same_bits(host["segments"], c["segments"])
    p_segs, p_flags = port.decode(rec, rho_scale)
    assert _same_bits(p_segs, c["segments"])
    pcam = (cam[0], cam[1], cam[4], w, h)
    for v, view in enumerate(views):
        assert _same_bits(host["dpose"][v], c["dpose"][v]) and _same_bits(host["dpos"][v], c["dpos"][v])
        assert _same_bits(host["flags"][v], c["flags"][v]) and host["s_num"][v] == int(c["s_num"][v])
        DPose, DPos, _ = port.update_pos(meta["em_nav"], view)
        assert _same_bits(DPose, c["dpose"][v]) and _same_bits(DPos, c["dpos"][v])
        s_num = port.hide_visible(p_segs, p_flags, DPose, DPos, meta["em_nav"][12], view[12], pcam)
        assert _same_bits(p_flags, c["flags"][v]) and s_num == int(c["s_num"][v])
    for name, a, b in zip(("rho", "s_rho", "fixed"), host["fill"], (c["fill_rho"], c["fill_s_rho"], c["fill_fixed"])):
        assert _same_bits(a, b), name
    rho, s_rho, fixed, gates = port.fill_depth_map(c["segments"], None, w, h, bw, bh, pcam, v_thresh, a_thresh)
    assert _same_bits(rho, c["fill_rho"]) and _same_bits(s_rho, c["fill_s_rho"]) and _same_bits(fixed.astype(np.uint8), c["fill_fixed"])
    assert np.array_equal(gates, host["gates"])
    ch = port.chain(rho, s_rho, fixed, w, h, bw, bh, iters, mode)
    assert _same_bits(ch[0].reshape(-1), c["chain_rho"]) and _same_bits(ch[1].reshape(-1), c["chain_s_rho"])
    assert _same_bits(ch[2].reshape(-1).astype(np.uint8), c["chain_fixed"])
    for k in ("fill_rho", "fill_s_rho", "chain_rho", "chain_s_rho"):
        assert np.isfinite(c[k]).all(), k          # no input creates a NaN: no cell is exempt


def test_every_branch_of_the_crafted_lists_is_populated(tool):
    meta, cases = crafted.load("crafted")
    assert sorted(cases) == sorted(crafted.names())
    gates, hit = {}, {}
    for name in crafted.names():
        c = crafted.case(name)
        assert _same_bits(np.frombuffer(c["records"].tobytes(), np.uint8).reshape(-1, 5), cases[name]["records"]), name
        assert [c["rho_scale"], c["v_thresh"], c["a_thresh"]] == [float(v) for v in cases[name]["params"]], name
        r = crafted.host_run(tool, c["records"], c["rho_scale"], c["v_thresh"], c["a_thresh"])
        gates[name], hit[name] = r["gates"], r
    G = port.GATE_NAMES.index
    assert gates["gate_sigma_k0"].tolist() == [G("sigma")] and gates["gate_sigma_k1"].tolist() == [G("sigma")]
    assert gates["gate_sum"].tolist() == [G("sum")]
    assert gates["gate_rel_k0"].tolist() == [G("rel")] and gates["gate_rel_k1"].tolist() == [G("rel")]
    assert gates["gate_rel_on_threshold"].tolist() == [G("folded")]
    assert gates["gate_angle"].tolist() == [G("angle"), G("folded")]
    assert gates["shared_vertex"].tolist() == [0, 0] and np.array_equal(hit["shared_vertex"]["segments"][0, 4:8], hit["shared_vertex"]["segments"][1, 0:4])
    assert len(hit["open_polyline"]["segments"]) == 1                      # the last record as partner only
    # a closing negative rho as k1: its magnitude is k1.rho, and the cursor passes over it — the record behind it starts the next segment
    hz, zb = hit["horizontal_nt_integer"]["segments"], hit["zeros_between"]["segments"]
    assert len(hz) == 1 and hz[0, 6] > 0 and hz[0, 6] == port.decode(crafted.case("horizontal_nt_integer")["records"], 1.0)[0][0, 6]
    assert hz[0, 6] == np.float32(np.float32(crafted.ONE + 300) / np.float32(np.float32(32767.0 / 20) / np.float32(1.0)))
    assert (zb[0, 4], zb[0, 5]) == (20.0, 8.0) and (zb[1, 0], zb[1, 1]) == (40.0, 30.0)   # the closing record is k1 once and never a k0
    nk = hit["negative_k0"]["segments"]
    assert (nk[0, 4], nk[0, 5]) == (20.0, 4.0) and (nk[1, 0], nk[1, 1]) == (40.0, 20.0) and np.array_equal(nk[1, 0:4], nk[1, 4:8])
    assert gates["negative_k0"].tolist() == [0, G("degenerate"), 0]      # a negative k0 pairs with itself
    assert len(hit["zeros_between"]["segments"]) == 2
    assert gates["degenerate_before_zero"].tolist() == [G("degenerate"), 0]
    assert gates["leading_negative"].tolist() == [G("degenerate"), 0]
    assert (hit["s_rho_byte_0"]["segments"][0, [3, 7]] == np.float32(1e-3)).all() and gates["s_rho_byte_0"].tolist() == [0]
    assert hit["horizontal_nt_integer"]["steps"] == 32                      # nt = 32 exactly: steps 0 .. 31
    assert hit["diagonal"]["steps"] == int(np.ceil(np.hypot(28, 28)))
    fixed = hit["clamp_right_bottom"]["fill"][2].reshape(crafted.H // crafted.BH, crafted.W // crafted.BW)
    assert fixed[-1, -1] and fixed.sum() == 1                              # steps past the image land in the last cell
    assert hit["clamp_right_edge"]["fill"][2].reshape(6, 8)[:, -1].all()
    # two segments through the same cells in both list orders: the fold is order dependent
    ab, ba = hit["cross_ab"]["fill"], hit["cross_ba"]["fill"]
    assert np.array_equal(ab[2], ba[2]) and not _same_bits(ab[0], ba[0])
    # steps exactly on a cell boundary belong to the cell that begins there
    fx = hit["on_cell_boundary"]["fill"][2].reshape(6, 8)
    assert fx[2, 2:5].all() and not fx[1, 2].any()                         # y = 16 is row 2, from x = 16 (column 2) on
    assert fx[1:4, 3].all() and not fx[1:4, 2].sum() > 1                   # x = 24 is column 3
    # the views: hidden, kept, already hidden, and a view from beyond the points (rho < 0 keeps)
    total = {k: 0 for k in ("hidden", "kept", "sticky")}
    for name in crafted.names():
        prev = np.ones(len(hit[name]["segments"]), np.uint8)
        for f in hit[name]["flags"]:
            total["hidden"] += int(((prev == 1) & (f == 0)).sum())
            total["kept"] += int(((prev == 1) & (f == 1)).sum())
            total["sticky"] += int((prev == 0).sum())
            assert not ((prev == 0) & (f == 1)).any()
            prev = f
    assert min(total.values()) > 0, total


def test_use_visibility_skips_hidden_segments(tool):
    """This library's extension, against the port only."""
    c = crafted.case("mixed")
    r = crafted.host_run(tool, c["records"], c["rho_scale"], c["v_thresh"], c["a_thresh"], use_visibility=True, views=crafted.VIEWS[1:2])
    segs, flags = port.decode(c["records"], c["rho_scale"])
    pcam = (crafted.CAM[0], crafted.CAM[1], crafted.CAM[4], crafted.W, crafted.H)
    for view in crafted.VIEWS[1:2]:     # one view: it hides some of the folded segments and keeps others
        DPose, DPos, _ = port.update_pos(crafted.EM_NAV, view)
        port.hide_visible(segs, flags, DPose, DPos, crafted.EM_NAV[12], view[12], pcam)
    assert 0 < flags.sum() < len(flags)
    rho, s_rho, fixed, gates = port.fill_depth_map(segs, flags, crafted.W, crafted.H, crafted.BW, crafted.BH, pcam, c["v_thresh"], c["a_thresh"], True)
    assert _same_bits(rho, r["fill"][0]) and _same_bits(s_rho, r["fill"][1]) and _same_bits(fixed.astype(np.uint8), r["fill"][2])
    assert np.array_equal(gates, r["gates"]) and (gates[flags == 0] == -1).all() and fixed.any()


def test_billboard_frames_through_compress_decode_fill(tool, tmp_path):
    """Three tracked frames of the 256x192 billboard: rebvo_compress_edgemap's records are the fixture's, and the chain behind their fill
    fixes more than 50 cells."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "edgemap", "billboard.npz"))
    meta, cases = crafted.load("billboard")
    exe = edgemap_crafted.build_host_tool(tmp_path)
    cam = tuple(float(v) for v in g["camera"])
    fixed_cells = 0
    for k in (int(v) for v in meta["frames"]):
        tag = f"frame{k}"
        kl = np.zeros(len(g[f"{tag}__rho"]), edgehip.KEYLINE_DTYPE)
        for f in ("c_p", "u_m", "rho", "s_rho", "m_num", "p_id", "n_id"):
            kl[f] = g[f"{tag}__{f}"]
        pr = g[f"{tag}__params"]
        p = dict(min_line_len=int(pr[0]), max_line_len=int(pr[1]), max_angle=float(pr[2]), match_n_t=int(pr[3]), rho_rel_max=float(pr[4]), scale=float(pr[5]))
        host = edgemap_crafted.host_run(exe, kl, p, 2 * len(kl) + 2, cam)
        assert _same_bits(host["records"], cases[tag]["records"])
        w, h, bw, bh, iters, mode = (int(v) for v in cases[tag]["geometry"])
        rho_scale, v_thresh, a_thresh = (float(v) for v in cases[tag]["params"])
        assert rho_scale == float(np.float32(p["scale"]))
        rec = np.frombuffer(host["records"].tobytes(), edgehip.COMPRESSED_KL_DTYPE)
        r = crafted.host_run(tool, rec, rho_scale, v_thresh, a_thresh, size=(w, h), block=(bw, bh), cam=cam, iter_num=iters, bound_mode=mode)
        assert _same_bits(r["fill"][0], cases[tag]["fill_rho"])
        n_fixed = int(cases[tag]["chain_fixed"].sum())
        assert n_fixed == int(r["fill"][2].sum()) and n_fixed > 50
        fixed_cells += n_fixed
    assert fixed_cells > 150


def test_guard_program_runs_clean(tmp_path):
    """tools/edgemap_decode_guard.cpp: the host binning and scatter of the (segment, step) items on random record lists, every index
    checked, under AddressSanitizer and UBSan."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is required")
    exe = tmp_path / "guard"
    inc = [os.path.join(ROOT, *q) for q in (("rebvo_amd", "host", "include"), ("include",), ("rebvo_amd", "csrc"))]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                   ["-I" + i for i in inc] + [os.path.join(ROOT, "tools", "edgemap_decode_guard.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "300"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
