"""Depth along the key-frame links without a GPU: the plain-numpy port (tests/keyframe_depth_port.py) against the reference's recorded
outputs (tests/golden/keyframe_depth/, written by tools/make_keyframe_depth_golden.py from kfvo::mapKFUsingIDK, translateDepth_F2KF,
translateDepth_KF2F and translateDepth_New2Old) bit for bit, the branch populations the crafted fixture was built to have, the rule that
translateDepth_New2Old reads every successor as it was before the iteration, and the size of the C ABI's struct.

Everything compared is IEEE +, -, *, / and sqrt in fp64 in a fixed order (no libm function whose last place may differ between
machines), so the port is held to the same bits here as on the machine that wrote the fixtures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import keyframe_depth_port as port

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_depth")
REQUIRED = ("branch_min", "branch_max", "branch_nonfinite", "branch_negative", "branch_none", "min_with_nan_s_rho", "rotate_zeros", "scale_behind",
            "scale_fallback_pairs")
_FX = {}


def fixture(name):
    if name not in _FX:
        _FX[name] = port.load_fixture(os.path.join(GOLD, name + ".npz"))
    return _FX[name]


def run(case, pair, trace=None):
    if case["call"] == "map":
        rho, s_rho, count, guard = port.map_depth(pair, *case["args"], trace=trace)
        return dict(rho=rho, s_rho=s_rho, m_num=np.asarray(pair["kf"]["m_num"]), count=count, guard=guard, K=0.0, rTr=0.0, rTr0=0.0)
    return port.translate(pair, case["direction"], bool(case["optim"]), trace)


@pytest.mark.parametrize("name", ["crafted", "chained"])
def test_port_equals_the_reference(name):
    f = fixture(name)
    assert len(f["cases"]) == 5 * sum(p["kind"] != "link_out_of_range" for p in f["pairs"])
    arrays = 0
    for c, case in enumerate(f["cases"]):
        ref = case["ref"]
        got = run(case, f["pairs"][case["pair"]])
        assert (got["count"], got["guard"]) == (ref["count"], 0), c
        assert port.same_bits([got["K"], got["rTr"], got["rTr0"]], [ref["K"], ref["rTr"], ref["rTr0"]]), (c, got["K"], ref["K"])   # (NaN sums in the nan_rho pair)
        assert port.digest(got["rho"], got["s_rho"], got["m_num"]) == ref["digest"], c
        if "rho" in ref:
            arrays += 1
            assert port.same_bits(got["rho"], ref["rho"]) and port.same_bits(got["s_rho"], ref["s_rho"]) and np.array_equal(got["m_num"], ref["m_num"]), c
            assert port.digest(ref["rho"], ref["s_rho"], ref["m_num"]) == ref["digest"], c
    assert arrays == (len(f["cases"]) if name == "crafted" else 2)
    for c, case in enumerate(f["list_cases"]):
        chain, ref = f["lists"][case["list"]], case["ref"]
        got, count, guard = port.list_translate(chain, case["iters"], float(f["cam"]["zfm"]))
        assert (count, guard) == (ref["count"], 0), c
        for i, k in enumerate(got):
            assert port.digest(k["kl"]["rho"], k["kl"]["s_rho"], k["kl"]["m_num"]) == ref["digests"][i], (c, i)
            if "rho" in ref:
                assert port.same_bits(k["kl"]["rho"], ref["rho"][i]) and port.same_bits(k["kl"]["s_rho"], ref["s_rho"][i]), (c, i)
                assert np.array_equal(k["kl"]["m_num"], ref["m_num"][i]), (c, i)
        if chain:   # the newest position is only read
            assert port.same_bits(got[-1]["kl"]["rho"], chain[-1]["kl"]["rho"]) and np.array_equal(got[-1]["kl"]["m_num"], chain[-1]["kl"]["m_num"])


def test_crafted_shapes_cases_and_populations():
    f = fixture("crafted")
    z = f["z"]
    assert (int(f["cam"]["w"]), int(f["cam"]["h"])) == (70, 50)
    assert [len(p["kf"]["rho"]) for p in f["pairs"]] == [0, 1, 5, 65, 257, 600, 1030, 65, 65, 65, 65, 65]
    assert [p["kind"] for p in f["pairs"]] == ["no_links", "few_links", "few_links"] + ["compared"] * 4 + ["nan_rho", "half_turn", "quarter_turn", "all_behind",
                                                                                                         "link_out_of_range"]
    assert [len(lst) for lst in f["lists"]] == [4, 2, 1] and [(c["list"], c["iters"]) for c in f["list_cases"]] == [(j, it) for j in range(3) for it in (1, 3)]
    # the populations, recomputed here from the port's trace (not read from the file), then set beside the file's
    st = {k: 0 for k in REQUIRED}
    for case in f["cases"]:
        pair, tr = f["pairs"][case["pair"]], {}
        run(case, pair, tr)
        if case["call"] == "map":
            for j, k in enumerate(port.BRANCHES):
                st["branch_" + k] += int((tr["branch"] == j).sum())
            st["min_with_nan_s_rho"] += tr["min_with_nan_s_rho"]
            st["rotate_zeros"] += tr["rotate_zeros"]
            if pair["kind"] == "compared":   # the comparison is of arithmetic, not of clamps
                assert (tr["branch"] == 4).mean() >= 0.5
                assert (tr["branch"] == 4).mean() == z["ref_none_share"][f["cases"].index(case)]
            # the classes on the REFERENCE's recorded outputs
            r, s, b = case["ref"]["rho"][tr["idx"]], case["ref"]["s_rho"][tr["idx"]], tr["branch"]
            assert (r[b == 0] == port.RHO_MIN).all() and (r[b == 1] == port.RHO_MAX).all()
            assert ((r[(b == 2) | (b == 3)] == port.RHO_INIT) & (s[(b == 2) | (b == 3)] == port.RHO_MAX)).all()
            assert int((np.isnan(s) & (r == port.RHO_MIN)).sum()) == tr["min_with_nan_s_rho"]
        elif case["optim"]:
            st["scale_behind"] += tr["scale_behind"]
            if tr["scale_links"] > 0 and tr["scale_behind"] == tr["scale_links"]:
                st["scale_fallback_pairs"] += 1
                assert case["ref"]["K"] == 1.0 and pair["kind"] == "all_behind"
    assert all(st[k] > 0 for k in REQUIRED), st
    assert st == dict(zip((str(k) for k in z["stat_names"]), (int(v) for v in z["stat_values"])))
    # where each population lives
    kind = {p["kind"]: j for j, p in enumerate(f["pairs"])}
    by = {(c["pair"], c["call"], c["args"]): c for c in f["cases"]}
    tr = {}
    run(by[(kind["quarter_turn"], "map", (0.0, 0.0, 1.0))], f["pairs"][kind["quarter_turn"]], tr)
    assert tr["rotate_zeros"] >= 3
    q = f["pairs"][kind["quarter_turn"]]
    R, _ = port.relative(q["Pose"], q["Pos"], q["kf_Pose"], q["kf_Pos"])
    assert np.array_equal(R, [[0, 0, 1], [0, 1, 0], [-1, 0, 0]])                 # exact zeros: qr[2] == 0 for p_m = (0, 0)
    tr = {}
    run(by[(kind["half_turn"], "map", (0.0, 0.0, 1.0))], f["pairs"][kind["half_turn"]], tr)
    assert (tr["branch"] == 3).any()
    tr = {}
    run(by[(kind["nan_rho"], "map", (0.0, 0.0, 1.0))], f["pairs"][kind["nan_rho"]], tr)
    assert (tr["branch"] == 2).sum() >= 1
    # about 20 % of the links dropped in either direction (the frame lists also have 7 KeyLines of their own)
    for j in range(3, 7):
        p = f["pairs"][j]
        assert 0.1 < (p["kf"]["m_id_f"] < 0).mean() < 0.3 and 0.1 < ((p["fr"]["m_id_kf"] < 0).sum() - 7) / len(p["kf"]["rho"]) < 0.3
    # the degenerate inputs
    oob = f["pairs"][kind["link_out_of_range"]]
    assert (oob["kf"]["m_id_f"] >= len(oob["fr"]["rho"])).sum() == 1 and (oob["fr"]["m_id_kf"] >= len(oob["kf"]["rho"])).sum() == 1
    assert port.map_depth(oob, 0.0, 0.0, 1.0)[3] == 4 and port.translate(oob, 0)["guard"] == 4 and port.translate(oob, 1)["guard"] == 4
    assert float(z["timing_ref_seconds_map"]) > 0 and float(z["timing_ref_seconds_list"]) > 0 and int(z["timing_kn"]) == 16000
    assert 0.75 < float(z["timing_linked_share"]) < 0.85


def test_chained_shapes():
    f = fixture("chained")
    assert (int(f["cam"]["w"]), int(f["cam"]["h"])) == (256, 192) and len(f["pairs"]) == 2 and [len(lst) for lst in f["lists"]] == [3]
    # one key frame (frame 0) against two frames; the list's entries are those three lists
    a, b = f["pairs"]
    assert a["kf"]["rho"].tobytes() == b["kf"]["rho"].tobytes() and not np.array_equal(a["kf"]["m_id_f"], b["kf"]["m_id_f"])
    lst = f["lists"][0]
    assert lst[0]["kl"]["rho"].tobytes() == a["kf"]["rho"].tobytes() and np.array_equal(lst[0]["kl"]["m_id_f"], a["kf"]["m_id_f"])
    assert lst[1]["kl"]["rho"].tobytes() == a["fr"]["rho"].tobytes() and lst[2]["kl"]["rho"].tobytes() == b["fr"]["rho"].tobytes()
    assert (lst[1]["kl"]["m_id_f"] >= 0).sum() > 1000 and (lst[1]["kl"]["m_id_f"] < len(lst[2]["kl"]["rho"])).all()
    assert all(c["ref"]["count"] > 5000 for c in f["cases"])
    assert os.path.getsize(os.path.join(GOLD, "chained.npz")) < 1000000 and os.path.getsize(os.path.join(GOLD, "crafted.npz")) < 1000000


def test_new2old_reads_before_it_updates():
    """Within one iteration the reference walks the positions upwards, so position i reads position i + 1 as it was BEFORE the iteration.
    Walking downwards (every successor updated first) gives other bits at every position but the last two, and the fixture shows it."""
    f = fixture("crafted")
    chain = f["lists"][0]
    case = [c for c in f["list_cases"] if c["list"] == 0 and c["iters"] == 1][0]
    zfm = float(f["cam"]["zfm"])
    up, _, _ = port.list_translate(chain, 1, zfm)
    down, _, _ = port.list_translate(chain, 1, zfm, successors_first=True)
    for i in (0, 1):
        assert port.same_bits(up[i]["kl"]["rho"], case["ref"]["rho"][i])
        assert not port.same_bits(down[i]["kl"]["rho"], case["ref"]["rho"][i]), i
    assert port.same_bits(down[2]["kl"]["rho"], case["ref"]["rho"][2])            # its successor is never written
    # iteration n + 1 reads iteration n's results: three iterations are three single ones
    thrice = chain
    for _ in range(3):
        thrice, _, _ = port.list_translate(thrice, 1, zfm)
    ref3 = [c for c in f["list_cases"] if c["list"] == 0 and c["iters"] == 3][0]["ref"]
    for i in range(4):
        assert port.same_bits(thrice[i]["kl"]["rho"], ref3["rho"][i]) and np.array_equal(thrice[i]["kl"]["m_num"], ref3["m_num"][i])
    # after n iterations position i carries the depth of position min(i + n, last): with 3 iterations position 0 differs from 1 iteration's
    assert not port.same_bits(ref3["rho"][0], case["ref"]["rho"][0])


def test_struct_size_and_header():
    from rebvo_amd import edgehip
    assert C.sizeof(edgehip.KfDepth) == 32 and edgehip.KF_DEPTH_DTYPE.itemsize == 32
    assert [(n, edgehip.KF_DEPTH_DTYPE.fields[n][1]) for n in edgehip.KF_DEPTH_DTYPE.names] == [("count", 0), ("guard", 4), ("K", 8), ("rTr", 16), ("rTr0", 24)]
    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "..", "include", "edgehip.h")).read()
    m = re.search(r"typedef struct edgehip_kf_depth \{(.*?)\} edgehip_kf_depth;", hdr, re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "int32_t count, guard; double K, rTr, rTr0;"
    for name in ("edgehip_keyframe_map_depth", "edgehip_keyframe_translate_depth", "edgehip_keyframe_list_translate_depth", "edgehip_keyframe_depth_ms"):
        assert name in edgehip.EXPORTS and re.search(r"\bint " + name + r"\(edgehip_ctx \*ctx", hdr), name
