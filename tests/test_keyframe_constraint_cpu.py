"""The key-frame relative-pose constraint without a GPU: the plain-numpy port (tests/keyframe_constraint_port.py) against the reference's
recorded outputs (tests/golden/keyframe_constraint/, written by tools/make_keyframe_constraint_golden.py from kfvo::OptimizeRelContraint
and kfvo::mutualExclusionSimple), the populations the crafted fixture was built to have, the sizes of the C ABI's structs, and the rule
that `residual` is ONE array for the whole call.

The port sums in the reference's order, so the fp64 outputs agree to libm's slack: 1e-12 relative here (the generator held 1e-13 on the
build machine; another libm may round sin / cos / asin differently in the last place)."""
import ctypes as C
import os

import numpy as np
import pytest

import keyframe_constraint_port as port

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_constraint")
REQUIRED = ("accepted_and_rejected_in_one_call", "reweighted", "unweighted", "unlinked_between", "scale_behind",
            "mutual_dropped_non_mutual", "mutual_failed_dist_kf", "mutual_passed_dist_kf", "mutual_failed_dist_fr", "mutual_passed_dist_fr")
_FX = {}


def fixture(name):
    if name not in _FX:
        _FX[name] = port.load_fixture(os.path.join(GOLD, name + ".npz"))
    return _FX[name]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


@pytest.mark.parametrize("name", ["crafted", "chained"])
def test_port_equals_the_reference(name):
    f = fixture(name)
    assert len(f["cases"]) >= 8
    for c, case in enumerate(f["cases"]):
        pair, cnt = port.pruned(f["pairs"][case["pair"]], case["dist_t"], case["discard"], case["prune"])
        ref = case["ref"]
        assert np.array_equal(pair["kf"]["m_id_f"], case["m_id_f"]) and np.array_equal(pair["fr"]["m_id_kf"], case["m_id_kf"]), c
        assert list(cnt) == list(ref["prune_counts"]), c
        got = port.constraint(pair, case["direction"], case["iter_max"], case["k_huber"])
        assert (got["links"], got["inliers"], got["guard"]) == (int(ref["links"]), int(ref["inliers"]), 0), c
        assert got["evals"] == case["iter_max"] + 2 and ref["links"] >= 30 and ref["ratio"] > 1e-6, c
        for k in ("X", "W_X", "R_X", "ratio", "E", "E0", "Kp", "W_Kp"):
            assert rel(got[k], ref[k]) <= 1e-12, (c, k, rel(got[k], ref[k]))
        assert (got["Kp"], got["W_Kp"]) == (0, 0) or case["direction"] == 1


def test_crafted_shapes_cases_and_populations():
    f = fixture("crafted")
    z = f["z"]
    assert (int(f["cam"]["w"]), int(f["cam"]["h"])) == (70, 50)
    assert [len(p["kf"]["rho"]) for p in f["pairs"]] == [0, 1, 5, 65, 257, 600, 1030, 65, 65]
    assert [p["kind"] for p in f["pairs"]] == ["no_links", "few_links", "few_links"] + ["compared"] * 4 + ["nan_rho", "link_out_of_range"]
    # the populations, recomputed here from the port's trace and pruning rule (not read from the file), then set beside the file's
    st = {}
    for case in f["cases"]:
        pair, _ = port.pruned(f["pairs"][case["pair"]], case["dist_t"], case["discard"], case["prune"])
        tr = {}
        port.constraint(pair, case["direction"], case["iter_max"], case["k_huber"], tr)
        if tr.get("accepted", 0) and tr.get("rejected", 0):
            st["accepted_and_rejected_in_one_call"] = st.get("accepted_and_rejected_in_one_call", 0) + 1
        for k in ("reweighted", "unweighted", "unlinked_between", "scale_behind", "accepted", "rejected"):
            st[k] = st.get(k, 0) + tr.get(k, 0)
    for p in f["pairs"][3:7]:
        for kf_to_frame, tag in ((True, "kf"), (False, "fr")):
            col0 = p["kf"]["m_id_f"] if kf_to_frame else p["fr"]["m_id_kf"]
            oth = p["fr"]["m_id_kf"] if kf_to_frame else p["kf"]["m_id_f"]
            col_d, _ = port.mutual_exclusion(p, 4.0, True, kf_to_frame)
            col_k, (seen, kept) = port.mutual_exclusion(p, 4.0, False, kf_to_frame)
            back = np.where(col0 >= 0, oth[np.maximum(col0, 0)], -1)
            st["mutual_dropped_non_mutual"] = st.get("mutual_dropped_non_mutual", 0) + int((col_d != col_k).sum())
            st["mutual_failed_dist_" + tag] = st.get("mutual_failed_dist_" + tag, 0) + int((col_k != col0).sum())
            st["mutual_passed_dist_" + tag] = st.get("mutual_passed_dist_" + tag, 0) + int(((col_k >= 0) & (back >= 0) & (back != np.arange(len(col0)))).sum())
            assert kept == int(((col_k >= 0) & (back >= 0)).sum()) and seen == int((col0 >= 0).sum())
    assert all(st.get(k, 0) > 0 for k in REQUIRED), {k: st.get(k, 0) for k in REQUIRED}
    stored = dict(zip([str(s) for s in z["stat_names"]], [int(v) for v in z["stat_values"]]))
    assert {k: st[k] for k in stored} == stored
    combos = {(c["pair"], c["direction"], c["k_huber"], c["iter_max"], c["prune"]) for c in f["cases"]}
    assert combos == {(p, d, kh, it, pr) for p in (3, 4, 5, 6) for d in (0, 1) for kh in (0.0, 2.0) for it in (0, 10) for pr in (0, 3)}
    # 20 % of the links dropped in each direction, and unlinked KeyLines between linked ones
    for p in f["pairs"][3:7]:
        for col in (p["kf"]["m_id_f"], p["fr"]["m_id_kf"]):
            assert 0.1 < (col < 0).mean() < 0.35
    # the degenerate inputs are what they are named after
    assert (f["pairs"][1]["kf"]["m_id_f"] >= 0).sum() == 1 and (f["pairs"][2]["fr"]["m_id_kf"] >= 0).sum() == 5
    nan, oob = f["pairs"][7], f["pairs"][8]
    assert np.isnan(nan["kf"]["rho"][nan["kf"]["m_id_f"] >= 0]).sum() == 1 and np.isnan(nan["fr"]["rho"][nan["fr"]["m_id_kf"] >= 0]).sum() == 1
    assert (oob["kf"]["m_id_f"] >= len(oob["fr"]["rho"])).sum() == 1 and (oob["fr"]["m_id_kf"] >= len(oob["kf"]["rho"])).sum() == 1


def test_chained_links_are_the_tracking_s():
    f = fixture("chained")
    assert (int(f["cam"]["w"]), int(f["cam"]["h"])) == (256, 192) and len(f["pairs"]) >= 1
    for p in f["pairs"]:
        assert len(p["kf"]["rho"]) > 1000 and (p["kf"]["m_id_f"] >= 0).sum() > 500 and (p["fr"]["m_id_kf"] >= 0).sum() > 500


def test_degenerate_inputs_follow_the_device_rule():
    f = fixture("crafted")
    for direction in (0, 1):
        none = port.constraint(f["pairs"][0], direction, 10, 2.0)
        assert none["guard"] == 3 and none["evals"] == 2 and none["accepted"] == 0 and none["links"] == 0
        R, T = port.start_pose(f["pairs"][0], direction)
        assert np.array_equal(none["X"], np.concatenate([T, port.so3_ln(R)]))
        for j, links in ((1, 1), (2, 5)):
            few = port.constraint(f["pairs"][j], direction, 10, 2.0)
            assert few["guard"] & 2 and few["links"] == links and np.isfinite(few["X"]).all()
        nan = port.constraint(f["pairs"][7], direction, 10, 2.0)
        assert nan["guard"] == 1 and nan["evals"] == 2
        R, T = port.start_pose(f["pairs"][7], direction)
        assert np.array_equal(nan["X"], np.concatenate([T, port.so3_ln(R)]))
        oob = port.constraint(f["pairs"][8], direction, 10, 2.0)
        assert oob["guard"] == 4 and oob["evals"] == 12 and np.isfinite(oob["X"]).all()
        # the link out of range was taken as unmatched: the same as with that link cleared
        p = f["pairs"][8]
        kf, fr = dict(p["kf"]), dict(p["fr"])
        kf["m_id_f"] = np.where(kf["m_id_f"] >= len(fr["rho"]), -1, kf["m_id_f"])
        fr["m_id_kf"] = np.where(fr["m_id_kf"] >= len(kf["rho"]), -1, fr["m_id_kf"])
        clean = port.constraint(dict(p, kf=kf, fr=fr), direction, 10, 2.0)
        assert clean["guard"] == 0 and all(np.array_equal(clean[k], oob[k]) for k in ("X", "W_X", "R_X", "ratio", "Kp", "links"))
    # iter_max = 0 never steps: no guard bit 0 even without links
    assert port.constraint(f["pairs"][0], 1, 0, 0.0)["guard"] == 2


def test_residual_is_shared_across_rejected_steps():
    """A case where a step is rejected and another evaluation follows: the weights of that evaluation are the rejected evaluation's
    residuals'.  Weighting by the last accepted evaluation's instead (Minimizer_RV_KF's swap) gives other weights there and another X; the
    reference's recorded X is the shared rule's."""
    f = fixture("crafted")
    shown = 0
    for case in f["cases"]:
        if case["k_huber"] <= 0 or case["iter_max"] == 0 or case["prune"]:
            continue
        pair = f["pairs"][case["pair"]]
        ta, tb = {}, {}
        a = port.constraint(pair, case["direction"], case["iter_max"], case["k_huber"], ta)
        b = port.constraint(pair, case["direction"], case["iter_max"], case["k_huber"], tb, shared_residual=False)
        if not ta.get("rejected"):
            continue
        differ = [n for n, (wa, wb) in enumerate(zip(ta["weights"], tb["weights"])) if not np.array_equal(wa, wb)]
        if not differ:
            continue
        assert differ[0] >= 3                      # evaluations 0, 1 (start pose) and 2 (the first step) see the same residuals either way
        assert rel(a["X"], case["ref"]["X"]) <= 1e-12
        if rel(b["X"], case["ref"]["X"]) > 1e-9:
            shown += 1
    assert shown > 0


def test_abi_struct_sizes():
    from rebvo_amd import edgehip
    assert C.sizeof(edgehip.KfConstraint) == 688 and edgehip.KF_CONSTRAINT_DTYPE.itemsize == 688
    assert C.sizeof(edgehip.KfConstraintArgs) == 16
    assert edgehip.KF_CONSTRAINT_DTYPE.names == ("X", "W_X", "R_X", "ratio", "E", "E0", "Kp", "W_Kp", "links", "inliers", "evals", "accepted",
                                                 "guard", "pad")
    assert edgehip.KfConstraint.links.offset == 664 and edgehip.KfConstraint.ratio.offset == 624
    for name in ("edgehip_keyframe_constraint", "edgehip_keyframe_mutual_exclusion", "edgehip_keyframe_constraint_ms"):
        assert name in edgehip.EXPORTS
