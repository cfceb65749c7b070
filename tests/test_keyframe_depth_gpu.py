"""Depth along the key-frame links on the device (edgehip_keyframe_map_depth, edgehip_keyframe_translate_depth,
edgehip_keyframe_list_translate_depth) against the reference's recorded outputs (tests/golden/keyframe_depth/): every rho / s_rho the calls
write bit for bit (NaN as a class), every count and m_num equal; with optim_scale K, rTr, rTr0, rho and s_rho within 1e-9 relative, the
project's tolerance for fp64 sums over KeyLines in another fixed order (tests/test_stage_b_gpu.py::test_minimizer_rv_kf).
Key frames are seeded with upload_keyframe, the frame lists with upload_keylines into ring slot 0, lists by consecutive upload_keyframe
calls with the list enabled; the batches are ragged."""
import ctypes as C
import os

import numpy as np
import pytest

import keyframe_depth_port as port
from rebvo_amd import edgehip, synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_depth")
_FX = {}
MAP_ARGS = ((0.0, 0.0, 1.0), (1e-3, 5e-2, 2.0))
# (call, direction, optim_scale, args) of the calls compared bit for bit
EXACT = [("map", 0, 0, MAP_ARGS[0]), ("map", 0, 0, MAP_ARGS[1]), ("translate", 0, 0, (0.0, 0.0, 0.0)), ("translate", 1, 0, (0.0, 0.0, 0.0))]
OUT = ("count", "guard", "K", "rTr", "rTr0")


def fixture(name):
    if name not in _FX:
        f = port.load_fixture(os.path.join(GOLD, name + ".npz"))
        f["by_key"] = {(c["pair"], c["call"], c["direction"], c["optim"], c["args"]): c for c in f["cases"]}
        f["kind"] = {p["kind"]: j for j, p in enumerate(f["pairs"])}
        sizes = [max(len(p["kf"]["rho"]), len(p["fr"]["rho"])) for p in f["pairs"]] + [len(k["kl"]["rho"]) for lst in f["lists"] for k in lst]
        f["max_points"] = 1100 if name == "crafted" else max(sizes) + 3
        _FX[name] = f
    return _FX[name]


def context(f, nseq, track=True, list_capacity=0):
    cam = f["cam"]
    p = edgehip.euroc_params(int(cam["w"]), int(cam["h"]), ppx=float(cam["ppx"]), ppy=float(cam["ppy"]), zfx=float(cam["zfx"]),
                             zfy=float(cam["zfy"]), max_points=f["max_points"])
    eh = edgehip.EdgeHip(p, nseq=nseq, nslots=2, device=0)
    if track:
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        if list_capacity:
            eh.keyframe_list_enable(list_capacity)
    return eh


def kf_records(p):
    return port.records(p["kf"], edgehip.KEYLINE_DTYPE, dict(m_id_f=p["kf"]["m_id_f"]))


def seed(eh, pairs, slot=0, kf_K=None):
    """pairs[seq]: the pair the sequence holds (None: no key frame, an empty slot)."""
    for s, p in enumerate(pairs):
        if p is None:
            continue
        eh.upload_keyframe(s, kf_records(p), edgehip.EdgeHip.kf_pose(p["kf_Pose"], p["kf_Pos"], K=float(p["kf_K"] if kf_K is None else kf_K[s])))
        eh.upload_keylines(s, slot, port.records(p["fr"], edgehip.KEYLINE_DTYPE, dict(m_id_kf=p["fr"]["m_id_kf"])))


def poses(pairs):
    P = np.stack([np.eye(3) if p is None else p["Pose"] for p in pairs])
    T = np.stack([np.zeros(3) if p is None else p["Pos"] for p in pairs])
    K = np.array([1.0 if p is None else float(p["K"]) for p in pairs])
    return P, T, K


def call(eh, what, d, opt, args, P=None, T=None, K=None):
    if what == "map":
        return eh.keyframe_map_depth(0, args[0], args[1], args[2], P, T)
    return eh.keyframe_translate_depth(0, d, opt, P, T, K)


def written(eh, s, what, d):
    """the list the call writes, as records"""
    return eh.download_keylines(s, 0, want_mask=False)[0] if (what == "translate" and d) else eh.download_keyframe(s)[0]


def want(what, d, opt, args, p):
    """the port's answer for a pair (the generator held it against the reference bit for bit)"""
    if what == "map":
        rho, s_rho, count, guard = port.map_depth(p, *args)
        return dict(rho=rho, s_rho=s_rho, m_num=np.asarray(p["kf"]["m_num"]), count=count, guard=guard, K=0.0, rTr=0.0, rTr0=0.0)
    return port.translate(p, d, bool(opt))


def equals_reference(kl, ref, tag):
    if "rho" in ref:
        assert port.same_bits(kl["rho"], ref["rho"]), (tag, "rho", np.nonzero(kl["rho"] != ref["rho"])[0][:8])
        assert port.same_bits(kl["s_rho"], ref["s_rho"]), (tag, "s_rho", np.nonzero(kl["s_rho"] != ref["s_rho"])[0][:8])
        assert np.array_equal(kl["m_num"], ref["m_num"]), (tag, "m_num")
    assert port.digest(kl["rho"], kl["s_rho"], kl["m_num"]) == (ref["digest"]), (tag, "digest")


def layouts(f, idx):
    return [None if j is None else f["pairs"][j] for j in idx]


PAIR_LAYOUTS = [("crafted", [5, None, 3]), ("crafted", [6, 1, 4, None, 9, 2, 10]), ("chained", [0, None, 1]), ("chained", [1, 0, None, 0, 1, 1, 0])]


@pytest.mark.parametrize("name,idx", PAIR_LAYOUTS)
def test_every_compared_case_equals_the_reference(name, idx):
    f = fixture(name)
    pairs = layouts(f, idx)
    eh = context(f, len(idx))
    try:
        P, T, K = poses(pairs)
        compared = 0
        for what, d, opt, args in EXACT:
            seed(eh, pairs)
            got = call(eh, what, d, opt, args, P, T, K)
            for s, j in enumerate(idx):
                if j is None:
                    assert (got["count"][s], got["guard"][s], got["K"][s]) == (0, 0, 0.0)
                    continue
                case = f["by_key"][(j, what, d, opt, args)]
                tag = f"{name} seq {s} pair {j} {what} dir {d} {args}"
                assert got["count"][s] == case["ref"]["count"] and got["guard"][s] == 0, tag
                assert (got["rTr"][s], got["rTr0"][s]) == (0.0, 0.0) and got["K"][s] == (float(pairs[s]["kf_K"]) if what == "translate" else 0.0), tag
                equals_reference(written(eh, s, what, d), dict(case["ref"], digest=case["ref"]["digest"]), tag)
                compared += 1
        assert compared == 4 * sum(j is not None for j in idx)
        assert eh.keyframe_depth_ms() > 0
    finally:
        eh.close()


def seed_lists(eh, chains):
    """chains[seq]: a key-frame list (None: no key frame): consecutive uploads, the older ones retire into the list"""
    for s, chain in enumerate(chains):
        for k in chain or []:
            eh.upload_keyframe(s, port.records(k["kl"], edgehip.KEYLINE_DTYPE, dict(m_id_f=k["kl"]["m_id_f"])),
                               edgehip.EdgeHip.kf_pose(k["Pose"], k["Pos"], K=float(k["K"])))


def list_positions(eh, s, n):
    """the records of the sequence's n positions: list entries, oldest first, then the current key frame"""
    return [eh.download_keyframe_list(s, i)[0] for i in range(n - 1)] + ([eh.download_keyframe(s)[0]] if n else [])


@pytest.mark.parametrize("name,idx,capacity", [("crafted", [0, None, 1], 3), ("crafted", [1, 2, 0, None, 0, 2, 1], 4), ("chained", [0, None, 0], 2)])
def test_list_pass_equals_the_reference(name, idx, capacity):
    f = fixture(name)
    chains = [None if j is None else f["lists"][j] for j in idx]
    eh = context(f, len(idx), list_capacity=capacity)
    try:
        for iters in (1, 3):
            eh.reset()
            seed_lists(eh, chains)
            got = eh.keyframe_list_translate_depth(iters)
            for s, j in enumerate(idx):
                if j is None:
                    assert (got["count"][s], got["guard"][s]) == (0, 0)
                    continue
                case = [c for c in f["list_cases"] if c["list"] == j and c["iters"] == iters][0]
                ref = case["ref"]
                assert got["count"][s] == ref["count"] and got["guard"][s] == 0 and (got["K"][s], got["rTr"][s], got["rTr0"][s]) == (0, 0, 0), (s, j, iters)
                for i, kl in enumerate(list_positions(eh, s, len(chains[s]))):
                    one = dict(digest=ref["digests"][i])
                    if "rho" in ref:
                        one.update(rho=ref["rho"][i], s_rho=ref["s_rho"][i], m_num=ref["m_num"][i])
                    equals_reference(kl, one, f"{name} seq {s} list {j} iters {iters} position {i}")
        # iters = 0 does nothing
        before = [list_positions(eh, s, len(c or [])) for s, c in enumerate(chains)]
        got = eh.keyframe_list_translate_depth(0)
        assert (got["count"] == 0).all()
        after = [list_positions(eh, s, len(c or [])) for s, c in enumerate(chains)]
        assert all(a.tobytes() == b.tobytes() for x, y in zip(before, after) for a, b in zip(x, y))
    finally:
        eh.close()


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = ~np.isnan(b)
    assert np.array_equal(np.isnan(a), ~ok)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300))) if ok.any() else 0.0


@pytest.mark.parametrize("name,idx", PAIR_LAYOUTS)
def test_optim_scale(name, idx):
    """K, rTr, rTr0, rho and s_rho within 1e-9 relative of the reference; and the rewrite is bit for bit the optim_scale = 0 call's with
    the key frame's K set to the K the device returned.
    Largest errors measured on an MI355X: see DESIGN.md §18."""
    f = fixture(name)
    pairs = layouts(f, idx)
    eh = context(f, len(idx))
    try:
        P, T, K = poses(pairs)
        seed(eh, pairs)
        got = eh.keyframe_translate_depth(0, 0, True, P, T, K)
        first = [None if p is None else eh.download_keyframe(s) for s, p in enumerate(pairs)]
        worst = dict(K=0.0, rTr=0.0, rTr0=0.0, rho=0.0, s_rho=0.0)
        for s, j in enumerate(idx):
            if j is None:
                assert (got["count"][s], got["K"][s]) == (0, 0.0)
                continue
            ref = f["by_key"][(j, "translate", 0, 1, (0.0, 0.0, 0.0))]["ref"]
            assert got["count"][s] == ref["count"] and got["guard"][s] == 0
            kl, pose, _ = first[s]
            assert pose.K == got["K"][s]                                       # the key frame's pose block took the K
            for k in ("K", "rTr", "rTr0"):
                worst[k] = max(worst[k], abs(got[k][s] - ref[k]) / max(abs(float(ref[k])), 1e-300))
            if "rho" in ref:
                worst["rho"] = max(worst["rho"], rel_err(kl["rho"], ref["rho"]))
                worst["s_rho"] = max(worst["s_rho"], rel_err(kl["s_rho"], ref["s_rho"]))
                assert np.array_equal(kl["m_num"], ref["m_num"])
        print(name, idx, "optim_scale: largest relative errors", worst)
        assert all(v <= 1e-9 for v in worst.values()), worst
        seed(eh, pairs, kf_K=got["K"])
        again = eh.keyframe_translate_depth(0, 0, False, P, T, K)
        for s, p in enumerate(pairs):
            if p is None:
                continue
            kl = eh.download_keyframe(s)[0]
            assert again["K"][s] == got["K"][s] and again["count"][s] == got["count"][s]
            assert port.same_bits(kl["rho"], first[s][0]["rho"]) and port.same_bits(kl["s_rho"], first[s][0]["s_rho"]), s
            assert np.array_equal(kl["m_num"], first[s][0]["m_num"])
    finally:
        eh.close()


def test_alone_and_inside_a_batch_bit_identical():
    f = fixture("crafted")
    calls = EXACT + [("translate", 0, 1, (0.0, 0.0, 0.0))]
    outs = []
    for idx in ([6], [3, 4, 5, 0, 6, 2, 7], [5, 6, 6]):
        pairs = layouts(f, idx)
        eh = context(f, len(idx), list_capacity=3)
        try:
            P, T, K = poses(pairs)
            for what, d, opt, args in calls:
                seed(eh, pairs)
                got = call(eh, what, d, opt, args, P, T, K)
                for s, j in enumerate(idx):
                    if j == 6:
                        kl = written(eh, s, what, d)
                        outs.append(((what, d, opt, args), [got[k][s].tobytes() for k in OUT], kl.tobytes(), bytes(eh.download_keyframe(s)[1])))
            eh.reset()
            seed_lists(eh, [f["lists"][0] if j == 6 else f["lists"][1] for j in idx])
            got = eh.keyframe_list_translate_depth(3)
            for s, j in enumerate(idx):
                if j == 6:
                    outs.append(("list", [got[k][s].tobytes() for k in OUT], b"".join(kl.tobytes() for kl in list_positions(eh, s, 4)), b""))
        finally:
            eh.close()
    for key in [c for c in calls] + ["list"]:
        same = [o[1:] for o in outs if o[0] == key]
        assert len(same) == 4 and all(o == same[0] for o in same), key


def only_changed(before, after, fields, at):
    """`after` differs from `before` in `fields` alone, and only at the indices `at`"""
    back = after.copy()
    for k in fields:
        assert np.array_equal(np.delete(after[k].view(np.int64 if after[k].dtype == np.float64 else np.int32), at),
                              np.delete(before[k].view(np.int64 if before[k].dtype == np.float64 else np.int32), at)), k
        back[k] = before[k]
    return back.tobytes() == before.tobytes()


def test_bytes_before_and_after():
    f = fixture("crafted")
    idx = [4, None, 5]
    pairs = layouts(f, idx)
    eh = context(f, 3)
    try:
        P, T, K = poses(pairs)
        for what, d, opt, args in EXACT + [("translate", 0, 1, (0.0, 0.0, 0.0))]:
            seed(eh, pairs)
            kf0 = [eh.download_keyframe(s) for s in range(3)]
            sl0 = [[eh.download_keylines(s, slot) for slot in range(2)] for s in range(3)]
            call(eh, what, d, opt, args, P, T, K)
            for s, p in enumerate(pairs):
                kl, pose, cnt = eh.download_keyframe(s)
                slots = [eh.download_keylines(s, slot) for slot in range(2)]
                assert cnt == kf0[s][2]
                assert slots[1][0].tobytes() == sl0[s][1][0].tobytes() and all(a[1].tobytes() == b[1].tobytes() for a, b in zip(slots, sl0[s]))
                if p is None:
                    assert kl.tobytes() == kf0[s][0].tobytes() and slots[0][0].tobytes() == sl0[s][0][0].tobytes()
                    continue
                if what == "translate" and d:      # KF2F: the slot's rho / s_rho at linked indices; the key frame untouched
                    at = port.linked(p["fr"]["m_id_kf"], len(p["kf"]["rho"]))[0]
                    assert kl.tobytes() == kf0[s][0].tobytes() and bytes(pose) == bytes(kf0[s][1])
                    assert only_changed(sl0[s][0][0], slots[0][0], ("rho", "s_rho"), at)
                    assert (slots[0][0]["rho"][at] != sl0[s][0][0]["rho"][at]).any()
                else:                              # the key frame's rho / s_rho (and m_num) at linked indices; the slot untouched
                    at = port.linked(p["kf"]["m_id_f"], len(p["fr"]["rho"]))[0]
                    assert slots[0][0].tobytes() == sl0[s][0][0].tobytes()
                    assert only_changed(kf0[s][0], kl, ("rho", "s_rho") + (("m_num",) if what == "translate" else ()), at)
                    assert (kl["rho"][at] != kf0[s][0]["rho"][at]).any()
                    if opt:                        # the pose block: K alone
                        q = edgehip.KfPose.from_buffer_copy(bytes(pose))
                        assert q.K != kf0[s][1].K
                        q.K = kf0[s][1].K
                        assert bytes(q) == bytes(kf0[s][1])
                    else:
                        assert bytes(pose) == bytes(kf0[s][1])
    finally:
        eh.close()
    # the list pass: rho, s_rho, m_num of the list entries at linked indices; the newest position and every pose untouched
    chains = [f["lists"][0], None, f["lists"][1]]
    eh = context(f, 3, list_capacity=3)
    try:
        seed_lists(eh, chains)
        before = [[eh.download_keyframe_list(s, i) for i in range(len(c or [])) if i + 1 < len(c)] for s, c in enumerate(chains)]
        cur = [eh.download_keyframe(s) for s in range(3)]
        slot0 = [eh.download_keylines(s, 0)[0] for s in range(3)]
        eh.keyframe_list_translate_depth(2)
        for s, c in enumerate(chains):
            now = eh.download_keyframe(s)
            assert now[0].tobytes() == cur[s][0].tobytes() and bytes(now[1]) == bytes(cur[s][1]) and now[2] == cur[s][2]
            assert eh.download_keylines(s, 0)[0].tobytes() == slot0[s].tobytes()
            for i, (kl0, pose0) in enumerate(before[s]):
                kl, pose = eh.download_keyframe_list(s, i)
                at = port.linked(c[i]["kl"]["m_id_f"], len(c[i + 1]["kl"]["rho"]))[0]
                assert bytes(pose) == bytes(pose0)
                assert only_changed(kl0, kl, ("rho", "s_rho", "m_num"), at) and (kl["m_num"][at] == kl0["m_num"][at] + 2).all()
    finally:
        eh.close()


def test_guards_and_neighbours():
    f = fixture("crafted")
    k = f["kind"]
    # a pair whose scale sums are not finite: a linked key-frame KeyLine and its partner without variance (v = 0)
    bad = dict(f["pairs"][4], kf=dict(f["pairs"][4]["kf"]), fr=dict(f["pairs"][4]["fr"]))
    i = int(np.nonzero(bad["kf"]["m_id_f"] >= 0)[0][7])
    bad["kf"]["s_rho"], bad["fr"]["s_rho"] = bad["kf"]["s_rho"].copy(), bad["fr"]["s_rho"].copy()
    bad["kf"]["s_rho"][i] = 0.0
    bad["fr"]["s_rho"][bad["kf"]["m_id_f"][i]] = 0.0
    idx = [3, k["link_out_of_range"], k["nan_rho"], 4]
    pairs = layouts(f, idx) + [bad]
    eh = context(f, 5)
    try:
        P, T, K = poses(pairs)
        for what, d, opt, args in EXACT + [("translate", 0, 1, (0.0, 0.0, 0.0))]:
            seed(eh, pairs)
            got = call(eh, what, d, opt, args, P, T, K)
            exp = [want(what, d, opt, args, p) for p in pairs]
            assert [int(g) for g in got["guard"]] == [e["guard"] for e in exp], (what, d, opt)
            assert list(got["guard"][:4]) == [0, 4, 0, 0] and got["guard"][4] == (1 if opt else 0)
            assert [int(c) for c in got["count"]] == [e["count"] for e in exp]
            for s, p in enumerate(pairs):
                if opt and s != 4:
                    continue                       # (with optim_scale the port's K is the serial sum's: test_optim_scale's tolerance covers it)
                kl = written(eh, s, what, d)
                assert port.same_bits(kl["rho"], exp[s]["rho"]) and port.same_bits(kl["s_rho"], exp[s]["s_rho"]), (what, d, opt, s)
                assert np.array_equal(kl["m_num"], exp[s]["m_num"])
            if opt:
                assert got["K"][4] == float(bad["kf_K"]) and eh.download_keyframe(4)[1].K == float(bad["kf_K"])   # kf.K left as it was
            if what == "map":
                # the NaN rho ended in the reference's (RhoInit, RHO_MAX) branch
                j = int(np.nonzero(np.isnan(pairs[2]["kf"]["rho"]))[0][0])
                kl = written(eh, 2, what, d)
                assert (kl["rho"][j], kl["s_rho"][j]) == (1.0, 20.0)
                equals_reference(kl, f["by_key"][(idx[2], what, d, opt, args)]["ref"], "nan_rho")
            if not opt:
                for s in (0, 3):                   # the neighbours are the fixture's
                    equals_reference(written(eh, s, what, d), f["by_key"][(idx[s], what, d, opt, args)]["ref"], f"neighbour {s}")
        # a link out of range in a list
        chain = [dict(kk, kl=dict(kk["kl"])) for kk in f["lists"][1]]
        chain[0]["kl"]["m_id_f"] = chain[0]["kl"]["m_id_f"].copy()
        chain[0]["kl"]["m_id_f"][int(np.nonzero(chain[0]["kl"]["m_id_f"] >= 0)[0][2])] = len(chain[1]["kl"]["rho"])
        eh.keyframe_list_enable(2)
        eh.reset()
        seed_lists(eh, [f["lists"][1], chain, None, f["lists"][1], None])
        got = eh.keyframe_list_translate_depth(1)
        exp, count, guard = port.list_translate(chain, 1, float(f["cam"]["zfm"]))
        assert list(got["guard"]) == [0, 4, 0, 0, 0] and guard == 4 and got["count"][1] == count == got["count"][0] - 1
        kl = eh.download_keyframe_list(1, 0)[0]
        assert port.same_bits(kl["rho"], exp[0]["kl"]["rho"]) and port.same_bits(kl["s_rho"], exp[0]["kl"]["s_rho"])
        assert eh.download_keyframe_list(0, 0)[0].tobytes() == eh.download_keyframe_list(3, 0)[0].tobytes()
    finally:
        eh.close()


def test_select_leaves_the_other_sequences_alone():
    f = fixture("crafted")
    idx = [4, 5, 3]
    pairs = layouts(f, idx)
    eh = context(f, 3, list_capacity=2)
    try:
        P, T, K = poses(pairs)
        for what, d, opt, args in EXACT:
            seed(eh, pairs)
            before = [(eh.download_keyframe(s)[0].tobytes(), eh.download_keylines(s, 0)[0].tobytes()) for s in range(3)]
            eh.keyframe_depth_select([1, 0, 1])
            got = call(eh, what, d, opt, args, P, T, K)
            assert (got["count"][1], got["guard"][1], got["K"][1]) == (0, 0, 0.0)
            assert (eh.download_keyframe(1)[0].tobytes(), eh.download_keylines(1, 0)[0].tobytes()) == before[1]
            for s in (0, 2):
                equals_reference(written(eh, s, what, d), f["by_key"][(idx[s], what, d, opt, args)]["ref"], f"selected {s}")
            eh.keyframe_depth_select(None)
            got = call(eh, what, d, opt, args, P, T, K)
            assert got["count"][1] == f["by_key"][(idx[1], what, d, opt, args)]["ref"]["count"]
        eh.reset()
        seed_lists(eh, [f["lists"][1]] * 3)
        eh.keyframe_depth_select([0, 1, 0])
        got = eh.keyframe_list_translate_depth(1)
        assert list(got["count"] > 0) == [False, True, False]
        kls = [eh.download_keyframe_list(s, 0)[0] for s in range(3)]
        assert kls[0].tobytes() == kls[2].tobytes() != kls[1].tobytes() and np.array_equal(kls[0]["rho"], f["lists"][1][0]["kl"]["rho"])
    finally:
        eh.close()


def test_null_pose_defaults():
    """Pose * R, Pos - Pose * R * V * K and K of seq_state (what edgehip_keyframe_constraint takes by default), formed as the device forms
    them: the explicit call with those values gives the same bits."""
    f = fixture("crafted")
    pairs = layouts(f, [5, 3, 6])
    eh = context(f, 3)
    try:
        rs = np.random.RandomState(3)
        P, T, K = poses(pairs)
        for s in range(3):
            st = eh.get_state(s)
            R = synth._so3_exp(rs.normal(0, 0.05, 3))
            V = rs.normal(0, 0.05, 3)
            base = P[s] @ R.T
            st.Pose[:], st.R[:], st.V[:], st.K = list(base.ravel()), list(R.ravel()), list(V), float(K[s])
            st.Pos[:] = list(T[s] + (base @ R) @ V * K[s])
            eh.set_state(s, st)
            for r in range(3):
                for c in range(3):
                    P[s, r, c] = base[r, 0] * R[0, c] + base[r, 1] * R[1, c] + base[r, 2] * R[2, c]
            pos = np.array(st.Pos[:])
            for i in range(3):
                T[s, i] = pos[i] - (P[s, i, 0] * V[0] + P[s, i, 1] * V[1] + P[s, i, 2] * V[2]) * K[s]
        for what, d, opt, args in EXACT + [("translate", 0, 1, (0.0, 0.0, 0.0))]:
            seed(eh, pairs)
            a = call(eh, what, d, opt, args, P, T, K)
            ka = [written(eh, s, what, d) for s in range(3)]
            seed(eh, pairs)
            b = call(eh, what, d, opt, args)
            for s in range(3):
                assert written(eh, s, what, d).tobytes() == ka[s].tobytes(), (what, d, opt, s)
            assert all(a[k].tobytes() == b[k].tobytes() for k in OUT)
        seed(eh, pairs)
        far = eh.keyframe_translate_depth(0, 0, True, P, T + 0.5, K)
        assert not np.allclose(far["K"], a["K"], rtol=1e-3)
    finally:
        eh.close()


def test_error_returns():
    f = fixture("crafted")
    eh = context(f, 3, track=False)
    try:
        lib = eh.lib
        out = np.zeros(3, edgehip.KF_DEPTH_DTYPE)
        po = out.ctypes.data_as(C.c_void_p)
        one = C.c_double(1.0)
        zero = C.c_double(0.0)
        ms = C.c_double(0)
        dp = C.POINTER(C.c_double)
        assert lib.edgehip_keyframe_map_depth(eh.ctx, 0, None, None, zero, zero, one, po) == -4                    # EDGEHIP_ERR_STATE
        assert lib.edgehip_keyframe_translate_depth(eh.ctx, 0, 0, None, None, None, 0, po) == -4
        assert lib.edgehip_keyframe_list_translate_depth(eh.ctx, 1, po) == -4
        assert lib.edgehip_keyframe_depth_ms(eh.ctx, C.byref(ms)) == -4
        assert lib.edgehip_keyframe_map_depth(None, 0, None, None, zero, zero, one, po) == -1                      # no context
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        assert lib.edgehip_keyframe_list_translate_depth(eh.ctx, 1, po) == -4                                      # no list
        for slot in (-1, 2):
            assert lib.edgehip_keyframe_map_depth(eh.ctx, slot, None, None, zero, zero, one, po) == -1             # EDGEHIP_ERR_ARG
            assert lib.edgehip_keyframe_translate_depth(eh.ctx, slot, 0, None, None, None, 0, po) == -1
        P, T, K = np.zeros((3, 9)), np.zeros((3, 3)), np.ones(3)
        pp, pt, pk = P.ctypes.data_as(dp), T.ctypes.data_as(dp), K.ctypes.data_as(dp)
        assert lib.edgehip_keyframe_map_depth(eh.ctx, 0, pp, None, zero, zero, one, po) == -1
        assert lib.edgehip_keyframe_map_depth(eh.ctx, 0, None, pt, zero, zero, one, po) == -1
        for a, b, c in ((pp, None, None), (pp, pt, None), (None, None, pk), (None, pt, pk)):
            assert lib.edgehip_keyframe_translate_depth(eh.ctx, 0, 0, a, b, c, 0, po) == -1
        assert lib.edgehip_keyframe_translate_depth(eh.ctx, 0, 1, None, None, None, 1, po) == -1                   # optim_scale with direction 1
        assert lib.edgehip_keyframe_translate_depth(eh.ctx, 0, 2, None, None, None, 0, po) == -1
        eh.keyframe_list_enable(2)
        assert lib.edgehip_keyframe_list_translate_depth(eh.ctx, -1, po) == -1                                     # iters < 0
        with pytest.raises(edgehip.EdgeHipError):
            eh.keyframe_translate_depth(0, 1, True)
        # the context stays usable: no key frames, no links
        assert lib.edgehip_keyframe_map_depth(eh.ctx, 0, None, None, zero, zero, one, po) == 0
        assert (out["count"] == 0).all() and (out["guard"] == 0).all()
        assert lib.edgehip_keyframe_list_translate_depth(eh.ctx, 0, po) == 0 and lib.edgehip_keyframe_list_translate_depth(eh.ctx, 2, None) == 0
        assert eh.keyframe_map_depth(0, 0.0, 0.0, 1.0, want_result=False) is None                                  # in-stream
        assert eh.keyframe_depth_ms() >= 0
    finally:
        eh.close()


def test_after_reset_and_a_resized_key_frame():
    f = fixture("crafted")
    eh = context(f, 3)
    try:
        big, small = layouts(f, [6, 6, 5]), layouts(f, [4, 3, 4])
        P, T, K = poses(small)
        seed(eh, big)
        eh.keyframe_map_depth(0, *MAP_ARGS[1], *poses(big)[:2])
        eh.keyframe_translate_depth(0, 1, False, *poses(big))
        for what, d, opt, args in EXACT:
            seed(eh, small)                        # a smaller key frame and slot list after a larger one: no stale rows
            got = call(eh, what, d, opt, args, P, T, K)
            for s, j in enumerate([4, 3, 4]):
                case = f["by_key"][(j, what, d, opt, args)]
                assert got["count"][s] == case["ref"]["count"]
                equals_reference(written(eh, s, what, d), case["ref"], f"resized seq {s} {what} {d}")
        eh.reset()
        for what, d, opt, args in EXACT + [("translate", 0, 1, (0.0, 0.0, 0.0))]:
            got = call(eh, what, d, opt, args, P, T, K)  # no key frames: no links, nothing written
            assert (got["count"] == 0).all() and (got["guard"] == 0).all() and (got["K"] == 0).all()
        for s in range(3):
            assert len(eh.download_keyframe(s)[0]) == 0
    finally:
        eh.close()


def nav_rows(eh):
    return np.frombuffer(b"".join(bytes(n) for n in eh.read_nav()), edgehip.NAV_DTYPE).copy()


def test_composition_feeds_nothing_back():
    """A 6-frame replay with the tracking in the frame driver: keyframe_map_depth after every frame leaves every nav record and every
    key-frame tracking record as the replay without the calls has them; then one direction = 1 call changes the slot's rho / s_rho alone."""
    W, H, N = 256, 192, 6
    p = edgehip.euroc_params(W, H)
    frames = [f for f, _, _ in synth.billboard_sequence(W, H, N)]
    A, B = (edgehip.EdgeHip(p, nseq=2, nslots=3, device=0) for _ in range(2))
    try:
        mapped = 0
        for eh in (A, B):
            eh.keyframe_track_enable(True, 0.7, True)
        for k in range(N):
            frame = np.stack([frames[k], frames[k]])
            for eh in (A, B):
                eh.upload_rgb(eh.next_slot(), frame)
                eh.process_frame(0.05 * k)
            mapped += int(A.keyframe_map_depth(A.cur_slot(), 1e-3, 5e-2, 2.0)["count"].sum())
            assert nav_rows(A).tobytes() == nav_rows(B).tobytes(), k
            assert A.read_keyframe_track().tobytes() == B.read_keyframe_track().tobytes(), k
        assert mapped > 0
        assert A.download_keyframe(0)[0]["m_id_f"].tobytes() == B.download_keyframe(0)[0]["m_id_f"].tobytes()
        slot = A.cur_slot()
        before = [A.download_keylines(s, slot) for s in range(2)]
        others = [[A.download_keylines(s, t)[0].tobytes() for t in range(3) if t != slot] for s in range(2)]
        kf = [A.download_keyframe(s)[0].tobytes() for s in range(2)]
        got = A.keyframe_translate_depth(slot, 1)
        assert (got["count"] > 0).all()
        for s in range(2):
            kl, mask = A.download_keylines(s, slot)
            at = np.nonzero(before[s][0]["m_id_kf"] >= 0)[0]
            assert len(at) == got["count"][s] and mask.tobytes() == before[s][1].tobytes()
            assert only_changed(before[s][0], kl, ("rho", "s_rho"), at) and (kl["rho"][at] != before[s][0]["rho"][at]).any()
            assert [A.download_keylines(s, t)[0].tobytes() for t in range(3) if t != slot] == others[s]
            assert A.download_keyframe(s)[0].tobytes() == kf[s]
    finally:
        A.close()
        B.close()
