"""The key-frame relative-pose constraint on the device (edgehip_keyframe_constraint, edgehip_keyframe_mutual_exclusion) against the
reference's recorded outputs (tests/golden/keyframe_constraint/): every count and every link after pruning equal; the fp64 outputs within
the project's tolerances for fp64 sums over KeyLines in another fixed order (tests/test_stage_b_gpu.py::test_minimizer_rv_kf):
X 1e-9 relative + 1e-12; ratio, E, E0, Kp, W_Kp 1e-9 relative; W_X 1e-9 of its largest entry; R_X 1e-7 of its largest entry.
Key frames are seeded with upload_keyframe, the frame lists with upload_keylines into ring slot 0; the batches are ragged."""
import ctypes as C
import os

import numpy as np
import pytest

import keyframe_constraint_port as port
from rebvo_amd import edgehip

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_constraint")
_FX = {}
FLOATS = ("X", "W_X", "R_X", "ratio", "E", "E0", "Kp", "W_Kp")
INTS = ("links", "inliers", "evals", "accepted", "guard")


def fixture(name):
    if name not in _FX:
        f = port.load_fixture(os.path.join(GOLD, name + ".npz"))
        f["by_key"] = {(c["pair"], c["direction"], c["k_huber"], c["iter_max"], c["prune"]): c for c in f["cases"]}
        f["max_points"] = 1100 if name == "crafted" else max(max(len(p["kf"]["rho"]), len(p["fr"]["rho"])) for p in f["pairs"]) + 3
        _FX[name] = f
    return _FX[name]


def context(f, nseq, track=True):
    cam = f["cam"]
    p = edgehip.euroc_params(int(cam["w"]), int(cam["h"]), ppx=float(cam["ppx"]), ppy=float(cam["ppy"]), zfx=float(cam["zfx"]),
                             zfy=float(cam["zfy"]), max_points=f["max_points"])
    eh = edgehip.EdgeHip(p, nseq=nseq, nslots=2, device=0)
    if track:
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
    return eh


def seed(eh, f, layout, slot=0):
    """layout[seq]: the fixture pair the sequence holds (None: no key frame, an empty slot)."""
    for s, j in enumerate(layout):
        if j is None:
            continue
        p = f["pairs"][j]
        eh.upload_keyframe(s, port.records(p["kf"], edgehip.KEYLINE_DTYPE, dict(m_id_f=p["kf"]["m_id_f"])),
                           edgehip.EdgeHip.kf_pose(p["kf_Pose"], p["kf_Pos"], K=float(p["kf_K"])))
        eh.upload_keylines(s, slot, port.records(p["fr"], edgehip.KEYLINE_DTYPE, dict(m_id_kf=p["fr"]["m_id_kf"])))


def poses(f, layout):
    P = np.stack([np.eye(3) if j is None else f["pairs"][j]["Pose"] for j in layout])
    T = np.stack([np.zeros(3) if j is None else f["pairs"][j]["Pos"] for j in layout])
    K = np.array([1.0 if j is None else float(f["pairs"][j]["K"]) for j in layout])
    return P, T, K


def close_to(got, ref, s, tag):
    """the issue's tolerances, each figure printed before it is asserted"""
    ex = np.abs(got["X"][s] - ref["X"])
    print(tag, "X err", ex.max(), "of", np.abs(ref["X"]).max())
    assert (ex <= 1e-9 * np.abs(ref["X"]) + 1e-12).all(), (tag, "X", got["X"][s], ref["X"])
    for k in ("ratio", "E", "E0", "Kp", "W_Kp"):
        e = abs(got[k][s] - ref[k])
        print(tag, k, "rel err", e / max(abs(float(ref[k])), 1e-300))
        assert e <= 1e-9 * abs(ref[k]), (tag, k, got[k][s], ref[k])
    for k, tol in (("W_X", 1e-9), ("R_X", 1e-7)):
        e = np.abs(got[k][s] - ref[k]).max() / np.abs(ref[k]).max()
        print(tag, k, "err of largest", e)
        assert e <= tol, (tag, k, e)
    assert (got["links"][s], got["inliers"][s]) == (ref["links"], ref["inliers"]), (tag, "match_num")
    assert got["guard"][s] == 0, (tag, "guard")


def links_of(eh, s, slot=0):
    return eh.download_keyframe(s)[0]["m_id_f"].copy(), eh.download_keylines(s, slot, want_mask=False)[0]["m_id_kf"].copy()


COMBOS = [(d, kh, it, pr) for d in (0, 1) for kh in (0.0, 2.0) for it in (0, 10) for pr in (0, 3)]


@pytest.mark.parametrize("name,layout", [("crafted", [3, 0, 4, 7, 5, 1, 6]), ("crafted", [6, 2, 3]), ("crafted", [5, 4, 8]),
                                         ("chained", [0, 1, 0]), ("chained", [1, 0, None, 0, 1, 1, 0])])
def test_every_compared_case_equals_the_reference(name, layout):
    f = fixture(name)
    eh = context(f, len(layout))
    try:
        P, T, K = poses(f, layout)
        compared = 0
        for pr in (0, 3):
            seed(eh, f, layout)
            if pr:
                c1 = eh.keyframe_mutual_exclusion(0, 4.0, True, True)
                c0 = eh.keyframe_mutual_exclusion(0, 4.0, True, False)
                for s, j in enumerate(layout):
                    if j is None:
                        assert list(c1[s]) + list(c0[s]) == [0, 0, 0, 0]
                        continue
                    _, want = port.pruned(f["pairs"][j], 4.0, 1, 3)
                    assert list(c1[s]) + list(c0[s]) == list(want), (s, j)
            for d, kh, it, _ in [c for c in COMBOS if c[3] == pr]:
                got = eh.keyframe_constraint(0, d, it, kh, P, T, K)
                for s, j in enumerate(layout):
                    case = f["by_key"].get((j, d, kh, it, pr))
                    if case is None:
                        continue
                    if pr:
                        mf, mk = links_of(eh, s)
                        assert np.array_equal(mf, case["m_id_f"]) and np.array_equal(mk, case["m_id_kf"]), (s, j, "pruned links")
                        assert list(c1[s]) + list(c0[s]) == list(case["ref"]["prune_counts"])
                    close_to(got, case["ref"], s, f"{name} seq {s} pair {j} dir {d} huber {kh} iter {it} prune {pr}")
                    assert got["evals"][s] == it + 2
                    compared += 1
        wanted = sum(layout.count(k[0]) for k in f["by_key"])
        assert compared == wanted and compared > 0
    finally:
        eh.close()


def test_alone_and_inside_a_batch_bit_identical():
    f = fixture("crafted")
    outs = []
    for layout in ([6], [3, 4, 5, 0, 6, 2, 7], [5, 6, 6]):
        eh = context(f, len(layout))
        try:
            seed(eh, f, layout)
            P, T, K = poses(f, layout)
            for d, kh in ((1, 2.0), (0, 0.0)):
                got = eh.keyframe_constraint(0, d, 10, kh, P, T, K)
                outs.append([{k: got[k][s].tobytes() for k in FLOATS + INTS} for s, j in enumerate(layout) if j == 6])
        finally:
            eh.close()
    for d in (0, 1):
        same = outs[d] + outs[2 + d] + outs[4 + d]
        assert len(same) == 4 and all(o == same[0] for o in same)


def test_degenerate_inputs_guard_bits_and_neighbours():
    f = fixture("crafted")
    layout = [0, 3, 1, 7, 2, 8, 4]
    eh = context(f, 7)
    try:
        seed(eh, f, layout)
        P, T, K = poses(f, layout)
        for d in (0, 1):
            got = eh.keyframe_constraint(0, d, 10, 2.0, P, T, K)
            want = [port.constraint(f["pairs"][j], d, 10, 2.0) for j in layout]
            assert [int(g) for g in got["guard"]] == [w["guard"] for w in want]
            assert got["guard"][0] == 3 and got["guard"][3] == 1 and got["guard"][5] == 4 and got["guard"][2] & 2 and got["guard"][4] & 2
            assert [int(x) for x in got["links"]] == [w["links"] for w in want] and list(got["links"][[0, 2, 4]]) == [0, 1, 5]
            assert list(got["evals"][[0, 3]]) == [2, 2] and list(got["accepted"][[0, 3]]) == [0, 0]
            for s in (0, 3):                     # nothing was accepted: the start pose comes back (ln is libm's: 1e-12)
                R, T0 = port.start_pose(f["pairs"][layout[s]], d)
                start = np.concatenate([T0, port.so3_ln(R)])
                assert np.allclose(got["X"][s], start, rtol=1e-12, atol=1e-15), s
            # the neighbours in the batch are the fixture's
            for s in (1, 6):
                close_to(got, f["by_key"][(layout[s], d, 2.0, 10, 0)]["ref"], s, f"neighbour seq {s} dir {d}")
            # the link out of range was taken as unmatched
            w = want[5]
            assert got["evals"][5] == 12 and np.isfinite(got["X"][5]).all()
            assert np.allclose(got["X"][5], w["X"], rtol=1e-9, atol=1e-12) and got["inliers"][5] == w["inliers"]
        # iter_max = 0 never steps
        got = eh.keyframe_constraint(0, 1, 0, 0.0, P, T, K)
        assert got["guard"][0] == 2 and got["evals"][0] == 2
    finally:
        eh.close()


def snapshot(eh):
    out = []
    for s in range(eh.nseq):
        kl, pose, count = eh.download_keyframe(s)
        out += [kl.tobytes(), bytes(pose), count]
        for slot in range(2):
            kl, mask = eh.download_keylines(s, slot)
            out += [kl.tobytes(), mask.tobytes()]
    return out


def test_constraint_is_read_only_and_pruning_edits_one_column():
    f = fixture("crafted")
    layout = [4, 0, 5]
    eh = context(f, 3)
    try:
        seed(eh, f, layout)
        P, T, K = poses(f, layout)
        before = snapshot(eh)
        for d in (0, 1):
            eh.keyframe_constraint(0, d, 10, 2.0, P, T, K)
        eh.keyframe_constraint(0, 1, 3, 0.0)
        assert snapshot(eh) == before
        for kf_to_frame, discard in ((True, False), (False, True), (True, True)):
            kfs = [eh.download_keyframe(s)[0] for s in range(3)]
            frs = [eh.download_keylines(s, 0)[0] for s in range(3)]
            other = [eh.download_keylines(s, 1)[0] for s in range(3)]
            cnt = eh.keyframe_mutual_exclusion(0, 4.0, discard, kf_to_frame)
            changed = 0
            for s in range(3):
                kf2, fr2 = eh.download_keyframe(s)[0], eh.download_keylines(s, 0)[0]
                assert eh.download_keylines(s, 1)[0].tobytes() == other[s].tobytes()
                pair = dict(f["pairs"][layout[s]], kf=dict(f["pairs"][layout[s]]["kf"], m_id_f=kfs[s]["m_id_f"]),
                            fr=dict(f["pairs"][layout[s]]["fr"], m_id_kf=frs[s]["m_id_kf"]))
                col, c = port.mutual_exclusion(pair, 4.0, discard, kf_to_frame)
                assert list(cnt[s]) == list(c), (s, kf_to_frame)
                edited, kept, name = (kf2, fr2, "m_id_f") if kf_to_frame else (fr2, kf2, "m_id_kf")
                was, kept_was = (kfs[s], frs[s]) if kf_to_frame else (frs[s], kfs[s])
                assert np.array_equal(edited[name], col)
                changed += int((edited[name] != was[name]).sum())
                assert kept.tobytes() == kept_was.tobytes()
                back = edited.copy()
                back[name] = was[name]
                assert back.tobytes() == was.tobytes()            # only the one column moved
            assert changed > 0
        # no counts wanted: in-stream, and the same edit
        assert eh.keyframe_mutual_exclusion(0, 1.0, True, True, want_counts=False) is None
    finally:
        eh.close()


def test_null_pose_defaults():
    """Pose * R, Pos - Pose * R * V * K and K of seq_state, as edgehip_keyframe_forward_correct takes them."""
    f = fixture("crafted")
    layout = [5, 3, 6]
    eh = context(f, 3)
    try:
        seed(eh, f, layout)
        P, T, K = poses(f, layout)
        rs = np.random.RandomState(3)
        for s in range(3):
            st = eh.get_state(s)
            R = port.so3_exp(rs.normal(0, 0.05, 3))
            V = rs.normal(0, 0.05, 3)
            base = P[s] @ R.T                                  # Pose_state * R = the frame's Pose
            st.Pose[:] = list(base.ravel())
            st.R[:] = list(R.ravel())
            st.V[:] = list(V)
            st.K = float(K[s])
            st.Pos[:] = list(T[s] + (base @ R) @ V * K[s])     # Pos_state - Pose * V * K = the frame's Pos
            eh.set_state(s, st)
        want = eh.keyframe_constraint(0, 1, 10, 2.0, P, T, K)
        got = eh.keyframe_constraint(0, 1, 10, 2.0)
        for s in range(3):
            assert np.allclose(got["X"][s], want["X"][s], rtol=1e-9, atol=1e-12)
            assert np.allclose(got["ratio"][s], want["ratio"][s], rtol=1e-9) and got["links"][s] == want["links"][s]
        far = eh.keyframe_constraint(0, 1, 0, 2.0, P, T + 0.5, K)
        assert not np.allclose(far["X"], want["X"], rtol=1e-3)
    finally:
        eh.close()


def test_error_returns():
    f = fixture("crafted")
    eh = context(f, 3, track=False)
    try:
        lib = eh.lib
        a = edgehip.KfConstraintArgs(1, 10, 2.0)
        out = np.zeros(3, edgehip.KF_CONSTRAINT_DTYPE)
        po = out.ctypes.data_as(C.c_void_p)
        cnt = np.zeros((3, 2), np.int32)
        g = C.c_double(0)
        assert lib.edgehip_keyframe_constraint(eh.ctx, 0, None, None, None, C.byref(a), po) == -4                  # EDGEHIP_ERR_STATE
        assert lib.edgehip_keyframe_mutual_exclusion(eh.ctx, 0, C.c_double(4.0), 1, 1, cnt.ctypes.data_as(C.c_void_p)) == -4
        assert lib.edgehip_keyframe_constraint_ms(eh.ctx, C.byref(g), C.byref(g)) == -4
        assert lib.edgehip_keyframe_constraint(None, 0, None, None, None, C.byref(a), po) == -1                    # no context
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        assert lib.edgehip_keyframe_constraint(eh.ctx, 0, None, None, None, None, po) == -1                        # EDGEHIP_ERR_ARG
        assert lib.edgehip_keyframe_constraint(eh.ctx, 0, None, None, None, C.byref(a), None) == -1
        for bad in (edgehip.KfConstraintArgs(1, -1, 2.0), edgehip.KfConstraintArgs(2, 10, 2.0), edgehip.KfConstraintArgs(-1, 10, 2.0)):
            assert lib.edgehip_keyframe_constraint(eh.ctx, 0, None, None, None, C.byref(bad), po) == -1
        for slot in (-1, 2):
            assert lib.edgehip_keyframe_constraint(eh.ctx, slot, None, None, None, C.byref(a), po) == -1
            assert lib.edgehip_keyframe_mutual_exclusion(eh.ctx, slot, C.c_double(4.0), 1, 1, None) == -1
        P = np.zeros((3, 9))
        assert lib.edgehip_keyframe_constraint(eh.ctx, 0, P.ctypes.data_as(C.POINTER(C.c_double)), None, None, C.byref(a), po) == -1
        with pytest.raises(edgehip.EdgeHipError):
            eh.keyframe_constraint(0, 3, 10, 2.0)
        assert lib.edgehip_keyframe_constraint(eh.ctx, 0, None, None, None, C.byref(a), po) == 0                   # the context stays usable
        assert (out["links"] == 0).all() and (out["guard"] == 3).all()
        gather_ms, solve_ms = eh.keyframe_constraint_ms()
        assert gather_ms > 0 and solve_ms > 0
    finally:
        eh.close()


def test_after_reset_and_a_resized_list():
    f = fixture("crafted")
    layout = [3, 6, 4]
    eh = context(f, 3)
    try:
        P, T, K = poses(f, layout)
        seed(eh, f, layout)
        first = eh.keyframe_constraint(0, 1, 10, 2.0, P, T, K)
        eh.reset()
        none = eh.keyframe_constraint(0, 1, 10, 2.0, P, T, K)            # no key frames: no links
        assert (none["links"] == 0).all() and (none["guard"] == 3).all()
        eh.keyframe_list_enable(2)
        seed(eh, f, [5, 5, 5])
        seed(eh, f, layout)                                              # (the first three retire into the list)
        again = eh.keyframe_constraint(0, 1, 10, 2.0, P, T, K)
        eh.keyframe_list_enable(1)
        third = eh.keyframe_constraint(0, 1, 10, 2.0, P, T, K)
        for k in FLOATS + INTS:
            assert again[k].tobytes() == first[k].tobytes() and third[k].tobytes() == first[k].tobytes(), k
        for s in range(3):
            close_to(first, f["by_key"][(layout[s], 1, 2.0, 10, 0)]["ref"], s, f"seq {s}")
    finally:
        eh.close()
