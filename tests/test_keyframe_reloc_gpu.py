"""Re-localisation against the key frames on the device (edgehip_keyframe_relocalize, _links, _ms).

What this file adds to tests/test_keyframe_reloc_ref_gpu.py (the reference's own OptimizePosGT, every fixture case): the batch and list
plumbing, where the reference has nothing to show.  Every served pair is put through the route the library offered before — the key frame's
records in a ring slot of their own (uploaded, or restored from the list), edgehip_minimizer_rv_kf with search_range = field_radius, the
links read back from the query slot — and everything around the minimisation (the request, optimizeScale, the returned pose) through
tests/keyframe_reloc_port.py.

Tolerances: the project's own for this minimiser.  mnum, m_id_f, evals, accepted exact; X, Pose rtol 1e-9 + atol 1e-12; Pos the same,
relative to the larger of |Pos_t| and |BRelPos K|; score_ratio, Kp, K 1e-9 relative; RRV 1e-7 relative.

Inputs: the key frames of tests/golden/keyframe_covis/ — `chained`, five consecutive frames of a rendered sequence (256 x 192, ~1900
KeyLines: a frame really is re-localised against the four before it), and `crafted` (70 x 50; lists of 0, 1, 65, 257 and 600 KeyLines:
no KeyLines, less than a wave, more than a 256-KeyLine tile, an odd list)."""
import ctypes as C
import os

import numpy as np
import pytest

import keyframe_covis_port as cport
import keyframe_reloc_port as port
from rebvo_amd import edgehip

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_covis")
ANG = 30.0 * np.pi / 180.0
INTS = ("mnum", "evals", "accepted", "guard")
_FX = {}


def fixture(name):
    if name not in _FX:
        f = cport.load_fixture(os.path.join(GOLD, name + ".npz"))
        f["rec"] = [cport.records(k, edgehip.KEYLINE_DTYPE) for k in f["kfs"]]
        _FX[name] = f
    return _FX[name]


# K != K_t and K_t != 1; key frame 1's Pose is not exactly orthonormal (SO3<>(Pose_t) coerces it)
K_OF = [1.1, 0.9, 1.2, 1.0, 1.05]


def pose_of(f, m):
    k = f["kfs"][m]
    P = np.array(k["Pose"], np.float64).reshape(3, 3).copy()
    if m == 1:
        P[0, 1] += 3e-7
        P[2, 2] *= 1 + 2e-7
    return P, np.array(k["Pos"], np.float64), K_OF[m] * float(k["K"])


def kf_pose(f, m):
    P, T, K = pose_of(f, m)
    return edgehip.EdgeHip.kf_pose(P, T, t=0.1 * m, K=K)


def context(f, nseq, capacity, radius, track=True):
    cam = f["cam"]
    mp = max(len(r) for r in f["rec"]) + 3
    p = edgehip.euroc_params(int(cam["w"]), int(cam["h"]), ppx=float(cam["ppx"]), ppy=float(cam["ppy"]), zfx=float(cam["zfx"]),
                             zfy=float(cam["zfy"]), max_points=mp, search_range=radius)
    eh = edgehip.EdgeHip(p, nseq=nseq, nslots=2, device=0)
    if track:
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        if capacity:
            eh.keyframe_list_enable(capacity)
    return eh


def seed(eh, f, orders):
    for s, order in enumerate(orders):
        for m in order:
            eh.upload_keyframe(s, f["rec"][m], kf_pose(f, m))


def positions(orders, capacity):
    return [list(o[-(capacity + 1):]) for o in orders]


def snapshot(eh):
    """Every key frame, list entry and ring slot, as bytes."""
    info = eh.keyframe_list_info()
    out = [info.tobytes()]
    for s in range(eh.nseq):
        kl, pose, count = eh.download_keyframe(s)
        out += [kl.tobytes(), bytes(pose), count]
        for j in range(info["first"][s], info["first"][s] + info["held"][s]):
            e = eh.download_keyframe_list(s, int(j))
            out += [e[0].tobytes(), bytes(e[1])]
        for slot in range(2):
            kl, mask = eh.download_keylines(s, slot)
            out += [kl.tobytes(), mask.tobytes()]
    return out


def close(got, want, rtol, atol=0.0, scale=None):
    """Within the tolerance where `want` is finite; the same NaN or infinity where it is not (a pair without a match has JtJ = 0: its RRV)."""
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    fin = np.isfinite(want)
    if not np.array_equal(np.isfinite(got), fin) or not np.array_equal(got[~fin], want[~fin], equal_nan=True):
        return False
    ref = np.abs(want) if scale is None else np.broadcast_to(scale, want.shape)
    return bool(np.all(np.abs(got[fin] - want[fin]) <= atol + rtol * ref[fin]))


def check_pair(tag, got, links, f, q, m, s_rho_q, route, route_links):
    """got: one edgehip_kf_reloc record of the query (fixture key frame q) against key frame m; route: edgehip_minimizer_rv_kf's result for the
    same pair (one sequence's values), route_links the m_id_f it left."""
    qp, kp = pose_of(f, q), pose_of(f, m)
    assert np.array_equal(links, route_links), tag
    assert int(got["mnum"]) == int(route["mnum"]) == int((route_links >= 0).sum()), tag
    assert int(got["evals"]) == int(route["evals"]), tag
    assert int(got["guard"]) == 0, tag
    X = np.array(got["X"])
    assert close(X, route["X"], 1e-9, 1e-12), (tag, X, route["X"])
    assert close(got["score_ratio"], route["score_ratio"], 1e-9) and close(got["F"], route["F"], 1e-9) and close(got["F0"], route["F0"], 1e-9), tag
    assert close(np.array(got["RRV"]).reshape(6, 6), route["RRV"], 1e-7), tag
    w = port.relocalize_around(f["kfs"][q], qp, f["kfs"][m], kp, f["cam"]["zfm"], X, links)
    assert close(got["Kp"], w["Kp"], 1e-9), (tag, got["Kp"], w["Kp"])
    assert close(got["K"], w["K"], 1e-9), tag
    assert close(np.array(got["Pose"]).reshape(3, 3), w["Pose"], 1e-9, 1e-12), tag
    scale = max(np.linalg.norm(kp[1]), np.linalg.norm(X[:3]) * w["K"])
    assert close(got["Pos"], w["Pos"], 1e-9, 1e-12, scale=scale), (tag, got["Pos"], w["Pos"])
    return w


def route_pair(eh, f, q, m, s_rho_q, a, seq=0, restore_ordinal=None):
    """The parent route for one pair in sequence `seq`: slot 1 <- key frame m (uploaded, or restored from the list), slot 0 the query."""
    if restore_ordinal is None:
        eh.upload_keylines(seq, 1, f["rec"][m])
    else:
        o = np.full(eh.nseq, -1, np.int32)
        o[seq] = restore_ordinal
        eh.keyframe_list_restore(1, o)
    X0, Kr = port.request(*pose_of(f, q), *pose_of(f, m))
    r = eh.minimizer_rv_kf(1, 0, X0, Kr, s_rho_q, 5.0, ANG, a["rho_tol"], a["iter_max"], a["rew_dis"], 0)
    kl, _ = eh.download_keylines(seq, 0)
    one = {k: v[seq] for k, v in r.items()}
    return one, kl["m_id_f"].copy(), X0


ARGS_CHAINED = dict(field_radius=40, iter_max=6, rew_dis=2.0, rho_tol=3.0)
ARGS_CRAFTED = dict(field_radius=5, iter_max=6, rew_dis=2.0, rho_tol=1.5)


@pytest.mark.parametrize("iter_max", [6, 0])
def test_chained_every_pair_against_the_parent_route_and_the_port(iter_max):
    """Capacity 3 (M = 4), nseq 3: a full list with the current key frame as the last position; one key frame alone; no key frame."""
    f = fixture("chained")
    a = dict(ARGS_CHAINED, iter_max=iter_max)
    q = 4
    s_rho_q = float(np.quantile(f["kfs"][q]["s_rho"], 0.9))
    eh = context(f, 3, 3, a["field_radius"])
    try:
        orders = [[0, 1, 2, 3], [2], []]
        seed(eh, f, orders)
        for s in range(3):
            eh.upload_keylines(s, 0, f["rec"][q])
        poses = [kf_pose(f, q)] * 3
        before = snapshot(eh)
        got, info = eh.keyframe_relocalize(0, s_rho_q, poses=poses, **a)
        assert got.shape == (3, 4)
        assert snapshot(eh) == before
        assert np.array_equal(info, eh.keyframe_list_info())
        again, _ = eh.keyframe_relocalize(0, s_rho_q, poses=poses, **a)
        assert again.tobytes() == got.tobytes()
        links = {(s, t): eh.keyframe_relocalize_links(s, t) for s in range(3) for t in range(4)}
        prep, solve = eh.keyframe_relocalize_ms()
        assert prep > 0 and solve > 0
        pos = positions(orders, 3)
        accepted = 0
        for s, p in enumerate(pos):
            for t in range(4):
                if t >= len(p):
                    assert all(int(got[n][s, t]) == -1 for n in INTS) and links[s, t] is None, (s, t)
                    assert not np.array(got["X"][s, t]).any() and got["Kp"][s, t] == 0
                    continue
                route, rl, _ = route_pair(eh, f, q, p[t], s_rho_q, a, seq=s)
                w = check_pair((s, t), got[s, t], links[s, t], f, q, p[t], s_rho_q, route, rl)
                assert w["mnum"] >= 30 and w["used"] > 0 and w["Kp"] != 1.0, (s, t, w["mnum"])
                assert 0 <= got["accepted"][s, t] <= iter_max and got["evals"][s, t] == iter_max + 1
                accepted += int(got["accepted"][s, t])
        assert got[0, 2].tobytes() == got[1, 0].tobytes()        # key frame 2 from the list and as a current key frame: the same bits
        if iter_max:
            assert accepted > 0
    finally:
        eh.close()


def test_restored_list_entry_is_the_same_pair():
    """The route the issue names: edgehip_keyframe_list_restore + edgehip_minimizer_rv_kf with field_radius = search_range, field_min_mod = -1."""
    f = fixture("chained")
    a = dict(ARGS_CHAINED)
    q = 3
    s_rho_q = 1e3
    eh = context(f, 2, 2, a["field_radius"])
    try:
        seed(eh, f, [[0, 1, 2], [1]])
        for s in range(2):
            eh.upload_keylines(s, 0, f["rec"][q])
        got, info = eh.keyframe_relocalize(0, s_rho_q, poses=[kf_pose(f, q)] * 2, field_min_mod=-1.0, **a)
        lk = eh.keyframe_relocalize_links(0, 1)
        route, rl, _ = route_pair(eh, f, q, 1, s_rho_q, a, seq=0, restore_ordinal=int(info["first"][0]) + 1)
        check_pair("restored", got[0, 1], lk, f, q, 1, s_rho_q, route, rl)
        assert int(got["mnum"][0, 1]) >= 30
    finally:
        eh.close()


def run_crafted(nseq, capacity, orders, queries, to_mask=None, a=ARGS_CRAFTED, s_rho_q=1e3):
    """queries[seq]: the fixture key frame whose KeyLines and pose are the query of that sequence, or None for an empty slot."""
    f = fixture("crafted")
    eh = context(f, nseq, capacity, a["field_radius"])
    try:
        seed(eh, f, orders)
        for s, q in enumerate(queries):
            if q is not None:                                # (a fresh context's slot holds no KeyLines)
                eh.upload_keylines(s, 0, f["rec"][q])
        poses = [kf_pose(f, 4 if q is None else q) for q in queries]
        before = snapshot(eh)
        got, info = eh.keyframe_relocalize(0, s_rho_q, poses=poses, to_mask=to_mask, **a)
        assert snapshot(eh) == before
        links = {(s, t): eh.keyframe_relocalize_links(s, t) for s in range(nseq) for t in range(capacity + 1)}
        return got, links, info
    finally:
        eh.close()


ORDERS7 = [[0, 1, 2, 3, 4], [], [4], [1, 2, 3], [4, 3, 2, 1, 0], [3, 3], [2, 4, 0, 1]]
QUERY7 = [4, 3, 3, 4, None, 4, 3]


@pytest.mark.parametrize("nseq", [3, 7])
def test_crafted_ragged_batch_capacity_3(nseq):
    """M = 4: one pass.  A sequence without key frames, one with an empty query, lists of 0, 1, 65, 257 and 600 KeyLines as key frames; every
    served pair against the parent route and the port; absent positions all -1."""
    f = fixture("crafted")
    orders, queries = ORDERS7[:nseq], QUERY7[:nseq]
    if nseq == 3:
        queries = [4, 3, None]
    got, links, info = run_crafted(nseq, 3, orders, queries)
    pos = positions(orders, 3)
    a = ARGS_CRAFTED
    eh = context(f, 1, 0, a["field_radius"])
    try:
        served = matched = 0
        for s, p in enumerate(pos):
            for t in range(4):
                if t >= len(p):
                    assert all(int(got[n][s, t]) == -1 for n in INTS) and links[s, t] is None, (s, t)
                    continue
                served += 1
                if queries[s] is None:
                    w = port.empty_query(pose_of(f, 4), pose_of(f, p[t]))
                    g = got[s, t]
                    assert [int(g[n]) for n in INTS] == [0, 0, 0, 0] and len(links[s, t]) == 0
                    assert g["score_ratio"] == 0 and g["Kp"] == 1 and not np.array(g["RRV"]).any()
                    assert close(g["X"], w["X"], 1e-9, 1e-12) and close(g["K"], w["K"], 1e-9)
                    assert close(np.array(g["Pose"]).reshape(3, 3), w["Pose"], 1e-9, 1e-12)
                    assert close(g["Pos"], w["Pos"], 1e-9, 1e-12, scale=max(np.linalg.norm(pose_of(f, p[t])[1]), np.linalg.norm(w["X"][:3]) * w["K"]))
                    continue
                eh.upload_keylines(0, 0, f["rec"][queries[s]])
                route, rl, _ = route_pair(eh, f, queries[s], p[t], 1e3, a)
                w = check_pair((s, t), got[s, t], links[s, t], f, queries[s], p[t], 1e3, route, rl)
                matched += w["mnum"]
                if w["mnum"] == 0 or w["used"] == 0:
                    assert got["Kp"][s, t] == 1.0            # optimizeScale's fallback
        assert served == sum(len(p) for p in pos) and matched > 0
    finally:
        eh.close()


def test_second_pass_masks_and_bit_identity():
    """Capacity 9 (M = 10 > P = 8: two passes).  The same (query, key frame) pair gives the same bits alone in a batch of one, at two places of a
    batch of five, in the first and in the second pass, and with a to_mask that deselects every other position; deselected positions are -1."""
    order = [0, 1, 2, 3, 4, 4, 3, 2, 1, 3]                   # positions 0 .. 9; key frame 3 at positions 3, 6 and 9 (the current one)
    got1, links1, _ = run_crafted(1, 9, [order], [4])
    assert got1.shape == (1, 10) and (got1["mnum"] >= 0).all()
    for t in (6, 9):
        assert got1[0, t].tobytes() == got1[0, 3].tobytes() and np.array_equal(links1[0, t], links1[0, 3])
    assert got1["mnum"][0, 4] > 0                            # the query against itself as a key frame
    assert got1[0, 5].tobytes() == got1[0, 4].tobytes()
    orders = [[2], order, [], order[2:], order]
    got5, links5, _ = run_crafted(5, 9, orders, [3, 4, 4, 4, 4])
    assert got5[1].tobytes() == got1[0].tobytes() and got5[4].tobytes() == got1[0].tobytes()
    assert got5[3, :8].tobytes() == got1[0, 2:].tobytes()     # the same pairs, served at other positions
    assert (got5["mnum"][2] == -1).all() and (got5["mnum"][0, 1:] == -1).all()
    for t in range(10):
        assert np.array_equal(links5[4, t], links1[0, t])
    mask = np.zeros((5, 10), np.uint8)
    mask[1, [3, 8]] = 1
    mask[4, 9] = 1
    mask[2, :] = 1                                            # selects positions the sequence does not have
    gotm, linksm, _ = run_crafted(5, 9, orders, [3, 4, 4, 4, 4], to_mask=mask)
    for s in range(5):
        for t in range(10):
            if mask[s, t] and s != 2:
                assert gotm[s, t].tobytes() == got5[s, t].tobytes() and np.array_equal(linksm[s, t], links5[s, t]), (s, t)
            else:
                assert all(int(gotm[n][s, t]) == -1 for n in INTS) and linksm[s, t] is None, (s, t)


def test_non_finite_rho_is_counted_and_the_call_returns():
    f = fixture("crafted")
    a = ARGS_CRAFTED
    eh = context(f, 2, 1, a["field_radius"])
    try:
        seed(eh, f, [[3, 4], [4]])
        rec = f["rec"][4].copy()
        rec["rho"][[5, 300]] = np.nan
        eh.upload_keylines(0, 0, rec)
        eh.upload_keylines(1, 0, f["rec"][4])
        bad = kf_pose(f, 4)
        bad.Pose[4] = float("nan")
        got, _ = eh.keyframe_relocalize(0, 1e3, poses=[kf_pose(f, 4), bad], **a)
        assert list(got["guard"][0]) == [2, 2]
        assert got["guard"][1, 0] >= 1 and got["guard"][1, 1] == -1
        ok, _ = eh.keyframe_relocalize(0, 1e3, poses=[kf_pose(f, 4), kf_pose(f, 4)], **a)      # the context stays usable
        assert ok["guard"][1, 0] == 0 and ok["mnum"][1, 0] > 0
    finally:
        eh.close()


def test_scratch_survives_reset_and_a_list_re_enable():
    f = fixture("crafted")
    a = ARGS_CRAFTED
    eh = context(f, 2, 0, a["field_radius"])
    try:
        seed(eh, f, [[4], []])
        for s in range(2):
            eh.upload_keylines(s, 0, f["rec"][4])
        poses = [kf_pose(f, 4)] * 2
        g0, _ = eh.keyframe_relocalize(0, 1e3, poses=poses, **a)       # M = 1: the current key frames alone
        assert g0.shape == (2, 1) and g0["mnum"][0, 0] > 0 and g0["mnum"][1, 0] == -1
        eh.keyframe_list_enable(2)
        seed(eh, f, [[3], [4]])
        g1, info = eh.keyframe_relocalize(0, 1e3, poses=poses, **a)
        assert g1.shape == (2, 3) and list(info["held"]) == [1, 0]
        assert g1[0, 0].tobytes() == g0[0, 0].tobytes() and g1[1, 0].tobytes() == g0[0, 0].tobytes()
        assert g1["mnum"][0, 2] == -1 and (g1["mnum"][1, 1:] == -1).all() and g1["mnum"][0, 1] >= 0
        eh.reset()
        g2, info = eh.keyframe_relocalize(0, 1e3, poses=poses, **a)
        assert all((g2[n] == -1).all() for n in INTS) and not info["kf_count"].any()
        seed(eh, f, [[4], []])
        for s in range(2):
            eh.upload_keylines(s, 0, f["rec"][4])
        g3, _ = eh.keyframe_relocalize(0, 1e3, poses=poses, **a)
        assert g3[0, 0].tobytes() == g0[0, 0].tobytes()
    finally:
        eh.close()


def test_error_returns():
    f = fixture("crafted")
    eh = context(f, 3, 0, 5, track=False)
    try:
        a = edgehip.KfRelocArgs(5, 0.0, 3, 2.0, 1.5)
        out = np.zeros((3, 1), edgehip.KF_RELOC_DTYPE)
        po = out.ctypes.data_as(C.c_void_p)
        q = np.full(3, 1e3)
        pq = q.ctypes.data_as(C.c_void_p)
        lib = eh.lib
        kn = C.c_int32(0)
        assert lib.edgehip_keyframe_relocalize(eh.ctx, 0, None, pq, None, C.byref(a), po, None) == -4          # EDGEHIP_ERR_STATE
        assert lib.edgehip_keyframe_relocalize_links(eh.ctx, 0, 0, None, C.byref(kn)) == -4
        assert lib.edgehip_keyframe_relocalize_ms(eh.ctx, None, None) == -4
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        assert lib.edgehip_keyframe_relocalize_links(eh.ctx, 0, 0, None, C.byref(kn)) == -4                    # no call yet
        assert lib.edgehip_keyframe_relocalize(eh.ctx, 0, None, pq, None, None, po, None) == -1                # EDGEHIP_ERR_ARG
        assert lib.edgehip_keyframe_relocalize(eh.ctx, 0, None, pq, None, C.byref(a), None, None) == -1
        assert lib.edgehip_keyframe_relocalize(eh.ctx, 0, None, None, None, C.byref(a), po, None) == -1
        for radius in (0, -3, 256):                                                                          # what build_field refuses
            bad = edgehip.KfRelocArgs(radius, 0.0, 3, 2.0, 1.5)
            assert lib.edgehip_keyframe_relocalize(eh.ctx, 0, None, pq, None, C.byref(bad), po, None) == -1, radius
        bad = edgehip.KfRelocArgs(5, 0.0, -1, 2.0, 1.5)
        assert lib.edgehip_keyframe_relocalize(eh.ctx, 0, None, pq, None, C.byref(bad), po, None) == -1
        for slot in (-1, 2):
            assert lib.edgehip_keyframe_relocalize(eh.ctx, slot, None, pq, None, C.byref(a), po, None) == -1, slot
        assert lib.edgehip_keyframe_relocalize(eh.ctx, 0, None, pq, None, C.byref(a), po, None) == 0           # the context stays usable
        assert all((out[n] == -1).all() for n in INTS)
        assert lib.edgehip_keyframe_relocalize_links(eh.ctx, 0, 0, None, C.byref(kn)) == 0 and kn.value == -1
        assert lib.edgehip_keyframe_relocalize_links(eh.ctx, 3, 0, None, C.byref(kn)) == -1
        assert lib.edgehip_keyframe_relocalize_links(eh.ctx, 0, 1, None, C.byref(kn)) == -1
        big = edgehip.KfRelocArgs(255, 0.0, 2, 2.0, 1.5)                                                      # the largest radius
        seed(eh, f, [[3], [], [4]])
        for s in range(3):
            eh.upload_keylines(s, 0, f["rec"][4])
        assert lib.edgehip_keyframe_relocalize(eh.ctx, 0, None, pq, None, C.byref(big), po, None) == 0
        assert out["mnum"][0, 0] >= 0 and out["mnum"][1, 0] == -1 and out["evals"][2, 0] == 3
    finally:
        eh.close()
