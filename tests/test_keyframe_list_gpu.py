"""The key-frame list (REBVO::kf_list) on the device: a retired key frame equals what edgehip_download_keyframe returned for it at that
moment, byte for byte and through every place that replaces a key frame; the ring; the way back into a ring slot; the frame driver
against a context stepped through the stage-level entry points; the run-time save flag; and the key-frame file written from the list.
Device against device and bytes against bytes: no tolerance anywhere."""
import os

import numpy as np
import pytest

from rebvo_amd import edgehip, synth

pytestmark = pytest.mark.gpu

T = 256          # k_kf_retire's tile (kKlTile, keyframe_list.hip): records per workgroup
NSEQ = 7


def rand_records(rs, n, w=64, h=48):
    """n 168-byte records with every field random (valid for the depth fill: c_p inside the image, positive rho / s_rho, m_num on both
    sides of its threshold); the fields the device does not keep hold what a download gives them."""
    kl = np.zeros(n, edgehip.KEYLINE_DTYPE)
    for f in ("m_m", "u_m", "p_m", "p_m_0", "m_m0"):
        kl[f] = rs.uniform(-100, 100, (n, 2)).astype(np.float32)
    kl["c_p"] = (rs.uniform(0, 1, (n, 2)) * [w - 1, h - 1]).astype(np.float32)
    for f in ("rho", "s_rho", "rho_nr", "s_rho_nr", "rho0", "s_rho0", "n_m0"):
        kl[f] = rs.uniform(0.01, 5, n)
    kl["n_m"] = rs.uniform(0, 50, n).astype(np.float32)
    kl["p_inx"], kl["m_num"] = rs.randint(0, w * h, n), rs.randint(0, 12, n)
    for f in ("m_id", "m_id_f", "m_id_kf", "p_id", "n_id"):
        kl[f] = rs.randint(-1, max(n, 1), n)
    kl["net_id"], kl["stereo_m_id"], kl["stereo_rho"], kl["stereo_s_rho"] = -1, -1, 1.0, 20.0
    return kl


def rand_pose(rs):
    q = edgehip.KfPose()
    q.t, q.K = rs.uniform(0, 100), rs.uniform(0.5, 2)
    for f, n in (("Rot", 9), ("RotLie", 3), ("Vel", 3), ("Pose", 9), ("PoseLie", 3), ("Pos", 3)):
        getattr(q, f)[:] = list(rs.uniform(-3, 3, n))
    return q


def snapshot(eh):
    """The current key frames, the lists' info and every held entry."""
    info = eh.keyframe_list_info()
    held = {(s, j): eh.download_keyframe_list(s, j) for s in range(eh.nseq) for j in range(info["first"][s], info["first"][s] + info["held"][s])}
    return dict(cur=[eh.download_keyframe(s) for s in range(eh.nseq)], info=info, held=held)


def same_entry(a, b):
    return a[0].tobytes() == b[0].tobytes() and bytes(a[1]) == bytes(b[1])


def check_retired(before, after, retired):
    """Sequences of `retired` gained exactly one entry, equal to the key frame downloaded before; nothing else in any list moved."""
    for s in range(len(before["cur"])):
        bi, ai = before["info"][s], after["info"][s]
        if not retired[s] or before["cur"][s][2] == 0:   # (a sequence without a key frame has nothing to retire)
            assert (ai["first"], ai["held"], ai["overwritten"]) == (bi["first"], bi["held"], bi["overwritten"]), s
            assert ai["kf_count"] == bi["kf_count"] + (1 if retired[s] else 0), s
            continue
        kl, pose, count = before["cur"][s]
        assert ai["kf_count"] == count + 1 and ai["first"] == bi["first"] and ai["held"] == bi["held"] + 1 and ai["overwritten"] == bi["overwritten"], s
        assert ai["first"] + ai["held"] == ai["kf_count"] - 1, s
        got = after["held"][(s, count - 1)]          # its ordinal: it was the count-th key frame
        assert len(got[0]) == len(kl), (s, len(got[0]), len(kl))
        assert got[0].tobytes() == kl.tobytes(), s   # byte for byte, the padding included
        assert bytes(got[1]) == bytes(pose), s
    for key, e in before["held"].items():
        assert same_entry(after["held"][key], e), key


@pytest.mark.parametrize("max_points", [777, 20000])
def test_retired_key_frame_equals_its_download(max_points):
    """kn of 0, 1, 2, 3, T-1, T, T+1, 2T+1 and max_points (an odd kn ends in half a 16-byte word; an odd max_points makes the entries'
    natural stride no multiple of 16), every one of them retired through edgehip_upload_keyframe and through edgehip_keyframe_insert with
    a mask and compared with its download: the set of (path, kn) pairs that were compared is asserted."""
    rs = np.random.RandomState(max_points)
    eh = edgehip.EdgeHip(edgehip.euroc_params(64, 48, zfx=420.0, zfy=420.0, max_points=max_points), nseq=NSEQ, nslots=2, device=0)
    try:
        assert eh.cap == max_points
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        eh.keyframe_list_enable(8)
        kns = [0, 1, 2, 3, T - 1, T, T + 1, 2 * T + 1, max_points]
        mp = max_points
        # (what, kn per sequence, the sequence that is left out of an insertion): uploads replace every sequence's key frame one by one,
        # insertions replace the key frames of all sequences but one from slot lists of these lengths.  Which kn retires where:
        #   upload 1: nothing (no key frame yet)         insert 1: 0, 1, 2, 255, 256, 257 (sequence 3 keeps its 3)
        #   upload 2: 513, mp, 0, 3, 2, 3, 255           insert 2: 513, mp, 257, 256, 1, 2 (sequence 0 keeps its 3)
        #   upload 3: 3, 1, 2, 256, 257, 513, mp         insert 3: 3, 0, 1, 2, 255, 256 (sequence 6 keeps its 257)
        schedule = [("upload", [0, 1, 2, 3, T - 1, T, T + 1], None), ("insert", [2 * T + 1, mp, 0, 1, 2, 3, T - 1], 3),
                    ("upload", [3, 2 * T + 1, mp, T + 1, T, 1, 2], None), ("insert", [0, 1, 2, T, T + 1, 2 * T + 1, mp], 0),
                    ("upload", [3, 0, 1, 2, T - 1, T, T + 1], None), ("insert", [5, 4, 3, 2, 1, 0, 7], 6)]
        compared = set()                                 # (path, kn) of every retired entry that was compared with its download
        first = snapshot(eh)
        assert not first["held"] and not first["info"]["kf_count"].any()
        for what, kn_r, left_out in schedule:
            if what == "upload":                         # one sequence at a time: it retires what the sequence had
                for s in range(NSEQ):
                    before = snapshot(eh)
                    eh.upload_keyframe(s, rand_records(rs, kn_r[s]), rand_pose(rs))
                    check_retired(before, snapshot(eh), [q == s for q in range(NSEQ)])
                    if before["cur"][s][2] > 0:
                        compared.add(("upload", len(before["cur"][s][0])))
            else:                                        # from a slot with other ragged lists, masked
                for s in range(NSEQ):
                    eh.upload_keylines(s, 1, rand_records(rs, kn_r[s]))
                mask = np.array([s != left_out for s in range(NSEQ)])
                before = snapshot(eh)
                eh.keyframe_insert(1, mask, [rand_pose(rs) for _ in range(NSEQ)])
                check_retired(before, snapshot(eh), mask)
                compared |= {("insert", len(before["cur"][s][0])) for s in range(NSEQ) if mask[s]}
        assert compared == {(path, kn) for path in ("upload", "insert") for kn in kns}, sorted(compared)
        info = eh.keyframe_list_info()
        assert (info["overwritten"] == 0).all() and (info["held"] >= 3).all()
        # edgehip_reset empties the list with the key frame
        eh.reset()
        info = eh.keyframe_list_info()
        assert not info["kf_count"].any() and not info["held"].any() and not info["first"].any() and not info["overwritten"].any()
    finally:
        eh.close()


def test_ring_overwrites_the_oldest_and_refuses_what_it_does_not_hold():
    rs = np.random.RandomState(3)
    eh = edgehip.EdgeHip(edgehip.euroc_params(64, 48, zfx=420.0, zfy=420.0, max_points=777), nseq=NSEQ, nslots=2, device=0)
    try:
        with pytest.raises(edgehip.EdgeHipError):     # needs tracking
            eh.keyframe_list_enable(2)
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        eh.keyframe_list_enable(2)
        taken = [[] for _ in range(NSEQ)]             # every key frame a sequence took, by ordinal
        for k in range(5):                            # the first insertion makes ordinal 0, four more retire ordinals 0..3
            for s in range(NSEQ):
                eh.upload_keylines(s, 0, rand_records(rs, 5 + 2 * s + k))
            eh.keyframe_insert(0, None, [rand_pose(rs) for _ in range(NSEQ)])
            for s in range(NSEQ):
                taken[s].append(eh.download_keyframe(s))
        info = eh.keyframe_list_info()
        assert (info["kf_count"] == 5).all() and (info["first"] == 2).all() and (info["held"] == 2).all() and (info["overwritten"] == 2).all()
        for s in range(NSEQ):
            for j in (2, 3):
                got = eh.download_keyframe_list(s, j)
                assert got[0].tobytes() == taken[s][j][0].tobytes() and bytes(got[1]) == bytes(taken[s][j][1]), (s, j)
        both = eh.download_keyframe_list([1, 4, 4], [3, 2, 3])   # the batch form
        for (s, j), got in zip([(1, 3), (4, 2), (4, 3)], both):
            assert got[0].tobytes() == taken[s][j][0].tobytes() and bytes(got[1]) == bytes(taken[s][j][1]), (s, j)
        # overwritten (0, 1), current (4) and future (5) ordinals: refused, and nothing changes
        for s in range(NSEQ):
            eh.upload_keylines(s, 1, rand_records(rs, 9 + s))
        slot_before = [eh.download_keylines(s, 1, want_mask=True) for s in range(NSEQ)]
        for bad in (0, 1, 4, 5, -2):
            with pytest.raises(edgehip.EdgeHipError):
                eh.download_keyframe_list(2, bad)
            with pytest.raises(edgehip.EdgeHipError):
                eh.keyframe_list_restore(1, [2, 3, bad, -1, 2, 3, 2])
        for s in range(NSEQ):
            kl, m = eh.download_keylines(s, 1, want_mask=True)
            assert kl.tobytes() == slot_before[s][0].tobytes() and np.array_equal(m, slot_before[s][1])
        after = eh.keyframe_list_info()
        assert after.tobytes() == info.tobytes()
        # capacity 0 frees the list alone: tracking goes on
        eh.keyframe_list_enable(0)
        with pytest.raises(edgehip.EdgeHipError):
            eh.keyframe_list_info()
        assert eh.download_keyframe(0)[2] == 5
    finally:
        eh.close()


def test_restore_leaves_the_slot_as_an_upload_of_the_same_records():
    """Context A restores list entries into a slot, context B gets the same records through edgehip_upload_keylines: the slots are
    equal byte for byte (mask plane included), sequences given -1 keep theirs, and the depth fill of both slots is the same grid."""
    rs = np.random.RandomState(17)
    p = edgehip.euroc_params(64, 48, zfx=420.0, zfy=420.0, max_points=777)
    A, B = (edgehip.EdgeHip(p, nseq=NSEQ, nslots=2, device=0) for _ in range(2))
    try:
        A.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        A.keyframe_list_enable(3)
        kns = [0, 1, T - 1, T, T + 1, 2 * T + 1, 777]   # an exact tile, one less, one more; 777: the last 16-byte load of the odd,
                                                        # full entry reaches into the stride's padding
        entries = [[], []]
        for j in range(3):                              # three key frames per sequence: ordinals 0 and 1 retire
            for s in range(NSEQ):
                kl, pose = rand_records(rs, kns[(s + j) % NSEQ]), rand_pose(rs)
                A.upload_keyframe(s, kl, pose)
                if j < 2:
                    entries[j].append(kl)
        now = [rand_records(rs, 40 + s) for s in range(NSEQ)]    # what the slot holds
        masks = rs.randint(-1, 5, (NSEQ, 48, 64)).astype(np.int32)
        for eh in (A, B):
            eh.depth_fill_enable(block=8, iter_num=5, thresh_rel_rho=0.5, thresh_match_num=5, bound_mode=0, discard=1)
            for s in range(NSEQ):
                eh.upload_keylines(s, 1, now[s], mask=masks[s], retuned=0.25)
        restored = set()
        for ordinals in ([0, -1, 0, 0, 0, 0, 0], [1, 1, -1, -1, 1, -1, 1]):
            A.keyframe_list_restore(1, ordinals)
            for s in range(NSEQ):
                if ordinals[s] >= 0:
                    now[s] = entries[ordinals[s]][s]
                    restored.add(len(now[s]))
                    B.upload_keylines(s, 1, now[s], None, 0.0)
            for s in range(NSEQ):
                ka, ma = A.download_keylines(s, 1, want_mask=True)
                kb, mb = B.download_keylines(s, 1, want_mask=True)
                assert len(ka) == len(now[s]) and ka.tobytes() == now[s].tobytes(), (s, ordinals[s])   # sequences given -1 keep theirs
                assert ka.tobytes() == kb.tobytes() and np.array_equal(ma, mb) and np.array_equal(ma, masks[s]), s
        assert restored == set(kns), restored           # every size above went through k_kf_restore
        for eh in (A, B):
            eh.depth_fill(1)
        for s in range(NSEQ):
            ga, gb = A.download_depth_grid(s), B.download_depth_grid(s)
            for x, y in zip(ga, gb):
                assert x.tobytes() == y.tobytes(), s
        assert any(A.download_depth_grid(s)[2].any() for s in range(NSEQ))   # (the fill had something to fix)
    finally:
        A.close(); B.close()


def same_bits(a, b):
    """Bit for bit, except that a NaN the arithmetic creates equals any NaN (include/edgehip.h, the depth fill: the GPU's default NaN is
    positive, x86 SSE's negative)."""
    return ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all()


def test_depth_fill_of_a_restored_entry_equals_the_reference_fill_of_the_file():
    """File -> the reference's loadKeyframesFromFile -> its initDepthFiller (tests/golden/keyframe_file, made by
    tools/make_keyframe_file_golden.py) against upload -> list -> restore -> edgehip_depth_fill, for the fixture's three key frames."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_file", "crafted.npz"))
    n = int(z["n"])
    p = edgehip.euroc_params(int(z["w"]), int(z["h"]), zfx=float(z["zfx"]), zfy=float(z["zfy"]), max_points=777)
    eh = edgehip.EdgeHip(p, nseq=n, nslots=2, device=0)
    try:
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        eh.keyframe_list_enable(2)
        eh.depth_fill_enable(block=int(z["fill_bw"]), block_h=int(z["fill_bh"]), iter_num=int(z["fill_iter_num"]),
                             thresh_rel_rho=float(z["fill_thresh_rel_rho"]), thresh_match_num=int(z["fill_thresh_match_num"]), bound_mode=0,
                             discard=int(z["fill_discard"]))
        rs = np.random.RandomState(1)
        for s in range(n):
            kl = np.ascontiguousarray(z[f"kf{s}_kl"]).view(edgehip.KEYLINE_DTYPE).reshape(-1)
            eh.upload_keyframe(s, kl, edgehip.KfPose.from_buffer_copy(z[f"kf{s}_pose"].tobytes()))
        for s in range(n):
            eh.upload_keyframe(s, rand_records(rs, 3), rand_pose(rs))     # retires the fixture's key frames: ordinal 0
        eh.keyframe_list_restore(1, [0] * n)
        eh.depth_fill(1)
        for s in range(n):
            rho, s_rho, fixed = eh.download_depth_grid(s)
            assert np.array_equal(fixed, z[f"kf{s}_grid_fixed"].astype(bool)), s
            assert same_bits(rho, z[f"kf{s}_grid_rho"]) and same_bits(s_rho, z[f"kf{s}_grid_s_rho"]), s
    finally:
        eh.close()


# ---- the frame driver ---------------------------------------------------------------------------------------------------------------
W, H, NS, NFRAMES = 256, 192, 3, 7
KF_SAVE_PERCENT = 0.985   # as tests/test_keyframe_track_gpu.py: a second key frame after two to four frames


def nav_rows(eh):
    return np.frombuffer(b"".join(bytes(n) for n in eh.read_nav()), edgehip.NAV_DTYPE).copy()


def local_pose(Pose, R, Pos, V, K):
    """rebvo_second_t.cpp:435-436: Pose * R and Pos - Pose * R * V * K, every dot product accumulated in ascending index."""
    Pose, R, V = np.asarray(Pose, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3), np.asarray(V, np.float64)
    lp = np.array([[Pose[r, 0] * R[0, c] + Pose[r, 1] * R[1, c] + Pose[r, 2] * R[2, c] for c in range(3)] for r in range(3)])
    pos = np.array([Pos[i] - (lp[i, 0] * V[0] + lp[i, 1] * V[1] + lp[i, 2] * V[2]) * K for i in range(3)])
    return lp, pos


def drive(nframes, save_rule):
    """Three sequences through `nframes` frames and three contexts: A with tracking and the list inside edgehip_process_frame, B stepped
    through the stage-level entry points in the reference's order (its key frame downloaded immediately before each insertion), C with
    tracking in the frame driver and no list.  save_rule(k, inserted_so_far) -> REBVO::saveKeyframes for frame k, applied to A and C
    through edgehip_keyframe_set_save and to B's insertion rule."""
    p = edgehip.euroc_params(W, H)
    seqs = [list(f for f, _, _ in synth.billboard_sequence(W, H, nframes, seed=11 + s, traj_seed=13 + s)) for s in range(NS)]
    A, B, Cx = (edgehip.EdgeHip(p, nseq=NS, nslots=3, device=0) for _ in range(3))
    out = dict(recA=[], recB=[], recC=[], navA=[], navC=[], retiredB=[[] for _ in range(NS)], save=[], would=[], params=p)
    try:
        A.keyframe_track_enable(True, KF_SAVE_PERCENT, True)
        A.keyframe_list_enable(4)
        B.keyframe_track_enable(True, KF_SAVE_PERCENT, True, in_frame_driver=False)
        Cx.keyframe_track_enable(True, KF_SAVE_PERCENT, True)
        criterion_inserts = 0
        for k in range(nframes):
            save = bool(save_rule(k, criterion_inserts))
            A.keyframe_set_save(save); Cx.keyframe_set_save(save)
            frame = np.stack([seqs[s][k] for s in range(NS)])
            recB = np.zeros(NS, edgehip.KF_TRACK_DTYPE)
            would = np.zeros(NS, bool)
            if k == 1:   # rebvo_second_t.cpp:156-162: the first key frame is the old frame, K = 1, whatever the flag says
                poses = []
                for n in B.read_nav():
                    q = edgehip.KfPose()
                    q.t, q.K = n.t, 1.0
                    for f in ("Rot", "RotLie", "Vel", "Pose", "PoseLie", "Pos"):
                        getattr(q, f)[:] = getattr(n, f)[:]
                    poses.append(q)
                B.keyframe_insert(B.cur_slot(), None, poses)
                recB["inserted"] = 1
            prev = [B.get_state(s) for s in range(NS)]
            for eh in (A, B, Cx):
                eh.upload_rgb(eh.next_slot(), frame)
                eh.process_frame(0.05 * k)
            navB = nav_rows(B)
            sn = B.cur_slot()
            if k >= 1:
                st = [B.get_state(s) for s in range(NS)]
                loc = [local_pose(prev[s].Pose[:], st[s].R[:], prev[s].Pos[:], st[s].V[:], prev[s].K) for s in range(NS)]
                Pose, Pos = np.array([l[0] for l in loc]), np.array([l[1] for l in loc])
                recB["back_m0"] = navB["kf_matchs"]
                recB["fow_m0"] = B.keyframe_build_forward_match(sn)
                recB["fow_m"] = B.keyframe_forward_correct(sn, Pose, Pos, 10.0, 0.0, True)
                recB["back_m"] = B.keyframe_back_correct(sn, Pose, Pos, 10.0, 0.0, True)
                would = recB["back_m"] < np.minimum(p.track_points, navB["kn"]) * KF_SAVE_PERCENT
                ins = would & save
                if ins.any():
                    for s in np.flatnonzero(ins):
                        kl, pose, _ = B.download_keyframe(int(s))
                        out["retiredB"][s].append((kl, pose))
                    B.keyframe_insert(sn, ins, None)
                    criterion_inserts += 1
                recB["inserted"] |= ins
            got = B.read_keyframe_track()
            recB["kf_count"], recB["kf_kn"] = got["kf_count"], got["kf_kn"]
            out["recA"].append(A.read_keyframe_track()); out["recB"].append(recB); out["recC"].append(Cx.read_keyframe_track())
            out["navA"].append(nav_rows(A)); out["navC"].append(nav_rows(Cx))
            out["save"].append(save); out["would"].append(would)
        out["infoA"] = A.keyframe_list_info()
        out["listA"] = [[A.download_keyframe_list(s, j) for j in range(out["infoA"]["first"][s], out["infoA"]["first"][s] + out["infoA"]["held"][s])]
                        for s in range(NS)]
        out["curA"] = [A.download_keyframe(s) for s in range(NS)]
        out["curB"] = [B.download_keyframe(s) for s in range(NS)]
    finally:
        for eh in (A, B, Cx):
            eh.close()
    return out


@pytest.fixture(scope="module")
def driven():
    return drive(NFRAMES, lambda k, n: True)


def test_frame_driver_retires_what_the_stage_level_context_downloaded(driven):
    d = driven
    assert sum(len(r) for r in d["retiredB"]) >= 1   # at least one sequence retired a key frame
    for s in range(NS):
        info = d["infoA"][s]
        assert (info["first"], info["held"], info["overwritten"]) == (0, len(d["retiredB"][s]), 0), s
        assert info["kf_count"] == d["curB"][s][2] == len(d["retiredB"][s]) + 1, s
        for j, (got, want) in enumerate(zip(d["listA"][s], d["retiredB"][s])):
            assert got[0].tobytes() == want[0].tobytes() and bytes(got[1]) == bytes(want[1]), (s, j)
        (ka, pa, ca), (kb, pb, cb) = d["curA"][s], d["curB"][s]
        assert ka.tobytes() == kb.tobytes() and bytes(pa) == bytes(pb) and ca == cb, s


def test_the_list_changes_nothing_a_frame_computes(driven):
    d = driven
    for k in range(NFRAMES):
        assert d["recA"][k].tobytes() == d["recC"][k].tobytes(), k     # the track records, every field
        assert d["navA"][k].tobytes() == d["navC"][k].tobytes(), k     # the nav records, every field
        for f in ("fow_m0", "fow_m", "back_m0", "back_m", "inserted", "kf_count", "kf_kn"):
            assert np.array_equal(d["recA"][k][f], d["recB"][k][f]), (k, f)


def test_key_frame_file_from_the_device_list(driven, tmp_path):
    d = driven
    for s in range(NS):
        path = str(tmp_path / f"kf_{s}.kf")
        edgehip.write_keyframe_file(path, [(e[1], e[0]) for e in d["listA"][s]] + [(d["curA"][s][1], d["curA"][s][0])], d["params"])
        back = edgehip.read_keyframe_file(path)
        want = d["retiredB"][s] + [(d["curB"][s][0], d["curB"][s][1])]
        assert len(back) == len(want) >= 1
        cam = edgehip.keyframe_file_camera(d["params"])
        for kf, (kl, pose) in zip(back, want):
            assert kf["kl"].tobytes() == kl.tobytes() and bytes(kf["pose"]) == bytes(pose)
            assert kf["max_r"] == d["params"].search_range and kf["camera"].tobytes() == cam.tobytes()


def test_save_flag_stops_and_resumes_insertion():
    """saveKeyframes goes off after the first insertion by the criterion and on again three frames later: kf_count stops rising while the
    repair goes on and the criterion holds, then rises again; key frame and list survive both calls; every record equals the
    stage-level context driven by the same rule."""
    state = dict(off_at=None)

    def rule(k, n):
        if n >= 1 and state["off_at"] is None:
            state["off_at"] = k
        return state["off_at"] is None or k >= state["off_at"] + 3

    nframes = 12
    d = drive(nframes, rule)
    off = state["off_at"]
    assert off is not None and off + 3 < nframes
    for k in range(nframes):
        for f in ("fow_m0", "fow_m", "back_m0", "back_m", "inserted", "kf_count", "kf_kn"):
            assert np.array_equal(d["recA"][k][f], d["recB"][k][f]), (k, f, d["recA"][k][f], d["recB"][k][f])
        assert d["recA"][k].tobytes() == d["recC"][k].tobytes(), k
    counts = np.array([r["kf_count"] for r in d["recA"]])
    held = [k for k in range(off, off + 3)]
    assert all((counts[k] == counts[off - 1]).all() for k in held)                       # no insertion while the flag is off
    assert any(d["would"][k].any() for k in held)                                        # though the criterion asked for one
    assert all(int(d["recA"][k]["back_m"][s]) > 0 for k in held for s in range(NS))      # and the repair went on
    assert (counts[-1] > counts[off + 2]).any()                                          # insertion resumed
    for s in range(NS):                                                                  # the list kept every retired key frame
        assert len(d["listA"][s]) == len(d["retiredB"][s]) == d["infoA"]["held"][s]
        for got, want in zip(d["listA"][s], d["retiredB"][s]):
            assert got[0].tobytes() == want[0].tobytes() and bytes(got[1]) == bytes(want[1]), s
        assert d["curA"][s][0].tobytes() == d["curB"][s][0].tobytes() and bytes(d["curA"][s][1]) == bytes(d["curB"][s][1])
