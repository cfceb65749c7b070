"""Key-frame tracking (TrackKeyFrames) on the device: the stage-level entry points against the fixtures the reference's own kfvo.cpp
produced (every id and every count equal: integers, no tolerance), insertion and the two resets, and edgehip_process_frame with the feature
on against a second context stepped through the stage-level entry points (device against device: exact)."""
import os

import numpy as np
import pytest

import keyframe_track_port as port
from rebvo_amd import edgehip, synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_track")


def crafted():
    z = np.load(os.path.join(GOLD, "crafted.npz"))
    return {str(n): {k[len(f"{n}_"):]: z[k] for k in z.files if k.startswith(f"{n}_")} for n in z["names"]}


def records(rs, p_m, p_id, n_id, m_id=None, m_id_f=None, m_id_kf=None):
    """168-byte records around the fields the steps read: everything else random, so that an untouched field shows."""
    n = len(p_id)
    kl = np.zeros(n, edgehip.KEYLINE_DTYPE)
    for f in ("m_m", "u_m", "c_p", "p_m_0", "m_m0"):
        kl[f] = rs.uniform(-100, 100, (n, 2)).astype(np.float32)
    for f in ("rho", "s_rho", "rho_nr", "s_rho_nr", "rho0", "s_rho0", "n_m0"):
        kl[f] = rs.uniform(0.01, 5, n)
    kl["n_m"] = rs.uniform(0, 50, n).astype(np.float32)
    kl["p_inx"], kl["m_num"] = rs.randint(0, 10000, n), rs.randint(0, 20, n)
    kl["p_m"] = np.asarray(p_m, np.float32).reshape(-1, 2)
    kl["p_id"], kl["n_id"] = p_id, n_id
    kl["m_id"] = rs.randint(-1, 50, n) if m_id is None else m_id
    kl["m_id_f"] = rs.randint(-1, 50, n) if m_id_f is None else m_id_f
    kl["m_id_kf"] = rs.randint(-1, 50, n) if m_id_kf is None else m_id_kf
    kl["net_id"], kl["stereo_m_id"], kl["stereo_rho"], kl["stereo_s_rho"] = -1, -1, 1.0, 20.0   # what a download gives these
    return kl


def same_but(a, b, *fields):
    assert len(a) == len(b)
    for f in edgehip.KEYLINE_DTYPE.names:
        if f not in fields:
            assert a[f].tobytes() == b[f].tobytes(), f


def run_batch(eh, cases, names):
    """One ragged batch through the three stage-level entry points; every id and count against the reference's."""
    rs = np.random.RandomState(5)
    c0 = cases[names[0]]
    up_kf, up_new, Pose, Pos = [], [], [], []
    for s in range(eh.nseq):
        c = cases[names[s % len(names)]]
        kf = records(rs, c["kf_p_m"], c["kf_p_id"], c["kf_n_id"], m_id_f=c["kf_m_id_f"])
        new = records(rs, c["new_p_m"], c["new_p_id"], c["new_n_id"], m_id=c["new_m_id"], m_id_kf=c["new_m_id_kf"])
        eh.upload_keylines(s, 0, new)
        eh.upload_keyframe(s, kf, eh.kf_pose(c["kf_Pose"], c["kf_Pos"]))
        up_kf.append(kf); up_new.append(new); Pose.append(c["Pose"]); Pos.append(c["Pos"])
    args = dict(Pose=np.array(Pose), Pos=np.array(Pos), dist_thresh=float(c0["dist_thresh"]), dist_tolerance=float(c0["dist_tolerance"]),
                augmentate=bool(c0["augmentate"]))
    got = {}
    got["c0"] = eh.keyframe_build_forward_match(0)
    got["f0"] = [eh.download_keyframe(s)[0] for s in range(eh.nseq)]
    got["c1"] = eh.keyframe_forward_correct(0, **args)
    got["f1"] = [eh.download_keyframe(s)[0] for s in range(eh.nseq)]
    got["c2"] = eh.keyframe_back_correct(0, **args)
    got["b1"] = [eh.download_keylines(s, 0, want_mask=False)[0] for s in range(eh.nseq)]
    got["f2"] = [eh.download_keyframe(s)[0] for s in range(eh.nseq)]
    rec = eh.read_keyframe_track()
    for s in range(eh.nseq):
        name = names[s % len(names)]
        c = cases[name]
        assert np.array_equal(got["f0"][s]["m_id_f"], c["ref_m_id_f_0"]), name
        assert np.array_equal(got["f1"][s]["m_id_f"], c["ref_m_id_f_1"]), name
        assert np.array_equal(got["b1"][s]["m_id_kf"], c["ref_m_id_kf_1"]), name
        assert [got["c0"][s], got["c1"][s], got["c2"][s]] == [int(v) for v in c["ref_counts"]], name
        assert [rec["fow_m0"][s], rec["fow_m"][s], rec["back_m"][s], rec["guard"][s]] == [int(v) for v in c["ref_counts"]] + [0], name
        # nothing else moved: the key frame apart from m_id_f, the frame's list apart from m_id_kf
        for k in ("f0", "f1", "f2"):
            same_but(got[k][s], up_kf[s], "m_id_f")
        assert got["f2"][s]["m_id_f"].tobytes() == got["f1"][s]["m_id_f"].tobytes()   # correctAugmentate leaves the key frame alone
        same_but(got["b1"][s], up_new[s], "m_id_kf")


@pytest.fixture(scope="module")
def crafted_ctx():
    eh = edgehip.EdgeHip(edgehip.euroc_params(64, 48, zfx=420.0, zfy=420.0, max_points=20000), nseq=7, nslots=2, device=0)
    eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
    yield eh
    eh.close()


def test_stage_entries_equal_the_reference_on_a_ragged_batch(crafted_ctx):
    """Crafted graphs (fan-in, cycle, self-links, competing seeds, duplicate m_id), E == 0, kn of 0 and 1 on either side, and a list of
    max_points = 20000 KeyLines (past 16384: the keys of that sequence live in HBM, the others' in LDS) in one launch set."""
    cases = crafted()
    assert len(cases["BIG"]["kf_p_id"]) == crafted_ctx.cap
    run_batch(crafted_ctx, cases, ["A", "E0", "K00", "K01", "K10", "K11", "BIG"])


@pytest.mark.parametrize("name", ["B", "NOAUG"])
def test_stage_entries_with_tolerance_and_without_augmentation(crafted_ctx, name):
    """dist_tolerance > 0 (slides that return at once or stop by tolerance); augmentate = false (phases 1 and 3 alone)."""
    run_batch(crafted_ctx, crafted(), [name, "K11", "K00"])


def test_stage_entries_equal_the_reference_on_chained_frames():
    """Frames 1..5 of the chained-realistic fixture as five sequences of one batch (key frames 0 and 1, lists of different lengths)."""
    z = np.load(os.path.join(GOLD, "chained.npz"))
    cases, names = {}, []
    for k in range(1, int(z["n_frames"])):
        c = {key[len(f"f{k}_"):]: z[key] for key in z.files if key.startswith(f"f{k}_")}
        for key in ("p_m", "p_id", "n_id", "Pose", "Pos"):
            c[f"kf_{key}"] = z[f"kf{int(c['kf'])}_{key}"]
        c.update(dist_thresh=z["dist_thresh"], dist_tolerance=z["dist_tolerance"], augmentate=np.int32(1))
        cases[f"f{k}"] = c
        names.append(f"f{k}")
    p = edgehip.euroc_params(int(z["w"]), int(z["h"]))
    assert np.float32((np.float32(p.zfx) + np.float32(p.zfy)) / np.float32(2)) == z["zf"]
    eh = edgehip.EdgeHip(p, nseq=len(names), nslots=2, device=0)
    try:
        eh.keyframe_track_enable(True, float(z["kf_save_percent"]), True, in_frame_driver=False)
        run_batch(eh, cases, names)
    finally:
        eh.close()


def test_insert_copies_the_slot_and_applies_both_resets(crafted_ctx):
    eh, cases, rs = crafted_ctx, crafted(), np.random.RandomState(9)
    lists, before = [], []
    for s in range(eh.nseq):
        c = cases[["A", "B", "K01", "K00"][s % 4]]
        kl = records(rs, c["new_p_m"], c["new_p_id"], c["new_n_id"])
        eh.upload_keylines(s, 1, kl)
        eh.upload_keyframe(s, records(rs, c["kf_p_m"], c["kf_p_id"], c["kf_n_id"]), eh.kf_pose(np.eye(3) * 2, [7, 8, 9], t=3.0, K=4.0))
        lists.append(kl)
        before.append(eh.download_keyframe(s))
    mask = np.array([1, 0, 1, 1, 0, 1, 0], bool)
    poses = [eh.kf_pose(np.arange(9.0) + s, [s, 2 * s, 3 * s], t=0.5 * s, K=1.0 + s) for s in range(eh.nseq)]
    eh.keyframe_insert(1, mask, poses)
    rec = eh.read_keyframe_track()
    for s in range(eh.nseq):
        kf, pose, count = eh.download_keyframe(s)
        slot = eh.download_keylines(s, 1, want_mask=False)[0]
        if not mask[s]:   # only masked sequences change
            assert kf.tobytes() == before[s][0].tobytes() and bytes(pose) == bytes(before[s][1]) and count == before[s][2]
            assert slot.tobytes() == lists[s].tobytes()
            continue
        want = lists[s].copy()
        want["m_id_f"] = np.arange(len(want))
        want["rho0"], want["s_rho0"] = want["rho"], want["s_rho"]
        assert kf.tobytes() == want.tobytes()
        assert bytes(pose) == bytes(poses[s]) and count == before[s][2] + 1 and rec["kf_count"][s] == count and rec["kf_kn"][s] == len(want)
        same_but(slot, lists[s], "m_id_kf")
        assert np.array_equal(slot["m_id_kf"], np.arange(len(slot)))


# ---- the frame driver ---------------------------------------------------------------------------------------------------------------
W, H, NSEQ, NFRAMES = 256, 192, 3, 7
KF_SAVE_PERCENT = 0.985   # the back-match share of these sequences falls from about 0.995 by about 0.01 per frame (chained.npz records the same
                          # scene's counts): a second key frame after two to four frames, none in the frame after an insertion


def nav_rows(eh):
    return np.frombuffer(b"".join(bytes(n) for n in eh.read_nav()), edgehip.NAV_DTYPE).copy()


@pytest.fixture(scope="module")
def driven():
    """Three sequences, seven frames, three contexts: A with the feature in the frame driver, B stepped through the stage-level entry
    points around its (feature-less) frames in the reference's order, C with the feature switched on and off again before the first frame."""
    p = edgehip.euroc_params(W, H)
    seqs = [list(f for f, _, _ in synth.billboard_sequence(W, H, NFRAMES, seed=11 + s, traj_seed=13 + s)) for s in range(NSEQ)]
    A, B, Cx = (edgehip.EdgeHip(p, nseq=NSEQ, nslots=3, device=0) for _ in range(3))
    out = dict(recA=[], recB=[], navA=[], navB=[], navC=[], kfA=[], kfB=[], idA=[], idB=[], ran=[])
    try:
        A.keyframe_track_enable(True, KF_SAVE_PERCENT, True)
        B.keyframe_track_enable(True, KF_SAVE_PERCENT, True, in_frame_driver=False)
        Cx.keyframe_track_enable(True, KF_SAVE_PERCENT, True)
        Cx.keyframe_track_enable(False)
        for k in range(NFRAMES):
            frame = np.stack([seqs[s][k] for s in range(NSEQ)])
            recB = np.zeros(NSEQ, edgehip.KF_TRACK_DTYPE)
            if k == 1:   # rebvo_second_t.cpp:156-162: the first key frame is the old frame, K = 1, with the old frame's nav record
                poses = []
                for n in B.read_nav():
                    q = edgehip.KfPose()
                    q.t, q.K = n.t, 1.0
                    for f in ("Rot", "RotLie", "Vel", "Pose", "PoseLie", "Pos"):
                        getattr(q, f)[:] = getattr(n, f)[:]
                    poses.append(q)
                B.keyframe_insert(B.cur_slot(), None, poses)
                recB["inserted"] = 1
            prev = [B.get_state(s) for s in range(NSEQ)]
            for eh in (A, B, Cx):
                eh.upload_rgb(eh.next_slot(), frame)
                eh.process_frame(0.05 * k)
            navA, navB, navC = nav_rows(A), nav_rows(B), nav_rows(Cx)
            sn = B.cur_slot()
            if k >= 1:
                st = [B.get_state(s) for s in range(NSEQ)]
                loc = [port.local_pose(prev[s].Pose[:], st[s].R[:], prev[s].Pos[:], st[s].V[:], prev[s].K) for s in range(NSEQ)]
                Pose, Pos = np.array([l[0] for l in loc]), np.array([l[1] for l in loc])
                recB["back_m0"] = navB["kf_matchs"]
                recB["fow_m0"] = B.keyframe_build_forward_match(sn)
                recB["fow_m"] = B.keyframe_forward_correct(sn, Pose, Pos, 10.0, 0.0, True)
                recB["back_m"] = B.keyframe_back_correct(sn, Pose, Pos, 10.0, 0.0, True)
                ins = recB["back_m"] < np.minimum(p.track_points, navB["kn"]) * KF_SAVE_PERCENT
                if ins.any():
                    B.keyframe_insert(sn, ins, None)
                recB["inserted"] |= ins
                out["ran"].append((navB["klm_num"] >= p.global_match_threshold) & (navB["estimation_ok"] != 0))
            got = B.read_keyframe_track()
            recB["kf_count"], recB["kf_kn"] = got["kf_count"], got["kf_kn"]
            out["recA"].append(A.read_keyframe_track()); out["recB"].append(recB)
            out["navA"].append(navA); out["navB"].append(navB); out["navC"].append(navC)
            out["kfA"].append([A.download_keyframe(s) for s in range(NSEQ)])
            out["kfB"].append([B.download_keyframe(s) for s in range(NSEQ)])
            out["idA"].append([A.download_keylines(s, A.cur_slot(), want_mask=False)[0]["m_id_kf"] for s in range(NSEQ)])
            out["idB"].append([B.download_keylines(s, sn, want_mask=False)[0]["m_id_kf"] for s in range(NSEQ)])
    finally:
        for eh in (A, B, Cx):
            eh.close()
    return out


def test_process_frame_equals_the_stage_level_entries(driven):
    d = driven
    assert all(r.all() for r in d["ran"])   # every frame pair reached the steps (otherwise the stage-level context, which runs them always, is no reference)
    for k in range(NFRAMES):
        for f in ("fow_m0", "fow_m", "back_m0", "back_m", "inserted", "kf_count", "kf_kn"):
            assert np.array_equal(d["recA"][k][f], d["recB"][k][f]), (k, f, d["recA"][k][f], d["recB"][k][f])
        assert not d["recA"][k]["guard"].any()
        for s in range(NSEQ):
            (ka, pa, ca), (kb, pb, cb) = d["kfA"][k][s], d["kfB"][k][s]
            assert ka.tobytes() == kb.tobytes() and bytes(pa) == bytes(pb) and ca == cb, (k, s)
            assert np.array_equal(d["idA"][k][s], d["idB"][k][s]), (k, s)
    counts = np.array([r["kf_count"] for r in d["recA"]])
    inserted = np.array([r["inserted"] for r in d["recA"]])
    assert (counts[0] == 0).all() and (counts[1] >= 1).all() and inserted[1].all()
    assert (counts[-1] >= 2).any(), counts          # at least one sequence took a second key frame by the criterion
    assert (inserted[2:] == 0).any(), inserted      # and at least one frame did not insert
    assert all(int(r["back_m"][s]) > 0 and int(r["fow_m"][s]) >= int(r["fow_m0"][s]) > 0 for r in d["recA"][1:] for s in range(NSEQ))


def test_nav_with_the_feature_on_differs_only_in_kf_matchs(driven):
    d = driven
    for k in range(NFRAMES):
        for f in edgehip.NAV_DTYPE.names:
            if f != "kf_matchs":
                assert d["navA"][k][f].tobytes() == d["navC"][k][f].tobytes(), (k, f)
        assert np.array_equal(d["navA"][k]["kf_matchs"], d["recA"][k]["back_m"])   # num_kf_back_m as the repair left it


def test_nav_with_the_feature_off_is_unchanged(driven):
    """A context whose feature was switched off again, and one that keeps the store for the stage-level calls only: their frames are the
    frames of a context without the feature; kf_matchs stays directed_matching's count (0 without a key frame)."""
    d = driven
    for k in range(NFRAMES):
        for f in edgehip.NAV_DTYPE.names:
            if f != "kf_matchs":
                assert d["navB"][k][f].tobytes() == d["navC"][k][f].tobytes(), (k, f)
        assert not d["navC"][k]["kf_matchs"].any()
        assert np.array_equal(d["navB"][k]["kf_matchs"], d["recB"][k]["back_m0"])
