#!/usr/bin/env python3
"""Generate tests/golden/keyframe_track/*.npz from the REFERENCE's own key-frame match repair (src/mtracklib/kfvo.cpp).

Build machine only (needs the reference tree and oracle/_ref/libreforacle.so from `make -C oracle`):
    python tools/make_keyframe_track_golden.py [--ref /path/to/reference]

tools/keyframe_track_ref_driver.cpp is compiled into a temporary directory outside the repository, with the reference's kfvo.cpp
included in place (nothing is written under oracle/, no reference source is copied).  Every case holds only what the three steps read and
write: p_m, p_id, n_id, m_id, m_id_f, m_id_kf per list, the poses, zf, the arguments, the reference's ids and counts after each step and
its seconds.  Before anything is written the plain-Python port (tests/keyframe_track_port.py) must equal the reference on every id and
count; the branch populations come from that port's run and are stored (and, for the crafted cases, asserted non-empty).

  crafted.npz   link graphs of a few hundred KeyLines built to populate every branch of the slides and of the augment walks (fan-in,
                cycles, self-links, competing seeds, duplicate m_id, dist_tolerance > 0, E == 0, kn of 0 and 1), plus one list of 20000
  chained.npz   consecutive frames of synth.billboard_sequence (256x192) through the reference oracle's own pipeline on the CPU; m_id_kf
                propagated as directed_matching / FordwardMatch do (the KeyLine a new one was matched to hands over its m_id_kf), the
                key-frame state fed from one frame's result into the next, insertion at frame 0 and by the criterion
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import keyframe_track_port as port  # noqa: E402
from oracle import oracle  # noqa: E402
from rebvo_amd import synth  # noqa: E402
from rebvo_amd.edgehip import KEYLINE_DTYPE  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "keyframe_track")
SIZE_LIMIT = 919829   # the largest file under tests/golden/depth_surface/
# A pre-included header: depth_filler.h's inline interpolation helpers (not on this path) call std::max(float, double), which this C++
# library does not resolve on its own.
PRELUDE = "#include <algorithm>\nnamespace std { inline double max(float a, double b) { return max((double)a, b); } }\n"

# what every "full" crafted case must populate (port.Stats keys), and the graph features counted by graph_features()
REQUIRED = ("slide_tolerance_at_once", "slide_along_n", "slide_along_p", "slide_stop_chain_end", "slide_stop_non_decrease",
            "slide_stop_tolerance", "walk_stop_missing_link", "walk_stop_matched", "walk_stop_failed_correction",
            "filled_after_failure_from_other_side", "walk_met_other_seed_fill", "far_seed_propagated",
            "fan_in", "cycle", "self_link", "duplicate_m_id")


def build_driver(ref, tmp):
    inc = os.path.join(ROOT, "oracle", "_ref", "inc")
    lib = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(lib, "libreforacle.so")):
        raise SystemExit("oracle/_ref/libreforacle.so is missing: run `make -C oracle` first")
    pre = os.path.join(tmp, "prelude.h")
    with open(pre, "w") as f:
        f.write(PRELUDE)
    exe = os.path.join(tmp, "kf_driver")
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-access-control", "-w", "-include", pre,
           "-I" + inc, "-I" + os.path.join(ref, "include"), "-I" + ref,
           os.path.join(ROOT, "tools", "keyframe_track_ref_driver.cpp"), os.path.join(ref, "src", "mtracklib", "keyframe.cpp"),
           os.path.join(ref, "src", "visualizer", "depth_filler.cpp"),
           "-L" + lib, "-Wl,-rpath," + lib, "-lreforacle", "-lm", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def records(p_m, p_id, n_id, m_id=None, m_id_f=None, m_id_kf=None):
    kl = np.zeros(len(p_id), KEYLINE_DTYPE)
    kl["p_m"] = np.asarray(p_m, np.float32).reshape(-1, 2)
    kl["p_id"], kl["n_id"] = p_id, n_id
    for name, v in (("m_id", m_id), ("m_id_f", m_id_f), ("m_id_kf", m_id_kf)):
        kl[name] = -1 if v is None else v
    return kl


def run_ref(exe, case):
    kf = records(case["kf_p_m"], case["kf_p_id"], case["kf_n_id"], m_id_f=case["kf_m_id_f"])
    new = records(case["new_p_m"], case["new_p_id"], case["new_n_id"], m_id=case["new_m_id"], m_id_kf=case["new_m_id_kf"])
    hdr = np.array([len(kf), len(new), int(case["old_kn"]), int(case["augmentate"])], np.int32).tobytes()
    d = np.concatenate([[case["dist_thresh"], case["dist_tolerance"]], np.ravel(case["kf_Pose"]), np.ravel(case["kf_Pos"]),
                        np.ravel(case["Pose"]), np.ravel(case["Pos"])]).astype(np.float64)
    assert d.size == 26
    payload = hdr + np.float32(case["zf"]).tobytes() + d.tobytes() + kf.tobytes() + new.tobytes()
    out = subprocess.run([exe], input=payload, check=True, capture_output=True).stdout
    nk, nn = len(kf), len(new)
    assert len(out) == 16 + 24 + 4 * (2 * nk + nn), (len(out), nk, nn)
    cnt = np.frombuffer(out, np.int32, 4, 0)
    sec = np.frombuffer(out, np.float64, 3, 16)
    f0 = np.frombuffer(out, np.int32, nk, 40)
    f1 = np.frombuffer(out, np.int32, nk, 40 + 4 * nk)
    b1 = np.frombuffer(out, np.int32, nn, 40 + 8 * nk)
    return {"ref_counts": cnt[:3].copy(), "ref_seconds": sec.copy(), "ref_m_id_f_0": f0.copy(), "ref_m_id_f_1": f1.copy(),
            "ref_m_id_kf_1": b1.copy()}


def run_port(case, order="serial"):
    st = port.Stats()
    kf = {k[3:]: case[k] for k in ("kf_p_m", "kf_p_id", "kf_n_id", "kf_m_id_f", "kf_Pose", "kf_Pos")}
    new = {k[4:]: case[k] for k in ("new_p_m", "new_p_id", "new_n_id", "new_m_id", "new_m_id_kf")}
    out = port.track_frame(kf, new, case["old_kn"], case["Pose"], case["Pos"], float(np.float32(case["zf"])), case["dist_thresh"],
                           case["dist_tolerance"], bool(case["augmentate"]), order=order, stats=st)
    return out, st


def check(case, ref, name):
    """port == reference on every id and count."""
    out, st = run_port(case)
    assert out["guard"] == 0, name
    for a, b in (("m_id_f_0", "ref_m_id_f_0"), ("m_id_f_1", "ref_m_id_f_1"), ("m_id_kf_1", "ref_m_id_kf_1")):
        assert np.array_equal(out[a], ref[b]), (name, a, int((out[a] != ref[b]).sum()))
    assert [out["fow_m0"], out["fow_m"], out["back_m"]] == list(ref["ref_counts"]), (name, out["fow_m0"], out["fow_m"], out["back_m"], ref["ref_counts"])
    return st


def graph_features(p_id, n_id, m_id):
    kn = len(p_id)
    st = {}
    tgt = n_id[(n_id >= 0)]
    st["fan_in"] = int((np.bincount(tgt, minlength=kn) > 1).sum()) if kn else 0
    st["self_link"] = int((n_id == np.arange(kn)).sum() + (p_id == np.arange(kn)).sum())
    cyc = 0
    for s in range(kn):   # n_id chains that come back to their start
        j, steps = n_id[s], 0
        while j >= 0 and j != s and steps < kn:
            j, steps = n_id[j], steps + 1
        cyc += j == s and n_id[s] != s
    st["cycle"] = int(cyc)
    mm = m_id[m_id >= 0]
    st["duplicate_m_id"] = int((np.bincount(mm) > 1).sum()) if mm.size else 0
    return st


# ---- crafted lists --------------------------------------------------------------------------------------------------------------
def curves(rs, n_curves, length, x_span, wiggle):
    """Chains of points running down the image: (p_m [n][2] float32, p_id, n_id, curve id, position on the curve)."""
    pm, p_id, n_id, cid, pos = [], [], [], [], []
    for c in range(n_curves):
        x0 = rs.uniform(-x_span, x_span)
        y0 = rs.uniform(-100, -100 + 40)
        slope = rs.uniform(-0.4, 0.4)
        base = len(pm)
        for s in range(length):
            pm.append((x0 + slope * s * 2 + rs.normal(0, wiggle), y0 + s * 2.0 + rs.normal(0, wiggle)))
            p_id.append(base + s - 1 if s else -1)
            n_id.append(base + s + 1 if s + 1 < length else -1)
            cid.append(c)
            pos.append(s)
    return (np.array(pm, np.float32).reshape(-1, 2), np.array(p_id, np.int32), np.array(n_id, np.int32), np.array(cid), np.array(pos))


def permute(rs, pm, p_id, n_id):
    """Shuffle the list order (an edge's KeyLines are not consecutive in a real list either) -> arrays + old->new index map."""
    kn = len(p_id)
    perm = rs.permutation(kn)          # new position k holds old element perm[k]
    inv = np.empty(kn, np.int64)
    inv[perm] = np.arange(kn)
    remap = lambda a: np.where(a >= 0, inv[np.maximum(a, 0)], -1).astype(np.int32)
    return pm[perm], remap(p_id[perm]), remap(n_id[perm]), inv


def crafted_case(seed, n_curves=10, length=30, tol=0.0, thresh=10.0, match_rate=0.3):
    rs = np.random.RandomState(seed)
    zf = np.float32(420.0)
    # the new frame's list, and the key frame's: the same curves seen from a camera a little to the side
    npm, npid, nnid, ncid, npos = curves(rs, n_curves, length, 150, 0.25)
    kpm = npm + np.float32([3.0, 0.0]) + rs.normal(0, 0.3, npm.shape).astype(np.float32)
    kpid, knid, kcid, kpos = npid.copy(), nnid.copy(), ncid.copy(), npos.copy()
    out = rs.rand(len(kpm)) < 0.04     # outliers: their own distance stays large, their neighbours' does not
    kpm[out] += np.float32([0.0, 1.0]) * rs.choice([-1, 1], out.sum())[:, None].astype(np.float32) * np.float32(80.0)
    kn = len(kpm)
    at = lambda c, s: c * length + int(np.clip(s, 0, length - 1))
    # wanted matches key frame -> new: along the same curve a few places off, some on another curve altogether
    want = np.full(kn, -1, np.int64)
    for k in range(kn):
        if rs.rand() < match_rate:
            want[k] = at(kcid[k], kpos[k] + rs.randint(-7, 8)) if rs.rand() > 0.12 else at(rs.randint(n_curves), rs.randint(length))
    back = np.full(kn, -1, np.int64)    # new -> key frame
    for j in range(kn):
        if rs.rand() < match_rate:
            back[j] = at(ncid[j], npos[j] + rs.randint(-7, 8)) if rs.rand() > 0.12 else at(rs.randint(n_curves), rs.randint(length))
    # graph features on both lists: fan-in (a chain's end joins the middle of another chain; p_id of the target still names its own
    # predecessor), a link cycle, self-links
    for p_id, n_id in ((kpid, knid), (npid, nnid)):
        n_id[at(0, length - 1)] = at(1, length // 2)
        n_id[at(2, length - 1)] = at(2, 0); p_id[at(2, 0)] = at(2, length - 1)
        n_id[at(3, length - 1)] = at(3, length - 1)
        p_id[at(4, 0)] = at(4, 0)
    kpm, kpid, knid, kinv = permute(rs, kpm, kpid, knid)
    npm, npid, nnid, ninv = permute(rs, npm, npid, nnid)
    new_m_id_kf = np.full(kn, -1, np.int32)
    new_m_id_kf[ninv] = np.where(back >= 0, kinv[np.maximum(back, 0)], -1)
    # buildForwardMatch's input: the key frame's m_id_f index the OLD list (here: k itself, as after resetForwardMatch, some lost), the
    # new KeyLines' m_id name old KeyLines; duplicates make "the largest new index wins" matter
    old_kn = kn + 7
    kf_m_id_f = np.where(rs.rand(kn) < 0.9, np.arange(kn), -1).astype(np.int32)
    new_m_id = np.full(kn, -1, np.int32)
    for k_old in range(kn):
        if want[k_old] >= 0:
            new_m_id[ninv[want[k_old]]] = kinv[k_old]
    for _ in range(kn // 10):   # duplicates and matches to old KeyLines the key frame does not point at
        new_m_id[rs.randint(kn)] = rs.randint(old_kn)
    ang = rs.uniform(-0.01, 0.01, 3)
    Pose = synth._so3_exp(ang)
    Pos = np.array([0.3, rs.uniform(-0.02, 0.02), rs.uniform(-0.02, 0.02)])
    return dict(kf_p_m=kpm, kf_p_id=kpid, kf_n_id=knid, kf_m_id_f=kf_m_id_f, new_p_m=npm, new_p_id=npid, new_n_id=nnid,
                new_m_id=new_m_id, new_m_id_kf=new_m_id_kf, old_kn=np.int32(old_kn), kf_Pose=np.eye(3), kf_Pos=np.zeros(3),
                Pose=Pose, Pos=Pos, zf=zf, dist_thresh=np.float64(thresh), dist_tolerance=np.float64(tol), augmentate=np.int32(1))


def tiny_case(kn_kf, kn_new):
    rs = np.random.RandomState(kn_kf * 7 + kn_new)
    mk = lambda n: (rs.uniform(-50, 50, (n, 2)).astype(np.float32), np.full(n, -1, np.int32), np.full(n, -1, np.int32))
    kpm, kpid, knid = mk(kn_kf)
    npm, npid, nnid = mk(kn_new)
    return dict(kf_p_m=kpm, kf_p_id=kpid, kf_n_id=knid, kf_m_id_f=np.arange(kn_kf, dtype=np.int32), new_p_m=npm, new_p_id=npid,
                new_n_id=nnid, new_m_id=np.zeros(kn_new, np.int32) if kn_kf else np.full(kn_new, -1, np.int32),
                new_m_id_kf=np.zeros(kn_new, np.int32) if kn_kf else np.full(kn_new, -1, np.int32), old_kn=np.int32(max(kn_kf, 1)),
                kf_Pose=np.eye(3), kf_Pos=np.zeros(3), Pose=np.eye(3), Pos=np.array([0.2, 0.0, 0.0]), zf=np.float32(420.0),
                dist_thresh=np.float64(10.0), dist_tolerance=np.float64(0.0), augmentate=np.int32(1))


def crafted(exe):
    cases = {}
    # seeds are searched, in order, for lists on which the reference (through the port that equals it) populates every branch
    def full(name, **kw):
        for seed in range(1000, 1200):
            case = crafted_case(seed, **kw)
            st = check(case, run_ref(exe, case), name)
            for d in (graph_features(case["kf_p_id"], case["kf_n_id"], case["new_m_id"]), ):
                st.update(d)
            if all(st.get(k, 0) > 0 for k in REQUIRED if kw.get("tol", 0.0) > 0 or "tolerance" not in k):
                case["seed"] = np.int32(seed)
                cases[name] = case
                return
        raise SystemExit(f"{name}: no seed populates every branch; last stats {dict(st)}")
    full("A")                                   # dist_tolerance = 0, as SecondThread calls the steps
    full("B", tol=1.5, n_curves=12, length=24)  # dist_tolerance > 0: slides return at once / stop by tolerance
    c = crafted_case(1000); c["Pos"] = np.zeros(3); c["Pose"] = np.eye(3); cases["E0"] = c      # V = 0: E == 0, every distance NaN
    c = crafted_case(1001); c["augmentate"] = np.int32(0); cases["NOAUG"] = c                   # phases 1 and 3 alone
    cases["K00"] = tiny_case(0, 0)
    cases["K01"] = tiny_case(0, 1)
    cases["K10"] = tiny_case(1, 0)
    cases["K11"] = tiny_case(1, 1)
    cases["BIG"] = crafted_case(7, n_curves=250, length=80)   # 20000 KeyLines: past 16384, where the device's keys leave LDS
    rec = {"names": np.array(sorted(cases))}
    for name, case in sorted(cases.items()):
        ref = run_ref(exe, case)
        st = check(case, ref, name)
        st.update(graph_features(case["kf_p_id"], case["kf_n_id"], case["new_m_id"]))
        if name in ("A", "B"):
            missing = [k for k in REQUIRED if st.get(k, 0) == 0 and (name == "B" or "tolerance" not in k)]   # (dist_tolerance = 0: no slide ends by it)
            assert not missing, (name, missing)
        if name == "B":
            assert st["slide_tolerance_at_once"] and st["slide_stop_tolerance"]
        if name == "E0":   # E == 0: nothing slides, nothing is dropped
            assert not any(k.startswith("slide_along") for k in st) and "walk_stop_failed_correction" not in st
        keys = sorted(st)
        case.update(ref)
        case["stat_names"], case["stat_values"] = np.array(keys), np.array([st[k] for k in keys], np.int64)
        for k, v in case.items():
            rec[f"{name}_{k}"] = np.asarray(v)
        print(f"crafted {name}: kf {len(case['kf_p_id'])} new {len(case['new_p_id'])} counts {list(ref['ref_counts'])} "
              f"ref seconds {ref['ref_seconds'].sum():.2e} stats {dict(st)}")
    return rec


# ---- chained realistic ------------------------------------------------------------------------------------------------------------
def chained(exe, w=256, h=192, n_frames=6):
    params = oracle.euroc_params(w, h)
    orc = oracle.Oracle("ref", params)
    zf = np.float32((np.float32(params.zfx) + np.float32(params.zfy)) / np.float32(2))
    frames = []
    prev_kl, prev_st = None, None
    for k, (f, _, _) in enumerate(synth.billboard_sequence(w, h, n_frames)):
        _, nav = orc.process_frame(f, 0.05 * k)
        st = orc.seq_state()
        kl = orc.keylines(orc.cur_slot()).copy()
        frames.append(dict(kl=kl, nav=nav.as_dict(), Pose=np.array(st.Pose[:]).reshape(3, 3), Pos=np.array(st.Pos[:]), K=st.K, V=np.array(st.V[:]),
                           prev_kn=0 if prev_kl is None else len(prev_kl)))
        prev_kl, prev_st = kl, st
    orc.close()
    # first pass with KFSavePercent = 0 (no insertion by the criterion) to see what the reference counts, then the real pass
    def run(save_percent):
        rec, kf, kf_id, m_id_kf_prev, inserts = {}, None, -1, None, []
        for k, fr in enumerate(frames):
            kl = fr["kl"]
            if k == 0:
                m_id_kf_prev = np.full(len(kl), -1, np.int32)
                continue
            old = frames[k - 1]
            if kf is None:   # rebvo_second_t.cpp:156-162: the first key frame is the OLD frame
                kf = dict(p_m=old["kl"]["p_m"].copy(), p_id=old["kl"]["p_id"].copy(), n_id=old["kl"]["n_id"].copy(),
                          m_id_f=np.arange(len(old["kl"]), dtype=np.int32), Pose=old["Pose"], Pos=old["Pos"])
                m_id_kf_prev = np.arange(len(old["kl"]), dtype=np.int32)
                kf_id += 1
                inserts.append(k - 1)
                for key in ("p_m", "p_id", "n_id", "Pose", "Pos"):
                    rec[f"kf{kf_id}_{key}"] = kf[key]
            m = kl["m_id"]
            m_id_kf = np.where(m >= 0, m_id_kf_prev[np.maximum(m, 0)], -1).astype(np.int32)
            Pose, Pos = port.local_pose(old["Pose"], np.array(fr["nav"]["Rot"]).reshape(3, 3), old["Pos"], fr["V"], old["K"])
            ran = fr["nav"]["klm_num"] >= params.global_match_threshold and fr["nav"]["estimation_ok"]
            case = dict(kf_p_m=kf["p_m"], kf_p_id=kf["p_id"], kf_n_id=kf["n_id"], kf_m_id_f=kf["m_id_f"], new_p_m=kl["p_m"],
                        new_p_id=kl["p_id"], new_n_id=kl["n_id"], new_m_id=m, new_m_id_kf=m_id_kf, old_kn=np.int32(fr["prev_kn"]),
                        kf_Pose=kf["Pose"], kf_Pos=kf["Pos"], Pose=Pose, Pos=Pos, zf=zf, dist_thresh=np.float64(10.0),
                        dist_tolerance=np.float64(0.0), augmentate=np.int32(1))
            assert ran, f"frame {k}: the reference did not reach the key-frame steps (klm_num {fr['nav']['klm_num']})"
            ref = run_ref(exe, case)
            stt = check(case, ref, f"chained frame {k}")
            back_m = int(ref["ref_counts"][2])
            kf["m_id_f"] = ref["ref_m_id_f_1"]
            m_id_kf_prev = ref["ref_m_id_kf_1"].copy()
            inserted = back_m < min(params.track_points, len(kl)) * save_percent
            for key in ("new_p_m", "new_p_id", "new_n_id", "new_m_id", "new_m_id_kf", "kf_m_id_f", "old_kn", "Pose", "Pos"):
                rec[f"f{k}_{key}"] = case[key]
            for key, v in ref.items():
                rec[f"f{k}_{key}"] = v
            rec[f"f{k}_kf"], rec[f"f{k}_inserted"] = np.int32(kf_id), np.int32(inserted)
            keys = sorted(stt)
            rec[f"f{k}_stat_names"], rec[f"f{k}_stat_values"] = np.array(keys), np.array([stt[q] for q in keys], np.int64)
            print(f"chained frame {k}: kf {kf_id} ({len(kf['p_id'])} KeyLines) new {len(kl)} counts {list(ref['ref_counts'])} "
                  f"min(TrackPoints, KNum) {min(params.track_points, len(kl))} inserted {inserted} ref seconds {ref['ref_seconds'].sum():.2e}")
            if inserted:   # :591-596: the new frame becomes the key frame, with its integrated pose
                kf = dict(p_m=kl["p_m"].copy(), p_id=kl["p_id"].copy(), n_id=kl["n_id"].copy(), m_id_f=np.arange(len(kl), dtype=np.int32),
                          Pose=fr["Pose"], Pos=fr["Pos"])
                m_id_kf_prev = np.arange(len(kl), dtype=np.int32)
                kf_id += 1
                inserts.append(k)
                for key in ("p_m", "p_id", "n_id", "Pose", "Pos"):
                    rec[f"kf{kf_id}_{key}"] = kf[key]
        return rec, inserts
    rec0, _ = run(0.0)
    ratios = [int(rec0[f"f{k}_ref_counts"][2]) / min(params.track_points, len(frames[k]["kl"])) for k in range(1, n_frames)]
    # a threshold the sequence crosses once or twice: between the smallest and the median ratio of a run without insertions
    save_percent = float(np.round((min(ratios) + float(np.median(ratios))) / 2, 3))
    rec, inserts = run(save_percent)
    assert inserts[0] == 0 and len(inserts) >= 2 and len(inserts) < n_frames, (inserts, ratios, save_percent)
    rec.update(w=np.int32(w), h=np.int32(h), n_frames=np.int32(n_frames), zf=zf, kf_save_percent=np.float64(save_percent),
               track_points=np.int32(params.track_points), inserts=np.array(inserts, np.int32), dist_thresh=np.float64(10.0),
               dist_tolerance=np.float64(0.0))
    print(f"chained: back-match ratios without insertion {np.round(ratios, 3)}, KFSavePercent {save_percent}, insertions after frames {inserts}")
    return rec


def write(path, rec):
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= SIZE_LIMIT, (path, size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF", "/root/reference"))
    a = ap.parse_args()
    os.makedirs(GOLD, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="keyframe_track_ref_") as tmp:
        exe = build_driver(a.ref, tmp)
        write(os.path.join(GOLD, "crafted.npz"), crafted(exe))
        write(os.path.join(GOLD, "chained.npz"), chained(exe))


if __name__ == "__main__":
    main()
