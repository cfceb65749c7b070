#!/usr/bin/env python3
"""Generate tests/golden/keyframe_constraint/*.npz from the REFERENCE's own kfvo::OptimizeRelContraint and kfvo::mutualExclusionSimple.

Build machine only (needs the reference tree and oracle/_ref/libreforacle.so from `make -C oracle`):
    python tools/make_keyframe_constraint_golden.py --ref /path/to/reference

tools/keyframe_constraint_ref_driver.cpp is compiled into a temporary directory outside the repository, with the reference's kfvo.cpp
included in place (nothing is written under oracle/, no reference source is copied).  A fixture holds, per KeyLine, only the numbers the
rules read (p_m, u_m as float32; rho, s_rho as float64; the link), the poses, the arguments, the reference's outputs and its seconds.
Nothing is written unless, for every numerically compared case,
  * the plain-numpy port (tests/keyframe_constraint_port.py) and the reference agree on every count and on every link after pruning,
    exactly, and on every fp64 output to 1e-13 relative (they sum in the same order; the slack is libm's);
  * the reference, run a second time with both lists shuffled and the links remapped, agrees with its first run to 1/100 of the tests'
    tolerances (an accept/reject that flips with the summation order disqualifies the case, not the device);
  * links >= 30 and E/E0 > 1e-6 in the reference;
and the stated branch populations are non-zero.  E is not among the reference function's outputs: the fixture's E is the port's, tied to
the reference through E/E0 (the return value) and E0 (the driver repeats the first two evaluations).

  crafted.npz   70x50, lists of 0, 1, 5, 65, 257, 600 and 1030 KeyLines: the frame list is the key-frame list moved by a known small pose with
                0.3 px of noise, 5 % 15-px outliers, 20 % of the links dropped in each direction independently and some links crossed to
                a neighbour (mutual pairs that pass and fail dist_t); cases: direction 0 / 1, k_huber 0 / 2, iter_max 0 / 10, with and
                without both pruning passes first.  Degenerate inputs (no link, 1 and 5 links, a NaN rho, a link out of range) are stored
                as inputs only.
  chained.npz   consecutive frames of synth.billboard_sequence (256x192) through the reference oracle on the CPU; the first is the key
                frame; the links are the reference's own buildForwardMatch / forwardCorrectAugmentate / correctAugmentate
                (tools/keyframe_track_ref_driver.cpp), as tests/golden/keyframe_track/chained.npz is made
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import keyframe_constraint_port as port  # noqa: E402
from rebvo_amd import synth  # noqa: E402
from rebvo_amd.edgehip import KEYLINE_DTYPE  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "keyframe_constraint")
SIZE_LIMIT = 919829   # the largest file under tests/golden/depth_surface/
PRELUDE = "#include <algorithm>\nnamespace std { inline double max(float a, double b) { return max((double)a, b); } }\n"
REQUIRED = ("accepted_and_rejected_in_one_call", "reweighted", "unweighted", "unlinked_between", "scale_behind",
            "mutual_dropped_non_mutual", "mutual_failed_dist_kf", "mutual_passed_dist_kf", "mutual_failed_dist_fr", "mutual_passed_dist_fr")
# the tests' tolerances (tests/test_keyframe_constraint_gpu.py)
TOL = dict(X=(1e-9, 1e-12), scalar=1e-9, W_X=1e-9, R_X=1e-7)


def build_driver(ref, tmp):
    inc = os.path.join(ROOT, "oracle", "_ref", "inc")
    lib = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(lib, "libreforacle.so")):
        raise SystemExit("oracle/_ref/libreforacle.so is missing: run `make -C oracle` first")
    pre = os.path.join(tmp, "prelude.h")
    with open(pre, "w") as f:
        f.write(PRELUDE)
    exe = os.path.join(tmp, "kf_constraint_driver")
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-access-control", "-w", "-include", pre,
           "-I" + inc, "-I" + os.path.join(ref, "include"), "-I" + ref,
           os.path.join(ROOT, "tools", "keyframe_constraint_ref_driver.cpp"), os.path.join(ref, "src", "mtracklib", "keyframe.cpp"),
           os.path.join(ref, "src", "visualizer", "depth_filler.cpp"),
           "-L" + lib, "-Wl,-rpath," + lib, "-lreforacle", "-lm", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def camera(w, h, ppx, ppy, zfx, zfy):
    """cam_model's members: pp and zf as float, zfm = (double)((zf.x + zf.y) / 2) computed in float (cam_model.h:51-52)."""
    zfm = np.float64(np.float32((np.float32(zfx) + np.float32(zfy)) / np.float32(2)))
    return dict(w=np.int32(w), h=np.int32(h), ppx=np.float32(ppx), ppy=np.float32(ppy), zfx=np.float32(zfx), zfy=np.float32(zfy), zfm=zfm)


def run_ref(exe, pair, cam, case):
    kf = port.records(pair["kf"], KEYLINE_DTYPE, dict(m_id_f=pair["kf"]["m_id_f"]))
    fr = port.records(pair["fr"], KEYLINE_DTYPE, dict(m_id_kf=pair["fr"]["m_id_kf"]))
    payload = np.array([len(kf), len(fr), case["direction"], case["iter_max"], case["prune"], case["discard"]], np.int32).tobytes()
    payload += np.array([cam["ppx"], cam["ppy"], cam["zfx"], cam["zfy"]], np.float32).tobytes()
    payload += np.array([cam["w"], cam["h"]], np.int32).tobytes()
    payload += np.concatenate([[case["k_huber"], case["dist_t"]], np.ravel(pair["kf_Pose"]), np.ravel(pair["kf_Pos"]), [pair["kf_K"]],
                               np.ravel(pair["Pose"]), np.ravel(pair["Pos"]), [pair["K"]]]).astype(np.float64).tobytes()
    payload += kf.tobytes() + fr.tobytes()
    out = subprocess.run([exe], input=payload, check=True, capture_output=True).stdout
    assert len(out) == 32 + 83 * 8 + 4 * (len(kf) + len(fr)), (len(out), len(kf), len(fr))
    head = np.frombuffer(out, np.int32, 8, 0)
    res = np.frombuffer(out, np.float64, 83, 32)
    assert head[6] == 4, "util::norm<float>'s sqrt no longer binds to the float overload: the port and the device take sqrtf"
    return dict(links=int(head[0]), inliers=int(head[1]), prune_counts=head[2:6].copy(), X=res[:6].copy(), W_X=res[6:42].reshape(6, 6).copy(),
                R_X=res[42:78].reshape(6, 6).copy(), ratio=res[78], E0=res[79], Kp=res[80], W_Kp=res[81], seconds=res[82],
                m_id_f=np.frombuffer(out, np.int32, len(kf), 32 + 83 * 8).copy(),
                m_id_kf=np.frombuffer(out, np.int32, len(fr), 32 + 83 * 8 + 4 * len(kf)).copy())


def shuffled(rs, pair):
    """Both lists in a random order, the links remapped."""
    nk, nf = len(pair["kf"]["rho"]), len(pair["fr"]["rho"])
    pk, pf = rs.permutation(nk), rs.permutation(nf)          # new position j holds old element pk[j]
    ik, jf = np.empty(nk, np.int64), np.empty(nf, np.int64)  # old index -> new index
    ik[pk], jf[pf] = np.arange(nk), np.arange(nf)
    kf = {k: pair["kf"][k][pk] for k in port.LIST_FIELDS}
    fr = {k: pair["fr"][k][pf] for k in port.LIST_FIELDS}
    lf, lb = pair["kf"]["m_id_f"][pk], pair["fr"]["m_id_kf"][pf]
    kf["m_id_f"] = np.where(lf >= 0, jf[np.maximum(lf, 0)], -1).astype(np.int32)
    fr["m_id_kf"] = np.where(lb >= 0, ik[np.maximum(lb, 0)], -1).astype(np.int32)
    return dict(pair, kf=kf, fr=fr)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def check_case(exe, rs, pair, cam, case, name):
    """-> (ref outputs with the port's E, the port's trace), or None when the case is on a knife edge (the shuffled run differs)."""
    ref = run_ref(exe, pair, cam, case)
    pp, pc = port.pruned(pair, case["dist_t"], case["discard"], case["prune"])
    assert np.array_equal(pp["kf"]["m_id_f"], ref["m_id_f"]) and np.array_equal(pp["fr"]["m_id_kf"], ref["m_id_kf"]), (name, "pruned links")
    assert list(pc) == list(ref["prune_counts"]), (name, "prune counts", pc, ref["prune_counts"])
    trace = {}
    got = port.constraint(pp, case["direction"], case["iter_max"], case["k_huber"], trace)
    assert got["guard"] == 0, (name, "guard", got["guard"])
    assert (got["links"], got["inliers"]) == (ref["links"], ref["inliers"]), (name, "match_num", got["links"], got["inliers"], ref["links"], ref["inliers"])
    assert ref["links"] >= 30 and ref["ratio"] > 1e-6, (name, "links / ratio", ref["links"], ref["ratio"])
    for k in ("X", "W_X", "R_X", "ratio", "E0", "Kp", "W_Kp"):
        e = rel(got[k], ref[k])
        assert e <= 1e-13, (name, "port vs reference", k, e)
    # the knife-edge screen: the reference against itself in another order
    sp = shuffled(rs, pair)
    r2 = run_ref(exe, sp, cam, case)
    ok = (r2["links"], r2["inliers"]) == (ref["links"], ref["inliers"]) and list(r2["prune_counts"]) == list(ref["prune_counts"])
    ok = ok and np.all(np.abs(r2["X"] - ref["X"]) <= (TOL["X"][0] * np.abs(ref["X"]) + TOL["X"][1]) / 100)
    for k in ("ratio", "E0", "Kp", "W_Kp"):
        ok = ok and abs(r2[k] - ref[k]) <= TOL["scalar"] / 100 * abs(ref[k])
    ok = ok and np.abs(r2["W_X"] - ref["W_X"]).max() <= TOL["W_X"] / 100 * np.abs(ref["W_X"]).max()
    ok = ok and np.abs(r2["R_X"] - ref["R_X"]).max() <= TOL["R_X"] / 100 * np.abs(ref["R_X"]).max()
    if not ok:
        print(f"{name}: the reference's shuffled run differs from its first: a knife edge, disqualified")
        return None
    ref["E"] = got["E"]
    trace["evals"], trace["acc"] = got["evals"], got["accepted"]
    return ref, trace


def rot(ax, ay, az):
    return synth._so3_exp(np.array([ax, ay, az], np.float64))


def crafted_pair(rs, n, cam, kind="compared", cross=True):
    w, h, zfm = int(cam["w"]), int(cam["h"]), float(cam["zfm"])
    pp = np.array([cam["ppx"], cam["ppy"]], np.float64)
    Rt, tt = rot(0.02, -0.03, 0.015), np.array([0.05, -0.03, 0.02])          # key frame -> frame
    pix = np.stack([rs.uniform(2, w - 3, n), rs.uniform(2, h - 3, n)], 1)
    p_m = (pix - pp).astype(np.float32)
    ang = rs.uniform(0, 2 * np.pi, n)
    u_m = np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
    rho, s_rho = rs.uniform(0.3, 1.5, n), rs.uniform(0.02, 0.4, n)
    x = np.stack([p_m[:, 0] / rho / zfm, p_m[:, 1] / rho / zfm, 1 / rho], 1)
    y = x @ Rt.T + tt
    q = np.stack([y[:, 0] / y[:, 2] * zfm, y[:, 1] / y[:, 2] * zfm], 1) + rs.normal(0, 0.3, (n, 2))
    out = rs.rand(n) < 0.05
    q[out] += 15 * np.stack([np.cos(ang[out] + 1.0), np.sin(ang[out] + 1.0)], 1)
    extra = 7 if n >= 5 else 0                                                  # frame KeyLines the key frame never saw
    nf = n + extra
    perm = rs.permutation(nf)[:n]                                               # key-frame KeyLine i is frame KeyLine perm[i]
    fp = np.zeros((nf, 2), np.float32)
    fu = np.zeros((nf, 2), np.float32)
    frho, fs = rs.uniform(0.3, 1.5, nf), rs.uniform(0.02, 0.4, nf)
    fang = rs.uniform(0, 2 * np.pi, nf)
    fp[:] = np.stack([rs.uniform(2, w - 3, nf), rs.uniform(2, h - 3, nf)], 1) - pp
    fu[:] = np.stack([np.cos(fang), np.sin(fang)], 1)
    fp[perm] = q
    a2 = ang + rs.normal(0, 0.05, n)
    fu[perm] = np.stack([np.cos(a2), np.sin(a2)], 1)
    frho[perm] = 1 / y[:, 2]
    if n >= 65:                                                                 # a few points behind the camera in the scale sum
        frho[perm[rs.choice(n, max(1, n // 100), replace=False)]] *= -1
    m_id_f = perm.astype(np.int32)
    m_id_kf = np.full(nf, -1, np.int32)
    m_id_kf[perm] = np.arange(n)
    if n >= 65 and cross:
        # crossed links: to the partner of the nearest other key-frame KeyLine (often within dist_t) or of a random one (far)
        d2 = ((pix[:, None, :] - pix[None, :, :]) ** 2).sum(-1) + np.eye(n) * 1e9
        near = d2.argmin(1)
        cross = rs.rand(n) < 0.08
        far = rs.rand(n) < 0.5
        other = np.where(far, rs.randint(0, n, n), near)
        m_id_f[cross] = perm[other[cross]]
        cross_b = rs.rand(n) < 0.08
        d2f = ((q[:, None, :] - q[None, :, :]) ** 2).sum(-1) + np.eye(n) * 1e9
        other_b = np.where(rs.rand(n) < 0.5, rs.randint(0, n, n), d2f.argmin(1))
        m_id_kf[perm[cross_b]] = other_b[cross_b]
    if n >= 65:
        m_id_f[rs.rand(n) < 0.2] = -1
        m_id_kf[rs.rand(nf) < 0.2] = -1
    # poses: the start pose is the true motion off by a small rotation and translation
    KP, KPos, KK = rot(0.1, -0.2, 0.05), np.array([0.3, -0.1, 0.2]), 1.1
    dR, dt = rot(0.008, -0.006, 0.01), np.array([0.02, 0.015, -0.01])
    Pose = KP @ Rt.T @ dR
    Pos = KPos - KK * (Pose @ (tt + dt))
    kf = dict(p_m=p_m, u_m=u_m, rho=rho, s_rho=s_rho, m_id_f=m_id_f)
    fr = dict(p_m=fp, u_m=fu, rho=frho, s_rho=fs, m_id_kf=m_id_kf)
    return dict(kf=kf, fr=fr, kf_Pose=KP, kf_Pos=KPos, kf_K=np.float64(KK), Pose=Pose, Pos=Pos, K=np.float64(1.05), zfm=zfm, kind=kind)


def mutual_stats(pair, dist_t):
    """populations of the pruning passes, from the port's rule"""
    st = {}
    for kf_to_frame, tag in ((True, "kf"), (False, "fr")):
        col0 = pair["kf"]["m_id_f"] if kf_to_frame else pair["fr"]["m_id_kf"]
        col_d, _ = port.mutual_exclusion(pair, dist_t, True, kf_to_frame)
        col_k, c = port.mutual_exclusion(pair, dist_t, False, kf_to_frame)
        st["mutual_dropped_non_mutual"] = st.get("mutual_dropped_non_mutual", 0) + int((col_d != col_k).sum())
        st["mutual_failed_dist_" + tag] = int(((col_k != col0)).sum())
        oth = pair["fr"]["m_id_kf"] if kf_to_frame else pair["kf"]["m_id_f"]
        back = np.where(col0 >= 0, oth[np.maximum(col0, 0)], -1)
        st["mutual_passed_dist_" + tag] = int(((col_k >= 0) & (back >= 0) & (back != np.arange(len(col0)))).sum())
    return st


def case_list(n_pairs_compared, iters=(0, 10)):
    return [dict(pair=p, direction=d, iter_max=it, k_huber=kh, prune=pr, discard=1, dist_t=4.0)
            for p in n_pairs_compared for d in (0, 1) for kh in (0.0, 2.0) for it in iters for pr in (0, 3)]


def pack(pairs, cam, cases, refs, stats, seconds):
    rec = {f"cam_{k}": np.asarray(v) for k, v in cam.items()}
    rec["n_pairs"], rec["n_cases"] = np.int32(len(pairs)), np.int32(len(cases))
    for j, p in enumerate(pairs):
        pre = f"p{j}_"
        for k in port.LIST_FIELDS:
            rec[pre + "kf_" + k], rec[pre + "fr_" + k] = p["kf"][k], p["fr"][k]
        rec[pre + "kf_m_id_f"], rec[pre + "fr_m_id_kf"] = p["kf"]["m_id_f"].astype(np.int32), p["fr"]["m_id_kf"].astype(np.int32)
        for k in ("kf_Pose", "kf_Pos", "kf_K", "Pose", "Pos", "K"):
            rec[pre + k] = np.asarray(p[k], np.float64)
        rec[pre + "kind"] = np.array(p["kind"])
    for k in ("pair", "direction", "iter_max", "prune", "discard"):
        rec["case_" + k] = np.array([c[k] for c in cases], np.int32)
    for k in ("k_huber", "dist_t"):
        rec["case_" + k] = np.array([c[k] for c in cases], np.float64)
    for k in ("X", "W_X", "R_X", "ratio", "E", "E0", "Kp", "W_Kp"):
        rec["ref_" + k] = np.array([r[k] for r in refs], np.float64)
    for k in ("links", "inliers", "prune_counts"):
        rec["ref_" + k] = np.array([r[k] for r in refs], np.int32)
    for c, r in enumerate(refs):
        rec[f"case{c}_m_id_f"], rec[f"case{c}_m_id_kf"] = r["m_id_f"], r["m_id_kf"]
    keys = sorted(stats)
    rec["stat_names"], rec["stat_values"] = np.array(keys), np.array([stats[k] for k in keys], np.int64)
    rec["ref_seconds"] = np.array(seconds, np.float64)
    return rec


def run_cases(exe, rs, pairs, cam, cases, name, drop=False):
    """drop: a case on a knife edge is left out of `cases` (in place); otherwise it fails the whole set (-> None)."""
    refs, stats, seconds = [], {}, []
    for c, case in enumerate(list(cases)):
        got = check_case(exe, rs, pairs[case["pair"]], cam, case, f"{name} case {c} {case}")
        if got is None:
            if drop:
                cases.remove(case)
                continue
            return None
        ref, tr = got
        refs.append(ref)
        seconds.append(ref["seconds"])
        if tr.get("accepted", 0) and tr.get("rejected", 0):
            stats["accepted_and_rejected_in_one_call"] = stats.get("accepted_and_rejected_in_one_call", 0) + 1
        for k in ("reweighted", "unweighted", "unlinked_between", "scale_behind", "accepted", "rejected"):
            stats[k] = stats.get(k, 0) + tr.get(k, 0)
    return refs, stats, seconds


TIMING = dict(w=752, h=480, kn=16000, iter_max=10, k_huber=2.0, seed=7)


def timing_pair(params):
    """tools/keyframe_constraint_timing.py's pair: TIMING["kn"] KeyLines at 752x480 with the crafted lists' noise, outliers and dropped links
    (no crossed links: their nearest-neighbour search is quadratic) -> (pair, cam)."""
    cam = camera(TIMING["w"], TIMING["h"], params.ppx, params.ppy, params.zfx, params.zfy)
    return crafted_pair(np.random.RandomState(TIMING["seed"]), TIMING["kn"], cam, cross=False), cam


def timing_reference(exe):
    """The reference's one-core seconds (the median of 3 runs) and results for the timing pair, either direction."""
    from rebvo_amd import edgehip
    pair, cam = timing_pair(edgehip.euroc_params(TIMING["w"], TIMING["h"]))
    rec = {}
    for d in (0, 1):
        case = dict(direction=d, iter_max=TIMING["iter_max"], k_huber=TIMING["k_huber"], prune=0, discard=0, dist_t=0.0)
        runs = [run_ref(exe, pair, cam, case) for _ in range(3)]
        rec[f"timing_ref_seconds_dir{d}"] = np.float64(np.median([r["seconds"] for r in runs]))
        rec[f"timing_ref_X_dir{d}"], rec[f"timing_ref_ratio_dir{d}"] = runs[0]["X"], np.float64(runs[0]["ratio"])
        rec[f"timing_ref_links_dir{d}"] = np.int32(runs[0]["links"])
    rec["timing_kn"] = np.int32(TIMING["kn"])
    print("timing reference:", {k: (v.tolist() if np.ndim(v) else float(v)) for k, v in rec.items()})
    return rec


def crafted(exe):
    cam = camera(70, 50, 34.3, 25.6, 60.0, 62.0)
    sizes = [0, 1, 5, 65, 257, 600, 1030]
    for seed in range(40):
        rs = np.random.RandomState(seed)
        pairs = [crafted_pair(rs, n, cam, "compared" if n >= 65 else "few_links") for n in sizes]
        pairs[0]["kind"] = "no_links"
        nan = crafted_pair(rs, 65, cam, "nan_rho")
        for lst, col in ((nan["kf"], "m_id_f"), (nan["fr"], "m_id_kf")):
            lst["rho"] = lst["rho"].copy()
            lst["rho"][np.nonzero(lst[col] >= 0)[0][3]] = np.nan
        oob = crafted_pair(rs, 65, cam, "link_out_of_range")
        oob["kf"]["m_id_f"][np.nonzero(oob["kf"]["m_id_f"] >= 0)[0][5]] = len(oob["fr"]["rho"]) + 2
        oob["fr"]["m_id_kf"][np.nonzero(oob["fr"]["m_id_kf"] >= 0)[0][5]] = len(oob["kf"]["rho"])
        pairs += [nan, oob]
        compared = [j for j, p in enumerate(pairs) if p["kind"] == "compared"]
        cases = case_list(compared)
        got = run_cases(exe, rs, pairs, cam, cases, f"crafted seed {seed}")
        if got is None:
            continue
        refs, stats, seconds = got
        for j in compared:
            for k, v in mutual_stats(pairs[j], 4.0).items():
                stats[k] = stats.get(k, 0) + v
        missing = [k for k in REQUIRED if stats.get(k, 0) == 0]
        if not missing:
            break
        print(f"crafted seed {seed}: populations missing {missing}")
    else:
        raise SystemExit("crafted: no seed passes the screen and populates every branch")
    rec = pack(pairs, cam, cases, refs, stats, seconds)
    rec["seed"] = np.int32(seed)
    rec.update(timing_reference(exe))
    print(f"crafted: seed {seed}, {len(cases)} cases, stats {stats}")
    return rec


def chained_pairs(ref_root, tmp, w=256, h=192, n_frames=4, keep=(2, 3)):
    """-> (pairs of frame 0 as key frame against the frames `keep`, cam, the frames); tools/make_keyframe_depth_golden.py builds its
    chained fixture from the same pairs."""
    import keyframe_track_port as tport
    import make_keyframe_track_golden as tg
    from oracle import oracle
    texe = tg.build_driver(ref_root, tmp)
    params = oracle.euroc_params(w, h)
    orc = oracle.Oracle("ref", params)
    frames = []
    for k, (f, _, _) in enumerate(synth.billboard_sequence(w, h, n_frames)):
        _, nav = orc.process_frame(f, 0.05 * k)
        st = orc.seq_state()
        frames.append(dict(kl=orc.keylines(orc.cur_slot()).copy(), nav=nav.as_dict(), Pose=np.array(st.Pose[:]).reshape(3, 3),
                           Pos=np.array(st.Pos[:]), K=st.K, V=np.array(st.V[:])))
    orc.close()
    cam = camera(w, h, params.ppx, params.ppy, params.zfx, params.zfy)
    zf = np.float32(cam["zfm"])
    kf0 = frames[0]
    lst = lambda kl: {k: kl[k].copy() for k in port.LIST_FIELDS}   # noqa: E731
    m_id_f = np.arange(len(kf0["kl"]), dtype=np.int32)
    m_id_kf_prev = np.arange(len(kf0["kl"]), dtype=np.int32)
    pairs = []
    for k in range(1, n_frames):
        fr, old = frames[k], frames[k - 1]
        m = fr["kl"]["m_id"]
        m_id_kf = np.where(m >= 0, m_id_kf_prev[np.maximum(m, 0)], -1).astype(np.int32)
        Pose, Pos = tport.local_pose(old["Pose"], np.array(fr["nav"]["Rot"]).reshape(3, 3), old["Pos"], fr["V"], old["K"])
        case = dict(kf_p_m=kf0["kl"]["p_m"], kf_p_id=kf0["kl"]["p_id"], kf_n_id=kf0["kl"]["n_id"], kf_m_id_f=m_id_f, new_p_m=fr["kl"]["p_m"],
                    new_p_id=fr["kl"]["p_id"], new_n_id=fr["kl"]["n_id"], new_m_id=m, new_m_id_kf=m_id_kf, old_kn=np.int32(len(old["kl"])),
                    kf_Pose=kf0["Pose"], kf_Pos=kf0["Pos"], Pose=Pose, Pos=Pos, zf=zf, dist_thresh=np.float64(10.0),
                    dist_tolerance=np.float64(0.0), augmentate=np.int32(1))
        r = tg.run_ref(texe, case)
        m_id_f, m_id_kf_prev = r["ref_m_id_f_1"].copy(), r["ref_m_id_kf_1"].copy()
        if k in keep:
            pairs.append(dict(kf=dict(lst(kf0["kl"]), m_id_f=m_id_f.copy()), fr=dict(lst(fr["kl"]), m_id_kf=m_id_kf_prev.copy()),
                              kf_Pose=kf0["Pose"], kf_Pos=kf0["Pos"], kf_K=np.float64(kf0["K"]), Pose=fr["Pose"], Pos=fr["Pos"], K=np.float64(fr["K"]),
                              zfm=float(cam["zfm"]), kind="compared"))
    return pairs, cam, frames


def chained(exe, ref_root, tmp):
    pairs, cam, _ = chained_pairs(ref_root, tmp)
    cases = case_list(range(len(pairs)), iters=(10,))
    refs, stats, seconds = run_cases(exe, np.random.RandomState(1), pairs, cam, cases, "chained", drop=True)
    if len(cases) < 8 or len({(c["direction"], c["k_huber"] > 0) for c in cases}) < 4:
        raise SystemExit(f"chained: only {len(cases)} cases passed the knife-edge screen")
    print(f"chained: kn {[(len(p['kf']['rho']), len(p['fr']['rho'])) for p in pairs]} links {[r['links'] for r in refs]} stats {stats} "
          f"ref seconds {np.round(seconds, 5).tolist()}")
    return pack(pairs, cam, cases, refs, stats, seconds)


def write(path, rec):
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= SIZE_LIMIT, (path, size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF"), help="the reference tree (or $REBVO_REF)")
    ap.add_argument("--only", choices=("crafted", "chained"))
    a = ap.parse_args()
    if not a.ref:
        raise SystemExit("give --ref /path/to/reference (or set REBVO_REF)")
    os.makedirs(GOLD, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="keyframe_constraint_ref_") as tmp:
        exe = build_driver(a.ref, tmp)
        if a.only != "chained":
            write(os.path.join(GOLD, "crafted.npz"), crafted(exe))
        if a.only != "crafted":
            write(os.path.join(GOLD, "chained.npz"), chained(exe, a.ref, tmp))


if __name__ == "__main__":
    main()
