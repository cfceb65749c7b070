#!/usr/bin/env python3
"""Generate tests/golden/keyframe_reloc/*.npz from the REFERENCE's own kfvo::OptimizePosGT (src/mtracklib/kfvo.cpp:58-112, with
Minimizer_RV_KF, TryVelRot, Calc_f_J_Complete and optimizeScale as it calls them).

Build machine only (needs the reference tree and oracle/_ref/libreforacle.so from `make -C oracle`):
    python tools/make_keyframe_reloc_golden.py [--ref /path/to/reference]

tools/keyframe_reloc_ref_driver.cpp is compiled into a temporary directory outside the repository, with the reference's kfvo.cpp and
global_tracker.cpp included in place (nothing is written under oracle/, no reference source is copied).  A fixture holds the KeyLines'
eleven numbers, poses, camera, per case the arguments and what the reference returned: mnum, every m_id_f, r = F / F0, X, RRV, K, Pose, Pos.

  crafted.npz   70x50; key-frame lists of 0, 1, 5, 65, 257, 600 and 1030 KeyLines.  A query is its key frame seen from a pose a few
                hundredths away (the points moved in 3-D, 0.3 px of noise), handed over with a pose that is off by a little more, so the
                minimiser has a way to go; K != K_t, K_t != 1; one Pose_t is not orthonormal.  A tenth of the query is pushed off the image;
                runs of in-image KeyLines whose gradient is turned by 90 degrees (Calc_f_J_Complete rejects them: the `fi` carry) lie across
                KeyLines 60..70 (a 64-lane boundary), 250..262 and 505..520 (256-KeyLine tile boundaries); key-frame KeyLines 10 and 11 are
                the same segment (a tie for every cell: the greater index wins); iter_max 6 and 0; a query that matches nothing (every
                gradient turned: Kp = 1); a query whose points all lie behind the camera (every q1[2] <= 0: Kp = 1).  Degenerate inputs
                (NaN rho, an empty query) are stored as inputs only: the reference is not run on them.
  chained.npz   the consecutive frames of tests/golden/keyframe_covis/chained.npz (synth.billboard_sequence at 256x192 through the
                reference's pipeline): its first three as key frames, its last as the query.

Gates (nothing is written otherwise), for every case: the port (tests/keyframe_reloc_port.py, the whole rule in numpy) equals the
reference on mnum and every m_id_f exactly and on every fp64 output to 1e-13 relative; re-run with plain sequential sums instead of the
pairwise ones it takes the same accept / reject decision at every LM step and lands within 1/100 of the tests' tolerances (a case that
flips with the summation order is disqualified, not the device); every case whose key frame has 65 KeyLines or more, except the two made
to match nothing, has mnum >= 30.  A list of 1 or 5 KeyLines cannot have 30 links (six unknowns from fewer rows: RRV and the last digits of X
are rounding noise): such a case is marked not numeric, only its links, mnum and evals are compared, exactly.  Across crafted.npz the
populations accepted step, rejected step, off-image, residual carried across a tile and across a wave, reweighted, tie cell and Kp fallback
are non-zero.  Kp, evals and accepted are not values OptimizePosGT returns: the fixture holds the port's, which the first gate ties to it."""
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
import keyframe_covis_port as cport  # noqa: E402
import keyframe_reloc_port as port  # noqa: E402
import make_keyframe_covis_golden as cgen  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "keyframe_reloc")
SIZE_LIMIT = cgen.SIZE_LIMIT
KNS = [0, 1, 5, 65, 257, 600, 1030]
RUNS = [(60, 70), (250, 262), (505, 520)]


def build_driver(ref, tmp):
    inc = os.path.join(ROOT, "oracle", "_ref", "inc")
    lib = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(lib, "libreforacle.so")):
        raise SystemExit("oracle/_ref/libreforacle.so is missing: run `make -C oracle` first")
    pre = os.path.join(tmp, "prelude.h")
    with open(pre, "w") as f:
        f.write(cgen.PRELUDE)
    exe = os.path.join(tmp, "kf_reloc_driver")
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-access-control", "-w", "-include", pre,
           "-I" + inc, "-I" + os.path.join(ref, "include"), "-I" + ref,
           os.path.join(ROOT, "tools", "keyframe_reloc_ref_driver.cpp"), os.path.join(ref, "src", "mtracklib", "keyframe.cpp"),
           os.path.join(ref, "src", "visualizer", "depth_filler.cpp"),
           "-L" + lib, "-Wl,-rpath," + lib, "-lreforacle", "-lm", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run_ref(exe, kfs, cam, a, pairs):
    M, w, h = len(kfs), int(cam["w"]), int(cam["h"])
    payload = np.array([M, w, h, a["field_radius"], a["iter_max"], len(pairs)], np.int32).tobytes()
    payload += np.array([a["field_min_mod"], cam["ppx"], cam["ppy"], cam["zfx"], cam["zfy"]], np.float32).tobytes()
    payload += np.array([a["rew_dis"], a["rho_tol"], a["s_rho_q"]], np.float64).tobytes()
    for kf in kfs:
        payload += np.array([len(kf["n_m"]), 0], np.int32).tobytes()
        payload += np.concatenate([np.asarray(kf["Pose"]).ravel(), kf["Pos"], [kf["K"]]]).astype(np.float64).tobytes()
        payload += cgen.records(kf).tobytes()
    payload += np.array(pairs, np.int32).reshape(-1, 2).tobytes()
    out = subprocess.run([exe], input=payload, check=True, capture_output=True).stdout
    res, at = [], 0
    for q, t in pairs:
        mnum, kn = np.frombuffer(out, np.int32, 2, at)
        d = np.frombuffer(out, np.float64, 56, at + 8)
        mid = np.frombuffer(out, np.int32, kn, at + 8 + 448).copy()
        at += 8 + 448 + 4 * int(kn)
        assert kn == len(kfs[q]["n_m"]) and mnum == (mid >= 0).sum()
        res.append(dict(mnum=int(mnum), r=d[0], K=d[1], X=d[2:8].copy(), RRV=d[8:44].reshape(6, 6).copy(), Pose=d[44:53].reshape(3, 3).copy(),
                        Pos=d[53:56].copy(), m_id_f=mid))
    assert at == len(out), (at, len(out))
    return res


def moved_query(rs, kf, cam, W, t, W0, t0, K, turn_all=False, behind=False):
    """The key frame's points seen from (exp(W), t) in its frame, 0.3 px of noise; handed over with the pose (exp(W0), t0) and scale K."""
    kn = len(kf["n_m"])
    zfm = float(cam["zfm"])
    R = cgen.rot(*W)
    z = 1.0 / kf["rho"]
    P = np.stack([kf["p_m"][:, 0].astype(np.float64) * z / zfm, kf["p_m"][:, 1].astype(np.float64) * z / zfm, z], 1)
    Pq = (P - np.asarray(t)) @ R                      # R^T (P - t)
    p_m = (zfm * Pq[:, :2] / Pq[:, 2:3] + rs.normal(0, 0.3, (kn, 2))).astype(np.float32)
    q = {k: np.array(kf[k]) for k in cport.FIELDS}
    q["rho"] = 1.0 / Pq[:, 2]
    off = rs.rand(kn) < 0.1
    p_m[off, 0] = -float(cam["ppx"]) - 4.0            # off the image under every pose used here
    q["p_m"] = p_m
    q["c_p"] = (p_m + np.array([cam["ppx"], cam["ppy"]], np.float32)).astype(np.float32)
    turned = np.zeros(kn, bool)
    for a, b in RUNS:
        turned[a:min(b, kn)] = True
    if turn_all:
        turned[:] = True
    for k in ("m_m", "u_m"):
        v = q[k].copy()
        v[turned] = np.stack([-q[k][turned, 1], q[k][turned, 0]], 1)
        q[k] = v
    if behind:
        q["rho"] = -q["rho"]
    R0 = cgen.rot(*W0)
    Pt = np.asarray(kf["Pose"], np.float64)
    q.update(Pose=Pt @ R0, Pos=np.asarray(kf["Pos"]) + (Pt @ np.asarray(t0)) * K, K=np.float64(K))
    return q, int(off.sum()), int((turned & ~off).sum())


def crafted(exe):
    w, h = 70, 50
    cam = cgen.camera(w, h, 34.3, 25.6, 60.0, 62.0)
    rs = np.random.RandomState(7)
    poses = [(cgen.rot(0.1 * j, -0.05 * j, 0.02 * j), [0.1 * j, -0.2, 0.05 * j], 0.8 + 0.07 * j) for j in range(len(KNS))]
    kfs, cases = [], []
    pop = dict(off_image=0, carried=0, tie=0, kp_fallback=0)
    for j, kn in enumerate(KNS):
        kf = cgen.crafted_keyframe(rs, kn, cam, *poses[j])
        if kn >= 65:
            for k in cport.FIELDS:                           # KeyLines 10 and 11: one segment twice
                kf[k][11] = kf[k][10]
            pop["tie"] += 1
        if j == 4:
            kf["Pose"] = kf["Pose"] + 1e-6 * np.arange(9).reshape(3, 3)      # not orthonormal: SO3<>(Pose_t) coerces it
        kfs.append(kf)
    base = dict(field_radius=5, field_min_mod=0.0, iter_max=6, rew_dis=2.0, rho_tol=1.5, s_rho_q=0.39)
    groups = []
    for a in (base, dict(base, iter_max=0)):
        qs, pairs = [], []
        for j, kn in enumerate(KNS):
            W, t = (0.01, -0.015, 0.02), (0.02, -0.01, 0.03)
            W0, t0 = ((0.02, -0.025, 0.03), (0.035, -0.02, 0.045)) if a["iter_max"] else (W, t)   # (iter_max 0 evaluates once: at the pose itself)
            q, n_off, n_turn = moved_query(rs, kfs[j], cam, W, t, W0, t0, K=1.3 - 0.05 * j)
            pop["off_image"] += n_off
            pop["carried"] += n_turn
            qs.append(q)
            pairs.append((len(KNS) + len(qs) - 1, j))
        groups.append((a, qs, pairs, "moved"))
    q_none, _, _ = moved_query(rs, kfs[3], cam, (0, 0, 0), (0, 0, 0), (0.01, 0, 0), (0.01, 0, 0), 1.0, turn_all=True)
    groups.append((base, [q_none], [(len(KNS), 3)], "no_match"))
    q_behind, _, _ = moved_query(rs, kfs[4], cam, (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, behind=True)
    groups.append((dict(base, rho_tol=1e3, s_rho_q=1e3), [q_behind], [(len(KNS), 4)], "behind"))
    rec = {f"cam_{k}": np.asarray(v) for k, v in cam.items()}
    rec["n_kf"] = np.int32(len(kfs))
    for m, kf in enumerate(kfs):
        for k, v in kf.items():
            rec[f"kf{m}_{k}"] = np.asarray(v)
    c = 0
    for a, qs, pairs, kind in groups:
        res = run_ref(exe, kfs + qs, cam, a, pairs)
        for (qi, t), r in zip(pairs, res):
            c = store_case(rec, c, cam, a, qs[qi - len(kfs)], kfs[t], t, r, kind, pop)
    rec["n_cases"] = np.int32(c)
    # degenerate inputs, stored as inputs only
    nanq = {k: np.array(v) for k, v in groups[0][1][5].items()}
    nanq["rho"] = nanq["rho"].copy()
    nanq["rho"][[5, 300]] = np.nan
    for k, v in nanq.items():
        rec[f"nan_query_{k}"] = np.asarray(v)
    rec["nan_query_kf"] = np.int32(5)
    need = ("accepted", "rejected", "off_image", "carried", "carried_across_tile", "carried_across_wave", "reweighted", "tie", "kp_fallback")
    missing = [k for k in need if pop.get(k, 0) == 0]
    assert not missing, (missing, pop)
    rec.update(pop_names=np.array(sorted(pop)), pop_values=np.array([pop[k] for k in sorted(pop)], np.int64))
    print("crafted:", c, "cases; populations", pop)
    return rec


TOL = dict(X=(1e-9, 1e-12), Pose=(1e-9, 1e-12), Pos=(1e-9, 1e-12), r=(1e-9, 0), Kp=(1e-9, 0), K=(1e-9, 0), RRV=(1e-7, 0))   # the tests' tolerances


def rel(a, b, scale=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin)
    if not fin.any():
        return 0.0
    s = np.abs(b[fin]).max() if scale is None else scale
    return float(np.abs(a[fin] - b[fin]).max() / s) if s > 0 else float(np.abs(a[fin] - b[fin]).max())


def store_case(rec, c, cam, a, q, kf, t, r, kind, pop):
    import collections
    kn_t = len(kf["n_m"])
    if len(q["n_m"]) == 0:   # the reference leaves X and RRV unset for an empty query and goes on with W0 / BRelPos: the library returns those
        r = dict(r, X=port.request(q["Pose"], q["Pos"], q["K"], kf["Pose"], kf["Pos"], kf["K"])[0], RRV=np.zeros((6, 6)))
    scale = max(np.linalg.norm(kf["Pos"]), np.linalg.norm(r["X"][:3]) * r["K"], 1e-300)
    # gate 1: the port — the whole rule, pairwise sums — equals the reference: links exactly, every fp64 output to 1e-13 relative
    st = collections.Counter()
    w = port.relocalize(q, kf, cam, a, True, st)
    assert w["mnum"] == r["mnum"] and np.array_equal(w["m_id_f"], r["m_id_f"]), (c, "links")
    err = dict(X=rel(w["X"], r["X"]), RRV=rel(w["RRV"], r["RRV"]), r=rel(w["r"], r["r"]), K=rel(w["K"], r["K"]), Pose=rel(w["Pose"], r["Pose"], 1.0),
               Pos=rel(w["Pos"], r["Pos"], scale))
    # a key frame of 1 or 5 KeyLines cannot have 30 links: 6 unknowns from fewer rows, RRV and the last digits of X are rounding noise.  Such a
    # case is not numerically compared: its links, mnum and evals are (they are exact), its fp64 outputs are stored for the record only.
    numeric = not (kind == "moved" and 0 < len(q["n_m"]) and r["mnum"] < 30)
    assert not numeric or max(err.values()) <= 1e-13, (c, err)
    # gate 2: with plain sequential sums the port takes the same accept / reject decision at every step and lands within 1/100 of the tests'
    # tolerances: a case that flips with the summation order is disqualified, not the device
    v = port.relocalize(q, kf, cam, a, False)
    assert np.array_equal(v["m_id_f"], w["m_id_f"]) and (not numeric or v["decisions"] == w["decisions"]), (c, "flips with the summation order")
    for k, (rt, at) in TOL.items() if numeric else ():
        sc = scale if k == "Pos" else None
        got, want = np.asarray(v[k], np.float64), np.asarray(w[k], np.float64)
        fin = np.isfinite(want)
        ref = np.abs(want[fin]) if sc is None else sc
        assert np.all(np.abs(got[fin] - want[fin]) <= (at + rt * ref) / 100), (c, k, "moves with the summation order")
    if kind in ("no_match", "behind"):
        assert w["Kp"] == 1.0 and (r["mnum"] == 0) == (kind == "no_match") and (kind != "behind" or (r["mnum"] > 0 and w["used"] == 0)), (kind, r["mnum"], w["used"])
        pop["kp_fallback"] += 1
    elif kn_t >= 65:
        assert r["mnum"] >= 30 and numeric, (c, kn_t, r["mnum"])
    for k in ("accepted", "rejected", "reweighted", "carried_across_tile", "carried_across_wave"):
        pop[k] = pop.get(k, 0) + st[k]
    for k, v2 in q.items():
        rec[f"case{c}_q_{k}"] = np.asarray(v2)
    rec[f"case{c}_t"] = np.int32(t)
    rec[f"case{c}_kind"] = np.array(kind)
    rec[f"case{c}_numeric"] = np.int32(numeric)
    for k, v2 in a.items():
        rec[f"case{c}_arg_{k}"] = np.asarray(v2, np.int32 if k in ("field_radius", "iter_max") else np.float64)
    for k in ("r", "K", "X", "RRV", "Pose", "Pos"):
        rec[f"case{c}_ref_{k}"] = np.asarray(r[k], np.float64)
    # what the reference does not return: Kp (K = K_t Kp alone), the evaluations and the accepted steps — the port's, which gate 1 ties to it
    rec[f"case{c}_ref_Kp"] = np.float64(w["Kp"])
    rec[f"case{c}_ref_evals"] = np.int32(w["evals"])
    rec[f"case{c}_ref_accepted"] = np.int32(w["accepted"])
    rec[f"case{c}_ref_mnum"] = np.int32(r["mnum"])
    rec[f"case{c}_ref_m_id_f"] = r["m_id_f"].astype(np.int16)
    print(f"  case {c} ({kind}): kf {t} kn_t {kn_t} kn_q {len(q['n_m'])} iter_max {a['iter_max']} mnum {r['mnum']} r {r['r']:.6f} Kp {w['Kp']:.6f} "
          f"accepted {w['accepted']} port-ref {max(err.values()):.1e}")
    return c + 1


def chained(exe):
    f = cport.load_fixture(os.path.join(ROOT, "tests", "golden", "keyframe_covis", "chained.npz"))
    cam = f["cam"]
    kfs = [dict(k) for k in f["kfs"][:3]]
    for j, k in enumerate(kfs):
        k["K"] = np.float64(float(k["K"]) * (1.1, 0.9, 1.2)[j])
    q = dict(f["kfs"][4])
    q["K"] = np.float64(1.05)
    rec = {f"cam_{k}": np.asarray(v) for k, v in cam.items()}
    rec["n_kf"] = np.int32(3)
    for m, kf in enumerate(kfs):
        for k, v in kf.items():
            rec[f"kf{m}_{k}"] = np.asarray(v)
    c = 0
    pop = dict(kp_fallback=0)
    for it in (6, 0):
        a = dict(field_radius=40, field_min_mod=0.0, iter_max=it, rew_dis=2.0, rho_tol=3.0, s_rho_q=float(np.quantile(q["s_rho"], 0.9)))
        pairs = [(3, t) for t in range(3)]
        for (qi, t), r in zip(pairs, run_ref(exe, kfs + [q], cam, a, pairs)):
            c = store_case(rec, c, cam, a, q, kfs[t], t, r, "moved", pop)
    rec["n_cases"] = np.int32(c)
    print("chained:", c, "cases")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF", "/root/reference"))
    a = ap.parse_args()
    os.makedirs(GOLD, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="keyframe_reloc_ref_") as tmp:
        exe = build_driver(a.ref, tmp)
        recs = [("crafted.npz", crafted(exe)), ("chained.npz", chained(exe))]
    for name, rec in recs:                                # (every gate has passed)
        cgen.write(os.path.join(GOLD, name), rec)


if __name__ == "__main__":
    main()
