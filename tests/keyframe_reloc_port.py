"""numpy restatement of what kfvo::OptimizePosGT (src/mtracklib/kfvo.cpp:58-112) does AROUND its minimisation, in the reference's types and
order of operations: the request it hands to Minimizer_RV_KF (:62-68, :74), kfvo::optimizeScale (:222-260, with kfvo::unProject / project,
kfvo.h:42-48) and the pose it returns (:89-96).  fp64 throughout; a matrix product is a dot product per element, summed from 0 in index
order (TooN); optimizeScale's two sums are SERIAL in KeyLine order, as the reference's `+=` are.

The first half of the module is everything AROUND the minimisation (request, optimize_scale, finish); the second half restates the
minimisation itself — kfvo::Minimizer_RV_KF with kfvo::TryVelRot and Calc_f_J_Complete — so that relocalize() is the whole rule.
tools/make_keyframe_reloc_golden.py holds it to the reference (links exact, fp64 outputs to 1e-13) before it writes a fixture."""
import numpy as np

from keyframe_constraint_port import matmul, matvec, so3_coerce, so3_exp, so3_ln


def request(Pose, Pos, K, Pose_t, Pos_t, K_t):
    """The query's (Pose, Pos, K) against key frame t's -> (X0 = [BRelPos, W0], Kr): kfvo.cpp:62-68 and the Kr of :74."""
    Pose, Pose_t = np.asarray(Pose, np.float64).reshape(3, 3), np.asarray(Pose_t, np.float64).reshape(3, 3)
    d = np.asarray(Pos, np.float64) - np.asarray(Pos_t, np.float64)
    BRelRot = matmul(Pose_t.T, Pose)
    BRelPos = matvec(Pose_t.T, d) / float(K)          # by the QUERY's K
    return np.concatenate([BRelPos, so3_ln(BRelRot)]), float(K) / float(K_t)


def optimize_scale(q, kf, m_id_f, R, p, zfm):
    """kfvo::optimizeScale(mkf, et, BRelRot = R, BRelPos = p) -> (Kp, rTr0, rTr, used): q the query's p_m [kn][2], rho, s_rho; kf the key
    frame's rho, s_rho; m_id_f [kn] the links."""
    rTr = rTr0 = 0.0
    used = 0
    zfm = float(zfm)
    with np.errstate(all="ignore"):
        for i in range(len(m_id_f)):
            b = int(m_id_f[i])
            if b < 0:
                continue
            x, y, rho = float(q["p_m"][i][0]), float(q["p_m"][i][1]), float(q["rho"][i])
            ir = 1 / rho
            u = np.array([(x / zfm) * ir, (y / zfm) * ir, 1.0 * ir])                  # unProject
            P = matvec(R, u) + p
            q2 = 1.0 * (1 / P[2])                                                       # project(...)[2]
            if q2 > 0:
                s, sb = float(q["s_rho"][i]), float(kf["s_rho"][b])
                v = s * s * 1.0 * 1.0 + sb * sb
                rTr0 += q2 * q2 / v
                rTr += q2 * float(kf["rho"][b]) / v
                used += 1
    Kp = rTr0 / rTr if (rTr0 > 0 and rTr > 0) else 1.0
    return Kp, rTr0, rTr, used


def finish(Pose_t, Pos_t, K_t, X, Kp):
    """kfvo.cpp:93-96 -> (K, Pose, Pos)."""
    Pc = so3_coerce(np.asarray(Pose_t, np.float64).reshape(3, 3))
    K = float(K_t) * float(Kp)
    Pose = matmul(Pc, so3_exp(X[3:6]))
    Pos = matvec(Pc, np.asarray(X[0:3], np.float64)) * K + np.asarray(Pos_t, np.float64)
    return K, Pose, Pos


def relocalize_around(q, q_pose, kf, kf_pose, zfm, X, m_id_f):
    """Everything of the rule but the minimisation, for one pair: q / kf dicts of KeyLine arrays, q_pose / kf_pose (Pose, Pos, K), X and
    m_id_f as the minimisation left them -> dict(X0, Kr, mnum, Kp, K, Pose, Pos, used)."""
    X0, Kr = request(*q_pose, *kf_pose)
    Kp, rTr0, rTr, used = optimize_scale(q, kf, m_id_f, so3_exp(X[3:6]), np.asarray(X[0:3], np.float64), zfm)
    K, Pose, Pos = finish(*kf_pose, X, Kp)
    return dict(X0=X0, Kr=Kr, mnum=int((np.asarray(m_id_f) >= 0).sum()), Kp=Kp, K=K, Pose=Pose, Pos=Pos, used=used, rTr0=rTr0, rTr=rTr)


def empty_query(q_pose, kf_pose):
    """What the call returns for a query without KeyLines: X = X0, RRV = 0, score_ratio = 0, mnum = 0, Kp = 1."""
    X0, Kr = request(*q_pose, *kf_pose)
    K, Pose, Pos = finish(*kf_pose, X0, 1.0)
    return dict(X=X0, Kp=1.0, K=K, Pose=Pose, Pos=Pos, mnum=0, score_ratio=0.0)


FIELDS = ("p_m", "c_p", "u_m", "m_m", "n_m", "rho", "s_rho")
ARGS = ("field_radius", "field_min_mod", "iter_max", "rew_dis", "rho_tol", "s_rho_q")


def load_fixture(path):
    """tests/golden/keyframe_reloc/*.npz (tools/make_keyframe_reloc_golden.py) -> dict(cam, kfs, cases, pop); a case holds the query `q`
    (KeyLines, Pose, Pos, K), the key frame's index `t`, `kind`, `args` and `ref`: what the reference's OptimizePosGT returned."""
    z = np.load(path)
    f = dict(cam={k[4:]: z[k] for k in z.files if k.startswith("cam_")})
    f["kfs"] = [{k: z[f"kf{m}_{k}"] for k in FIELDS + ("Pose", "Pos", "K")} for m in range(int(z["n_kf"]))]
    f["cases"] = []
    for c in range(int(z["n_cases"])):
        f["cases"].append(dict(q={k: z[f"case{c}_q_{k}"] for k in FIELDS + ("Pose", "Pos", "K")}, t=int(z[f"case{c}_t"]), kind=str(z[f"case{c}_kind"]),
                               numeric=bool(z[f"case{c}_numeric"]),
                               args={k: z[f"case{c}_arg_{k}"].item() for k in ARGS},
                               ref={k: z[f"case{c}_ref_{k}"] for k in ("r", "K", "Kp", "X", "RRV", "Pose", "Pos", "mnum", "m_id_f", "evals", "accepted")}))
    f["pop"] = dict(zip(z["pop_names"].tolist(), z["pop_values"].tolist())) if "pop_names" in z.files else {}
    if "nan_query_rho" in z.files:
        f["nan_query"] = dict(q={k: z[f"nan_query_{k}"] for k in FIELDS + ("Pose", "Pos", "K")}, t=int(z["nan_query_kf"]))
    return f


# ---- the minimisation: kfvo::Minimizer_RV_KF<double,false> (kfvo.cpp:1679-1825) with kfvo::TryVelRot<double,true,true,false> (:1389-1668)
# and global_tracker::Calc_f_J_Complete<double> (global_tracker.cpp:116-165), vectorised over the KeyLines but for the `fi` carry ----------
def _sum(v, pairwise):
    """Ne10::DotProduct's sum: pairwise adds (numpy's blocked pairwise sum stands for it), or one running sum in KeyLine order."""
    v = np.asarray(v, np.float64)
    if len(v) == 0:
        return 0.0
    return float(np.sum(v)) if pairwise else float(np.cumsum(v)[-1])


def try_vel_rot(X, q, kf, field_ikl, cam, Kr, match_mod, match_cang, rho_tol, s_rho_min, k_huber, resid, max_r, pairwise=True, stats=None):
    """One evaluation -> (score, JtJ, JtF, resid_new, m_id_f).  resid: DResidual of the last accepted evaluation."""
    import keyframe_constraint_port as kc
    kn = len(q["n_m"])
    w, h, zfm = int(cam["w"]), int(cam["h"]), float(cam["zfm"])
    R = kc.so3_exp(X[3:6])
    V = np.asarray(X[0:3], np.float64)
    rho0 = np.asarray(q["rho"], np.float64)
    s_rho = np.asarray(q["s_rho"], np.float64)
    with np.errstate(all="ignore"):
        z = 1.0 / rho0
        zz = z / zfm
        P0 = np.stack([zz * q["p_m"][:, 0].astype(np.float64), zz * q["p_m"][:, 1].astype(np.float64), z], 1)
        Pt = np.stack([(R[i, 0] * P0[:, 0] + R[i, 1] * P0[:, 1]) + R[i, 2] * P0[:, 2] + V[i] for i in range(3)], 1)
        rho_p = 1.0 / Pt[:, 2]
        pix, piy = (zfm * rho_p) * Pt[:, 0], (zfm * rho_p) * Pt[:, 1]
        px, py = pix + float(cam["ppx"]), piy + float(cam["ppy"])
        xi, yi = np.floor(px + 0.5), np.floor(py + 0.5)            # (int)(x + 0.5): truncation == floor wherever the in-image test passes
        skip = s_rho > s_rho_min
        inside = ~skip & (xi >= 1) & (yi >= 1) & (xi < w - 1) & (yi < h - 1)
        weight = np.ones(kn)
        big = np.abs(resid) > k_huber
        weight[big] = k_huber / np.abs(resid[big])
        ikf = np.full(kn, -1, np.int64)
        ikf[inside] = field_ikl[yi[inside].astype(np.int64), xi[inside].astype(np.int64)]
        hit = ikf >= 0
        b = np.where(hit, ikf, 0)
        m_m, n_m = q["m_m"], q["n_m"]
        cang = ((m_m[:, 0] * kf["m_m"][b, 0] + m_m[:, 1] * kf["m_m"][b, 1]) / n_m).astype(np.float64)           # float products and quotient
        rho_t = rho_p / Kr
        rej = (cang < match_cang) | (np.abs(n_m / kf["n_m"][b] - np.float32(1)).astype(np.float64) > match_mod) | \
              (np.abs(rho_t - kf["rho"][b]) > rho_tol * (kf["s_rho"][b] + s_rho * rho_t / rho0))
        match = hit & ~rej
        fi = (px - kf["c_p"][b, 0].astype(np.float64)) * kf["u_m"][b, 0].astype(np.float64) + \
             (py - kf["c_p"][b, 1].astype(np.float64)) * kf["u_m"][b, 1].astype(np.float64)
    # DResidualNew: the matched KeyLine's own fi; an in-image KeyLine without a match inherits the last matched one's (0 before the first)
    resid_new = np.array(resid, np.float64).copy()
    idx = np.where(match, np.arange(kn), -1)
    last = np.maximum.accumulate(idx) if kn else idx
    carried = np.where(last >= 0, fi[np.maximum(last, 0)], 0.0)
    off = ~skip & ~inside
    resid_new[inside] = carried[inside]
    resid_new[off] = max_r
    fm = np.zeros(kn)
    fm[off] = max_r
    fm[inside & ~match] = max_r
    fm[match] = fi[match]
    dfx = np.where(match, kf["u_m"][b, 0].astype(np.float64), 0.0)
    dfy = np.where(match, kf["u_m"][b, 1].astype(np.float64), 0.0)
    ev = ~skip
    fm = np.where(ev, fm * weight, 0.0)
    dfx, dfy = dfx * weight, dfy * weight
    with np.errstate(all="ignore"):
        t0 = zfm * rho_p
        J = np.zeros((kn, 6))
        J[:, 0], J[:, 1] = t0 * dfx, t0 * dfy
        J[:, 2] = (rho_p * pix) * dfx + (rho_p * piy) * dfy
        J[:, 3] = J[:, 1] * Pt[:, 2] + J[:, 2] * Pt[:, 1]
        J[:, 4] = J[:, 0] * Pt[:, 2] + J[:, 2] * Pt[:, 0]
        J[:, 5] = -1.0 * (J[:, 0] * Pt[:, 1]) + J[:, 1] * Pt[:, 0]
        qvel = zfm * dfx * V[0] + zfm * dfy * V[1] + (pix * dfx + piy * dfy) * V[2]
        q_rho = np.sqrt(s_rho * qvel * s_rho * qvel + 1)
        J = np.where(ev[:, None], J / q_rho[:, None], 0.0)
        fm = np.where(ev, fm / q_rho, 0.0)
    JtJ = np.zeros((6, 6))
    JtF = np.zeros(6)
    for i in range(6):
        for j in range(i, 6):
            JtJ[i, j] = _sum(J[:, i] * J[:, j], pairwise)
        JtF[i] = _sum(J[:, i] * fm, pairwise)
    for i in range(2):
        JtF[i + 2] = -JtF[i + 2]
        for j in range(2):
            JtJ[i, j + 2] = -JtJ[i, j + 2]
            JtJ[i + 2, j + 4] = -JtJ[i + 2, j + 4]
    JtJ = np.triu(JtJ) + np.triu(JtJ, 1).T
    if stats is not None:
        stats["off_image"] += int(off.sum()); stats["carried"] += int((inside & ~match).sum()); stats["reweighted"] += int((big & ev).sum())
        stats["matched"] += int(match.sum()); stats["skipped"] += int(skip.sum())
        inh = inside & ~match & (last >= 0)                  # inherits a residual; from another tile / wave when it is the first of its own
        k = np.arange(kn)
        stats["carried_across_tile"] += int((inh & (k % 256 == 0)).sum()); stats["carried_across_wave"] += int((inh & (k % 64 == 0) & (k % 256 != 0)).sum())
    return _sum(fm * fm, pairwise), JtJ, JtF, resid_new, np.where(match, ikf, -1).astype(np.int32)


def minimizer_rv_kf(X0, q, kf, field_ikl, cam, Kr, rho_tol, iter_max, rew_dis, s_rho_q, max_r, match_mod=5.0, match_ang=30.0 * np.pi / 180.0,
                    pairwise=True, stats=None):
    """-> dict(X, RRV, r, F, F0, m_id_f, evals, accepted, decisions).  An empty query returns X0, zeros and r = 0 (the library's convention)."""
    import collections
    import math
    import keyframe_constraint_port as kc
    stats = collections.Counter() if stats is None else stats
    X = np.array(X0, np.float64)
    kn = len(q["n_m"])
    if kn == 0:
        return dict(X=X, RRV=np.zeros((6, 6)), r=0.0, F=0.0, F0=0.0, m_id_f=np.zeros(0, np.int32), evals=0, accepted=0, decisions=[])
    cang = math.cos(match_ang)
    ev = lambda Xe, res: try_vel_rot(Xe, q, kf, field_ikl, cam, Kr, match_mod, cang, rho_tol, s_rho_q, rew_dis, res, max_r, pairwise, stats)
    resid = np.zeros(kn)
    F, JtJ, JtF, resid_new, mid = ev(X, resid)
    F0 = F
    u, v = 1e-3 * JtJ.max(), 2.0
    decisions = []
    for _ in range(iter_max):
        with np.errstate(all="ignore"):
            hh = kc.Cholesky6(JtJ + np.eye(6) * u).backsub(-JtF)
            Xn = X + hh
            Fn, JtJn, JtFn, resid_n, mid = ev(Xn, resid)
            gain = (F - Fn) / kc.dot(0.5 * hh, u * hh - JtF)
        decisions.append(bool(gain > 0))
        if gain > 0:
            F, X, JtJ, JtF = Fn, Xn, JtJn, JtFn
            g = 2 * gain - 1
            u *= max(0.33, 1 - g * g * g)
            v = 2.0
            resid, resid_new = resid_n, resid                   # std::swap(ResidualNew, Residual)
            stats["accepted"] += 1
        else:
            u *= v
            v *= 2
            stats["rejected"] += 1
    with np.errstate(all="ignore"):
        RRV = kc.Cholesky6(JtJ).inverse()
        r = F / F0
    return dict(X=X, RRV=RRV, r=r, F=F, F0=F0, m_id_f=mid, evals=iter_max + 1, accepted=sum(decisions), decisions=decisions)


def relocalize(q, kf, cam, a, pairwise=True, stats=None):
    """The whole rule for one pair (steps 1-6 of kfvo::OptimizePosGT) -> dict(X, RRV, r, mnum, m_id_f, Kp, K, Pose, Pos, evals, accepted)."""
    import keyframe_covis_port as cport
    _, ikl = cport.build_field(kf, int(cam["w"]), int(cam["h"]), int(a["field_radius"]), a["field_min_mod"])
    qp, kp = (q["Pose"], q["Pos"], q["K"]), (kf["Pose"], kf["Pos"], kf["K"])
    X0, Kr = request(*qp, *kp)
    m = minimizer_rv_kf(X0, q, kf, ikl, cam, Kr, a["rho_tol"], int(a["iter_max"]), a["rew_dis"], a["s_rho_q"], float(a["field_radius"]),
                        pairwise=pairwise, stats=stats)
    w = relocalize_around(q, qp, kf, kp, cam["zfm"], m["X"], m["m_id_f"])
    m.update(mnum=w["mnum"], Kp=w["Kp"], K=w["K"], Pose=w["Pose"], Pos=w["Pos"], used=w["used"])
    return m
