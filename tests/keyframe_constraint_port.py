"""Plain-numpy restatement of the key-frame relative-pose constraint: kfvo::OptimizeRelContraint (src/mtracklib/kfvo.cpp:527-604), its
evaluation OptimizeRelConstraint1Iter (:344-420), optimizeScaleF2KF (:263-302) and mutualExclusionSimple (:423-522), with the device's own
rule where the reference has no defined result (the guard bits of include/edgehip.h).

Every per-KeyLine quantity is computed element-wise in the reference's order of operations (numpy's element-wise fp64 operations are the
IEEE ones, with no contraction); every sum over KeyLines is SERIAL in index order (np.add.accumulate), as TooN's J.T()*J and the
reference's `E +=` are.  The 3x3 and 6x6 algebra is TooN's: products as row dot products from 0 in index order, Cholesky<6> as L D L^T.

A pair is a dict: kf and fr (each: p_m, u_m float32 (n, 2); rho, s_rho float64; the key frame's m_id_f / the frame's m_id_kf int32), the key
frame's kf_Pose, kf_Pos, kf_K, the frame's Pose, Pos, K, and zfm."""
import math

import numpy as np

F32 = np.float32


# ---- TooN pieces ------------------------------------------------------------------------------------------------------------------
def dot(a, b):
    s = 0.0
    for x, y in zip(a, b):
        s += float(x) * float(y)
    return s


def matmul(A, B):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return np.array([[dot(A[i, :], B[:, j]) for j in range(B.shape[1])] for i in range(A.shape[0])])


def matvec(A, x):
    return np.array([dot(A[i, :], x) for i in range(A.shape[0])])


def unit(v):
    return v * (1 / math.sqrt(dot(v, v)))


def so3_exp(w):
    """TooN::SO3<>::exp with rodrigues_so3_exp (so3.h:203-285)."""
    one_6th, one_20th = 1.0 / 6.0, 1.0 / 20.0
    theta_sq = dot(w, w)
    theta = math.sqrt(theta_sq)
    if theta_sq < 1e-8:
        A, B = 1.0 - one_6th * theta_sq, 0.5
    elif theta_sq < 1e-6:
        B = 0.5 - 0.25 * one_6th * theta_sq
        A = 1.0 - theta_sq * one_6th * (1.0 - one_20th * theta_sq)
    else:
        inv_theta = 1.0 / theta
        A = math.sin(theta) * inv_theta
        B = (1 - math.cos(theta)) * (inv_theta * inv_theta)
    w = [float(x) for x in w]
    R = np.zeros((3, 3))
    wx2, wy2, wz2 = w[0] * w[0], w[1] * w[1], w[2] * w[2]
    R[0, 0] = 1.0 - B * (wy2 + wz2)
    R[1, 1] = 1.0 - B * (wx2 + wz2)
    R[2, 2] = 1.0 - B * (wx2 + wy2)
    a, b = A * w[2], B * (w[0] * w[1])
    R[0, 1], R[1, 0] = b - a, b + a
    a, b = A * w[1], B * (w[0] * w[2])
    R[0, 2], R[2, 0] = b + a, b - a
    a, b = A * w[0], B * (w[1] * w[2])
    R[1, 2], R[2, 1] = b - a, b + a
    return R


def so3_coerce(M):
    """What SO3<>(Matrix) does (so3.h:110-118): Gram-Schmidt on the rows."""
    r0, r1, r2 = M[0].copy(), M[1].copy(), M[2].copy()
    r0 = unit(r0)
    r1 = r1 - r0 * dot(r0, r1)
    r1 = unit(r1)
    r2 = r2 - r0 * dot(r0, r2)
    r2 = r2 - r1 * dot(r1, r2)
    r2 = unit(r2)
    return np.stack([r0, r1, r2])


def so3_ln(Min):
    """SO3<>(M).ln() (so3.h:288-334)."""
    M = so3_coerce(np.asarray(Min, np.float64))
    cos_angle = (M[0, 0] + M[1, 1] + M[2, 2] - 1.0) * 0.5
    r = np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2])
    sin_angle_abs = math.sqrt(dot(r, r))
    if cos_angle > math.sqrt(0.5):
        if sin_angle_abs > 0:
            r = r * (math.asin(sin_angle_abs) / sin_angle_abs)
    elif cos_angle > -math.sqrt(0.5):
        r = r * (math.acos(cos_angle) / sin_angle_abs)
    else:
        angle = math.pi - math.asin(sin_angle_abs)
        d0, d1, d2 = M[0, 0] - cos_angle, M[1, 1] - cos_angle, M[2, 2] - cos_angle
        if d0 * d0 > d1 * d1 and d0 * d0 > d2 * d2:
            r2 = np.array([d0, (M[1, 0] + M[0, 1]) / 2, (M[0, 2] + M[2, 0]) / 2])
        elif d1 * d1 > d2 * d2:
            r2 = np.array([(M[1, 0] + M[0, 1]) / 2, d1, (M[2, 1] + M[1, 2]) / 2])
        else:
            r2 = np.array([(M[0, 2] + M[2, 0]) / 2, (M[2, 1] + M[1, 2]) / 2, d2])
        if dot(r2, r) < 0:
            r2 = r2 * -1.0
        r = unit(r2) * angle
    return r


class Cholesky6:
    """TooN::Cholesky<6> (Cholesky.h:88-200): L D L^T in place, backsub, get_inverse."""

    def __init__(self, A):
        L = np.array(A, np.float64)
        n = len(L)
        with np.errstate(all="ignore"):
            for col in range(n):
                inv_diag = 1.0
                stop = False
                for row in range(col, n):
                    val = L[row, col]
                    for col2 in range(col):
                        val -= L[col2, col] * L[row, col2]
                    if row == col:
                        L[row, col] = val
                        if val == 0:
                            stop = True
                            break
                        inv_diag = 1 / val
                    else:
                        L[col, row] = val
                        L[row, col] = val * inv_diag
                if stop:
                    break
        self.L = L

    def _solve(self, v, mul):
        L, n = self.L, len(self.L)
        y, r = np.zeros(n), np.zeros(n)
        with np.errstate(all="ignore"):
            for i in range(n):
                val = v[i]
                for j in range(i):
                    val -= L[i, j] * y[j]
                y[i] = val
            for i in range(n):
                y[i] = y[i] * (np.float64(1) / L[i, i]) if mul else y[i] / L[i, i]
            for i in range(n - 1, -1, -1):
                val = y[i]
                for j in range(i + 1, n):
                    val -= L[j, i] * r[j]
                r[i] = val
        return r

    def backsub(self, v):
        return self._solve(np.asarray(v, np.float64), False)

    def inverse(self):
        n = len(self.L)
        return np.stack([self._solve(np.eye(n)[c], True) for c in range(n)], 1)


def serial(a):
    """sum over axis 0, one term after the other from 0"""
    a = np.asarray(a, np.float64)
    if a.shape[0] == 0:
        return np.zeros(a.shape[1:])
    return np.add.accumulate(a, axis=0)[-1]


# ---- the rules --------------------------------------------------------------------------------------------------------------------
def start_pose(pair, direction):
    KP, KPos, KK = pair["kf_Pose"], pair["kf_Pos"], float(pair["kf_K"])
    Pose, Pos, K = pair["Pose"], pair["Pos"], float(pair["K"])
    if direction:   # kfvo.cpp:538-541
        return matmul(KP.T, Pose), matvec(KP.T, Pos - KPos) / K
    return matmul(Pose.T, KP), matvec(Pose.T, KPos - Pos) / KK


def gather(pair, direction):
    """The walked list's linked rows -> (dict of arrays over the rows, number of walked KeyLines, guard bit 2)."""
    own, oth = (pair["fr"], pair["kf"]) if direction else (pair["kf"], pair["fr"])
    link = np.asarray(own["m_id_kf"] if direction else own["m_id_f"], np.int64)
    nb = len(oth["rho"])
    bad = link >= nb
    idx = np.nonzero((link >= 0) & ~bad)[0]
    lk = link[idx]
    rows = dict(i=idx, px=own["p_m"][idx, 0].astype(np.float64), py=own["p_m"][idx, 1].astype(np.float64), rho=own["rho"][idx].astype(np.float64),
                s_rho=own["s_rho"][idx].astype(np.float64), pbx=oth["p_m"][lk, 0].astype(np.float64), pby=oth["p_m"][lk, 1].astype(np.float64),
                ubx=oth["u_m"][lk, 0].astype(np.float64), uby=oth["u_m"][lk, 1].astype(np.float64), rho_b=oth["rho"][lk].astype(np.float64),
                s_rho_b=oth["s_rho"][lk].astype(np.float64))
    return rows, len(link), (4 if bad.any() else 0)


def evaluate(rows, R, T, zfm, k_huber, residual, trace=None):
    """OptimizeRelConstraint1Iter -> (E, JtJ, JtF, (links, inliers)); `residual` is read for the weights and then overwritten."""
    with np.errstate(all="ignore"):
        x = [rows["px"] / rows["rho"] / zfm, rows["py"] / rows["rho"] / zfm, 1.0 / rows["rho"]]
        Rx = [(R[r, 0] * x[0] + R[r, 1] * x[1]) + R[r, 2] * x[2] for r in range(3)]
        p = [Rx[r] + T[r] for r in range(3)]
        q0, q1, q2 = p[0] / p[2] * zfm, p[1] / p[2] * zfm, 1 / p[2]
        ux, uy = rows["ubx"], rows["uby"]
        f = (q0 - rows["pbx"]) * ux + (q1 - rows["pby"]) * uy
        d = [q2 * zfm * ux, q2 * zfm * uy, -q2 * q0 * ux - q2 * q1 * uy]
        E = serial(f * f)
        dt = (d[0] * T[0] + d[1] * T[1]) + d[2] * T[2]
        sd = dt * rows["s_rho"] / q2
        stddev = np.sqrt(1.0 * 1.0 + sd * sd)
        res = residual[rows["i"]]
        rew = (np.abs(res) > k_huber) if k_huber > 0 else np.zeros(len(res), bool)
        weight = np.where(rew, k_huber / np.where(rew, np.abs(res), 1.0), 1.0)
        residual[rows["i"]] = f
        fw = f * (weight / stddev)
        wd = [weight * d[c] for c in range(3)]
        z = np.zeros_like(f)
        C = [[z, Rx[2], -Rx[1]], [-Rx[2], z, Rx[0]], [Rx[1], -Rx[0], z]]   # crossMatrix(Rx0).T()
        J = [wd[c] / stddev for c in range(3)] + [((wd[0] * C[0][c] + wd[1] * C[1][c]) + wd[2] * C[2][c]) / stddev for c in range(3)]
        JtJ = np.zeros((6, 6))
        for r in range(6):
            for c in range(r, 6):
                JtJ[r, c] = JtJ[c, r] = serial(J[r] * J[c])
        JtF = np.array([serial(J[r] * fw) for r in range(6)])
    if trace is not None:
        trace["reweighted"] = trace.get("reweighted", 0) + int(rew.sum())
        trace["unweighted"] = trace.get("unweighted", 0) + int((~rew).sum())
        trace.setdefault("weights", []).append(weight.copy())
    return float(E), JtJ, JtF, (len(f), int((~rew).sum()))


def scale_f2kf(rows, R, T, zfm, trace=None):
    """optimizeScaleF2KF with kfvo::unProject / kfvo::project (kfvo.h:42-48) -> (Kp, W_Kp)."""
    with np.errstate(all="ignore"):
        iz = 1 / rows["rho"]
        x = [rows["px"] / zfm * iz, rows["py"] / zfm * iz, 1.0 * iz]
        s = (R[2, 0] * x[0] + R[2, 1] * x[1]) + R[2, 2] * x[2]
        q = 1.0 * (1 / (s + T[2]))
        ok = q > 0
        v = rows["s_rho"] * rows["s_rho"] * (q / rows["rho"]) * (q / rows["rho"]) + rows["s_rho_b"] * rows["s_rho_b"]
        rTr0 = float(serial((q * q / v)[ok]))
        rTr = float(serial((rows["rho_b"] * rows["rho_b"] / v)[ok]))
    if trace is not None:
        trace["scale_behind"] = int((~ok).sum())
    return ((rTr / rTr0) if (rTr0 > 0 and rTr > 0) else 1.0), rTr0


def constraint(pair, direction, iter_max, k_huber, trace=None, shared_residual=True):
    """-> dict with the fields of edgehip_kf_constraint (X, W_X (6, 6), R_X (6, 6), ratio, E, E0, Kp, W_Kp, links, inliers, evals, accepted,
    guard).  trace (a dict) collects the branch populations and the weights of every evaluation.  shared_residual=False is NOT the
    reference's rule: it weights an evaluation by the residuals of the last ACCEPTED one, as Minimizer_RV_KF's swap does (for the test
    that tells the two rules apart)."""
    zfm = float(pair["zfm"])
    rows, n, guard = gather(pair, direction)
    R, T = start_pose(pair, direction)
    residual = np.zeros(n)
    evals = accepted = 0
    E, JtJ, JtF, mn = evaluate(rows, R, T, zfm, k_huber, residual, trace)
    E, JtJ, JtF, mn = evaluate(rows, R, T, zfm, k_huber, residual, trace)
    evals = 2
    E0 = E
    kept = residual.copy()
    u, v = 1e-3 * JtJ.max() if not np.isnan(JtJ).any() else 1e-3 * _max_first(JtJ), 2.0
    with np.errstate(all="ignore"):
        for _ in range(iter_max):
            if not np.isfinite(JtJ).all():
                guard |= 1
                break
            dX = Cholesky6(JtJ + np.eye(6) * u).backsub(-JtF)
            if not np.isfinite(dX).all():
                guard |= 1
                break
            Tn = T + dX[:3]
            Rn = so3_coerce(matmul(so3_exp(dX[3:]), R))
            if not shared_residual:
                residual[:] = kept
            En, Jn, Fn, mn = evaluate(rows, Rn, Tn, zfm, k_huber, residual, trace)
            evals += 1
            gain = np.float64(E - En) / np.float64(dot(0.5 * dX, u * dX - JtF))   # (IEEE division: x / 0 is inf or NaN, as in C)
            if gain > 0:
                E, T, R, JtJ, JtF = En, Tn, Rn, Jn, Fn
                g = 2 * gain - 1
                u *= max(0.33, 1 - (g * g * g))
                v = 2.0
                accepted += 1
                kept = residual.copy()
                if trace is not None:
                    trace["accepted"] = trace.get("accepted", 0) + 1
            else:
                u *= v
                v *= 2
                if trace is not None:
                    trace["rejected"] = trace.get("rejected", 0) + 1
        out = dict(X=np.concatenate([T, so3_ln(R)]), W_X=JtJ.copy(), R_X=Cholesky6(JtJ).inverse(), ratio=np.float64(E) / np.float64(E0), E=E, E0=E0,
                   Kp=0.0, W_Kp=0.0, links=mn[0], inliers=mn[1], evals=evals, accepted=accepted)
    if direction:
        out["Kp"], out["W_Kp"] = scale_f2kf(rows, R, T, zfm, trace)
    if mn[0] < 6:
        guard |= 2
    out["guard"] = guard
    if trace is not None:
        link = np.asarray((pair["fr"]["m_id_kf"] if direction else pair["kf"]["m_id_f"]), np.int64)
        lk = np.nonzero(link >= 0)[0]
        trace["unlinked_between"] = int((link[lk[0]:lk[-1]] < 0).sum()) if len(lk) else 0
    return out


def _max_first(A):
    """TooN::max_element: the running maximum under `>` from the first entry (a NaN never wins unless it is first)."""
    m = A.flat[0]
    for x in A.flat[1:]:
        if x > m:
            m = x
    return m


def mutual_exclusion(pair, dist_t, discard, kf_to_frame):
    """mutualExclusionSimple -> (the edited link column (a copy), (seen, kept)).  A link outside the list it indexes is left alone and not
    counted; a back link outside the walked list is counted as seen and left alone (the device's rule; the reference reads out of bounds)."""
    own, oth = (pair["kf"], pair["fr"]) if kf_to_frame else (pair["fr"], pair["kf"])
    mine = np.array(own["m_id_f"] if kf_to_frame else own["m_id_kf"], np.int32)
    other = np.asarray(oth["m_id_kf"] if kf_to_frame else oth["m_id_f"], np.int64)
    n, nb = len(mine), len(other)
    pm, um = own["p_m"].astype(F32), own["u_m"].astype(F32)
    seen = kept = 0
    out = mine.copy()
    for i in range(n):
        m_f = int(mine[i])
        if m_f < 0 or m_f >= nb:
            continue
        seen += 1
        m_b = int(other[m_f])
        if m_b < 0:
            if discard:
                out[i] = -1
            continue
        if m_b >= n:
            continue
        dx, dy = F32(pm[i, 0] - pm[m_b, 0]), F32(pm[i, 1] - pm[m_b, 1])
        if kf_to_frame:
            dist = float(np.sqrt(F32(F32(dx * dx) + F32(dy * dy))))        # util::norm<float>: sqrtf of the float sum
        else:
            dist = float(np.abs(F32(F32(dx * um[i, 0]) + F32(dy * um[i, 1]))))
        if dist > dist_t:
            out[i] = -1
        else:
            kept += 1
    return out, (seen, kept)


def pruned(pair, dist_t, discard, prune):
    """The pair after the pruning passes of `prune` (bit 0: key frame -> frame, then bit 1: frame -> key frame) -> (pair, counts[4])."""
    cnt = [0, 0, 0, 0]
    if prune & 1:
        col, c = mutual_exclusion(pair, dist_t, discard, True)
        pair = dict(pair, kf=dict(pair["kf"], m_id_f=col))
        cnt[0:2] = c
    if prune & 2:
        col, c = mutual_exclusion(pair, dist_t, discard, False)
        pair = dict(pair, fr=dict(pair["fr"], m_id_kf=col))
        cnt[2:4] = c
    return pair, cnt


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
LIST_FIELDS = ("p_m", "u_m", "rho", "s_rho")


def load_fixture(path):
    z = np.load(path)
    f = dict(z=z, cam={k[4:]: z[k] for k in z.files if k.startswith("cam_")}, pairs=[], cases=[])
    for j in range(int(z["n_pairs"])):
        pre = f"p{j}_"
        pair = dict(kf={k: z[pre + "kf_" + k] for k in LIST_FIELDS + ("m_id_f",)}, fr={k: z[pre + "fr_" + k] for k in LIST_FIELDS + ("m_id_kf",)},
                    zfm=float(z["cam_zfm"]), kind=str(z[pre + "kind"]))
        for k in ("kf_Pose", "kf_Pos", "kf_K", "Pose", "Pos", "K"):
            pair[k] = z[pre + k]
        f["pairs"].append(pair)
    for c in range(int(z["n_cases"])):
        case = {k: z["case_" + k][c] for k in ("pair", "direction", "iter_max", "k_huber", "prune", "discard", "dist_t")}
        case = {k: (float(v) if k in ("k_huber", "dist_t") else int(v)) for k, v in case.items()}
        case["ref"] = {k: z["ref_" + k][c] for k in ("X", "W_X", "R_X", "ratio", "E", "E0", "Kp", "W_Kp", "links", "inliers", "prune_counts")}
        case["m_id_f"] = z[f"case{c}_m_id_f"]
        case["m_id_kf"] = z[f"case{c}_m_id_kf"]
        f["cases"].append(case)
    return f


def records(lst, dtype, links):
    """168-byte KeyLine records of a fixture list: the four fields the rules read and the given m_id_f / m_id_kf; every other id -1."""
    kl = np.zeros(len(lst["rho"]), dtype)
    for k in LIST_FIELDS:
        kl[k] = lst[k]
    kl["c_p"] = lst["p_m"]
    kl["m_m"] = lst["u_m"]
    kl["n_m"] = 1
    for k in ("m_id", "m_id_f", "m_id_kf", "p_id", "n_id", "net_id", "stereo_m_id"):
        kl[k] = -1
    for k, v in links.items():
        kl[k] = v
    return kl
