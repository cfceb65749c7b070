"""Plain-numpy restatement of the depth moves along the key-frame links: kfvo::mapKFUsingIDK / mapKLUsingIDK
(src/mtracklib/kfvo.cpp:1147-1184, 1276-1360, through rotateQs, include/mtracklib/kfvo.h:68-81), translateDepth_F2KF with
optimizeScaleBack (:653-686, 305-341), translateDepth_KF2F (:607-634) and translateDepth_New2Old (:637-650), with the device's own rule
where the reference has no defined result (the guard bits of include/edgehip.h).

Every per-KeyLine quantity is computed element-wise in fp64 in the reference's order of operations (numpy's element-wise operations
are the IEEE ones, with no contraction); the two sums of optimizeScaleBack are SERIAL in index order, as the reference's `+=` are.
Relative poses are TooN's products: row dot products from 0 in index order.

A list is a dict: p_m, u_m float32 (n, 2); rho, s_rho float64; m_num int32; and its links (a key frame's m_id_f, a frame's m_id_kf).
A pair is a dict: kf and fr (lists), the key frame's kf_Pose, kf_Pos, kf_K, the frame's Pose, Pos, K, and zfm.  A key-frame list is a
list of dicts: kl (a list whose m_id_f index the next entry's KeyLines), Pose, Pos, K."""
import hashlib

import numpy as np

from keyframe_constraint_port import matmul, matvec

RHO_MAX, RHO_MIN, RHO_INIT = 20.0, 1e-3, 1.0   # edge_finder.h:38-40
LIST_FIELDS = ("p_m", "u_m", "rho", "s_rho", "m_num")
BRANCHES = ("min", "max", "nonfinite", "negative", "none")


def relative(A, PA, B, PB):
    """A^T * B, A^T * (PB - PA)"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return matmul(A.T, B), matvec(A.T, np.asarray(PB, np.float64) - np.asarray(PA, np.float64))


def serial(x):
    x = np.asarray(x, np.float64)
    return np.float64(np.add.accumulate(x)[-1]) if len(x) else np.float64(0.0)


def linked(link, nb):
    """-> (indices of the walked rows whose link is used, their links, guard)"""
    link = np.asarray(link, np.int64)
    bad = link >= nb
    idx = np.nonzero((link >= 0) & ~bad)[0]
    return idx, link[idx], (4 if bad.any() else 0)


def rotate_qs(q, R, zf):
    """kfvo::rotateQs on columns q = [q0, q1, q2, q3]"""
    a = [q[0] / zf, q[1] / zf, np.ones_like(q[0])]
    qr = [((0.0 + R[r, 0] * a[0]) + R[r, 1] * a[1]) + R[r, 2] * a[2] for r in range(3)]
    ok = np.abs(qr[2]) > 0
    den = np.where(ok, qr[2], 1.0)
    return [np.where(ok, qr[0] / den * zf, 0.0), np.where(ok, qr[1] / den * zf, 0.0), np.where(ok, q[2] / den, 0.0), np.where(ok, q[3] / den, 0.0)], ok


def map_depth(pair, q_abs, q_rel, loc_unc, trace=None):
    """mapKFUsingIDK -> (rho, s_rho of the key frame (copies), count, guard).  trace: the clamp branch of every linked KeyLine and whether
    either rotateQs returned zeros."""
    kf, fr, zf = pair["kf"], pair["fr"], float(pair["zfm"])
    R, T = relative(pair["Pose"], pair["Pos"], pair["kf_Pose"], pair["kf_Pos"])
    idx, lk, guard = linked(kf["m_id_f"], len(fr["rho"]))
    rho_out, s_out = np.array(kf["rho"], np.float64), np.array(kf["s_rho"], np.float64)
    with np.errstate(all="ignore"):
        q0 = [kf["p_m"][idx, 0].astype(np.float64), kf["p_m"][idx, 1].astype(np.float64), rho_out[idx], s_out[idx]]
        q, ok0 = rotate_qs(q0, R, zf)
        q0x, q0y = fr["p_m"][lk, 0].astype(np.float64), fr["p_m"][lk, 1].astype(np.float64)
        u_x, u_y = fr["u_m"][lk, 0].astype(np.float64), fr["u_m"][lk, 1].astype(np.float64)
        v_rho = q[3] * q[3]
        rho_p = q[2]
        rq = q[2] * q_rel
        p_p = v_rho + rq * rq + q_abs * q_abs
        Y = u_x * (q0x - q[0]) + u_y * (q0y - q[1])
        H = u_x * (T[0] * zf - T[2] * q0x) + u_y * (T[1] * zf - T[2] * q0y)
        e = Y - H * rho_p
        S = H * p_p * H + loc_unc * loc_unc
        K = p_p * H * (1 / S)
        q[2] = rho_p + (K * e)
        v_rho = (1 - K * H) * p_p
        q[3] = np.sqrt(v_rho)
        up, ok1 = rotate_qs(q, R.T, zf)
        r, s = up[2], up[3]
        b_min = r < RHO_MIN
        b_max = ~b_min & (r > RHO_MAX)
        b_nf = ~b_min & ~b_max & (np.isnan(r) | np.isnan(s) | np.isinf(r) | np.isinf(s))
        b_neg = ~b_min & ~b_max & ~b_nf & (s < 0)
        reset = b_nf | b_neg
        s = np.where(b_min, s + (RHO_MIN - r), np.where(reset, RHO_MAX, s))
        r = np.where(b_min, RHO_MIN, np.where(b_max, RHO_MAX, np.where(reset, RHO_INIT, r)))
    rho_out[idx], s_out[idx] = r, s
    if trace is not None:
        trace["idx"] = idx
        trace["branch"] = np.where(b_min, 0, np.where(b_max, 1, np.where(b_nf, 2, np.where(b_neg, 3, 4))))
        trace["min_with_nan_s_rho"] = int((b_min & np.isnan(s)).sum())
        trace["rotate_zeros"] = int((~ok0).sum()) + int((~ok1).sum())
    return rho_out, s_out, len(idx), guard


def reproject_rho(R, T, K, zf, p_m, rho):
    """q1[2] of cam.projectHomCordVec(BRelRot * cam.unprojectHomCordVec(p_m.x, p_m.y, rho) * K + BRelPos)"""
    x = [p_m[:, 0].astype(np.float64) / rho / zf, p_m[:, 1].astype(np.float64) / rho / zf, 1.0 / rho]
    s = ((0.0 + R[2, 0] * x[0]) + R[2, 1] * x[1]) + R[2, 2] * x[2]
    return 1 / (s * K + T[2])


def scale_back(kf, fr, idx, lk, R, T, K, kf_K, zf, trace=None):
    """optimizeScaleBack's sums -> (Kr, rTr, rTr0)"""
    with np.errstate(all="ignore"):
        rho, s_rho = np.asarray(fr["rho"], np.float64)[lk], np.asarray(fr["s_rho"], np.float64)[lk]
        iz = 1 / rho
        x = [fr["p_m"][lk, 0].astype(np.float64) / zf * iz, fr["p_m"][lk, 1].astype(np.float64) / zf * iz, 1.0 * iz]
        s = ((0.0 + R[2, 0] * x[0]) + R[2, 1] * x[1]) + R[2, 2] * x[2]
        q2 = 1.0 * (1 / (s * K + T[2]))
        ok = q2 > 0
        w = s_rho * q2 / rho * kf_K
        s_b = np.asarray(kf["s_rho"], np.float64)[idx]
        v = w * w + s_b * s_b
        rTr0 = serial((q2 * q2 / v)[ok])
        rTr = serial((q2 * np.asarray(kf["rho"], np.float64)[idx] / v)[ok])
        Kr = (rTr / rTr0) if (rTr0 > 0 and rTr > 0) else np.float64(1.0)
    if trace is not None:
        trace["scale_behind"] = int((~ok).sum())
        trace["scale_links"] = len(idx)
    return np.float64(Kr), rTr, rTr0


def translate_f2kf(kf, fr, kf_Pose, kf_Pos, kf_K, Pose, Pos, K, zf, optim_scale=False, trace=None):
    """translateDepth_F2KF -> dict(rho, s_rho, m_num (copies of the key frame's), count, guard, K, rTr, rTr0)."""
    R, T = relative(kf_Pose, kf_Pos, Pose, Pos)
    idx, lk, guard = linked(kf["m_id_f"], len(fr["rho"]))
    kf_K, K = np.float64(kf_K), np.float64(K)
    rTr = rTr0 = np.float64(0.0)
    if optim_scale:
        Kn, rTr, rTr0 = scale_back(kf, fr, idx, lk, R, T, K, kf_K, zf, trace)
        if np.isfinite(Kn):
            kf_K = Kn
        else:
            guard |= 1
    rho_out, s_out, m_out = np.array(kf["rho"], np.float64), np.array(kf["s_rho"], np.float64), np.array(kf["m_num"], np.int32)
    with np.errstate(all="ignore"):
        rho_b, s_b = np.asarray(fr["rho"], np.float64)[lk], np.asarray(fr["s_rho"], np.float64)[lk]
        r = reproject_rho(R, T, K, zf, fr["p_m"][lk], rho_b) * kf_K
        rho_out[idx] = r
        s_out[idx] = r * (s_b / rho_b)
    m_out[idx] += 1
    return dict(rho=rho_out, s_rho=s_out, m_num=m_out, count=len(idx), guard=guard, K=kf_K, rTr=rTr, rTr0=rTr0)


def translate_kf2f(pair):
    """translateDepth_KF2F -> dict(rho, s_rho (copies of the frame's), count, guard, K)."""
    kf, fr, zf = pair["kf"], pair["fr"], float(pair["zfm"])
    R, T = relative(pair["Pose"], pair["Pos"], pair["kf_Pose"], pair["kf_Pos"])
    idx, lk, guard = linked(fr["m_id_kf"], len(kf["rho"]))
    rho_out, s_out = np.array(fr["rho"], np.float64), np.array(fr["s_rho"], np.float64)
    with np.errstate(all="ignore"):
        rho_b, s_b = np.asarray(kf["rho"], np.float64)[lk], np.asarray(kf["s_rho"], np.float64)[lk]
        r = reproject_rho(R, T, np.float64(pair["K"]), zf, kf["p_m"][lk], rho_b) * np.float64(pair["kf_K"])
        rho_out[idx] = r
        s_out[idx] = r / rho_b * s_b
    return dict(rho=rho_out, s_rho=s_out, m_num=np.array(fr["m_num"], np.int32), count=len(idx), guard=guard, K=np.float64(pair["kf_K"]),
                rTr=np.float64(0.0), rTr0=np.float64(0.0))


def translate(pair, direction, optim_scale=False, trace=None):
    if direction:
        assert not optim_scale
        return translate_kf2f(pair)
    return translate_f2kf(pair["kf"], pair["fr"], pair["kf_Pose"], pair["kf_Pos"], pair["kf_K"], pair["Pose"], pair["Pos"], pair["K"], float(pair["zfm"]),
                          optim_scale, trace)


def list_translate(kfs, iters, zf, successors_first=False):
    """translateDepth_New2Old -> (the list after `iters` iterations (copies), count of the last iteration, guard).  successors_first=True
    is NOT the reference's rule: it walks the positions downwards, so that each reads a successor this iteration has already rewritten
    (for the test that tells the two apart)."""
    kfs = [dict(k, kl={f: np.array(v) for f, v in k["kl"].items()}) for k in kfs]
    count = guard = 0
    for _ in range(iters):
        count = 0
        order = range(len(kfs) - 1)
        for i in (reversed(order) if successors_first else order):
            a, b = kfs[i], kfs[i + 1]
            got = translate_f2kf(a["kl"], b["kl"], a["Pose"], a["Pos"], a["K"], b["Pose"], b["Pos"], b["K"], zf)
            for f in ("rho", "s_rho", "m_num"):
                a["kl"][f] = got[f]
            count += got["count"]
            guard |= got["guard"]
    return kfs, count, guard


def digest(rho, s_rho, m_num):
    """A list's written fields as one hash: the doubles' bits with every NaN as one value, and the counts."""
    h = hashlib.sha256()
    for x in (rho, s_rho):
        x = np.array(x, np.float64)
        x[np.isnan(x)] = np.nan
        h.update(np.ascontiguousarray(x).tobytes())
    h.update(np.ascontiguousarray(np.asarray(m_num, np.int32)).tobytes())
    return h.hexdigest()


def same_bits(a, b):
    """fp64 arrays equal bit for bit, NaN as a class"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
class _Npz:
    """np.load's mapping, with the generator's aliases resolved (an array stored once under the first of its names)"""

    def __init__(self, path):
        self.z = np.load(path)
        self.files = [k[:-len("__alias")] if k.endswith("__alias") else k for k in self.z.files]

    def __getitem__(self, k):
        return self.z[k] if k in self.z.files else self.z[str(self.z[k + "__alias"])]


def load_fixture(path):
    z = _Npz(path)
    f = dict(z=z, cam={k[4:]: z[k] for k in z.files if k.startswith("cam_")}, pairs=[], cases=[], lists=[], list_cases=[])
    zfm = float(z["cam_zfm"])
    for j in range(int(z["n_pairs"])):
        pre = f"p{j}_"
        pair = dict(kf={k: z[pre + "kf_" + k] for k in LIST_FIELDS + ("m_id_f",)}, fr={k: z[pre + "fr_" + k] for k in LIST_FIELDS + ("m_id_kf",)},
                    zfm=zfm, kind=str(z[pre + "kind"]))
        for k in ("kf_Pose", "kf_Pos", "kf_K", "Pose", "Pos", "K"):
            pair[k] = z[pre + k]
        f["pairs"].append(pair)
    for c in range(int(z["n_cases"])):
        case = dict(pair=int(z["case_pair"][c]), call=str(z["case_call"][c]), direction=int(z["case_direction"][c]), optim=int(z["case_optim"][c]),
                    args=tuple(float(x) for x in z["case_args"][c]))
        ref = dict(count=int(z["ref_count"][c]), K=z["ref_K"][c], rTr=z["ref_rTr"][c], rTr0=z["ref_rTr0"][c], digest=str(z["ref_digest"][c]))
        for k in ("rho", "s_rho", "m_num"):
            if f"case{c}_{k}" in z.files:
                ref[k] = z[f"case{c}_{k}"]
        case["ref"] = ref
        f["cases"].append(case)
    for j in range(int(z["n_lists"])):
        n = int(z[f"l{j}_len"])
        f["lists"].append([dict(kl={k: z[f"l{j}_{i}_{k}"] for k in LIST_FIELDS + ("m_id_f",)}, Pose=z[f"l{j}_{i}_Pose"], Pos=z[f"l{j}_{i}_Pos"],
                                K=z[f"l{j}_{i}_K"]) for i in range(n)])
    for c in range(int(z["n_list_cases"])):
        j, iters = int(z["lcase_list"][c]), int(z["lcase_iters"][c])
        ref = dict(count=int(z["lref_count"][c]), digests=[str(d) for d in z[f"lcase{c}_digests"]])
        for i in range(len(f["lists"][j])):
            for k in ("rho", "s_rho", "m_num"):
                if f"lcase{c}_{i}_{k}" in z.files:
                    ref.setdefault(k, {})[i] = z[f"lcase{c}_{i}_{k}"]
        f["list_cases"].append(dict(list=j, iters=iters, ref=ref))
    return f


def records(lst, dtype, links):
    """168-byte KeyLine records of a fixture list: the fields the rules read or write and the given m_id_f / m_id_kf; every other id -1."""
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
