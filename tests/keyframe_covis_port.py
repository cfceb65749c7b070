"""Plain-numpy restatement of the three rules rebvo_amd/csrc/keyframe_covis.hip implements, with per-branch statistics:

  build_field   global_tracker::build_field(edges, radius, min_mod) (global_tracker.cpp:61-105, GetIndexRC image.h:121-126)
  count_pair    kfvo::countMatches (kfvo.cpp:18-55: reProjectTo keyframe.h:110-114, Calc_f_J_Complete<float> global_tracker.cpp:115-165)
                and kfvo::kls_on_fov (kfvo.cpp:688-712) for one ordered pair (to, from), plus the device's guard count

A key frame is a dict: p_m, c_p, u_m, m_m float32 [kn][2]; n_m float32 [kn]; rho, s_rho float64 [kn]; Pose [3][3], Pos [3], K (float64).
A camera is a dict: w, h, ppx, ppy (float32), zfm (float64).  Every operation is written in the width the reference's expression has;
numpy's float32 arrays do not contract, and the TooN products are dot products per row, result = 0 and += in index order.

tools/make_keyframe_covis_golden.py refuses to write a fixture unless this file equals the reference on every count and field cell.
"""
import collections
import ctypes
import ctypes.util

import numpy as np

FIELDS = ("p_m", "c_p", "u_m", "m_m", "n_m", "rho", "s_rho")
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cosf.restype = ctypes.c_float
_libm.cosf.argtypes = [ctypes.c_float]


def simil_cang(match_ang):
    """kfvo.cpp:45's cos(match_ang): the float overload (<math.h>'s C++ form puts std::cos(float) into the global namespace), the C
    library's cosf, not numpy's."""
    return np.float32(_libm.cosf(float(np.float32(match_ang))))


class Stats(collections.Counter):
    pass


def keyframe(kl, Pose, Pos, K):
    """From KeyLine records (any structured array with the fields) and a pose."""
    kf = {k: np.ascontiguousarray(kl[k]).astype(np.float64 if k in ("rho", "s_rho") else np.float32) for k in FIELDS}
    for k in ("p_m", "c_p", "u_m", "m_m"):
        kf[k] = kf[k].reshape(-1, 2)
    kf.update(Pose=np.asarray(Pose, np.float64).reshape(3, 3), Pos=np.asarray(Pos, np.float64).reshape(3), K=np.float64(K))
    return kf


def _round_half_away(x):
    """C's round() of a float, as a float64 array (exact: |x| + 0.5 of a float32 is representable in float64)."""
    x = x.astype(np.float64)
    return np.copysign(np.floor(np.abs(x) + 0.5), x)


def build_field(kf, w, h, radius, min_mod=0.0, stats=None):
    """-> (dist [h][w] int32, ikl [h][w] int32; ikl -1 and dist 0 where empty).  The serial rule overwrites a cell when |t| <= its dist,
    ikl ascending: the cell keeps the least |t| and, among those, the greatest ikl.  Restated as a minimum over (|t|, -ikl)."""
    kn = len(kf["n_m"])
    min_mod = np.float32(min_mod)
    big = np.int64(1) << 40
    key = np.full(h * w, big, np.int64)
    hits = np.zeros(h * w, np.int64)
    if kn and radius > 0:
        use = np.ones(kn, bool) if not min_mod > 0 else ~(kf["n_m"] < min_mod)
        if stats is not None:
            stats["field_min_mod_skipped"] += int((~use).sum())
        t = np.arange(-radius, radius, dtype=np.int64)
        tf = t.astype(np.float32)[None, :]
        x = _round_half_away(kf["u_m"][:, 0:1] * tf + kf["c_p"][:, 0:1])      # float32 product, float32 sum
        y = _round_half_away(kf["u_m"][:, 1:2] * tf + kf["c_p"][:, 1:2])
        with np.errstate(invalid="ignore"):
            inside = (x >= 0) & (x < w) & (y >= 0) & (y < h) & use[:, None]  # (int)round() of NaN / out of range is INT_MIN on x86-64: < 0
        if stats is not None:
            u = use[:, None]
            stats["field_off_left"] += int((u & (x < 0)).sum()); stats["field_off_right"] += int((u & (x >= w)).sum())
            stats["field_off_top"] += int((u & (y < 0)).sum()); stats["field_off_bottom"] += int((u & (y >= h)).sum())
        ii, tt = np.nonzero(inside)
        inx = (y[ii, tt] * w + x[ii, tt]).astype(np.int64)
        k = np.abs(t[tt]) * (np.int64(1) << 24) + (np.int64((1 << 24) - 1) - ii)
        np.minimum.at(key, inx, k)
        if stats is not None:
            # cells that samples of more than one KeyLine reach (overlapping segments), and cells whose least |t| more than one reaches
            pair = np.unique(np.stack([inx, ii]), axis=1)
            np.add.at(hits, pair[0], 1)
            stats["field_overlap_cells"] += int((hits > 1).sum())
            best = key[inx] >> 24
            tie = np.unique(np.stack([inx, ii])[:, np.abs(t[tt]) == best], axis=1)
            n_best = np.zeros(h * w, np.int64)
            np.add.at(n_best, tie[0], 1)
            stats["field_tie_cells"] += int((n_best > 1).sum())
    empty = key == big
    dist = np.where(empty, 0, key >> 24).astype(np.int32)
    ikl = np.where(empty, -1, ((1 << 24) - 1) - (key & ((1 << 24) - 1))).astype(np.int32)
    return dist.reshape(h, w), ikl.reshape(h, w)


def _mat_vec(Mx, v):
    """TooN Matrix * Vector per column of v [3][n]."""
    out = []
    for r in range(3):
        s = np.zeros_like(v[0])
        for k in range(3):
            s = s + Mx[r, k] * v[k]
        out.append(s)
    return out


def count_pair(to, frm, field, cam, match_mod, match_ang, rho_tol, max_r, stats=None):
    """-> (kl_on_fov, kl_match, kls_on_fov, guard) of the ordered pair; field = build_field(to, ...)."""
    st = stats if stats is not None else Stats()
    w, h = int(cam["w"]), int(cam["h"])
    ppx, ppy, zfm = np.float32(cam["ppx"]), np.float32(cam["ppy"]), np.float64(cam["zfm"])
    match_mod, rho_tol, max_r = np.float32(match_mod), np.float32(rho_tol), np.float32(max_r)
    cang_min = np.float64(simil_cang(match_ang))
    kn = len(frm["n_m"])
    if kn == 0:
        return 0, 0, 0, 0
    dist, ikl = field
    with np.errstate(all="ignore"):
        rho, s_rho = frm["rho"], frm["s_rho"]
        # unprojectHomCordVec, Local2WorldScaled
        u = [frm["p_m"][:, 0].astype(np.float64) / rho / zfm, frm["p_m"][:, 1].astype(np.float64) / rho / zfm, 1.0 / rho]
        wp = [s * frm["K"] + frm["Pos"][r] for r, s in enumerate(_mat_vec(frm["Pose"], u))]
        # World2LocalScaled, projectHomCordVec
        d = [wp[r] - to["Pos"][r] for r in range(3)]
        lc = [s / to["K"] for s in _mat_vec(to["Pose"].T, d)]
        px, py, pz = lc[0] / lc[2] * zfm, lc[1] / lc[2] * zfm, 1 / lc[2]
        ix, iy = px.astype(np.float32) + ppx, py.astype(np.float32) + ppy
        bad = ~(np.isfinite(ix) & np.isfinite(iy))
        c_l, c_t, c_r, c_b, c_z = ix < 1, iy < 1, ix >= np.float32(w - 1), iy >= np.float32(h - 1), pz <= 0
        outside = c_l | c_t | c_r | c_b | c_z | bad
        st["out_left"] += int((c_l & ~bad).sum()); st["out_top"] += int((c_t & ~bad).sum())
        st["out_right"] += int((c_r & ~bad).sum()); st["out_bottom"] += int((c_b & ~bad).sum())
        st["behind"] += int((c_z & ~bad).sum())
        on = ~outside
        x = np.where(on, ix.astype(np.float64) + 0.5, 0).astype(np.int64)     # round2int_positive: (int)(r + 0.5), the sum a double
        y = np.where(on, iy.astype(np.float64) + 0.5, 0).astype(np.int64)
        f = ikl[y, x]
        has = on & (f >= 0)
        st["empty_cell"] += int((on & (f < 0)).sum())
        q = np.where(has, f, 0)
        if len(to["n_m"]) == 0:      # (no field KeyLine to gather: every cell is empty)
            kl_match = 0
        else:
            fm, fn, f_rho, f_s_rho = to["m_m"][q], to["n_m"][q], to["rho"][q], to["s_rho"][q]
            cang = ((frm["m_m"][:, 0] * fm[:, 0] + frm["m_m"][:, 1] * fm[:, 1]) / frm["n_m"]).astype(np.float64)
            r_ang = cang < cang_min
            r_mod = np.abs(frm["n_m"] / fn - np.float32(1)) > match_mod
            frho = pz.astype(np.float32)
            r_rho = np.abs(frho.astype(np.float64) - f_rho) > np.float64(rho_tol) * (f_s_rho + s_rho * frho.astype(np.float64) / rho)
            rej = r_ang | r_mod | r_rho
            st["rej_angle"] += int((has & r_ang).sum())
            st["rej_mod"] += int((has & ~r_ang & r_mod).sum())
            st["rej_rho"] += int((has & ~r_ang & ~r_mod & r_rho).sum())
            dx, dy = ix - to["c_p"][q, 0], iy - to["c_p"][q, 1]
            fi = dx * to["u_m"][q, 0] + dy * to["u_m"][q, 1]
            ok = has & ~rej
            m = ok & (fi < max_r)
            st["matched_over_max_r"] += int((ok & ~(fi < max_r)).sum())
            st["match_negative_fi"] += int((m & (fi < 0)).sum())
            st["match_positive_fi"] += int((m & (fi > 0)).sum())
            kl_match = int(m.sum())
        # kls_on_fov
        R = np.zeros((3, 3))
        for i in range(3):
            for j in range(3):
                s = 0.0
                for k in range(3):
                    s = s + to["Pose"][k, i] * frm["Pose"][k, j]
                R[i, j] = s
        dP = frm["Pos"] - to["Pos"]
        T = np.zeros(3)
        for i in range(3):
            s = 0.0
            for k in range(3):
                s = s + to["Pose"][k, i] * dP[k]
            T[i] = s
        p0 = [c * frm["K"] for c in u]
        v = [s + T[r] for r, s in enumerate(_mat_vec(R, p0))]
        qx, qy, qz = v[0] / v[2] * zfm + np.float64(ppx), v[1] / v[2] * zfm + np.float64(ppy), 1 / v[2]

        def cvt(a):   # (int)double on x86-64: NaN and out-of-range give INT_MIN
            okr = (a > -2147483649.0) & (a < 2147483648.0)
            return np.where(okr, np.trunc(np.where(okr, a, 0)), -2147483648.0).astype(np.int64)
        kx, ky = cvt(qx + 0.5), cvt(qy + 0.5)
        on_kls = ~((kx < 0) | (ky < 0) | (kx >= w) | (ky >= h) | (qz <= 0))
        st["kls_x_0"] += int((on_kls & (kx == 0)).sum())
        st["kls_x_w_minus_1"] += int((on_kls & (kx == w - 1)).sum())
    return int(on.sum()), kl_match, int(on_kls.sum()), int(bad.sum())


def covisibility(kfs, cam, field_radius, match_mod, match_ang, rho_tol, max_r, field_min_mod=0.0, stats=None, fields_out=None):
    """Every ordered pair -> int32 [M][M][4] indexed [to][from] (kl_on_fov, kl_match, kls_on_fov, guard)."""
    M = len(kfs)
    out = np.zeros((M, M, 4), np.int32)
    for to in range(M):
        field = build_field(kfs[to], int(cam["w"]), int(cam["h"]), field_radius, field_min_mod, stats)
        if fields_out is not None:
            fields_out.append(field)
        for frm in range(M):
            out[to, frm] = count_pair(kfs[to], kfs[frm], field, cam, match_mod, match_ang, rho_tol, max_r, stats)
    return out


def load_fixture(path):
    """tests/golden/keyframe_covis/*.npz -> dict(kfs, cam, args, counts [M][M][3], field_dist, field_ikl [M][h][w], stats, z)."""
    z = np.load(path)
    M = int(z["n_kf"])
    kfs = [{k: z[f"kf{m}_{k}"] for k in FIELDS + ("Pose", "Pos", "K")} for m in range(M)]
    cam = {k: z[f"cam_{k}"][()] for k in ("w", "h", "ppx", "ppy", "zfx", "zfy", "zfm")}
    args = {k: z[f"arg_{k}"][()] for k in ("field_radius", "field_min_mod", "match_mod", "match_ang", "rho_tol", "max_r")}
    stats = dict(zip(z["stat_names"].tolist(), z["stat_values"].tolist()))
    return dict(kfs=kfs, cam=cam, args=args, counts=z["counts"], field_dist=z["field_dist"].astype(np.int32),
                field_ikl=z["field_ikl"].astype(np.int32), stats=stats, z=z)


def records(kf, dtype):
    """The key frame's KeyLines as 168-byte records (dtype = rebvo_amd.edgehip.KEYLINE_DTYPE): the eleven numbers, every id -1."""
    kl = np.zeros(len(kf["n_m"]), dtype)
    for k in FIELDS:
        kl[k] = kf[k]
    for k in ("m_id", "m_id_f", "m_id_kf", "p_id", "n_id", "net_id", "stereo_m_id"):
        kl[k] = -1
    return kl
