"""CPU restatement in numpy of the receiving side of the reference's compressed edge map, edgemap_com_decoder
(src/CommLib/edgemap_com.cpp): getPair's cursor walk and Decode (:46-86, :431-440), UpdatePos (:142-160), TransformPos (:106-127),
HideVisible (:443-473) and fillDepthMap (:475-528), in the reference's own order and number types: np.float32 scalars where the reference
computes in float, Python floats (double) where it computes in double.  The chain behind the fill (InitCoarseFine, Integrate) is
tests/depth_fill_port.py's.

Written from the reference's text independently of rebvo_amd/csrc/edgemap_seg.h: decode() is the serial cursor walk, not the local rule
the device runs, and fill_depth_map() updates cell after cell in the reference's nested loops."""
import math

import numpy as np

from tests import depth_fill_port as dfp

F = np.float32
RHO_SCALING = F(32767.0 / 20)     # COMPRESSED_RHO_SCALING
SRHO_SCALING = F(255.0 / 20)      # COMPRESSED_SRHO_SCALING
CRHO_MIN = F(1e-3)
GATE_NAMES = ("folded", "sigma", "sum", "rel", "angle", "degenerate")


def _conv(rec, rho, rho_scale, xs, ys):
    r = F(rho)
    r = F(r / F(RHO_SCALING / F(rho_scale)))
    x = F(int(rec["x"]) / xs)
    y = F(int(rec["y"]) / ys)
    s = F(F(int(rec["s_rho"])) / SRHO_SCALING) if int(rec["s_rho"]) > 0 else CRHO_MIN
    return [x, y, r, s]


def decode(records, rho_scale, seg_max=1 << 30, x_scaling=0.5, y_scaling=1.0):
    """Decode: getPair from the first record on -> (segments (n, 8) float32, flags (n,) uint8 all 1)."""
    n = len(records)
    rho = [int(v) for v in records["rho"]]
    segs = []
    i = 0
    while len(segs) < seg_max:
        while i < n - 1 and rho[i] == 0:
            i += 1
        if i >= n - 1:
            break
        k0 = _conv(records[i], abs(rho[i]), rho_scale, x_scaling, y_scaling)
        i += 1
        if rho[i] == 0 or rho[i - 1] < 0:
            k1 = list(k0)
        else:
            k1 = _conv(records[i], rho[i], rho_scale, x_scaling, y_scaling)
            if k1[2] < 0:
                k1[2] = F(-k1[2])
                i += 1
        segs.append(k0 + k1)
    segs = np.array(segs, np.float32).reshape(-1, 8)
    return segs, np.ones(len(segs), np.uint8)


def _so3_exp_f(w):
    """TooN::SO3<>::exp on a Vector<3, float>: theta_sq and the mixed products in float, the rest in double."""
    w = [F(v) for v in w]
    d = F(0)
    for v in w:
        d = F(d + F(v * v))
    theta_sq = float(d)
    theta = math.sqrt(theta_sq)
    if theta_sq < 1e-8:
        A = 1.0 - (1.0 / 6.0) * theta_sq
        B = 0.5
    elif theta_sq < 1e-6:
        B = 0.5 - 0.25 * (1.0 / 6.0) * theta_sq
        A = 1.0 - theta_sq * (1.0 / 6.0) * (1.0 - (1.0 / 20.0) * theta_sq)
    else:
        inv = 1.0 / theta
        A = math.sin(theta) * inv
        B = (1 - math.cos(theta)) * (inv * inv)
    wd = [float(v) for v in w]
    wx2, wy2, wz2 = wd[0] * wd[0], wd[1] * wd[1], wd[2] * wd[2]
    R = np.zeros((3, 3))
    R[0, 0] = 1.0 - B * (wy2 + wz2)
    R[1, 1] = 1.0 - B * (wx2 + wz2)
    R[2, 2] = 1.0 - B * (wx2 + wy2)
    a, b = A * wd[2], B * float(F(w[0] * w[1]))
    R[0, 1], R[1, 0] = b - a, b + a
    a, b = A * wd[1], B * float(F(w[0] * w[2]))
    R[0, 2], R[2, 0] = b + a, b - a
    a, b = A * wd[0], B * float(F(w[1] * w[2]))
    R[1, 2], R[2, 1] = b - a, b + a
    return R


def _dot3(a, b):
    s = 0.0
    for i in range(3):
        s += float(a[i]) * float(b[i])
    return s


def update_pos(em_nav, new_nav):
    """UpdatePos -> (DPose (3, 3), DPos (3,), DK).  A nav package is 17 floats: p[3], w[3], g[3], ps[3], K, ref_err[4]."""
    em_nav, new_nav = np.asarray(em_nav, np.float32), np.asarray(new_nav, np.float32)
    Rn, Ro = _so3_exp_f(new_nav[3:6]), _so3_exp_f(em_nav[3:6])
    RnT = Rn.T
    DPose = np.array([[_dot3(RnT[r], Ro[:, c]) for c in range(3)] for r in range(3)])
    dv = [float(em_nav[k]) - float(new_nav[k]) for k in range(3)]
    DPos = np.array([_dot3(RnT[r], dv) for r in range(3)])
    return DPose, DPos, float(em_nav[12])


def transform_pos(p, DPose, DPos, k_em, k_new, cam):
    """TransformPos of (x, y, rho, s_rho) float32 -> the same.  cam: (ppx, ppy, zfm, w, h)."""
    ppx, ppy, zfm = F(cam[0]), F(cam[1]), float(cam[2])
    x, y = F(F(p[0]) - ppx), F(F(p[1]) - ppy)
    rho = float(F(p[2]))
    with np.errstate(all="ignore"):
        P0 = [np.float64(float(x) / zfm) / rho, np.float64(float(y) / zfm) / rho, np.float64(1.0) / rho]
        P1 = [np.float64(_dot3(DPose[r], P0)) * float(F(k_em)) + float(DPos[r]) for r in range(3)]
        r1 = F(np.float64(1.0) / np.float64(P1[2]))
        ox = F(np.float64(P1[0]) * float(r1) * zfm)
        oy = F(np.float64(P1[1]) * float(r1) * zfm)
        r1 = F(r1 * F(k_new))
        return F(ox + ppx), F(oy + ppy), r1, F(F(p[3]) * F(k_new))


def hide_visible(segs, flags, DPose, DPos, k_em, k_new, cam):
    """HideVisible with UpdatePos already applied: clears flags in place -> s_num."""
    w, h = F(cam[3]), F(cam[4])

    def seen(t):
        return bool(t[0] >= 0 and t[1] >= 0 and t[0] < w and t[1] < h and t[2] > 0)

    s_num = 0
    for i in range(len(segs)):
        if not flags[i]:
            continue
        if seen(transform_pos(segs[i, 0:4], DPose, DPos, k_em, k_new, cam)) or seen(transform_pos(segs[i, 4:8], DPose, DPos, k_em, k_new, cam)):
            flags[i] = 0
        else:
            s_num += 1
    return s_num


def _unproject(x, y, rho, cam):
    """cam_model::unprojectImgCordVec on a Vector<3, float>: float storage."""
    ppx, ppy, zfm = F(cam[0]), F(cam[1]), float(cam[2])
    with np.errstate(all="ignore"):
        return [float(F(float(F(F(x - ppx) / rho)) / zfm)), float(F(float(F(F(y - ppy) / rho)) / zfm)), float(F(np.float64(1.0) / float(rho)))]


def cangle(seg, cam):
    k0x, k0y, k0r, _, k1x, k1y, _, _ = (F(v) for v in seg)
    p0, p1 = _unproject(k0x, k0y, k0r, cam), _unproject(k1x, k1y, k0r, cam)
    d = [p0[i] - p1[i] for i in range(3)]
    with np.errstate(all="ignore"):
        return float(np.float64(abs(_dot3(d, p0))) / np.float64(math.sqrt(_dot3(p0, p0))) / np.float64(math.sqrt(_dot3(d, d))))


def _d2i(q):
    return int(q) if -2147483649.0 < q < 2147483648.0 else -(1 << 31)


def _axis(x, bl, g):
    hh = (x & 0xFFFFFFFF) // bl
    if hh >= 1 << 31:
        hh -= 1 << 32
    return min(max(hh, 0), g - 1)


def fill_depth_map(segs, flags, w, h, bw, bh, cam, v_thresh, a_thresh_deg, use_visibility=False):
    """ResetData + fillDepthMap -> rho, s_rho, fixed (flat), gates (per segment: index into GATE_NAMES, -1 skipped as hidden)."""
    gw, gh = w // bw, h // bh
    G = gw * gh
    rho, s_rho, I = np.ones(G), np.full(G, dfp.S_RHO0), np.full(G, dfp.I_RHO0)
    fixed = np.zeros(G, bool)
    cos_a = math.cos(a_thresh_deg * math.pi / 180.0)
    gates = np.full(len(segs), -1, np.int32)
    for j in range(len(segs)):
        if use_visibility and not flags[j]:
            continue
        k0x, k0y, k0r, k0s, k1x, k1y, k1r, k1s = (F(v) for v in segs[j])
        if float(F(k0s * SRHO_SCALING)) > 254.0 or float(F(k1s * SRHO_SCALING)) > 254.0:
            gates[j] = 1
            continue
        if F(k0s + k1s) > F(k0r + k1r):
            gates[j] = 2
            continue
        if float(F(k0r / k0s)) < v_thresh or float(F(k1r / k1s)) < v_thresh:
            gates[j] = 3
            continue
        if cangle(segs[j], cam) > cos_a:
            gates[j] = 4
            continue
        tx, ty = float(F(k1x - k0x)), float(F(k1y - k0y))
        nt = math.sqrt(tx * tx + ty * ty)
        if not nt > 0:
            gates[j] = 5
            continue
        gates[j] = 0
        tx, ty = tx / nt, ty / nt
        r1 = float(F(k1r - k0r)) / nt
        sr = float(F(F(k0s + k1s) / F(2)))
        kl_I = 1 / (sr * sr)
        i = 0
        while i < nt:
            qx, qy = float(k0x) + tx * i, float(k0y) + ty * i
            r = r1 * i + float(k0r)
            c = _axis(_d2i(qy), bh, gh) * gw + _axis(_d2i(qx), bw, gw)
            i_rho = I[c] * rho[c]
            i_rho += r * kl_I
            I[c] += kl_I
            v = 1.0 / I[c] if I[c] > 0 else 1e20
            rho[c] = i_rho * v
            s_rho[c] = math.sqrt(v)
            fixed[c] = True
            i += 1
    return rho, s_rho, fixed, gates


def chain(rho, s_rho, fixed, w, h, bw, bh, iter_num, bound_mode):
    """InitCoarseFine + Integrate(iter_num) behind a fill -> (gh, gw) arrays (copies)."""
    gw, gh = w // bw, h // bh
    rho, s_rho, fixed = rho.copy().reshape(gh, gw), s_rho.copy().reshape(gh, gw), fixed.copy().reshape(gh, gw)
    dfp.init_coarse_fine(rho, s_rho, fixed, gw, gh, bound_mode)
    dfp.sweeps(rho, s_rho, fixed, gw, gh, bound_mode, iter_num)
    return rho, s_rho, fixed
