"""Crafted KeyLine lists for forward and directed matching — edge_tracker::FordwardMatch (edge_tracker.cpp:380-436), search_match and
directed_matching (:158-374) — shared by tests/test_matching_crafted_cpu.py (the reference against the restatement below, class
populations, the iteration cap) and tests/test_matching_crafted_gpu.py (k_fwd_key / k_fwd_win / k_fwd_apply / k_rotate / k_directed and the
one-pass form k_rotate<OUT, WIN> + k_directed_fused against the reference).  This module imports no GPU code.

Geometry.  160 x 120, max_points = 2048, principal point (80, 60), zf = 128 (zfm = 128: all exact in float).  Two contexts: "near" with
search_range = 40 (the shipped value) and "far" with search_range = 255, the largest the library accepts (dq_max = 257: walks of up to
259 steps from a positive start, both runs of the segment code); match_thresh_module = 1, match_thresh_angle = 45 and
loc_unc_match = 2 as shipped.  Under the pose "x" (BackRot = I, V = (-2^-7, 0, 0), RVel = diag(2^-15, 2^-15, 0)) everything is an exact
binary number: p_m stays as it is, k_rho = rho, t = (1, -0), norm_t = 1, sigma2_t = 1, so dq_rho = rho IS the start of the walk in
pixels, the probe at counter t is pixel (X0 + t, row) for a new KeyLine at pixel (X0, row), dq_min = max(0, rho - s_rho) - 2 and
dq_max = min(search_range, rho + s_rho) + 2.  Every class (SUBS) has a row of its own in the old mask of its context, so walks of
different classes along x share no old KeyLine.  Row 0 and column 0 of the old mask are full of old KeyLines that pass every gate
("traps", s_rho = 1e3): a probe whose coordinate is NaN is out of the image in the reference (round() of a NaN converts to INT_MIN on
x86-64, Image::GetIndexRC image.h:121-126), while a conversion that turned a NaN into 0 would land on them.

A class is built for one pose (its first) and asserted there; under every other pose its lists still run, and the comparison with the
reference is on every KeyLine.  Classes whose walks would cost the reference millions of empty iterations under another pose (negative
rho under a diverged velocity) are left out of the lists of that pose (subs_of); under a diverged velocity norm_t (rho - s_rho) ~ 1e6 is dq_min and the reference walks
half of it per KeyLine, so the lists of those poses carry s_rho >= |rho| (POSES[...]['wide']).  The reference executes every step of a walk, so the
far classes are chosen by their cost: test_matching_crafted_cpu.py counts the iterations of everything it runs (cap 2e8).  A walk whose
round2int_positive argument is just below 2^31 - 0.5 would cost 2^31 iterations per KeyLine: only the two values on the overflowing side
(the argument exactly 2^31 - 0.5, where argument + 0.5 = 2^31 converts to INT_MIN, and one above) are built.

Found while building this (asserted in the CPU test):
  * the kernel's two step-index runs never exist apart.  With a = dq_rho and T = Tmax: a > T + 3 leaves no tp run (p1 < 0), a < -T - 3
    no tn run, and in between p0 = 0 and n0 = 0 whenever both exist — they always overlap from step 0 and are merged; the
    branch that orders two separate runs is never taken.  Nor is a tn run ever entered beyond step 0: that needs dq_rho > Tmax + 2 >= 286,
    while dq_rho <= dq_max <= SearchRange + loc_unc <= 257 with the largest SearchRange the library accepts.  The classes are therefore:
    tp run alone (entered at p0 > 0: a negative k_rho) and both runs merged from step 0;
  * a run that does not start at step 0 starts Tmax away from the image, so a candidate "within the first two steps of a run" exists only
    for runs that start at step 0; the last two steps of a run (bounded by dq_min, dq_max or t_steps) are in the image;
  * cang is a float divided by the product of two floats: the three operand sets that give exactly cos(45 deg) and the doubles either
    side of it (CANG) come from a search, and the module asserts them;
  * FordwardMatch's rule `target.m_id >= 0 && target.rho > k.rho -> skip` lets a NaN rho through in both positions (every comparison
    with a NaN is false), and +0.0 > -0.0 is false: see forward_match(rule="device") for what the two atomicMax passes do instead.

Out of domain: the reference's outcome depends on the target's earlier m_id only through :407; with m_id = -1 on entry (as the detector
leaves it, with m_num = 0) the first writer always writes.  A new list that arrives with m_id >= 0 is out of the domain and not built.
"""
import math

import numpy as np

from oracle.oracle import KEYLINE_DTYPE

F32, F64 = np.float32, np.float64
INT_MIN = -2 ** 31
W, H, CAP = 160, 120, 2048
ZF = 128.0
PP = (80.0, 60.0)
SEARCH_RANGE = {"near": 40, "far": 255}     # 255: the largest SearchRange edgehip_create accepts
ARGS = dict(min_thr_mod=1.0, min_thr_ang=45.0, loc_unc=2.0)
RHO_INIT, RHO_MAX = 1.0, 20.0
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025)
FULL = 1025
MIN_POP = 8
NAN, INF = float("nan"), float("inf")
TEN = ("rho", "s_rho", "rho_nr", "s_rho_nr", "m_num", "m_id", "p_m_0", "m_m0", "n_m0", "m_id_kf")
COS45 = math.cos(45.0 * math.pi / 180.0)          # the expression of edge_tracker.cpp:170 and of directed_enqueue: one libm, one value
# operands with (double)num / ((double)n_old * (double)n_new) == cos(45 deg) exactly / the double above / the double below
CANG = {"on": dict(n_new=1.9099726676940918, n_old=1.3982274532318115, num=1.8883825540542603),
        "below": dict(n_new=1.9485554695129395, n_old=1.787575602531433, num=2.4629874229431152),
        "above": dict(n_new=1.6820471286773682, n_old=1.795395016670227, num=2.1354193687438965)}
for _k, _want in (("on", COS45), ("above", float(np.nextafter(COS45, 1.0))), ("below", float(np.nextafter(COS45, 0.0)))):
    _c = CANG[_k]
    assert all(float(F32(v)) == v for v in _c.values()) and _c["num"] / (_c["n_old"] * _c["n_new"]) == _want
    assert abs(_c["n_old"] / _c["n_new"] - 1) < 1.0
C_1EM6 = 1e-6
assert math.sqrt(C_1EM6 * C_1EM6) == C_1EM6
_C_UP, _C_DN = float(np.nextafter(C_1EM6, 1.0)), float(np.nextafter(C_1EM6, 0.0))
assert math.sqrt(_C_UP * _C_UP) == _C_UP and math.sqrt(_C_DN * _C_DN) == _C_DN


def so3_exp(w):
    """exp of a rotation vector (Rodrigues): helpers.so3_exp."""
    w = np.asarray(w, F64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-9:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


_DIAG = np.diag([2.0 ** -15, 2.0 ** -15, 0.0])
_FULL = np.array([[3e-5, 1e-5, -2e-6], [1e-5, 4e-5, 5e-6], [-2e-6, 5e-6, 2e-5]])
# W: rotate_keylines turns the old list by R0 = exp(W) and directed_matching gets BackRot = R0^T.  BR: a back-rotation given as it is
# (the launch chain only; the one-pass form always forms it from W): the exact quarter turn about y, for p3[2] = 0.  exp(W) on the
# device has a cosine of ~6e-17 there, not 0, so the class "p3[2] = 0 with V[2] = 0" reaches k_directed and not k_directed_fused.
POSES = {
    "x": dict(W=(0, 0, 0), V=(-2.0 ** -7, 0, 0), RVel=_DIAG),
    "zero": dict(W=(0, 0, 0), V=(0, 0, 0), RVel=_FULL),
    "nt_on": dict(W=(0, 0, 0), V=(-C_1EM6 / 128, 0, 0), RVel=_DIAG),
    "nt_below": dict(W=(0, 0, 0), V=(-_C_DN / 128, 0, 0), RVel=_DIAG),
    "nt_above": dict(W=(0, 0, 0), V=(-_C_UP / 128, 0, 0), RVel=_DIAG),
    "rot_a": dict(W=(0.01, -0.02, 0.015), V=(3e-3, -2e-3, 5e-3), RVel=_FULL),
    "rot_b": dict(W=(-0.2, 0.1, 0.3), V=(1e3, -5e2, 2e2), RVel=_DIAG, wide=True),
    "xdiv": dict(W=(0, 0, 0), V=(-1000.0, 0, 0), RVel=_DIAG, wide=True),
    "flip": dict(W=(math.pi, 0, 0), V=(-2.0 ** -7, 0, 0), RVel=_DIAG),
    "quarter": dict(W=(0, -math.pi / 2, 0), V=(0, 2.0 ** -7, 3e-3), RVel=_FULL, BR=np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])),
}
COMBOS = [("near", p) for p in POSES] + [("far", p) for p in ("x", "rot_a", "zero")]


def pose_matrices(pose):
    """-> (R0 for rotate_keylines, BackRot for directed_matching, V, RVel) of the launch chain."""
    p = POSES[pose]
    if "BR" in p:
        return p["BR"].T.copy(), p["BR"].copy(), np.array(p["V"], F64), p["RVel"].copy()
    R0 = so3_exp(p["W"])
    return R0, R0.T.copy(), np.array(p["V"], F64), p["RVel"].copy()


# ---------------------------------------------------------------------------------------------------------------------------------
# The restatement: numpy scalars and arrays in the reference's operand order (x86-64 SSE2, no contraction)
# ---------------------------------------------------------------------------------------------------------------------------------
def std_max(a, b):
    return b if a < b else a


def std_min(a, b):
    return b if b < a else a


def cvttsd2si(x):
    """(int)x for a double on x86-64: NaN and values outside int give INT_MIN."""
    x = float(x)
    if x != x or x >= 2147483648.0 or x <= -2147483649.0:
        return INT_MIN
    return int(x)


def _matvec(R, v):
    out = []
    for c in range(3):                              # TooN: result = 0; result += m[c][j] * v[j]
        d = F64(0.0)
        for j in range(3):
            d = d + F64(R[c][j]) * v[j]
        out.append(d)
    return out


def _matmat(A, B):
    out = [[F64(0.0)] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            d = F64(0.0)
            for k in range(3):
                d = d + F64(A[i][k]) * F64(B[k][j])
            out[i][j] = d
    return out


def _round_to_int(f):
    """const int xi = round(x) for an array of floats -> (integer value as double, convertible): half away from zero; NaN and values
    outside int convert to INT_MIN, which is out of every image."""
    x = f.astype(F64)
    ok = np.abs(x) < 2147483648.0
    r = np.copysign(np.floor(np.abs(x) + 0.5), x)
    return r, ok


_CHUNK = 1 << 16


def search_match(k, old, mask, V, RVel, BR, max_radius, a=ARGS, nan_to_zero=False):
    """edge_tracker::search_match (:158-295) for the new KeyLine record k; V and RVel are already back-rotated (directed_matching does
    that).  -> (index of the match or -1, info): info has the branch ("epipolar" / "midpoint" / "across"), the argument of
    round2int_positive (t_arg), t_steps, k_rho, dq_rho / dq_min / dq_max, whether the bounds were clamped, the number of iterations of
    the outer loop the reference executes, and the step and direction of the match."""
    h, w = mask.shape
    zf = F64(ZF)
    loc, thr = F64(a["loc_unc"]), F64(a["min_thr_mod"])
    cmin = F64(math.cos(a["min_thr_ang"] * math.pi / 180.0))
    max_radius = F64(max_radius)
    p3 = _matvec(BR, [F64(k["p_m"][0]), F64(k["p_m"][1]), zf])
    pmx, pmy = F32(p3[0] * zf / p3[2]), F32(p3[1] * zf / p3[2])              # Point2DF p_m
    k_rho = F64(k["rho"]) * zf / p3[2]
    pi0x, pi0y = F32(pmx + F32(PP[0])), F32(pmy + F32(PP[1]))                # Hom2Img on floats
    t_x = -(V[0] * zf - V[2] * F64(pmx))
    t_y = -(V[1] * zf - V[2] * F64(pmy))
    norm_t = np.sqrt(t_x * t_x + t_y * t_y)
    drdv = [zf, zf, F64(F32(-pmx) - pmy)]                                    # -p_m.x - p_m.y in float
    row = []
    for j in range(3):
        d = F64(0.0)
        for i in range(3):
            d = d + drdv[i] * RVel[i][j]
        row.append(d)
    sigma2_t = F64(0.0)
    for j in range(3):
        sigma2_t = sigma2_t + row[j] * drdv[j]
    s_rho_k = F64(k["s_rho"])
    info = dict(clamp_min=False, clamp_max=False)
    if norm_t > 1e-6:
        t_x, t_y = t_x / norm_t, t_y / norm_t
        dq_rho = norm_t * k_rho
        lo, hi = norm_t * (k_rho - s_rho_k), norm_t * (k_rho + s_rho_k)
        dq_min = std_max(F64(0.0), lo) - loc
        dq_max = std_min(max_radius, hi) + loc
        info["clamp_min"], info["clamp_max"] = not (F64(0.0) < lo), not (hi < max_radius)
        if dq_rho > dq_max:
            dq_rho = (dq_max + dq_min) / 2
            t_arg, branch = dq_rho, "midpoint"
        else:
            t_arg, branch = std_max(dq_max - dq_rho, dq_rho - dq_min), "epipolar"
        t_steps = cvttsd2si(t_arg + 0.5)
    else:
        t_x, t_y, norm_t = F64(k["m_m"][0]), F64(k["m_m"][1]), F64(k["n_m"])
        t_x, t_y = t_x / norm_t, t_y / norm_t
        norm_t = F64(1.0)
        dq_min, dq_max, dq_rho = -max_radius - loc, max_radius + loc, F64(0.0)
        t_arg, branch = dq_max, "across"
        t_steps = cvttsd2si(dq_max)
    norm_m = F64(k["n_m"])
    kmx, kmy = F32(k["m_m"][0]), F32(k["m_m"][1])
    info.update(branch=branch, t_arg=float(t_arg), t_steps=t_steps, k_rho=float(k_rho), dq_rho=float(dq_rho), dq_min=float(dq_min),
                dq_max=float(dq_max), pi0=(float(pi0x), float(pi0y)), norm_t=float(norm_t), step=-1, dir=-1, iters=max(t_steps, 0), probes=0)
    tn, tp = dq_rho, dq_rho + 1
    i0 = 0
    while i0 < t_steps:
        n = min(_CHUNK, t_steps - i0)
        ones = np.ones(n + 1)
        ones[0] = tn
        tns = np.subtract.accumulate(ones)            # tn, tn - 1, (tn - 1) - 1, ...: the reference's counter, step by step
        ones[0] = tp
        tps = np.add.accumulate(ones)
        events = []
        for d, ts in ((0, tns[:n]), (1, tps[:n])):
            go = ~(ts > dq_max) if d else ~(ts < dq_min)
            fx, fy = (t_x * ts + F64(pi0x)).astype(F32), (t_y * ts + F64(pi0y)).astype(F32)     # GetIndexRC(float, float)
            (xr, xok), (yr, yok) = _round_to_int(fx), _round_to_int(fy)
            if nan_to_zero:
                xr, yr = np.where(np.isnan(fx), 0.0, xr), np.where(np.isnan(fy), 0.0, yr)
                xok, yok = xok | np.isnan(fx), yok | np.isnan(fy)
            inside = go & xok & yok & (xr < w) & (yr < h) & (xr >= 0) & (yr >= 0)
            st = np.nonzero(inside)[0]
            info["probes"] += len(st)
            if len(st):
                j = mask[yr[st].astype(np.int64), xr[st].astype(np.int64)]
                for s_, j_ in zip(st[j >= 0], j[j >= 0]):
                    events.append((int(s_), d, int(j_), ts[s_]))
        for s_, d, j, t in sorted(events, key=lambda e: (e[0], e[1])):
            norm_m0 = F64(old["n_m"][j])
            num = F32(F32(old["m_m"][j, 0]) * kmx) + F32(F32(old["m_m"][j, 1]) * kmy)
            cang = F64(num) / (norm_m0 * norm_m)
            if cang < cmin or abs(norm_m0 / norm_m - 1) > thr:
                continue
            s_rho, rho = F64(old["s_rho"][j]), F64(old["rho"][j])
            v_rho_dr = loc * loc + s_rho * s_rho * norm_t * norm_t + sigma2_t * rho * rho
            dd = t - norm_t * rho
            if dd * dd > v_rho_dr:
                continue
            info.update(step=i0 + s_, dir=d, iters=i0 + s_ + 1)
            return j, info
        tn, tp = tns[n], tps[n]
        i0 += n
    return -1, info


def directed_matching(new, old, mask, pose_or_mats, ctx, stereo_mode=False, nan_to_zero=False, only=None):
    """edge_tracker::directed_matching (:302-374) -> (new list after it, nmatch, kf_matchs, per-KeyLine info).  `old` is the TURNED old
    list (rotate_keylines has run).  pose_or_mats: a pose name or (V, RVel, BackRot)."""
    if isinstance(pose_or_mats, str):
        _, BR, V, RVel = pose_matrices(pose_or_mats)
    else:
        V, RVel, BR = pose_or_mats
    out = new.copy()
    infos = [None] * len(new)
    nmatch = kf = 0
    with np.errstate(all="ignore"):
        Vb = _matvec(BR, [F64(v) for v in V])                                # Vel = BackRot * Vel
        RVb = _matmat(_matmat(BR, RVel), np.asarray(BR).T)                   # RVel = BackRot * RVel * BackRot.T()
        for i in (range(len(new)) if only is None else only):
            j, infos[i] = search_match(new[i], old, mask, Vb, RVb, BR, SEARCH_RANGE[ctx], nan_to_zero=nan_to_zero)
            if j < 0:
                continue
            if stereo_mode:
                out["rho"][i], out["s_rho"][i] = old["rho0"][j], old["s_rho0"][j]
            else:
                for f in ("rho", "s_rho", "rho_nr", "s_rho_nr"):
                    out[f][i] = old[f][j]
            out["m_id"][i] = j
            out["m_num"][i] = old["m_num"][j] + 1
            out["p_m_0"][i], out["m_m0"][i], out["n_m0"][i] = old["p_m"][j], old["m_m"][j], old["n_m"][j]
            out["m_id_kf"][i] = old["m_id_kf"][j]
            kf += int(old["m_id_kf"][j] >= 0)
            nmatch += 1
    return out, nmatch, kf, infos


def ord_bits(v):
    b = int(np.array([v], F64).view(np.uint64)[0])
    return (~b & 0xFFFFFFFFFFFFFFFF) if b >> 63 else (b | 0x8000000000000000)


def forward_match(old, new, rule="reference"):
    """edge_tracker::FordwardMatch (:380-436), old list -> new list.  -> (new list after it, the reference's return value).
    rule = "device": what k_fwd_key / k_fwd_win (and k_rotate<OUT, WIN>) state instead of :407 — among the old KeyLines that point at one
    new KeyLine the largest ord_bits(rho) wins, the largest index among equals.  ord_bits orders doubles by their bits: -NaN < -inf <
    ... < -0.0 < +0.0 < ... < +inf < +NaN.  Equal to the sequential rule wherever `>` on doubles and that order agree: no NaN, and
    no +0.0 against -0.0."""
    out = new.copy()
    n = 0

    def write(i, f):
        for fld in ("rho", "s_rho", "rho_nr", "s_rho_nr"):
            out[fld][f] = old[fld][i]
        out["m_num"][f] = old["m_num"][i] + 1
        out["m_id"][f] = i
        out["p_m_0"][f], out["m_m0"][f], out["n_m0"][f], out["m_id_kf"][f] = old["p_m"][i], old["m_m"][i], old["n_m"][i], old["m_id_kf"][i]

    if rule == "device":
        best = {}
        for i in range(len(old)):
            f = int(old["m_id_f"][i])
            if f < 0 or f >= len(new):
                continue
            key = (ord_bits(old["rho"][i]), i)
            if f not in best or key > best[f]:
                best[f] = key
        for f, (_, i) in best.items():
            write(i, f)
        return out, len(best)
    for i in range(len(old)):
        f = int(old["m_id_f"][i])
        if f < 0 or f >= len(new):
            continue
        if out["m_id"][f] >= 0 and out["rho"][f] > old["rho"][i]:
            continue
        write(i, f)
        n += 1
    return out, n


def segment_runs(info, ctx):
    """The kernel's two step-index runs (stage_c.hip directed_body, t_steps > 256) from a walk's bounds -> None for a walk that is not
    long, else dict(hn, hp, n0, n1, p0, p1).  Used to name the long-walk classes and to assert that two runs never exist apart."""
    ts = info["t_steps"]
    a = info["dq_rho"]
    T = float(W + H) + abs(info["pi0"][0]) + abs(info["pi0"][1]) + 4.0
    if not (ts > 256 and abs(a) < 1e15 and T < 1e15):
        return None
    n0, n1 = max(0.0, math.floor(a - T) - 2.0), min(float(ts), math.ceil(min(a + T, a - info["dq_min"])) + 2.0)
    p0, p1 = max(0.0, math.floor(-T - a - 1.0) - 2.0), min(float(ts), math.ceil(min(T - a - 1.0, info["dq_max"] - a - 1.0)) + 2.0)
    return dict(hn=n1 > n0, hp=p1 > p0, n0=n0, n1=n1, p0=p0, p1=p1)


# ---------------------------------------------------------------------------------------------------------------------------------
# The classes
# ---------------------------------------------------------------------------------------------------------------------------------
_UP = lambda v: float(np.nextafter(v, INF))
_DN = lambda v: float(np.nextafter(v, -INF))
NEG_D = (300.0, 1000.0, 301.0, 30000.0, 999.0, 1.0e6, 300.5, 5000.0, 1.0e5, 1.0e7, 2000.0, 400.0)     # one 1e7 in twelve members


def _subs():
    """dict(name, cls, ctx ("near" / "far" / "*"), poses (the first is the one it is built for; "*" = every pose), new fields (X0 = its
    pixel column; a callable value gets the member's occurrence number), olds (dt = offset from X0 along the row, or px / py), expect
    (index into olds, "trap", None = no match, "any" = whatever the reference says), pred(info) the branch it must reach)."""
    subs = []

    def sub(name, cls, ctx="*", poses=("x", "*"), olds=(), expect="any", pred=None, blind_trap=False, **new):
        m = dict(X0=60.0, rho=10.0, s_rho=4.0, m_m=(1.0, 0.0), n_m=1.0)
        m.update(new)
        subs.append(dict(name=name, cls=cls, ctx=ctx, poses=tuple(poses), new=m, olds=[dict(o) for o in olds], expect=expect, pred=pred, blind_trap=blind_trap))

    epi = lambda i: i["branch"] == "epipolar"
    mid = lambda i: i["branch"] == "midpoint"
    ONLY_X = ("x",)
    sub("plain", "start", olds=[dict(dt=8)], expect=0, pred=lambda i: epi(i) and i["t_steps"] == 6 and (i["step"], i["dir"]) == (2, 0))
    # ---- start of the walk (pose x: dq_rho = rho) ----
    sub("start_on_max", "start", "near", olds=[dict(dt=42)], expect=0, rho=42.0, pred=lambda i: epi(i) and i["dq_rho"] == i["dq_max"] == 42.0)
    sub("start_above_max", "start", "near", olds=[dict(dt=39)], expect=0, rho=_UP(42.0), pred=lambda i: mid(i) and i["t_steps"] == 39)
    sub("start_on_max_far", "start", "far", olds=[dict(px=5, rho=105.0)], expect=0, X0=-100.0, rho=257.0, s_rho=200.0,
        pred=lambda i: epi(i) and i["dq_rho"] == i["dq_max"] == 257.0 and i["step"] == 152)
    sub("start_above_max_far", "start", "far", olds=[dict(px=40, rho=140.0)], expect=0, X0=-100.0, rho=_UP(257.0), s_rho=200.0,
        pred=lambda i: mid(i) and i["t_steps"] == 156)
    sub("min_clamped", "start", olds=[dict(dt=-2)], expect=0, rho=3.0, s_rho=10.0, pred=lambda i: i["clamp_min"] and i["dq_min"] == -2.0 and i["dir"] == 0)
    sub("min_not_clamped", "start", olds=[dict(dt=5), dict(dt=4)], expect=0, pred=lambda i: not i["clamp_min"] and i["dq_min"] == 4.0)
    sub("max_clamped", "start", "near", olds=[dict(dt=42)], expect=0, rho=30.0, s_rho=30.0, pred=lambda i: i["clamp_max"] and i["dq_max"] == 42.0)
    sub("max_not_clamped", "start", olds=[dict(dt=16), dict(dt=17)], expect=0, pred=lambda i: not i["clamp_max"] and i["dq_max"] == 16.0)
    e40 = 2.0 ** -40
    sub("half_on", "start", olds=[dict(dt=4)], expect=0, s_rho=4.5, pred=lambda i: i["t_arg"] == 6.5 and i["t_steps"] == 7)
    sub("half_below", "start", olds=[dict(dt=4)], expect=None, s_rho=4.5 - e40, pred=lambda i: 6.4 < i["t_arg"] < 6.5 and i["t_steps"] == 6)
    sub("half_above", "start", olds=[dict(dt=4)], expect=0, s_rho=4.5 + e40, pred=lambda i: 6.5 < i["t_arg"] < 6.6 and i["t_steps"] == 7)
    sub("steps_0", "start", olds=[dict(dt=10)], expect=None, s_rho=-2.0, pred=lambda i: i["t_steps"] == 0)
    sub("steps_1", "start", olds=[dict(dt=10), dict(dt=11), dict(dt=9)], expect=0, s_rho=-1.25, pred=lambda i: i["t_steps"] == 1)
    for n_ in (255, 256, 257):                       # rho = 256, s_rho = n - 2: dq_min = 256 - n, t_steps = n; the match sits at the last step
        sub(f"steps_{n_}", "start", "far", ONLY_X + ("rot_a", "zero"), olds=[dict(dt=256 - (n_ - 1)), dict(dt=256 - n_)], expect=0, X0=10.0, rho=256.0, s_rho=n_ - 2.0,
            pred=lambda i, n_=n_: i["t_steps"] == n_ and (i["step"], i["dir"]) == (n_ - 1, 0))
    # ---- order of probes ----
    sub("order_tn_tp", "order", olds=[dict(dt=14), dict(dt=7)], expect=1, pred=lambda i: (i["step"], i["dir"]) == (3, 0))
    sub("order_tp_tn_even", "order", olds=[dict(dt=7), dict(dt=13)], expect=1, rho=10.0, s_rho=4.0, pred=lambda i: (i["step"], i["dir"]) == (2, 1))
    sub("order_tp_tn_odd", "order", olds=[dict(dt=8), dict(dt=12)], expect=1, pred=lambda i: (i["step"], i["dir"]) == (1, 1))
    sub("order_last_step", "order", olds=[dict(dt=5)], expect=0, pred=lambda i: i["step"] == i["t_steps"] - 1 == 5)
    sub("order_step_t_steps", "order", olds=[dict(dt=4)], expect=None, pred=lambda i: i["t_steps"] == 6 and i["dq_min"] == 4.0)
    # tn walks on below dq_min (skipped: the KeyLine at t = -3 is never probed) while tp still climbs to dq_max at the last step
    sub("order_skipped_min", "order", olds=[dict(dt=-3), dict(dt=15)], expect=1, rho=3.0, s_rho=10.0,
        pred=lambda i: i["dq_min"] == -2.0 and (i["step"], i["dir"]) == (11, 1) and i["t_steps"] == 12)
    # tp walks on above dq_max (skipped: t = 43) while tn still comes down to dq_min + 1 at the last step
    sub("order_skipped_max", "order", "near", olds=[dict(dt=43), dict(dt=27)], expect=1, rho=38.0, s_rho=10.0,
        pred=lambda i: i["dq_max"] == 42.0 and (i["step"], i["dir"]) == (11, 0) and i["t_steps"] == 12)
    # ---- long walks ----
    big = lambda D: 2.0 * D + 100.0
    neg = lambda o: -NEG_D[o % len(NEG_D)]
    sneg = lambda o: big(NEG_D[o % len(NEG_D)])
    long_p = lambda i: i["t_steps"] > 256 and i["k_rho"] < 0
    sub("long_neg_last", "long", "near", ONLY_X, blind_trap=True, olds=[dict(dt=42)], expect=0, rho=neg, s_rho=sneg,
        pred=lambda i: long_p(i) and i["step"] >= i["t_steps"] - 2 and i["dir"] == 1)
    sub("long_neg_first_in_image", "long", "near", ONLY_X, olds=[dict(dt=-59), dict(dt=0)], expect="any", rho=neg, s_rho=sneg, X0=60.0,
        pred=lambda i: long_p(i) and i["dir"] == 1)
    sub("long_neg_none", "long", "near", ONLY_X, blind_trap=True, olds=[], expect=None, rho=neg, s_rho=sneg, pred=lambda i: long_p(i) and i["iters"] == i["t_steps"])
    sub("long_neg_rho_big_step", "long", "near", ONLY_X, blind_trap=True, olds=[dict(dt=41)], expect=0, rho=-1.0e5, s_rho=INF, pred=long_p)
    sub("long_flip", "long", "near", ("flip",), olds=[dict(px=30, rho=1.0, s_rho=1e3)], expect="any",
        rho=lambda o: (300.0, 1000.0, 20000.0, 350.0)[o % 4], s_rho=lambda o: 2 * (300.0, 1000.0, 20000.0, 350.0)[o % 4] + 50, pred=long_p)
    sub("long_xdiv", "long", "near", ("xdiv",), olds=[dict(dt=30, rho=30 / 128000.0)], expect="any",
        rho=lambda o: -(300.0, 1000.0, 50000.0, 400.0)[o % 4] / 128000.0, s_rho=1.0e3, pred=lambda i: long_p(i) and i["dir"] == 1)
    sub("long_pos_both_last", "long", "far", ONLY_X + ("rot_a",), olds=[dict(dt=-1)], expect=0, X0=5.0, rho=255.0, s_rho=300.0,
        pred=lambda i: i["t_steps"] == 257 and (i["step"], i["dir"]) == (256, 0))
    sub("long_pos_both_first", "long", "far", ONLY_X + ("rot_a",), olds=[dict(dt=256), dict(dt=255)], expect=0, X0=-150.0, rho=256.0, s_rho=300.0,
        pred=lambda i: i["t_steps"] == 258 and i["step"] == 0)
    sub("long_pos_both_second", "long", "far", ONLY_X + ("rot_a",), olds=[dict(dt=256, rho=255.5)], expect=0, X0=-150.0, rho=256.5, s_rho=300.0,
        pred=lambda i: i["t_steps"] == 259 and (i["step"], i["dir"]) == (1, 0))     # 105.5 rounds to pixel 106
    sub("far_on", "long", "near", ONLY_X, olds=[dict(dt=10)], expect=None, rho=-(2.0 ** 31 - 42.5), s_rho=2.0 ** 33,
        pred=lambda i: i["t_arg"] == 2.0 ** 31 - 0.5 and i["t_steps"] == INT_MIN)
    sub("far_above", "long", "near", ONLY_X, olds=[dict(dt=10)], expect=None, rho=-(2.0 ** 31 - 42.0), s_rho=2.0 ** 33,
        pred=lambda i: i["t_arg"] == 2.0 ** 31 and i["t_steps"] == INT_MIN)
    sub("rho_huge", "long", olds=[dict(dt=20)], expect="any", rho=1e300, s_rho=1e300, pred=mid)
    # ---- image border (pose x along the row; pose zero along m_m) ----
    sub("left_in", "border", olds=[], expect="trap", X0=2.0, rho=3.0, s_rho=10.0, pred=lambda i: (i["step"], i["dir"]) == (5, 0))
    sub("left_half", "border", olds=[], expect=None, X0=1.5, rho=3.0, s_rho=10.0, pred=epi)          # -0.5 rounds to -1: pixel 0 is skipped
    sub("right_in", "border", olds=[dict(px=159, rho=9.0)], expect=0, X0=150.0, rho=3.0, s_rho=10.0, pred=epi)
    sub("right_half", "border", olds=[dict(px=159, rho=8.0)], expect=0, X0=150.5, rho=3.0, s_rho=10.0, pred=lambda i: (i["step"], i["dir"]) == (4, 1))   # 158.5 -> 159; 159.5 -> 160 is out
    up = dict(rho=3.0, s_rho=1.0, m_m=(0.0, 1.0))
    for nm, y0, expect in (("top_in", 3.0, "trap"), ("top_half", 3.5, None), ("bottom_in", 116.0, 0), ("bottom_half", 115.5, 0)):
        sub(nm, "border", poses=("zero", "*"), olds=[dict(px="col", py=119, rho=3.0, s_rho=1.0, m_m=(0.0, 1.0))] if expect == 0 else [],
            expect=expect, X0="col", Y0=y0, pred=lambda i: i["branch"] == "across", **up)
    # ---- gates ----
    for nm, exp in (("on", 0), ("above", 0), ("below", None)):
        c = CANG[nm]
        sub("cang_" + nm, "gate", olds=[dict(dt=8, m_m=(c["num"], 0.0), n_m=c["n_old"])], expect=exp, n_m=c["n_new"], pred=epi)
    sub("mod_on", "gate", olds=[dict(dt=8, n_m=2.0, m_m=(2.0, 0.0))], expect=0, pred=epi)
    sub("mod_above", "gate", olds=[dict(dt=8, n_m=float(np.nextafter(F32(2), F32(3))), m_m=(2.0, 0.0))], expect=None, pred=epi)
    sub("mod_below", "gate", olds=[dict(dt=8, n_m=float(np.nextafter(F32(2), F32(0))), m_m=(2.0, 0.0))], expect=0, pred=epi)
    # (t - norm_t rho)^2 against loc^2 + s_rho^2 + sigma2_t rho^2 with t = 5, rho = 2, s_rho = 1, sigma2_t = 1: 9 against 9
    sub("model_on", "gate", olds=[dict(dt=5, rho=2.0, s_rho=1.0)], expect=0, rho=5.0, pred=lambda i: i["step"] == 0)
    # (the doubles next to 2 round back into the equality: 5 - (2 - 2^-52) = 3 and 5 + (2 - 2^-52)^2 = 9 after rounding)
    sub("model_above", "gate", olds=[dict(dt=5, rho=2.0 - e40, s_rho=1.0)], expect=None, rho=5.0, pred=epi)
    sub("model_below", "gate", olds=[dict(dt=5, rho=2.0 + e40, s_rho=1.0)], expect=0, rho=5.0, pred=epi)
    sub("norm_m0_zero", "gate", olds=[dict(dt=8, n_m=0.0)], expect=0, pred=epi)                      # cang = +inf, |0 / 1 - 1| = 1 is not > 1
    sub("norm_m0_zero_m_m_zero", "gate", olds=[dict(dt=8, n_m=0.0, m_m=(0.0, 0.0))], expect=0, pred=epi)   # cang = NaN: not < cos
    sub("norm_m_zero", "gate", olds=[dict(dt=8)], expect=None, n_m=0.0, pred=epi)                    # 1 / 0 - 1 = inf
    # ---- non-finite inputs: none may match a trap ----
    for nm, rho, s in (("rho_nan", NAN, 4.0), ("rho_inf", INF, 4.0), ("rho_ninf", -INF, 4.0), ("rho_ninf_s_inf", -INF, INF)):
        sub("nf_" + nm, "nonfinite", olds=[dict(dt=8)], expect=None, rho=rho, s_rho=s, pred=lambda i: i["t_steps"] == INT_MIN)
    sub("nf_rho_s_rho_inf", "nonfinite", "near", olds=[dict(dt=8)], expect=0, rho=INF, s_rho=INF, pred=lambda i: mid(i) and i["t_steps"] == 20)
    sub("nf_s_rho_nan", "nonfinite", "near", olds=[dict(dt=12)], expect=0, s_rho=NAN, pred=lambda i: i["dq_min"] == -2.0 and i["t_steps"] == 32)
    sub("nf_s_rho_inf", "nonfinite", "near", olds=[dict(dt=12)], expect=0, s_rho=INF, pred=lambda i: i["clamp_min"] and i["clamp_max"])
    sub("nf_s_rho_ninf", "nonfinite", olds=[dict(dt=12)], expect=None, s_rho=-INF, pred=lambda i: i["t_steps"] == INT_MIN)
    sub("nf_pm_x_nan", "nonfinite", olds=[dict(dt=8)], expect=None, pm=(NAN, None), pred=lambda i: i["branch"] == "across" and i["probes"] == 0)
    sub("nf_pm_y_nan", "nonfinite", olds=[dict(dt=8)], expect=None, pm=(None, NAN), pred=lambda i: i["branch"] == "across" and i["probes"] == 0)
    sub("nf_p3z_zero", "nonfinite", poses=("quarter", "*"), olds=[], expect=None, pm=(0.0, None), pred=lambda i: i["branch"] == "across" and i["probes"] == 0)
    sub("nf_across_n_m_zero", "nonfinite", poses=("zero", "*"), olds=[dict(dt=8)], expect=None, n_m=0.0, pred=lambda i: i["branch"] == "across" and i["probes"] == 0)
    sub("nf_across_m_m_nan", "nonfinite", poses=("zero", "*"), olds=[dict(dt=8)], expect=None, m_m=(NAN, 1.0), pred=lambda i: i["branch"] == "across" and i["probes"] == 0)
    sub("nf_across_m_m_y_nan", "nonfinite", poses=("zero", "*"), olds=[dict(dt=8)], expect=None, m_m=(1.0, NAN), pred=lambda i: i["branch"] == "across" and i["probes"] == 0)
    sub("nf_cand_rho_nan", "nonfinite", olds=[dict(dt=8, rho=NAN)], expect=0, pred=epi)              # NaN > v_rho_dr is false: it matches
    sub("nf_cand_s_rho_nan", "nonfinite", olds=[dict(dt=8, s_rho=NAN)], expect=0, pred=epi)
    sub("nf_cand_far_s_rho_inf", "nonfinite", olds=[dict(dt=8, rho=1e6, s_rho=INF)], expect=0, pred=epi)
    return subs


SUBS = _subs()
assert len({s["name"] for s in SUBS}) == len(SUBS)
CLASSES = ("start", "order", "long", "border", "gate", "nonfinite")
PLAIN = 0


def subs_of(ctx, pose):
    """The classes a list of this context and pose is dealt from (the others fall back to the plain class)."""
    return [si for si, s in enumerate(SUBS) if s["ctx"] in ("*", ctx) and (pose in s["poses"] or "*" in s["poses"])]


def home(s, ctx, pose):
    return s["ctx"] in ("*", ctx) and s["poses"][0] == pose


_ROW0 = 16


def old_list(ctx):
    """The old list of a context and its mask: the candidates of every class of the context (class k in row 16 + k; classes along y in a
    column of their own from 150 up), the traps of row 0 and column 0, and N_FWD old KeyLines that are on no pixel and carry the forward
    matches.  Every old KeyLine has values of its own in every field that is cloned.  -> (list, mask, first candidate per class name,
    index of the first trap, index of the first forward KeyLine, row and column per class)."""
    recs, mask, first, place = [], np.full((H, W), -1, np.int32), {}, {}
    row, col = _ROW0, 150
    for s in SUBS:
        if s["ctx"] not in ("*", ctx):
            continue
        m = s["new"]
        x0 = m["X0"]
        if x0 == "col":
            place[s["name"]] = (m["Y0"], float(col))
            col += 1
        else:
            place[s["name"]] = (float(row), x0)
            row += 1
        assert row <= H and col <= W - 1
        first[s["name"]] = len(recs)
        y_, x_ = place[s["name"]]
        for o in s["olds"]:
            q = dict(m_m=(1.0, 0.0), n_m=1.0, s_rho=1.0)
            q.update(o)
            px = int(x_ if q.get("px") == "col" else q["px"] if "px" in q else x_ + q["dt"])
            py = int(q.get("py", y_))
            q.setdefault("rho", float(q.get("dt", 0.0)))
            assert 0 < px < W and 0 < py < H and mask[py, px] == -1, (s["name"], px, py)
            q["px"], q["py"] = px, py
            mask[py, px] = len(recs)
            recs.append(q)
    trap0 = len(recs)
    for x in range(W):
        mask[0, x] = len(recs)
        recs.append(dict(px=x, py=0, m_m=(0.0, 1.0) if x >= 150 else (1.0, 0.0), n_m=1.0, rho=3.0, s_rho=1e3))
    blind = {int(place[s["name"]][0]) for s in SUBS if s["blind_trap"] and s["name"] in place}
    for y in range(1, H):                             # (a tp run that comes in from the left meets column 0 first: the classes that look at
        mask[y, 0] = len(recs)                        # the end of such a run have a trap in their row that fails the angle gate)
        recs.append(dict(px=0, py=y, m_m=(-1.0, 0.0) if y in blind else (1.0, 0.0), n_m=1.0, rho=3.0, s_rho=1e3))
    fwd0 = len(recs)
    for _ in range(N_FWD):
        recs.append(dict(px=None, py=None, m_m=(1.0, 0.0), n_m=1.0, rho=1.0, s_rho=1.0))
    kl = np.zeros(len(recs), KEYLINE_DTYPE)
    j = np.arange(len(recs))
    for i, q in enumerate(recs):
        if q["px"] is None:
            kl["p_inx"][i], kl["c_p"][i], kl["p_m"][i] = 5 * W + 5 + i % 100, (5.0 + i % 100, 5.0), (5.0 + i % 100 - PP[0], 5.0 - PP[1])
        else:
            kl["p_inx"][i], kl["c_p"][i], kl["p_m"][i] = q["py"] * W + q["px"], (q["px"], q["py"]), (q["px"] - PP[0], q["py"] - PP[1])
        kl["m_m"][i], kl["n_m"][i], kl["rho"][i], kl["s_rho"][i] = q["m_m"], q["n_m"], q["rho"], q["s_rho"]
    kl["u_m"] = kl["m_m"]
    kl["p_m_0"] = kl["p_m"] + F32(0.25)
    kl["rho_nr"], kl["s_rho_nr"] = 500.0 + j * 1.5, 0.001 * (j + 1)
    kl["rho0"], kl["s_rho0"] = -(700.0 + j * 0.5), 9000.0 + j
    kl["m_num"] = j % 7
    kl["m_id"] = np.where(j % 3 == 0, -1, j % 11)
    kl["m_id_kf"] = np.where(j % 2 == 0, j + 5, -1 - j % 3)
    kl["m_m0"], kl["n_m0"] = kl["m_m"] * F32(3), 77.0 + j
    for f in ("m_id_f", "p_id", "n_id", "net_id", "stereo_m_id"):
        kl[f] = -1
    assert len(kl) <= CAP
    return kl, mask, first, trap0, fwd0, place


def _sentinels(n, salt):
    """NaN payloads and plain values of its own per KeyLine."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt * 4096)
    v = ((2000.0 + 7 * salt) + np.arange(n)) * 1.0009765625
    b = v.view(np.uint64).copy()
    nan = i % np.uint64(3) == 0
    b[nan] = np.uint64(0x7FF8000000000000) | (i[nan] + np.uint64(1))
    neg = i % np.uint64(4) == 1
    b[neg] = np.uint64(0xFFF0000000000001) | (i[neg] << np.uint64(4))
    return b.view(F64)


def new_list(n, rot, ctx, pose, place, defaults=False):
    """n new KeyLines: KeyLine i belongs to class subs_of(ctx, pose)[(i + rot) % ...].  m_id = -1 and m_num = 0 as the detector leaves
    them; rho / s_rho are the class's search prior; the other six of the ten fields carry a sentinel of the KeyLine's own (NaN payloads
    in the doubles) — or, with defaults, what edge_finder.cpp:176-196 writes.  -> (list, index into SUBS per KeyLine)."""
    pool = subs_of(ctx, pose)
    wide = POSES[pose].get("wide", False)     # a diverged velocity: norm_t (rho - s_rho) ~ 1e6 is dq_min, and the reference walks half of it
    which = np.array([pool[(i + rot) % len(pool)] for i in range(n)], np.int64)
    occ = (np.arange(n) + rot) // len(pool)
    kl = np.zeros(n, KEYLINE_DTYPE)
    for i in range(n):
        s = SUBS[which[i]]
        m = s["new"]
        y_, x_ = place[s["name"]]
        val = lambda v: v(int(occ[i])) if callable(v) else v
        pm = [x_ - PP[0], y_ - PP[1]]
        for c, v in enumerate(m.get("pm", (None, None))):
            if v is not None:
                pm[c] = v
        kl["p_m"][i] = pm
        kl["c_p"][i] = (min(max(x_, 0.0), W - 1.0), min(max(y_, 0.0), H - 1.0))
        rho_, s_ = val(m["rho"]), val(m["s_rho"])
        if wide and math.isfinite(rho_) and math.isfinite(s_):
            s_ = abs(rho_) + abs(s_)
        kl["rho"][i], kl["s_rho"][i] = rho_, s_
        kl["m_m"][i], kl["n_m"][i] = m["m_m"], m["n_m"]
    kl["u_m"] = kl["m_m"]
    kl["p_inx"] = kl["c_p"][:, 1].astype(np.int32) * W + kl["c_p"][:, 0].astype(np.int32)
    kl["rho0"], kl["s_rho0"] = -5.0 - np.arange(n), -6.0 - np.arange(n)
    for f in ("m_id", "m_id_f", "p_id", "n_id", "net_id", "stereo_m_id"):
        kl[f] = -1
    kl["m_num"] = 0
    if defaults:
        kl["rho"], kl["s_rho"], kl["rho_nr"], kl["s_rho_nr"] = RHO_INIT, RHO_MAX, RHO_INIT, RHO_MAX
        kl["p_m_0"], kl["m_m0"], kl["n_m0"], kl["m_id_kf"] = kl["p_m"], 0.0, 0.0, -1
    else:
        kl["rho_nr"], kl["s_rho_nr"], kl["n_m0"] = _sentinels(n, 1), _sentinels(n, 2), _sentinels(n, 3)
        with np.errstate(invalid="ignore"):           # (the payloads of signalling patterns go through a cast)
            kl["p_m_0"] = np.stack([_sentinels(n, 4), _sentinels(n, 5)], 1).astype(F32)
            kl["m_m0"] = np.stack([-1000.0 - np.arange(n), _sentinels(n, 6)], 1).astype(F32)
        kl["m_id_kf"] = -1000 - np.arange(n)
    return kl, which


def garbage_ten(kl):
    """The list with garbage in the ten fields FordwardMatch / directed_matching write: what a detector in fill mode leaves."""
    g = kl.copy()
    n = len(g)
    g["rho"], g["s_rho"], g["rho_nr"], g["s_rho_nr"], g["n_m0"] = (_sentinels(n, 11 + c) for c in range(5))
    g["m_num"], g["m_id"], g["m_id_kf"] = 12345 + np.arange(n), 7 + np.arange(n), 99 - np.arange(n)
    g["p_m_0"], g["m_m0"] = np.full((n, 2), 1e9, F32), np.full((n, 2), -1e9, F32)
    return g


# ---- forward matches: classes of OLD KeyLines (the N_FWD KeyLines that are on no pixel) ----
NZ = -0.0
FWD_GROUPS = (
    ("increasing", (1.0, 2.0, 3.0)), ("decreasing", (3.0, 2.0, 1.0)), ("mixed", (2.0, 3.0, 1.0, 3.0, 2.0)), ("equal", (2.0, 2.0)),
    ("equal_three", (0.5, 0.5, 0.5)), ("negative", (-1.0, -3.0, -2.0)), ("pinf_first", (INF, 1.0)), ("pinf_last", (1.0, INF)),
    ("ninf_first", (-INF, 1.0)), ("ninf_last", (1.0, -INF)), ("inf_equal", (INF, INF)),
    ("zero_pn", (0.0, NZ)), ("zero_np", (NZ, 0.0)),
    ("nan_first", (NAN, 1.0, 2.0)), ("nan_middle", (1.0, NAN, 0.5)), ("nan_last", (1.0, 2.0, NAN)), ("nan_neg_last", (1.0, -NAN)),
    ("single", (4.0,)),
)
# where `>` on doubles and the order of the bits disagree: unreachable in the pipeline (rho comes out of the EKF's clamp to
# [RHO_MIN, RHO_MAX]); the device's rule is stated in forward_match(rule="device") and asserted for these groups by name
FWD_DEVICE_RULE = ("zero_pn", "nan_first", "nan_middle", "nan_neg_last")
# position in the group of the old KeyLine that wins, by :407 read by hand (reference) and by the order of the bits (device)
FWD_WINNER = dict(increasing=2, decreasing=0, mixed=3, equal=1, equal_three=2, negative=0, pinf_first=0, pinf_last=1, ninf_first=1, ninf_last=0,
                  inf_equal=1, zero_pn=1, zero_np=1, nan_first=2, nan_middle=2, nan_last=2, nan_neg_last=1, single=0)
FWD_WINNER_DEVICE = dict(FWD_WINNER, zero_pn=0, nan_first=0, nan_middle=1, nan_neg_last=0)
assert {k for k in FWD_WINNER if FWD_WINNER[k] != FWD_WINNER_DEVICE[k]} == set(FWD_DEVICE_RULE)
_FWD_REPEAT = 8
N_FWD = _FWD_REPEAT * sum(len(g) for _, g in FWD_GROUPS) + 4 * _FWD_REPEAT


def with_forward(old, fwd0, kn_new, salt=0):
    """The old list with its forward matches for a new list of kn_new KeyLines: every group of FWD_GROUPS eight times, each time at a
    target of its own (as long as kn_new has room: targets 0 .. kn_new - 2), then eight times m_id_f = kn_new - 1 (the last one),
    kn_new (one past: ignored), 2^30 and -1.  -> (list, {group name: [targets]})."""
    o = old.copy()
    i, f = fwd0, salt % 5
    targets = {}
    neg_nan = np.array([0xFFF8000000000001], np.uint64).view(F64)[0]
    for rep in range(_FWD_REPEAT):
        for name, rhos in FWD_GROUPS:
            ok = f < kn_new - 1
            for r in rhos:
                o["m_id_f"][i] = f if ok else -1
                o["rho"][i] = neg_nan if (r != r and math.copysign(1.0, r) < 0) else r
                i += 1
            if ok:
                targets.setdefault(name, []).append((f, i - len(rhos)))      # (target, first old KeyLine of the group)
                f += 1 + (rep + salt) % 2
    for rep in range(_FWD_REPEAT):
        for v in (kn_new - 1, kn_new, 2 ** 30, -1):
            o["m_id_f"][i] = v
            o["rho"][i] = 5.0 + rep
            i += 1
    assert i == len(o)
    if kn_new > 0:
        targets["last"] = [(kn_new - 1, i - 4)]                              # the last writer among equals... rho rises: the last repeat wins
    return o, targets


def jobs(combo_index):
    """[(length, rot)] in launch order for three sequences per launch: neighbours differ in length and class mix, and the mix of
    sequence 0 rotates from launch to launch and from combo to combo."""
    return [(n, 7 * j + 3 + 11 * combo_index) for j, n in enumerate(LENGTHS)]


# ---------------------------------------------------------------------------------------------------------------------------------
# The reference
# ---------------------------------------------------------------------------------------------------------------------------------
def make_reference(oracle, ctx, stereo_mode=False):
    orc = oracle.Oracle("ref", oracle.euroc_params(W, H, max_points=CAP, ppx=PP[0], ppy=PP[1], zfx=ZF, zfy=ZF, search_range=SEARCH_RANGE[ctx]), nslots=2)
    orc.set_stereo_mode(stereo_mode)
    return orc


def reference_chain(orc, old, mask, new, R0, BR, V, RVel, ctx):
    """FordwardMatch -> rotate_keylines(R0) -> directed_matching(BackRot) on the reference: slot 0 the old list, slot 1 the new one.
    -> dict(new list after the forward match, n_fwd, turned old list, new list after the directed match, nmatch, kf_matchs)."""
    orc.set_keylines(0, old, mask, 0.0)
    orc.set_keylines(1, new, None, 0.0)
    n_fwd = orc.forward_match(0, 1)
    fwd = orc.keylines(1).copy()
    orc.rotate_keylines(0, R0)
    turned = orc.keylines(0).copy()
    n, kf = orc.directed_matching(1, 0, V, RVel, BR, ARGS["min_thr_mod"], ARGS["min_thr_ang"], float(SEARCH_RANGE[ctx]), ARGS["loc_unc"])
    return dict(fwd=fwd, n_fwd=n_fwd, turned=turned, new=orc.keylines(1).copy(), nmatch=n, kf=kf)
