"""Plain-Python restatement of the reference's key-frame match repair (TrackKeyFrames): kfvo::buildForwardMatch,
forwardCorrectAugmentate / forwardStereoCorrect and correctAugmentate / stereoCorrect (src/mtracklib/kfvo.cpp:739-771, 969-1142, 804-966),
and the two resets (:774-787).

Two forms of the order-dependent phase 2 live here:
  order="serial"      the reference's loop: seeds i = 0 .. kn-1, each walking its p_id chain, then its n_id chain;
  order="components"  what rebvo_amd/csrc/keyframe_track.hip runs: components of the undirected graph of all p_id / n_id links, labelled by
                      their minimum index; per component its members in ascending index, components in any order (here: shuffled);
                      members that cannot act (no link to a KeyLine that is unmatched when phase 2 begins) are left out.
tools/make_keyframe_track_golden.py asserts serial == the reference on every id and count before it writes a fixture;
tests/test_keyframe_track_cpu.py asserts components == serial.

Everything is IEEE double in the reference's order of operations (TooN dot products accumulate in ascending index; p_m is widened from
float).  Every chain walk is capped at the length of the list it walks, as on the device: on finite p_m it ends before; a NaN p_m inside a
link cycle — where the reference never returns — ends at the cap and sets `guard`.
"""
import math
import random

import numpy as np


class Stats(dict):
    """Branch populations of a run (the fixture generator stores them)."""

    def hit(self, k, n=1):
        self[k] = self.get(k, 0) + n


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _mat_tn(A, B):
    """A^T * B, 3x3 as row-major lists of 9."""
    return [_dot3([A[0 * 3 + r], A[1 * 3 + r], A[2 * 3 + r]], [B[0 * 3 + c], B[1 * 3 + c], B[2 * 3 + c]]) for r in range(3) for c in range(3)]


def _essential(R, t):
    X = [0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0]   # util::crossMatrix
    return [_dot3(R[r * 3:r * 3 + 3], [X[c], X[3 + c], X[6 + c]]) for r in range(3) for c in range(3)]


def _f9(M):
    return [float(x) for x in np.asarray(M, np.float64).reshape(9)]


def _f3(v):
    return [float(x) for x in np.asarray(v, np.float64).reshape(3)]


def essential_forward(kf_Pose, kf_Pos, Pose, Pos):
    """kfvo.cpp:972-974: R = Pose^T kf.Pose, t = kf.Pose^T (Pos - kf.Pos), E = R [t]x."""
    KP, Kt, P, T = _f9(kf_Pose), _f3(kf_Pos), _f9(Pose), _f3(Pos)
    R = _mat_tn(P, KP)
    d = [T[i] - Kt[i] for i in range(3)]
    t = [_dot3([KP[0 * 3 + i], KP[1 * 3 + i], KP[2 * 3 + i]], d) for i in range(3)]
    return _essential(R, t)


def essential_back(kf_Pose, kf_Pos, Pose, Pos):
    """kfvo.cpp:896-898: R = kf.Pose^T Pose, t = Pose^T (kf.Pos - Pos)."""
    KP, Kt, P, T = _f9(kf_Pose), _f3(kf_Pos), _f9(Pose), _f3(Pos)
    R = _mat_tn(KP, P)
    d = [Kt[i] - T[i] for i in range(3)]
    t = [_dot3([P[0 * 3 + i], P[1 * 3 + i], P[2 * 3 + i]], d) for i in range(3)]
    return _essential(R, t)


def local_pose(Pose, R, Pos, V, K):
    """rebvo_second_t.cpp:435-436: localPose = Pose * R, localPos = Pos - localPose * V * K."""
    P, Rm, T, Vv = _f9(Pose), _f9(R), _f3(Pos), _f3(V)
    LP = [_dot3(P[r * 3:r * 3 + 3], [Rm[c], Rm[3 + c], Rm[6 + c]]) for r in range(3) for c in range(3)]
    LT = [T[i] - _dot3(LP[i * 3:i * 3 + 3], Vv) * float(K) for i in range(3)]
    return np.array(LP).reshape(3, 3), np.array(LT)


class _List:
    """The fields of a KeyLine list the repair reads, as Python lists."""

    def __init__(self, p_m, p_id, n_id):
        pm = np.asarray(p_m, np.float32).reshape(-1, 2)
        self.x = [float(v) for v in pm[:, 0]]
        self.y = [float(v) for v in pm[:, 1]]
        self.p = [int(v) for v in p_id]
        self.n = [int(v) for v in n_id]
        self.kn = len(self.x)


def slide(E, zf, x, y, f, oth, tol, st, guard):
    """forwardStereoCorrect / stereoCorrect of a KeyLine at (x, y) with match f -> (distance, match)."""
    if f < 0:
        return -1.0, f
    e0 = (E[0] * x + E[1] * y) + E[2] * zf
    e1 = (E[3] * x + E[4] * y) + E[5] * zf
    e2 = (E[6] * x + E[7] * y) + E[8] * zf
    nrm = math.sqrt(e0 * e0 + e1 * e1)
    r0, r1, r2 = _div(e0, nrm), _div(e1, nrm), _div(e2, nrm) * zf

    def dist(j):
        return abs((oth.x[j] * r0 + oth.y[j] * r1) + r2)

    def link(l, j):
        t = l[j]
        return t if t < oth.kn else -1

    d0 = dist(f)
    if d0 < tol:
        st.hit("slide_tolerance_at_once")
        return d0, f
    steps = 0
    for side, l in (("n", oth.n), ("p", oth.p)):
        nx = link(l, f)
        if nx < 0:
            continue
        d = dist(nx)
        if not d < d0:
            continue
        st.hit("slide_along_" + side)
        while True:
            f, d0 = nx, d
            if d0 < tol:
                st.hit("slide_stop_tolerance")
                return d0, f
            nx = link(l, f)
            if nx < 0:
                st.hit("slide_stop_chain_end")
                return d0, f
            d = dist(nx)
            if d >= d0:
                st.hit("slide_stop_non_decrease")
                return d0, f
            steps += 1
            if steps > oth.kn:
                guard[0] |= 1
                return d0, f
    return d0, f


def _augment_seed(i, own, m, oth, E, zf, thresh, tol, st, guard, book):
    if m[i] < 0:
        return
    filled_any = False
    for l in (own.p, own.n):
        kl, steps = i, 0
        while True:
            j = l[kl]
            if j < 0 or j >= own.kn:
                st.hit("walk_stop_missing_link")
                break
            if m[j] >= 0:
                st.hit("walk_stop_matched")
                if book["filled_by"].get(j, i) != i:
                    st.hit("walk_met_other_seed_fill")   # two seeds competed for one unmatched run
                break
            d, f = slide(E, zf, own.x[j], own.y[j], m[kl], oth, tol, st, guard)
            if d > thresh:
                m[j] = -1
                book["failed"].add(j)
                book["fail_value"][j] = f
                st.hit("walk_stop_failed_correction")
                break
            m[j] = f
            filled_any = True
            book["filled_by"][j] = i
            if j in book["failed"] and f != book["fail_value"].get(j):
                st.hit("filled_after_failure_from_other_side")
            kl = j
            steps += 1
            if steps > own.kn:
                guard[0] |= 1
                break
    if filled_any and book["dist"][i] > thresh:
        st.hit("far_seed_propagated")


def components(p_id, n_id, kn):
    """Label of every KeyLine = minimum index of its component in the undirected graph of all in-range p_id / n_id links."""
    lab = list(range(kn))

    def find(i):
        while lab[i] != i:
            lab[i] = lab[lab[i]]
            i = lab[i]
        return i
    for i in range(kn):
        for j in (p_id[i], n_id[i]):
            if 0 <= j < kn and j != i:
                a, b = find(i), find(j)
                if a != b:
                    lab[max(a, b)] = min(a, b)
    return [find(i) for i in range(kn)]


def correct_augment(own_pm, own_p, own_n, own_m, oth_pm, oth_p, oth_n, E, zf, dist_thresh, dist_tolerance, augmentate=True,
                    order="serial", rng=None, stats=None):
    """The three phases on the own list's matches `own_m` (m_id_f of the key frame against the new list, or m_id_kf of the new list
    against the key frame) -> (matches int32[kn], count, guard)."""
    own, oth = _List(own_pm, own_p, own_n), _List(oth_pm, oth_p, oth_n)
    m = [int(v) for v in own_m]
    st = stats if stats is not None else Stats()
    guard = [0]
    E, zf = [float(v) for v in E], float(zf)
    dist = [0.0] * own.kn
    for i in range(own.kn):   # phase 1
        dist[i], m[i] = slide(E, zf, own.x[i], own.y[i], m[i], oth, dist_tolerance, st, guard)
    if augmentate:            # phase 2
        book = {"filled_by": {}, "failed": set(), "fail_value": {}, "dist": dist}
        if order == "serial":
            seeds = range(own.kn)
        else:
            lab = components(own.p, own.n, own.kn)
            groups = {}
            for i in range(own.kn):
                # only members that can act are seeds: one of their links names a KeyLine that is unmatched now (during phase 2 a
                # KeyLine never goes from matched to unmatched, so the others walk nowhere whenever their turn comes)
                if any(0 <= j < own.kn and m[j] < 0 for j in (own.p[i], own.n[i])):
                    groups.setdefault(lab[i], []).append(i)   # ascending index inside a component
            roots = list(groups)
            (rng or random.Random(0)).shuffle(roots)      # components in any order
            seeds = [i for r in roots for i in groups[r]]
        for i in seeds:
            _augment_seed(i, own, m, oth, E, zf, dist_thresh, dist_tolerance, st, guard, book)
    count = 0
    for i in range(own.kn):   # phase 3
        if dist[i] > dist_thresh:
            m[i] = -1
        if m[i] >= 0:
            count += 1
    return np.array(m, np.int32), count, guard[0]


def build_forward_match(kf_m_id_f, new_m_id, old_kn):
    """kfvo::buildForwardMatch -> (m_id_f int32[kf kn], count); the last i with new[i].m_id == j wins fowMatch[j]."""
    fow = [-1] * max(int(old_kn), 0)
    for i, mm in enumerate(new_m_id):
        if mm >= 0:
            fow[int(mm)] = i
    out = np.array(kf_m_id_f, np.int32).copy()
    count = 0
    for i, f in enumerate(out):
        if f >= 0:
            nm = fow[int(f)]
            out[i] = nm if nm >= 0 else -1
            count += nm >= 0
    return out, int(count)


def forward_correct_augmentate(kf, new, Pose, Pos, zf, dist_thresh=10.0, dist_tolerance=0.0, augmentate=True, **kw):
    """kf / new: dicts with p_m, p_id, n_id (+ kf: m_id_f, Pose, Pos) -> (kf m_id_f, count, guard)."""
    E = essential_forward(kf["Pose"], kf["Pos"], Pose, Pos)
    return correct_augment(kf["p_m"], kf["p_id"], kf["n_id"], kf["m_id_f"], new["p_m"], new["p_id"], new["n_id"], E, zf,
                           dist_thresh, dist_tolerance, augmentate, **kw)


def back_correct_augmentate(kf, new, Pose, Pos, zf, dist_thresh=10.0, dist_tolerance=0.0, augmentate=True, **kw):
    """-> (new m_id_kf, count, guard)."""
    E = essential_back(kf["Pose"], kf["Pos"], Pose, Pos)
    return correct_augment(new["p_m"], new["p_id"], new["n_id"], new["m_id_kf"], kf["p_m"], kf["p_id"], kf["n_id"], E, zf,
                           dist_thresh, dist_tolerance, augmentate, **kw)


def track_frame(kf, new, old_kn, Pose, Pos, zf, dist_thresh=10.0, dist_tolerance=0.0, augmentate=True, order="serial", stats=None):
    """The three steps of rebvo_second_t.cpp:432-442 -> dict of ids and counts after each."""
    out = {}
    out["m_id_f_0"], out["fow_m0"] = build_forward_match(kf["m_id_f"], new["m_id"], old_kn)
    kf1 = dict(kf, m_id_f=out["m_id_f_0"])
    out["m_id_f_1"], out["fow_m"], g1 = forward_correct_augmentate(kf1, new, Pose, Pos, zf, dist_thresh, dist_tolerance, augmentate,
                                                                    order=order, stats=stats)
    out["m_id_kf_1"], out["back_m"], g2 = back_correct_augmentate(kf, new, Pose, Pos, zf, dist_thresh, dist_tolerance, augmentate,
                                                                  order=order, stats=stats)
    out["guard"] = g1 | g2
    return out
