"""Crafted KeyLine lists for the tracker's evaluations — global_tracker::TryVelRot (global_tracker.cpp:289-543), TryVel (:830-934) and the
minimisers around them (:580-819, :1037-1093) — shared by tests/test_tracker_crafted_cpu.py (the reference alone: the lists reach what
they claim) and tests/test_tracker_crafted_gpu.py (k_try_velrot, k_try_velrot2, k_try_vel and the LM steps against the reference).  This
module imports no GPU code; the compiled reference (oracle/_ref) is the only oracle, there is no numpy restatement of the tracker.

What the lists are for.  TryVelRot keeps ONE scalar `fi` across its loop (:344): a KeyLine that is in the image but fails Test_f_k (or
finds an empty field entry) writes DResidualNew = the fi of the last matched KeyLine before it (:391, :406), however far back, and 0 when
there is none.  The device rebuilds that carry from a ballot inside a wave, s_whas / s_wlast across the waves of a 256-KeyLine block, a NaN
marker in the residual buffer and block_last -> resid_carry across blocks; k_try_vel has a copy of the machinery.  On rendered pairs
most KeyLines match, so runs of unmatched KeyLines longer than a wave never occur.  Here they do.

Family A, "edited donor" (376 x 240, default cap): helpers.oracle_pair(376, 240, 4); the new list, its mask and its field stay as
detected; the old list is edited field by field.  An edit makes a KeyLine
  skipped         s_rho = 20 (RHO_MAX, what the detector initialises) — above the gate;
  out of image    p_m.x = -ppx - 4: four pixels left of the image under every pose used here;
  unmatched       m_m turned by 90 degrees, n_m kept: |m . f_m - n^2| ~ n^2 > 0.5 n^2 against the KeyLines of its own edge (where the field holds
                  another edge's KeyLine, one in ten, the turn is -90 or 180 degrees instead, or the KeyLine copies a neighbour: family_a.settle);
  matched         (the "anchors" that bound a run) p_m, rho, s_rho, m_m, u_m, n_m, m_num copied from the nearest KeyLine that the
                  reference matches under EVERY evaluation point of the protocol.
KeyLines inside a run that the donor would skip or lose over the border under some pose get s_rho / (p_m, rho) of such a KeyLine too, so
that a run is unmatched KeyLines and nothing else.  Variants: runs, head, tail, hole, none, plain (VARIANTS_A), gates, behind; the `record` pair edits the
NEW list (one u_m[0] moved by one float ulp) so that edgehip_upload_keylines must choose the 32-byte gather record.

Family B, "exact grid" (the geometry of matching_crafted.py: 160 x 120, max_points = 2048, principal point (80, 60), zf = 128, X = 0):
with rho a power of two 1 / rho, x z / zf, zf rho_p x are all exact, so an old KeyLine projects to p_m + pp exactly and every old
KeyLine is aimed at the pixel of one new KeyLine (or at none).  Classes: border, test_f_k, empty / perp, behind, plain, carry.

Out of domain (not built).  The kernels form 1 / rho, 1 / z, k / |r| and x / q_rho with division and square-root sequences that drop the
exponent scaling of the compiler's own (rebvo_amd/csrc/ctx.h:143-149 div_mid / inv_mid / MidDivisor: "operands in the middle of the
exponent range", |exponent| below ~900; :206-208 div_rn: "no operand here is near the exponent range's ends"; :214-216 sqrt_ge1:
arguments >= 1; :233-235 sqrtf_mid and :249-252 div2_mid_f32: a gradient modulus that passed the detector's threshold).  So: no
subnormal or huge rho / s_rho, no rho = 0 on an evaluated KeyLine, no NaN and no infinity.  Everything built here has |rho| in
[2^-3, 2^4] (family B) or the detector's and the EKF's own [1e-3, 20] (family A).  The skipped KeyLine with s_rho = 0 is covered by
tests/test_whole_batch_vs_ref_gpu.py.
"""
import functools

import numpy as np

from oracle.oracle import KEYLINE_DTYPE

F32, F64 = np.float32, np.float64
BLOCK = 256                                            # KeyLines per evaluation block (kTvrBlock; k_try_vel's blocks too)
W_A, H_A = 376, 240
MAX_R = 40                                             # field radius = max_r of family A (the shipped SearchRange)
MATCH_THRESH, K_HUBER = 0.5, 2.0
RUN_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 513)
CUTS = (513, 1, None, 256, 255, 257, 511, 512)         # None = the full length; a short list follows a long one in the same context
MODES = ((False, True), (True, True), (False, False), (True, False))      # (reweight, procjf) of the pass under test
SKIPPED, OUT, MATCHED, UNMATCHED = 0, 1, 2, 3          # the kernel's own status codes
VARIANTS_A = ("runs", "head", "tail", "hole", "none", "plain")
HEAD_LEN, TAIL_START, HOLE = 300, 200, (500, 1030)     # hole: KeyLines 500 .. 1030 unmatched — blocks 2 and 3 hold no match
GATE_SETS = ("s_rho_at", "s_rho_above", "s_rho_below", "m_num_-1", "m_num_0", "m_num_1", "m_num_2", "m_num_3")
GATE_POP = 16
GATES_MNT, GATES_FC = 2, (0, 1, 5)
BEHIND = ((100, 140), (256, 512), (700, 764))


# ---------------------------------------------------------------------------------------------------------------------------------
# The reference's evaluation and what it says about every KeyLine
# ---------------------------------------------------------------------------------------------------------------------------------
def evaluate(orc, sn, so, X, gate, mnt, reweight, procjf, resid_in=None, match_thresh=MATCH_THRESH, k_huber=K_HUBER):
    F, JtJ, JtF, r = orc.try_velrot(sn, so, np.asarray(X, F64), reweight, procjf, match_thresh, gate, mnt, k_huber, resid_in=resid_in)
    return dict(F=F, JtJ=JtJ, JtF=JtF, r=r, mid=orc.keylines(so)["m_id_f"].copy())


def two_pass(orc, sn, so, X, gate, mnt, reweight, procjf, match_thresh=MATCH_THRESH, k_huber=K_HUBER):
    """The protocol of the GPU test: pass 1 unweighted at X / 2 (buffer 1), pass 2 under test at X reading it (buffer 2)."""
    X = np.asarray(X, F64)
    p1 = evaluate(orc, sn, so, X * 0.5, gate, mnt, False, True, None, match_thresh, k_huber)
    p2 = evaluate(orc, sn, so, X, gate, mnt, reweight, procjf, p1["r"], match_thresh, k_huber)
    return p1, p2


def gate_skips(kl, gate, mnt=0, fc=0):
    """global_tracker.cpp:356 on the inputs: int m_num against an unsigned threshold."""
    return (kl["s_rho"] > gate) | (kl["m_num"].astype(np.uint32) < np.uint32(min(mnt, fc)))


def classify(kl, ev, gate, mnt=0, fc=0, max_r=MAX_R):
    """Status of every old KeyLine, from the gate on the inputs and the reference's own outputs."""
    st = np.full(len(kl), UNMATCHED, np.int8)
    st[(ev["r"][:len(kl)] == max_r) & (ev["mid"] == -1)] = OUT
    st[ev["mid"] >= 0] = MATCHED
    st[gate_skips(kl, gate, mnt, fc)] = SKIPPED
    return st


def carry_runs(st):
    """Maximal runs of unmatched KeyLines with no matched KeyLine between them (skipped and out-of-image KeyLines neither feed the
    carry nor reset it) -> [(first, last, number of unmatched KeyLines)]."""
    runs, cur = [], None
    for i, s in enumerate(st):
        if s == UNMATCHED:
            cur = [i, i, 1] if cur is None else [cur[0], i, cur[2] + 1]
        elif s == MATCHED and cur is not None:
            runs.append(tuple(cur))
            cur = None
    if cur is not None:
        runs.append(tuple(cur))
    return runs


def cut(kl, mask, n):
    from helpers import cut_list
    return (kl, mask) if n is None or n >= len(kl) else cut_list(kl, mask, n)


def consistent_u_m(kl):
    """The host's expression of edgehip_upload_keylines (u_m == m_m / sqrt(m_m . m_m), every step a float) per KeyLine."""
    mx, my = kl["m_m"][:, 0], kl["m_m"][:, 1]
    n2 = mx * mx
    t2 = my * my
    nn = np.sqrt(n2 + t2)
    assert nn.dtype == F32
    with np.errstate(all="ignore"):
        return (mx / nn == kl["u_m"][:, 0]) & (my / nn == kl["u_m"][:, 1])


# ---------------------------------------------------------------------------------------------------------------------------------
# Family A
# ---------------------------------------------------------------------------------------------------------------------------------
GEOMETRY = ("p_m", "rho", "s_rho", "m_m", "u_m", "n_m", "m_num")


TURNS = ((0.0, -1.0, 1.0, 0.0), (0.0, 1.0, -1.0, 0.0), (-1.0, 0.0, 0.0, -1.0))      # +90, -90, 180 degrees: exact in float


def _turn(kl, src, idx, k=0):
    """m_m and u_m of the KeyLines idx = those of `src` turned by TURNS[k]; n_m stays."""
    a, b, c, d = (F32(v) for v in TURNS[k])
    for f in ("m_m", "u_m"):
        m = src[f][idx]
        kl[f][idx] = np.stack([a * m[:, 0] + b * m[:, 1], c * m[:, 0] + d * m[:, 1]], 1)


def run_layout(kn):
    """[(start, length, kind)]: every length of RUN_LENGTHS once from a multiple of 256 and once from an odd offset, in turns, then the
    interleaved run (kind "mixed": KeyLine j of it is unmatched for j % 4 < 2, skipped for j % 4 == 2, out of image for j % 4 == 3)."""
    runs, cursor = [], 1
    for k, L in enumerate(RUN_LENGTHS):
        start = -(-(cursor + 1) // BLOCK) * BLOCK
        runs.append((start, L, "aligned"))
        cursor = start + L
        L2 = RUN_LENGTHS[(k + 3) % len(RUN_LENGTHS)]
        start = cursor + 2
        start += (start % 2 == 0)
        assert start % BLOCK != 0
        runs.append((start, L2, "odd"))
        cursor = start + L2
    start = cursor + 3
    start += (start % 2 == 0)
    runs.append((start, 400, "mixed"))
    assert start + 400 + 1 < kn, (start, kn)
    return runs


@functools.lru_cache(maxsize=None)
def family_a():
    """-> dict(orc, so, sn, nav, gate, poses, old (the donor's old list), old_mask, old_retuned, new, new_mask, new_retuned, variants =
    {name: old list}, runs = {name: [(start, length, kind)]}, gate_sets = {set: indices}, robust = indices of the anchors' sources,
    record = dict(new list edited, index))."""
    from helpers import oracle_pair
    orc, so, sn, nav, _ = oracle_pair(W_A, H_A, 4)
    old, new = orc.keylines(so), orc.keylines(sn)
    old_mask, new_mask, old_ret, new_ret = orc.mask(so), orc.mask(sn), orc.retuned(so), orc.retuned(sn)
    gate = orc.quantile(so)
    orc.build_field(sn, MAX_R, new_ret)
    rs = np.random.RandomState(1)
    poses = [np.zeros(6), np.r_[np.array(nav.V[:]), np.array(nav.W[:])], rs.normal(size=6) * np.array([3e-3] * 3 + [2e-3] * 3)]
    points = [poses[0]] + [f * p for p in poses[1:] for f in (0.5, 1.0)]
    kn = len(old)
    # robust: evaluated, matched under every evaluation point; steady: in the image under every evaluation point
    robust = old["s_rho"] <= gate
    steady = np.ones(kn, bool)
    for X in points:
        robust &= classify(old, evaluate(orc, sn, so, X, gate, 0, False, True), gate) == MATCHED
        steady &= classify(old, evaluate(orc, sn, so, X, 1e30, 0, False, True), 1e30) != OUT      # (also of the KeyLines the gate skips)
    robust_i = np.nonzero(robust)[0]
    assert len(robust_i) > kn // 3, len(robust_i)

    def nearest(i):
        j = np.searchsorted(robust_i, i)
        c = robust_i[[max(j - 1, 0), min(j, len(robust_i) - 1)]]
        return int(c[np.argmin(np.abs(c - i))])

    def anchor(kl, i):
        if 0 <= i < kn:
            src = nearest(i)
            for f in GEOMETRY:
                kl[f][i] = old[f][src]

    def unmatched(kl, lo, hi):
        """KeyLines lo .. hi - 1: evaluated, in the image, Test_f_k fails."""
        idx = np.arange(lo, hi)
        for i in idx[old["s_rho"][idx] > gate]:
            kl["s_rho"][i] = old["s_rho"][nearest(i)]
        for i in idx[~steady[idx]]:
            src = nearest(i)
            kl["p_m"][i], kl["rho"][i] = old["p_m"][src], old["rho"][src]
        _turn(kl, old, idx)
        turned.extend(idx)

    def settle(kl):
        """A quarter turn leaves a KeyLine matched where the field holds a KeyLine of another edge, about one in ten: such a KeyLine takes
        the opposite quarter turn, then the half turn, until the reference matches it under no evaluation point."""
        idx = np.array(sorted(set(turned)), np.int64)
        del turned[:]
        for k in (1, 2, 0):
            orc.set_keylines(so, kl, old_mask, old_ret)
            hit = np.zeros(kn, bool)
            for X in points + [np.r_[V_STARTS[1], 0.0, 0.0, 0.0]]:      # (and where Minimizer_V's second start looks first)
                hit |= evaluate(orc, sn, so, X, gate, 0, False, True)["mid"] >= 0
            again = idx[hit[idx]]
            if len(again) == 0:
                return 0
            if k:
                _turn(kl, old, again, k)
                continue
            # every turn matches somewhere (the field holds other KeyLines at the pixels of other poses): such a KeyLine becomes a copy
            # of the nearest turned KeyLine that is settled
            good = idx[~hit[idx]]
            for i in again:
                src = good[np.argmin(np.abs(good - i))]
                for f in GEOMETRY:
                    kl[f][i] = kl[f][src]
            return len(again)

    def skip(kl, idx):
        kl["s_rho"][idx] = 20.0

    def outside(kl, idx):
        kl["p_m"][idx, 0] = F32(-float(F32(orc.p.ppx)) - 4.0)
        kl["s_rho"][idx] = np.minimum(kl["s_rho"][idx], gate * 0.5)

    variants, runs, turned, left = {"plain": old.copy()}, {}, [], {}
    # runs
    kl = old.copy()
    layout = run_layout(kn)
    for start, L, kind in layout:
        if kind == "mixed":
            j = np.arange(L)
            u = start + j[j % 4 < 2]
            for a, b in zip(u[::2], u[1::2]):
                unmatched(kl, a, b + 1)
            skip(kl, start + j[j % 4 == 2])
            outside(kl, start + j[j % 4 == 3])
        else:
            unmatched(kl, start, start + L)
        anchor(kl, start - 1)
        anchor(kl, start + L)
    left["runs"] = settle(kl)
    variants["runs"], runs["runs"] = kl, layout
    # head, tail, hole, none
    kl = old.copy()
    unmatched(kl, 0, HEAD_LEN)
    anchor(kl, HEAD_LEN)
    left["head"] = settle(kl)
    variants["head"], runs["head"] = kl, [(0, HEAD_LEN, "head")]
    kl = old.copy()
    unmatched(kl, TAIL_START, kn)
    anchor(kl, TAIL_START - 1)
    left["tail"] = settle(kl)
    variants["tail"], runs["tail"] = kl, [(TAIL_START, kn - TAIL_START, "tail")]
    kl = old.copy()
    unmatched(kl, HOLE[0], HOLE[1] + 1)
    anchor(kl, HOLE[0] - 1)
    anchor(kl, HOLE[1] + 1)
    left["hole"] = settle(kl)
    variants["hole"], runs["hole"] = kl, [(HOLE[0], HOLE[1] + 1 - HOLE[0], "hole")]
    kl = old.copy()
    _turn(kl, old, np.arange(kn))
    turned.extend(range(kn))
    left["none"] = settle(kl)
    variants["none"] = kl
    # behind (Minimizer_V only): a whole block and a part of another with rho < 0, so that 1 / rho + V[2] <= 0 (global_tracker.cpp:869-874)
    kl = old.copy()
    for lo, hi in BEHIND:
        kl["rho"][lo:hi] = -kl["rho"][lo:hi]
    variants["behind"] = kl
    # gates: disjoint sets of robust KeyLines, a quarter of each inside the first 250 so that every cut but the shortest holds some
    kl = old.copy()
    early, late = robust_i[robust_i < 250], robust_i[robust_i >= 250]
    q = GATE_POP // 4
    assert len(early) >= q * len(GATE_SETS) and len(late) >= (GATE_POP - q) * len(GATE_SETS)
    pe, pl = rs.permutation(early), rs.permutation(late)
    gate_sets = {n: np.sort(np.r_[pe[j * q:(j + 1) * q], pl[j * (GATE_POP - q):(j + 1) * (GATE_POP - q)]]) for j, n in enumerate(GATE_SETS)}
    kl["s_rho"][gate_sets["s_rho_at"]] = gate
    kl["s_rho"][gate_sets["s_rho_above"]] = np.nextafter(gate, np.inf)
    kl["s_rho"][gate_sets["s_rho_below"]] = np.nextafter(gate, 0.0)
    for v in (-1, 0, 1, 2, 3):
        kl["m_num"][gate_sets[f"m_num_{v}"]] = v
    variants["gates"] = kl
    # record: the new KeyLine most old KeyLines match at X = 0, its u_m[0] one float ulp away
    orc.set_keylines(so, old, old_mask, old_ret)
    ev = evaluate(orc, sn, so, poses[0], gate, 0, False, True)
    hit = np.bincount(ev["mid"][ev["mid"] >= 0], minlength=len(new))
    hit = hit + 1000 * np.bincount(ev["mid"][:255][ev["mid"][:255] >= 0], minlength=len(new))      # (seen from the short cuts too)
    assert consistent_u_m(new).all(), "the detector's own list fails the host's consistency expression"
    rec_new = None
    for j in np.argsort(-hit):
        cand = new.copy()
        cand["u_m"][j, 0] = np.nextafter(cand["u_m"][j, 0], F32(2.0) if cand["u_m"][j, 0] < 0.5 else F32(0.0))
        if (~consistent_u_m(cand)).sum() == 1:
            rec_new, rec_j = cand, int(j)
            break
    assert rec_new is not None
    orc.set_keylines(so, old, old_mask, old_ret)
    return dict(orc=orc, so=so, sn=sn, nav=nav, gate=gate, poses=poses, points=points, old=old, old_mask=old_mask, old_retuned=old_ret, new=new,
                new_mask=new_mask, new_retuned=new_ret, variants=variants, runs=runs, gate_sets=gate_sets, robust=robust_i,
                record=dict(new=rec_new, index=rec_j, hits=int(hit[rec_j])), copied=left)


def jobs_a(names=VARIANTS_A, nseq=3):
    """[(cut, [variant per sequence])] in launch order: per cut, the variants in groups of nseq; the group's order rotates from launch to
    launch so that sequence 0 holds another variant every time."""
    out, k = [], 0
    names = list(names)
    for c in CUTS:
        for g in range(0, len(names), nseq):
            grp = [names[(g + j) % len(names)] for j in range(nseq)]
            out.append((c, grp[k % nseq:] + grp[:k % nseq]))
            k += 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Family B
# ---------------------------------------------------------------------------------------------------------------------------------
W_B, H_B, CAP_B = 160, 120, 2048
ZF_B, PP_B = 128.0, (80.0, 60.0)
MAX_R_B = 4                                            # field radius: a new KeyLine paints x - 4 .. x + 3 of its row
GATE_B = 8.0
MIN_POP = 8
RHOS = (1.0, 0.5, 2.0, 4.0, 0.25, 8.0, 0.125, 16.0)
_DN = lambda v: float(np.nextafter(F32(v), F32(-np.inf)))
BORDER_X = (0.0, 1.0, W_B - 2.0, W_B - 1.0, 0.5, _DN(0.5 - 80) + 80, W_B - 1.5, _DN(W_B - 1.5 - 80) + 80, _DN(0.0 - 80) + 80, -0.25, -1.0)
BORDER_Y = (0.0, 1.0, H_B - 2.0, H_B - 1.0, 0.5, _DN(0.5 - 60) + 60, H_B - 1.5, _DN(H_B - 1.5 - 60) + 60, _DN(0.0 - 60) + 60, -0.25, -1.0)
TFK_F = (3.0, float(np.nextafter(F32(3), F32(4))), 1.0, float(np.nextafter(F32(1), F32(0))))      # f_m.x: on / beyond the threshold, twice
TFK_MATCH = (True, False, True, False)
CARRY_LEN = 340


def _pixel(p):
    """round2int_positive of an exact projection (global_tracker.cpp:367; util.h:43): (int)(p + 0.5), truncation towards zero."""
    return int(np.trunc(p + 0.5))


@functools.lru_cache(maxsize=None)
def family_b(salt=0):
    """-> dict(new, new_mask, old, cls (class name per old KeyLine), expect (index of the new KeyLine it must match; -1 unmatched in the
    image; -2 out of image), fi (the exact residual of a matched one), carry = (first, last) of the long unmatched run)."""
    new, old = [], []

    def target(x, y, m=(3.0, 0.0)):
        new.append(dict(x=float(x), y=float(y), m=m))
        return len(new) - 1

    def aim(cls, px, py, k, expect, m=(2.0, 0.0), n_m=2.0, sign=1.0):
        old.append(dict(cls=cls, px=px, py=py, rho=sign * RHOS[(k + salt) % len(RHOS)], m=m, n_m=n_m, expect=expect))

    # targets: plain ones on a grid in rows 8 .. 46, the border ones, the Test_f_k ones, the perpendicular ones
    grid = [target(x, y) for y in range(8, 26, 2) for x in range(12, 150, 12)]
    bx = {(x, y): target(x, y) for y in (30, 34) for x in (1, W_B - 2)}
    by = {(x, y): target(x, y) for x in (40, 100) for y in (1, H_B - 2)}
    tfk = [target(20 + 12 * j, 40, m=(f, 0.0)) for j, f in enumerate(TFK_F)]
    perp = [target(20 + 12 * j, 44, m=(0.0, 2.0)) for j in range(4)]
    offs = (0.0, 0.25, -0.25, 0.125, -0.375, 0.375, -0.125, 0.4375)

    def plain(n, k0):
        for k in range(n):
            t = grid[(k0 + k + 5 * salt) % len(grid)]
            aim("plain", new[t]["x"] + offs[(k0 + k) % 8], new[t]["y"] + offs[(k0 + 3 * k) % 8], k, t)

    def border():
        for k, p in enumerate(BORDER_X):
            for y in (30, 34):
                x = _pixel(p)
                aim("border", p, float(y), k, bx[(x, y)] if 1 <= x < W_B - 1 else -2)
        for k, p in enumerate(BORDER_Y):
            for x in (40, 100):
                y = _pixel(p)
                aim("border", float(x), p, k, by[(x, y)] if 1 <= y < H_B - 1 else -2)

    def test_f_k():
        for j, t in enumerate(tfk):
            for k in range(4):
                aim("test_f_k", new[t]["x"] + offs[k], 40.0, k + j, t if TFK_MATCH[j] else -1)

    def empty(n, cls="empty"):
        for k in range(n):
            aim(cls, 20.0 + (k * 7) % 120 + offs[k % 8], 60.0 + (k * 3) % 50, k, -1)

    def perpendicular():
        for k in range(MIN_POP):
            aim("perp", new[perp[k % 4]]["x"] + offs[k], 44.0, k, -1)

    def behind():
        for k in range(MIN_POP):
            t = grid[(11 + k) % len(grid)]
            aim("behind", new[t]["x"] + offs[k], new[t]["y"], k, t, sign=-1.0)

    parts = [lambda: plain(16, 0), test_f_k, border, perpendicular, behind, lambda: empty(MIN_POP)]
    for f in parts[salt % len(parts):] + parts[:salt % len(parts)]:
        f()
    plain(190 + 13 * salt - len(old), 3)                 # up to the carry run: a matched KeyLine with fi != 0 right before it
    c0 = len(old)
    empty(CARRY_LEN, "carry")                            # an unmatched run over two block boundaries
    plain(MIN_POP, 1)
    behind()
    empty(MIN_POP)
    plain(MIN_POP, 6)

    nk = np.zeros(len(new), KEYLINE_DTYPE)
    new_mask = np.full((H_B, W_B), -1, np.int32)
    for j, t in enumerate(new):
        nk["c_p"][j] = (t["x"], t["y"])
        nk["p_m"][j] = (t["x"] - PP_B[0], t["y"] - PP_B[1])
        nk["p_inx"][j] = int(t["y"]) * W_B + int(t["x"])
        nk["m_m"][j] = t["m"]
        new_mask[int(t["y"]), int(t["x"])] = j
    mx, my = nk["m_m"][:, 0], nk["m_m"][:, 1]
    nn = np.sqrt(mx * mx + my * my)
    nk["n_m"] = nn
    nk["u_m"] = np.stack([mx / nn, my / nn], 1)
    assert consistent_u_m(nk).all()
    nk["rho"], nk["s_rho"], nk["rho_nr"], nk["s_rho_nr"] = 1.0, 20.0, 1.0, 20.0
    nk["p_m_0"] = nk["p_m"]
    for f in ("m_id", "m_id_f", "m_id_kf", "p_id", "n_id", "net_id", "stereo_m_id"):
        nk[f] = -1

    ok = np.zeros(len(old), KEYLINE_DTYPE)
    for i, o in enumerate(old):
        pm = (F32(o["px"] - PP_B[0]), F32(o["py"] - PP_B[1]))
        assert float(pm[0]) + PP_B[0] == o["px"] and float(pm[1]) + PP_B[1] == o["py"], o      # the aim is exact in float
        ok["p_m"][i] = pm
        ok["c_p"][i] = (min(max(o["px"], 0.0), W_B - 1.0), min(max(o["py"], 0.0), H_B - 1.0))
        ok["rho"][i], ok["m_m"][i], ok["n_m"][i] = o["rho"], o["m"], o["n_m"]
    ok["u_m"] = ok["m_m"] / ok["n_m"][:, None]
    ok["s_rho"] = 2.0 ** ((np.arange(len(old)) + salt) % 3 - 1)          # 0.5, 1, 2: exact divisors
    ok["rho_nr"], ok["s_rho_nr"], ok["m_num"] = ok["rho"], ok["s_rho"], 3
    ok["p_inx"] = ok["c_p"][:, 1].astype(np.int32) * W_B + ok["c_p"][:, 0].astype(np.int32)
    ok["p_m_0"], ok["m_m0"], ok["n_m0"] = ok["p_m"], ok["m_m"], ok["n_m"]
    for f in ("m_id", "m_id_f", "m_id_kf", "p_id", "n_id", "net_id", "stereo_m_id"):
        ok[f] = -1
    expect = np.array([o["expect"] for o in old])
    fi = np.zeros(len(old))
    for i, o in enumerate(old):
        if o["expect"] >= 0:
            t = o["expect"]
            fi[i] = (o["px"] - new[t]["x"]) * float(nk["u_m"][t, 0]) + (o["py"] - new[t]["y"]) * float(nk["u_m"][t, 1])
    assert len(ok) <= CAP_B and len(ok) > 513
    return dict(new=nk, new_mask=new_mask, old=ok, old_mask=np.full((H_B, W_B), -1, np.int32), cls=np.array([o["cls"] for o in old]),
                expect=expect, fi=fi, carry=(c0, c0 + CARRY_LEN - 1))


CLASSES_B = ("plain", "border", "test_f_k", "empty", "perp", "behind", "carry")


def make_reference_b(oracle):
    return oracle.Oracle("ref", oracle.euroc_params(W_B, H_B, max_points=CAP_B, ppx=PP_B[0], ppy=PP_B[1], zfx=ZF_B, zfy=ZF_B), nslots=2)


def load_b(orc, fam, n=None):
    """Family B into slots 0 (old, cut to n) and 1 (new) of a reference context, field built -> the old list as loaded."""
    kl, m = cut(fam["old"], fam["old_mask"], n)
    orc.set_keylines(0, kl, m, 0.0)
    orc.set_keylines(1, fam["new"], fam["new_mask"], 0.0)
    orc.build_field(1, MAX_R_B, 0.0)
    return kl


def huber_requests(orc, fam):
    """k_huber values for the reweighted pass: |r0[i]| and the doubles on either side of it, for a KeyLine with a positive, one with a
    negative and one with an inherited first-pass residual (inside the carry run, a block behind the KeyLine it inherits from).
    -> [(k_huber, index, kind)]"""
    load_b(orc, fam)
    r0 = evaluate(orc, 1, 0, np.zeros(6), GATE_B, 0, False, True)["r"]
    m = fam["expect"] >= 0
    pos = int(np.nonzero(m & (r0 > 0.2))[0][0])
    neg = int(np.nonzero(m & (r0 < -0.2))[0][0])
    c0, c1 = fam["carry"]
    inh = (c0 // BLOCK + 1) * BLOCK + 7
    assert c0 - 1 < BLOCK <= inh <= c1 and r0[inh] == r0[c0 - 1] != 0 and fam["expect"][inh] == -1
    out = []
    for i, kind in ((pos, "positive"), (neg, "negative"), (inh, "inherited")):
        k = abs(float(r0[i]))
        out += [(k, i, kind), (float(np.nextafter(k, 0.0)), i, kind), (float(np.nextafter(k, np.inf)), i, kind)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# The minimisers' jobs (family A)
# ---------------------------------------------------------------------------------------------------------------------------------
TOL_POSE_REL, TOL_POSE_ABS = 1e-7, 1e-9                # the bounds of tests/test_stage_b_gpu.py::test_minimizer_rv / test_minimizer_v
TOL_P, TOL_SCORE = 1e-6, 1e-8
TOL_V_REL, TOL_V_ABS, TOL_V_F, TOL_V_RVEL = 1e-9, 1e-12, 1e-11, 1e-8
MIN_CUTS = (None, 257)
RV_LISTS = (("runs", 0), ("head", 0), ("hole", 0), ("none", 0), ("gates", 1), ("gates", 5))       # (variant, FrameCount); MatchNumThresh = 2 throughout
V_LISTS = (("runs", 0), ("head", 0), ("hole", 0), ("none", 0), ("gates", 5), ("behind", 0))
V_REQUESTS = ((0, None), (3, None), (3, 1.5))          # (iter_max, min_mod; None = the old slot's retuned threshold as the pipeline passes it)
V_STARTS = ((0.0, 0.0, 0.0), (2e-3, 1e-3, -3e-4))
RV_ARGS = dict(match_thresh=MATCH_THRESH, iter_max=5, reweight_distance=K_HUBER, init_iter=2)
# seeds of the start poses: a job whose reference result moves by more than a tenth of the tolerance when the start moves by 1e-12 sits on an
# accept / reject knife edge of the LM loop (gain > 0) and takes the next seed.  Replaced: ("none", 257) takes seed 1 — with seed 0 the
# minimiser ends on a pose with ONE chance match, J^T J of rank 1, and its Cholesky inverse is 1e25 from one start and NaN from the other.
# test_tracker_crafted_cpu.py asserts that every job is stable with the seed recorded here.
RV_SEED = {("none", 0, 257): 1}


def rv_jobs():
    """[(variant, FrameCount, cut)] of Minimizer_RV, in an order in which neighbours differ in variant and length."""
    return [(v, fc, c) for k, c in enumerate(MIN_CUTS) for v, fc in (RV_LISTS[k:] + RV_LISTS[:k])]


def rv_start(fam, job, k):
    """Start pose of job k: the donor's nav pose plus a seeded 2e-4."""
    seed = RV_SEED.get(job, 0)
    nav = np.r_[np.array(fam["nav"].V[:]), np.array(fam["nav"].W[:])]
    return nav + np.random.RandomState(1000 + 10 * k + seed).normal(size=6) * 2e-4


def ref_minimizer_rv(fam, job, start, init_type):
    v, fc, c = job
    orc, so, sn = fam["orc"], fam["so"], fam["sn"]
    kl, m = cut(fam["variants"][v], fam["old_mask"], c)
    orc.set_keylines(so, kl, m, fam["old_retuned"])
    orc.set_framecount(sn, fc)
    ref = orc.minimizer_rv(sn, so, start[:3], start[3:], RV_ARGS["match_thresh"], RV_ARGS["iter_max"], init_type, RV_ARGS["reweight_distance"],
                           fam["gate"], GATES_MNT, RV_ARGS["init_iter"])
    ref["mid"] = orc.keylines(so)["m_id_f"].copy()
    ref["fc"] = orc.get_framecount(sn)
    return ref


def close_or_both_nonfinite(got, want, rel, abs_=0.0):
    """|got - want| <= rel * max|want| + abs_ on the finite entries of `want`; where `want` is not finite, `got` must not be either."""
    got, want = np.atleast_1d(np.asarray(got, F64)), np.atleast_1d(np.asarray(want, F64))
    fin = np.isfinite(want)
    if not np.array_equal(fin, np.isfinite(got)):
        return False
    if not fin.any():
        return True
    return bool(np.max(np.abs(got[fin] - want[fin])) <= rel * np.max(np.abs(want[fin])) + abs_)


def pose_close(got, want, rel, abs_):
    """np.allclose(got, want, rtol, atol) where `want` is finite; non-finite entries must be non-finite on both sides."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    fin = np.isfinite(want)
    return bool(np.array_equal(fin, np.isfinite(got)) and np.all(np.abs(got[fin] - want[fin]) <= abs_ + rel * np.abs(want[fin])))


def rv_agree(got, ref, scale=1.0):
    """The bounds of test_minimizer_rv (scale = 0.1: the stability screen) on dict(V, W, RVel, RW0, F) -> list of what differs."""
    bad = []
    for k in ("V", "W"):
        if not pose_close(got[k], ref[k], TOL_POSE_REL * scale, TOL_POSE_ABS * scale):
            bad.append(f"{k} {got[k]} vs {ref[k]}")
    for k in ("RVel", "RW0"):
        if not close_or_both_nonfinite(got[k], ref[k], TOL_P * scale):
            bad.append(f"{k} {np.ravel(got[k])} vs {np.ravel(ref[k])}")
    if not close_or_both_nonfinite(got["F"], ref["F"], TOL_SCORE * scale):
        bad.append(f"F {got['F']} vs {ref['F']}")
    return bad


def v_jobs():
    return [(v, fc, c) for k, c in enumerate(MIN_CUTS) for v, fc in (V_LISTS[k:] + V_LISTS[:k])]


def ref_minimizer_v(fam, job, V0, iter_max, min_mod):
    v, fc, c = job
    orc, so, sn = fam["orc"], fam["so"], fam["sn"]
    kl, m = cut(fam["variants"][v], fam["old_mask"], c)
    orc.set_keylines(so, kl, m, fam["old_retuned"])
    orc.set_framecount(sn, fc)
    ref = orc.minimizer_v(sn, so, V0, MATCH_THRESH, iter_max, fam["gate"], GATES_MNT, K_HUBER, fam["old_retuned"] if min_mod is None else min_mod)
    ref["mid"] = orc.keylines(so)["m_id_f"].copy()
    return ref


def v_agree(got, ref, scale=1.0):
    bad = []
    if not pose_close(got["V"], ref["V"], TOL_V_REL * scale, TOL_V_ABS * scale):
        bad.append(f"V {got['V']} vs {ref['V']}")
    if not close_or_both_nonfinite(got["F"], ref["F"], TOL_V_F * scale):
        bad.append(f"F {got['F']} vs {ref['F']}")
    if not close_or_both_nonfinite(got["RVel"], ref["RVel"], TOL_V_RVEL * scale):
        bad.append(f"RVel {np.ravel(got['RVel'])} vs {np.ravel(ref['RVel'])}")
    return bad
