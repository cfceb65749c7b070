"""Crafted inputs for three kernels that feed the tracker and the mapper: edge_tracker::EstimateQuantile (edge_tracker.cpp:1148-1186;
k_quantile<1024> / k_quantile<256>), the tail of edge_finder::reEstimateThresh (edge_finder.cpp:373-405; k_retune and the last wave of
k_quantile) and edge_tracker::ExtRotVel (edge_tracker.cpp:1207-1301; k_ext_rotvel and the 6x6 solve of edgehip_ext_rot_vel).  Shared by
tests/test_stats_crafted_cpu.py (the reference alone: the inputs reach what they claim, the named defects are caught) and
tests/test_stats_crafted_gpu.py (the device against the reference).  This module imports no GPU code.  The oracle is the compiled reference
(oracle/_ref); the numpy restatements below exist to show, through their `defect=` argument, that the cases can tell a subtly wrong kernel from
a right one.

Lists are built per length (a "cut" L is a list of L KeyLines built for that length, not a prefix: a quantile list on its threshold is on it
for one length only).  Every list starts from base_list(): KeyLines on distinct pixels of a 160 x 120 image with consistent m_m / u_m / n_m.

Quantile (only s_rho is overwritten).  A `probe` list holds one value v at a chosen index and fillers of the last bin everywhere else: with
pct = 0 the first bin whose exclusive prefix exceeds 0 is bin(v) + 1, so the answer names the bin of v — and is 1e3 when the KeyLine at that
index is not read.  `edges` and `clamps` are probe lists; the index is the first or last KeyLine of a 4 * NT stride of either instantiation
(0, 1023, 1024, 4095, 4096, L - 1).  `threshold` lists put exactly floor(pct * L) (`balanced`) or one more (`tipped`) KeyLines below a gap
of empty bins, the KeyLines of the low group on the stride boundaries first: one KeyLine lost or one stale KeyLine read moves the answer across
the gap.  Stale s_rho behind a shorter list is what the previous, longer list of the same slot left there; every list here keeps most of
its KeyLines in the low bins, so a stale read tips a balanced list.

ExtRotVel (fields read: m_id, u_m, p_m, p_m_0, rho, s_rho).  See erv_list().
"""
import functools

import numpy as np

from oracle.oracle import KEYLINE_DTYPE

F32, F64 = np.float32, np.float64
INT_MIN = -2 ** 31
W, H = 160, 120
CAP = 8448                                             # admits the longest cut
ZFX, ZFY = 458.654, 457.296                            # the EuRoC focal lengths, unscaled: ExtRotVel reads no image
SMIN, SMAX = 1e-3, 20.0                                # RHO_MIN, RHO_MAX
Q_CUTS = (1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
Q_CUTS_256 = (1025, 1, 1024, 1023)                     # the 65-sequence context: both sides of k_quantile<256>'s stride, and 1
Q_NBINS = (1, 4, 5, 100, 255, 256)
Q_PCTS = (0.0, 0.5, 0.9, 1.0)
Q_TENS = (250, 1020, 1030, 4090, 4100, 8190)           # lengths for which 0.9 * L is an integer in double (asserted in test_stats_crafted_cpu.py)
E_CUTS = (513, 1, None, 256, 255, 257)                 # None = E_FULL; a short list follows a long one
E_FULL = 700
E_VELS = ((0.0, 0.0, 0.0), (1e-3, -4e-4, 3e-4), (2e-4, -1e-4, 5e-2))
LOC_UNC, HUB = 1.0, 2.0


def params(oracle_module, **over):
    """Parameters of the reference contexts (and, field for field, of the device's): 160 x 120, CAP KeyLines."""
    kw = dict(max_points=CAP, zfx=ZFX, zfy=ZFY)
    kw.update(over)
    return oracle_module.euroc_params(W, H, **kw)


def zfm():
    """cam_model::zfm: (zfx + zfy) / 2 in float (cam_model.h:57)."""
    return float((F32(ZFX) + F32(ZFY)) / F32(2))


@functools.lru_cache(maxsize=None)
def _base(n, seed):
    rs = np.random.RandomState(seed)
    pix = rs.permutation((W - 4) * (H - 4))[:n]
    x, y = 2 + pix % (W - 4), 2 + pix // (W - 4)
    kl = np.zeros(n, KEYLINE_DTYPE)
    kl["p_inx"] = y * W + x
    kl["c_p"] = np.stack([x, y], 1).astype(F32)
    kl["p_m"] = kl["c_p"] - np.array([F32(80), F32(60)])
    kl["p_m_0"] = kl["p_m"]
    ang, mod = rs.uniform(0, 2 * np.pi, n), rs.uniform(1.0, 5.0, n)
    mx, my = (mod * np.cos(ang)).astype(F32), (mod * np.sin(ang)).astype(F32)
    nn = np.sqrt(mx * mx + my * my)
    assert nn.dtype == F32
    kl["m_m"], kl["n_m"], kl["u_m"] = np.stack([mx, my], 1), nn, np.stack([mx / nn, my / nn], 1)
    kl["m_m0"], kl["n_m0"] = kl["m_m"], kl["n_m"]
    for f in ("rho", "rho_nr", "rho0"):
        kl[f] = 1.0
    for f in ("s_rho", "s_rho_nr", "s_rho0"):
        kl[f] = 20.0
    for f in ("m_id", "m_id_f", "m_id_kf", "p_id", "n_id", "net_id", "stereo_m_id"):
        kl[f] = -1
    return kl


def base_list(n, seed=3):
    return _base(n, seed).copy()


# ---------------------------------------------------------------------------------------------------------------------------------
# EstimateQuantile
# ---------------------------------------------------------------------------------------------------------------------------------
def cvttsd2si(t):
    """(int)double of an x86-64 build: truncation; INT_MIN for NaN and for everything outside the int range."""
    t = np.asarray(t, F64)
    with np.errstate(invalid="ignore"):
        ok = (t > -2147483649.0) & (t < 2147483648.0)
        return np.where(ok, np.trunc(np.where(ok, t, 0.0)), float(INT_MIN)).astype(np.int64)


def cvt_saturating(t):
    """The GPU's v_cvt_i32_f64: saturates, 0 for NaN."""
    t = np.asarray(t, F64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(t), 0.0, np.clip(np.trunc(np.where(np.isnan(t), 0.0, t)), INT_MIN, 2 ** 31 - 1)).astype(np.int64)


QUANTILE_DEFECTS = ("ge", "saturating", "clamp_order", "clamp_before_convert", "kn_minus_1")


def quantile_bins(s_rho, smin, smax, n, defect=None):
    """Histogram position of every KeyLine (edge_tracker.cpp:1162-1165)."""
    with np.errstate(all="ignore"):
        t = F64(n) * (np.asarray(s_rho, F64) - smin) / (smax - smin)
        if defect == "clamp_before_convert":                       # fmin(fmax(t, 0), n - 1), then the conversion
            t = np.fmin(np.fmax(t, 0.0), F64(n - 1))
    i = cvt_saturating(t) if defect == "saturating" else cvttsd2si(t)
    if defect == "clamp_order":                                    # i < 0 first, then i > n - 1: the same function for every n >= 1
        i = np.where(i < 0, 0, i)
        i = np.where(i > n - 1, n - 1, i)
    else:
        i = np.where(i > n - 1, n - 1, i)
        i = np.where(i < 0, 0, i)
    return i


def quantile_np(s_rho, smin=SMIN, smax=SMAX, pct=0.9, n=100, defect=None):
    """edge_tracker::EstimateQuantile restated.  defect: `ge` (>= for >), `saturating` (the GPU's own conversion), `clamp_order` (the two
    integer clamps swapped — equal to the reference for every n >= 1, see test_stats_crafted_cpu.py), `clamp_before_convert` (the clamps
    on the double, before the conversion), `kn_minus_1` (pct * (kn - 1))."""
    kn = len(s_rho)
    histo = np.bincount(quantile_bins(s_rho, smin, smax, n, defect), minlength=n) if kn else np.zeros(n, np.int64)
    lim = pct * ((kn - 1) if defect == "kn_minus_1" else kn)
    a = 0
    for i in range(n):
        if (a >= lim) if defect == "ge" else (a > lim):
            return F64(i) * (smax - smin) / F64(n) + smin
        a += int(histo[i])
    return 1e3


def bin_edge(i, n, smin=SMIN, smax=SMAX):
    """The reference's value for "first bin past the quantile is i" (edge_tracker.cpp:1176)."""
    return F64(i) * (smax - smin) / F64(n) + smin


def filler(n, smin=SMIN, smax=SMAX):
    """A value in the middle of the last bin (of the only bin for n = 1)."""
    return smin + (n - 0.5) * (smax - smin) / n


def edge_values(n, smin=SMIN, smax=SMAX):
    """[(name, value)]: the double smin + i (smax - smin) / n and its two neighbours for i = 0, 1, 2, n / 2, n - 1, n."""
    out = []
    for i in sorted({0, 1, 2, n // 2, n - 1, n} & set(range(n + 1))):
        v = smin + i * (smax - smin) / n
        out += [(f"edge {i}/{n} -", float(np.nextafter(v, -np.inf))), (f"edge {i}/{n}", float(v)), (f"edge {i}/{n} +", float(np.nextafter(v, np.inf)))]
    return out


CLAMP_VALUES = (("-0.0", -0.0), ("0.0", 0.0), ("just below smin", float(np.nextafter(SMIN, 0.0))), ("truncates to 0", SMIN - 0.1),
                ("bin -1", SMIN - 0.3), ("large negative", -1e12), ("smax", SMAX), ("above smax", float(np.nextafter(SMAX, np.inf))),
                ("2 smax", 2 * SMAX), ("4.3e8", 4.3e8), ("1e300", 1e300), ("+inf", np.inf), ("-inf", -np.inf), ("NaN", np.nan))


def decisive_indices(L):
    """First and last KeyLine of every 4 * NT stride of k_quantile<256> (1024) and k_quantile<1024> (4096) inside a list of L, and of the list."""
    c = {0, L - 1}
    for s in (1024, 4096):
        for k in range(s, L + 1, s):
            c |= {k - 1, k}
    return sorted(i for i in c if 0 <= i < L)


def probe_list(L, v, at, n=100):
    """s_rho of a list of L: the filler of the last bin of an n-bin histogram everywhere, v at index `at`."""
    s = np.full(L, filler(n))
    s[at] = v
    return s


def threshold_list(L, pct, tipped, n=100, lo_bin=10, hi_bin=60):
    """floor(pct L) KeyLines (`tipped`: one more) in bins 0 .. lo_bin, the rest in bins hi_bin .. n - 2, nothing between.  With the strict
    a > pct L the balanced list answers with a bin past hi_bin, the tipped one with bin lo_bin + 1 at the latest.  The low group takes the
    stride boundaries first.  -> (s_rho, number of KeyLines in the low group)."""
    low = int(np.floor(pct * L)) + (1 if tipped else 0)
    low = min(low, L)
    order = decisive_indices(L)
    taken = set(order)
    rest = [i for i in range(L) if i not in taken]
    idx = np.array(order + rest, np.int64)
    width = (SMAX - SMIN) / n
    s = np.empty(L)
    k = np.arange(L)
    lo_vals = SMIN + ((k % (lo_bin + 1)) + 0.5) * width          # bins 0 .. lo_bin, all of them populated when the group is large enough
    lo_vals[0] = SMIN + (lo_bin + 0.5) * width                   # (the first member sits in lo_bin itself)
    hi_vals = SMIN + (hi_bin + (k % (n - 1 - hi_bin)) + 0.5) * width
    s[idx[:low]] = lo_vals[:low]
    s[idx[low:]] = hi_vals[:L - low]
    return s, low


def pct_is_exact(pct, L):
    """pct * L, as the reference computes it in double, is an integer."""
    return float(pct * L) == float(np.floor(pct * L))


def quantile_cases(cuts=Q_CUTS, tens=Q_TENS):
    """[(name, s_rho)] in an order in which a short list follows a long one: per length (longest first, then alternating), the variants.
    Every length gets the threshold pairs for pct = 0.5 and 0.9, all_last, all_first and the +inf probe at its last index.  The other
    edge and clamp probes are dealt out over the lengths by a running counter: one placement (length, stride-boundary index) per probe (two for the
    first few: seven probes per length) — not every probe at every length.  `empty` follows the longest list."""
    probes = [(nm, v, 100) for nm, v in edge_values(100)] + [(nm, v, 100) for nm, v in CLAMP_VALUES]
    for n in Q_NBINS:
        if n != 100:
            probes += [(nm, v, n) for nm, v in edge_values(n)]
    desc = sorted(set(cuts) | set(tens), reverse=True)
    lengths = [desc[j // 2] if j % 2 == 0 else desc[-1 - j // 2] for j in range(len(desc))]                          # long, short, long, ...
    out, p = [], 0
    per = -(-len(probes) // len(lengths))
    for L in lengths:
        for pct in (0.5, 0.9):
            for tipped in (False, True):
                s, low = threshold_list(L, pct, tipped)
                out.append((f"threshold L={L} pct={pct} {'tipped' if tipped else 'balanced'} low={low}", s))
        out.append((f"all_last L={L}", np.full(L, filler(100))))
        out.append((f"all_first L={L}", np.full(L, SMIN + 0.25 * (SMAX - SMIN) / 256)))        # bin 0 for every nbins <= 256
        dec = decisive_indices(L)
        for j in range(per):
            nm, v, n = probes[p % len(probes)]
            at = dec[p % len(dec)]
            out.append((f"probe {nm} (nbins {n}) at {at} L={L}", probe_list(L, v, at, n)))
            p += 1
        out.append((f"probe +inf (nbins 100) at {L - 1}, every length, L={L}", probe_list(L, np.inf, L - 1)))      # INT_MIN -> bin 0, at every length
        if L == max(lengths):
            out.append(("empty", np.zeros(0)))
    return out


def quantile_keylines(s_rho):
    kl = base_list(len(s_rho))
    kl["s_rho"] = s_rho
    return kl


# ---------------------------------------------------------------------------------------------------------------------------------
# reEstimateThresh
# ---------------------------------------------------------------------------------------------------------------------------------
RT_W, RT_H = 192, 144
RETUNE_DEFECTS = ("bin0", "gt")


def cvttss2si(t):
    t = np.asarray(t, F32)
    with np.errstate(invalid="ignore"):
        ok = (t >= F32(-2147483648.0)) & (t < F32(2147483648.0))
        return np.where(ok, np.trunc(np.where(ok, t, F32(0))), float(INT_MIN)).astype(np.int64)


def modulus_histogram(n_m, n):
    """The histogram of reEstimateThresh (edge_finder.cpp:376-398) in float32 -> (histo[n], max_dog, min_dog)."""
    n_m = np.asarray(n_m, F32)
    mx, mn = n_m.max(), n_m.min()
    with np.errstate(all="ignore"):
        t = F32(n) * (mx - n_m) / (mx - mn)
    assert t.dtype == F32
    i = cvttss2si(t)
    i = np.where(i > n - 1, n - 1, i)
    i = np.where(i < 0, 0, i)
    return np.bincount(i, minlength=n), mx, mn


def retune_bins(histo, knum, defect=None):
    """The walk of edge_finder.cpp:400-401: for (a = 0; i < n && a < knum; i++, a += histo[i]) — bin 0 is never counted."""
    n, i, a = len(histo), 0, 0
    while i < n and ((a <= knum) if defect == "gt" else (a < knum)):
        if defect == "bin0":
            a += int(histo[i])
            i += 1
        else:
            i += 1
            if i < n:
                a += int(histo[i])
    return i


def retune_np(n_m, knum, n=100, defect=None):
    """reTunedThresh as a float32.  defect: `bin0` (bin 0 counted), `gt` (the walk goes on while a <= knum: > for >= against knum)."""
    histo, mx, mn = modulus_histogram(n_m, n)
    i = retune_bins(histo, knum, defect)
    r = mx - F32(i) * (mx - mn) / F32(n)
    assert r.dtype == F32
    return r


def retune_track_points(histo):
    """The TrackPoints values of the issue from a frame's histogram: 0, 1, the count of bins 1 .. i for an i in the middle of the walk, that
    count + 1, the total without bin 0, that total + 1."""
    c = np.cumsum(histo[1:])
    total = int(c[-1])
    i = int(np.searchsorted(c, total // 2)) + 1                   # some bin in the middle whose own count is not 0
    while histo[i] == 0:
        i += 1
    ci = int(c[i - 1])
    return [0, 1, ci, ci + 1, total, total + 1]


def retune_frames(n=3):
    """n pairs (frame 1, frame 2) of different small scenes (synth.rects_sequence, 192 x 144)."""
    from rebvo_amd import synth
    return [list(synth.rects_sequence(RT_W, RT_H, 2, seed=7 + 4 * s)) for s in range(n)]


RT_NBINS = (100, 256)                                  # QCutOffNumBins is reEstimateThresh's n too; 256: lane 63 of the search holds bins 252 .. 255


def retune_params(module, track_points, nbins=100, **over):
    """auto_gain = 0: the detector's threshold stays put, so a frame yields the same KeyLines whatever ran before it."""
    return module.euroc_params(RT_W, RT_H, track_points=int(track_points), qcut_nbins=int(nbins), auto_gain=0.0, **over)


# ---------------------------------------------------------------------------------------------------------------------------------
# ExtRotVel
# ---------------------------------------------------------------------------------------------------------------------------------
ERV_DEFECTS = ("m_id_gt0", "skip_last", "no_fabs", "early_promote", "weight_mul")
ERV_VARIANTS = ("plain", "promote", "signs", "loner_first", "loner_last", "loner_255", "loner_256", "none", "few1", "few3", "few5", "parallel",
                "pole", "rho_zero", "s_rho_inf", "s_rho_nan")
ERV_LONERS = ("loner_first", "loner_last", "loner_255", "loner_256")
ERV_FULL_RANK = ("plain", "promote", "signs") + ERV_LONERS


def _unit(kl, idx, mx, my):
    mx, my = np.broadcast_to(F32(mx), np.shape(idx)), np.broadcast_to(F32(my), np.shape(idx))
    nn = np.sqrt(mx * mx + my * my)
    kl["m_m"][idx], kl["n_m"][idx] = np.stack([mx, my], 1), nn
    kl["u_m"][idx] = np.stack([mx / nn, my / nn], 1)


def pole_rho(v2):
    """A double rho with 1 / rho + v2 == 0 exactly (+inf for v2 == 0)."""
    if v2 == 0:
        return np.inf
    lo = hi = -1.0 / v2
    cand = [lo]
    for _ in range(16):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        cand += [lo, hi]
    pole = [c for c in cand if 1.0 / c + v2 == 0]
    assert pole, v2
    return float(pole[0])


def loner_index(name, L):
    return {"loner_first": 0, "loner_last": L - 1, "loner_255": min(255, L - 1), "loner_256": min(256, L - 1)}[name]


def erv_list(name, L=None, vel=E_VELS[1], seed=11):
    """KeyLine list of L (None: E_FULL) KeyLines for ExtRotVel.

    plain      three KeyLines in four matched (m_id a non-negative number, 0 included), u_m of every direction, p_m within (+-150, +-110) with
               full mantissas, p_m_0 a pixel or two from p_m: |Y| < 1.5 < hub, weight 1 throughout
    promote    as plain with |p_m| up to (350, 300): -u_x q_x q_y and q_y q_y are products of floats that round in float before they are
               divided by the double zf (edge_tracker.cpp:1255-1257)
    signs      as plain; every fourth matched KeyLine has Y = +-2, +-10, +-1000 times hub (p_m_0 moved along u_m): weight |Y| / hub
    loner_*    every KeyLine lies on an image axis with its gradient along that axis (u = (+-1, 0), p_m = (x, 0) or u = (0, +-1), p_m = (0, y)):
               column 5 of Phi (-u_x q_y + u_y q_x) is exactly 0 in every row, and columns 0 .. 4 have rank 5.  ONE KeyLine, the loner, has
               u = (0, 1), p_m = (x, 0): the only row that constrains the rotation about the optical axis.  It sits at KeyLine 0 with m_id = 0,
               at the last KeyLine, at KeyLine 255 or 256 (the last and first thread of a block).  Without its row Wx has rank 5.
    none       no KeyLine matched
    few1/3/5   1, 3, 5 matched KeyLines (the first, the last and three between), the rest unmatched
    parallel   plain with every u_m = (3, 4) / 5: columns 0 and 1 proportional
    pole       plain; KeyLine L / 2 has 1 / rho + vel[2] == 0 exactly.  rho_zero, s_rho_inf, s_rho_nan: that KeyLine has rho = 0, s_rho = inf, NaN
    """
    L = E_FULL if L is None else L
    rs = np.random.RandomState(seed + 1000 * L)
    kl = base_list(L, seed=5)
    _unit(kl, np.arange(L), kl["m_m"][:, 0], kl["m_m"][:, 1])
    ext = (350.0, 300.0) if name == "promote" else (150.0, 110.0)
    kl["p_m"] = np.stack([rs.uniform(-ext[0], ext[0], L), rs.uniform(-ext[1], ext[1], L)], 1).astype(F32)
    kl["rho"] = rs.uniform(0.2, 3.0, L)
    kl["s_rho"] = rs.uniform(0.05, 2.0, L)
    matched = rs.uniform(size=L) < 0.75
    matched[[0, L - 1]] = True
    kl["m_id"] = np.where(matched, rs.randint(0, 4000, L), -1)
    kl["m_id"][0] = 0                                              # "matched with KeyLine 0" is a match
    if name in ERV_LONERS:
        on_x = np.arange(L) % 2 == 0
        sign = np.where(rs.uniform(size=L) < 0.5, -1.0, 1.0)
        _unit(kl, np.arange(L), np.where(on_x, sign, 0.0), np.where(on_x, 0.0, sign))
        t = rs.uniform(20.0, 150.0, L) * np.where(rs.uniform(size=L) < 0.5, -1.0, 1.0)
        kl["p_m"] = np.stack([np.where(on_x, t, 0.0), np.where(on_x, 0.0, t)], 1).astype(F32)
        i = loner_index(name, L)
        _unit(kl, np.array([i]), 0.0, 1.0)
        kl["p_m"][i] = (F32(97.3), F32(0.0))
        kl["m_id"][i] = 0 if i == 0 else 7
        kl["rho"][i], kl["s_rho"][i] = 1.25, 0.125
    if name == "parallel":
        _unit(kl, np.arange(L), 3.0, 4.0)
    d = rs.uniform(-1.0, 1.0, L)                                   # Y ~ d: the displacement since p_m_0 along u_m
    if name == "signs":
        k = np.nonzero(kl["m_id"] >= 0)[0][::4]
        d[k] = np.resize(np.array([2.0, -2.0, 10.0, -10.0, 1000.0, -1000.0]) * HUB, len(k))
    kl["p_m_0"] = (kl["p_m"].astype(F64) - d[:, None] * kl["u_m"].astype(F64)).astype(F32)
    if name == "none":
        kl["m_id"] = -1
    if name.startswith("few"):
        keep = np.unique(np.linspace(0, L - 1, int(name[3:])).astype(int))
        kl["m_id"] = -1
        kl["m_id"][keep] = np.arange(len(keep))
    mid = L // 2
    if name in ("pole", "rho_zero", "s_rho_inf", "s_rho_nan"):
        kl["m_id"][mid] = 3
    if name == "pole":
        kl["rho"][mid] = pole_rho(vel[2])
    if name == "rho_zero":
        kl["rho"][mid] = 0.0
    if name == "s_rho_inf":
        kl["s_rho"][mid] = np.inf
    if name == "s_rho_nan":
        kl["s_rho"][mid] = np.nan
    return kl


def erv_rows(kl, vel, zf, loc_unc=LOC_UNC, hub=HUB, defect=None):
    """Phi and Y of edge_tracker.cpp:1230-1274, one rounding per operation of the reference's (float products stay float until the
    reference promotes them).  defect: `m_id_gt0`, `skip_last`, `no_fabs`, `early_promote`, `weight_mul`."""
    m = kl["m_id"] > 0 if defect == "m_id_gt0" else kl["m_id"] >= 0
    if defect == "skip_last" and len(m):
        m = m.copy()
        m[-1] = False
    k = kl[m]
    v0, v1, v2 = (F64(v) for v in vel)
    T = F64 if defect == "early_promote" else F32
    ux, uy = k["u_m"][:, 0], k["u_m"][:, 1]
    uxd, uyd = ux.astype(F64), uy.astype(F64)
    qx, qy = k["p_m"][:, 0].astype(T), k["p_m"][:, 1].astype(T)
    uxT, uyT = ux.astype(T), uy.astype(T)
    p0x, p0y = k["p_m_0"][:, 0].astype(F64), k["p_m_0"][:, 1].astype(F64)
    with np.errstate(all="ignore"):
        rho_t = 1 / (1 / k["rho"] + v2)
        qt_x = (p0x + rho_t * (v0 * zf - v2 * p0x)).astype(T)
        qt_y = (p0y + rho_t * (v1 * zf - v2 * p0y)).astype(T)
        qxd, qyd = qx.astype(F64), qy.astype(F64)
        Phi = np.empty((len(k), 6))
        Phi[:, 0] = uxd * rho_t * zf
        Phi[:, 1] = uyd * rho_t * zf
        Phi[:, 2] = uxd * (-rho_t * qxd) + uyd * (-rho_t * qyd)
        Phi[:, 3] = ((-uxT) * qx * qy).astype(F64) / zf - uyd * (zf + (qy * qy).astype(F64) / zf)
        Phi[:, 4] = (uyT * qx * qy).astype(F64) / zf + uxd * (zf + (qx * qx).astype(F64) / zf)
        Phi[:, 5] = ((-uxT) * qy + uyT * qx).astype(F64)
        Y = (uxT * (qx - qt_x) + uyT * (qy - qt_y)).astype(F64)
        dqvel = (uxd * (v0 * zf - v2 * p0x) + uyd * (v1 * zf - v2 * p0y)).astype(F32).astype(F64)
        s_y = np.sqrt(k["s_rho"] * k["s_rho"] * dqvel * dqvel + loc_unc * loc_unc).astype(F32).astype(F64)
        big = (Y > hub) if defect == "no_fabs" else (np.abs(Y) > hub)
        wgt = np.where(big, (Y if defect == "no_fabs" else np.abs(Y)) / hub, 1.0)
        den = s_y / wgt if defect == "weight_mul" else s_y * wgt
        Phi /= den[:, None]
        Y = Y / den
    return Phi, Y


def toon_solve(JtJ, JtF):
    """X = SVD(JtJ).backsub(JtF), Rx = SVD(JtJ).get_pinv() with TooN's cut (singular values with s * 1e9 <= s_max are dropped) and the
    reference's ok = no NaN in Rx or X."""
    try:
        with np.errstate(all="ignore"):
            U, s, Vt = np.linalg.svd(JtJ)
            inv = np.where(s * 1e9 <= s.max(), 0.0, 1.0 / np.where(s == 0, 1.0, s))
            Rx = (Vt.T * inv) @ U.T
            X = Rx @ JtF
    except np.linalg.LinAlgError:
        X, Rx = np.full(6, np.nan), np.full((6, 6), np.nan)
    ok = not (np.isnan(Rx).any() or np.isnan(X).any())
    return X, Rx, ok


def ext_rot_vel_np(kl, vel, zf=None, loc_unc=LOC_UNC, hub=HUB, defect=None):
    Phi, Y = erv_rows(kl, vel, zfm() if zf is None else zf, loc_unc, hub, defect)
    with np.errstate(all="ignore"):
        Wx, JtF = Phi.T @ Phi, Phi.T @ Y
    X, Rx, ok = toon_solve(Wx, JtF)
    return dict(ok=ok, X=X, Wx=Wx, Rx=Rx)


def kept_condition(Wx):
    """s_max over the smallest singular value TooN keeps (s * 1e9 > s_max) of a finite Wx; 1 for Wx = 0 -> (cond, singular values)."""
    s = np.linalg.svd(Wx, compute_uv=False)
    if s.max() == 0:
        return 1.0, s
    return float(s.max() / s[s * 1e9 > s.max()].min()), s


def erv_bounds(ref, n_rows):
    """The tolerances of the comparison, from the reference alone -> (tol_Wx[6,6], tol_X, tol_Rx, cond).
    Wx: two summation orders over n_rows products differ by at most n_rows 2^-52 sum |a_i b_i| <= n_rows 2^-52 sqrt(Wx_ii Wx_jj)
    (Cauchy-Schwarz).  X, Rx: cond (n_rows 2^-52 + 1e-11) of the largest entry; 1e-11 is what tests/test_port_vs_ref_cpu.py allows
    between the Jacobi solve and LAPACK.  (NaN where the reference's Wx is not finite: nothing finite is left to bound.)"""
    Wx = ref["Wx"]
    eps = n_rows * 2.0 ** -52
    with np.errstate(all="ignore"):
        d = np.sqrt(np.abs(np.diag(Wx)))
        tol_w = eps * np.outer(d, d)
    if not np.isfinite(Wx).all():
        return tol_w, np.nan, np.nan, np.nan
    cond, _ = kept_condition(Wx)
    rel = cond * (eps + 1e-11)
    fx, fr = ref["X"][np.isfinite(ref["X"])], ref["Rx"][np.isfinite(ref["Rx"])]
    return tol_w, rel * (np.abs(fx).max() if len(fx) else 0.0), rel * (np.abs(fr).max() if len(fr) else 0.0), cond


def erv_agree(got, ref, n_rows):
    """THE comparison of the GPU test (and of the restatement, the port and every defect on the CPU) -> list of what differs.
    ok equal; Wx within erv_bounds wherever the reference's entry is finite (exactly 0 where the scale is 0), non-finite where the
    reference's is; X and Rx likewise."""
    bad = []
    if bool(got["ok"]) != bool(ref["ok"]):
        bad.append(f"ok {bool(got['ok'])} vs {bool(ref['ok'])}")
    tol_w, tol_x, tol_r, cond = erv_bounds(ref, n_rows)
    for name, g, r, tol in (("Wx", got["Wx"], ref["Wx"], tol_w), ("X", got["X"], ref["X"], tol_x), ("Rx", got["Rx"], ref["Rx"], tol_r)):
        g, r = np.asarray(g, F64), np.asarray(r, F64)
        fin = np.isfinite(r)
        if not np.array_equal(fin, np.isfinite(g)):
            bad.append(f"{name}: finite pattern differs ({np.isfinite(g).sum()} vs {fin.sum()} finite entries)")
            continue
        if not fin.any():
            continue
        t = np.broadcast_to(tol, r.shape)[fin]
        with np.errstate(all="ignore"):
            err = np.abs(g[fin] - r[fin])
            if not np.all(err <= t):                                 # (a NaN bound fails: a finite entry beside non-finite ones has no derived bound)
                w = np.argmax(np.where(t > 0, err / np.where(t > 0, t, 1), np.where(err > 0, np.inf, 0)))
                bad.append(f"{name}: |d| {err[w]:.3e} against a bound of {t[w]:.3e} (cond {cond:.2e}, {n_rows} rows)")
    return bad


def erv_jobs(nseq=3):
    """[(cut, [variant per sequence], [velocity per sequence])] in launch order: per cut the variants in groups of nseq.  The variant at
    position j of its group takes velocity (j + index of the cut) % 3: all three velocities in every launch, and over the six cuts every
    variant meets every velocity twice (108 lists: one velocity per (variant, cut), not the full crossing).  The (variant, velocity) pairs
    of a launch are then rotated together from launch to launch so that sequence 0 holds another variant every time."""
    out, k = [], 0
    names = list(ERV_VARIANTS)
    for ci, c in enumerate(E_CUTS):
        for g in range(0, len(names), nseq):
            grp = [(names[(g + j) % len(names)], E_VELS[(j + ci) % len(E_VELS)]) for j in range(nseq)]
            r = k % nseq
            grp = grp[r:] + grp[:r]
            out.append((c, [n for n, _ in grp], [v for _, v in grp]))
            k += 1
    return out
